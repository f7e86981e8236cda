// stream_set_plan.h -- the bookkeeping of a stream set (sr_stream_*, sr_bigram_stream_*; the definition is in include/srgpu.h) that
// needs no device: the slots and their ids, the resolution of a call's id list, the window checks of a push and the layout of the
// pinned block the stable and trim calls share.  Host code over plain integers and vectors, no HIP include:
// tests/cpp/stream_set_plan_driver.cpp compiles it with the host compiler alone.  Every function returns a code and an index; the
// caller (stream_api.cpp) words the message.
#pragma once
#include <cstddef>
#include <cstdint>
#include <vector>

namespace srplan {

// The slots of a stream set: slot i holds one open utterance, named by the id slot + max_streams * generation, and its frame count.
struct StreamSlots {
  uint32_t max_streams = 0;
  uint64_t max_frames = 0;
  std::vector<uint8_t> open;        // [max_streams]
  std::vector<uint32_t> id;         // [max_streams] id of the slot's current (or last) utterance
  std::vector<uint32_t> generation; // [max_streams] of the next utterance begun in the slot
  std::vector<uint64_t> frames;     // [max_streams] frames searched so far (of the window: less what sr_stream_trim dropped)
  StreamSlots() = default;
  StreamSlots(uint32_t n, uint64_t max_frames_)
      : max_streams(n), max_frames(max_frames_), open(n, 0), id(n, 0), generation(n, 0), frames(n, 0) {}
  // opens the first free slot for a fresh utterance: its slot (id[slot] is its id), or -1 when every slot is open.  The generation
  // wraps before the id leaves 32 bits.
  int64_t begin() {
    uint32_t slot = 0;
    while (slot < max_streams && open[slot]) slot++;
    if (slot == max_streams) return -1;
    uint32_t g = generation[slot];
    if ((uint64_t)slot + (uint64_t)max_streams * g > 0xFFFFFFFFull) g = 0;
    generation[slot] = g + 1;
    id[slot] = slot + max_streams * g;
    open[slot] = 1;
    frames[slot] = 0;  // the first push starts from the initial state
    return slot;
  }
  // the slot of an open utterance's id, or -1
  int64_t find(uint32_t i) const {
    const uint32_t slot = i % max_streams;
    return open[slot] && id[slot] == i ? (int64_t)slot : -1;
  }
};

// The ids of a call, entry by entry: slots[i] = the slot of ids[i], stored `stride` bytes behind slots[i - 1] (a caller with a record
// per entry points at the records' slot field and spares itself an array).  The first entry whose id is not open, or names a slot an
// earlier entry named, ends the resolution: `entry` is its index and `fault` says which; slots[0 .. entry) are set.  No fault:
// entry == n.
enum IdFault : int { kIdsGood = 0, kIdNotOpen = 1, kIdTwice = 2 };
struct IdResolution { uint32_t entry; IdFault fault; };
inline IdResolution resolve_ids(const StreamSlots& sl, uint32_t n, const uint32_t* ids, uint32_t* slots, size_t stride = sizeof(uint32_t)) {
  std::vector<uint8_t> seen(sl.max_streams, 0);
  for (uint32_t i = 0; i < n; i++) {
    const int64_t slot = sl.find(ids[i]);
    if (slot < 0) return {i, kIdNotOpen};
    if (seen[slot]) return {i, kIdTwice};
    seen[slot] = 1;
    *reinterpret_cast<uint32_t*>(reinterpret_cast<unsigned char*>(slots) + stride * i) = (uint32_t)slot;
  }
  return {n, kIdsGood};
}

// A push's window check for one utterance that has `have` rows (or frames) of which sr_stream_trim dropped `base`, and gains `add`:
// max_frames bounds the window (what was received since the last dropped frame), 2^32 - 1 the utterance.  The window is looked at
// first.  (base <= have <= 2^32 - 1 and have - base <= max_frames: what the earlier pushes' checks let in.)
enum WindowFault : int { kWindowGood = 0, kWindowOverMaxFrames = 1, kWindowOverUtterance = 2 };
inline WindowFault check_window(uint64_t max_frames, uint64_t base, uint64_t have, uint64_t add) {
  if (add > max_frames - (have - base)) return kWindowOverMaxFrames;
  if (add > 0xFFFFFFFFull - have) return kWindowOverUtterance;
  return kWindowGood;
}

// The pinned block of a stable or trim call over n utterances that have seen F frames between them: the jobs (in), the results, then
// the items, frame_bytes for every frame (an utterance gives at most one item per frame; its items start `frames of the utterances
// before it` into each item area).
struct BlockLayout { size_t res_at, items_at, need; };
inline BlockLayout block_layout(size_t job_bytes, size_t result_bytes, size_t frame_bytes, uint32_t n, uint64_t F) {
  BlockLayout b;
  b.res_at = job_bytes * n;
  b.items_at = b.res_at + result_bytes * n;
  b.need = b.items_at + frame_bytes * (size_t)F;
  return b;
}
// the size a block of `have` bytes grows to for `need` (geometrically: pinning costs milliseconds, the need grows with every push)
inline size_t block_grown(size_t need, size_t have) { return need <= have ? have : need > 2 * have ? need : 2 * have; }

}  // namespace srplan
