// fb_plan.h -- the host planning every forward-backward style pass over a corpus shares (srgpu_api.cpp): the launch groups of a
// chunk, the longest-first order inside a group with its per-frame alive count, the mixture lists of the item kernels, the trellis
// offsets and lists of an occupancy pass, and the segments of the adaptation statistics' fixed summation order.  Host code
// over plain arrays, no HIP include: tests/cpp/fb_plan_driver.cpp compiles it with the host compiler alone and
// tests/test_fb_plan_cpu.py restates it in Python.
//
// Launch groups.  A pass runs a chunk's utterances in groups of consecutive utterances whose workspace fits a budget together.  The
// workspace of utterances [u, v) is cost[v] - cost[u] bytes, for a prefix cost[U + 1] the pass chooses (linear_cost, or 8 bytes per
// trellis cell).  A group takes its first utterance whatever it costs -- the entry points reject an utterance that does not fit
// alone -- and then every next utterance of the chunk while the whole stays within the budget.  A trellis is sized from max_span()
// of the very groups the launches walk.
#pragma once
#include <algorithm>
#include <cstdint>
#include <utility>
#include <vector>

namespace srplan {

struct Chunk { uint32_t u0, u1; uint64_t f0, f1; };  // utterances [u0, u1), frames [f0, f1)
struct Group { uint32_t u0, u1; };                   // utterances [u0, u1), never empty

struct Groups {
  std::vector<std::vector<Group>> of_chunk;  // in corpus order
  // the largest off[u1] - off[u0] over the groups, for any prefix off[U + 1]: frame_off gives the frames, cost the bytes
  uint64_t max_span(const uint64_t* off) const {
    uint64_t mx = 0;
    for (const auto& gs : of_chunk)
      for (const Group& g : gs) mx = std::max(mx, off[g.u1] - off[g.u0]);
    return mx;
  }
  uint32_t max_utts() const {
    uint32_t mx = 0;
    for (const auto& gs : of_chunk)
      for (const Group& g : gs) mx = std::max(mx, g.u1 - g.u0);
    return mx;
  }
};

// the longest off[u + 1] - off[u] of a group's utterances (automaton or chain positions: sizes a launch's LDS), at least 1
inline uint32_t max_positions(const Group& g, const uint64_t* off) {
  uint32_t mx = 1;
  for (uint32_t u = g.u0; u < g.u1; u++) mx = std::max(mx, (uint32_t)(off[u + 1] - off[u]));
  return mx;
}

// The threads of a forward-backward launch over the aligner's automata (viterbi_fb.hip) whose longest automaton has max_positions
// positions: one wave while every position has a lane of its own, else four -- a barrier of one wave costs nothing, and at 65
// positions a second wave already pays for itself.  (The kernels stride positions over whatever block they get: the same bits.)
inline uint32_t fb_block_threads(uint32_t max_positions) { return max_positions <= 64 ? 64u : 256u; }
// ... and of a launch over the transcripts' chains (viterbi_mmi.hip) whose longest chain has max_positions positions: a wave up to 64,
// four up to 256, else the network kernels' eight.  (These kernels, too, stride positions over whatever block they get.)
inline uint32_t chain_block_threads(uint32_t max_positions) { return max_positions <= 64 ? 64u : (max_positions <= 256 ? 256u : 512u); }

// cost[u] = per_frame * frame_off[u] + u * per_utt
inline std::vector<uint64_t> linear_cost(const uint64_t* frame_off, uint32_t U, uint64_t per_frame, uint64_t per_utt = 0) {
  std::vector<uint64_t> cost(U + 1);
  for (uint32_t u = 0; u <= U; u++) cost[u] = per_frame * frame_off[u] + u * per_utt;
  return cost;
}

inline Groups launch_groups(const std::vector<Chunk>& chunks, const uint64_t* cost, uint64_t budget) {
  Groups out;
  out.of_chunk.resize(chunks.size());
  for (size_t i = 0; i < chunks.size(); i++)
    for (uint32_t u = chunks[i].u0; u < chunks[i].u1;) {
      uint32_t v = u + 1;
      while (v < chunks[i].u1 && cost[v + 1] - cost[u] <= budget) v++;
      out.of_chunk[i].push_back({u, v});
      u = v;
    }
  return out;
}

// The per-frame passes step a group's utterances together, longest first, so that those still running at frame t are a prefix.
struct StepOrder {
  std::vector<uint32_t> order;  // [U]: every group's range sorted by descending length (ties in corpus order)
  const uint64_t* frame_off = nullptr;

  StepOrder() = default;
  StepOrder(const Groups& groups, const uint64_t* frame_off_, uint32_t U) : order(U), frame_off(frame_off_) {
    for (uint32_t u = 0; u < U; u++) order[u] = u;
    for (const auto& gs : groups.of_chunk)
      for (const Group& g : gs)
        std::stable_sort(order.begin() + g.u0, order.begin() + g.u1, [&](uint32_t x, uint32_t y) { return len(x) > len(y); });
  }
  uint64_t len(uint32_t u) const { return frame_off[u + 1] - frame_off[u]; }
  uint32_t t_max(const Group& g) const { return (uint32_t)len(order[g.u0]); }  // frames of the group's longest utterance
  uint32_t alive(const Group& g, uint32_t t) const {                           // utterances of the group with more than t frames
    uint32_t n = 0;
    while (n < g.u1 - g.u0 && len(order[g.u0 + n]) > t) n++;
    return n;
  }
};

// The distinct mixtures (ascending) of sets of positions and the positions carrying each: set s owns mix[mix_off[s] ..
// mix_off[s + 1]), and mixture entry k the positions slot_pos[slot_beg[k] .. slot_beg[k + 1]) (ascending, counted inside its
// set).  slot_beg always ends with its closing entry.  Pos is the position type the item kernel reads.
template <class Pos>
struct MixLists {
  std::vector<uint32_t> mix_off{0}, slot_beg{0};
  std::vector<uint16_t> mix;
  std::vector<Pos> slot_pos;

  // appends the set of positions 0 .. N - 1, position i carrying mixture ids[i] & mask
  template <class Id>
  void add(const Id* ids, uint64_t N, uint32_t mask = 0xFFFFFFFFu) {
    ps_.clear();
    for (uint64_t i = 0; i < N; i++) ps_.push_back({(uint16_t)(ids[i] & mask), (Pos)i});
    std::sort(ps_.begin(), ps_.end());
    slot_beg.pop_back();
    for (size_t i = 0; i < ps_.size(); i++) {
      if (i == 0 || ps_[i].first != ps_[i - 1].first) {
        mix.push_back(ps_[i].first);
        slot_beg.push_back((uint32_t)slot_pos.size());
      }
      slot_pos.push_back(ps_[i].second);
    }
    slot_beg.push_back((uint32_t)slot_pos.size());
    mix_off.push_back((uint32_t)mix.size());
  }
  uint32_t n_mix(uint32_t set) const { return mix_off[set + 1] - mix_off[set]; }

 private:
  std::vector<std::pair<uint16_t, Pos>> ps_;
};

// What an occupancy pass over U utterances plans ahead of its launch groups.  Chains (chain_off[U + 1] non-null): utterance u owns
// the positions info[chain_off[u] .. chain_off[u + 1]) and, with `lists`, set u of the mixture lists.  The free network (chain_off
// null): every utterance has the P positions of `info` and the lists hold their one set.  A position's mixture is the low 16 bits of
// its info word.  tr_off[U + 1] = prefix sums of positions x frames; item_bound = the sum of frames x distinct mixtures (0 without
// lists), which the caller holds below 2^31.
template <class Pos>
struct OccPlan {
  std::vector<uint64_t> tr_off;
  MixLists<Pos> ml;
  uint64_t item_bound = 0;

  OccPlan(const uint64_t* frame_off, uint32_t U, const uint64_t* chain_off, const uint32_t* info, uint64_t P, bool lists) : tr_off(U + 1, 0) {
    if (!chain_off && lists) ml.add(info, P, 0xFFFFu);
    for (uint32_t u = 0; u < U; u++) {
      const uint64_t N = chain_off ? chain_off[u + 1] - chain_off[u] : P, T = frame_off[u + 1] - frame_off[u];
      tr_off[u + 1] = tr_off[u] + N * T;
      if (!lists) continue;
      if (chain_off) ml.add(info + chain_off[u], N, 0xFFFFu);
      item_bound += T * ml.n_mix(chain_off ? u : 0);
    }
  }
};

// Ranges cut into segments of at most L: range r = [bounds[r], bounds[r + 1]) (non-decreasing) owns segments [off[r], off[r + 1]),
// segment g the positions [begin[g], begin[g] + len[g]).  An empty range has no segment.
struct Segments {
  std::vector<uint32_t> begin, len, off;

  Segments(const uint32_t* bounds, uint32_t n_ranges, uint32_t L) : off((size_t)n_ranges + 1, 0) {
    for (uint32_t r = 0; r < n_ranges; r++) {
      for (uint32_t b = bounds[r]; b < bounds[r + 1]; b += L) {
        begin.push_back(b);
        len.push_back(std::min(L, bounds[r + 1] - b));
      }
      off[r + 1] = (uint32_t)begin.size();
    }
  }
};

}  // namespace srplan
