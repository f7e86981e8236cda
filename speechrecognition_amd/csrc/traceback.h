// traceback.h -- the end of Recognizer::recognizeSequence_pruned (sietill/Recognizer.cpp:222-231), shared by the three
// search kernels, the device re-walk (sr_traceback_corpus) and the host walk (sr_traceback_words):
//
//     t = T; while (t > 0) { if (traceback[t].word != silence) push(word); t = traceback[t].bkp; }  reverse
//
// In a traceback the reference (or one of the kernels here) wrote, bkp is the frame before the word started
// (`bkp = t - 1` of an earlier frame, Recognizer.cpp:140; 16-bit truncation keeps it below t), so t falls strictly and at
// most T words are pushed.  The walk does not take that on trust: an entry whose bkp is not below its frame, whose word is
// not a word of the lexicon, or a word list that outgrows its buffer ends the walk with kTbCorrupt, and the caller raises
// out_flags bit 2 -> SR_ECORRUPT.  (Round 2: a timing-probe build with the word-end reduction stubbed out left
// traceback entries unwritten; the unguarded walk followed the stale bytes, never reached t = 0 and wrote words past the
// end of out_words until it left the allocation -- the "Memory access fault" of gpurun_out/ab_fp2.log)
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "kernels.h"

namespace srgpu {

static constexpr uint32_t kFlagSlowPath = 1u;   // out_flags: the sequential boundary replay was taken (informational)
static constexpr uint32_t kFlagReplay = 2u;     // a fast kernel met a negative emission cost: the replay kernel (launch_decode) redoes the utterance
static constexpr uint32_t kFlagCorrupt = 4u;    // the traceback did not walk: no words are reported, the entry point returns SR_ECORRUPT
static constexpr uint32_t kTbCorrupt = 0xFFFFFFFFu;

// words[0 .. return) = the recognised words in time order; load_word(t) / load_bkp(t) read traceback[t], t = 1..T.
template <class LoadWord, class LoadBkp>
__host__ __device__ inline uint32_t walk_traceback(uint32_t T, uint32_t silence_word, uint32_t n_words, LoadWord load_word,
                                                   LoadBkp load_bkp, uint32_t* words, uint32_t capacity) {
  uint32_t n = 0, t = T;
  while (t > 0) {
    const uint32_t w = load_word(t);
    if (w >= n_words) return kTbCorrupt;
    if (w != silence_word) {
      if (n >= capacity) return kTbCorrupt;
      words[n++] = w;
    }
    const uint32_t b = load_bkp(t);
    if (b >= t) return kTbCorrupt;
    t = b;
  }
  for (uint32_t i = 0; i < n / 2; i++) { const uint32_t x = words[i]; words[i] = words[n - 1 - i]; words[n - 1 - i] = x; }
  return n;
}

// ---- the end of utterance u in the zerogram search kernels (every thread of the workgroup calls these) ----------------------------
// Traceback entries 1..T of a kernel that records the winning word-end SLOT (0xFFFF: no surviving word end -> word 0,
// Recognizer.cpp:118,191) become words through slot_word [n_slots]; a slot out of range raises kFlagCorrupt.  Ends behind a barrier.
template <int NT>
__device__ __forceinline__ void traceback_slots_to_words(const DecodeArgs& a, uint32_t u, uint64_t tb0, uint32_t T, const uint32_t* slot_word,
                                                         uint32_t n_slots) {
  bool bad = false;
  for (uint32_t t = 1 + threadIdx.x; t <= T; t += NT) {
    const uint32_t sl = __hip_atomic_load(&a.tb_word[tb0 + t], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    uint16_t w = 0;
    if (sl != 0xFFFFu) { if (sl < n_slots) w = (uint16_t)slot_word[sl]; else bad = true; }
    a.tb_word[tb0 + t] = w;
  }
  if (bad) atomicOr(&a.out_flags[u], kFlagCorrupt);
  __threadfence();
  __syncthreads();
}
// The guarded walk of the word entries 1..T by thread 0 (Recognizer.cpp:222-231): the words at out_words + f0, out_count[u];
// kFlagCorrupt where it does not walk, kFlagSlowPath from every thread that took the sequential boundary replay.
__device__ __forceinline__ void traceback_walk(const DecodeArgs& a, uint32_t u, uint64_t f0, uint64_t tb0, uint32_t T, bool slow_taken) {
  if (slow_taken) atomicOr(&a.out_flags[u], kFlagSlowPath);
  if (threadIdx.x == 0) {
    const uint32_t n = walk_traceback(
        T, a.net.silence_word, a.net.n_words,
        [&](uint32_t t) -> uint32_t { return __hip_atomic_load(&a.tb_word[tb0 + t], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); },
        [&](uint32_t t) -> uint32_t { return __hip_atomic_load(&a.tb_bkp[tb0 + t], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); },
        a.out_words + f0, T);
    if (n == kTbCorrupt) atomicOr(&a.out_flags[u], kFlagCorrupt);
    a.out_count[u] = n == kTbCorrupt ? 0u : n;
  }
}
// A fast kernel's premise (every emission cost >= 0) failed somewhere in the workgroup: flag the utterance kFlagReplay for the replay
// kernel and report no words.  (The kernel keeps the workgroup-uniform test and its `return`: folded into a helper that returns a flag,
// it changes the code around the walk.)
__device__ __forceinline__ void hand_off_to_replay(const DecodeArgs& a, uint32_t u) {
  if (threadIdx.x == 0) { atomicOr(&a.out_flags[u], kFlagReplay); a.out_count[u] = 0; }
}

}  // namespace srgpu
