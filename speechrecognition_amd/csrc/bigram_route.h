// bigram_route.h -- which instantiation of the bigram search (viterbi_bigram.hip) runs for a lexicon, decided in ONE place, and the LDS
// size formulas that decide it.  Host arithmetic only, nothing from HIP in here: tests/cpp/bigram_route_driver.cpp compiles this header
// with the host compiler alone and sweeps it (tests/test_bigram_route_cpu.py); the launchers switch on its result and decide nothing
// themselves; the kernels read their LDS offsets from the same formulas (constexpr functions are host and device functions to hipcc).
#pragma once
#include <stddef.h>
#include <stdint.h>
#include <stdio.h>

namespace srgpu {

constexpr int kBgThreads = 1024;
constexpr int kBgWaves = kBgThreads / 64;
constexpr int kBgStage = 256;  // word ends staged per pass of the recombination loop (more for big lexica, see `stage`)
constexpr size_t kBgLdsBytes = 160 * 1024;  // the LDS of a CU (gfx950)
constexpr uint32_t kBgMaxWords = 8 * kBgThreads;

// LDS image without the state hypotheses: entries, staging, scan scratch, the two active lists, the flags  (= 26 W + 3268)
constexpr size_t bigram_lds_small(uint32_t n_words) {
  return 2 * (size_t)n_words * 8 + (3 * kBgStage + kBgWaves + 1 + kBgWaves) * 4 + 2 * (size_t)n_words * 2 * 2 + 2 * (size_t)n_words + 64;
}
// dense layout: the image with the state hypotheses (score and back pointer of every position)
constexpr size_t bigram_lds_bytes(uint32_t n_words, uint32_t n_positions) { return (size_t)n_positions * 8 + bigram_lds_small(n_words); }

// global states: offset of step 3's prefix sums [2W] behind the small image (without the entries where they live in device memory)
constexpr size_t bigram_gs_pre_off(uint32_t n_words, bool entries_global) {
  return (bigram_lds_small(n_words) - (entries_global ? 2 * (size_t)n_words * 8 : 0) + 15u) & ~(size_t)15u;
}
constexpr size_t bigram_gs_lds(uint32_t n_words, bool entries_global) {
  return bigram_gs_pre_off(n_words, entries_global) + 2 * (size_t)n_words * 4;
}
constexpr bool bigram_gs_entries_global(uint32_t n_words) { return bigram_gs_lds(n_words, false) > kBgLdsBytes; }
// global-states workspace per workgroup, 32-bit words
constexpr uint64_t bigram_gs_ws_words(uint32_t n_words, uint32_t n_positions) {
  return 4ull * n_positions + (bigram_gs_entries_global(n_words) ? 4ull * n_words : 0ull);
}

// register layout: offset of the emission row behind the small image and the LM row bounds, and the whole image (the row: ld doubles
// in pieces of 1 KB)
constexpr size_t bigram_lds_row_off(uint32_t n_words) {
  return (((bigram_lds_small(n_words) + 15u) & ~(size_t)15u) + 2 * (size_t)n_words * 4 + 1023u) & ~(size_t)1023u;
}
constexpr size_t bigram_lds_regs(uint32_t n_words, uint32_t ld) {
  return bigram_lds_row_off(n_words) + (((size_t)ld * 8 + 1023u) & ~(size_t)1023u);
}

enum class BigramLayout { kRegisters, kLds, kGlobal, kNone };  // kNone: dense_states asked for an image the LDS cannot hold

// The kernel that runs: bigram_kernel<kw, 4, kw, npm> (registers), bigram_kernel<kw, kp, 0, 0> (lds),
// bigram_gs_kernel / bigram_stream_kernel<kw, gsm> (global), with `smem` bytes of dynamic LDS.
struct BigramRoute {
  BigramLayout layout;
  int kw, kp, npm, gsm;
  size_t smem;
};

// n_words W (1 .. kBgMaxWords), n_positions P2 = the states of the 2W slots (words and their silence copies: P2 >= 2W), the score
// table's row stride ld, the most states of a slot, the silence word's states, row4_mask (bit k = a word of four or more states among
// the words k * 1024 ..; 0 = unknown: every row) and the two flags of sr_bigram_params.  What cannot be is kNone.
//
// The dense LDS layout has no <4, 4> and no <8, .> instantiation: its image takes 8 P2 + 26 W + 3268 <= 163 840 bytes with P2 >= 2 W,
// so 42 W <= 160 572, W <= 3823 < 4097 (no KW 8); and W >= 2049 (KW 4) means P2 >= 4098 > 4 * 1024 (no KP 4 beside it).
constexpr BigramRoute bigram_route(uint32_t W, uint32_t P2, uint32_t ld, uint32_t max_slot_states, uint32_t silence_states,
                                   uint32_t row4_mask, bool dense_states, bool global_states) {
  const BigramRoute none{BigramLayout::kNone, 0, 0, 0, 0, 0};
  if (W == 0 || W > kBgMaxWords || P2 < 2 * (uint64_t)W || (dense_states && global_states)) return none;
  const uint32_t rows = (W + kBgThreads - 1) / kBgThreads;  // 1 .. 8
  if (!global_states) {
    if (!dense_states && max_slot_states <= 4 && silence_states == 1 && W <= 3 * (uint32_t)kBgThreads && bigram_lds_regs(W, ld) <= kBgLdsBytes) {
      // lane tid: words tid + k * 1024 and their silence copies; three states per word, four in the slot rows of the mask
      const uint32_t all = (1u << rows) - 1u;
      const uint32_t mask = max_slot_states <= 3 ? 0u : ((row4_mask & all) ? (row4_mask & all) : all);
      return BigramRoute{BigramLayout::kRegisters, (int)rows, 4, (int)mask, 0, bigram_lds_regs(W, ld)};
    }
    if (bigram_lds_bytes(W, P2) <= kBgLdsBytes) {
      const uint32_t pr = (P2 + kBgThreads - 1) / kBgThreads;
      const int kw = rows <= 1 ? 1 : rows <= 2 ? 2 : rows <= 4 ? 4 : 8, kp = pr <= 4 ? 4 : pr <= 12 ? 12 : pr <= 20 ? 20 : 0;
      if (kp == 0) return none;  // (8 P2 <= 163 840: never)
      return BigramRoute{BigramLayout::kLds, kw, kp, 0, 0, (bigram_lds_bytes(W, P2) + 15) & ~(size_t)15};
    }
    if (dense_states) return none;
  }
  // the entries move to device memory too (GSM 2) where entries, lists and flags alone crowd the LDS: W >= 4723, all of them KW 8
  const int kw = rows <= 1 ? 1 : rows <= 2 ? 2 : rows <= 4 ? 4 : 8;
  const bool eng = bigram_gs_entries_global(W);
  return BigramRoute{BigramLayout::kGlobal, kw, 0, 0, eng ? 2 : 1, bigram_gs_lds(W, eng)};
}

// "registers 3 rows4 0b100", "lds 2 x 12", "global 8 entries lds", "global 8 entries global", "none"
inline void bigram_route_text(const BigramRoute& r, char* out, size_t cap) {
  if (r.layout == BigramLayout::kRegisters) {
    char bits[33];
    int n = 0;
    for (int b = 31; b >= 0; b--)
      if (n || ((r.npm >> b) & 1) || b == 0) bits[n++] = ((r.npm >> b) & 1) ? '1' : '0';
    bits[n] = 0;
    snprintf(out, cap, "registers %d rows4 0b%s", r.kw, bits);
  } else if (r.layout == BigramLayout::kLds) {
    snprintf(out, cap, "lds %d x %d", r.kw, r.kp);
  } else if (r.layout == BigramLayout::kGlobal) {
    snprintf(out, cap, "global %d entries %s", r.kw, r.gsm == 2 ? "global" : "lds");
  } else {
    snprintf(out, cap, "none");
  }
}

}  // namespace srgpu
