// bigram_route_driver.cpp -- runs speechrecognition_amd/csrc/bigram_route.h (host code, no HIP) for tests/test_bigram_route_cpu.py.
//   bigram_route_driver sweep
//     every W = 1 .. 8192 x P2 at the break points (2W, 2W + 1, 4096 / 4097, 12288 / 12289, the largest P2 whose dense image fits the LDS
//     at this W and one more; those below 2W left out) x ld (8, 264, 2104, the largest row the register layout takes at this W and 8
//     more) x most states of a slot 1 .. 5 x silence states 1 .. 2 x row4_mask 0 .. 7 x flags (none, dense, global)
//     -> per distinct route, sorted: "<text> | <calls> <W min> <W max> <P2 min> <P2 max> <smem max>"
//   bigram_route_driver <cases.txt>
//     lines "W P2 ld max_slot_states silence_states row4_mask dense global" -> per line "<text> | <smem>"
#include <cstdio>
#include <cstring>
#include <fstream>
#include <map>
#include <string>
#include <vector>

#include "bigram_route.h"

using namespace srgpu;

struct Seen { unsigned long long calls = 0; uint32_t w0 = ~0u, w1 = 0, p0 = ~0u, p1 = 0; size_t smem = 0; };

static int sweep() {
  // (per route, keyed by its numbers: the text is made once at the end)
  std::vector<Seen> by_key(4 * 16 * 32 * 8 * 4);
  std::vector<BigramRoute> route_of(by_key.size());
  for (uint32_t W = 1; W <= kBgMaxWords; W++) {
    const size_t small = bigram_lds_small(W);
    const uint32_t fit = small <= kBgLdsBytes ? (uint32_t)((kBgLdsBytes - small) / 8) : 0;
    const uint32_t p2s[] = {2 * W, 2 * W + 1, 4096, 4097, 12288, 12289, fit, fit + 1};
    const size_t row_off = bigram_lds_row_off(W);
    const uint32_t ld_fit = row_off < kBgLdsBytes ? (uint32_t)((kBgLdsBytes - row_off) / 1024 * 128) : 0;
    const uint32_t lds[] = {8, 264, 2104, ld_fit, ld_fit + 8};
    for (uint32_t P2 : p2s) {
      if (P2 < 2 * W) continue;
      for (uint32_t ld : lds) {
        if (ld == 0) continue;
        for (uint32_t mss = 1; mss <= 5; mss++)
          for (uint32_t sil = 1; sil <= 2 && sil <= mss; sil++)
            for (uint32_t mask = 0; mask < 8; mask++)
              for (int flags = 0; flags < 3; flags++) {
                const BigramRoute r = bigram_route(W, P2, ld, mss, sil, mask, flags == 1, flags == 2);
                const size_t key = ((((size_t)r.layout * 16 + r.kw) * 32 + r.kp) * 8 + r.npm) * 4 + r.gsm;
                Seen& s = by_key[key];
                route_of[key] = r;
                s.calls++;
                if (W < s.w0) s.w0 = W;
                if (W > s.w1) s.w1 = W;
                if (P2 < s.p0) s.p0 = P2;
                if (P2 > s.p1) s.p1 = P2;
                if (r.smem > s.smem) s.smem = r.smem;
              }
      }
    }
  }
  std::map<std::string, Seen> seen;
  char text[64];
  for (size_t key = 0; key < by_key.size(); key++)
    if (by_key[key].calls) {
      bigram_route_text(route_of[key], text, sizeof text);
      seen[text] = by_key[key];
    }
  for (const auto& kv : seen)
    printf("%s | %llu %u %u %u %u %zu\n", kv.first.c_str(), kv.second.calls, kv.second.w0, kv.second.w1, kv.second.p0, kv.second.p1, kv.second.smem);
  return 0;
}

int main(int argc, char** argv) {
  if (argc != 2) { fprintf(stderr, "usage: bigram_route_driver sweep | <cases.txt>\n"); return 2; }
  if (!strcmp(argv[1], "sweep")) return sweep();
  std::ifstream in(argv[1]);
  if (!in) { fprintf(stderr, "cannot read %s\n", argv[1]); return 2; }
  uint32_t W, P2, ld, mss, sil, mask;
  int dense, global;
  char text[64];
  while (in >> W >> P2 >> ld >> mss >> sil >> mask >> dense >> global) {
    const BigramRoute r = bigram_route(W, P2, ld, mss, sil, mask, dense != 0, global != 0);
    bigram_route_text(r, text, sizeof text);
    printf("%s | %zu\n", text, r.smem);
  }
  return 0;
}
