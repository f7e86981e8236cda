// bigram_device.h -- device helpers the kernels over the bigram search network share (viterbi_bigram_fb.hip, viterbi_bigram_mmi.hip,
// viterbi_bigram_smbr.hip, viterbi_bigram_lattice.hip): the network's penalties in FP64 and the few one-liners on its tables.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "netfb_device.h"

namespace srgpu {

// tdp[isSilence][loop, forward, skip, exit] widened to FP64; s and j select by comparison, so the table stays in scalar registers
struct BgCosts { double t[2][4]; };
// times kappa: the forward-backward family (BgFbArgs, BgChainArgs)
__device__ inline BgCosts bg_costs(const float (&tdp)[2][4], double scale) {
  BgCosts c;
  for (int s = 0; s < 2; s++)
    for (int j = 0; j < 4; j++) c.t[s][j] = scale * (double)tdp[s][j];
  return c;
}
// without a scale: the lattice (BgLatArgs)
__device__ inline BgCosts bg_costs(const float (&tdp)[2][4]) {
  BgCosts c;
  for (int s = 0; s < 2; s++)
    for (int j = 0; j < 4; j++) c.t[s][j] = (double)tdp[s][j];
  return c;
}
template <int J>
__device__ inline double bgs_pen(const BgCosts& c, bool sil) { return sil ? c.t[1][J] : c.t[0][J]; }
// cost of a linear-domain sum x relative to the offset m
__device__ inline double bg_unscale(double m, double x) { return (m < kInf && x > 0.0) ? m - log(x) : kInf; }
// is the position of this pos_info word a silence state (of the silence word or of a copy)?
__device__ inline int bgc_sil(uint32_t info) { return (info >> 16) & 8u ? 1 : 0; }

}  // namespace srgpu
