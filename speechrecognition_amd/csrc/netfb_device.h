// netfb_device.h -- device helpers the forward-backward kernels over the recognition network share (viterbi_netfb.hip,
// viterbi_mmi.hip): log-semiring additions in FP64, the block-wide log-sum-exp and the network's penalties.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "dpp_util.h"
#include "kernels.h"

namespace srgpu {

static constexpr double kInf = __builtin_huge_val();
static constexpr int kNetFbThreads = 512;
static constexpr int kNetFbWaves = kNetFbThreads / 64;

// Non-finite terms, in every sum below and in smbr_device.h's: a NaN cost (a NaN emission) counts as +inf in whichever slot it stands,
// so that alpha and beta leave out the same paths; -inf is sticky (a -inf emission takes every path through it, and F_u, to -inf)
// and never meets exp(-inf + inf).  For finite and +inf terms nothing here changes a bit.
__device__ inline double nf_nan_inf(double x) { return x < kInf ? x : kInf; }

// -log(exp(-a) + exp(-b))
__device__ inline double nf_ladd(double a, double b) {
  a = nf_nan_inf(a);
  b = nf_nan_inf(b);
  const double m = a < b ? a : b, x = a < b ? b : a;
  if (!(x < kInf) || !(m > -kInf)) return m;
  return m - log1p(exp(m - x));
}
// -log(exp(-a) + exp(-b) + exp(-c))
__device__ inline double nf_ladd3(double a, double b, double c) {
  a = nf_nan_inf(a);
  b = nf_nan_inf(b);
  c = nf_nan_inf(c);
  double m, x, y;
  if (a <= b && a <= c) { m = a; x = b; y = c; }
  else if (b <= c) { m = b; x = a; y = c; }
  else { m = c; x = a; y = b; }
  if (!(m < kInf)) return kInf;
  if (!(m > -kInf)) return m;
  double s = 0.0;
  if (x < kInf) s += exp(m - x);
  if (y < kInf) s += exp(m - y);
  return s == 0.0 ? m : m - log1p(s);
}

// running log-sum-exp (m = smallest cost seen, s = sum exp(m - x)); empty = (inf, 0); a NaN term is dropped, a -inf term leaves
// (-inf, 1) whatever else is added
struct Lse {
  double m, s;
  __device__ Lse() : m(kInf), s(0.0) {}
  __device__ void add(double x) {
    if (!(x < kInf) || !(m > -kInf)) return;
    if (!(x > -kInf)) { m = x; s = 1.0; return; }
    if (x < m) { s = s * exp(x - m) + 1.0; m = x; }
    else s += exp(m - x);
  }
  __device__ void merge(double om, double os) {  // symmetric in the two operands
    if (!(om < kInf)) return;
    if (!(m < kInf)) { m = om; s = os; return; }
    const double n = m < om ? m : om;
    if (!(n > -kInf)) { m = n; s = 1.0; return; }
    s = s * exp(n - m) + os * exp(n - om);
    m = n;
  }
  __device__ double cost() const { return m < kInf ? m - log(s) : kInf; }
};

// The block-wide sum of every thread's Lse: wave butterfly, then lane 0 of each wave stores to red[2 * wave]; read back with
// block_lse_read after a barrier.
__device__ inline void block_lse_store(Lse v, double* red) {
#pragma unroll
  for (int k = 1; k < 64; k <<= 1) {
    const double om = shfl_xor_f64(v.m, k), os = shfl_xor_f64(v.s, k);
    v.merge(om, os);
  }
  if ((threadIdx.x & 63) == 0) {
    red[2 * (threadIdx.x >> 6)] = v.m;
    red[2 * (threadIdx.x >> 6) + 1] = v.s;
  }
}
__device__ inline double block_lse_read(const double* red, int n_waves) {
  Lse v;
  for (int w = 0; w < n_waves; w++) v.merge(red[2 * w], red[2 * w + 1]);
  return v.cost();
}

struct NfCosts {  // the launch's penalties, multiplied by kappa
  double tl, tf, ts, wp, k;
};
__device__ inline NfCosts nf_costs(const NetFbArgs& a) {
  const double k = a.scale;
  return NfCosts{k * a.net.tdp_loop, k * a.net.tdp_forward, k * a.net.tdp_skip, k * a.word_penalty, k};
}
// penalty of a jump of j positions INTO a slot with flags f (keyed on the destination's state; silence: always forward)
__device__ inline double nf_tdp_into(uint32_t f, int j, const NfCosts& c) {
  if (f & kSlotSilState) return c.tf;
  return j == 0 ? c.tl : (j == 1 ? c.tf : c.ts);
}
// entry into the slot (position 0 or 1 of its word) from the word-end sum E, before any emission
__device__ inline double nf_entry(uint32_t f, double E, const NfCosts& c) {
  const double wp = (f & kSlotSilWord) ? 0.0 : c.wp;
  const double t = (f & kSlotPos0) ? c.tf : ((f & kSlotFirstSil) ? c.tf : c.ts);  // tdp(first, init + 1)
  return E + wp + t;
}

}  // namespace srgpu
