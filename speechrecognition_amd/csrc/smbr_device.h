// smbr_device.h -- device helpers the sMBR kernels share (viterbi_smbr.hip, viterbi_bigram_smbr.hip): a log-semiring cost with the
// expected accuracy of the paths it sums beside it, in the linear domain.  The cost of every sum is bit for bit what netfb_device.h's
// nf_ladd / nf_ladd3 / Lse give for the same operands, non-finite ones included (a NaN cost counts as +inf, -inf is sticky; the accuracy
// beside a -inf cost means nothing, and the kernels return none for such an utterance): the accuracy rides on the exp values those
// take anyway.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "dpp_util.h"
#include "netfb_device.h"

namespace srgpu {

struct La {  // a log-semiring cost and the expected accuracy of the paths it sums; a is finite, and ignored where x = +inf
  double x, a;
};
__device__ inline La la_add(La p, La q) {
  p.x = nf_nan_inf(p.x);
  q.x = nf_nan_inf(q.x);
  const bool pm = !(q.x < p.x);
  const La m = pm ? p : q, o = pm ? q : p;
  if (!(o.x < kInf) || !(m.x > -kInf)) return m;
  const double w = exp(m.x - o.x);
  return La{m.x - log1p(w), (m.a + w * o.a) / (1.0 + w)};
}
__device__ inline La la_add3(La p, La q, La r) {
  p.x = nf_nan_inf(p.x);
  q.x = nf_nan_inf(q.x);
  r.x = nf_nan_inf(r.x);
  // (m, x, y) = (the smallest, the other two) as nf_ladd3 picks them, by selects on the scalars
  const bool pm = p.x <= q.x && p.x <= r.x, qm = !pm && q.x <= r.x, rm = !pm && !qm;
  const La m{pm ? p.x : (qm ? q.x : r.x), pm ? p.a : (qm ? q.a : r.a)};
  const La x{pm ? q.x : p.x, pm ? q.a : p.a}, y{rm ? q.x : r.x, rm ? q.a : r.a};
  if (!(m.x < kInf)) return La{kInf, 0.0};
  if (!(m.x > -kInf)) return m;
  double s = 0.0, sa = m.a;
  if (x.x < kInf) { const double w = exp(m.x - x.x); s += w; sa += w * x.a; }
  if (y.x < kInf) { const double w = exp(m.x - y.x); s += w; sa += w * y.a; }
  return s == 0.0 ? m : La{m.x - log1p(s), sa / (1.0 + s)};
}

// Lse with the accuracy-weighted sum sa = sum exp(m - x) a beside it
struct LseA {
  double m, s, sa;
  __device__ LseA() : m(kInf), s(0.0), sa(0.0) {}
  __device__ void add(double x, double a) {
    if (!(x < kInf) || !(m > -kInf)) return;
    if (!(x > -kInf)) { m = x; s = 1.0; sa = 0.0; return; }
    if (x < m) { const double r = exp(x - m); s = s * r + 1.0; sa = sa * r + a; m = x; }
    else { const double w = exp(m - x); s += w; sa += w * a; }
  }
  __device__ void merge(double om, double os, double osa) {  // symmetric in the two operands
    if (!(om < kInf)) return;
    if (!(m < kInf)) { m = om; s = os; sa = osa; return; }
    const double n = m < om ? m : om;
    if (!(n > -kInf)) { m = n; s = 1.0; sa = 0.0; return; }
    const double r = exp(n - m), q = exp(n - om);
    s = s * r + os * q;
    sa = sa * r + osa * q;
    m = n;
  }
  __device__ La value() const { return m < kInf ? La{m - log(s), sa / s} : La{kInf, 0.0}; }
};

// a frame's accuracy term: does the position with slot_info / pos_info word f carry the reference mixture?
__device__ inline double hit(uint32_t f, uint32_t ref) { return (f & 0xFFFFu) == ref ? 1.0 : 0.0; }

// block_lse_store with the third component: lane 0 of each wave stores to red[3 * wave]
__device__ inline void block_lsea_store(LseA v, double* red) {
#pragma unroll
  for (int k = 1; k < 64; k <<= 1) {
    const double om = shfl_xor_f64(v.m, k), os = shfl_xor_f64(v.s, k), osa = shfl_xor_f64(v.sa, k);
    v.merge(om, os, osa);
  }
  if ((threadIdx.x & 63) == 0) {
    double* r = red + 3 * (threadIdx.x >> 6);
    r[0] = v.m; r[1] = v.s; r[2] = v.sa;
  }
}

}  // namespace srgpu
