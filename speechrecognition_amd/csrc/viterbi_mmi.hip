// viterbi_mmi.hip -- the kernels of MMI training over the recognition network (viterbi_netfb.hip's network, scale kappa, penalties and
// start hypothesis): mixture occupancies of the free network (denominator) and of the network restricted to a transcript (numerator),
// and the extended Baum-Welch update.  Their items for the EM accumulation come from the item path (posterior_items.hip).
//
// Occupancy.  occ_t(k) = the posterior probability that frame t's emission is mixture k's = dF / d e(t, k).  A slot's gamma is that
// of its own state, except at position 1 of a word: a path that ENTERS there emits the word's first state (the reference's quirk).
// Position 1 therefore keeps only its in-word part (predecessors s and s - 1, emission of its own state), and its entry part
// (nf_entry(E_{t-1}) + kappa e(t, first), then beta_t(s)) is added to the gamma of the word's position 0, whose state IS the first
// state.  After that a mixture's occupancy is the sum over the slots that carry it, in slot order, and sums to 1 over a frame.
//
//   netocc_backward_kernel  netfb_backward_kernel with that split; needs the E_t netfb_forward_kernel keeps in NetFbArgs::ends
//   chain_forward_kernel    the network restricted to the transcript w_1 .. w_n: the chain of segments sil_0 w_1 sil_1 ... w_n sil_n,
//   chain_backward_kernel   each with the slots and in-word moves of its lexicon word.  The word end of a segment enters the next word
//                           segment, the silence segment after it and, from a silence segment, that segment again; so the entry sum
//                           of a segment has at most two terms of the previous row (ChainArgs::src) and no block-wide sum is needed.
//                           The start hypothesis sits at position 0 of sil_0; paths end in the word end of w_n or sil_n.
//   ebw_combine_kernel      one thread per (density, dimension): the EBW means and variances from numerator and denominator statistics
//
// One workgroup per utterance, two FP64 rows in LDS, the trellis at 8 B per (frame, position) -- alpha, replaced by the occupancy part
// of the position --, no atomics: two identical calls return identical bits.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "fb_plan.h"
#include "kernels.h"
#include "netfb_device.h"

namespace srgpu {

// The occupancy part slot s keeps at frame t.  f = its flags, f1 = those of slot s + 1 (read only at position 0 of a longer word),
// a_ts = alpha_t(s), ap0 / ap1 = alpha_{t-1}(s) / alpha_{t-1}(s - 1) (read only at position 1), b0 / b1 = beta_t(s) / beta_t(s + 1),
// Ep = the entry sum E_{t-1} of the slot's word, e = kappa e(t, state(s)), F = kappa F_u.
__device__ inline double occ_part(uint32_t f, uint32_t f1, double a_ts, double ap0, double ap1, double b0, double b1, double Ep, double e,
                                  double F, const NfCosts& c) {
  double g = 0.0;
  if (f & kSlotPos1) {
    const double l0 = (f & kSlotEnd) ? kInf : ap0 + nf_tdp_into(f, 0, c);
    const double x = nf_ladd(l0, ap1 + nf_tdp_into(f, 1, c)) + e + b0;
    if (x < kInf) g = exp(F - x);
    return g;
  }
  const double x = a_ts + b0;
  if (x < kInf) g = exp(F - x);
  if ((f & kSlotPos0) && !(f & kSlotEnd)) {  // the entries into position 1 emit this slot's state
    const double y = nf_entry(f1, Ep, c) + e + b1;
    if (y < kInf) g += exp(F - y);
  }
  return g;
}

// LDS: beta[2][P] f64, red[2][2 * kNetFbWaves] f64.  Runs after netfb_forward_kernel (a.ends set) on the same launch.
__global__ __launch_bounds__(kNetFbThreads) void netocc_backward_kernel(NetFbArgs a) {
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  const uint32_t u = a.utt_first + blockIdx.x, tid = threadIdx.x;
  const uint32_t P = a.net.n_slots;
  const uint64_t f0 = a.frame_off[u];
  const int T = (int)(a.frame_off[u + 1] - f0);
  if (T == 0) return;
  double* be = reinterpret_cast<double*>(smem);
  double* red = be + 2 * (size_t)P;
  double* tr = a.trellis + (f0 - a.group_f0) * P;
  const double* ends = a.ends + (f0 - a.group_f0);
  const double* row0 = a.scores + (f0 - a.frame_base) * a.ld;
  const uint32_t* info = a.net.slot_info;
  const NfCosts c = nf_costs(a);
  const double F = a.out_cost[u];  // kappa F_u
  const bool dead = !(F < kInf && F > -kInf);  // no complete path (or a -inf emission took F along): every occupancy is 0

  // beta_t is whole in b (after the frame's barrier): the occupancy parts over alpha_t in the trellis.  Row t - 1 still holds alpha.
  auto occupy = [&](int t, const double* b, const double* row) {
    double* r = tr + (size_t)t * P;
    const double* ap = r - P;
    const double Ep = t > 0 ? ends[t - 1] : ((info[0] & kSlotEnd) ? 0.0 : kInf);
    for (uint32_t s = tid; s < P; s += kNetFbThreads) {
      const uint32_t f = info[s];
      double g = 0.0;
      if (!dead) {
        const bool p1 = f & kSlotPos1, p0 = (f & kSlotPos0) && !(f & kSlotEnd);
        const double ap0 = !p1 ? kInf : (t > 0 ? ap[s] : kInf);  // (the start hypothesis sits at slot 0, never a position 1)
        const double ap1 = !p1 ? kInf : (t > 0 ? ap[s - 1] : (s == 1 ? 0.0 : kInf));
        g = occ_part(f, p0 ? info[s + 1] : 0u, r[s], ap0, ap1, b[s], p0 ? b[s + 1] : kInf, Ep, c.k * row[f & 0xFFFFu], F, c);
      }
      r[s] = g;
    }
  };
  // the slot's term of B_{t-1}: entry into it at frame t (penalty, the entry's emission at t, beta_t)
  auto entry_term = [&](uint32_t s, uint32_t f, double b, const double* row, Lse& entries) {
    if ((f & (kSlotPos0 | kSlotPos1)) && b < kInf) {
      const uint32_t first = (f & kSlotPos0) ? f : info[s - 1];
      entries.add(nf_entry(f, 0.0, c) + c.k * row[first & 0xFFFFu] + b);
    }
  };
  {  // frame T - 1: beta = 0 at the word ends
    double* cur = be + (size_t)((T - 1) & 1) * P;
    const double* row = row0 + (uint64_t)(T - 1) * a.ld;
    Lse entries;
    for (uint32_t s = tid; s < P; s += kNetFbThreads) {
      const uint32_t f = info[s];
      const double b = (f & kSlotEnd) ? 0.0 : kInf;
      cur[s] = b;
      entry_term(s, f, b, row, entries);
    }
    block_lse_store(entries, red + ((T - 1) & 1) * 2 * kNetFbWaves);
    __syncthreads();
    occupy(T - 1, cur, row);
  }
  for (int t = T - 2; t >= 0; t--) {
    const double* nxt = be + (size_t)((t + 1) & 1) * P;
    double* cur = be + (size_t)(t & 1) * P;
    const double* rn = row0 + (uint64_t)(t + 1) * a.ld;  // emissions of the successors
    const double* row = row0 + (uint64_t)t * a.ld;
    const double B = block_lse_read(red + ((t + 1) & 1) * 2 * kNetFbWaves, kNetFbWaves);
    Lse entries;
    for (uint32_t s = tid; s < P; s += kNetFbThreads) {
      const uint32_t f = info[s];
      double b;
      if (f & kSlotEnd) {
        b = B;
      } else {
        const uint32_t f1 = info[s + 1];  // (s is not its word's last position: s + 1 is in the word)
        const double x0 = nf_tdp_into(f, 0, c) + c.k * rn[f & 0xFFFFu] + nxt[s];
        const double x1 = nf_tdp_into(f1, 1, c) + c.k * rn[f1 & 0xFFFFu] + nxt[s + 1];
        double x2 = kInf;
        if (!(f1 & kSlotEnd)) {
          const uint32_t f2 = info[s + 2];
          x2 = nf_tdp_into(f2, 2, c) + c.k * rn[f2 & 0xFFFFu] + nxt[s + 2];
        }
        b = nf_ladd3(x0, x1, x2);
      }
      cur[s] = b;
      entry_term(s, f, b, row, entries);
    }
    block_lse_store(entries, red + (t & 1) * 2 * kNetFbWaves);
    __syncthreads();
    occupy(t, cur, row);  // (reads cur only; the next frame writes the other row, after its own reads of this one)
  }
}

hipError_t launch_netocc_backward(const NetFbArgs& a, hipStream_t stream) {
  if (a.n_utts == 0) return hipSuccess;
  const size_t smem = (size_t)a.net.n_slots * 2 * 8 + 2 * 2 * kNetFbWaves * 8;
  hipError_t e = hipFuncSetAttribute((const void*)netocc_backward_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)smem);
  if (e != hipSuccess) return e;
  hipLaunchKernelGGL(netocc_backward_kernel, dim3(a.n_utts), dim3(kNetFbThreads), smem, stream, a);
  return hipGetLastError();
}

// ---- the transcript's chain -------------------------------------------------------------------------------------------------
static constexpr uint32_t kNoLink = 0xFFFFu;

__device__ inline NfCosts chain_costs(const ChainArgs& a) {
  const double k = a.scale;
  return NfCosts{k * a.tdp_loop, k * a.tdp_forward, k * a.tdp_skip, k * a.word_penalty, k};
}
// the entry sum of a segment from a row of alpha (ChainArgs::src of one of its entry positions)
__device__ inline double chain_entry_sum(uint32_t link, const double* row) {
  const uint32_t s0 = link & 0xFFFFu, s1 = link >> 16;
  return nf_ladd(s0 != kNoLink ? row[s0] : kInf, s1 != kNoLink ? row[s1] : kInf);
}

// LDS: alpha[2][N] f64
__global__ __launch_bounds__(kNetFbThreads) void chain_forward_kernel(ChainArgs a) {
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  const uint32_t u = a.utt_first + blockIdx.x, tid = threadIdx.x, nt = blockDim.x;
  const uint64_t f0 = a.frame_off[u];
  const int T = (int)(a.frame_off[u + 1] - f0);
  const uint32_t N = (uint32_t)(a.chain_off[u + 1] - a.chain_off[u]);
  double* al = reinterpret_cast<double*>(smem);
  double* tr = a.trellis + (a.trellis_off[u] - a.trellis_off[a.utt_first]);  // [T][N]
  const double* row0 = a.scores + (f0 - a.frame_base) * a.ld;
  const uint32_t* info = a.info + a.chain_off[u];
  const uint32_t* src = a.src + a.chain_off[u];
  const NfCosts c = chain_costs(a);
  if (T == 0) {
    if (tid == 0) a.out_cost[u] = kInf;
    return;
  }
  // the virtual row before frame 0 (parity 1): the start hypothesis at position 0 of sil_0, cost 0
  for (uint32_t s = tid; s < N; s += nt) al[N + s] = s == 0 ? 0.0 : kInf;
  __syncthreads();
  for (int t = 0; t < T; t++) {
    const double* prev = al + (size_t)((t + 1) & 1) * N;
    double* cur = al + (size_t)(t & 1) * N;
    const double* row = row0 + (uint64_t)t * a.ld;
    for (uint32_t s = tid; s < N; s += nt) {
      const uint32_t f = info[s];
      const double e = c.k * row[f & 0xFFFFu];
      const double l0 = (f & kSlotEnd) ? kInf : prev[s] + nf_tdp_into(f, 0, c);
      double v;
      if (f & kSlotPos0) {
        v = nf_ladd(l0, nf_entry(f, chain_entry_sum(src[s], prev), c)) + e;
      } else if (f & kSlotPos1) {
        const double in = nf_ladd(l0, prev[s - 1] + nf_tdp_into(f, 1, c));
        const double first = c.k * row[info[s - 1] & 0xFFFFu];
        v = nf_ladd(in < kInf ? in + e : kInf, nf_entry(f, chain_entry_sum(src[s], prev), c) + first);
      } else {
        v = nf_ladd3(l0, prev[s - 1] + nf_tdp_into(f, 1, c), prev[s - 2] + nf_tdp_into(f, 2, c));
        v = v < kInf ? v + e : kInf;
      }
      cur[s] = v;
      tr[(size_t)t * N + s] = v;
    }
    __syncthreads();
  }
  if (tid == 0) {  // the word ends of sil_n and (n >= 1) w_n
    const double* last = al + (size_t)((T - 1) & 1) * N;
    a.out_cost[u] = nf_ladd(last[N - 1], N > a.sil_len ? last[N - 1 - a.sil_len] : kInf);  // kappa F_u (the host divides)
  }
}

// LDS: beta[2][N] f64.  Runs after chain_forward_kernel on the same launch (reads out_cost).
__global__ __launch_bounds__(kNetFbThreads) void chain_backward_kernel(ChainArgs a) {
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  const uint32_t u = a.utt_first + blockIdx.x, tid = threadIdx.x, nt = blockDim.x;
  const uint64_t f0 = a.frame_off[u];
  const int T = (int)(a.frame_off[u + 1] - f0);
  if (T == 0) return;
  const uint32_t N = (uint32_t)(a.chain_off[u + 1] - a.chain_off[u]);
  double* be = reinterpret_cast<double*>(smem);
  double* tr = a.trellis + (a.trellis_off[u] - a.trellis_off[a.utt_first]);
  const double* row0 = a.scores + (f0 - a.frame_base) * a.ld;
  const uint32_t* info = a.info + a.chain_off[u];
  const uint32_t* src = a.src + a.chain_off[u];
  const uint32_t* dst = a.dst + a.chain_off[u];
  const NfCosts c = chain_costs(a);
  const double F = a.out_cost[u];
  const bool dead = !(F < kInf && F > -kInf);

  auto occupy = [&](int t, const double* b, const double* row) {
    double* r = tr + (size_t)t * N;
    const double* ap = r - N;
    for (uint32_t s = tid; s < N; s += nt) {
      const uint32_t f = info[s];
      double g = 0.0;
      if (!dead) {
        const bool p1 = f & kSlotPos1, p0 = (f & kSlotPos0) && !(f & kSlotEnd);
        const double ap0 = !p1 ? kInf : (t > 0 ? ap[s] : kInf);
        const double ap1 = !p1 ? kInf : (t > 0 ? ap[s - 1] : (s == 1 ? 0.0 : kInf));
        double Ep = kInf;
        if (p0) {
          const uint32_t l = src[s], s0 = l & 0xFFFFu, s1 = l >> 16;
          if (t > 0) Ep = chain_entry_sum(l, ap);
          else if (s0 == 0 || s1 == 0) Ep = 0.0;  // (the virtual row: only position 0 holds a hypothesis)
        }
        g = occ_part(f, p0 ? info[s + 1] : 0u, r[s], ap0, ap1, b[s], p0 ? b[s + 1] : kInf, Ep, c.k * row[f & 0xFFFFu], F, c);
      }
      r[s] = g;
    }
  };
  {  // frame T - 1: beta = 0 at the word ends of sil_n and w_n
    double* cur = be + (size_t)((T - 1) & 1) * N;
    for (uint32_t s = tid; s < N; s += nt) cur[s] = (s == N - 1 || s + a.sil_len == N - 1) ? 0.0 : kInf;
    __syncthreads();
    occupy(T - 1, cur, row0 + (uint64_t)(T - 1) * a.ld);
  }
  for (int t = T - 2; t >= 0; t--) {
    const double* nxt = be + (size_t)((t + 1) & 1) * N;
    double* cur = be + (size_t)(t & 1) * N;
    const double* rn = row0 + (uint64_t)(t + 1) * a.ld;
    // the entries into the segment whose position 0 is d, at frame t + 1
    auto enter = [&](uint32_t d) -> double {
      if (d == kNoLink) return kInf;
      const uint32_t fd = info[d];
      const double em = c.k * rn[fd & 0xFFFFu];
      double x = nf_entry(fd, 0.0, c) + em + nxt[d];
      if (!(fd & kSlotEnd)) x = nf_ladd(x, nf_entry(info[d + 1], 0.0, c) + em + nxt[d + 1]);
      return x;
    };
    for (uint32_t s = tid; s < N; s += nt) {
      const uint32_t f = info[s];
      double b;
      if (f & kSlotEnd) {
        b = nf_ladd(enter(dst[s] & 0xFFFFu), enter(dst[s] >> 16));
      } else {
        const uint32_t f1 = info[s + 1];
        const double x0 = nf_tdp_into(f, 0, c) + c.k * rn[f & 0xFFFFu] + nxt[s];
        const double x1 = nf_tdp_into(f1, 1, c) + c.k * rn[f1 & 0xFFFFu] + nxt[s + 1];
        double x2 = kInf;
        if (!(f1 & kSlotEnd)) {
          const uint32_t f2 = info[s + 2];
          x2 = nf_tdp_into(f2, 2, c) + c.k * rn[f2 & 0xFFFFu] + nxt[s + 2];
        }
        b = nf_ladd3(x0, x1, x2);
      }
      cur[s] = b;
    }
    __syncthreads();
    occupy(t, cur, row0 + (uint64_t)t * a.ld);
  }
}

static_assert(kNetFbThreads == 512, "srplan::chain_block_threads' largest block is the kernels' launch bound");
static uint32_t chain_block(uint32_t max_positions) { return srplan::chain_block_threads(max_positions); }

hipError_t launch_chain_forward(const ChainArgs& a, hipStream_t stream) {
  if (a.n_utts == 0) return hipSuccess;
  const size_t smem = (size_t)a.max_positions * 2 * 8;
  hipError_t e = hipFuncSetAttribute((const void*)chain_forward_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)smem);
  if (e != hipSuccess) return e;
  hipLaunchKernelGGL(chain_forward_kernel, dim3(a.n_utts), dim3(chain_block(a.max_positions)), smem, stream, a);
  return hipGetLastError();
}

hipError_t launch_chain_backward(const ChainArgs& a, hipStream_t stream) {
  if (a.n_utts == 0) return hipSuccess;
  const size_t smem = (size_t)a.max_positions * 2 * 8;
  hipError_t e = hipFuncSetAttribute((const void*)chain_backward_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)smem);
  if (e != hipSuccess) return e;
  hipLaunchKernelGGL(chain_backward_kernel, dim3(a.n_utts), dim3(chain_block(a.max_positions)), smem, stream, a);
  return hipGetLastError();
}

// ---- extended Baum-Welch ----------------------------------------------------------------------------------------------------
// Density c, dimension d, with D the density's smoothing constant: mu' = (xn - xd + D mu) / (gn - gd + D),
// var' = (sn - sd + D (var + mu^2)) / (gn - gd + D) - mu'^2.  Every thread of a density finds the same D: max(E gd, d_min) doubled (at
// most 64 times) until no dimension's new variance lies below the floor; what still does is set to the floor.  No FMA, so that the
// update can be restated operation by operation on a host.
#pragma clang fp contract(off)
__global__ __launch_bounds__(256) void ebw_combine_kernel(EbwArgs a) {
  const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= a.n_dens * a.dim) return;
  const uint64_t c = i / a.dim;
  const uint32_t d = (uint32_t)(i % a.dim), D = a.dim;
  const uint64_t rm = a.dens_mean[c], rv = a.dens_var[c];
  double gn = a.num_mean_w[rm];
  const double gd = a.den_mean_w[rm];
  if (gn == 0.0 && gd == 0.0) {  // never seen: the density stays as it is
    a.means[i] = a.old_means[i];
    a.inv_vars[i] = a.old_inv_vars[i];
    a.vars[i] = 1.0 / a.old_inv_vars[i];
    return;
  }
  double ns = 1.0;  // I-smoothing scales the numerator's count and sums
  if (a.tau > 0.0 && gn > 0.0) {
    ns = (gn + a.tau) / gn;
    gn = gn * ns;
  }
  const double diff = gd - gn;
  double Dc = a.E * gd;
  const double d_min = 2.0 * (diff > 0.0 ? diff : 0.0) + 1e-10;
  if (!(Dc > d_min)) Dc = d_min;
  // dimension k at constant Dk -> (mu', var')
  auto update = [&](uint32_t k, double Dk, double* mu_new) -> double {
    const double mu = a.old_means[c * D + k], var = 1.0 / a.old_inv_vars[c * D + k];
    const double xn = a.num_mean_acc[rm * D + k] * ns, xd = a.den_mean_acc[rm * D + k];
    const double sn = (a.num_var_acc[rv * D + k] - 1e-4) * ns, sd = a.den_var_acc[rv * D + k] - 1e-4;
    const double den = (gn - gd) + Dk;
    const double m = ((xn - xd) + Dk * mu) / den;
    *mu_new = m;
    return ((sn - sd) + Dk * (var + mu * mu)) / den - m * m;
  };
  for (int it = 0; it < 64; it++) {
    bool ok = true;
    for (uint32_t k = 0; k < D && ok; k++) {
      double m;
      ok = update(k, Dc, &m) >= a.var_floor;
    }
    if (ok) break;
    Dc = Dc * 2.0;
  }
  double m;
  double v = update(d, Dc, &m);
  if (!(v >= a.var_floor)) v = a.var_floor;
  a.means[i] = m;
  a.vars[i] = v;
  a.inv_vars[i] = 1.0 / v;
}

hipError_t launch_ebw_combine(const EbwArgs& a, hipStream_t stream) {
  const uint64_t n = a.n_dens * a.dim;
  if (n == 0) return hipSuccess;
  hipLaunchKernelGGL(ebw_combine_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, stream, a);
  return hipGetLastError();
}

}  // namespace srgpu
