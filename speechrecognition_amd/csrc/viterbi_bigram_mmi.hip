// viterbi_bigram_mmi.hip -- the kernels of MMI training over the bigram search network (viterbi_bigram_fb.hip's network, scale kappa,
// penalties and start): the network restricted to a transcript (numerator).  The free network (denominator) is
// viterbi_bigram_fb.hip's forward-backward unchanged.
//
// Occupancy.  occ_t(k) = the posterior probability that frame t's emission is mixture k's = dF / d e(t, k).  An entry in this network
// emits the mixture of the state it moves TO, so a position's gamma counts for its own mixture whole: the occupancy of a mixture is
// the sum of gamma over the positions that carry it, and the trellis stays at 8 B per (frame, position).
//
//   bgchain_forward_kernel   the network restricted to the transcript w_1 .. w_n: the chain of segments S w_1 c_1 .. w_n c_n, S the
//   bgchain_backward_kernel  silence word, c_i the silence copy after w_i, each with the states, penalties and in-word moves of its slot
//                            of the search net.  S is entered from the start's word end (cost 0, before frame 0) and from its own word
//                            end, w_i from the word ends of w_{i-1} and c_{i-1} (w_1: of the start and S) at kappa lm[w_i, w_{i-1}]
//                            (BgChainArgs::lmc; +inf: forbidden), c_i from the word end of w_i alone.  So the entry sum of a segment
//                            has at most two terms of the previous row (src), a word end at most two segments to enter (dst), and no
//                            block-wide sum is needed.  Paths end in the word end of w_n or c_n (n = 0: of S).  Everything in log
//                            space: no product, nothing underflows to "forbidden".
// The items come from the item path (posterior_items.hip) over 32-bit position lists (the free net has up to 2^31 positions), a mixture
// of more than 16 positions summed across the wave.
//
// One workgroup per utterance and two FP64 rows in LDS for the chain, one barrier per frame, gamma written over alpha, no atomics and
// a fixed summation order: two identical calls return identical bits.  +inf stays +inf, never NaN; a transcript without a path
// leaves F = +inf and an all-zero trellis.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "bigram_device.h"
#include "kernels.h"
#include "netfb_device.h"

namespace srgpu {

static constexpr uint32_t kNoLink = 0xFFFFu;

// LDS: alpha[2][N] f64
__global__ __launch_bounds__(kNetFbThreads) void bgchain_forward_kernel(BgChainArgs a) {
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  const uint32_t u = a.utt_first + blockIdx.x, tid = threadIdx.x, nt = blockDim.x;
  const uint64_t f0 = a.frame_off[u];
  const int T = (int)(a.frame_off[u + 1] - f0);
  const uint32_t N = (uint32_t)(a.chain_off[u + 1] - a.chain_off[u]);
  if (T == 0) {  // the start's word end is S': an empty transcript ends there
    if (tid == 0) a.out_cost[u] = N == a.sil_len ? 0.0 : kInf;
    return;
  }
  double* al = reinterpret_cast<double*>(smem);
  double* tr = a.trellis + (a.trellis_off[u] - a.trellis_off[a.utt_first]);  // [T][N]
  const double* row0 = a.scores + (f0 - a.frame_base) * a.ld;
  const uint32_t* info = a.info + a.chain_off[u];
  const uint32_t* src = a.src + a.chain_off[u];
  const double* lmc = a.lmc + a.chain_off[u];
  const BgCosts c = bg_costs(a.tdp, a.scale);
  const uint32_t end_S = a.sil_len - 1;
  for (int t = 0; t < T; t++) {
    const double* prev = al + (size_t)((t + 1) & 1) * N;  // (read only for t > 0)
    double* cur = al + (size_t)(t & 1) * N;
    const double* row = row0 + (uint64_t)t * a.ld;
    auto word_end = [&](uint32_t p) { return p == kNoLink ? kInf : prev[p] + c.t[bgc_sil(info[p])][3]; };
    for (uint32_t s = tid; s < N; s += nt) {
      const uint32_t f = info[s], fl = f >> 16;
      const int sl = bgc_sil(f);
      double ent = kInf;
      if (fl & 3u) {  // first or second state of its segment: the segment's entry
        const uint32_t l = src[s], s0 = l & 0xFFFFu, s1 = l >> 16;
        const double E = t ? nf_ladd(word_end(s0), word_end(s1)) : (s0 == end_S ? 0.0 : kInf);
        ent = E + lmc[s];
        if (fl & 2u) ent += c.t[sl][2];
      }
      double v = ent;
      if (t) {
        const double l1 = (fl & 1u) ? kInf : prev[s - 1] + c.t[sl][1];
        const double l2 = (fl & 3u) ? kInf : prev[s - 2] + c.t[sl][2];
        v = nf_ladd(nf_ladd3(prev[s] + c.t[sl][0], l1, l2), ent);
      }
      v = v < kInf ? v + a.scale * row[f & 0xFFFFu] : kInf;
      cur[s] = v;
      tr[(size_t)t * N + s] = v;
    }
    __syncthreads();
  }
  if (tid == 0) {  // the word ends of c_n (n = 0: S) and w_n
    const double* last = al + (size_t)((T - 1) & 1) * N;
    const double e0 = last[N - 1] + c.t[bgc_sil(info[N - 1])][3];
    const double e1 = N > a.sil_len ? last[N - 1 - a.sil_len] + c.t[bgc_sil(info[N - 1 - a.sil_len])][3] : kInf;
    a.out_cost[u] = nf_ladd(e0, e1);  // kappa F_u (the host divides)
  }
}

// LDS: x[2][N] f64, x_t(s) = kappa e_t(s) + beta_t(s).  Runs after bgchain_forward_kernel on the same launch (reads out_cost).
__global__ __launch_bounds__(kNetFbThreads) void bgchain_backward_kernel(BgChainArgs a) {
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  const uint32_t u = a.utt_first + blockIdx.x, tid = threadIdx.x, nt = blockDim.x;
  const uint64_t f0 = a.frame_off[u];
  const int T = (int)(a.frame_off[u + 1] - f0);
  if (T == 0) return;
  const uint32_t N = (uint32_t)(a.chain_off[u + 1] - a.chain_off[u]);
  double* xb = reinterpret_cast<double*>(smem);
  double* tr = a.trellis + (a.trellis_off[u] - a.trellis_off[a.utt_first]);
  const double* row0 = a.scores + (f0 - a.frame_base) * a.ld;
  const uint32_t* info = a.info + a.chain_off[u];
  const uint32_t* dst = a.dst + a.chain_off[u];
  const double* lmc = a.lmc + a.chain_off[u];
  const BgCosts c = bg_costs(a.tdp, a.scale);
  const double F = a.out_cost[u];
  const bool dead = !(F < kInf);  // no complete path: every occupancy is 0
  for (int t = T - 1; t >= 0; t--) {
    const double* xn = xb + (size_t)((t + 1) & 1) * N;  // (read only for t < T - 1)
    double* xc = xb + (size_t)(t & 1) * N;
    const double* row = row0 + (uint64_t)t * a.ld;
    // entering the segment whose first state is d at frame t + 1
    auto enter = [&](uint32_t d) -> double {
      if (d == kNoLink) return kInf;
      const uint32_t fd = info[d];
      const double x1 = ((fd >> 16) & 4u) ? kInf : c.t[bgc_sil(fd)][2] + xn[d + 1];
      return nf_ladd(xn[d], x1) + lmc[d];
    };
    for (uint32_t s = tid; s < N; s += nt) {
      const uint32_t f = info[s], fl = f >> 16;
      const int sl = bgc_sil(f);
      double b;
      if (t == T - 1) {
        b = (s == N - 1 || s + a.sil_len == N - 1) ? c.t[sl][3] : kInf;
      } else {
        const bool last = fl & 4u, last1 = last || ((info[s + 1] >> 16) & 4u);  // (s is not its segment's last: s + 1 is in it)
        const double s1 = last ? kInf : c.t[sl][1] + xn[s + 1];
        const double s2 = last1 ? kInf : c.t[sl][2] + xn[s + 2];
        b = nf_ladd3(c.t[sl][0] + xn[s], s1, s2);
        if (last) b = nf_ladd(b, c.t[sl][3] + nf_ladd(enter(dst[s] & 0xFFFFu), enter(dst[s] >> 16)));
      }
      double g = 0.0;
      if (!dead) {
        const double y = tr[(size_t)t * N + s] + b;
        if (y < kInf) g = exp(F - y);
      }
      tr[(size_t)t * N + s] = g;
      xc[s] = b < kInf ? a.scale * row[f & 0xFFFFu] + b : kInf;
    }
    __syncthreads();  // (the next frame reads xc and writes the other row, whose readers are past this barrier)
  }
}

// a wave for chains of up to 64 positions, four up to 256, else the network kernels' eight
static uint32_t bgchain_block(uint32_t max_positions) { return max_positions <= 64 ? 64u : (max_positions <= 256 ? 256u : (uint32_t)kNetFbThreads); }

hipError_t launch_bgchain_forward(const BgChainArgs& a, hipStream_t stream) {
  if (a.n_utts == 0) return hipSuccess;
  const size_t smem = (size_t)a.max_positions * 2 * 8;
  hipError_t e = hipFuncSetAttribute((const void*)bgchain_forward_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)smem);
  if (e != hipSuccess) return e;
  hipLaunchKernelGGL(bgchain_forward_kernel, dim3(a.n_utts), dim3(bgchain_block(a.max_positions)), smem, stream, a);
  return hipGetLastError();
}

hipError_t launch_bgchain_backward(const BgChainArgs& a, hipStream_t stream) {
  if (a.n_utts == 0) return hipSuccess;
  const size_t smem = (size_t)a.max_positions * 2 * 8;
  hipError_t e = hipFuncSetAttribute((const void*)bgchain_backward_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)smem);
  if (e != hipSuccess) return e;
  hipLaunchKernelGGL(bgchain_backward_kernel, dim3(a.n_utts), dim3(bgchain_block(a.max_positions)), smem, stream, a);
  return hipGetLastError();
}

}  // namespace srgpu
