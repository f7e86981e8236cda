// viterbi_fb.hip -- forward-backward (Baum-Welch) over the forced aligner's automata: the same paths, 0-1-2 topology and
// source-keyed transition penalties as align_full_kernel (viterbi_align.hip), summed in the log semiring instead of minimised.
//
//   fb_forward_kernel    alpha_t(s) = e(t, ref[s]) + logadd_j (alpha_{t-1}(s-j) + tdp(ref[s-j], j)); F_u = alpha_{T-1}(N-1)
//   fb_backward_kernel   beta_t(s) = logadd_j (tdp(ref[s], j) + e(t+1, ref[s+j]) + beta_{t+1}(s+j)), and in the same frame loop
//                        gamma_t(s) = exp(F_u - alpha_t(s) - beta_t(s)) over alpha_t(s) in the trellis
// The posteriors of each frame's distinct mixtures, and the largest of them, come from the item path (posterior_items.hip).
//
// One workgroup per utterance (one wave when no automaton of the launch has more than 64 positions); positions strided over the
// threads, the two alpha (beta) rows in LDS, FP64 throughout.  logadd of up to three costs: m - log1p(sum exp(m - x)) over the
// two that are not the minimum m; +inf (a forbidden jump, an unreachable cell) stays +inf and never turns into NaN.
// Trellis workspace: 8 B per (frame, position) -- alpha, overwritten in place by gamma -- for the utterances of one launch.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "fb_plan.h"
#include "kernels.h"

namespace srgpu {

static constexpr double kInf = __builtin_huge_val();
static constexpr int kFbThreads = 256;

// keyed on the SOURCE position's state, any jump out of silence costs `forward` (align_full_kernel's tdp_score)
__device__ inline double fb_tdp(uint32_t from, int jump, uint32_t sil, double tl, double tf, double ts) {
  if (from == sil) return tf;
  return jump == 0 ? tl : (jump == 1 ? tf : ts);
}

// -log(exp(-a) + exp(-b) + exp(-c))
__device__ inline double logadd3(double a, double b, double c) {
  // A NaN cost (a NaN emission: outside the contract, but it must not leak) counts as +inf wherever it stands, so that alpha and beta
  // leave out the same paths: the ordering below would drop a NaN in `a` alone but the finite terms beside a NaN in `c`, and the
  // posteriors of a frame would then add up to more than 1.
  a = a < kInf ? a : kInf;
  b = b < kInf ? b : kInf;
  c = c < kInf ? c : kInf;
  double m, x, y;
  if (a <= b && a <= c) { m = a; x = b; y = c; }
  else if (b <= c) { m = b; x = a; y = c; }
  else { m = c; x = a; y = b; }
  if (!(m < kInf)) return kInf;
  if (!(m > -kInf)) return m;  // (a -inf emission, as little in the contract: it takes every path through it, and F_u, to -inf)
  double s = 0.0;
  if (x < kInf) s += exp(m - x);
  if (y < kInf) s += exp(m - y);
  return s == 0.0 ? m : m - log1p(s);
}

// positions of the 0-1-2 topology that lie on some complete path at frame t (align_full_kernel's window)
__device__ inline void fb_window(int t, int T, int N, int* lo, int* hi) {
  const int l = N - 1 - 2 * (T - 1 - t);
  *lo = l > 0 ? l : 0;
  *hi = (N - 1 < 2 * t) ? N - 1 : 2 * t;
}

// LDS layout: alpha[2][N] f64, ref[N] u16
__global__ __launch_bounds__(kFbThreads) void fb_forward_kernel(FbArgs a) {
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  const uint32_t u = a.utt_first + blockIdx.x, tid = threadIdx.x, nt = blockDim.x;
  const uint64_t f0 = a.frame_off[u];
  const int T = (int)(a.frame_off[u + 1] - f0);
  const int N = (int)(a.aut_off[u + 1] - a.aut_off[u]);
  const uint16_t* ref_g = a.automata + a.aut_off[u];
  double* al = reinterpret_cast<double*>(smem);
  uint16_t* ref = reinterpret_cast<uint16_t*>(al + 2 * (size_t)N);
  double* tr = a.trellis + (a.trellis_off[u] - a.trellis_off[a.utt_first]);  // [T][N]
  const double* row0 = a.scores + (f0 - a.frame_base) * a.ld;
  const uint32_t sil = a.silence_state;
  const double tl = a.tdp_loop, tf = a.tdp_forward, ts = a.tdp_skip;

  for (int s = tid; s < N; s += nt) {
    ref[s] = ref_g[s];
    al[s] = kInf;
    al[N + s] = kInf;
  }
  __syncthreads();
  if (tid == 0) {
    al[0] = row0[ref[0]];
    tr[0] = al[0];
  }
  __syncthreads();

  for (int t = 1; t < T; t++) {
    const double* prev = al + (size_t)((t - 1) & 1) * N;
    double* cur = al + (size_t)(t & 1) * N;
    const double* row = row0 + (uint64_t)t * a.ld;
    int lo, hi;
    fb_window(t, T, N, &lo, &hi);
    for (int s = lo + (int)tid; s <= hi; s += nt) {
      const double lp = prev[s] + fb_tdp(ref[s], 0, sil, tl, tf, ts);
      const double fw = s > 0 ? prev[s - 1] + fb_tdp(ref[s - 1], 1, sil, tl, tf, ts) : kInf;
      const double sk = s > 1 ? prev[s - 2] + fb_tdp(ref[s - 2], 2, sil, tl, tf, ts) : kInf;
      const double acc = logadd3(lp, fw, sk);
      const double v = acc < kInf ? row[ref[s]] + acc : kInf;
      cur[s] = v;
      tr[(size_t)t * N + s] = v;
    }
    __syncthreads();
  }
  if (tid == 0) a.out_cost[u] = al[(size_t)((T - 1) & 1) * N + (N - 1)];
}

// LDS layout: beta[2][N] f64, ref[N] u16.  Runs after fb_forward_kernel on the same launch range.
__global__ __launch_bounds__(kFbThreads) void fb_backward_kernel(FbArgs a) {
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  const uint32_t u = a.utt_first + blockIdx.x, tid = threadIdx.x, nt = blockDim.x;
  const uint64_t f0 = a.frame_off[u];
  const int T = (int)(a.frame_off[u + 1] - f0);
  const int N = (int)(a.aut_off[u + 1] - a.aut_off[u]);
  const uint16_t* ref_g = a.automata + a.aut_off[u];
  double* be = reinterpret_cast<double*>(smem);
  uint16_t* ref = reinterpret_cast<uint16_t*>(be + 2 * (size_t)N);
  double* tr = a.trellis + (a.trellis_off[u] - a.trellis_off[a.utt_first]);
  const double* row0 = a.scores + (f0 - a.frame_base) * a.ld;
  const uint32_t sil = a.silence_state;
  const double tl = a.tdp_loop, tf = a.tdp_forward, ts = a.tdp_skip;
  const double F = a.out_cost[u];
  const bool dead = !(F < kInf && F > -kInf);  // no complete path (or a NaN or -inf emission took F along): every posterior is 0

  for (int s = tid; s < N; s += nt) {
    ref[s] = ref_g[s];
    be[s] = kInf;
    be[N + s] = kInf;
  }
  __syncthreads();
  if (tid == 0) be[(size_t)((T - 1) & 1) * N + (N - 1)] = 0.0;
  __syncthreads();

  // gamma_t over the whole row (0 off the window): alpha_t(s) is read and replaced by the thread that owns position s
  auto gamma_row = [&](int t, const double* b) {
    int lo, hi;
    fb_window(t, T, N, &lo, &hi);
    double* r = tr + (size_t)t * N;
    for (int s = tid; s < N; s += nt) {
      double g = 0.0;
      if (!dead && s >= lo && s <= hi) {
        const double c = r[s] + b[s];
        if (c < kInf) g = exp(F - c);
      }
      r[s] = g;
    }
  };
  gamma_row(T - 1, be + (size_t)((T - 1) & 1) * N);

  for (int t = T - 2; t >= 0; t--) {
    const double* nxt = be + (size_t)((t + 1) & 1) * N;
    double* cur = be + (size_t)(t & 1) * N;
    const double* row = row0 + (uint64_t)(t + 1) * a.ld;
    int lo, hi;
    fb_window(t, T, N, &lo, &hi);
    for (int s = lo + (int)tid; s <= hi; s += nt) {
      const uint32_t r = ref[s];
      const double lp = fb_tdp(r, 0, sil, tl, tf, ts) + row[r] + nxt[s];
      const double fw = s + 1 < N ? fb_tdp(r, 1, sil, tl, tf, ts) + row[ref[s + 1]] + nxt[s + 1] : kInf;
      const double sk = s + 2 < N ? fb_tdp(r, 2, sil, tl, tf, ts) + row[ref[s + 2]] + nxt[s + 2] : kInf;
      cur[s] = logadd3(lp, fw, sk);
    }
    __syncthreads();
    gamma_row(t, cur);  // (reads cur only; the next frame writes the other row, after its own reads of this one)
  }
}

static_assert(kFbThreads == 256, "srplan::fb_block_threads' larger block is the kernels' launch bound");
static uint32_t fb_block(uint32_t max_positions) { return srplan::fb_block_threads(max_positions); }

hipError_t launch_fb_forward(const FbArgs& a, hipStream_t stream) {
  if (a.n_utts == 0) return hipSuccess;
  const size_t smem = (size_t)a.max_positions * (2 * 8 + 2) + 16;
  hipError_t e = hipFuncSetAttribute((const void*)fb_forward_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)smem);
  if (e != hipSuccess) return e;
  hipLaunchKernelGGL(fb_forward_kernel, dim3(a.n_utts), dim3(fb_block(a.max_positions)), smem, stream, a);
  return hipGetLastError();
}

hipError_t launch_fb_backward(const FbArgs& a, hipStream_t stream) {
  if (a.n_utts == 0) return hipSuccess;
  const size_t smem = (size_t)a.max_positions * (2 * 8 + 2) + 16;
  hipError_t e = hipFuncSetAttribute((const void*)fb_backward_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)smem);
  if (e != hipSuccess) return e;
  hipLaunchKernelGGL(fb_backward_kernel, dim3(a.n_utts), dim3(fb_block(a.max_positions)), smem, stream, a);
  return hipGetLastError();
}

}  // namespace srgpu
