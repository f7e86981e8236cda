// viterbi_fb.hip -- forward-backward (Baum-Welch) over the forced aligner's automata: the same paths, 0-1-2 topology and
// source-keyed transition penalties as align_full_kernel (viterbi_align.hip), summed in the log semiring instead of minimised.
//
//   fb_forward_kernel    alpha_t(s) = e(t, ref[s]) + logadd_j (alpha_{t-1}(s-j) + tdp(ref[s-j], j)); F_u = alpha_{T-1}(N-1)
//   fb_backward_kernel   beta_t(s) = logadd_j (tdp(ref[s], j) + e(t+1, ref[s+j]) + beta_{t+1}(s+j)), and in the same frame loop
//                        gamma_t(s) = exp(F_u - alpha_t(s) - beta_t(s)) over alpha_t(s) in the trellis
//   fb_items_kernel      per frame the posteriors of the automaton's distinct mixtures (positions of one mixture summed in
//                        position order), kept when > 0 and >= floor: a count pass, a device scan, a write pass
//   fb_top_kernel        per frame the largest items in AlignmentItem shape
//
// One workgroup per utterance (one wave when no automaton of the launch has more than 64 positions); positions strided over the
// threads, the two alpha (beta) rows in LDS, FP64 throughout.  logadd of up to three costs: m - log1p(sum exp(m - x)) over the
// two that are not the minimum m; +inf (a forbidden jump, an unreachable cell) stays +inf and never turns into NaN.
// Trellis workspace: 8 B per (frame, position) -- alpha, overwritten in place by gamma -- for the utterances of one launch.
#include <hip/hip_runtime.h>
#include <hipcub/hipcub.hpp>
#include <stdint.h>

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
  double m, x, y;
  if (a <= b && a <= c) { m = a; x = b; y = c; }
  else if (b <= c) { m = b; x = a; y = c; }
  else { m = c; x = a; y = b; }
  if (!(m < kInf)) return kInf;
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
  const bool dead = !(F < kInf);  // no complete path: every posterior is 0

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

static uint32_t fb_block(uint32_t max_positions) { return max_positions <= 64 ? 64u : (uint32_t)kFbThreads; }

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

// One workgroup per utterance, one thread per frame: the posterior of each distinct mixture of the automaton (ascending id) is the
// sum of gamma over its positions, in position order.  WRITE = false counts the items of each frame, WRITE = true stores them at
// *item_base + the exclusive scan of the counts.
template <bool WRITE>
__global__ __launch_bounds__(256) void fb_items_kernel(FbArgs a) {
  const uint32_t u = a.utt_first + blockIdx.x;
  const uint64_t f0 = a.frame_off[u];
  const int T = (int)(a.frame_off[u + 1] - f0);
  const int N = (int)(a.aut_off[u + 1] - a.aut_off[u]);
  const double* tr = a.trellis + (a.trellis_off[u] - a.trellis_off[a.utt_first]);
  const uint32_t j0 = a.mix_off[u], j1 = a.mix_off[u + 1];
  const double fl = a.floor;
  const uint32_t base = WRITE ? *a.item_base : 0u;
  for (int t = threadIdx.x; t < T; t += blockDim.x) {
    const double* g = tr + (size_t)t * N;
    const uint64_t gf = f0 + (uint64_t)t - a.group_f0;  // frame within the launch
    const uint32_t o = WRITE ? base + a.group_scan[gf] : 0u;
    uint32_t n = 0;
    for (uint32_t j = j0; j < j1; j++) {
      double p = 0.0;
      for (uint32_t i = a.slot_beg[j]; i < a.slot_beg[j + 1]; i++) p += g[a.slot_pos[i]];
      if (p > 0.0 && p >= fl) {
        if (WRITE) {
          a.item_frame[o + n] = (uint32_t)(f0 + t);
          a.item_mix[o + n] = a.mix[j];
          a.item_w[o + n] = p;
        }
        n++;
      }
    }
    if (WRITE) a.item_off[f0 + t] = o;
    else a.group_cnt[gf] = n;
  }
}

// *item_base += the launch's items; item_off[first frame after the launch] = *item_base (overwritten by the next launch with
// the same value, the corpus' total after the last one)
__global__ void fb_items_advance_kernel(FbArgs a, uint64_t n_frames) {
  const uint32_t total = *a.item_base + a.group_scan[n_frames - 1] + a.group_cnt[n_frames - 1];
  *a.item_base = total;
  a.item_off[a.group_f0 + n_frames] = total;
}

size_t fb_scan_temp_bytes(uint64_t n_frames) {
  size_t bytes = 0;
  (void)hipcub::DeviceScan::ExclusiveSum(nullptr, bytes, (const uint32_t*)nullptr, (uint32_t*)nullptr, (int)n_frames);
  return bytes;
}

hipError_t launch_fb_items(const FbArgs& args, uint64_t n_frames, void* scan_temp, size_t scan_temp_bytes, uint32_t* scan_out,
                           hipStream_t stream) {
  if (args.n_utts == 0 || n_frames == 0) return hipSuccess;
  FbArgs a = args;
  a.group_scan = scan_out;
  hipLaunchKernelGGL((fb_items_kernel<false>), dim3(a.n_utts), dim3(256), 0, stream, a);
  hipError_t e = hipGetLastError();
  if (e != hipSuccess) return e;
  e = hipcub::DeviceScan::ExclusiveSum(scan_temp, scan_temp_bytes, a.group_cnt, scan_out, (int)n_frames, stream);
  if (e != hipSuccess) return e;
  hipLaunchKernelGGL((fb_items_kernel<true>), dim3(a.n_utts), dim3(256), 0, stream, a);
  hipLaunchKernelGGL(fb_items_advance_kernel, dim3(1), dim3(1), 0, stream, a, n_frames);
  return hipGetLastError();
}

// one thread per frame: max_items rounds of "the best item ranked after the previous pick" (gamma descending, then id ascending)
__global__ __launch_bounds__(256) void fb_top_kernel(const uint32_t* item_off, const uint16_t* item_mix, const double* item_w,
                                                     uint64_t n_frames, uint32_t K, uint16_t* out_count, uint16_t* out_state,
                                                     double* out_weight) {
  const uint64_t f = (uint64_t)blockIdx.x * 256 + threadIdx.x;
  if (f >= n_frames) return;
  const uint32_t b = item_off[f], e = item_off[f + 1];
  double pw = kInf;
  uint32_t pid = 0;
  bool first = true;
  uint32_t r = 0;
  for (; r < K; r++) {
    double bw = -1.0;
    uint32_t bid = 0xFFFFFFFFu;
    for (uint32_t i = b; i < e; i++) {
      const double w = item_w[i];
      const uint32_t id = item_mix[i];
      if (!first && !(w < pw || (w == pw && id > pid))) continue;  // ranked at or before the previous pick
      if (w > bw || (w == bw && id < bid)) { bw = w; bid = id; }
    }
    if (bid == 0xFFFFFFFFu) break;
    out_state[f * K + r] = (uint16_t)bid;
    out_weight[f * K + r] = bw;
    pw = bw; pid = bid; first = false;
  }
  out_count[f] = (uint16_t)r;
  for (uint32_t q = r; q < K; q++) {
    out_state[f * K + q] = 0;
    out_weight[f * K + q] = 0.0;
  }
}

hipError_t launch_fb_top(const uint32_t* item_off, const uint16_t* item_mix, const double* item_w, uint64_t n_frames,
                         uint32_t max_items, uint16_t* out_count, uint16_t* out_state, double* out_weight, hipStream_t stream) {
  if (n_frames == 0) return hipSuccess;
  hipLaunchKernelGGL(fb_top_kernel, dim3((unsigned)((n_frames + 255) / 256)), dim3(256), 0, stream, item_off, item_mix, item_w, n_frames,
                     max_items, out_count, out_state, out_weight);
  return hipGetLastError();
}

}  // namespace srgpu
