// viterbi_netfb.hip -- forward-backward over the recognition network: the paths the zerogram decoder searches (every word may follow
// any word end; orc_decode_pruned, Recognizer.cpp:103-232), summed in the log semiring instead of minimised, with no beam and every
// cost multiplied by a scale kappa.  Slots = the lexicon's (word, position) pairs in DecodeNet order, read from its slot_info /
// slot_word / word_end_slot tables (viterbi_decode.hip, build_decode_net).
//
//   netfb_forward_kernel   alpha_t(s) = in-word log-add over s-j (j = 0, 1, 2; destination-keyed tdp) + e(t, state(s)), with the
//                          word-end sum E_{t-1} entering position 0 (+ wp + tdp(first, 1)) and position 1 (+ wp + tdp(first, 2) +
//                          e(t, first): the reference emits the FIRST state there); kappa F_u = E_{T-1}.  Before frame 0 the
//                          start hypothesis sits at slot 0 with cost 0.
//   netfb_backward_kernel  beta_t(s) the mirror image, one word-end value B_t = log-add over every entry; gamma_t(s) =
//                          exp(F - alpha_t(s) - beta_t(s)) overwrites alpha_t(s) in the trellis
//   netfb_words_kernel     p_t(w) = sum of gamma over w's slots in position order, [frames of the launch x W]
//   netfb_top_kernel       per frame the largest p_t(w) (ties: smaller word first), at most K of them, > 0 and >= floor
//   netfb_conf_kernel      per recognised word (the decoder's traceback): its frames bkp .. t-1 and the max of p_t(word) over them
//
// Log space in FP64 like viterbi_fb.hip rather than per-frame scaled probabilities: a scaled linear recursion still needs one exp
// per slot and frame (the emission), works only as far as the frame's range of costs stays inside the double exponent (kappa and
// negative emission costs move it), and +inf penalties stay exact here without special cases.
//
// One workgroup per utterance, slots strided over the threads, the two alpha (beta) rows in LDS (16 B per slot: 8192 slots = 128 KiB).
// The word-end sum is one block-wide log-sum-exp per frame: every thread folds its slots into (min m, sum exp(m - x)) in slot
// order, the waves combine by an xor butterfly (each combine is symmetric, so every lane gets the same bits) and every thread folds
// the per-wave results in wave order.  No atomics: two identical calls return identical bits.  +inf stays +inf, never NaN.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "dpp_util.h"
#include "kernels.h"
#include "netfb_device.h"

namespace srgpu {

// LDS: alpha[2][P] f64, red[2][2 * kNetFbWaves] f64
__global__ __launch_bounds__(kNetFbThreads) void netfb_forward_kernel(NetFbArgs a) {
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  const uint32_t u = a.utt_first + blockIdx.x, tid = threadIdx.x;
  const uint32_t P = a.net.n_slots;
  const uint64_t f0 = a.frame_off[u];
  const int T = (int)(a.frame_off[u + 1] - f0);
  double* al = reinterpret_cast<double*>(smem);
  double* red = al + 2 * (size_t)P;
  double* tr = a.trellis + (f0 - a.group_f0) * P;  // [T][P]
  const double* row0 = a.scores + (f0 - a.frame_base) * a.ld;
  const uint32_t* info = a.net.slot_info;
  const NfCosts c = nf_costs(a);
  if (T == 0) {
    if (tid == 0) a.out_cost[u] = kInf;
    return;
  }
  // the virtual row before frame 0 (parity 1): the start hypothesis at slot 0, cost 0
  for (uint32_t s = tid; s < P; s += kNetFbThreads) al[P + s] = s == 0 ? 0.0 : kInf;
  double E = (info[0] & kSlotEnd) ? 0.0 : kInf;
  __syncthreads();
  for (int t = 0; t < T; t++) {
    const double* prev = al + (size_t)((t + 1) & 1) * P;
    double* cur = al + (size_t)(t & 1) * P;
    const double* row = row0 + (uint64_t)t * a.ld;
    Lse ends;
    for (uint32_t s = tid; s < P; s += kNetFbThreads) {
      const uint32_t f = info[s];
      const double e = c.k * row[f & 0xFFFFu];
      const double l0 = (f & kSlotEnd) ? kInf : prev[s] + nf_tdp_into(f, 0, c);
      double v;
      if (f & kSlotPos0) {
        v = nf_ladd(l0, nf_entry(f, E, c)) + e;
      } else if (f & kSlotPos1) {
        const double in = nf_ladd(l0, prev[s - 1] + nf_tdp_into(f, 1, c));
        const double first = c.k * row[info[s - 1] & 0xFFFFu];
        v = nf_ladd(in < kInf ? in + e : kInf, nf_entry(f, E, c) + first);
      } else {
        v = nf_ladd3(l0, prev[s - 1] + nf_tdp_into(f, 1, c), prev[s - 2] + nf_tdp_into(f, 2, c));
        v = v < kInf ? v + e : kInf;
      }
      cur[s] = v;
      tr[(size_t)t * P + s] = v;
      if (f & kSlotEnd) ends.add(v);
    }
    block_lse_store(ends, red + (t & 1) * 2 * kNetFbWaves);
    __syncthreads();
    E = block_lse_read(red + (t & 1) * 2 * kNetFbWaves, kNetFbWaves);
    if (a.ends && tid == 0) a.ends[f0 - a.group_f0 + t] = E;  // (viterbi_mmi.hip splits gamma at position 1 with it)
  }
  if (tid == 0) a.out_cost[u] = E;  // kappa F_u (the host divides)
}

// LDS: beta[2][P] f64, red[2][2 * kNetFbWaves] f64.  Runs after netfb_forward_kernel on the same launch (reads out_cost).
__global__ __launch_bounds__(kNetFbThreads) void netfb_backward_kernel(NetFbArgs a) {
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  const uint32_t u = a.utt_first + blockIdx.x, tid = threadIdx.x;
  const uint32_t P = a.net.n_slots;
  const uint64_t f0 = a.frame_off[u];
  const int T = (int)(a.frame_off[u + 1] - f0);
  if (T == 0) return;
  double* be = reinterpret_cast<double*>(smem);
  double* red = be + 2 * (size_t)P;
  double* tr = a.trellis + (f0 - a.group_f0) * P;
  const double* row0 = a.scores + (f0 - a.frame_base) * a.ld;
  const uint32_t* info = a.net.slot_info;
  const NfCosts c = nf_costs(a);
  const double F = a.out_cost[u];  // kappa F_u
  const bool dead = !(F < kInf && F > -kInf);  // no complete path (or a -inf emission took F along): every posterior is 0

  // beta_t(s) of the thread's slots is final: gamma_t over alpha_t in the trellis, and the slot's term of B_{t-1} (entry into
  // it at frame t: penalty, the entry's emission at t, beta_t)
  auto finish = [&](int t, uint32_t s, uint32_t f, double b, const double* row, Lse& entries) {
    double* r = tr + (size_t)t * P;
    double g = 0.0;
    if (!dead) {
      const double x = r[s] + b;
      if (x < kInf) g = exp(F - x);
    }
    r[s] = g;
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
      finish(T - 1, s, f, b, row, entries);
    }
    block_lse_store(entries, red + ((T - 1) & 1) * 2 * kNetFbWaves);
    __syncthreads();
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
      finish(t, s, f, b, row, entries);
    }
    block_lse_store(entries, red + (t & 1) * 2 * kNetFbWaves);
    __syncthreads();
  }
}

static size_t netfb_smem(uint32_t P) { return (size_t)P * 2 * 8 + 2 * 2 * kNetFbWaves * 8; }
size_t netfb_max_slots() { return 8192; }

hipError_t launch_netfb_forward(const NetFbArgs& a, hipStream_t stream) {
  if (a.n_utts == 0) return hipSuccess;
  const size_t smem = netfb_smem(a.net.n_slots);
  hipError_t e = hipFuncSetAttribute((const void*)netfb_forward_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)smem);
  if (e != hipSuccess) return e;
  hipLaunchKernelGGL(netfb_forward_kernel, dim3(a.n_utts), dim3(kNetFbThreads), smem, stream, a);
  return hipGetLastError();
}

hipError_t launch_netfb_backward(const NetFbArgs& a, hipStream_t stream) {
  if (a.n_utts == 0) return hipSuccess;
  const size_t smem = netfb_smem(a.net.n_slots);
  hipError_t e = hipFuncSetAttribute((const void*)netfb_backward_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)smem);
  if (e != hipSuccess) return e;
  hipLaunchKernelGGL(netfb_backward_kernel, dim3(a.n_utts), dim3(kNetFbThreads), smem, stream, a);
  return hipGetLastError();
}

// one wave per frame of the launch, lanes over words: post[frame][w] = sum of gamma over w's slots in position order
__global__ __launch_bounds__(256) void netfb_words_kernel(NetFbArgs a, uint64_t n_frames) {
  const uint64_t f = (uint64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (f >= n_frames) return;
  const uint32_t W = a.net.n_words, P = a.net.n_slots;
  const double* g = a.trellis + f * P;
  double* out = a.post + f * W;
  for (uint32_t w = threadIdx.x & 63; w < W; w += 64) {
    const uint32_t e = a.net.word_end_slot[w], b = w ? a.net.word_end_slot[w - 1] + 1 : 0;
    double p = 0.0;
    for (uint32_t s = b; s <= e; s++) p += g[s];
    out[w] = p;
  }
}

hipError_t launch_netfb_words(const NetFbArgs& a, uint64_t n_frames, hipStream_t stream) {
  if (n_frames == 0) return hipSuccess;
  hipLaunchKernelGGL(netfb_words_kernel, dim3((unsigned)((n_frames + 3) / 4)), dim3(256), 0, stream, a, n_frames);
  return hipGetLastError();
}

// one wave per frame of the launch: K rounds of "the best word ranked after the previous pick" (p descending, then id ascending)
// among the words with p > 0 and p >= floor; written at the frame's corpus index
__global__ __launch_bounds__(256) void netfb_top_kernel(NetFbArgs a, uint64_t n_frames, uint32_t K, double floor, uint16_t* out_count,
                                                        uint32_t* out_word, double* out_weight) {
  const uint64_t f = (uint64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (f >= n_frames) return;
  const uint32_t lane = threadIdx.x & 63, W = a.net.n_words;
  const double* p = a.post + f * W;
  const uint64_t gf = a.group_f0 + f;
  double pw = kInf;
  uint32_t pid = 0, r = 0;
  for (; r < K; r++) {
    double bw = -1.0;
    uint32_t bid = 0xFFFFFFFFu;
    for (uint32_t w = lane; w < W; w += 64) {
      const double x = p[w];
      if (!(x > 0.0 && x >= floor)) continue;
      if (r > 0 && !(x < pw || (x == pw && w > pid))) continue;  // ranked at or before the previous pick
      if (x > bw || (x == bw && w < bid)) { bw = x; bid = w; }
    }
#pragma unroll
    for (int k = 1; k < 64; k <<= 1) {
      const double ow = shfl_xor_f64(bw, k);
      const uint32_t oid = (uint32_t)__shfl_xor((int)bid, k);
      if (ow > bw || (ow == bw && oid < bid)) { bw = ow; bid = oid; }
    }
    if (bid == 0xFFFFFFFFu) break;
    if (lane == 0) {
      out_word[gf * K + r] = bid;
      out_weight[gf * K + r] = bw;
    }
    pw = bw; pid = bid;
  }
  if (lane == 0) out_count[gf] = (uint16_t)r;
  for (uint32_t q = r + lane; q < K; q += 64) {
    out_word[gf * K + q] = 0;
    out_weight[gf * K + q] = 0.0;
  }
}

hipError_t launch_netfb_top(const NetFbArgs& a, uint64_t n_frames, uint32_t max_items, double floor, uint16_t* out_count,
                            uint32_t* out_word, double* out_weight, hipStream_t stream) {
  if (n_frames == 0) return hipSuccess;
  hipLaunchKernelGGL(netfb_top_kernel, dim3((unsigned)((n_frames + 3) / 4)), dim3(256), 0, stream, a, n_frames, max_items, floor,
                     out_count, out_word, out_weight);
  return hipGetLastError();
}

// one thread per utterance of the launch: the walk of the decoder's traceback (Recognizer.cpp:222-231, entries frame_off[u] + u + t)
// with the guards of traceback.h; recognised word k of utterance u (time order) at out_*[frame_off[u] + k]
__global__ __launch_bounds__(64) void netfb_conf_kernel(NetFbArgs a, const uint16_t* tb_word, const uint16_t* tb_bkp,
                                                        const uint32_t* out_count, double* out_conf, uint32_t* out_first,
                                                        uint32_t* out_last) {
  const uint32_t i = blockIdx.x * 64 + threadIdx.x;
  if (i >= a.n_utts) return;
  const uint32_t u = a.utt_first + i, W = a.net.n_words;
  const uint64_t f0 = a.frame_off[u], tb0 = f0 + u;
  const uint32_t T = (uint32_t)(a.frame_off[u + 1] - f0);
  const double* post = a.post + (f0 - a.group_f0) * W;
  uint32_t k = out_count[u], t = T;
  while (t > 0 && k > 0) {
    const uint32_t w = tb_word[tb0 + t], b = tb_bkp[tb0 + t];
    if (w >= W || b >= t) break;  // not a traceback: the decoder has flagged the utterance (SR_ECORRUPT)
    if (w != a.net.silence_word) {
      double mx = 0.0;
      for (uint32_t s = b; s < t; s++) mx = fmax(mx, post[(size_t)s * W + w]);
      k--;
      out_conf[f0 + k] = fmin(mx, 1.0);  // (a sum of posteriors may round above 1)
      out_first[f0 + k] = b;
      out_last[f0 + k] = t - 1;
    }
    t = b;
  }
}

hipError_t launch_netfb_conf(const NetFbArgs& a, const uint16_t* tb_word, const uint16_t* tb_bkp, const uint32_t* out_count,
                             double* out_conf, uint32_t* out_first, uint32_t* out_last, hipStream_t stream) {
  if (a.n_utts == 0) return hipSuccess;
  hipLaunchKernelGGL(netfb_conf_kernel, dim3((a.n_utts + 63) / 64), dim3(64), 0, stream, a, tb_word, tb_bkp, out_count, out_conf,
                     out_first, out_last);
  return hipGetLastError();
}

}  // namespace srgpu
