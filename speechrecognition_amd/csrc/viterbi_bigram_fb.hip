// viterbi_bigram_fb.hip -- forward-backward over the bigram-LM search network: the paths the bigram decoder searches (viterbi_bigram.hip;
// Teaching::LinearSearch), summed in the log semiring instead of minimised, with no acoustic and no LM beam and every cost
// multiplied by a scale kappa.  Slots and positions are the search's own (build_bigram_net: words 0 .. W-1, then the silence copy
// h + W of every word h; positions = their states back to back, pos_info / pos_slot / slot_off).
//
// The network: before frame 1 one word end, the silence word at cost 0.  A word end of slot x has history x (a word), h (the copy
// h + W) or silence (the silence word); the cost of a history is the log-sum of its word ends.  This is the decoder's merge WITHOUT
// the positional cut of mergeSilenceToBigramNodes (LinearSearch.cc:378-395): every history is kept.  Word w != silence is entered from
// every history h at hist_h + lm[w, h] (NaN and +inf: forbidden), the copy h + W from the word end of word h alone, the silence word
// from its own word end.  An entry moves to the first state at no penalty or to the second at the skip penalty; a state moves to
// itself and the next two at tdp[isSilence][0..2]; the destination's mixture is emitted; a word end is the last state plus
// tdp[isSilence][3].
//
// What differs from viterbi_netfb.hip is the word entry: W x W terms per frame and utterance.  It is taken in the linear domain for
// all utterances of a launch group at the same frame index at once, as the FP64 matrix product [W x W] . [W x U]:
//
//   bgfb_table_kernel      Lk[w][h] = exp(-kappa lm[w, h]) (0 for NaN, +inf and the silence row) and its transpose, padded to Kp
//   bgfb_forward_kernel    one frame of one utterance per workgroup: alpha_t from row t-1 of the trellis and the entry costs
//                          m_u - log X[w, u]; then the per-history word-end costs, their minimum m_u and a[h, u] = exp(m_u - hist_h)
//   bgfb_product_kernel    X[w, u] = sum_h Lk[w][h] a[h, u] with v_mfma_f64_16x16x4_f64 (backward: the transposed table,
//                          Y[h, u] = sum_w Lk[w][h] b[w, u])
//   bgfb_backward_kernel   the mirror image; x_t(p) = kappa e_t(p) + beta_t(p) double-buffered per utterance, gamma over alpha
//   bgfb_words_kernel      p_t(w) = sum of gamma over w's positions (silence: the silence word and every copy)
//   bgfb_conf_kernel       per item of the bigram search's result: max of p_t(word) over the item's frames
// The top-K items come from netfb_top_kernel (viterbi_netfb.hip).
//
// The utterances of a group are ordered longest first, so the ones alive at frame t are a prefix of that order; two launches per
// frame and direction, no kernel waits on another workgroup.  No atomics and a fixed summation order in the product (each wave
// sums its quarter of the k range in ascending chunks, the four quarters are added in wave order): two identical calls return
// identical bits.  +inf stays +inf, never NaN.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "bigram_device.h"
#include "kernels.h"
#include "netfb_device.h"

namespace srgpu {

typedef double v4d __attribute__((ext_vector_type(4)));

__global__ __launch_bounds__(256) void bgfb_table_kernel(const float* lmT, uint32_t W, uint32_t Kp, uint32_t silence, double kappa,
                                                         double* lk, double* lkT) {
  const uint64_t i = (uint64_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= (uint64_t)Kp * Kp) return;
  const uint32_t w = (uint32_t)(i / Kp), h = (uint32_t)(i % Kp);
  double v = 0.0;
  if (w < W && h < W && w != silence) {
    const double x = (double)lmT[(size_t)h * W + w];
    if (x < kInf) v = exp(-kappa * x);  // (NaN fails the comparison: forbidden like +inf)
  }
  lk[(size_t)w * Kp + h] = v;
  lkT[(size_t)h * Kp + w] = v;
}

hipError_t launch_bgfb_table(const float* lmT, uint32_t W, uint32_t Kp, uint32_t silence, double kappa, double* lk, double* lkT,
                             hipStream_t stream) {
  const uint64_t n = (uint64_t)Kp * Kp;
  hipLaunchKernelGGL(bgfb_table_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, stream, lmT, W, Kp, silence, kappa, lk, lkT);
  return hipGetLastError();
}

// the block-wide sum of every thread's Lse (netfb_device.h's butterfly), the minimum kept beside the cost
__device__ inline Lse block_lse(Lse v, double* red) {
  block_lse_store(v, red);
  __syncthreads();
  Lse r;
  for (int w = 0; w < kNetFbWaves; w++) r.merge(red[2 * w], red[2 * w + 1]);
  return r;
}

// workgroup b: frame a.t of utterance a.order[b]
__global__ __launch_bounds__(kNetFbThreads) void bgfb_forward_kernel(BgFbArgs a) {
  __shared__ double red[2 * kNetFbWaves];
  const uint32_t j = blockIdx.x, u = a.order[j], tid = threadIdx.x, t = a.t;
  const uint32_t W = a.n_words, P = a.n_positions, sil = a.silence;
  const uint64_t f0 = a.frame_off[u];
  const uint32_t T = (uint32_t)(a.frame_off[u + 1] - f0);
  double* cur = a.trellis + (f0 - a.group_f0 + t) * P;
  const double* prev = cur - P;  // (read only for t > 0)
  const double* row = a.scores + (f0 - a.frame_base + t) * a.ld;
  const double* X = a.prod + (size_t)j * a.Kp;
  double* vec = a.vec + (size_t)j * a.Kp;
  double* wend = a.wend + (size_t)j * a.Kp;
  const BgCosts c = bg_costs(a.tdp, a.scale);
  const double m_in = t ? a.m[j] : 0.0;

  for (uint32_t p = tid; p < P; p += kNetFbThreads) {
    const uint32_t info = a.pos_info[p], fl = info >> 16, x = a.pos_slot[p];
    const int s = (fl & 8u) ? 1 : 0;
    double ent = kInf;
    if (fl & 3u) {  // first or second state of its slot: the slot's entry
      if (t == 0) {  // from the start's word end: the silence word at cost 0
        if (x == sil) ent = 0.0;
        else if (x < W) { const double l = (double)a.lmT[(size_t)sil * W + x]; if (l < kInf) ent = a.scale * l; }
      } else if (x < W && x != sil) ent = bg_unscale(m_in, X[x]);
      else if (x == sil) ent = wend[sil];
      else if (x - W != sil) ent = wend[x - W];
      if (fl & 2u) ent += c.t[s][2];
    }
    double v = ent;
    if (t) {
      const double l1 = (fl & 1u) ? kInf : prev[p - 1] + c.t[s][1];
      const double l2 = (fl & 3u) ? kInf : prev[p - 2] + c.t[s][2];
      v = nf_ladd(nf_ladd3(prev[p] + c.t[s][0], l1, l2), ent);
    }
    cur[p] = v < kInf ? v + a.scale * row[info & 0xFFFFu] : kInf;
  }
  __syncthreads();  // the row is read back below at the slots' last positions
  Lse ends;
  for (uint32_t h = tid; h < W; h += kNetFbThreads) {
    const double ww = cur[a.slot_off[h + 1] - 1] + c.t[h == sil ? 1 : 0][3];
    const double wc = h == sil ? kInf : cur[a.slot_off[h + W + 1] - 1] + c.t[1][3];
    const double hist = nf_ladd(ww, wc);
    wend[h] = ww;
    vec[h] = hist;
    ends.add(hist);
  }
  const Lse all = block_lse(ends, red);
  for (uint32_t h = tid; h < W; h += kNetFbThreads) {
    const double hist = vec[h];
    vec[h] = hist < kInf ? exp(all.m - hist) : 0.0;
  }
  if (tid == 0) {
    a.m[j] = all.m;
    if (t + 1 == T) a.out_cost[u] = all.cost();  // kappa F_u
  }
}

// workgroup b: frame a.t of utterance a.order[b] (a.t <= T_u - 1); rows t + 1 .. of it are done
__global__ __launch_bounds__(kNetFbThreads) void bgfb_backward_kernel(BgFbArgs a) {
  __shared__ double red[2 * kNetFbWaves];
  const uint32_t j = blockIdx.x, u = a.order[j], tid = threadIdx.x, t = a.t;
  const uint32_t W = a.n_words, P = a.n_positions, sil = a.silence;
  const uint64_t f0 = a.frame_off[u];
  const uint32_t T = (uint32_t)(a.frame_off[u + 1] - f0);
  double* tr = a.trellis + (f0 - a.group_f0 + t) * P;
  const double* row = a.scores + (f0 - a.frame_base + t) * a.ld;
  double* xcur = a.xb + ((size_t)(t & 1) * a.n_group + j) * P;
  const double* xnxt = a.xb + ((size_t)((t + 1) & 1) * a.n_group + j) * P;
  const double* Y = a.prod + (size_t)j * a.Kp;
  double* vec = a.vec + (size_t)j * a.Kp;
  double* wend = a.wend + (size_t)j * a.Kp;
  const BgCosts c = bg_costs(a.tdp, a.scale);
  const double F = a.out_cost[u];
  const bool dead = !(F < kInf), final = t + 1 == T;
  const double m_in = final ? kInf : a.m[j];

  for (uint32_t p = tid; p < P; p += kNetFbThreads) {
    const uint32_t info = a.pos_info[p], fl = info >> 16, x = a.pos_slot[p];
    const int s = (fl & 8u) ? 1 : 0;
    double b;
    if (final) {
      b = (fl & 4u) ? c.t[s][3] : kInf;
    } else {
      const uint32_t left = a.slot_off[x + 1] - 1 - p;  // positions after p in its slot
      const double s1 = left >= 1 ? c.t[s][1] + xnxt[p + 1] : kInf;
      const double s2 = left >= 2 ? c.t[s][2] + xnxt[p + 2] : kInf;
      b = nf_ladd3(c.t[s][0] + xnxt[p], s1, s2);
      if (fl & 4u) {  // a word end: into every word through the LM, and into the own copy (the silence word: into itself)
        const uint32_t h = x < W ? x : x - W;
        double r = bg_unscale(m_in, Y[h]);
        if (x < W) r = nf_ladd(r, wend[x]);
        b = nf_ladd(b, c.t[s][3] + r);
      }
    }
    double g = 0.0;
    if (!dead) {
      const double y = tr[p] + b;
      if (y < kInf) g = exp(F - y);
    }
    tr[p] = g;
    xcur[p] = b < kInf ? a.scale * row[info & 0xFFFFu] + b : kInf;
  }
  if (t == 0) return;
  __syncthreads();
  // the cost of entering each slot before this frame; b[w, u] for the product, the own-entry costs beside it
  auto entry = [&](uint32_t y, int s) {
    const uint32_t p0 = a.slot_off[y], n = a.slot_off[y + 1] - p0;
    return nf_ladd(xcur[p0], n >= 2 ? c.t[s][2] + xcur[p0 + 1] : kInf);
  };
  Lse ents;
  for (uint32_t w = tid; w < W; w += kNetFbThreads) {
    const double e = entry(w, w == sil ? 1 : 0);
    if (w == sil) {
      wend[w] = e;
      vec[w] = kInf;
    } else {
      wend[w] = entry(w + W, 1);
      vec[w] = e;
      ents.add(e);
    }
  }
  const Lse all = block_lse(ents, red);
  for (uint32_t w = tid; w < W; w += kNetFbThreads) {
    const double e = vec[w];
    vec[w] = e < kInf ? exp(all.m - e) : 0.0;
  }
  if (tid == 0) a.m[j] = all.m;
}

hipError_t launch_bgfb_forward(const BgFbArgs& a, hipStream_t stream) {
  if (a.n_alive == 0) return hipSuccess;
  hipLaunchKernelGGL(bgfb_forward_kernel, dim3(a.n_alive), dim3(kNetFbThreads), 0, stream, a);
  return hipGetLastError();
}
hipError_t launch_bgfb_backward(const BgFbArgs& a, hipStream_t stream) {
  if (a.n_alive == 0) return hipSuccess;
  hipLaunchKernelGGL(bgfb_backward_kernel, dim3(a.n_alive), dim3(kNetFbThreads), 0, stream, a);
  return hipGetLastError();
}

// out[n][m] = sum_k A[m][k] v[n][k] for n < n_alive: A [Kp x Kp] row-major, v and out [.. x Kp]; Kp a multiple of 64, v has rows up to
// the next multiple of 64 of n_alive.  Workgroup (bx, by): rows 16 bx .. + 15, columns 64 by .. + 63; wave q takes the k chunks
// 16 q + 64 i.  Within a chunk, MFMA step s of lane group g carries k = 4 g + s on BOTH operands (a permutation of the chunk: the sum
// does not care), so that a lane's four A values and four B values are 32 contiguous bytes each and neither operand needs a
// transposing stage; the LDS holds the four waves' partial tiles for the fixed-order final sum.
static constexpr int kProdNT = 4;  // 16-column tiles per workgroup
__global__ __launch_bounds__(256) void bgfb_product_kernel(const double* __restrict__ A, const double* __restrict__ v,
                                                           double* __restrict__ out, uint32_t Kp, uint32_t n_alive) {
  __shared__ double part[4][kProdNT * 4 * 64];
  const uint32_t lane = threadIdx.x & 63, q = threadIdx.x >> 6, r = lane & 15, g = lane >> 4;
  const uint32_t m0 = blockIdx.x * 16, n0 = blockIdx.y * 64;
  const uint32_t ntc = min((uint32_t)kProdNT, (n_alive - n0 + 15) / 16);
  v4d acc[kProdNT];
#pragma unroll
  for (int nt = 0; nt < kProdNT; nt++) acc[nt] = v4d{0.0, 0.0, 0.0, 0.0};
  const double* ap = A + (size_t)(m0 + r) * Kp + 4 * g;
  const double* bp = v + (size_t)(n0 + r) * Kp + 4 * g;
  for (uint32_t kc = q * 16; kc < Kp; kc += 64) {
    const v4d av = *reinterpret_cast<const v4d*>(ap + kc);
    v4d bv[kProdNT];
#pragma unroll
    for (int nt = 0; nt < kProdNT; nt++)
      bv[nt] = (uint32_t)nt < ntc ? *reinterpret_cast<const v4d*>(bp + (size_t)nt * 16 * Kp + kc) : v4d{0.0, 0.0, 0.0, 0.0};
#pragma unroll
    for (int s = 0; s < 4; s++)
#pragma unroll
      for (int nt = 0; nt < kProdNT; nt++)
        if ((uint32_t)nt < ntc) acc[nt] = __builtin_amdgcn_mfma_f64_16x16x4f64(av[s], bv[nt][s], acc[nt], 0, 0, 0);
  }
#pragma unroll
  for (int nt = 0; nt < kProdNT; nt++)
#pragma unroll
    for (int i = 0; i < 4; i++) part[q][(nt * 4 + i) * 64 + lane] = acc[nt][i];
  __syncthreads();
  for (uint32_t o = threadIdx.x; o < kProdNT * 4 * 64; o += 256) {
    const uint32_t nt = o >> 8, i = (o >> 6) & 3, l = o & 63;
    const uint32_t n = n0 + nt * 16 + (l & 15), m = m0 + (l >> 4) + 4 * i;  // f64 C/D layout: row = (lane >> 4) + 4 reg
    if (n < n_alive) out[(size_t)n * Kp + m] = ((part[0][o] + part[1][o]) + part[2][o]) + part[3][o];
  }
}

hipError_t launch_bgfb_product(const double* table, const double* v, double* out, uint32_t Kp, uint32_t n_alive, hipStream_t stream) {
  if (n_alive == 0) return hipSuccess;
  hipLaunchKernelGGL(bgfb_product_kernel, dim3(Kp / 16, (n_alive + 63) / 64), dim3(256), 0, stream, table, v, out, Kp, n_alive);
  return hipGetLastError();
}

// one wave per frame of the group, lanes over words: post[frame][w] = sum of gamma over w's positions; the silence word also takes
// every copy, in slot order
__global__ __launch_bounds__(256) void bgfb_words_kernel(BgFbArgs a, uint64_t n_frames) {
  const uint64_t f = (uint64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (f >= n_frames) return;
  const uint32_t W = a.n_words, P = a.n_positions;
  const double* g = a.trellis + f * P;
  double* out = a.post + f * W;
  for (uint32_t w = threadIdx.x & 63; w < W; w += 64) {
    if (w == a.silence) continue;
    double p = 0.0;
    for (uint32_t s = a.slot_off[w]; s < a.slot_off[w + 1]; s++) p += g[s];
    out[w] = p;
  }
  // silence: the word, then the copies' positions (contiguous from slot_off[W]) in strides of 64, summed in lane order
  double p = 0.0;
  for (uint32_t s = a.slot_off[W] + (threadIdx.x & 63); s < P; s += 64) p += g[s];
  double tot = 0.0;
  for (int l = 0; l < 64; l++) tot += __hiloint2double(__shfl(__double2hiint(p), l), __shfl(__double2loint(p), l));
  if ((threadIdx.x & 63) == 0) {
    for (uint32_t s = a.slot_off[a.silence]; s < a.slot_off[a.silence + 1]; s++) tot += g[s];
    out[a.silence] = tot;
  }
}

hipError_t launch_bgfb_words(const BgFbArgs& a, uint64_t n_frames, hipStream_t stream) {
  if (n_frames == 0) return hipSuccess;
  hipLaunchKernelGGL(bgfb_words_kernel, dim3((unsigned)((n_frames + 3) / 4)), dim3(256), 0, stream, a, n_frames);
  return hipGetLastError();
}

// one thread per utterance of the group: item i of the search's result (BigramArgs' out_* layout, utterance u at frame_off[u] + u)
// covers the 0-based frames time_{i-1} .. time_i - 1
__global__ __launch_bounds__(64) void bgfb_conf_kernel(BgFbArgs a, uint32_t n_utts, const uint32_t* it_word, const uint32_t* it_time,
                                                       const uint32_t* it_count, double* out_conf) {
  const uint32_t i = blockIdx.x * 64 + threadIdx.x;
  if (i >= n_utts) return;
  const uint32_t u = a.order[i], W = a.n_words;
  const uint64_t f0 = a.frame_off[u], o = f0 + u;
  const uint32_t T = (uint32_t)(a.frame_off[u + 1] - f0);
  const double* post = a.post + (f0 - a.group_f0) * W;
  uint32_t t0 = 0;
  for (uint32_t k = 0; k < it_count[u]; k++) {
    const uint32_t w = it_word[o + k], t1 = min(it_time[o + k], T);
    double mx = 0.0;
    if (w < W)
      for (uint32_t s = t0; s < t1; s++) mx = fmax(mx, post[(size_t)s * W + w]);
    out_conf[o + k] = fmin(mx, 1.0);  // (a sum of posteriors may round above 1)
    t0 = t1;
  }
}

hipError_t launch_bgfb_conf(const BgFbArgs& a, uint32_t n_utts, const uint32_t* it_word, const uint32_t* it_time,
                            const uint32_t* it_count, double* out_conf, hipStream_t stream) {
  if (n_utts == 0) return hipSuccess;
  hipLaunchKernelGGL(bgfb_conf_kernel, dim3((n_utts + 63) / 64), dim3(64), 0, stream, a, n_utts, it_word, it_time, it_count, out_conf);
  return hipGetLastError();
}

}  // namespace srgpu
