// viterbi_bigram_smbr.hip -- the step kernels of sMBR training over the bigram search network (viterbi_bigram_fb.hip's network, scale
// kappa, penalties, start and launch groups): beside alpha and beta, the expected number of correctly labelled frames of the paths
// through every (frame, position), and from it the signed weights gamma_t(s) = occ_t(s) (abar_t(s) + bbar_t(s) - Abar).
//
// Accuracy.  A path scores 1 at frame t when the mixture of the position it occupies there is ref[t].  An entry in this network emits
// the mixture of the state it moves TO, so every source of a position pays the same emission and scores the same [state(s) == ref_t]:
// the accuracy of a sum is the mean of its sources' plus that one term.  ref[t] >= the state count matches no position.
//
//   bgsmbr_forward_kernel    bgfb_forward_kernel with an accuracy beside every cost (smbr_device.h's La: the weights are the exp values
//                            the log-add takes anyway, the costs keep bgfb_forward_kernel's bits).  abar_t(s) = the expected accuracy
//                            of frames 0 .. t over the paths reaching s at t.  A history's accuracy hbar_h is the mean of its word's
//                            and its copy's ends; the block-wide sum carries sum exp(m - hist_h) hbar_h as a third component and gives
//                            kappa F_u and Abar_u at the last frame.  Two operand vectors per utterance: a[h, u] = exp(m_u - hist_h)
//                            and a[h, u] hbar_h; launch_bgfb_product on both (twice the columns) gives X and Xa, the entry of word w
//                            costs m_u - log X[w, u] at accuracy Xa / X, and is taken iff X > 0.
//   bgsmbr_backward_kernel   the mirror image: beta_t(s) and bbar_t(s) = the expected accuracy of frames t + 1 .. over the
//                            continuations of s at t.  Double-buffered per utterance are x_t(s) = kappa e_t(s) + beta_t(s) and, beside
//                            it, [state(s) == ref_t] + bbar_t(s); the operands are b[w, u] = exp(m_u - entry cost of w) and b times
//                            the entry's accuracy, multiplied with the transposed table.  A thread reads row t of the trellis at its
//                            own position only, so the signed gamma_t(s) goes over alpha_t(s) in the same loop.
// The items and their ranking come from the item path (posterior_items.hip): the signed sums, wide mixtures across the wave.
//
// Per utterance of a group: trellis rows [alpha[P], abar[P]] = 16 B per (frame, position); vec / prod / wend of two rows [Kp] each (the
// second row is the accuracy side); x of [2][2][P].  No atomics and a fixed summation order: two identical calls return identical bits.
// +inf stays +inf, never NaN: an accuracy is finite everywhere, 0 where its cost is +inf.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "bigram_device.h"
#include "kernels.h"
#include "netfb_device.h"
#include "smbr_device.h"

namespace srgpu {

// workgroup b: frame a.t of utterance a.order[b]
__global__ __launch_bounds__(kNetFbThreads) void bgsmbr_forward_kernel(BgSmbrArgs sa) {
  __shared__ double red[3 * kNetFbWaves];
  const BgFbArgs& a = sa.fb;
  const uint32_t j = blockIdx.x, u = a.order[j], tid = threadIdx.x, t = a.t;
  const uint32_t W = a.n_words, P = a.n_positions, sil = a.silence;
  const uint64_t f0 = a.frame_off[u];
  const uint32_t T = (uint32_t)(a.frame_off[u + 1] - f0);
  double* cur = a.trellis + (f0 - a.group_f0 + t) * 2 * P;
  double* cura = cur + P;
  const double* prev = cur - 2 * (size_t)P;  // (read only for t > 0)
  const double* preva = prev + P;
  const double* row = a.scores + (f0 - a.frame_base + t) * a.ld;
  const double* X = a.prod + (size_t)2 * j * a.Kp;
  const double* Xa = X + a.Kp;
  double* vec = a.vec + (size_t)2 * j * a.Kp;
  double* veca = vec + a.Kp;
  double* wend = a.wend + (size_t)2 * j * a.Kp;
  double* wenda = wend + a.Kp;
  const BgCosts c = bg_costs(a.tdp, a.scale);
  const double m_in = t ? a.m[j] : 0.0;
  const uint32_t rf = sa.ref[f0 + t];

  for (uint32_t p = tid; p < P; p += kNetFbThreads) {
    const uint32_t info = a.pos_info[p], fl = info >> 16, x = a.pos_slot[p];
    const bool s = (fl & 8u) != 0;
    La ent{kInf, 0.0};
    if (fl & 3u) {  // first or second state of its slot: the slot's entry
      if (t == 0) {  // from the start's word end: the silence word at cost 0, no frame scored
        if (x == sil) ent.x = 0.0;
        else if (x < W) { const double l = (double)a.lmT[(size_t)sil * W + x]; if (l < kInf) ent.x = a.scale * l; }
      } else if (x < W && x != sil) {
        const double y = X[x];
        ent.x = bg_unscale(m_in, y);
        if (ent.x < kInf) ent.a = Xa[x] / y;
      } else if (x == sil) ent = La{wend[sil], wenda[sil]};
      else if (x - W != sil) ent = La{wend[x - W], wenda[x - W]};
      if (fl & 2u) ent.x += bgs_pen<2>(c, s);
    }
    La v = ent;
    if (t) {
      const La l0{prev[p] + bgs_pen<0>(c, s), preva[p]};
      La l1{kInf, 0.0}, l2{kInf, 0.0};
      if (!(fl & 1u)) l1 = La{prev[p - 1] + bgs_pen<1>(c, s), preva[p - 1]};
      if (!(fl & 3u)) l2 = La{prev[p - 2] + bgs_pen<2>(c, s), preva[p - 2]};
      v = la_add(la_add3(l0, l1, l2), ent);
    }
    const bool ok = v.x < kInf;
    cur[p] = ok ? v.x + a.scale * row[info & 0xFFFFu] : kInf;
    cura[p] = ok ? v.a + hit(info, rf) : 0.0;
  }
  __syncthreads();  // the row is read back below at the slots' last positions
  LseA ends;
  for (uint32_t h = tid; h < W; h += kNetFbThreads) {
    const uint32_t e = a.slot_off[h + 1] - 1;
    const La ww{cur[e] + bgs_pen<3>(c, h == sil), cura[e]};
    La wc{kInf, 0.0};
    if (h != sil) {
      const uint32_t ec = a.slot_off[h + W + 1] - 1;
      wc = La{cur[ec] + c.t[1][3], cura[ec]};
    }
    const La hist = la_add(ww, wc);
    wend[h] = ww.x; wenda[h] = ww.a;
    vec[h] = hist.x; veca[h] = hist.a;
    ends.add(hist.x, hist.a);
  }
  block_lsea_store(ends, red);
  __syncthreads();
  LseA all;
  for (int w = 0; w < kNetFbWaves; w++) all.merge(red[3 * w], red[3 * w + 1], red[3 * w + 2]);
  for (uint32_t h = tid; h < W; h += kNetFbThreads) {
    const double hist = vec[h];
    const double av = hist < kInf ? exp(all.m - hist) : 0.0;
    vec[h] = av;
    veca[h] = av * veca[h];
  }
  if (tid == 0) {
    a.m[j] = all.m;
    if (t + 1 == T) {
      const La E = all.value();
      a.out_cost[u] = E.x;   // kappa F_u
      sa.out_acc[u] = E.a;   // Abar_u (0 for F_u = +inf)
    }
  }
}

// the cost of entering slot y before the frame whose (x, xa) rows are given, and the expected accuracy from that frame on
__device__ inline La bgs_entry(const double* x, const double* xa, const uint32_t* slot_off, uint32_t y, double skip) {
  const uint32_t p0 = slot_off[y], n = slot_off[y + 1] - p0;
  const La e0{x[p0], xa[p0]};
  La e1{kInf, 0.0};
  if (n >= 2) e1 = La{skip + x[p0 + 1], xa[p0 + 1]};
  return la_add(e0, e1);
}

// workgroup b: frame a.t of utterance a.order[b] (a.t <= T_u - 1); rows t + 1 .. of it are done
__global__ __launch_bounds__(kNetFbThreads) void bgsmbr_backward_kernel(BgSmbrArgs sa) {
  __shared__ double red[2 * kNetFbWaves];
  const BgFbArgs& a = sa.fb;
  const uint32_t j = blockIdx.x, u = a.order[j], tid = threadIdx.x, t = a.t;
  const uint32_t W = a.n_words, P = a.n_positions, sil = a.silence;
  const uint64_t f0 = a.frame_off[u];
  const uint32_t T = (uint32_t)(a.frame_off[u + 1] - f0);
  double* tr = a.trellis + (f0 - a.group_f0 + t) * 2 * P;
  const double* row = a.scores + (f0 - a.frame_base + t) * a.ld;
  double* xcur = a.xb + ((size_t)(t & 1) * a.n_group + j) * 2 * P;
  double* xcura = xcur + P;
  const double* xnxt = a.xb + ((size_t)((t + 1) & 1) * a.n_group + j) * 2 * P;
  const double* xnxta = xnxt + P;
  const double* Y = a.prod + (size_t)2 * j * a.Kp;
  const double* Ya = Y + a.Kp;
  double* vec = a.vec + (size_t)2 * j * a.Kp;
  double* veca = vec + a.Kp;
  double* wend = a.wend + (size_t)2 * j * a.Kp;
  double* wenda = wend + a.Kp;
  const BgCosts c = bg_costs(a.tdp, a.scale);
  const double F = a.out_cost[u], A = sa.out_acc[u];  // kappa F_u, Abar_u
  const bool dead = !(F < kInf), final = t + 1 == T;
  const double m_in = final ? kInf : a.m[j];
  const uint32_t rf = sa.ref[f0 + t];

  for (uint32_t p = tid; p < P; p += kNetFbThreads) {
    const uint32_t info = a.pos_info[p], fl = info >> 16, x = a.pos_slot[p];
    const bool s = (fl & 8u) != 0;
    La b{kInf, 0.0};
    if (final) {
      if (fl & 4u) b.x = bgs_pen<3>(c, s);
    } else {
      const uint32_t left = a.slot_off[x + 1] - 1 - p;  // positions after p in its slot
      const La s0{bgs_pen<0>(c, s) + xnxt[p], xnxta[p]};
      La s1{kInf, 0.0}, s2{kInf, 0.0};
      if (left >= 1) s1 = La{bgs_pen<1>(c, s) + xnxt[p + 1], xnxta[p + 1]};
      if (left >= 2) s2 = La{bgs_pen<2>(c, s) + xnxt[p + 2], xnxta[p + 2]};
      b = la_add3(s0, s1, s2);
      if (fl & 4u) {  // a word end: into every word through the LM, and into the own copy (the silence word: into itself)
        const uint32_t h = x < W ? x : x - W;
        const double y = Y[h];
        La r{bg_unscale(m_in, y), 0.0};
        if (r.x < kInf) r.a = Ya[h] / y;
        if (x < W) r = la_add(r, La{wend[x], wenda[x]});
        b = la_add(b, La{bgs_pen<3>(c, s) + r.x, r.a});
      }
    }
    const bool ok = b.x < kInf;
    if (!ok) b.a = 0.0;
    double g = 0.0;
    if (!dead) {
      const double y = tr[p] + b.x;
      if (y < kInf) g = exp(F - y) * (tr[P + p] + b.a - A);
    }
    tr[p] = g;
    xcur[p] = ok ? a.scale * row[info & 0xFFFFu] + b.x : kInf;
    xcura[p] = ok ? hit(info, rf) + b.a : 0.0;
  }
  if (t == 0) return;
  __syncthreads();
  // the cost of entering each slot before this frame with the accuracy from it on; b[w, u] and b times that accuracy for the
  // product, the own-entry pairs beside them
  Lse ents;
  for (uint32_t w = tid; w < W; w += kNetFbThreads) {
    const La e = bgs_entry(xcur, xcura, a.slot_off, w, bgs_pen<2>(c, w == sil));
    if (w == sil) {
      wend[w] = e.x; wenda[w] = e.a;
      vec[w] = kInf; veca[w] = 0.0;
    } else {
      const La ec = bgs_entry(xcur, xcura, a.slot_off, w + W, c.t[1][2]);
      wend[w] = ec.x; wenda[w] = ec.a;
      vec[w] = e.x; veca[w] = e.a;
      ents.add(e.x);
    }
  }
  block_lse_store(ents, red);
  __syncthreads();
  Lse all;
  for (int w = 0; w < kNetFbWaves; w++) all.merge(red[2 * w], red[2 * w + 1]);
  for (uint32_t w = tid; w < W; w += kNetFbThreads) {
    const double e = vec[w];
    const double bv = e < kInf ? exp(all.m - e) : 0.0;
    vec[w] = bv;
    veca[w] = bv * veca[w];
  }
  if (tid == 0) a.m[j] = all.m;
}

hipError_t launch_bgsmbr_forward(const BgSmbrArgs& a, hipStream_t stream) {
  if (a.fb.n_alive == 0) return hipSuccess;
  hipLaunchKernelGGL(bgsmbr_forward_kernel, dim3(a.fb.n_alive), dim3(kNetFbThreads), 0, stream, a);
  return hipGetLastError();
}
hipError_t launch_bgsmbr_backward(const BgSmbrArgs& a, hipStream_t stream) {
  if (a.fb.n_alive == 0) return hipSuccess;
  hipLaunchKernelGGL(bgsmbr_backward_kernel, dim3(a.fb.n_alive), dim3(kNetFbThreads), 0, stream, a);
  return hipGetLastError();
}

}  // namespace srgpu
