// viterbi_bigram_lattice.hip -- word lattices over the bigram-LM search network: the network of viterbi_bigram_fb.hip (slots 0 .. W-1
// the words, slot h + W the silence copy after word h, every history kept, no beams) in the MIN semiring, in FP64 and without a
// scale, lm and tdp widened from float.  The order of additions is the specification (tests/bigram_lattice_reference.py):
//   a position's cost = min(candidates) + emission; in-word candidate = prev + penalty; word entry = hist_h + (double) lm[w, h];
//   entry to the second state = entry + skip penalty; word end = last state + exit penalty.
// Equal candidates: in-word from the same position, one back, two back, then the entry; among equal entry terms the smallest h.
//
//   bglat_init_kernel      the history costs before frame 0 (silence 0, everything else +inf; the padding columns +inf for good)
//   bglat_entry_kernel     the min-plus W x W entry for every alive utterance of the group at once:
//                          out[u][i] = min_k (vec[u][k] + (double) tab[k][i]), forward with tab = lmT (k = history, i = word) and
//                          the arg-min (smallest k among equal terms), backward with the other orientation (k = word, i = history).
//                          A workgroup stages a 64 x 64 float tile of the table in the LDS once and shares it between its four
//                          waves, which take one utterance column each; the column's 64 values go through the LDS beside the tile
//                          (one broadcast read per term).
//                          Two arg-min routes (kSelect: compare-and-select in the loop; kRescan: min-only loop, then an equality
//                          rescan from the far end) give the same bits.
//   bglat_forward_kernel   one frame of one utterance per workgroup: (cost, first, pred) per position from the rolling row of the
//                          frame before and the entries; the word ends fwd / first / pred [frame][2W] and the history costs leave
//   bglat_backward_kernel  the mirror image on rolling rows of e_t + beta_t; bwd [frame][2W] = the cheapest continuation from a
//                          word end of the slot after frame t (0 at the last frame) leaves
//   bglat_count_kernel /   per frame the arcs (slot x, fwd finite) with fwd + bwd <= best + beam, an exclusive scan over the
//   bglat_write_kernel     group's frames (hipcub) and the arcs compacted in (frame, slot) order behind those of the groups before:
//                          lattice_emit.h's stage, shared with viterbi_lattice.hip; here its policy, BgLatEmit
//
// The utterances of a group are ordered longest first, so the ones alive at frame t are a prefix of that order; no kernel waits on
// another workgroup.  min and + only, no atomics: two identical calls return identical bits; +inf stays +inf.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "bigram_device.h"
#include "dpp_util.h"
#include "kernels.h"
#include "lattice_emit.h"

namespace srgpu {

static constexpr int kBgLatThreads = 512;
static constexpr int kBgLatWaves = kBgLatThreads / 64;

__device__ inline double bglat_min(double a, double b) { return b < a ? b : a; }

// out[h * W + w] = in[w * W + h]
__global__ __launch_bounds__(256) void bglat_transpose_kernel(const float* in, uint32_t W, float* out) {
  const uint64_t i = (uint64_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= (uint64_t)W * W) return;
  const uint32_t h = (uint32_t)(i / W), w = (uint32_t)(i % W);
  out[i] = in[(size_t)w * W + h];
}
hipError_t launch_bglat_transpose(const float* in, uint32_t W, float* out, hipStream_t stream) {
  const uint64_t n = (uint64_t)W * W;
  hipLaunchKernelGGL(bglat_transpose_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, stream, in, W, out);
  return hipGetLastError();
}

// vec[j][h] for every row of the group's vectors: the histories before frame 0
__global__ __launch_bounds__(256) void bglat_init_kernel(double* vec, uint64_t n, uint32_t Kp, uint32_t silence) {
  const uint64_t i = (uint64_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= n) return;
  vec[i] = (uint32_t)(i % Kp) == silence ? 0.0 : kInf;
}
hipError_t launch_bglat_init(const BgLatArgs& a, uint32_t rows, hipStream_t stream) {
  const uint64_t n = (uint64_t)rows * a.Kp;
  if (n == 0) return hipSuccess;
  hipLaunchKernelGGL(bglat_init_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, stream, a.vec, n, a.Kp, a.silence);
  return hipGetLastError();
}

// ---- the min-plus entry -------------------------------------------------------------------------------------------------------
static constexpr int kEntTile = 64;  // table tile: 64 k x 64 i floats (16 KiB of LDS)
static constexpr int kEntCols = 1;   // utterance columns per wave; 4 per workgroup (4 per wave: measured slower, profiles/bigram_lattice.txt)
enum { kMinOnly = 0, kSelect = 1, kRescan = 2 };

// tab [W x W] row-major (row k, column i), vec / out [.. x Kp] (vec[.][k] = +inf for k >= W), arg [.. x Kp].  Workgroup (bx, by):
// outputs i = 64 bx + lane, columns 4 kEntCols by + kEntCols wave + 0 .. kEntCols - 1 (clamped to n_alive - 1 for the loads, stores
// guarded).
template <int kMode>
__global__ __launch_bounds__(256) void bglat_entry_kernel(const float* __restrict__ tab, const double* __restrict__ vec,
                                                          double* __restrict__ out, uint32_t* __restrict__ arg, uint32_t W, uint32_t Kp,
                                                          uint32_t n_alive) {
  __shared__ float tile[kEntTile][kEntTile];
  __shared__ double vtile[4 * kEntCols][kEntTile];  // the waves' columns, the tile's 64 k each
  const uint32_t lane = threadIdx.x & 63, q = (uint32_t)__builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
  const uint32_t i = blockIdx.x * kEntTile + lane, n0 = blockIdx.y * (4 * kEntCols) + q * kEntCols;
  const double* vp[kEntCols];
#pragma unroll
  for (int c = 0; c < kEntCols; c++) vp[c] = vec + (size_t)min(n0 + c, n_alive - 1) * Kp;
  double m[kEntCols];
  uint32_t am[kEntCols];
#pragma unroll
  for (int c = 0; c < kEntCols; c++) { m[c] = kInf; am[c] = 0; }
  // a NaN score is a forbidden transition like +inf; rows and columns beyond the table are +inf.  A tile is fetched into registers
  // while the tile before is worked on, and committed to the LDS between two barriers.
  float reg[kEntTile / 4];
  double vreg[kEntCols];
  auto fetch = [&](uint32_t k0) {
#pragma unroll
    for (int c = 0; c < kEntCols; c++) vreg[c] = vp[c][k0 + lane];
#pragma unroll
    for (int r = 0; r < kEntTile / 4; r++) {
      const uint32_t k = k0 + q + 4 * r;
      float v = __builtin_huge_valf();
      if (k < W && i < W) {
        const float x = tab[(size_t)k * W + i];
        v = x == x ? x : v;
      }
      reg[r] = v;
    }
  };
  auto commit = [&]() {
    __syncthreads();  // (the tile before is consumed)
#pragma unroll
    for (int r = 0; r < kEntTile / 4; r++) tile[q + 4 * r][lane] = reg[r];
#pragma unroll
    for (int c = 0; c < kEntCols; c++) vtile[q * kEntCols + c][lane] = vreg[c];
    __syncthreads();
  };
  fetch(0);
  for (uint32_t k0 = 0; k0 < Kp; k0 += kEntTile) {
    commit();
    if (k0 + kEntTile < Kp) fetch(k0 + kEntTile);
    else if (kMode == kRescan) fetch(Kp - kEntTile);  // (the rescan starts where the loop ends)
#pragma unroll 8
    for (int kk = 0; kk < kEntTile; kk++) {
      const double l = (double)tile[kk][lane];
#pragma unroll
      for (int c = 0; c < kEntCols; c++) {
        const double t = vtile[q * kEntCols + c][kk] + l;
        const double mn = __builtin_fmin(m[c], t);
        if (kMode == kSelect) am[c] = mn != m[c] ? k0 + kk : am[c];  // (an equal term leaves the earlier k)
        m[c] = mn;
      }
    }
  }
  if (kMode == kRescan) {  // from the far end, so that the smallest k among the equal terms is the one that stays
    for (uint32_t k0 = Kp; k0 > 0;) {
      k0 -= kEntTile;
      commit();
      if (k0) fetch(k0 - kEntTile);
#pragma unroll 8
      for (int kk = kEntTile - 1; kk >= 0; kk--) {
        const double l = (double)tile[kk][lane];
#pragma unroll
        for (int c = 0; c < kEntCols; c++) am[c] = vtile[q * kEntCols + c][kk] + l == m[c] ? k0 + kk : am[c];
      }
    }
  }
#pragma unroll
  for (int c = 0; c < kEntCols; c++)
    if (n0 + c < n_alive) {
      out[(size_t)(n0 + c) * Kp + i] = m[c];
      if (kMode != kMinOnly) arg[(size_t)(n0 + c) * Kp + i] = am[c];
    }
}

hipError_t launch_bglat_entry(const float* tab, const double* vec, double* out, uint32_t* arg, uint32_t W, uint32_t Kp, uint32_t n_alive,
                              int argmin, hipStream_t stream) {
  if (n_alive == 0) return hipSuccess;
  const dim3 grid(Kp / kEntTile, (n_alive + 4 * kEntCols - 1) / (4 * kEntCols));
  if (!arg) hipLaunchKernelGGL(bglat_entry_kernel<kMinOnly>, grid, dim3(256), 0, stream, tab, vec, out, arg, W, Kp, n_alive);
  else if (argmin == 1) hipLaunchKernelGGL(bglat_entry_kernel<kRescan>, grid, dim3(256), 0, stream, tab, vec, out, arg, W, Kp, n_alive);
  else hipLaunchKernelGGL(bglat_entry_kernel<kSelect>, grid, dim3(256), 0, stream, tab, vec, out, arg, W, Kp, n_alive);
  return hipGetLastError();
}

// ---- the in-word steps ----------------------------------------------------------------------------------------------------------
// workgroup b: frame a.t of utterance a.order[b]
__global__ __launch_bounds__(kBgLatThreads) void bglat_forward_kernel(BgLatArgs a) {
  __shared__ double red[kBgLatWaves];
  const uint32_t j = blockIdx.x, u = a.order[j], tid = threadIdx.x, t = a.t;
  const uint32_t W = a.n_words, P = a.n_positions, sil = a.silence, S = 2 * W;
  const uint64_t f0 = a.frame_off[u];
  const uint32_t T = (uint32_t)(a.frame_off[u + 1] - f0);
  const uint64_t g = f0 - a.group_f0 + t;  // the frame within the group
  const size_t rc = ((size_t)(t & 1) * a.n_group + j) * P, rp = ((size_t)((t + 1) & 1) * a.n_group + j) * P;
  double* cur = a.row + rc;
  uint16_t* cst = a.row_first + rc;
  uint32_t* cpr = a.row_pred + rc;
  const double* prev = a.row + rp;  // (read only for t > 0)
  const uint16_t* pst = a.row_first + rp;
  const uint32_t* ppr = a.row_pred + rp;
  const double* row = a.scores + (f0 - a.frame_base + t) * a.ld;
  const double* X = a.prod + (size_t)j * a.Kp;
  const uint32_t* XA = a.arg + (size_t)j * a.Kp;
  const double* wprev = a.fwd + (t ? g - 1 : g) * S;  // the word ends of the frame before (read only for t > 0)
  const BgCosts c = bg_costs(a.tdp);

  for (uint32_t p = tid; p < P; p += kBgLatThreads) {
    const uint32_t info = a.pos_info[p], fl = info >> 16, x = a.pos_slot[p];
    const int s = (fl & 8u) ? 1 : 0;
    double v = kInf;
    uint32_t b = 0, pr = 0;
    if (t) {
      v = prev[p] + c.t[s][0]; b = pst[p]; pr = ppr[p];
      if (!(fl & 1u)) {
        const double x1 = prev[p - 1] + c.t[s][1];
        if (x1 < v) { v = x1; b = pst[p - 1]; pr = ppr[p - 1]; }
      }
      if (!(fl & 3u)) {
        const double x2 = prev[p - 2] + c.t[s][2];
        if (x2 < v) { v = x2; b = pst[p - 2]; pr = ppr[p - 2]; }
      }
    }
    if (fl & 3u) {  // first or second state of its slot: the slot's entry
      double ent = kInf;
      uint32_t epr;
      if (x < W && x != sil) { ent = X[x]; epr = XA[x]; }
      else if (x == sil) { ent = t ? wprev[sil] : 0.0; epr = sil; }  // the start's word end: the silence word at cost 0
      else { epr = x - W; if (t && epr != sil) ent = wprev[epr]; }
      if (fl & 2u) ent += c.t[s][2];
      if (ent < v) { v = ent; b = t; pr = epr; }
    }
    double r = v + row[info & 0xFFFFu];
    if (!(r < kInf)) r = kInf;
    cur[p] = r;
    cst[p] = (uint16_t)b;
    cpr[p] = pr;
  }
  __syncthreads();  // the row is read back below at the slots' last positions
  double* fw = a.fwd + g * S;
  uint16_t* fi = a.first + g * S;
  uint32_t* pd = a.pred + g * S;
  double* vec = a.vec + (size_t)j * a.Kp;
  double mine = kInf;
  for (uint32_t h = tid; h < W; h += kBgLatThreads) {
    const uint32_t pw = a.slot_off[h + 1] - 1, pc = a.slot_off[h + W + 1] - 1;
    const double ww = cur[pw] + c.t[h == sil ? 1 : 0][3], wc = cur[pc] + c.t[1][3];
    fw[h] = ww; fi[h] = cst[pw]; pd[h] = cpr[pw];
    fw[h + W] = wc; fi[h + W] = cst[pc]; pd[h + W] = cpr[pc];
    vec[h] = h == sil ? ww : bglat_min(ww, wc);
    mine = bglat_min(mine, bglat_min(ww, wc));
  }
  if (t + 1 != T) return;
#pragma unroll
  for (int k = 1; k < 64; k <<= 1) mine = bglat_min(mine, shfl_xor_f64(mine, k));
  if ((tid & 63) == 0) red[tid >> 6] = mine;
  __syncthreads();
  if (tid == 0) {
    double best = red[0];
    for (int w = 1; w < kBgLatWaves; w++) best = bglat_min(best, red[w]);
    a.out_best[u] = best;
  }
}

// workgroup b: frame a.t of utterance a.order[b] (a.t <= T_u - 1); the frames after it are done
__global__ __launch_bounds__(kBgLatThreads) void bglat_backward_kernel(BgLatArgs a) {
  const uint32_t j = blockIdx.x, u = a.order[j], tid = threadIdx.x, t = a.t;
  const uint32_t W = a.n_words, P = a.n_positions, sil = a.silence, S = 2 * W;
  const uint64_t f0 = a.frame_off[u];
  const uint32_t T = (uint32_t)(a.frame_off[u + 1] - f0);
  const uint64_t g = f0 - a.group_f0 + t;
  const double* row = a.scores + (f0 - a.frame_base + t) * a.ld;
  double* xcur = a.row + ((size_t)(t & 1) * a.n_group + j) * P;
  const double* xnxt = a.row + ((size_t)((t + 1) & 1) * a.n_group + j) * P;
  const double* Y = a.prod + (size_t)j * a.Kp;
  double* vec = a.vec + (size_t)j * a.Kp;
  double* wend = a.wend + (size_t)j * a.Kp;
  double* bw = a.bwd + g * S;
  const BgCosts c = bg_costs(a.tdp);
  const bool final = t + 1 == T;

  for (uint32_t p = tid; p < P; p += kBgLatThreads) {
    const uint32_t info = a.pos_info[p], fl = info >> 16, x = a.pos_slot[p];
    const int s = (fl & 8u) ? 1 : 0;
    double b;
    if (final) {
      b = (fl & 4u) ? c.t[s][3] : kInf;
      if (fl & 4u) bw[x] = 0.0;
    } else {
      const uint32_t left = a.slot_off[x + 1] - 1 - p;  // positions after p in its slot
      b = c.t[s][0] + xnxt[p];
      if (left >= 1) b = bglat_min(b, c.t[s][1] + xnxt[p + 1]);
      if (left >= 2) b = bglat_min(b, c.t[s][2] + xnxt[p + 2]);
      if (fl & 4u) {  // a word end: into every word through the LM, and into the own copy (the silence word: into itself)
        double r = Y[x < W ? x : x - W];
        if (x < W) r = bglat_min(r, wend[x]);
        bw[x] = r;
        b = bglat_min(b, c.t[s][3] + r);
      }
    }
    if (!(b < kInf)) b = kInf;
    xcur[p] = b < kInf ? row[info & 0xFFFFu] + b : kInf;
  }
  if (t == 0) return;
  __syncthreads();
  // the cost of entering each slot before this frame: the words' for the min-plus entry, the own-entry costs beside it
  auto entry = [&](uint32_t y, int s) {
    const uint32_t p0 = a.slot_off[y], n = a.slot_off[y + 1] - p0;
    return bglat_min(xcur[p0], n >= 2 ? c.t[s][2] + xcur[p0 + 1] : kInf);
  };
  for (uint32_t w = tid; w < W; w += kBgLatThreads) {
    const double e = entry(w, w == sil ? 1 : 0);
    if (w == sil) {
      wend[w] = e;
      vec[w] = kInf;  // no transition into silence through the LM
    } else {
      wend[w] = entry(w + W, 1);
      vec[w] = e;
    }
  }
}

hipError_t launch_bglat_forward(const BgLatArgs& a, hipStream_t stream) {
  if (a.n_alive == 0) return hipSuccess;
  hipLaunchKernelGGL(bglat_forward_kernel, dim3(a.n_alive), dim3(kBgLatThreads), 0, stream, a);
  return hipGetLastError();
}
hipError_t launch_bglat_backward(const BgLatArgs& a, hipStream_t stream) {
  if (a.n_alive == 0) return hipSuccess;
  hipLaunchKernelGGL(bglat_backward_kernel, dim3(a.n_alive), dim3(kBgLatThreads), 0, stream, a);
  return hipGetLastError();
}

// ---- the arcs (lattice_emit.h) ----------------------------------------------------------------------------------------------------
struct BgLatEmit {
  const BgLatArgs& a;
  __device__ uint32_t n_utts() const { return a.n_group; }
  __device__ uint32_t slots() const { return 2 * a.n_words; }
  __device__ bool keep(uint64_t g, uint32_t x, double limit) const {
    const size_t i = g * 2 * a.n_words + x;
    const double f = a.fwd[i];
    const double tot = f + a.bwd[i];
    return f < kInf && tot < kInf && tot <= limit;
  }
  __device__ int frame(uint64_t) const { return 0; }  // (bwd depends on the slot: nothing to hold)
  __device__ void write(uint64_t i, uint64_t g, uint32_t x, uint64_t uf, int) const {
    const uint32_t W = a.n_words, S = 2 * W, sil = a.silence;
    const double f = a.fwd[g * S + x];
    const uint32_t b = a.first[g * S + x], pr = a.pred[g * S + x];
    const bool word = x < W && x != sil;
    double c_in = 0.0;  // the cost the entry started from (the start: 0)
    if (b) {
      const double* we = a.fwd + (uf + b - 1) * S;
      if (!word) c_in = we[x < W ? sil : x - W];
      else c_in = pr == sil ? we[sil] : bglat_min(we[pr], we[pr + W]);
    }
    const double lmc = word ? (double)a.lmT[(size_t)pr * W + x] : 0.0;
    a.arc_word[i] = x < W ? x : sil;
    a.arc_hist[i] = x < W ? x : x - W;
    a.arc_pred[i] = pr;
    a.arc_first[i] = b;
    a.arc_last[i] = (uint32_t)(g - uf);
    a.arc_fwd[i] = f;
    a.arc_bwd[i] = a.bwd[g * S + x];
    a.arc_am[i] = (f - c_in) - lmc;
  }
};

__global__ __launch_bounds__(256) void bglat_count_kernel(BgLatArgs a, uint64_t n_frames, uint64_t* cnt) {
  emit_count(BgLatEmit{a}, n_frames, cnt);
}
__global__ __launch_bounds__(256) void bglat_write_kernel(BgLatArgs a, uint64_t n_frames, const uint64_t* scan, const uint64_t* arc_base,
                                                          uint64_t* frame_arc, uint64_t cap) {
  emit_write(BgLatEmit{a}, n_frames, scan, arc_base, frame_arc, cap);
}
__global__ void bglat_advance_kernel(const uint64_t* cnt, const uint64_t* scan, uint64_t n_frames, uint64_t* arc_base) {
  emit_advance(cnt, scan, n_frames, arc_base);
}

hipError_t launch_bglat_emit(const BgLatArgs& a, uint64_t n_frames, void* scan_temp, size_t scan_temp_bytes, uint64_t* cnt, uint64_t* scan,
                             uint64_t* arc_base, uint64_t* frame_arc, uint64_t cap, hipStream_t stream) {
  return launch_emit(bglat_count_kernel, bglat_write_kernel, bglat_advance_kernel, a, a.n_group, n_frames, scan_temp, scan_temp_bytes,
                     cnt, scan, arc_base, frame_arc, cap, stream);
}

}  // namespace srgpu
