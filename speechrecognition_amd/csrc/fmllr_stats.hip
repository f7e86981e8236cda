// fmllr_stats.hip -- fMLLR / constrained MLLR (Gales 1998): per-speaker statistics of a set of (frame, density, weight) pairs, and the
// adapted corpus.
//
// With xi_t = (x_t1 .. x_tD, 1), iv = 1/var and mu the tables of density d, speaker s collects over the pairs (t, d, gamma) of its
// utterances
//   beta       = sum gamma
//   k[i][j]    = sum gamma mu_di iv_di xi_tj                  i < D, j <= D
//   G[i][j][k] = sum gamma iv_di xi_tj xi_tk                  i < D, j, k <= D
// The pairs are em_assign_kernel's / em_assign_weighted_kernel's (em_accumulate.hip), with the density id kept beside the accumulator
// keys (EmArgs::pair_dens); a pair whose key is 0xFFFFFFFF was dropped there and is skipped here.
//
//   1. fmllr_fold_kernel     one thread per (frame, row): the frame's pairs, in pair order, folded into a_t[i] = sum_d gamma iv_di and
//                            c_t[i] = sum_d (gamma iv_di) mu_di; row D of c_t is g_t = sum_d gamma (row D of a_t is 0).
//   2. fmllr_contract_kernel G[i][(j,k)] = sum_t a_t[i] (xi_tj xi_tk): the shared symmetric contraction (sym_contract.h) over a speaker's
//                            frames in corpus order, staged as xi_t (FP64 from the float features) and the rows a_t, c_t.  k is the
//                            same contraction with c_t and the columns (j, D): xi_tD = 1, so its row D, column D is beta.
//   3. grouped_reduce_kernel the partials of a speaker's segments added in ascending order: both triangles of G from the one sum, k and
//                            beta.  MLLR's groups go through the same kernel (launch_grouped_reduce).
// Segments, summation order and the promise of identical bits are sym_contract.h's.
//
//   fmllr_transform_kernel   y_ti = (float)(b_i + sum_j A_ij (double) x_tj), j ascending, no contraction into FMAs: the order of operations
//                            is the specification.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "kernels.h"
#include "sym_contract.h"

namespace srgpu {

#pragma clang fp contract(off)

uint32_t fmllr_seg_frames() { return kSegLen; }
uint32_t fmllr_max_dim() { return 63; }

FmllrShape fmllr_shape(uint32_t dim) {
  FmllrShape s{};
  const uint32_t E = dim + 1;
  s.rows = (E + 15u) & ~15u;
  s.g_cols = E * (E + 1) / 2;
  s.g_tiles = (s.g_cols + 15u) / 16u;
  s.k_tiles = (E + 15u) / 16u;
  s.cols = (s.g_tiles + s.k_tiles) * 16u;
  return s;
}

// frame_pair_off[t] = first pair of frame t's items (Baum-Welch pairs: items in frame order, item i's pairs end at item_pair_end[i])
__global__ __launch_bounds__(256) void fmllr_item_frames_kernel(const uint32_t* item_off, const uint64_t* item_pair_end, uint64_t n_frames,
                                                                uint64_t* frame_pair_off) {
  const uint64_t t = (uint64_t)blockIdx.x * 256 + threadIdx.x;
  if (t > n_frames) return;
  const uint32_t i = item_off[t];
  frame_pair_off[t] = i ? item_pair_end[i - 1] : 0;
}

hipError_t launch_fmllr_item_frames(const uint32_t* item_off, const uint64_t* item_pair_end, uint64_t n_frames, uint64_t* frame_pair_off,
                                    hipStream_t stream) {
  hipLaunchKernelGGL(fmllr_item_frames_kernel, dim3((unsigned)(n_frames / 256 + 1)), dim3(256), 0, stream, item_off, item_pair_end, n_frames,
                     frame_pair_off);
  return hipGetLastError();
}

__global__ __launch_bounds__(256) void fmllr_fold_kernel(FmllrArgs a) {
  const uint32_t R = a.g.shape.rows, D = a.dim;
  const uint64_t idx = (uint64_t)blockIdx.x * 256 + threadIdx.x;
  if (idx >= a.n_frames * R) return;
  const uint64_t t = idx / R;
  const uint32_t i = (uint32_t)(idx - t * R);
  double av = 0.0, cv = 0.0;
  if (i <= D) {
    const uint64_t p0 = a.frame_pair_off[t], p1 = a.frame_pair_off[t + 1];
    for (uint64_t p = p0; p < p1; p++) {
      if (a.pair_key[p] == 0xFFFFFFFFu) continue;  // dropped by the assignment (membership < 1e-8, empty mixture)
      const double g = a.pair_w[p];
      if (i == D) { cv = cv + g; continue; }
      const uint64_t o = (uint64_t)a.pair_dens[p] * D + i;
      const double giv = g * a.inv_vars[o];
      av = av + giv;
      cv = cv + giv * a.means[o];
    }
  }
  a.fold_a[idx] = av;
  a.fold_c[idx] = cv;
}

// a stage of a speaker's frames: xi_t on the column side, the fold's a_t and c_t on the row side
struct FmllrStager {
  static constexpr bool kTwoRows = true, kPreStage = false;
  const FmllrArgs& a;
  const uint32_t s0, sn;  // the segment: frame_list[s0 .. s0 + sn)
  __device__ void column(uint32_t n, uint32_t* j, uint32_t* k) const { affine_column(a.g.shape, a.dim + 1, n, j, k); }
  __device__ double col(uint32_t f0, uint32_t f, uint32_t j) const {
    const uint32_t D = a.dim;
    if (f0 + f < sn && j <= D) return j < D ? (double)a.feats[(uint64_t)a.frame_list[s0 + f0 + f] * D + j] : 1.0;
    return 0.0;
  }
  __device__ void rows(uint32_t f0, uint32_t f, uint32_t i, double* va, double* vc) const {
    if (f0 + f >= sn) return;
    const uint64_t o = (uint64_t)a.frame_list[s0 + f0 + f] * a.g.shape.rows + i;
    *va = a.fold_a[o];
    *vc = a.fold_c[o];
  }
};

// grid (segments, column-tile groups); RT = row tiles of 16
template <int RT>
__global__ __launch_bounds__(kWaves * 64) void fmllr_contract_kernel(FmllrArgs a) {
  const uint32_t seg = blockIdx.x, sn = a.g.seg_len[seg];
  const FmllrShape& s = a.g.shape;
  contract_segment<RT>(FmllrStager{a, a.g.seg_begin[seg], sn}, sn, s.g_tiles + s.k_tiles, s.g_tiles,
                       a.g.partial + (uint64_t)seg * s.rows * s.cols, s.cols);
}

// One thread per (group, row, column) of a GroupedStats contraction (fMLLR: group = speaker; MLLR: speaker x class): the partials of
// the group's segments added in ascending order; writes both triangles of G from the one sum (exactly symmetric), k and beta.
// grid (groups x ceil(cols / 256), rows <= D)
__global__ __launch_bounds__(256) void grouped_reduce_kernel(GroupedStats a, uint32_t D) {
  const uint32_t E = D + 1, C = a.shape.cols;
  const uint32_t nb = (C + 255u) / 256u, g = blockIdx.x / nb;
  const uint32_t n = (blockIdx.x - g * nb) * 256 + threadIdx.x, i = blockIdx.y;
  if (n >= C) return;
  uint32_t j, k;
  affine_column(a.shape, E, n, &j, &k);
  if (j >= E) return;  // padding column
  const bool is_k = n >= a.shape.g_tiles * 16u;
  if (i == D && !(is_k && j == D)) return;  // of row D only beta is kept
  double sum = 0.0;
  for (uint32_t sg = a.grp_seg_off[g]; sg < a.grp_seg_off[g + 1]; sg++) sum = sum + a.partial[((uint64_t)sg * a.shape.rows + i) * C + n];
  if (is_k) {
    if (i == D) a.out_beta[g] = sum;
    else a.out_k[((uint64_t)g * D + i) * E + j] = sum;
    return;
  }
  double* G = a.out_G + ((uint64_t)g * D + i) * E * E;
  G[(uint64_t)j * E + k] = sum;
  G[(uint64_t)k * E + j] = sum;
}

hipError_t launch_grouped_reduce(const GroupedStats& a, uint32_t dim, hipStream_t stream) {
  hipLaunchKernelGGL(grouped_reduce_kernel, dim3(a.n_groups * ((a.shape.cols + 255) / 256), dim + 1), dim3(256), 0, stream, a, dim);
  return hipGetLastError();
}

hipError_t launch_fmllr_statistics(const FmllrArgs& a, hipStream_t stream) {
  if (a.n_frames) {
    const uint64_t n = a.n_frames * a.g.shape.rows;
    hipLaunchKernelGGL(fmllr_fold_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, stream, a);
  }
  if (a.g.n_segs) {
    const hipError_t e = launch_contract<fmllr_contract_kernel<1>, fmllr_contract_kernel<2>, fmllr_contract_kernel<3>, fmllr_contract_kernel<4>>(
        a, a.g.shape.rows, a.g.n_segs, a.g.shape.g_tiles + a.g.shape.k_tiles, stream);
    if (e != hipSuccess) return e;
  }
  return launch_grouped_reduce(a.g, a.dim, stream);
}

// One workgroup per utterance: its speaker's W = [A b] in the LDS, a thread per (frame, row)
__global__ __launch_bounds__(256) void fmllr_transform_kernel(const float* feats, const uint64_t* frame_off, const uint32_t* utt_speaker,
                                                              const double* W, uint32_t D, float* out) {
  extern __shared__ double w[];  // [D][D + 1]
  const uint32_t u = blockIdx.x, E = D + 1;
  const double* Ws = W + (uint64_t)utt_speaker[u] * D * E;
  for (uint32_t e = threadIdx.x; e < D * E; e += 256) w[e] = Ws[e];
  __syncthreads();
  const uint64_t e0 = frame_off[u] * D, e1 = frame_off[u + 1] * D;
  for (uint64_t e = e0 + threadIdx.x; e < e1; e += 256) {
    const uint64_t t = e / D;
    const uint32_t i = (uint32_t)(e - t * D);
    out[e] = (float)affine_row(w + i * E, feats + t * D, D);
  }
}

hipError_t launch_fmllr_transform(const float* feats, const uint64_t* frame_off, uint32_t n_utts, const uint32_t* utt_speaker, const double* W,
                                  uint32_t dim, float* out, hipStream_t stream) {
  if (n_utts == 0) return hipSuccess;
  hipLaunchKernelGGL(fmllr_transform_kernel, dim3(n_utts), dim3(256), sizeof(double) * dim * (dim + 1), stream, feats, frame_off, utt_speaker,
                     W, dim, out);
  return hipGetLastError();
}

}  // namespace srgpu
