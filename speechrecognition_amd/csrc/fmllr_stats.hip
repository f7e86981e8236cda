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
//   2. fmllr_contract_kernel G[i][(j,k)] = sum_t a_t[i] (xi_tj xi_tk) on v_mfma_f64_16x16x4_f64: rows i on the 16-row side, the columns
//                            (j <= k) on the 16-column side, frames as K.  k is the same contraction with c_t and the columns (j, D):
//                            xi_tD = 1, so its row D, column D is beta.  The products xi_tj xi_tk are formed in FP64 from the float
//                            features when a frame block is staged into the LDS.
//      A speaker's frames, in corpus order, are cut into SEGMENTS of kSegFrames; a workgroup takes one segment and kWaves * kTilesPerWave
//      column tiles, walks the segment kStageFrames at a time (one chain of MFMA accumulations per tile, frames ascending) and writes
//      the segment's partial sums.
//   3. fmllr_reduce_kernel   one thread per (speaker, row, column): the partials of the speaker's segments added in ascending order;
//                            writes both triangles of G from the one sum (exactly symmetric), k and beta.
// No atomics; the order of every sum is fixed by the frame lists and kSegFrames alone, never by the grid: two identical calls return
// identical bits.
//
//   fmllr_transform_kernel   y_ti = (float)(b_i + sum_j A_ij (double) x_tj), j ascending, no contraction into FMAs: the order of operations
//                            is the specification.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "kernels.h"

namespace srgpu {

#pragma clang fp contract(off)

static constexpr int kSegFrames = 1024;   // frames per segment (the unit of the fixed summation order)
static constexpr int kStageFrames = 32;   // frames staged in the LDS at a time
static constexpr int kWaves = 4;
static constexpr int kTilesPerWave = 2;   // column tiles whose accumulators a wave keeps
static constexpr int kTilesPerGroup = kWaves * kTilesPerWave;

uint32_t fmllr_seg_frames() { return kSegFrames; }
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
  const uint32_t R = a.shape.rows, D = a.dim;
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

// column n of the contraction -> (j, k): n < g_cols: the n-th pair j <= k in row-major order of the upper triangle; beyond the G tiles:
// (j, D) of k; padding: (E, E), which reads the zero column of the staged frame
__device__ inline void fmllr_column(const FmllrShape& s, uint32_t E, uint32_t n, uint32_t* j, uint32_t* k) {
  if (n >= s.g_tiles * 16u) {
    const uint32_t c = n - s.g_tiles * 16u;
    *j = c < E ? c : E;
    *k = c < E ? E - 1 : E;
    return;
  }
  if (n >= s.g_cols) { *j = E; *k = E; return; }
  uint32_t r = 0, left = n;
  while (left >= E - r) { left -= E - r; r++; }  // row r of the triangle holds E - r columns
  *j = r;
  *k = r + left;
}

// grid (segments, column-tile groups); RT = row tiles of 16
template <int RT>
__global__ __launch_bounds__(kWaves * 64) void fmllr_contract_kernel(FmllrArgs a) {
  constexpr int R = RT * 16;
  constexpr int kXs = 66;      // doubles per staged xi row: E <= 64 values, then zeros (column E is read by padding columns)
  constexpr int kAs = R + 2;   // doubles per staged a / c row
  __shared__ double xs[kStageFrames * kXs];
  __shared__ double as[kStageFrames * kAs];
  __shared__ double cs[kStageFrames * kAs];
  const uint32_t D = a.dim, E = D + 1;
  const uint32_t seg = blockIdx.x;
  const uint32_t s0 = a.seg_begin[seg], sn = a.seg_len[seg];
  const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
  const uint32_t kk = lane >> 4, cc = lane & 15u;
  const uint32_t n_tiles = a.shape.g_tiles + a.shape.k_tiles;
  uint32_t tile[kTilesPerWave], cj[kTilesPerWave], ck[kTilesPerWave];
  bool live[kTilesPerWave], isk[kTilesPerWave];
#pragma unroll
  for (int q = 0; q < kTilesPerWave; q++) {
    tile[q] = blockIdx.y * kTilesPerGroup + wave * kTilesPerWave + q;
    live[q] = tile[q] < n_tiles;          // wave-uniform
    isk[q] = tile[q] >= a.shape.g_tiles;  // wave-uniform: a k tile takes c_t on the row side
    fmllr_column(a.shape, E, (live[q] ? tile[q] : 0u) * 16u + cc, &cj[q], &ck[q]);
  }
  typedef double d4 __attribute__((ext_vector_type(4)));
  d4 acc[kTilesPerWave][RT];
#pragma unroll
  for (int q = 0; q < kTilesPerWave; q++)
#pragma unroll
    for (int r = 0; r < RT; r++) acc[q][r] = d4{0.0, 0.0, 0.0, 0.0};

  for (uint32_t f0 = 0; f0 < sn; f0 += kStageFrames) {
    __syncthreads();  // the previous stage has been read
    for (uint32_t e = threadIdx.x; e < kStageFrames * kXs; e += kWaves * 64) {
      const uint32_t f = e / kXs, j = e - f * kXs;
      double v = 0.0;
      if (f0 + f < sn && j < E) v = j < D ? (double)a.feats[(uint64_t)a.frame_list[s0 + f0 + f] * D + j] : 1.0;
      xs[e] = v;
    }
    for (uint32_t e = threadIdx.x; e < kStageFrames * R; e += kWaves * 64) {
      const uint32_t f = e / R, i = e - f * R;
      double va = 0.0, vc = 0.0;
      if (f0 + f < sn) {
        const uint64_t o = (uint64_t)a.frame_list[s0 + f0 + f] * R + i;
        va = a.fold_a[o];
        vc = a.fold_c[o];
      }
      as[f * kAs + i] = va;
      cs[f * kAs + i] = vc;
    }
    __syncthreads();
#pragma unroll 2
    for (uint32_t f = 0; f < kStageFrames; f += 4) {
      const double* xr = xs + (f + kk) * kXs;
#pragma unroll
      for (int q = 0; q < kTilesPerWave; q++) {
        if (!live[q]) continue;
        const double b = xr[cj[q]] * xr[ck[q]];
        const double* ar = (isk[q] ? cs : as) + (f + kk) * kAs + cc;
#pragma unroll
        for (int r = 0; r < RT; r++) acc[q][r] = __builtin_amdgcn_mfma_f64_16x16x4f64(ar[r * 16], b, acc[q][r], 0, 0, 0);
      }
    }
  }
  // partial[seg][row][column]: the result's row of register v is kk + 4 v, its column cc
  const uint32_t C = a.shape.cols;
  double* out = a.partial + (uint64_t)seg * a.shape.rows * C;
#pragma unroll
  for (int q = 0; q < kTilesPerWave; q++) {
    if (!live[q]) continue;
#pragma unroll
    for (int r = 0; r < RT; r++)
#pragma unroll
      for (int v = 0; v < 4; v++) out[(uint64_t)(r * 16 + kk + 4 * v) * C + tile[q] * 16u + cc] = acc[q][r][v];
  }
}

// grid (speakers x ceil(cols / 256), rows <= D)
__global__ __launch_bounds__(256) void fmllr_reduce_kernel(FmllrArgs a) {
  const uint32_t D = a.dim, E = D + 1, C = a.shape.cols;
  const uint32_t nb = (C + 255u) / 256u, s = blockIdx.x / nb;
  const uint32_t n = (blockIdx.x - s * nb) * 256 + threadIdx.x, i = blockIdx.y;
  if (n >= C) return;
  uint32_t j, k;
  fmllr_column(a.shape, E, n, &j, &k);
  if (j >= E) return;  // padding column
  const bool is_k = n >= a.shape.g_tiles * 16u;
  if (i == D && !(is_k && j == D)) return;  // of row D only beta is kept
  double sum = 0.0;
  for (uint32_t g = a.spk_seg_off[s]; g < a.spk_seg_off[s + 1]; g++) sum = sum + a.partial[((uint64_t)g * a.shape.rows + i) * C + n];
  if (is_k) {
    if (i == D) a.out_beta[s] = sum;
    else a.out_k[((uint64_t)s * D + i) * E + j] = sum;
    return;
  }
  double* G = a.out_G + ((uint64_t)s * D + i) * E * E;
  G[(uint64_t)j * E + k] = sum;
  G[(uint64_t)k * E + j] = sum;
}

hipError_t launch_fmllr_statistics(const FmllrArgs& a, hipStream_t stream) {
  if (a.n_frames) {
    const uint64_t n = a.n_frames * a.shape.rows;
    hipLaunchKernelGGL(fmllr_fold_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, stream, a);
  }
  if (a.n_segs) {
    const uint32_t groups = (a.shape.g_tiles + a.shape.k_tiles + kTilesPerGroup - 1) / kTilesPerGroup;
    const dim3 grid(a.n_segs, groups), block(kWaves * 64);
    switch (a.shape.rows / 16) {
      case 1: hipLaunchKernelGGL((fmllr_contract_kernel<1>), grid, block, 0, stream, a); break;
      case 2: hipLaunchKernelGGL((fmllr_contract_kernel<2>), grid, block, 0, stream, a); break;
      case 3: hipLaunchKernelGGL((fmllr_contract_kernel<3>), grid, block, 0, stream, a); break;
      case 4: hipLaunchKernelGGL((fmllr_contract_kernel<4>), grid, block, 0, stream, a); break;
      default: return hipErrorInvalidValue;
    }
  }
  hipLaunchKernelGGL(fmllr_reduce_kernel, dim3(a.n_speakers * ((a.shape.cols + 255) / 256), a.dim + 1), dim3(256), 0, stream, a);
  return hipGetLastError();
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
    const float* x = feats + t * D;
    const double* wi = w + i * E;
    double acc = wi[D];
    for (uint32_t j = 0; j < D; j++) acc = acc + wi[j] * (double)x[j];
    out[e] = (float)acc;
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
