// mllt_stats.hip -- MLLT, the global semi-tied covariance transform (Gales 1999, one transform class): the statistics of a set of
// (frame, density, weight) pairs.
//
// With z = (double) x_t - mu_d and iv = 1/var of density d, the pairs (t, d, gamma) collect
//   beta       = sum gamma
//   G[i][j][k] = sum (gamma iv_di) z_j z_k                    i, j, k < D
// The features are centred on each density's own mean, so the density cannot be folded out of the sum per frame the way
// fmllr_fold_kernel does: the contraction runs over the pairs.  They are em_assign_kernel's / em_assign_weighted_kernel's
// (em_accumulate.hip) with the density id beside them (EmArgs::pair_dens) and the frame in EmArgs::pair_frame; a pair whose key is
// 0xFFFFFFFF was dropped there: it stays in its place with weight 0 and its density is not read.
//
//   1. mllt_contract_kernel  G[i][(j,k)] = sum_p (gamma iv_di) (z_j z_k) on v_mfma_f64_16x16x4_f64: rows i on the 16-row side, plus row D
//                            that carries gamma alone; the columns (j <= k) on the 16-column side, plus one "ones" column whose row D
//                            is beta; the pairs as K.  The pairs, in pair order (frames ascending), are cut into SEGMENTS of kSegPairs; a
//                            workgroup takes one segment and kWaves * kTilesPerWave column tiles, walks the segment kStagePairs at a
//                            time (z formed in FP64 when a block is staged into the LDS, the products z_j z_k in FP64 from there; one chain
//                            of MFMA accumulations per tile, pairs ascending) and writes the segment's partial sums.
//   2. mllt_reduce_kernel    one thread per (row, column): the partials of a round's segments added in ascending order onto the running
//                            sum; writes both triangles of G from the one sum (exactly symmetric) and beta.
// The host runs the segments in rounds that fit the partials' workspace; a round's reduction continues the chain of additions where
// the round before stopped, so the bits do not depend on the workspace.  No atomics; the order of every sum is fixed by the pair
// order and kSegPairs alone, never by the grid: two identical calls return identical bits.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "kernels.h"

namespace srgpu {

#pragma clang fp contract(off)

static constexpr int kSegPairs = 1024;   // pairs per segment (the unit of the fixed summation order)
static constexpr int kStagePairs = 32;   // pairs staged in the LDS at a time
static constexpr int kWaves = 4;
static constexpr int kTilesPerWave = 2;  // column tiles whose accumulators a wave keeps
static constexpr int kTilesPerGroup = kWaves * kTilesPerWave;

uint32_t mllt_seg_pairs() { return kSegPairs; }
uint32_t mllt_max_dim() { return 63; }

MlltShape mllt_shape(uint32_t dim) {
  MlltShape s{};
  s.rows = (dim + 1 + 15u) & ~15u;
  s.tri = dim * (dim + 1) / 2;
  s.tiles = (s.tri + 1 + 15u) / 16u;
  s.cols = s.tiles * 16u;
  return s;
}

// column n of the contraction -> (j, k): n < tri: the n-th pair j <= k in row-major order of the upper triangle; n == tri: (D, D), the
// staged 1; padding: (D + 1, D + 1), which reads the zero behind it
__device__ inline void mllt_column(uint32_t tri, uint32_t D, uint32_t n, uint32_t* j, uint32_t* k) {
  if (n >= tri) { *j = *k = n == tri ? D : D + 1; return; }
  uint32_t r = 0, left = n;
  while (left >= D - r) { left -= D - r; r++; }  // row r of the triangle holds D - r columns
  *j = r;
  *k = r + left;
}

// grid (segments of the round, column-tile groups); RT = row tiles of 16
template <int RT>
__global__ __launch_bounds__(kWaves * 64) void mllt_contract_kernel(MlltArgs a) {
  constexpr int R = RT * 16;
  constexpr int kZs = 66;      // doubles per staged z row: D <= 63 values, a 1, then zeros (column D + 1 is read by padding columns)
  constexpr int kWs = R + 2;   // doubles per staged weight row
  __shared__ double zs[kStagePairs * kZs];
  __shared__ double ws[kStagePairs * kWs];
  __shared__ double pw[kStagePairs];
  __shared__ uint32_t pf[kStagePairs], pd[kStagePairs];
  const uint32_t D = a.dim;
  const uint32_t seg = blockIdx.x;
  const uint64_t p0 = (uint64_t)(a.seg0 + seg) * kSegPairs;
  const uint32_t sn = (uint32_t)(a.n_pairs - p0 < (uint64_t)kSegPairs ? a.n_pairs - p0 : (uint64_t)kSegPairs);
  const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
  const uint32_t kk = lane >> 4, cc = lane & 15u;
  uint32_t tile[kTilesPerWave], cj[kTilesPerWave], ck[kTilesPerWave];
  bool live[kTilesPerWave];
#pragma unroll
  for (int q = 0; q < kTilesPerWave; q++) {
    tile[q] = blockIdx.y * kTilesPerGroup + wave * kTilesPerWave + q;
    live[q] = tile[q] < a.shape.tiles;  // wave-uniform
    mllt_column(a.shape.tri, D, (live[q] ? tile[q] : 0u) * 16u + cc, &cj[q], &ck[q]);
  }
  typedef double d4 __attribute__((ext_vector_type(4)));
  d4 acc[kTilesPerWave][RT];
#pragma unroll
  for (int q = 0; q < kTilesPerWave; q++)
#pragma unroll
    for (int r = 0; r < RT; r++) acc[q][r] = d4{0.0, 0.0, 0.0, 0.0};

  for (uint32_t f0 = 0; f0 < sn; f0 += kStagePairs) {
    __syncthreads();  // the previous stage has been read
    if (threadIdx.x < kStagePairs) {
      const uint32_t f = threadIdx.x;
      double w = 0.0;
      uint32_t fr = 0, de = 0xFFFFFFFFu;  // no density: a dropped pair keeps its place with weight 0 and z = 0
      if (f0 + f < sn && a.pair_key[p0 + f0 + f] != 0xFFFFFFFFu) {
        w = a.pair_w[p0 + f0 + f];
        fr = a.pair_frame[p0 + f0 + f];
        de = a.pair_dens[p0 + f0 + f];
      }
      pw[f] = w; pf[f] = fr; pd[f] = de;
    }
    __syncthreads();
    for (uint32_t e = threadIdx.x; e < kStagePairs * kZs; e += kWaves * 64) {
      const uint32_t f = e / kZs, j = e - f * kZs;
      double v = 0.0;
      if (pd[f] != 0xFFFFFFFFu && j <= D)
        v = j < D ? (double)a.feats[(uint64_t)pf[f] * D + j] - a.means[(uint64_t)pd[f] * D + j] : 1.0;
      zs[e] = v;
    }
    for (uint32_t e = threadIdx.x; e < kStagePairs * R; e += kWaves * 64) {
      const uint32_t f = e / R, i = e - f * R;
      double v = 0.0;
      if (pd[f] != 0xFFFFFFFFu && i <= D) v = i < D ? pw[f] * a.inv_vars[(uint64_t)pd[f] * D + i] : pw[f];
      ws[f * kWs + i] = v;
    }
    __syncthreads();
#pragma unroll 2
    for (uint32_t f = 0; f < kStagePairs; f += 4) {
      const double* zr = zs + (f + kk) * kZs;
#pragma unroll
      for (int q = 0; q < kTilesPerWave; q++) {
        if (!live[q]) continue;
        const double b = zr[cj[q]] * zr[ck[q]];
        const double* wr = ws + (f + kk) * kWs + cc;
#pragma unroll
        for (int r = 0; r < RT; r++) acc[q][r] = __builtin_amdgcn_mfma_f64_16x16x4f64(wr[r * 16], b, acc[q][r], 0, 0, 0);
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

// grid (ceil(cols / 256), rows <= D)
__global__ __launch_bounds__(256) void mllt_reduce_kernel(MlltArgs a) {
  const uint32_t D = a.dim, C = a.shape.cols, tri = a.shape.tri;
  const uint32_t n = blockIdx.x * 256 + threadIdx.x, i = blockIdx.y;
  if (n > tri) return;                   // padding column
  if ((i == D) != (n == tri)) return;    // of row D only beta is kept, of the ones column only row D
  uint32_t j, k;
  mllt_column(tri, D, n, &j, &k);
  double* dst = i == D ? a.out_beta : a.out_G + ((uint64_t)i * D + j) * D + k;
  double sum = a.seg0 ? *dst : 0.0;
  for (uint32_t g = 0; g < a.n_segs; g++) sum = sum + a.partial[((uint64_t)g * a.shape.rows + i) * C + n];
  *dst = sum;
  if (i < D) a.out_G[((uint64_t)i * D + k) * D + j] = sum;
}

hipError_t launch_mllt_round(const MlltArgs& a, hipStream_t stream) {
  if (a.n_segs) {
    const uint32_t groups = (a.shape.tiles + kTilesPerGroup - 1) / kTilesPerGroup;
    const dim3 grid(a.n_segs, groups), block(kWaves * 64);
    switch (a.shape.rows / 16) {
      case 1: hipLaunchKernelGGL((mllt_contract_kernel<1>), grid, block, 0, stream, a); break;
      case 2: hipLaunchKernelGGL((mllt_contract_kernel<2>), grid, block, 0, stream, a); break;
      case 3: hipLaunchKernelGGL((mllt_contract_kernel<3>), grid, block, 0, stream, a); break;
      case 4: hipLaunchKernelGGL((mllt_contract_kernel<4>), grid, block, 0, stream, a); break;
      default: return hipErrorInvalidValue;
    }
  }
  hipLaunchKernelGGL(mllt_reduce_kernel, dim3((a.shape.cols + 255) / 256, a.dim + 1), dim3(256), 0, stream, a);
  return hipGetLastError();
}

}  // namespace srgpu
