// sym_contract.h -- the symmetric FP64 contraction that the fMLLR, MLLR and MLLT statistics share (fmllr_stats.hip, mllr_stats.hip,
// mllt_stats.hip), device side.
//
//   P[i][(j,k)] = sum_f row_f[i] (x_f[j] x_f[k])        on v_mfma_f64_16x16x4_f64
// rows i on the 16-row side, the columns (j <= k) of the upper triangle on the 16-column side, the items f (frames, entries, pairs) as
// K.  The items of one sum, in their fixed order, are cut into SEGMENTS of kSegLen; a workgroup takes one segment and kTilesPerGroup
// column tiles, walks the segment kStage items at a time (one chain of MFMA accumulations per tile, items ascending) and writes the
// segment's partial sums; a reduction then adds the segments' partials in ascending order and writes both triangles from the one sum.
// No atomics; the order of every sum is fixed by the item order and kSegLen alone, never by the grid: two identical calls return
// identical bits.  The products x_f[j] x_f[k] are formed in FP64, and rounded, from the staged row before the matrix instruction adds
// them (the including files are built without contraction into FMAs).
//
// A statistic supplies a STAGER: what one stage puts into the LDS, and which (j, k) a column stands for.
//   static constexpr bool kTwoRows    a second row operand: the column tiles from second_from on take it (fMLLR / MLLR: the k tiles)
//   static constexpr bool kPreStage   pre_stage(f0) runs, with a barrier behind it, before a stage's operands are formed
//   void column(n, &j, &k)            column n of the contraction; a padding column names an index whose staged value is 0
//   double col(f0, f, j)              x_f[j] of item f0 + f of the segment, j < kColStride (0 beyond the segment and the operand)
//   void rows(f0, f, i, &r1, &r2)     the row operands of item f0 + f, row i (r2 is dropped without kTwoRows)
// Barriers, accumulators, the MFMA loop and the epilogue are contract_segment's.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "kernels.h"

namespace srgpu {

#pragma clang fp contract(off)

static constexpr int kSegLen = 1024;     // items per segment (the unit of the fixed summation order)
static constexpr int kStage = 32;        // items staged in the LDS at a time
static constexpr int kWaves = 4;
static constexpr int kTilesPerWave = 2;  // column tiles whose accumulators a wave keeps
static constexpr int kTilesPerGroup = kWaves * kTilesPerWave;
static constexpr int kColStride = 66;    // doubles per staged column-side row: at most 64 values, then zeros (read by padding columns)

// the n-th pair j <= k, in row-major order, of the upper triangle of an n_elems x n_elems matrix
__device__ inline void tri_column(uint32_t n_elems, uint32_t n, uint32_t* j, uint32_t* k) {
  uint32_t r = 0, left = n;
  while (left >= n_elems - r) { left -= n_elems - r; r++; }  // row r of the triangle holds n_elems - r columns
  *j = r;
  *k = r + left;
}

// column n of fmllr_shape's contraction -> (j, k): n < g_cols: tri_column; beyond the G tiles: (j, D) of k; padding: (E, E), which
// reads the zero column of the staged item
__device__ inline void affine_column(const FmllrShape& s, uint32_t E, uint32_t n, uint32_t* j, uint32_t* k) {
  if (n >= s.g_tiles * 16u) {
    const uint32_t c = n - s.g_tiles * 16u;
    *j = c < E ? c : E;
    *k = c < E ? E - 1 : E;
    return;
  }
  if (n >= s.g_cols) { *j = E; *k = E; return; }
  tri_column(E, n, j, k);
}

// One segment of sn items and this workgroup's column tiles (blockIdx.y) of n_tiles; out = the segment's partial[row][column], C
// columns a row.  RT = row tiles of 16.
template <int RT, class Stager>
__device__ __forceinline__ void contract_segment(Stager st, uint32_t sn, uint32_t n_tiles, uint32_t second_from, double* out, uint32_t C) {
  constexpr int R = RT * 16;
  constexpr int kRs = R + 2;  // doubles per staged row of either row-side operand
  __shared__ double xs[kStage * kColStride];
  __shared__ double rs[(Stager::kTwoRows ? 2 : 1) * kStage * kRs];
  double* const r2s = rs + kStage * kRs;  // the second row operand, with kTwoRows
  const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
  const uint32_t kk = lane >> 4, cc = lane & 15u;
  uint32_t tile[kTilesPerWave], cj[kTilesPerWave], ck[kTilesPerWave];
  bool live[kTilesPerWave], second[kTilesPerWave];
#pragma unroll
  for (int q = 0; q < kTilesPerWave; q++) {
    tile[q] = blockIdx.y * kTilesPerGroup + wave * kTilesPerWave + q;
    live[q] = tile[q] < n_tiles;                               // wave-uniform
    second[q] = Stager::kTwoRows && tile[q] >= second_from;   // wave-uniform
    st.column((live[q] ? tile[q] : 0u) * 16u + cc, &cj[q], &ck[q]);
  }
  typedef double d4 __attribute__((ext_vector_type(4)));
  d4 acc[kTilesPerWave][RT];
#pragma unroll
  for (int q = 0; q < kTilesPerWave; q++)
#pragma unroll
    for (int r = 0; r < RT; r++) acc[q][r] = d4{0.0, 0.0, 0.0, 0.0};

  for (uint32_t f0 = 0; f0 < sn; f0 += kStage) {
    __syncthreads();  // the previous stage has been read
    if constexpr (Stager::kPreStage) {
      st.pre_stage(f0);
      __syncthreads();
    }
    for (uint32_t e = threadIdx.x; e < kStage * kColStride; e += kWaves * 64) {
      const uint32_t f = e / kColStride, j = e - f * kColStride;
      xs[e] = st.col(f0, f, j);
    }
    for (uint32_t e = threadIdx.x; e < kStage * R; e += kWaves * 64) {
      const uint32_t f = e / R, i = e - f * R;
      double r1 = 0.0, r2 = 0.0;
      st.rows(f0, f, i, &r1, &r2);
      rs[f * kRs + i] = r1;
      if constexpr (Stager::kTwoRows) r2s[f * kRs + i] = r2;
    }
    __syncthreads();
#pragma unroll 2
    for (uint32_t f = 0; f < kStage; f += 4) {
      const double* xr = xs + (f + kk) * kColStride;
#pragma unroll
      for (int q = 0; q < kTilesPerWave; q++) {
        if (!live[q]) continue;
        const double b = xr[cj[q]] * xr[ck[q]];
        const double* ar = (second[q] ? r2s : rs) + (f + kk) * kRs + cc;
#pragma unroll
        for (int r = 0; r < RT; r++) acc[q][r] = __builtin_amdgcn_mfma_f64_16x16x4f64(ar[r * 16], b, acc[q][r], 0, 0, 0);
      }
    }
  }
  // partial[seg][row][column]: the result's row of register v is kk + 4 v, its column cc
#pragma unroll
  for (int q = 0; q < kTilesPerWave; q++) {
    if (!live[q]) continue;
#pragma unroll
    for (int r = 0; r < RT; r++)
#pragma unroll
      for (int v = 0; v < 4; v++) out[(uint64_t)(r * 16 + kk + 4 * v) * C + tile[q] * 16u + cc] = acc[q][r][v];
  }
}

// Kernel = the contraction's instantiations for 1, 2, .. row tiles; grid (segments, column-tile groups)
template <auto... Kernel, class Args>
hipError_t launch_contract(const Args& a, uint32_t rows, uint32_t n_segs, uint32_t n_tiles, hipStream_t stream) {
  void (*const kernel[])(Args) = {Kernel...};
  const uint32_t rt = rows / 16;
  if (rt < 1 || rt > sizeof...(Kernel)) return hipErrorInvalidValue;
  hipLaunchKernelGGL(kernel[rt - 1], dim3(n_segs, (n_tiles + kTilesPerGroup - 1) / kTilesPerGroup), dim3(kWaves * 64), 0, stream, a);
  return hipGetLastError();
}

// One row of an affine transform W = [A b] ([D + 1] doubles, the LDS): acc = w[D]; acc = acc + w[j] * x[j], j ascending, no contraction
// into FMAs: the order of operations is the specification (sr_corpus_transform, sr_model_transform_means)
template <class T>
__device__ inline double affine_row(const double* w, const T* x, uint32_t D) {
  double acc = w[D];
  for (uint32_t j = 0; j < D; j++) acc = acc + w[j] * (double)x[j];
  return acc;
}

}  // namespace srgpu
