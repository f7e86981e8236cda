// mllr_stats.hip -- MLLR of the means (Leggetter & Woodland 1995): the statistics of a set of (frame, density, weight) pairs per
// (speaker, regression class), and a model's means under one transform per class.
//
// With xi_d = (mu_d1 .. mu_dD, 1) and iv = 1/var of density d, class r = dens_class[d], the group (s, r) collects
//   occ[s][d]  = sum_t gamma,   x_acc[s][d][i] = sum_t gamma x_ti                (the speaker's pairs of density d, frames ascending)
//   beta       = sum_d occ[s][d]
//   k[i][j]    = sum_d (iv_di x_acc[s][d][i]) xi_dj                              i < D, j <= D
//   G[i][j][k] = sum_d (occ[s][d] iv_di) xi_dj xi_dk                             i < D, j, k <= D
// over the densities d of class r, in ascending density id.  The pairs are em_assign_kernel's / em_assign_weighted_kernel's
// (em_accumulate.hip) with the density id beside them (EmArgs::pair_dens); a pair whose key is 0xFFFFFFFF was dropped there.
//
//   1. mllr_key_kernel       a pair's key = speaker * n_dens + density (dropped: 0xFFFFFFFF); a STABLE radix sort then keeps every
//                            key's pairs in generation (= frame) order, and a run-length encoding of the sorted keys names the occupied
//                            (speaker, density) "entries" -- em_accumulate.hip's scheme with the rows found by their runs, since a
//                            table of n_speakers * n_dens rows would mostly be empty.
//   2. mllr_group_key_kernel an entry's group = speaker * n_classes + class; a stable sort by it orders the entries by (speaker,
//                            class, density); mllr_bounds_kernel finds every group's first entry.
//   3. mllr_entry_kernel     one wave per entry, a lane per dimension: occ and x_acc, the entry's pairs one after the other.
//   4. mllr_contract_kernel  fmllr_contract_kernel's scheme (fmllr_stats.hip) with entries in the place of frames: rows i on the 16-row
//                            side of v_mfma_f64_16x16x4_f64 (occ iv_di for G, iv_di x_acc_i for k; row D of the k side is occ, so that
//                            its column D is beta), the columns (j <= k) and (j, D) on the other side, the products xi_dj xi_dk formed
//                            from the FP64 means when a block of entries is staged into the LDS.  A group's entries are cut into
//                            segments of fmllr_seg_frames(); a workgroup takes one segment and writes its partial sums.
//   5. mllr_reduce_kernel    one thread per (group, row, column): the partials of the group's segments added in ascending order; both
//                            triangles of G from the one sum.
// No atomics; every order of summation is fixed by the pairs and the segment length alone: two identical calls return identical bits.
//
//   mllr_means_kernel        mu'_di = acc, acc from b_i taking acc = acc + A_ij * mu_dj, j ascending, no contraction into FMAs.
#include <hip/hip_runtime.h>
#include <hipcub/hipcub.hpp>
#include <stdint.h>

#include <algorithm>

#include "kernels.h"

namespace srgpu {

#pragma clang fp contract(off)

static constexpr int kStageEntries = 32;  // entries staged in the LDS at a time
static constexpr int kWaves = 4;
static constexpr int kTilesPerWave = 2;   // column tiles whose accumulators a wave keeps
static constexpr int kTilesPerGroup = kWaves * kTilesPerWave;
static constexpr int kDensPerBlock = 64;  // densities a workgroup of mllr_means_kernel transforms

uint32_t mllr_dens_per_block() { return kDensPerBlock; }

__global__ __launch_bounds__(256) void mllr_key_kernel(MllrArgs a) {
  const uint64_t p = (uint64_t)blockIdx.x * 256 + threadIdx.x;
  if (p >= a.n_pairs) return;
  const bool kept = a.pair_key[p] != 0xFFFFFFFFu;
  a.key[p] = kept ? a.frame_speaker[a.pair_frame[p]] * a.n_dens + a.pair_dens[p] : 0xFFFFFFFFu;
  a.iota[p] = (uint32_t)p;
}

__global__ __launch_bounds__(256) void mllr_group_key_kernel(MllrArgs a) {
  const uint32_t e = blockIdx.x * 256 + threadIdx.x;
  if (e >= a.n_entries) return;
  const uint32_t key = a.run_key[e], s = key / a.n_dens;
  a.gkey[e] = s * a.n_classes + a.dens_class[key - s * a.n_dens];
  a.iota[e] = e;
}

// grp_begin[g] = first entry position whose group is >= g (g = 0 .. n_groups)
__global__ __launch_bounds__(256) void mllr_bounds_kernel(const uint32_t* sorted, uint32_t n, uint32_t n_groups, uint32_t* grp_begin) {
  const uint32_t g = blockIdx.x * 256 + threadIdx.x;
  if (g > n_groups) return;
  uint32_t lo = 0, hi = n;
  while (lo < hi) { const uint32_t mid = (lo + hi) >> 1; if (sorted[mid] < g) lo = mid + 1; else hi = mid; }
  grp_begin[g] = lo;
}

// one wave per entry position, lane i < D: x_acc[i]; every lane adds the same occ
__global__ __launch_bounds__(256) void mllr_entry_kernel(MllrArgs a) {
  const uint32_t D = a.dim, lane = threadIdx.x & 63u;
  const uint32_t q = blockIdx.x * 4u + (threadIdx.x >> 6);
  if (q >= a.n_entries) return;  // wave-uniform
  const uint32_t e = a.ent_order[q];
  const uint32_t p0 = a.run_begin[e], p1 = p0 + a.run_len[e];
  const float* col = a.feats + (lane < D ? lane : 0u);
  double occ = 0.0, sum = 0.0;
  for (uint32_t p = p0; p < p1; p++) {
    const uint32_t pr = a.pairs_sorted[p];
    const double w = a.pair_w[pr];
    sum = sum + w * (double)col[(uint64_t)a.pair_frame[pr] * D];
    occ = occ + w;
  }
  if (lane < D) a.ent_x[(uint64_t)q * D + lane] = sum;
  if (lane == 0) {
    const uint32_t key = a.run_key[e];
    a.ent_dens[q] = key - (key / a.n_dens) * a.n_dens;
    a.ent_occ[q] = occ;
  }
}

// fmllr_column (fmllr_stats.hip): column n of the contraction -> (j, k): n < g_cols: the n-th pair j <= k in row-major order of the upper
// triangle; beyond the G tiles: (j, D) of k; padding: (E, E), which reads the zero column of the staged entry
__device__ inline void mllr_column(const FmllrShape& s, uint32_t E, uint32_t n, uint32_t* j, uint32_t* k) {
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
__global__ __launch_bounds__(kWaves * 64) void mllr_contract_kernel(MllrArgs a) {
  constexpr int R = RT * 16;
  constexpr int kXs = 66;      // doubles per staged xi row: E <= 64 values, then zeros (column E is read by padding columns)
  constexpr int kAs = R + 2;   // doubles per staged row of either row-side operand
  __shared__ double xs[kStageEntries * kXs];
  __shared__ double as[kStageEntries * kAs];
  __shared__ double cs[kStageEntries * kAs];
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
    isk[q] = tile[q] >= a.shape.g_tiles;  // wave-uniform: a k tile takes iv x_acc on the row side
    mllr_column(a.shape, E, (live[q] ? tile[q] : 0u) * 16u + cc, &cj[q], &ck[q]);
  }
  typedef double d4 __attribute__((ext_vector_type(4)));
  d4 acc[kTilesPerWave][RT];
#pragma unroll
  for (int q = 0; q < kTilesPerWave; q++)
#pragma unroll
    for (int r = 0; r < RT; r++) acc[q][r] = d4{0.0, 0.0, 0.0, 0.0};

  for (uint32_t f0 = 0; f0 < sn; f0 += kStageEntries) {
    __syncthreads();  // the previous stage has been read
    for (uint32_t e = threadIdx.x; e < kStageEntries * kXs; e += kWaves * 64) {
      const uint32_t f = e / kXs, j = e - f * kXs;
      double v = 0.0;
      if (f0 + f < sn && j < E) v = j < D ? a.means[(uint64_t)a.ent_dens[s0 + f0 + f] * D + j] : 1.0;
      xs[e] = v;
    }
    for (uint32_t e = threadIdx.x; e < kStageEntries * R; e += kWaves * 64) {
      const uint32_t f = e / R, i = e - f * R;
      double va = 0.0, vc = 0.0;
      if (f0 + f < sn && i <= D) {
        const uint32_t q = s0 + f0 + f;
        const double occ = a.ent_occ[q];
        if (i == D) {
          vc = occ;
        } else {
          const double iv = a.inv_vars[(uint64_t)a.ent_dens[q] * D + i];
          va = occ * iv;
          vc = iv * a.ent_x[(uint64_t)q * D + i];
        }
      }
      as[f * kAs + i] = va;
      cs[f * kAs + i] = vc;
    }
    __syncthreads();
#pragma unroll 2
    for (uint32_t f = 0; f < kStageEntries; f += 4) {
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

// grid (groups x ceil(cols / 256), rows <= D)
__global__ __launch_bounds__(256) void mllr_reduce_kernel(MllrArgs a) {
  const uint32_t D = a.dim, E = D + 1, C = a.shape.cols;
  const uint32_t nb = (C + 255u) / 256u, g = blockIdx.x / nb;
  const uint32_t n = (blockIdx.x - g * nb) * 256 + threadIdx.x, i = blockIdx.y;
  if (n >= C) return;
  uint32_t j, k;
  mllr_column(a.shape, E, n, &j, &k);
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

size_t mllr_temp_bytes(uint64_t n_pairs) {
  size_t sort = 0, rle = 0, scan = 0;
  (void)hipcub::DeviceRadixSort::SortPairs(nullptr, sort, (const uint32_t*)nullptr, (uint32_t*)nullptr, (const uint32_t*)nullptr,
                                           (uint32_t*)nullptr, (int)n_pairs);
  (void)hipcub::DeviceRunLengthEncode::Encode(nullptr, rle, (const uint32_t*)nullptr, (uint32_t*)nullptr, (uint32_t*)nullptr,
                                              (uint32_t*)nullptr, (int)n_pairs);
  (void)hipcub::DeviceScan::ExclusiveSum(nullptr, scan, (const uint32_t*)nullptr, (uint32_t*)nullptr, (int)n_pairs);
  return std::max(sort, std::max(rle, scan));
}

hipError_t launch_mllr_runs(const MllrArgs& a, hipStream_t stream) {
  if (a.n_pairs == 0) return hipSuccess;
  hipLaunchKernelGGL(mllr_key_kernel, dim3((unsigned)((a.n_pairs + 255) / 256)), dim3(256), 0, stream, a);
  hipError_t e = hipGetLastError();
  if (e != hipSuccess) return e;
  size_t bytes = a.sort_temp_bytes;
  // LSD radix sort is stable: the pairs of one key stay in generation (= frame) order
  e = hipcub::DeviceRadixSort::SortPairs(a.sort_temp, bytes, a.key, a.keys_sorted, a.iota, a.pairs_sorted, (int)a.n_pairs, 0, 32, stream);
  if (e != hipSuccess) return e;
  bytes = a.sort_temp_bytes;
  return hipcub::DeviceRunLengthEncode::Encode(a.sort_temp, bytes, a.keys_sorted, a.run_key, a.run_len, a.n_runs, (int)a.n_pairs, stream);
}

hipError_t launch_mllr_groups(const MllrArgs& a, hipStream_t stream) {
  const uint32_t n_groups = a.n_speakers * a.n_classes;
  if (a.n_entries) {
    size_t bytes = a.sort_temp_bytes;
    hipError_t e = hipcub::DeviceScan::ExclusiveSum(a.sort_temp, bytes, a.run_len, a.run_begin, (int)a.n_entries, stream);
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(mllr_group_key_kernel, dim3((a.n_entries + 255) / 256), dim3(256), 0, stream, a);
    if ((e = hipGetLastError()) != hipSuccess) return e;
    bytes = a.sort_temp_bytes;
    e = hipcub::DeviceRadixSort::SortPairs(a.sort_temp, bytes, a.gkey, a.gkey_sorted, a.iota, a.ent_order, (int)a.n_entries, 0, 32, stream);
    if (e != hipSuccess) return e;
  }
  hipLaunchKernelGGL(mllr_bounds_kernel, dim3(n_groups / 256 + 1), dim3(256), 0, stream, a.gkey_sorted, a.n_entries, n_groups, a.grp_begin);
  return hipGetLastError();
}

hipError_t launch_mllr_statistics(const MllrArgs& a, hipStream_t stream) {
  if (a.n_entries) hipLaunchKernelGGL(mllr_entry_kernel, dim3((a.n_entries + 3) / 4), dim3(256), 0, stream, a);
  if (a.n_segs) {
    const uint32_t groups = (a.shape.g_tiles + a.shape.k_tiles + kTilesPerGroup - 1) / kTilesPerGroup;
    const dim3 grid(a.n_segs, groups), block(kWaves * 64);
    switch (a.shape.rows / 16) {
      case 1: hipLaunchKernelGGL((mllr_contract_kernel<1>), grid, block, 0, stream, a); break;
      case 2: hipLaunchKernelGGL((mllr_contract_kernel<2>), grid, block, 0, stream, a); break;
      case 3: hipLaunchKernelGGL((mllr_contract_kernel<3>), grid, block, 0, stream, a); break;
      case 4: hipLaunchKernelGGL((mllr_contract_kernel<4>), grid, block, 0, stream, a); break;
      default: return hipErrorInvalidValue;
    }
  }
  hipLaunchKernelGGL(mllr_reduce_kernel, dim3(a.n_speakers * a.n_classes * ((a.shape.cols + 255) / 256), a.dim + 1), dim3(256), 0, stream,
                     a);
  return hipGetLastError();
}

// One workgroup per block of at most kDensPerBlock densities of one class: the class's W = [A b] in the LDS, a thread per (density, row)
__global__ __launch_bounds__(256) void mllr_means_kernel(const double* means, const uint32_t* order, const uint32_t* blk, const double* W,
                                                         uint32_t D, double* out) {
  extern __shared__ double w[];  // [D][D + 1]
  const uint32_t E = D + 1;
  const uint32_t r = blk[3 * blockIdx.x], b0 = blk[3 * blockIdx.x + 1], b1 = blk[3 * blockIdx.x + 2];
  const double* Wr = W + (uint64_t)r * D * E;
  for (uint32_t e = threadIdx.x; e < D * E; e += 256) w[e] = Wr[e];
  __syncthreads();
  for (uint32_t e = threadIdx.x; e < (b1 - b0) * D; e += 256) {
    const uint32_t n = e / D, i = e - n * D;
    const uint64_t d = order[b0 + n];
    const double* mu = means + d * D;
    const double* wi = w + i * E;
    double acc = wi[D];
    for (uint32_t j = 0; j < D; j++) acc = acc + wi[j] * mu[j];
    out[d * D + i] = acc;
  }
}

hipError_t launch_mllr_transform_means(const double* means, const uint32_t* order, const uint32_t* blk, uint32_t n_blocks, const double* W,
                                       uint32_t dim, double* out, hipStream_t stream) {
  if (n_blocks == 0) return hipSuccess;
  hipLaunchKernelGGL(mllr_means_kernel, dim3(n_blocks), dim3(256), sizeof(double) * dim * (dim + 1), stream, means, order, blk, W, dim, out);
  return hipGetLastError();
}

}  // namespace srgpu
