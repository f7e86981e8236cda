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
//   4. mllr_contract_kernel  the shared symmetric contraction (sym_contract.h) with a group's entries as the items: xi_d from the FP64 means
//                            on the column side; on the row side occ iv_di for G and iv_di x_acc_i for k (row D of the k side is occ, so
//                            that its column D is beta).  A group's entries are cut into segments of fmllr_seg_frames().
//   5. grouped_reduce_kernel (fmllr_stats.hip) the partials of a group's segments added in ascending order: G, k and beta.
// No atomics; every order of summation is fixed by the pairs and the segment length alone: two identical calls return identical bits.
//
//   mllr_means_kernel        mu'_di = acc, acc from b_i taking acc = acc + A_ij * mu_dj, j ascending, no contraction into FMAs.
#include <hip/hip_runtime.h>
#include <hipcub/hipcub.hpp>
#include <stdint.h>

#include <algorithm>

#include "kernels.h"
#include "sym_contract.h"

namespace srgpu {

#pragma clang fp contract(off)

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

// a stage of a group's entries: xi_d on the column side, occ iv and iv x_acc on the row side
struct MllrStager {
  static constexpr bool kTwoRows = true, kPreStage = false;
  const MllrArgs& a;
  const uint32_t s0, sn;  // the segment: entry positions [s0, s0 + sn)
  __device__ void column(uint32_t n, uint32_t* j, uint32_t* k) const { affine_column(a.g.shape, a.dim + 1, n, j, k); }
  __device__ double col(uint32_t f0, uint32_t f, uint32_t j) const {
    const uint32_t D = a.dim;
    if (f0 + f < sn && j <= D) return j < D ? a.means[(uint64_t)a.ent_dens[s0 + f0 + f] * D + j] : 1.0;
    return 0.0;
  }
  __device__ void rows(uint32_t f0, uint32_t f, uint32_t i, double* va, double* vc) const {
    const uint32_t D = a.dim;
    if (f0 + f >= sn || i > D) return;
    const uint32_t q = s0 + f0 + f;
    const double occ = a.ent_occ[q];
    if (i == D) {
      *vc = occ;
    } else {
      const double iv = a.inv_vars[(uint64_t)a.ent_dens[q] * D + i];
      *va = occ * iv;
      *vc = iv * a.ent_x[(uint64_t)q * D + i];
    }
  }
};

// grid (segments, column-tile groups); RT = row tiles of 16
template <int RT>
__global__ __launch_bounds__(kWaves * 64) void mllr_contract_kernel(MllrArgs a) {
  const uint32_t seg = blockIdx.x, sn = a.g.seg_len[seg];
  const FmllrShape& s = a.g.shape;
  contract_segment<RT>(MllrStager{a, a.g.seg_begin[seg], sn}, sn, s.g_tiles + s.k_tiles, s.g_tiles,
                       a.g.partial + (uint64_t)seg * s.rows * s.cols, s.cols);
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
  if (a.g.n_segs) {
    const hipError_t e = launch_contract<mllr_contract_kernel<1>, mllr_contract_kernel<2>, mllr_contract_kernel<3>, mllr_contract_kernel<4>>(
        a, a.g.shape.rows, a.g.n_segs, a.g.shape.g_tiles + a.g.shape.k_tiles, stream);
    if (e != hipSuccess) return e;
  }
  return launch_grouped_reduce(a.g, a.dim, stream);
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
    out[d * D + i] = affine_row(w + i * E, means + d * D, D);
  }
}

hipError_t launch_mllr_transform_means(const double* means, const uint32_t* order, const uint32_t* blk, uint32_t n_blocks, const double* W,
                                       uint32_t dim, double* out, hipStream_t stream) {
  if (n_blocks == 0) return hipSuccess;
  hipLaunchKernelGGL(mllr_means_kernel, dim3(n_blocks), dim3(256), sizeof(double) * dim * (dim + 1), stream, means, order, blk, W, dim, out);
  return hipGetLastError();
}

}  // namespace srgpu
