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
//   1. mllt_contract_kernel  G[i][(j,k)] = sum_p (gamma iv_di) (z_j z_k): the shared symmetric contraction (sym_contract.h) with the pairs,
//                            in pair order (frames ascending), as the items: one row operand, gamma iv_di, plus row D that carries
//                            gamma alone; the columns (j <= k), plus one "ones" column whose row D is beta.  A stage first reads its
//                            pairs' weight, frame and density, then forms z in FP64 from them.
//   2. mllt_reduce_kernel    one thread per (row, column): the partials of a round's segments added in ascending order onto the running
//                            sum; writes both triangles of G from the one sum (exactly symmetric) and beta.
// The host runs the segments in rounds that fit the partials' workspace; a round's reduction continues the chain of additions where
// the round before stopped, so the bits do not depend on the workspace.  No atomics; the order of every sum is fixed by the pair
// order and the segment length alone, never by the grid: two identical calls return identical bits.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "kernels.h"
#include "sym_contract.h"

namespace srgpu {

#pragma clang fp contract(off)

uint32_t mllt_seg_pairs() { return kSegLen; }
uint32_t mllt_max_dim() { return 63; }

MlltShape mllt_shape(uint32_t dim) {
  MlltShape s{};
  s.rows = (dim + 1 + 15u) & ~15u;
  s.tri = dim * (dim + 1) / 2;
  s.tiles = (s.tri + 1 + 15u) / 16u;
  s.cols = s.tiles * 16u;
  return s;
}

// column n of the contraction -> (j, k): n < tri: tri_column; n == tri: (D, D), the staged 1; padding: (D + 1, D + 1), which reads the
// zero behind it
__device__ inline void mllt_column(uint32_t tri, uint32_t D, uint32_t n, uint32_t* j, uint32_t* k) {
  if (n >= tri) { *j = *k = n == tri ? D : D + 1; return; }
  tri_column(D, n, j, k);
}

// a stage of pairs: first the pairs themselves (weight, frame, density) into the LDS, then z = x - mu and a 1 on the column side,
// gamma iv and gamma on the row side
struct MlltStager {
  static constexpr bool kTwoRows = false, kPreStage = true;
  const MlltArgs& a;
  const uint64_t p0;  // the segment: pairs [p0, p0 + sn)
  const uint32_t sn;
  double* pw; uint32_t* pf; uint32_t* pd;  // LDS [kStage]
  __device__ void column(uint32_t n, uint32_t* j, uint32_t* k) const { mllt_column(a.shape.tri, a.dim, n, j, k); }
  __device__ void pre_stage(uint32_t f0) const {
    if (threadIdx.x >= kStage) return;
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
  __device__ double col(uint32_t, uint32_t f, uint32_t j) const {
    const uint32_t D = a.dim;
    if (pd[f] != 0xFFFFFFFFu && j <= D) return j < D ? (double)a.feats[(uint64_t)pf[f] * D + j] - a.means[(uint64_t)pd[f] * D + j] : 1.0;
    return 0.0;
  }
  __device__ void rows(uint32_t, uint32_t f, uint32_t i, double* v, double*) const {
    const uint32_t D = a.dim;
    if (pd[f] != 0xFFFFFFFFu && i <= D) *v = i < D ? pw[f] * a.inv_vars[(uint64_t)pd[f] * D + i] : pw[f];
  }
};

// grid (segments of the round, column-tile groups); RT = row tiles of 16
template <int RT>
__global__ __launch_bounds__(kWaves * 64) void mllt_contract_kernel(MlltArgs a) {
  __shared__ double pw[kStage];
  __shared__ uint32_t pf[kStage], pd[kStage];
  const uint32_t seg = blockIdx.x;
  const uint64_t p0 = (uint64_t)(a.seg0 + seg) * kSegLen;
  const uint32_t sn = (uint32_t)(a.n_pairs - p0 < (uint64_t)kSegLen ? a.n_pairs - p0 : (uint64_t)kSegLen);
  contract_segment<RT>(MlltStager{a, p0, sn, pw, pf, pd}, sn, a.shape.tiles, 0,
                       a.partial + (uint64_t)seg * a.shape.rows * a.shape.cols, a.shape.cols);
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
    const hipError_t e = launch_contract<mllt_contract_kernel<1>, mllt_contract_kernel<2>, mllt_contract_kernel<3>, mllt_contract_kernel<4>>(
        a, a.shape.rows, a.n_segs, a.shape.tiles, stream);
    if (e != hipSuccess) return e;
  }
  hipLaunchKernelGGL(mllt_reduce_kernel, dim3((a.shape.cols + 255) / 256, a.dim + 1), dim3(256), 0, stream, a);
  return hipGetLastError();
}

}  // namespace srgpu
