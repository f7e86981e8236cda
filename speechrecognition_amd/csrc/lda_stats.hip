// lda_stats.hip -- LDA with frame splicing: the statistics of the spliced frames and the projected corpus.
//
// The spliced vector of frame t, whose utterance holds the frames [a, b), stacks the frame with its c neighbours on either side, edge
// frames repeated:   z_t[(o + c) D + j] = (double) x[min(max(t + o, a), b - 1)][j],   o = -c .. c, j < D;   E = (2c + 1) D.
// It is never stored: every kernel gathers it from the float corpus while staging into the LDS (a corpus row is read 2c + 1 times,
// from cache).  The items are the kept frames (a class other than SR_LDA_SKIP), in corpus order.
//
//   1. lda_scatter_kernel     S[j][k] = sum_items z_j z_k on v_mfma_f64_16x16x4_f64: a symmetric rank-k update.  The E columns are cut
//                             into panels of kBlock = 64; a workgroup takes one segment of kSegLen items and one block (I <= J) of the
//                             upper triangle, stages kStage items of the two panels I and J at a time (one panel for a diagonal block:
//                             both operands are the same) and keeps a 2 x 2 set of 16 x 16 tiles per wave.  A stage's gathers are
//                             issued one stage ahead, into registers, so that they land under the matrix instructions.  One chain of accumulations
//                             per output, items ascending.  Both operands are floats widened to double: every product is exact, the
//                             only roundings are the additions'.
//   2. lda_reduce_kernel      one thread per (j <= k): the partials of a round's segments added in ascending order onto the running
//                             sum; writes both triangles from the one sum (exactly symmetric).
//   3. lda_class_sum_kernel   one workgroup per segment of a class' items (grouped stably by class on the host), a thread per column,
//                             plain FP64 additions, items ascending; lda_class_reduce_kernel adds a class' segments, ascending.
//   4. lda_project_kernel     out[t][i] = (float) acc, acc = M[i][E], then acc = acc + M[i][n] * z_t[n] for n ascending, no contraction
//                             into FMAs: the loop is the specification.  A tile of kRows rows of M (blockIdx.y) and the spliced rows
//                             of a group of kFrames frames pass through the LDS, kChunk columns at a time; a thread keeps one row of
//                             M against four frames.
// The host runs the scatter's segments in rounds that fit the partials' workspace; a round's reduction continues the chain of
// additions where the round before stopped, so the bits do not depend on the workspace.  No atomics; the order of every sum is fixed
// by the item order and the segment length alone, never by the grid: two identical calls return identical bits.
//
// LDS layout of a staged panel: [item][64 columns], column n of item f at f * 64 + (n ^ ((f & 1) << 4)).  An operand read takes, per
// 32-lane half, 16 consecutive doubles of item f and 16 of item f + 1; with rows of 64 doubles (128 dwords = 0 mod the 64 banks an
// 8-byte read sees) those would fall on the same banks, and the exchange of the two 16-column halves of every odd item moves them 32
// banks apart: conflict-free without padding.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "kernels.h"
#include "splice_clamp.h"

namespace srgpu {

#pragma clang fp contract(off)

static constexpr int kSegLen = 1024;  // items per segment (the unit of the fixed summation order)
static constexpr int kStage = 32;     // items staged in the LDS at a time
static constexpr int kBlock = 64;     // columns per panel: a workgroup's output block is kBlock x kBlock
static constexpr int kMaxE = 512;
static constexpr int kRows = 16;      // the projection: rows of M per workgroup ...
static constexpr int kFrames = 64;    // ... frames per frame group (one per workgroup) ...
static constexpr int kChunk = 128;    // ... and columns of M's tile and of the spliced rows in the LDS at a time

uint32_t lda_seg_items() { return kSegLen; }
uint32_t lda_max_e() { return kMaxE; }
uint32_t lda_block() { return kBlock; }

// x[clamp(t + o - c)][j] of frame t, whose utterance is [lo, hi)
__device__ inline float lda_splice(const float* feats, uint32_t D, uint32_t c, uint32_t t, uint32_t lo, uint32_t hi, uint32_t o, uint32_t j) {
  return feats[(uint64_t)srplan::splice_frame(t, o, c, lo, hi) * D + j];
}

// grid (segments of the round, blocks I <= J)
__global__ __launch_bounds__(256) void lda_scatter_kernel(LdaArgs a) {
  __shared__ double pa[kStage * kBlock], pb[kStage * kBlock];
  const uint32_t E = a.E, D = a.dim, nP = (E + kBlock - 1) / kBlock;
  uint32_t I = 0, J = blockIdx.y;
  while (J >= nP - I) { J -= nP - I; I++; }
  J += I;
  const bool diag = I == J;
  const uint64_t p0 = (uint64_t)(a.seg0 + blockIdx.x) * kSegLen;
  const uint32_t sn = (uint32_t)(a.n_items - p0 < (uint64_t)kSegLen ? a.n_items - p0 : (uint64_t)kSegLen);
  const uint32_t col = threadIdx.x & 63u, wave = threadIdx.x >> 6, kk = (threadIdx.x >> 4) & 3u, cc = threadIdx.x & 15u;
  // staging: this thread's column of either panel, items wave, wave + 4, ..
  const uint32_t nA = I * kBlock + col, nB = J * kBlock + col;
  const bool hasA = nA < E, hasB = !diag && nB < E;
  const uint32_t oA = hasA ? nA / D : 0, jA = hasA ? nA - oA * D : 0, oB = hasB ? nB / D : 0, jB = hasB ? nB - oB * D : 0;
  // the MFMA side: row tiles rt0, rt0 + 1 of panel I against column tiles ct0, ct0 + 1 of panel J
  const uint32_t rt0 = (wave >> 1) * 2, ct0 = (wave & 1u) * 2;
  bool live[2][2];  // wave-uniform: inside E, and on a diagonal block not below the diagonal (never read)
#pragma unroll
  for (int r = 0; r < 2; r++)
#pragma unroll
    for (int q = 0; q < 2; q++)
      live[r][q] = I * kBlock + (rt0 + r) * 16 < E && J * kBlock + (ct0 + q) * 16 < E && !(diag && rt0 + r > ct0 + q);
  typedef double d4 __attribute__((ext_vector_type(4)));
  d4 acc[2][2];
#pragma unroll
  for (int r = 0; r < 2; r++)
#pragma unroll
    for (int q = 0; q < 2; q++) acc[r][q] = d4{0.0, 0.0, 0.0, 0.0};
  const double* const pbr = diag ? pa : pb;
  const uint32_t sw = (kk & 1u) << 4;  // items f + kk with f a multiple of 4: odd exactly when kk is

  // a stage's values travel through registers: the gathers of stage f0 + kStage are issued before the matrix instructions of stage f0
  // and land while those run
  float ra[kStage / 4], rb[kStage / 4];
  auto gather = [&](uint32_t f0) {
#pragma unroll
    for (uint32_t i = 0; i < kStage / 4; i++) {
      const uint32_t f = wave + 4 * i;
      ra[i] = rb[i] = 0.f;
      if (f0 + f < sn) {
        const uint32_t* it = a.items + 3 * (p0 + f0 + f);
        const uint32_t t = it[0], lo = it[1], hi = it[2];
        if (hasA) ra[i] = lda_splice(a.feats, D, a.context, t, lo, hi, oA, jA);
        if (hasB) rb[i] = lda_splice(a.feats, D, a.context, t, lo, hi, oB, jB);
      }
    }
  };
  gather(0);
  for (uint32_t f0 = 0; f0 < sn; f0 += kStage) {
    __syncthreads();  // the previous stage has been read
#pragma unroll
    for (uint32_t i = 0; i < kStage / 4; i++) {
      const uint32_t f = wave + 4 * i, at = f * kBlock + (col ^ ((f & 1u) << 4));
      pa[at] = (double)ra[i];
      if (!diag) pb[at] = (double)rb[i];
    }
    __syncthreads();
    if (f0 + kStage < sn) gather(f0 + kStage);
#pragma unroll 2
    for (uint32_t f = 0; f < kStage; f += 4) {
      const double* ar = pa + (f + kk) * kBlock;
      const double* br = pbr + (f + kk) * kBlock;
      const double a0 = ar[(rt0 * 16 + cc) ^ sw], a1 = ar[((rt0 + 1) * 16 + cc) ^ sw];
      const double b0 = br[(ct0 * 16 + cc) ^ sw], b1 = br[((ct0 + 1) * 16 + cc) ^ sw];
      if (live[0][0]) acc[0][0] = __builtin_amdgcn_mfma_f64_16x16x4f64(a0, b0, acc[0][0], 0, 0, 0);
      if (live[0][1]) acc[0][1] = __builtin_amdgcn_mfma_f64_16x16x4f64(a0, b1, acc[0][1], 0, 0, 0);
      if (live[1][0]) acc[1][0] = __builtin_amdgcn_mfma_f64_16x16x4f64(a1, b0, acc[1][0], 0, 0, 0);
      if (live[1][1]) acc[1][1] = __builtin_amdgcn_mfma_f64_16x16x4f64(a1, b1, acc[1][1], 0, 0, 0);
    }
  }
  // partial[seg][block][row][column]: the result's row of register v is kk + 4 v, its column cc
  double* out = a.partial + ((uint64_t)blockIdx.x * gridDim.y + blockIdx.y) * (kBlock * kBlock);
#pragma unroll
  for (int r = 0; r < 2; r++)
#pragma unroll
    for (int q = 0; q < 2; q++) {
      if (!live[r][q]) continue;
#pragma unroll
      for (int v = 0; v < 4; v++) out[((rt0 + r) * 16 + kk + 4 * v) * kBlock + (ct0 + q) * 16 + cc] = acc[r][q][v];
    }
}

// grid (ceil(E / 256), E): thread (k, j = blockIdx.y), j <= k
__global__ __launch_bounds__(256) void lda_reduce_kernel(LdaArgs a) {
  const uint32_t E = a.E, nP = (E + kBlock - 1) / kBlock;
  const uint32_t k = blockIdx.x * 256 + threadIdx.x, j = blockIdx.y;
  if (k >= E || k < j) return;
  const uint32_t I = j / kBlock, J = k / kBlock, pair = I * nP - I * (I - 1) / 2 + (J - I), n_pairs = nP * (nP + 1) / 2;
  const double* src = a.partial + (uint64_t)pair * (kBlock * kBlock) + (j - I * kBlock) * kBlock + (k - J * kBlock);
  double sum = a.seg0 ? a.out_scatter[(uint64_t)j * E + k] : 0.0;
  for (uint32_t g = 0; g < a.n_segs; g++) sum = sum + src[(uint64_t)g * n_pairs * (kBlock * kBlock)];
  a.out_scatter[(uint64_t)j * E + k] = sum;
  a.out_scatter[(uint64_t)k * E + j] = sum;
}

hipError_t launch_lda_round(const LdaArgs& a, hipStream_t stream) {
  if (a.E == 0 || a.E > (uint32_t)kMaxE || a.dim == 0) return hipErrorInvalidValue;
  if (a.n_segs) {
    hipLaunchKernelGGL(lda_scatter_kernel, dim3(a.n_segs, lda_pairs(a.E)), dim3(256), 0, stream, a);
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e;
  }
  hipLaunchKernelGGL(lda_reduce_kernel, dim3((a.E + 255) / 256, a.E), dim3(256), 0, stream, a);
  return hipGetLastError();
}

// grid (class segments): a thread per column
__global__ __launch_bounds__(256) void lda_class_sum_kernel(LdaArgs a) {
  const uint32_t E = a.E, D = a.dim, g = blockIdx.x, b = a.cseg_begin[g], len = a.cseg_len[g];
  for (uint32_t n = threadIdx.x; n < E; n += 256) {
    const uint32_t o = n / D, j = n - o * D;
    double sum = 0.0;
    for (uint32_t q = 0; q < len; q++) {
      const uint32_t t = a.class_items[b + q], lo = a.frame_span[2 * (uint64_t)t], hi = a.frame_span[2 * (uint64_t)t + 1];
      sum = sum + (double)lda_splice(a.feats, D, a.context, t, lo, hi, o, j);
    }
    a.cpartial[(uint64_t)g * E + n] = sum;
  }
}

// grid (classes x ceil(E / 256)): the classes in blockIdx.x, whose limit n_classes cannot reach
__global__ __launch_bounds__(256) void lda_class_reduce_kernel(LdaArgs a) {
  const uint32_t E = a.E, nb = (E + 255) / 256, k = blockIdx.x / nb, n = (blockIdx.x - k * nb) * 256 + threadIdx.x;
  if (n >= E) return;
  double sum = 0.0;
  for (uint32_t g = a.class_seg_off[k]; g < a.class_seg_off[k + 1]; g++) sum = sum + a.cpartial[(uint64_t)g * E + n];
  a.out_sum[(uint64_t)k * E + n] = sum;
}

hipError_t launch_lda_class_sums(const LdaArgs& a, hipStream_t stream) {
  if (a.E == 0 || a.E > (uint32_t)kMaxE || a.dim == 0 || a.n_classes == 0) return hipErrorInvalidValue;
  if (a.n_csegs) {
    hipLaunchKernelGGL(lda_class_sum_kernel, dim3(a.n_csegs), dim3(256), 0, stream, a);
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e;
  }
  hipLaunchKernelGGL(lda_class_reduce_kernel, dim3(a.n_classes * ((a.E + 255) / 256)), dim3(256), 0, stream, a);
  return hipGetLastError();
}

// grid (ceil(frames / kFrames), ceil(p / kRows)); thread: row threadIdx.x & 15 of the tile against frames (threadIdx.x >> 4) + 16 q,
// q < 4, of the group: four independent chains.  M's tile and the group's spliced rows pass through the LDS kChunk columns at a time,
// n ascending, so the LDS does not grow with E; the rows' stride kChunk + 1 is odd: the 16 rows of M a half-wave reads (8-byte reads)
// and its two frames (4-byte reads) fall on different banks.
__global__ __launch_bounds__(256) void lda_project_kernel(const float* feats, const uint32_t* frame_span, uint64_t n_frames, uint32_t D,
                                                          uint32_t c, const double* M, uint32_t p, float* out) {
  constexpr int kStride = kChunk + 1;
  __shared__ double ms[kRows * kStride];
  __shared__ float zs[kFrames * kStride];
  __shared__ uint32_t span[kFrames * 2];
  const uint32_t E = (2 * c + 1) * D, row0 = blockIdx.y * kRows;
  const uint64_t t0 = (uint64_t)blockIdx.x * kFrames;
  const uint32_t nf = (uint32_t)(n_frames - t0 < (uint64_t)kFrames ? n_frames - t0 : (uint64_t)kFrames);
  if (threadIdx.x < 2 * kFrames) span[threadIdx.x] = threadIdx.x < 2 * nf ? frame_span[2 * t0 + threadIdx.x] : 0u;
  const uint32_t r = threadIdx.x & 15u, fs = threadIdx.x >> 4;
  const bool has_row = row0 + r < p;
  const double bias = has_row ? M[(uint64_t)(row0 + r) * (E + 1) + E] : 0.0;
  double acc[4] = {bias, bias, bias, bias};
  // staging: this thread's column of a chunk, rows / frames (threadIdx.x >> 7) + 2 i
  const uint32_t col = threadIdx.x & (kChunk - 1), half = threadIdx.x >> 7;
  for (uint32_t n0 = 0; n0 < E; n0 += kChunk) {
    __syncthreads();  // the spans are staged / the previous chunk has been read
    const uint32_t n = n0 + col;
    if (n < E) {
      const uint32_t o = n / D, j = n - o * D;
#pragma unroll
      for (uint32_t i = 0; i < kRows / 2; i++) {
        const uint32_t q = half + 2 * i;
        ms[q * kStride + col] = row0 + q < p ? M[(uint64_t)(row0 + q) * (E + 1) + n] : 0.0;
      }
#pragma unroll 8
      for (uint32_t i = 0; i < kFrames / 2; i++) {
        const uint32_t f = half + 2 * i;
        zs[f * kStride + col] = f < nf ? lda_splice(feats, D, c, (uint32_t)(t0 + f), span[2 * f], span[2 * f + 1], o, j) : 0.f;
      }
    }
    __syncthreads();
    const uint32_t cn = E - n0 < (uint32_t)kChunk ? E - n0 : (uint32_t)kChunk;
    const double* const mr = ms + r * kStride;
    const float* const z = zs + fs * kStride;
    for (uint32_t k = 0; k < cn; k++) {
      const double w = mr[k];
#pragma unroll
      for (int q = 0; q < 4; q++) acc[q] = acc[q] + w * (double)z[q * 16 * kStride + k];
    }
  }
  if (has_row)
#pragma unroll
    for (int q = 0; q < 4; q++)
      if (fs + 16 * q < nf) out[(t0 + fs + 16 * q) * p + row0 + r] = (float)acc[q];
}

hipError_t launch_lda_project(const float* feats, const uint32_t* frame_span, uint64_t n_frames, uint32_t dim, uint32_t context,
                              const double* M, uint32_t p, float* out, hipStream_t stream) {
  if (n_frames == 0) return hipSuccess;
  const uint32_t E = (2 * context + 1) * dim;
  if (E == 0 || E > (uint32_t)kMaxE || p == 0) return hipErrorInvalidValue;
  hipLaunchKernelGGL(lda_project_kernel, dim3((unsigned)((n_frames + kFrames - 1) / kFrames), (p + kRows - 1) / kRows), dim3(256), 0, stream,
                     feats, frame_span, n_frames, dim, context, M, p, out);
  return hipGetLastError();
}

}  // namespace srgpu
