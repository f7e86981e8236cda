// stream_pipeline.hip -- the feature pipeline of a stream set: frame splicing with a projection (sr_corpus_splice_transform's row)
// and a per-utterance affine transform (sr_corpus_transform's row) applied to the rows of a push before they are scored.
//
// stream_pipeline_kernel, one workgroup per pushed utterance (kernels.h: StreamPipelineJob; stream_pipeline_plan.h has the
// bookkeeping).  The utterance had R input rows before the push and gains k; its history -- the input rows R - min(R, 2c) .. R - 1,
// row g at ring position g mod 2c of the slot's block -- is what earlier pushes left.
//   (a) the history goes into the LDS (at most 2c D < 512 floats); the new rows stay where they are, in the push's input buffer
//       (uploaded, or written by stream_frontend_kernel earlier on the same stream);
//   (b) the output rows [row0, row0 + rows), kFrames at a time, a tile of kRows rows of M at a time: M's tile and the spliced rows pass
//       through the LDS kChunk columns at a time, n ascending -- lda_project_kernel's loop, acc = M[i][E], acc = acc + M[i][n] * z[n],
//       no contraction into FMAs -- so the LDS does not grow with E.  A thread keeps one row of M against two frames;
//   (c) with a transform for the slot, the projected rows are rounded to float into the LDS and W = [A b], staged once, is applied
//       through affine_row; the result goes to the buffer the scoring reads.  Without one, (b) writes there directly;
//   (d) after a barrier the new input rows max(R, R + k - 2c) .. R + k - 1 are stored at their ring positions.
// Without a projection (M == nullptr) c is 0 and (b) is skipped: (c) reads the new rows themselves.  A push that readies no row runs
// (a) and (d) alone.  No atomics: a slot's history is touched by its own workgroup alone, and read only into the LDS before a barrier.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "kernels.h"
#include "splice_clamp.h"
#include "stream_pipeline_plan.h"
#include "sym_contract.h"

namespace srgpu {

#pragma clang fp contract(off)

namespace {

constexpr int kRows = 16;    // rows of M per tile ...
constexpr int kFrames = 32;  // ... output rows per group ...
constexpr int kChunk = 64;   // ... and columns of M's tile and of the spliced rows in the LDS at a time
constexpr int kStride = kChunk + 1;  // odd: the 16 rows of M a half-wave reads and its frames fall on different banks

__global__ __launch_bounds__(256) void stream_pipeline_kernel(StreamPipelineArgs a) {
  __shared__ double ms[kRows * kStride];
  __shared__ float zs[kFrames * kStride];
  extern __shared__ double dyn[];  // W [p][p + 1] (with a transform), then y [kFrames][p] floats (with both stages), then the history
  const StreamPipelineJob j = a.jobs[blockIdx.x];
  const uint32_t D = a.in_dim, c = a.context, p = a.dim, H = 2 * c, PE = p + 1;
  const bool project = a.M != nullptr, transform = j.has_w != 0;
  double* const w = dyn;
  float* const y = reinterpret_cast<float*>(dyn + a.w_doubles);
  float* const hs = y + a.y_floats;
  float* const hist = a.hist + (size_t)j.slot * H * D;
  const float* const fresh = a.in + j.in0 * D;
  float* const out = a.out + j.out0 * p;
  const uint32_t R = j.R, hi = j.R + j.k;
  // (a)
  for (uint32_t e = threadIdx.x; e < H * D; e += 256) hs[e] = R >= H || e / D < R ? hist[e] : 0.0f;  // (R < 2c: positions 0 .. R - 1 are written)
  if (transform) {
    const double* Ws = a.W + (size_t)j.slot * p * PE;
    for (uint32_t e = threadIdx.x; e < p * PE; e += 256) w[e] = Ws[e];
  }
  __syncthreads();
  if (!project) {
    // (c) alone: output row row0 + f is the new row f (c == 0: row0 == R)
    for (uint64_t e = threadIdx.x; e < (uint64_t)j.rows * p; e += 256) {
      const uint64_t f = e / p;
      const uint32_t i = (uint32_t)(e - f * p);
      out[e] = transform ? (float)affine_row(w + i * PE, fresh + f * p, p) : fresh[e];
    }
  } else {
    const uint32_t E = (H + 1) * D;
    const uint32_t r = threadIdx.x & 15u, fs = threadIdx.x >> 4;  // compute: row r of the tile against frames fs, fs + 16
    const uint32_t col = threadIdx.x & (kChunk - 1), quarter = threadIdx.x >> 6;  // staging: column col, rows / frames quarter + 4 i
    for (uint32_t f0 = 0; f0 < j.rows; f0 += kFrames) {
      const uint32_t nf = j.rows - f0 < (uint32_t)kFrames ? j.rows - f0 : (uint32_t)kFrames;
      for (uint32_t i0 = 0; i0 < p; i0 += kRows) {
        const bool has_row = i0 + r < p;
        const double bias = has_row ? a.M[(size_t)(i0 + r) * (E + 1) + E] : 0.0;
        double acc[2] = {bias, bias};
        for (uint32_t n0 = 0; n0 < E; n0 += kChunk) {
          __syncthreads();  // the previous chunk has been read
          const uint32_t n = n0 + col;
          if (n < E) {
            const uint32_t o = n / D, d = n - o * D;
#pragma unroll
            for (uint32_t i = 0; i < kRows / 4; i++) {
              const uint32_t q = quarter + 4 * i;
              ms[q * kStride + col] = i0 + q < p ? a.M[(size_t)(i0 + q) * (E + 1) + n] : 0.0;
            }
#pragma unroll
            for (uint32_t i = 0; i < kFrames / 4; i++) {
              const uint32_t f = quarter + 4 * i;
              float v = 0.f;
              if (f < nf) {
                const uint32_t g = (uint32_t)srplan::splice_frame(j.row0 + f0 + f, o, c, 0, hi);
                const srplan::PipelineSource src = srplan::pipeline_source(c, R, g);  // (c == 0: no row comes from the history)
                v = src.history ? hs[src.index * D + d] : fresh[src.index * D + d];
              }
              zs[f * kStride + col] = v;
            }
          }
          __syncthreads();
          const uint32_t cn = E - n0 < (uint32_t)kChunk ? E - n0 : (uint32_t)kChunk;
          const double* const mr = ms + r * kStride;
          const float* const z = zs + fs * kStride;
          for (uint32_t k = 0; k < cn; k++) {
            const double m = mr[k];
#pragma unroll
            for (int q = 0; q < 2; q++) acc[q] = acc[q] + m * (double)z[q * 16 * kStride + k];
          }
        }
        if (has_row)
#pragma unroll
          for (int q = 0; q < 2; q++) {
            const uint32_t f = fs + 16 * q;
            if (f >= nf) continue;
            if (transform) y[f * p + i0 + r] = (float)acc[q];
            else out[(size_t)(f0 + f) * p + i0 + r] = (float)acc[q];
          }
      }
      if (transform) {
        __syncthreads();  // the group's projected rows are in y
        for (uint32_t e = threadIdx.x; e < nf * p; e += 256) {
          const uint32_t f = e / p, i = e - f * p;
          out[(size_t)f0 * p + e] = (float)affine_row(w + i * PE, y + f * p, p);
        }
        __syncthreads();  // ... and read, before the next group's are written
      }
    }
  }
  // (d) (the history was read into the LDS before the first barrier)
  if (H) {
    const uint32_t keep0 = (uint32_t)srplan::pipeline_keep0(c, R, j.k);
    for (uint32_t e = threadIdx.x; e < (hi - keep0) * D; e += 256) {
      const uint32_t g = keep0 + e / D, d = e % D;
      hist[(g % H) * D + d] = fresh[(size_t)(g - R) * D + d];
    }
  }
}

}  // namespace

size_t stream_pipeline_lds_bytes(uint32_t in_dim, uint32_t context, uint32_t dim, bool projection, bool transforms) {
  const size_t w = transforms ? (size_t)dim * (dim + 1) : 0, y = projection && transforms ? (size_t)kFrames * dim : 0;
  return sizeof(double) * w + sizeof(float) * (y + (projection ? 2 * (size_t)context * in_dim : 0)) +
         sizeof(double) * kRows * kStride + sizeof(float) * kFrames * kStride;
}

hipError_t launch_stream_pipeline(const StreamPipelineArgs& a, uint32_t n_jobs, hipStream_t stream) {
  if (n_jobs == 0) return hipSuccess;
  const bool projection = a.M != nullptr;
  if (!projection && (a.context != 0 || a.in_dim != a.dim)) return hipErrorInvalidValue;
  if (projection && (2 * a.context + 1) * a.in_dim > 512) return hipErrorInvalidValue;
  if (a.w_doubles != (a.W ? a.dim * (a.dim + 1) : 0u) || a.y_floats != (projection && a.W ? (uint32_t)kFrames * a.dim : 0u))
    return hipErrorInvalidValue;
  if (stream_pipeline_lds_bytes(a.in_dim, a.context, a.dim, projection, a.W != nullptr) > 65536) return hipErrorInvalidValue;
  const size_t dyn = sizeof(double) * a.w_doubles + sizeof(float) * ((size_t)a.y_floats + 2 * (size_t)a.context * a.in_dim);
  hipLaunchKernelGGL(stream_pipeline_kernel, dim3(n_jobs), dim3(256), dyn, stream, a);
  return hipGetLastError();
}

uint32_t stream_pipeline_group_rows() { return kFrames; }

}  // namespace srgpu
