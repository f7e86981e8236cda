// frontend.hip -- the audio front end's kernels: MFCC from PCM samples, and SignalAnalysis::process_features (static | delta |
// delta-delta, mean / deviation, energy maximum) on resident cepstra.  The definitions are in include/srgpu.h (sr_frontend_*); the
// host side -- checks, tables, entry points -- is frontend.cpp.
//
// mfcc_kernel.  A workgroup takes a span of consecutive frames of one utterance.  It reads the span's samples once, pre-emphasises
// them (y[n] = x[n] - alpha x[n - 1], x[-1] = 0 before the utterance's first sample only, so a frame never knows where spans begin)
// and keeps them in the LDS as floats.  Then every wave64 takes frames of the span in turn, one frame at a time, in LDS of its own:
//   the windowed frame, zero-extended to n_fft, as M = n_fft / 2 complex points z[n] = (x[2n], x[2n + 1]);
//   Z = FFT_M(z): Stockham stages of radix 4 (and one of radix 2 when log2 M is odd) between two buffers, so no digit reversal; the
//   twiddles come from the host's table;
//   X[k] = E[k] + w^k O[k], E = (Z[k] + conj Z[M - k]) / 2, O = (Z[k] - conj Z[M - k]) / 2i, w = exp(-2 pi i / n_fft), k = 0 .. M;
//   P[k] = |X[k]|^2; lane m sums filter m's bins in ascending order and takes the clamped logarithm; lane i sums cepstrum i over
//   the filters in ascending order.
// No atomics, and nothing a frame computes depends on its span or its batch: the same samples give the same bits anywhere.
// With a per-utterance warp index (sr_corpus_from_audio_warped) a span's workgroup takes its utterance's filters instead of the
// unwarped ones; nothing else changes.
//
// mfcc_warps_kernel and vtln_reduce_kernel (sr_vtln_costs_corpus): every warp's cepstra from one power spectrum per frame, and the
// costs' sums in their defined order; described where they stand.
//
// stream_frontend_kernel (sr_stream_push_audio).  The same two stages for utterances whose samples arrive in pieces: a workgroup per
// pushed utterance computes the new frames' statics with mfcc_kernel's per-frame body (mfcc_power, mfcc_cepstra), stages them behind the 2 step
// statics the slot keeps, and emits the rows whose windows are complete with feature_post_kernel's arithmetic (post_value).  With no
// energy maximum a streamed row carries the batch's bits; the maximum is the causal one of include/srgpu.h.  A job may name a warp
// (sr_stream_set_warp): its workgroup then takes that warp's filters as mfcc_kernel does, and the slot's history holds warped statics.
//
// Compiled with -ffp-contract=off: the post-processing is specified to the bit (float subtractions, FP64 subtraction and division),
// and the MFCC stage's bits must not depend on what the compiler may fuse around a frame.
#include <hip/hip_runtime.h>

#include "kernels.h"

namespace srgpu {

#pragma clang fp contract(off)

namespace {

__device__ __forceinline__ float2 cmul(float2 a, float2 b) { return make_float2(a.x * b.x - a.y * b.y, a.x * b.y + a.y * b.x); }
__device__ __forceinline__ float2 cadd(float2 a, float2 b) { return make_float2(a.x + b.x, a.y + b.y); }
__device__ __forceinline__ float2 csub(float2 a, float2 b) { return make_float2(a.x - b.x, a.y - b.y); }

// One frame through window, transform, filterbank, logarithm and DCT, in two halves: one wave64 in LDS of its own (A, B: M complex
// points each, L: 64 floats).  Every wave of the workgroup goes through every barrier: one without a frame left computes some frame
// again and stores nothing.
//
// The first half: yf, the frame's pre-emphasised samples -> P[k] = |X[k]|^2, k = 0 .. M, in whichever of A and B the transform did not
// end in; complete for the whole wave on return.
__device__ __forceinline__ const float* mfcc_power(const MfccArgs& a, const float* yf, float2* A, float2* B, uint32_t lane) {
  const uint32_t M = a.n_fft >> 1;
  for (uint32_t n = lane; n < M; n += 64) {
    const uint32_t i0 = 2 * n, i1 = 2 * n + 1;
    A[n] = make_float2(i0 < a.window ? a.win[i0] * yf[i0] : 0.0f, i1 < a.window ? a.win[i1] * yf[i1] : 0.0f);
  }
  float2 *src = A, *dst = B;
  uint32_t Ns = 1;
  for (; Ns * 4 <= M; Ns *= 4) {
    __syncthreads();
    const uint32_t q = M >> 2, tstep = M / (2 * Ns);
    for (uint32_t j = lane; j < q; j += 64) {
      const uint32_t k = j & (Ns - 1);
      const float2 v0 = src[j], v1 = cmul(src[j + q], a.twiddle[k * tstep]), v2 = cmul(src[j + 2 * q], a.twiddle[2 * k * tstep]),
                   v3 = cmul(src[j + 3 * q], a.twiddle[3 * k * tstep]);
      const float2 s02 = cadd(v0, v2), d02 = csub(v0, v2), s13 = cadd(v1, v3), d13 = csub(v1, v3);
      const float2 md13 = make_float2(d13.y, -d13.x);  // -i (v1 - v3)
      const uint32_t j0 = ((j - k) << 2) + k;
      dst[j0] = cadd(s02, s13);
      dst[j0 + Ns] = cadd(d02, md13);
      dst[j0 + 2 * Ns] = csub(s02, s13);
      dst[j0 + 3 * Ns] = csub(d02, md13);
    }
    float2* t = src; src = dst; dst = t;
  }
  if (Ns < M) {  // log2 M is odd: Ns == M / 2
    __syncthreads();
    for (uint32_t j = lane; j < Ns; j += 64) {
      const float2 v0 = src[j], v1 = cmul(src[j + Ns], a.twiddle[2 * j]);
      dst[j] = cadd(v0, v1);
      dst[j + Ns] = csub(v0, v1);
    }
    float2* t = src; src = dst; dst = t;
  }
  __syncthreads();
  float* P = reinterpret_cast<float*>(dst);  // [M + 1] of the buffer the transform is not in
  for (uint32_t k = lane; k <= M; k += 64) {
    const float2 zk = src[k & (M - 1)], zm = src[(M - k) & (M - 1)];
    const float2 e = make_float2(0.5f * (zk.x + zm.x), 0.5f * (zk.y - zm.y));
    const float2 o = make_float2(0.5f * (zk.y + zm.y), -0.5f * (zk.x - zm.x));
    const float2 xk = cadd(e, cmul(a.twiddle[k], o));
    P[k] = xk.x * xk.x + xk.y * xk.y;
  }
  __syncthreads();
  return P;
}

// a filterbank: per filter its first bin, its bins and where its weights begin in w
struct MelFilters {
  const uint32_t* first; const uint32_t* count; const uint32_t* off;
  const float* w;
};

// The second half: P, a filterbank and the DCT -> out, the frame's n_cepstra cepstra, stored by an active wave only.
__device__ __forceinline__ void mfcc_cepstra(const MfccArgs& a, const MelFilters& f, const float* P, float* L, uint32_t lane, bool active,
                                             float* out) {
  if (lane < a.n_mel) {
    const float* w = f.w + f.off[lane];
    const float* p = P + f.first[lane];
    const uint32_t n = f.count[lane];
    float e = 0.0f;
    for (uint32_t j = 0; j < n; j++) e += w[j] * p[j];
    L[lane] = logf(fmaxf(e, a.energy_floor));
  }
  __syncthreads();
  if (lane < a.n_cepstra && active) {
    const float* d = a.dct + lane * a.n_mel;
    float c = 0.0f;
    for (uint32_t m = 0; m < a.n_mel; m++) c += d[m] * L[m];
    out[lane] = c;
  }
  __syncthreads();
}

__global__ __launch_bounds__(256) void mfcc_kernel(MfccArgs a, uint32_t y_floats) {
  extern __shared__ float lds[];
  const uint32_t lane = threadIdx.x & 63, wave = threadIdx.x >> 6, n_waves = blockDim.x >> 6;
  const uint32_t M = a.n_fft >> 1;
  const uint2 sp = a.spans[blockIdx.x];
  const uint64_t f0 = a.frame_off[sp.x];
  const uint32_t T = (uint32_t)(a.frame_off[sp.x + 1] - f0), t0 = sp.y;
  const uint32_t nf = min(a.span_frames, T - t0);
  const uint32_t n_samp = (nf - 1) * a.shift + a.window;  // <= mfcc_span_cap() by the choice of span_frames
  const uint64_t first = (uint64_t)t0 * a.shift;          // the span's first sample within the utterance
  const int16_t* x = a.samples + a.sample_off[sp.x] + first;
  float* y = lds;
  for (uint32_t i = threadIdx.x; i < n_samp; i += blockDim.x) {
    const float prev = first + i ? (float)x[(int64_t)i - 1] : 0.0f;
    y[i] = (float)x[i] - a.preemphasis * prev;
  }
  float* mine = lds + y_floats + (size_t)wave * (4 * M + 64);
  float2* A = reinterpret_cast<float2*>(mine);
  // the utterance's filters: its warp's, read once for the workgroup, or the unwarped ones
  MelFilters f{a.mel_first, a.mel_count, a.mel_off, a.mel_w};
  if (a.utt_warp) {
    const uint32_t w0 = a.utt_warp[sp.x] * a.n_mel;
    f = MelFilters{a.warp_first + w0, a.warp_count + w0, a.warp_off + w0, a.warp_w};
  }
  __syncthreads();
  const uint32_t rounds = (a.span_frames + n_waves - 1) / n_waves;
  for (uint32_t r = 0; r < rounds; r++) {
    const uint32_t fi = r * n_waves + wave;
    const bool active = fi < nf;
    const float* P = mfcc_power(a, y + (active ? fi : 0) * a.shift, A, A + M, lane);
    mfcc_cepstra(a, f, P, mine + 4 * M, lane, active, a.out + (f0 + t0 + (active ? fi : 0)) * a.n_cepstra);
  }
}

// The warp search's MFCC stage (kernels.h): mfcc_kernel's spans, but a frame's P is computed once and every warp's filters are applied
// to it from the LDS.  The (warp, filter) pairs are dealt to the wave's lanes, pair q = warp n_mel + filter to lane q mod 64 -- 13 warps
// of 24 filters are five rounds of 64, not 13 of 24 -- and so are the (warp, cepstrum) pairs.  A pair sums its bins (its filters)
// ascending exactly as mfcc_cepstra's lane does, so warp w's cepstra carry the bits mfcc_kernel gives with warp w's filters.
// mine: A, B, then L[n_warps][n_mel].  out [n_warps][n_frames][n_cepstra].
__global__ __launch_bounds__(256) void mfcc_warps_kernel(MfccArgs a, uint32_t y_floats, uint32_t pair_floats) {
  extern __shared__ float lds[];
  const uint32_t lane = threadIdx.x & 63, wave = threadIdx.x >> 6, n_waves = blockDim.x >> 6;
  const uint32_t M = a.n_fft >> 1;
  const uint2 sp = a.spans[blockIdx.x];
  const uint64_t f0 = a.frame_off[sp.x];
  const uint32_t T = (uint32_t)(a.frame_off[sp.x + 1] - f0), t0 = sp.y;
  const uint32_t nf = min(a.span_frames, T - t0);
  const uint32_t n_samp = (nf - 1) * a.shift + a.window;
  const uint64_t first = (uint64_t)t0 * a.shift;
  const int16_t* x = a.samples + a.sample_off[sp.x] + first;
  float* y = lds;
  for (uint32_t i = threadIdx.x; i < n_samp; i += blockDim.x) {
    const float prev = first + i ? (float)x[(int64_t)i - 1] : 0.0f;
    y[i] = (float)x[i] - a.preemphasis * prev;
  }
  float* mine = lds + y_floats + (size_t)wave * (4 * M + pair_floats);
  float2* A = reinterpret_cast<float2*>(mine);
  float* L = mine + 4 * M;
  const uint32_t n_pairs = a.n_warps * a.n_mel, n_outs = a.n_warps * a.n_cepstra;
  __syncthreads();
  const uint32_t rounds = (a.span_frames + n_waves - 1) / n_waves;
  for (uint32_t r = 0; r < rounds; r++) {
    const uint32_t fi = r * n_waves + wave;
    const bool active = fi < nf;
    const float* P = mfcc_power(a, y + (active ? fi : 0) * a.shift, A, A + M, lane);
    for (uint32_t q = lane; q < n_pairs; q += 64) {
      const float* w = a.warp_w + a.warp_off[q];
      const float* p = P + a.warp_first[q];
      const uint32_t n = a.warp_count[q];
      float e = 0.0f;
      for (uint32_t j = 0; j < n; j++) e += w[j] * p[j];
      L[q] = logf(fmaxf(e, a.energy_floor));
    }
    __syncthreads();
    if (active) {
      float* out = a.out + (f0 + t0 + fi) * a.n_cepstra;
      for (uint32_t q = lane; q < n_outs; q += 64) {
        const uint32_t wq = q / a.n_cepstra, i = q - wq * a.n_cepstra;
        const float* d = a.dct + i * a.n_mel;
        const float* Lw = L + wq * a.n_mel;
        float c = 0.0f;
        for (uint32_t m = 0; m < a.n_mel; m++) c += d[m] * Lw[m];
        out[(uint64_t)wq * a.n_frames * a.n_cepstra + i] = c;
      }
    }
    __syncthreads();
  }
}

// the sums of sr_vtln_costs_corpus (kernels.h: VtlnReduceArgs): a thread per (row, warp), neighbouring threads neighbouring rows
__global__ __launch_bounds__(256) void vtln_reduce_kernel(VtlnReduceArgs a) {
  const uint64_t e = (uint64_t)blockIdx.x * 256 + threadIdx.x;
  if (e >= (uint64_t)a.n_rows * a.n_warps) return;
  const uint32_t w = (uint32_t)(e / a.n_rows), r = (uint32_t)(e - (uint64_t)w * a.n_rows);
  const double* s = a.src + w * a.src_stride;
  const uint64_t j0 = a.off[r], j1 = a.off[r + 1];
  double sum = 0.0;
  if (j1 > j0) {
    sum = s[a.items ? a.items[j0] : j0];  // the first addend as it is
    for (uint64_t j = j0 + 1; j < j1; j++) sum = sum + s[a.items ? a.items[j] : j];
  }
  a.out[r * a.out_row + w * a.out_warp] = sum;
}

// the utterance of frame f: the last u with frame_off[u] <= f (an empty utterance is never it)
__device__ __forceinline__ uint32_t utterance_of(const uint64_t* frame_off, uint32_t n_utts, uint64_t f) {
  uint32_t lo = 0, hi = n_utts;  // frame_off[lo] <= f < frame_off[hi]
  while (hi - lo > 1) {
    const uint32_t mid = lo + (hi - lo) / 2;
    if (frame_off[mid] <= f) lo = mid; else hi = mid;
  }
  return lo;
}

// Row t, component c of FeaturePostProcessor::process_features for an utterance of T frames: statics, deltas, normalisation (not the
// energy maximum).  Static idx of the utterance is at s[(idx - origin) nf + k].  T == kStreamFrontendOpen, "not known yet", leaves
// every clamp at the end inactive: such a row needs static t + step to exist.
__device__ __forceinline__ float post_value(const float* s, int64_t origin, uint32_t nf, uint32_t n_first, uint32_t step, uint32_t T,
                                            uint32_t t, uint32_t c, const double* mean, const double* stddev) {
  auto at = [&](uint32_t idx, uint32_t k) { return s[(uint64_t)((int64_t)idx - origin) * nf + k]; };
  // delta of component k at frame t: window clamped at the start
  auto delta = [&](uint32_t tt, uint32_t k) {
    const uint32_t hi = min(max(tt, step), T - 1), lo = hi >= step ? hi - step : 0;
    return at(hi, k) - at(lo, k);
  };
  float v;
  if (c < nf) {
    v = at(t, c);
  } else if (c < nf + n_first) {
    v = delta(t, c - nf);
  } else {  // from the deltas, window clamped at the end
    const uint32_t k = c - nf - n_first, ahead = T > step ? min(t, T - 1 - step) + step : T - 1;
    v = delta(ahead, k) - delta(t, k);
  }
  if (mean) {
    v = (float)((double)v - mean[c]);
    v = (float)((double)v / stddev[c]);
  }
  return v;
}

// a thread per (frame, output component): FeaturePostProcessor::process_features' statics, deltas and normalisation
__global__ __launch_bounds__(256) void feature_post_kernel(FeaturePostArgs a) {
  const uint32_t nt = a.n_static + a.n_first + a.n_second, nf = a.n_static;
  const uint64_t e = (uint64_t)blockIdx.x * 256 + threadIdx.x;
  if (e >= a.n_frames * nt) return;
  const uint64_t f = e / nt;
  const uint32_t c = (uint32_t)(e - f * nt);
  const uint32_t u = utterance_of(a.frame_off, a.n_utts, f);
  const uint64_t f0 = a.frame_off[u];
  const uint32_t T = (uint32_t)(a.frame_off[u + 1] - f0), t = (uint32_t)(f - f0);
  a.out[e] = post_value(a.cepstra + f0 * nf, 0, nf, a.n_first, a.step, T, t, c, a.mean, a.stddev);
}

// a workgroup per utterance: component 0 minus its maximum over the utterance.  The host loop keeps the first frame that reaches
// the maximum (it replaces on `<` alone), which tells -0 from +0; the pairs (value, frame) are reduced to the same one.
__global__ __launch_bounds__(256) void energy_max_kernel(const uint64_t* frame_off, uint32_t nt, float* out) {
  __shared__ float sv[256];
  __shared__ uint32_t si[256];
  const uint64_t f0 = frame_off[blockIdx.x];
  const uint32_t T = (uint32_t)(frame_off[blockIdx.x + 1] - f0);
  float* x = out + f0 * nt;
  float bv = -INFINITY;
  uint32_t bi = 0xFFFFFFFFu;
  for (uint32_t t = threadIdx.x; t < T; t += 256) {
    const float v = x[(uint64_t)t * nt];
    if (bv < v || (bv == v && t < bi)) { bv = v; bi = t; }
  }
  sv[threadIdx.x] = bv;
  si[threadIdx.x] = bi;
  __syncthreads();
  for (uint32_t h = 128; h > 0; h >>= 1) {
    if (threadIdx.x < h) {
      const float v = sv[threadIdx.x + h];
      const uint32_t i = si[threadIdx.x + h];
      if (sv[threadIdx.x] < v || (sv[threadIdx.x] == v && i < si[threadIdx.x])) { sv[threadIdx.x] = v; si[threadIdx.x] = i; }
    }
    __syncthreads();
  }
  const float mx = sv[0];
  for (uint32_t t = threadIdx.x; t < T; t += 256) x[(uint64_t)t * nt] -= mx;
}

// Streaming: one workgroup per pushed utterance (kernels.h: StreamFrontendJob).  (a) the new statics, span by span through the LDS
// exactly as mfcc_kernel computes them, (b) staged behind the slot's 2 step statics of history; after a barrier (c) the rows that
// became ready, post_value on the staging rows, straight into the push's feature buffer, the running maximum advanced in frame
// order by one thread; (d) the slot's new history and maximum.  No atomics: a slot's state is touched by its workgroup alone.
__global__ __launch_bounds__(256) void stream_frontend_kernel(StreamFrontendArgs s, uint32_t y_floats) {
  extern __shared__ float lds[];
  const MfccArgs& a = s.mfcc;
  const uint32_t lane = threadIdx.x & 63, wave = threadIdx.x >> 6, n_waves = blockDim.x >> 6;
  const uint32_t M = a.n_fft >> 1, nf = s.n_static, nt = s.n_static + s.n_first + s.n_second, H = 2 * s.step;
  const StreamFrontendJob j = s.jobs[blockIdx.x];
  float* st = s.state + (size_t)j.slot * ((size_t)H * nf + 1);
  float* stage = s.stage + j.stage0 * nf;
  for (uint32_t i = threadIdx.x; i < H * nf; i += blockDim.x) stage[i] = j.S ? st[i] : 0.0f;
  const int16_t* x = a.samples + j.sample0 + 1;  // the first sample of frame S; x[-1] is the sample before it, 0 before sample 0
  float* y = lds;
  float* mine = lds + y_floats + (size_t)wave * (4 * M + 64);
  float2* A = reinterpret_cast<float2*>(mine);
  // the utterance's filters, chosen once for the workgroup as mfcc_kernel chooses them: its warp's, or the unwarped ones
  MelFilters filters{a.mel_first, a.mel_count, a.mel_off, a.mel_w};
  if (j.warp != kStreamNoWarp) {
    const uint32_t w0 = j.warp * a.n_mel;
    filters = MelFilters{a.warp_first + w0, a.warp_count + w0, a.warp_off + w0, a.warp_w};
  }
  for (uint32_t j0 = 0; j0 < j.k; j0 += a.span_frames) {
    const uint32_t n = min(a.span_frames, j.k - j0);
    const uint32_t n_samp = (n - 1) * a.shift + a.window;
    const int16_t* xs = x + (uint64_t)j0 * a.shift;
    for (uint32_t i = threadIdx.x; i < n_samp; i += blockDim.x) y[i] = (float)xs[i] - a.preemphasis * (float)xs[(int64_t)i - 1];
    __syncthreads();
    for (uint32_t r = 0; r * n_waves < n; r++) {
      const uint32_t fi = r * n_waves + wave;
      const bool active = fi < n;
      const float* P = mfcc_power(a, y + (active ? fi : 0) * a.shift, A, A + M, lane);
      mfcc_cepstra(a, filters, P, mine + 4 * M, lane, active, stage + (size_t)(H + j0 + (active ? fi : 0)) * nf);
    }
  }
  __syncthreads();
  const int64_t origin = (int64_t)j.S - H;  // the utterance's static at the first staging row
  float* out = s.out + j.out0 * nt;
  for (uint32_t e = threadIdx.x; e < j.rows * nt; e += blockDim.x) {
    const uint32_t r = e / nt, c = e - r * nt;
    out[e] = post_value(stage, origin, nf, s.n_first, s.step, j.T, j.row0 + r, c, s.mean, s.stddev);
  }
  if (s.energy_max_norm) {
    __syncthreads();
    if (threadIdx.x == 0) {
      // m after static i: the maximum over statics 0 .. i, replaced on `<` alone; row i - step takes it, the finish's last rows the last
      float m = j.S ? st[(size_t)H * nf] : -INFINITY;
      for (uint32_t i = j.S; i < j.S + j.k; i++) {
        const float v = post_value(stage, origin, nf, s.n_first, s.step, j.T, i, 0, s.mean, s.stddev);
        if (m < v) m = v;
        if (i >= s.step) out[(size_t)(i - s.step - j.row0) * nt] -= m;
      }
      if (j.T != kStreamFrontendOpen)
        for (uint32_t t = max(j.row0, j.T > s.step ? j.T - s.step : 0u); t < j.T; t++) out[(size_t)(t - j.row0) * nt] -= m;
      st[(size_t)H * nf] = m;
    }
  }
  for (uint32_t i = threadIdx.x; i < H * nf; i += blockDim.x) st[i] = stage[(size_t)j.k * nf + i];
}

}  // namespace

hipError_t launch_mfcc(const MfccArgs& a, hipStream_t stream) {
  if (a.n_spans == 0) return hipSuccess;
  const uint32_t waves = mfcc_waves(a.n_fft), M = a.n_fft / 2;
  const uint32_t y_floats = ((a.span_frames - 1) * a.shift + a.window + 3) & ~3u;
  const size_t lds_bytes = sizeof(float) * ((size_t)y_floats + (size_t)waves * (4 * M + 64));
  hipLaunchKernelGGL(mfcc_kernel, dim3(a.n_spans), dim3(64 * waves), lds_bytes, stream, a, y_floats);
  return hipGetLastError();
}

hipError_t launch_mfcc_warps(const MfccArgs& a, hipStream_t stream) {
  if (a.n_spans == 0 || a.n_warps == 0) return hipSuccess;
  const uint32_t y_floats = ((a.span_frames - 1) * a.shift + a.window + 3) & ~3u;
  const uint32_t pair_floats = mfcc_warps_pair_floats(a.n_warps, a.n_mel);
  const uint32_t waves = mfcc_warps_waves(y_floats, a.n_fft, pair_floats);
  const size_t lds_bytes = mfcc_warps_lds_bytes(y_floats, a.n_fft, pair_floats, waves);
  if (lds_bytes > 65536) return hipErrorInvalidValue;  // (sr_frontend_create_warped's limits keep a single wave within it)
  hipLaunchKernelGGL(mfcc_warps_kernel, dim3(a.n_spans), dim3(64 * waves), lds_bytes, stream, a, y_floats, pair_floats);
  return hipGetLastError();
}

hipError_t launch_vtln_reduce(const VtlnReduceArgs& a, hipStream_t stream) {
  const uint64_t n = (uint64_t)a.n_rows * a.n_warps;
  if (n == 0) return hipSuccess;
  hipLaunchKernelGGL(vtln_reduce_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, stream, a);
  return hipGetLastError();
}

hipError_t launch_feature_post(const FeaturePostArgs& a, hipStream_t stream) {
  if (a.n_frames == 0) return hipSuccess;
  const uint64_t n = a.n_frames * (a.n_static + a.n_first + a.n_second);
  hipLaunchKernelGGL(feature_post_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, stream, a);
  if (a.energy_max_norm)
    hipLaunchKernelGGL(energy_max_kernel, dim3(a.n_utts), dim3(256), 0, stream, a.frame_off, a.n_static + a.n_first + a.n_second, a.out);
  return hipGetLastError();
}

hipError_t launch_stream_frontend(const StreamFrontendArgs& a, uint32_t n_jobs, hipStream_t stream) {
  if (n_jobs == 0) return hipSuccess;
  const uint32_t waves = mfcc_waves(a.mfcc.n_fft), M = a.mfcc.n_fft / 2;
  const uint32_t y_floats = ((a.mfcc.span_frames - 1) * a.mfcc.shift + a.mfcc.window + 3) & ~3u;
  const size_t lds_bytes = sizeof(float) * ((size_t)y_floats + (size_t)waves * (4 * M + 64));
  hipLaunchKernelGGL(stream_frontend_kernel, dim3(n_jobs), dim3(64 * waves), lds_bytes, stream, a, y_floats);
  return hipGetLastError();
}

}  // namespace srgpu
