// vtln_tables.h -- the mel filterbank's tables, unwarped and under a vocal-tract-length warp, and the choice of a speaker's warp from the
// search's costs (sr_frontend_create, sr_frontend_create_warped, sr_vtln_choose; the definitions are in include/srgpu.h).  Host code
// over plain arrays, no HIP include: tests/cpp/vtln_tables_driver.cpp compiles it with the host compiler alone.
//
// The warp has one break point and is piecewise linear: with f0 = break_frac f_high min(1, 1 / alpha),
//   g(f) = alpha f                                                   for f <= f0
//        = alpha f0 + (f_high - alpha f0) / (f_high - f0) (f - f0)   for f >  f0,
// so g(f_high) = f_high.  alpha == 1.0 is the identity by definition, with no arithmetic.  The filters' edges stay where they are; bin k
// has, in filter m of warp alpha, the weight of the unwarped triangle at g(f_k).  g is monotone, so the bins of positive weight are
// still one run and the table stays a CSR: first bin, count, offset of the run's weights.
#pragma once
#include <algorithm>
#include <cmath>
#include <cstdint>
#include <vector>

namespace srplan {

constexpr uint32_t kVtlnMaxWarps = 32;
constexpr uint32_t kVtlnMaxPairs = 1024;  // n_warps x n_mel: the logarithms of one frame under every warp, 4 KiB of a wave's LDS

inline double mel(double f) { return 2595.0 * std::log10(1.0 + f / 700.0); }
inline double mel_inv(double m) { return 700.0 * (std::pow(10.0, m / 2595.0) - 1.0); }

inline double vtln_warp(double f, double alpha, double f_high, double break_frac) {
  if (alpha == 1.0) return f;
  const double f0 = break_frac * f_high * std::min(1.0, 1.0 / alpha);
  if (f <= f0) return alpha * f;
  return alpha * f0 + (f_high - alpha * f0) / (f_high - f0) * (f - f0);
}

// the filters of one warp, appended to the CSR: n_mel entries more in first / count / off, the runs' weights behind those already in w
struct MelTables {
  std::vector<uint32_t> first, count, off;
  std::vector<float> w;
};

// -1: done; else the first filter without a bin of positive weight (edges *l .. *r Hz), nothing appended for it or the filters after it
inline int append_mel_filters(double sample_rate, uint32_t n_fft, uint32_t n_mel, double f_low, double f_high, double alpha,
                              double break_frac, MelTables* t, double* l_out, double* r_out) {
  const uint32_t N = n_fft, bins = N / 2 + 1;
  const double lo = mel(f_low), hi = mel(f_high), step = (hi - lo) / (n_mel + 1);
  std::vector<double> edge(n_mel + 2);
  for (uint32_t j = 0; j < n_mel + 2; j++) edge[j] = mel_inv(lo + j * step);
  std::vector<float> w(bins);
  for (uint32_t m = 0; m < n_mel; m++) {
    const double l = edge[m], c = edge[m + 1], r = edge[m + 2];
    uint32_t first = bins, last = 0;  // the bins of positive weight: first .. last
    for (uint32_t k = 0; k < bins; k++) {
      const double fk = vtln_warp(k * (sample_rate / N), alpha, f_high, break_frac);
      const double v = std::max(0.0, std::min((fk - l) / (c - l), (r - fk) / (r - c)));
      w[k] = (float)v;
      if (w[k] > 0.0f) { first = std::min(first, k); last = k; }
    }
    if (first == bins) { *l_out = l; *r_out = r; return (int)m; }
    t->first.push_back(first);
    t->count.push_back(last - first + 1);
    t->off.push_back((uint32_t)t->w.size());
    t->w.insert(t->w.end(), w.begin() + first, w.begin() + last + 1);
  }
  return -1;
}

// sr_vtln_params' own checks: 0 fine, 1 invalid (SR_EINVAL), 2 beyond a limit (SR_ELIMIT); *what says which
inline int vtln_check(uint32_t n_warps, const double* alpha, double break_frac, uint32_t n_mel, const char** what) {
  if (n_warps == 0) { *what = "n_warps is 0"; return 1; }
  if (!alpha) { *what = "alpha is null"; return 1; }
  if (!(break_frac > 0.0 && break_frac < 1.0)) { *what = "break_frac must lie in (0, 1)"; return 1; }
  if (n_warps > kVtlnMaxWarps) { *what = "more than 32 warps"; return 2; }
  for (uint32_t a = 0; a < n_warps; a++)
    if (!(alpha[a] > 0.0) || !std::isfinite(alpha[a])) { *what = "an alpha is not positive and finite"; return 1; }
  if ((uint64_t)n_warps * n_mel > kVtlnMaxPairs) { *what = "n_warps x n_mel exceeds 1024, what a wave's LDS holds of one frame"; return 2; }
  return 0;
}

// sr_vtln_choose: per speaker the first warp of smallest cost; the fallback for fewer than min_frames frames or a smallest cost that is
// not finite (a NaN anywhere in the speaker's row counts as that)
inline void vtln_choose(uint32_t n_speakers, uint32_t n_warps, const double* cost, const uint64_t* frames, uint64_t min_frames,
                        uint32_t fallback_warp, uint32_t* out_warp) {
  for (uint32_t s = 0; s < n_speakers; s++) {
    const double* c = cost + (size_t)s * n_warps;
    uint32_t best = 0;
    bool nan = false;
    for (uint32_t a = 0; a < n_warps; a++) {
      if (std::isnan(c[a])) nan = true;
      else if (std::isnan(c[best]) || c[a] < c[best]) best = a;
    }
    out_warp[s] = frames[s] < min_frames || nan || !std::isfinite(c[best]) ? fallback_warp : best;
  }
}

}  // namespace srplan

// The LDS geometry of the front end's kernels (frontend.hip), here so that the host-only driver checks the very functions the
// launches use.
namespace srgpu {

constexpr uint32_t mfcc_span_cap() { return 4096; }    // pre-emphasised samples a workgroup keeps in the LDS
constexpr uint32_t mfcc_waves(uint32_t n_fft) { return n_fft <= 1024 ? 4 : 2; }  // waves per workgroup: at most 48 KiB of LDS
// mfcc_warps_kernel: a wave keeps, beside its two transform buffers (2 n_fft floats), the n_warps x n_mel logarithms, rounded up to 64
// floats.  Waves per workgroup: mfcc_waves(), halved while the workgroup would take more than 64 KiB, which keeps two workgroups on
// a CU's 160 KiB whatever the shape (512 / 24 filters / 13 warps, 16 frames of shift 160: 10.9 + 4 x 5.25 = 31.9 KiB, four of them).
// Under the present limits (1024 pairs, n_fft <= 2048, a span of 4096 samples) the largest workgroup is exactly 64 KiB.
constexpr uint32_t mfcc_warps_pair_floats(uint32_t n_warps, uint32_t n_mel) { return (n_warps * n_mel + 63) & ~63u; }
constexpr uint32_t mfcc_warps_lds_bytes(uint32_t y_floats, uint32_t n_fft, uint32_t pair_floats, uint32_t waves) {
  return 4 * (y_floats + waves * (2 * n_fft + pair_floats));
}
constexpr uint32_t mfcc_warps_waves(uint32_t y_floats, uint32_t n_fft, uint32_t pair_floats) {
  uint32_t w = mfcc_waves(n_fft);
  while (w > 1 && mfcc_warps_lds_bytes(y_floats, n_fft, pair_floats, w) > 65536) w >>= 1;
  return w;
}

}  // namespace srgpu
