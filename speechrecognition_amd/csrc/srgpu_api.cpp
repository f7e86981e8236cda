// srgpu_api.cpp -- C ABI of libsrgpu.so (include/srgpu.h): handles, device memory, model packing,
// the chunked score -> search pipeline on two HIP streams, and event-based kernel timing.
//
// Nothing here computes scores or paths on the host: every sr_score_* / sr_recognize_* / sr_align_*
// call runs the HIP kernels of gmm_mfma.hip / gmm_exact.hip / viterbi_decode.hip / viterbi_align.hip
// and fails loudly (SR_EHIP / SR_ENODEV) when no gfx950 device is usable.  There is no CPU fallback.
// The forward-backward style passes (fb_check .. sr_bigram_word_lattice_corpus) plan their launch groups, step order and mixture lists
// with fb_plan.h, host code that is tested on its own.  Host algorithms on plain arrays, with no handle and no HIP call, are files of
// their own that this unit includes, each complete by itself and built alone under the sanitizers by a test driver: chains.cpp (the
// transcripts' chains of the MMI passes) and nbest.cpp (sr_lattice_nbest, sr_bigram_lattice_nbest).  The streaming entry points
// (sr_stream_*, sr_bigram_stream_*) and their helpers are stream_api.cpp, included behind the scoring and chunk helpers they use.
// Every entry point is declared extern "C" with SR_API in include/srgpu.h: the definitions here take linkage and visibility from there.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstdarg>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <functional>
#include <limits>
#include <map>
#include <memory>
#include <mutex>
#include <numeric>
#include <string>
#include <type_traits>
#include <vector>

#include "../../include/srgpu.h"
#include "fb_plan.h"
#include "host_util.h"
#include "kernels.h"
#include "traceback.h"

using namespace srgpu;
using srhost::guarded;

#include "handles.h"

using srhost::fail;

namespace {
thread_local char g_err[512] = "";
}  // namespace
namespace srhost {
int fail(int code, const char* fmt, ...) {
  va_list ap;
  va_start(ap, fmt);
  vsnprintf(g_err, sizeof g_err, fmt, ap);
  va_end(ap);
  return code;
}
int set_error(int code, const char* msg) { return fail(code, "%s", msg); }
}  // namespace srhost

namespace {

// ---- model packing for the MFMA kernel ---------------------------------------------------------
// States are sorted by density count (stable, descending) and chunked into groups of four; group q
// owns ceil(max_count/4) blocks of 16 model rows; row r of block j holds density 4*j + (r>>2) of the
// group's state slot (r&3).  Fragment order: apack[block][kstep][lane] = A[row = lane&15][k = 4*kstep + (lane>>4)].
int pack_model(sr_model* m, const uint32_t* dens_off, const double* means, const double* inv_vars,
               const double* norm, const double* logw) {
  const uint32_t S = m->n_states, D = m->dim;
  const int KS = m->ksteps;
  std::vector<uint32_t> order(S);
  std::iota(order.begin(), order.end(), 0u);
  std::stable_sort(order.begin(), order.end(), [&](uint32_t x, uint32_t y) {
    return (dens_off[x + 1] - dens_off[x]) > (dens_off[y + 1] - dens_off[y]);
  });
  const uint32_t n_groups = (S + 3) / 4;
  std::vector<uint32_t> grp_state(4 * (size_t)n_groups, 0xFFFFFFFFu), first_block(n_groups + 1, 0);
  for (uint32_t q = 0; q < n_groups; q++) {
    uint32_t mx = 0;
    for (uint32_t g = 0; g < 4; g++) {
      const uint32_t i = 4 * q + g;
      if (i < S) {
        grp_state[4 * q + g] = order[i];
        mx = std::max(mx, dens_off[order[i] + 1] - dens_off[order[i]]);
      }
    }
    first_block[q + 1] = first_block[q] + std::max(1u, (mx + 3) / 4);
  }
  const uint32_t n_blocks = first_block[n_groups];
  const size_t blk_doubles = (size_t)KS * 64;
  std::vector<double> apack(blk_doubles * n_blocks, 0.0);
  std::vector<uint32_t> meta(n_blocks);
  const double inf = std::numeric_limits<double>::infinity();
  for (uint32_t q = 0; q < n_groups; q++) {
    for (uint32_t b = first_block[q]; b < first_block[q + 1]; b++) {
      meta[b] = (q << 1) | (b + 1 == first_block[q + 1] ? 1u : 0u);
      const uint32_t j = b - first_block[q];
      for (uint32_t r = 0; r < 16; r++) {
        const uint32_t g = r & 3, sub = r >> 2;
        const uint32_t st = grp_state[4 * q + g];
        const uint32_t i = 4 * j + sub;
        const bool real = st != 0xFFFFFFFFu && i < dens_off[st + 1] - dens_off[st];
        const size_t c = real ? (size_t)dens_off[st] + i : 0;
        double konst = inf;  // padding row: +inf never wins the min and adds exp(-inf) = 0 to a sum
        if (real) {
          double q2 = 0.0;
          for (uint32_t d = 0; d < D; d++) q2 += means[c * D + d] * means[c * D + d] * inv_vars[c * D + d];
          konst = norm[c] - logw[c] + 0.5 * q2;
        }
        for (int ks = 0; ks < KS; ks++) {
          for (uint32_t kk = 0; kk < 4; kk++) {
            const uint32_t k = 4 * ks + kk;
            double v = 0.0;
            if (k < 2 * D) {
              if (real) {
                const uint32_t d = k >> 1;
                v = (k & 1) ? -means[c * D + d] * inv_vars[c * D + d] : 0.5 * inv_vars[c * D + d];
              }
            } else if (k == 2 * D) {
              v = konst;
            }
            apack[(size_t)b * blk_doubles + (size_t)ks * 64 + kk * 16 + r] = v;
          }
        }
      }
    }
  }
  m->n_groups = n_groups;
  m->n_blocks = n_blocks;
  m->group_first_block = first_block;
  HIP_TRY(m->apack.upload(apack.data(), apack.size()));
  HIP_TRY(m->blk_meta.upload(meta.data(), meta.size()));
  HIP_TRY(m->grp_state.upload(grp_state.data(), grp_state.size()));
  return SR_OK;
}

// ---- model packing for the fp16 prefilter ---------------------------------------------------------------------
// Groups of four (pseudo-)states in natural order, each padded to 8 blocks of 16 rows (32 density slots per state);
// row r of block j = density 4*j + (r & 3) of state slot (r >> 2).  Coefficients are scaled by a power of two and
// rounded once to fp16; fragment order [group][block][k-step of 32][lane][8]: lane l holds row l & 15,
// k = 32*ks + 8*(l >> 4) + j -- the A operand of v_mfma_f32_16x16x32_f16.
int pack_prefilter(sr_model* m, const uint32_t* dens_off, const double* means, const double* inv_vars,
                   const double* norm, const double* logw) {
  const uint32_t S = m->n_states, D = m->dim;
  uint32_t mx = 0;
  for (uint32_t s = 0; s < S; s++) mx = std::max(mx, dens_off[s + 1] - dens_off[s]);
  m->max_dens = std::max(1u, mx);
  m->pf_ks32 = 0;
  const uint32_t DP = gmm_refine_padded_dim(D);  // the odd dimension the refinement runs in (pairs | zeros | odd tail)
  // not eligible: callers get the exact kernel (> 128 densities per mixture need all eight panels of a state in one workgroup's LDS)
  if (!m->max_approx || mx > 256 || (mx > 128 && DP > 39) || 2 * D + 3 > 128 || DP == 0) return SR_OK;
  const int KS = (int)((2 * D + 3 + 31) / 32);
  {
    bool preserved = false;
    HIP_TRY(probe_fp16_denormals(m->s_gmm, &preserved));
    if (!preserved) return SR_OK;  // the bound of gmm_prefilter.hip does not hold with flushed subnormals: exact kernel
    bool accumulates = false;
    HIP_TRY(probe_fp16_accumulation(m->s_gmm, KS <= 3 ? 3 : 4, &accumulates, nullptr));  // the chain length this model runs
    if (!accumulates) return SR_OK;  // ... nor with an accumulator outside its model
  }
  m->pf_dp = DP;
  // A mixture of more than 32 densities is cut into Cs = 2 or 4 chunks of 32: the kernels see S*Cs pseudo-states
  // (ps = st*Cs + chunk), the prefilter takes the minimum across a state's chunks, the refinement folds them.
  // (129 .. 256 densities: Cs = 8 = two halves of four chunks; the fp16 pass sees each half as a four-chunk state of its own)
  const uint32_t Cs = mx <= 32 ? 1u : mx <= 64 ? 2u : mx <= 128 ? 4u : 8u;
  const uint32_t PS = S * Cs;
  m->pf_chunks = Cs;
  m->pf_pstates = PS;
  auto ps_count = [&](uint32_t ps) -> uint32_t {  // densities of pseudo-state ps
    const uint32_t n = dens_off[ps / Cs + 1] - dens_off[ps / Cs], lo = 32u * (ps % Cs);
    return n > lo ? std::min(32u, n - lo) : 0u;
  };
  {
    std::vector<uint32_t> cnt(PS);
    for (uint32_t ps = 0; ps < PS; ps++) cnt[ps] = ps_count(ps);
    HIP_TRY(m->pf_ndens.upload(cnt.data(), cnt.size()));
  }
  // FP64 planes for the refinement: [pseudo-state][mu_0 | 1/var_0 | ... | norm | logw][density slot]; 1 KB of slack
  // for the LDS-DMA's last piece
  {
    const uint32_t NS = (uint32_t)gmm_refine_slots(std::min(32u, m->max_dens), DP), planes = 2 * DP + 2;
    // padded plane order (gmm_refine_kernel): dimensions 0 .. D - D % 2 - 1 in place, zero planes, an odd D's last dimension in slot
    // DP - 1; a zero plane pair (mean 0, inverse variance 0) contributes +0.0 to the sums
    const uint32_t pairs = D - (D & 1u);
    auto slot_of = [&](uint32_t d) -> uint32_t { return d < pairs ? d : DP - 1u; };
    m->pf_slots = NS;
    // (the packings are built on first use of their kernel: on 16 host threads, a new model's first prefilter call was 170 ms)
    const size_t n_rows_d = (size_t)PS * planes * NS + 128;
    std::unique_ptr<double[]> rows_own(new double[n_rows_d]);
    double* const rows_p = rows_own.get();
    std::fill(rows_p + (size_t)PS * planes * NS, rows_p + n_rows_d, 0.0);
    srhost::parallel_ranges(PS, 64, [&](size_t ps0, size_t ps1) {
    for (uint32_t ps = (uint32_t)ps0; ps < (uint32_t)ps1; ps++) {
      double* r = rows_p + (size_t)ps * planes * NS;
      std::fill(r, r + (size_t)planes * NS, 0.0);
      for (uint32_t i = 0; i < ps_count(ps); i++) {
        const size_t c = (size_t)dens_off[ps / Cs] + 32u * (ps % Cs) + i;
        // density i sits in slot i (round 1 rotated a workgroup's states against each other for a phase in which a wave
        // instruction mixed states; since round 2 every wave instruction evaluates candidates of ONE state, so lanes on
        // different densities hit different bank pairs and lanes on the same density share a broadcast read as it is)
        const uint32_t sl = i;
        for (uint32_t d = 0; d < D; d++) { r[(2 * slot_of(d)) * NS + sl] = means[c * D + d]; r[(2 * slot_of(d) + 1) * NS + sl] = inv_vars[c * D + d]; }
        r[(2 * DP) * NS + sl] = norm[c];
        r[(2 * DP + 1) * NS + sl] = logw[c];
      }
    }
    });
    HIP_TRY(m->pf_rows.upload(rows_p, n_rows_d));
  }
  const uint32_t n_groups = (PS + 3) / 4;
  const float finf = std::numeric_limits<float>::infinity();
  // per density: coefficients a = [1/(2 var); -mu/var] and the constant
  auto coeffs = [&](size_t c, std::vector<double>& arow) -> double {
    double q2 = 0.0;
    for (uint32_t d = 0; d < D; d++) {
      const double mu = means[c * D + d], iv = inv_vars[c * D + d];
      arow[2 * d] = 0.5 * iv;
      arow[2 * d + 1] = -mu * iv;
      q2 += mu * mu * iv;
    }
    return norm[c] - logw[c] + 0.5 * q2;
  };
  // one power-of-two scale for the whole model, the largest finite |coefficient| or |constant| -> [2^13, 2^14)
  double sA = 1.0;
  {
    std::mutex mu_big;
    double big = 0.0;
    srhost::parallel_ranges((size_t)m->n_dens, 4096, [&](size_t c0, size_t c1) {
      std::vector<double> arow(32 * (size_t)KS);
      double mine = 0.0;
      for (size_t c = c0; c < c1; c++) {
        const double konst = coeffs(c, arow);
        if (std::isfinite(konst)) mine = std::max(mine, std::fabs(konst));
        for (uint32_t k = 0; k < 2 * D; k++)
          if (std::isfinite(arow[k])) mine = std::max(mine, std::fabs(arow[k]));
      }
      std::lock_guard<std::mutex> lock(mu_big);
      big = std::max(big, mine);
    });
    if (big > 0.0) sA = std::ldexp(1.0, 13 - std::ilogb(big));
  }
  const size_t blk_bytes = (size_t)KS * 1024;
  std::vector<uint16_t> ap((size_t)n_groups * 8 * blk_bytes / 2, 0);
  // per state slot: sA |a|, sA |konst|, sA |a^ - a|, sA |a^| (a^ = the fp16 coefficients packed below), each the largest over the
  // slot's densities, rounded up -- the candidate limit of gmm_prefilter16_kernel
  constexpr int kNF = 4;
  std::vector<float> anorm(kNF * 4 * (size_t)n_groups, 0.0f);
  auto half_bits = [](double v) { const _Float16 h = (_Float16)(float)v; uint16_t u; memcpy(&u, &h, 2); return u; };
  auto half_value = [](uint16_t u) { _Float16 h; memcpy(&h, &u, 2); return (double)(float)h; };
  auto up = [finf](double v) { return std::nextafter((float)(v * (1.0 + 1e-6)), finf); };
  srhost::parallel_ranges(n_groups, 16, [&](size_t q0, size_t q1) {
  std::vector<double> arow(32 * (size_t)KS);
  for (uint32_t q = (uint32_t)q0; q < (uint32_t)q1; q++) {
    for (uint32_t j = 0; j < 8; j++) {
      const size_t b = (size_t)q * 8 + j;
      for (uint32_t r = 0; r < 16; r++) {
        const uint32_t g = r >> 2, ps = 4 * q + g, i = 4 * j + (r & 3);
        const bool real = ps < PS && i < ps_count(ps);
        const uint32_t st = ps < PS ? ps / Cs : 0;
        std::fill(arow.begin(), arow.end(), 0.0);
        double konst = (double)finf;  // padding slot: never below a real score, masked off again by the refinement
        // A state slot beyond the last pseudo-state has no real score to stay above: with +inf everywhere its minimum is +inf, and
        // inf <= inf + limit made every one of its 32 densities a "candidate" (0xFFFFFFFF in words nobody reads).  Its rows score 0
        // and its limit is negative (below): 0 > 0 - 1, no candidate, the word is 0 for every frame that is a number.
        if (ps >= PS) konst = 0.0;
        if (real) {
          konst = coeffs((size_t)dens_off[st] + 32u * (ps % Cs) + i, arow) * sA;
          double n2 = 0.0, d2 = 0.0, h2 = 0.0;
          for (uint32_t k = 0; k < 2 * D; k++) {
            arow[k] *= sA;
            const double h = half_value(half_bits(arow[k]));  // exactly what the packing below writes
            n2 += arow[k] * arow[k];
            d2 += (h - arow[k]) * (h - arow[k]);
            h2 += h * h;
          }
          const float f[kNF] = {up(std::sqrt(n2)), up(std::fabs(konst)), up(std::sqrt(d2)), up(std::sqrt(h2))};
          // NaN sticks: everything of that state then stays a candidate
          for (int t = 0; t < kNF; t++)
            if (!(f[t] <= anorm[kNF * (4 * q + g) + t])) anorm[kNF * (4 * q + g) + t] = f[t];
        }
        // konst = c1 + c2 + c3 (3 x 11 bits), multiplied by 1 in three spare k slots: exact products
        double rest = konst;
        for (uint32_t t = 0; t < 3; t++) {
          const double c = (real || t == 0) ? half_value(half_bits(rest)) : 0.0;
          arow[2 * D + t] = c;
          rest -= c;
        }
        for (int ks = 0; ks < KS; ks++)
          for (uint32_t kk = 0; kk < 32; kk++) {
            const uint32_t k = 32 * ks + kk;
            const double v = arow[k];
            const uint32_t lane = r + 16 * (kk >> 3), e = kk & 7;
            ap[(b * blk_bytes) / 2 + (size_t)ks * 512 + (size_t)lane * 8 + e] = half_bits(v);
          }
      }
    }
  }
  });
  if (Cs > 1) {  // the candidate test of every chunk uses the whole state's largest norms
    for (uint32_t st = 0; st < S; st++)
      for (int f = 0; f < kNF; f++) {
        float mxv = 0.0f;
        for (uint32_t ch = 0; ch < Cs; ch++) {
          const float v = anorm[kNF * (size_t)(st * Cs + ch) + f];
          if (!(v <= mxv)) mxv = v;
        }
        for (uint32_t ch = 0; ch < Cs; ch++) anorm[kNF * (size_t)(st * Cs + ch) + f] = mxv;
      }
  }
  HIP_TRY(m->pf_apack.upload(reinterpret_cast<const unsigned char*>(ap.data()), ap.size() * 2));
  // -> the candidate limit per state slot, 2 eps = limD |b^ - b| + lim1 |b| + lim0 (gmm_prefilter.hip header).  lim0 and the
  // norm-only lim1 are evaluated in float as the kernel did before; the residual form is taken only where its coefficients, rounded
  // up, stay 2^-12 below the norm-only lim1 with |b^ - b| at its cap, and where kAbs |a| holds what the cap leaves out.  A NaN
  // fails both tests and reaches the limit through lim0 and lim1: every density of that state stays a candidate.
  {
    const PfBound B = pf_bound(KS);
    for (size_t slot = 0; slot < 4 * (size_t)n_groups; slot++) {
      float* v = &anorm[kNF * slot];
      const float na = v[0], nk = v[1], nd = v[2], nh = v[3];
      const float lim0 = 2.0f * (B.acc * nk + B.abs * na), lim1_norm = 2.0f * (B.kappa * na + B.abs);
      const float lim1_res = up(2.0 * ((double)nd + (double)B.acc * nh + (double)B.abs)), limd_res = up(2.0 * (1.0 + (double)B.acc) * nh);
      const bool res = (double)limd_res * kPfRes16 + lim1_res <= lim1_norm * (1.0 - 0x1p-12) &&
                       (1.0 + (double)B.acc) * (double)B.sub * nh <= (double)B.abs * na;
      v[0] = res ? lim1_res : lim1_norm;
      v[1] = res ? limd_res : 0.0f;
      v[2] = lim0;
      v[3] = 0.0f;
      if (slot >= PS) { v[0] = 0.0f; v[1] = 0.0f; v[2] = -1.0f; }  // a slot without a pseudo-state: all rows score 0, none is <= 0 - 1
    }
  }
  HIP_TRY(m->pf_lim.upload(anorm.data(), anorm.size()));
  m->pf_groups = n_groups;
  m->pf_ks32 = KS;
  m->pf_ny = 0;
  return SR_OK;
}

int set_prefilter_splits(sr_model* m, uint32_t nx) {
  const uint32_t target_wgs = 16 * 768;
  uint32_t ny = (target_wgs + nx - 1) / std::max(1u, nx);
  ny = std::max(1u, std::min(ny, std::max(1u, m->pf_groups / 8)));
  if (ny >= 8) ny &= ~7u;
  // one table per split count, kept: launches of different sizes (the pieces of a corpus that is still being fed) alternate
  // between them without touching a table a queued kernel may still read
  auto it = m->pf_split_tabs.find(ny);
  if (it == m->pf_split_tabs.end() || !it->second || !it->second->p) {
    std::vector<uint32_t> sb(ny + 1);
    for (uint32_t y = 0; y <= ny; y++) sb[y] = (uint32_t)((uint64_t)m->pf_groups * y / ny);
    std::unique_ptr<DevBuf<uint32_t>> fresh(new DevBuf<uint32_t>());
    HIP_TRY(fresh->upload(sb.data(), sb.size()));  // (a failed upload leaves no entry behind: the next call tries again)
    it = m->pf_split_tabs.insert_or_assign(ny, std::move(fresh)).first;
  }
  m->pf_split_cur = it->second->p;
  m->pf_ny = ny;
  return SR_OK;
}

// choose the state-range split count for a launch over `nx` frame tiles and upload group-aligned ranges
int set_splits(sr_model* m, uint32_t nx) {
  // Equal-sized workgroups run in rounds of (2 per CU x 256 CUs); aim for ~32 rounds so the last,
  // partly filled round costs ~3 %, but keep >= 32 model blocks (~70 us of MFMA work) per workgroup
  // so the feature-tile prologue stays negligible.
  const uint32_t target_wgs = 32 * 512;
  uint32_t ny = (target_wgs + nx - 1) / std::max(1u, nx);
  ny = std::max(1u, std::min(ny, std::min(m->n_groups, std::max(1u, m->n_blocks / 32))));
  if (ny >= 8) ny &= ~7u;  // multiples of 8 enable the XCD-aware tile map
  auto it = m->split_tabs.find(ny);  // (kept per split count, see set_prefilter_splits)
  if (it == m->split_tabs.end() || !it->second || !it->second->p) {
    std::vector<uint32_t> sb(ny + 1);
    for (uint32_t y = 0; y <= ny; y++) {
      // balance by blocks, cut at group boundaries
      const uint64_t want = (uint64_t)m->n_blocks * y / ny;
      auto it = std::lower_bound(m->group_first_block.begin(), m->group_first_block.end(), (uint32_t)want);
      sb[y] = *it;
    }
    sb[0] = 0;
    sb[ny] = m->n_blocks;
    std::unique_ptr<DevBuf<uint32_t>> fresh(new DevBuf<uint32_t>());
    HIP_TRY(fresh->upload(sb.data(), sb.size()));
    it = m->split_tabs.insert_or_assign(ny, std::move(fresh)).first;
  }
  m->split_cur = it->second->p;
  m->split_ny = ny;
  return SR_OK;
}

int prof_begin(sr_model* m, hipStream_t s, int kind, EventPair* ep) {
  if (!m->profiling) return SR_OK;
  ep->kind = kind;
  HIP_TRY(hipEventCreate(&ep->a));
  HIP_TRY(hipEventCreate(&ep->b));
  HIP_TRY(hipEventRecord(ep->a, s));
  return SR_OK;
}
int prof_end(sr_model* m, hipStream_t s, EventPair* ep) {
  if (!m->profiling) return SR_OK;
  HIP_TRY(hipEventRecord(ep->b, s));
  m->events.push_back(*ep);
  return SR_OK;
}

// kernel-specific model packing (first use) and workspaces for scoring launches of up to n_max frames: growing a
// workspace frees the old one, which must not happen between launches that are still queued
// SR_GMM_DEFAULT for a dense table: the fastest kernel that gives the reference's results -- the bit-exact prefilter path for
// max-approx models; for sum scoring (Mixtures.cpp:719-728) the FP64-MFMA kernel with its fused -log sum exp epilogue, within
// SR_GMM_MFMA's 1e-9 (the direct form stays 1e-12 from the reference's libm in sum mode, at 3x the time: SR_GMM_EXACT on request).
int resolve_dense_kernel(const sr_model* m, int gmm_kernel) {
  if (gmm_kernel == SR_GMM_DEFAULT) gmm_kernel = m->max_approx ? SR_GMM_PREFILTER : SR_GMM_MFMA;
  if (gmm_kernel == SR_GMM_MFMA && m->ksteps == 0) gmm_kernel = SR_GMM_EXACT;  // dimension 64 .. 160: the exact kernel (tighter, not looser)
  return gmm_kernel;
}

// the shape of a refinement launch over n_frames, all that its workspaces depend on
GmmRefineArgs refine_shape(const sr_model* m, uint64_t n_frames) {
  GmmRefineArgs ra{};
  ra.n_frames = n_frames; ra.dim = m->pf_dp; ra.n_pstates = m->pf_pstates; ra.n_slots = m->pf_slots; ra.chunks = m->pf_chunks;
  return ra;
}
// deferred leftovers of a refinement launch over n_frames: entries per segment (0: the route is off), total entries, total counts
struct DeferLayout { uint32_t cap; size_t n_e, n_c; };
DeferLayout defer_layout(const sr_model* m, uint64_t n_frames) {
  DeferLayout d;
  gmm_refine_defer_layout(refine_shape(m, n_frames), m->defer_budget, m->defer_cap_limit, &d.cap, &d.n_e, &d.n_c);
  return d;
}

int reserve_scoring(sr_model* m, int gmm_kernel, uint64_t n_max, int pf_route = -1) {  // pf_route: the model's own unless given
  gmm_kernel = resolve_dense_kernel(m, gmm_kernel);
  if (pf_route < 0) pf_route = m->pf_route;
  if ((gmm_kernel == SR_GMM_MFMA && !m->mfma_packed) || (gmm_kernel == SR_GMM_PREFILTER && !m->pf_packed)) {
    int rc = srhost::ensure_host_tables(m);
    if (rc) return rc;
  }
  if (gmm_kernel == SR_GMM_MFMA && !m->mfma_packed) {
    int rc = pack_model(m, m->h_dens_off.data(), m->h_means.data(), m->h_inv_vars.data(), m->h_norm.data(), m->h_logw.data());
    if (rc) return rc;
    m->mfma_packed = true;
  }
  if (gmm_kernel == SR_GMM_PREFILTER && !m->pf_packed) {
    int rc = pack_prefilter(m, m->h_dens_off.data(), m->h_means.data(), m->h_inv_vars.data(), m->h_norm.data(), m->h_logw.data());
    if (rc) return rc;
    m->pf_packed = true;
  }
  if (gmm_kernel == SR_GMM_PREFILTER && m->pf_ks32 > 0 && n_max > 0) {
    const uint64_t ldT = (n_max + 63) & ~(uint64_t)63;
    const size_t want_T = (size_t)ldT * m->pf_dp, want_mask = (size_t)((m->pf_groups + 1u) & ~1u) * n_max * 4;
    const size_t want_P = m->pf_dp != m->dim ? (size_t)n_max * m->pf_dp + 4 : 0;  // (+4: the rows are read in 16-byte pieces)
    const size_t want_ring = gmm_refine_ring_words(refine_shape(m, n_max));
    if (want_T > m->featsT.n || want_P > m->featsP.n || want_mask > m->pf_mask.n || want_ring > m->pf_ring.n) HIP_TRY(hipStreamSynchronize(m->s_gmm));
    HIP_TRY(m->featsT.ensure(want_T));
    if (want_P) HIP_TRY(m->featsP.ensure(want_P));
    const DeferLayout dl = defer_layout(m, n_max);  // within SRGPU_DEFER_MB (default 32 GiB; 0 switches the route off)
    if (dl.n_e > m->pf_defer.n || dl.n_c > m->pf_defer_cnt.n) HIP_TRY(hipStreamSynchronize(m->s_gmm));
    if (dl.n_e) { HIP_TRY(m->pf_defer.ensure(dl.n_e)); HIP_TRY(m->pf_defer_cnt.ensure(dl.n_c)); }
    HIP_TRY(m->pf_mask.ensure(want_mask));  // the refinement reads group pairs
    HIP_TRY(m->pf_ring.ensure(want_ring));
    if (gmm_prefilter_route(m->pf_ks32, pf_route) == kPfStationary) {
      size_t want_frag, want_norm;
      gmm_prefilter_operand_sizes(m->pf_ks32, n_max, &want_frag, &want_norm);
      if (want_frag > m->pf_bfrag.n || want_norm > m->pf_bnorm.n) HIP_TRY(hipStreamSynchronize(m->s_gmm));
      HIP_TRY(m->pf_bfrag.ensure(want_frag));
      HIP_TRY(m->pf_bnorm.ensure(want_norm));
    }
  }
  return SR_OK;
}

// the prefilter's arguments for a launch over n_frames (either route; the workspaces are reserve_scoring's)
int prefilter_args(sr_model* m, const float* d_feats, uint64_t n_frames, GmmPrefilterArgs* pa) {
  const uint32_t tile = gmm_prefilter_frames_per_tile();
  const uint32_t nx = (uint32_t)((n_frames + tile - 1) / tile);
  int rc = set_prefilter_splits(m, nx);
  if (rc) return rc;
  pa->feats = d_feats; pa->n_frames = n_frames; pa->dim = m->dim;
  pa->apack = m->pf_apack.p; pa->grp_lim = m->pf_lim.p; pa->split_begin = m->pf_split_cur;
  pa->mask = m->pf_mask.p; pa->nx = nx; pa->ny = m->pf_ny; pa->chunks = std::min(4u, m->pf_chunks);
  pa->n_groups = m->pf_groups; pa->bfrag = m->pf_bfrag.p; pa->bnorm = m->pf_bnorm.p;
  return SR_OK;
}

// the refinement's arguments for a launch over n_frames into d_out (row stride m->ld; the workspaces are reserve_scoring's): the feature
// buffers launch_transpose_feats fills, the deferred-leftover segments where their layout (SRGPU_DEFER_MB / SRGPU_DEFER_CAP) fits what is
// reserved, the evaluation counter while profiling
GmmRefineArgs refine_args(sr_model* m, const float* d_feats, uint64_t n_frames, double* d_out) {
  GmmRefineArgs ra = refine_shape(m, n_frames);
  const bool padded = m->pf_dp != m->dim;
  ra.feats = padded ? m->featsP.p : d_feats; ra.featsT = m->featsT.p; ra.n_frames_ld = (n_frames + 63) & ~(uint64_t)63;
  ra.n_dens_ps = m->pf_ndens.p; ra.rows = m->pf_rows.p;
  ra.mask = m->pf_mask.p; ra.out = d_out; ra.ld = m->ld;
  ra.n_refined = m->profiling ? m->pf_counter.p : nullptr;
  ra.ring = m->pf_ring.p;
  const DeferLayout dl = defer_layout(m, n_frames);
  if (dl.cap && dl.n_e <= m->pf_defer.n && dl.n_c <= m->pf_defer_cnt.n) { ra.defer = m->pf_defer.p; ra.defer_cnt = m->pf_defer_cnt.p; ra.defer_cap = dl.cap; }
  return ra;
}

// score frames [f_begin, f_end) of `feats` into `out` (device, row stride m->ld) on stream s_gmm
int launch_scoring(sr_model* m, const float* d_feats, uint64_t n_frames, int gmm_kernel, double* d_out) {
  if (n_frames == 0) return SR_OK;
  gmm_kernel = resolve_dense_kernel(m, gmm_kernel);
  EventPair ep{};
  {
    int rc = reserve_scoring(m, gmm_kernel, n_frames);
    if (rc) return rc;
  }
  if (gmm_kernel == SR_GMM_MFMA) {
    const uint32_t tile = gmm_mfma_frames_per_tile(m->ksteps);
    const uint32_t nx = (uint32_t)((n_frames + tile - 1) / tile);
    int rc = set_splits(m, nx);
    if (rc) return rc;
    GmmMfmaArgs a{};
    a.feats = d_feats; a.n_frames = n_frames; a.dim = m->dim;
    a.apack = m->apack.p; a.blk_meta = m->blk_meta.p; a.grp_state = m->grp_state.p; a.split_begin = m->split_cur;
    a.out = d_out; a.ld = m->ld; a.nx = nx; a.ny = m->split_ny;
    if ((rc = prof_begin(m, m->s_gmm, 0, &ep))) return rc;
    HIP_TRY(launch_gmm_mfma(a, m->ksteps, !m->max_approx, m->s_gmm));
    if ((rc = prof_end(m, m->s_gmm, &ep))) return rc;
  } else if (gmm_kernel == SR_GMM_PREFILTER && m->pf_ks32 > 0) {
    GmmPrefilterArgs pa{};
    int rc = prefilter_args(m, d_feats, n_frames, &pa);
    if (rc) return rc;
    const GmmRefineArgs ra = refine_args(m, d_feats, n_frames, d_out);
    const uint64_t ldT = ra.n_frames_ld;
    const bool padded = m->pf_dp != m->dim;
    if (m->profiling) m->prof.refined_pairs += n_frames * (uint64_t)m->n_states;
    EventPair ep_p{}, ep_r{};
    if ((rc = prof_begin(m, m->s_gmm, 0, &ep))) return rc;
    if ((rc = prof_begin(m, m->s_gmm, 2, &ep_p))) return rc;
    HIP_TRY(launch_transpose_feats(d_feats, n_frames, m->dim, m->pf_dp, ldT, m->featsT.p, padded ? m->featsP.p : nullptr, m->s_gmm));
    HIP_TRY(launch_gmm_prefilter(pa, m->pf_ks32, m->pf_route, m->s_gmm));
    if ((rc = prof_end(m, m->s_gmm, &ep_p))) return rc;
    if ((rc = prof_begin(m, m->s_gmm, 3, &ep_r))) return rc;
    HIP_TRY(launch_gmm_refine(ra, m->s_gmm));
    if ((rc = prof_end(m, m->s_gmm, &ep_r))) return rc;
    if ((rc = prof_end(m, m->s_gmm, &ep))) return rc;
  } else if (gmm_kernel == SR_GMM_EXACT || gmm_kernel == SR_GMM_PREFILTER) {
    // (a model the prefilter cannot take -- sum scoring, > 256 densities per mixture (> 128 beyond dim 39), dim > 62, or a device that fails
    // the fp16 probes -- is scored by the exact kernel: same bits, FP64 VALU speed)
    GmmExactArgs a{};
    a.feats = d_feats; a.n_frames = n_frames; a.dim = m->dim; a.n_states = m->n_states;
    a.dens_off = m->dens_off.p; a.means = m->means.p; a.inv_vars = m->inv_vars.p; a.norm = m->norm.p; a.logw = m->logw.p;
    a.out = d_out; a.ld = m->ld;
    const uint32_t nx = (uint32_t)((n_frames + 255) / 256);
    uint32_t ny = std::max(1u, std::min(m->n_states, (4096 + nx - 1) / nx));
    a.states_per_split = (m->n_states + ny - 1) / ny;
    ny = (m->n_states + a.states_per_split - 1) / a.states_per_split;
    int rc;
    if ((rc = prof_begin(m, m->s_gmm, 0, &ep))) return rc;
    HIP_TRY(launch_gmm_exact(a, !m->max_approx, ny, m->s_gmm));
    if ((rc = prof_end(m, m->s_gmm, &ep))) return rc;
  } else {
    return fail(SR_EINVAL, "unknown gmm_kernel %d", gmm_kernel);
  }
  if (m->profiling) m->prof.gmm_flops += 4.0 * m->dim * (double)m->n_dens * (double)n_frames;
  return SR_OK;
}

// utterance chunks whose score table fits the workspace
using srplan::Chunk;
std::vector<Chunk> make_chunks(const sr_corpus* c, size_t chunk_frames) {
  std::vector<Chunk> out;
  // chunks of whole utterances, at most chunk_frames each (a longer utterance is a chunk of its own), and of about equal size
  // when several are needed: the search of chunk i runs beside the scoring of chunk i+1, and a short last chunk leaves the
  // long one's search without company (configs[4]: 147 ms per step with 16 + 3.4 GB chunks, 138.5 with 2 x 9.7)
  const uint64_t total = c->n_frames;
  const uint64_t n_target = std::max<uint64_t>(1, (total + chunk_frames - 1) / std::max<size_t>(1, chunk_frames));
  const uint64_t even = (total + n_target - 1) / n_target;
  uint32_t u = 0;
  while (u < c->n_utts) {
    uint32_t v = u + 1;
    while (v < c->n_utts && c->frame_off[v + 1] - c->frame_off[u] <= chunk_frames && c->frame_off[v] - c->frame_off[u] < even) v++;
    out.push_back({u, v, c->frame_off[u], c->frame_off[v]});
    u = v;
  }
  return out;
}

// One workgroup searches / aligns one utterance, and a launch has only a few workgroups per CU (configs[2]: 1000 utterances of
// 200..400 frames on 256 CUs): handed out in corpus order, the last CU finishes ~19 % after the average one.  Every launch range
// is therefore walked longest utterance first (ties in corpus order); results do not depend on the order.
int ensure_utt_order(sr_model* m, sr_corpus* c, const std::vector<Chunk>& chunks) {
  if (c->order_chunk_frames == m->chunk_frames && c->utt_order.p) return SR_OK;
  std::vector<uint32_t> order(c->n_utts);
  for (uint32_t u = 0; u < c->n_utts; u++) order[u] = u;
  for (const Chunk& ch : chunks)
    std::stable_sort(order.begin() + ch.u0, order.begin() + ch.u1, [&](uint32_t a, uint32_t b) {
      return c->frame_off[a + 1] - c->frame_off[a] > c->frame_off[b + 1] - c->frame_off[b];
    });
  HIP_TRY(c->utt_order.upload(order.data(), order.size()));
  c->order_chunk_frames = m->chunk_frames;
  return SR_OK;
}

// Scores frames [f0, f1) of the corpus into `table` (row 0 = frame f0).  While the feeder is still copying
// (sr_corpus_upload_async) the range is scored in four launches -- the first 1/24, up to the sixth, up to the half, the rest -- each
// waiting on the device only for its own pieces: scoring starts ~1 ms into the transfer and the rest of it hides behind
// the kernels (the feeder delivers 5-10 GB/s, scoring consumes 2 GB/s of features).  The search that follows sees one table.
int score_chunk(sr_model* m, sr_corpus* c, uint64_t f0, uint64_t f1, int gmm_kernel, double* table) {
  const uint64_t n = f1 - f0;
  uint64_t cuts[4] = {f1, f1, f1, f1};
  int n_cuts = 1;
  // (the first launch is what the transfer cannot hide behind: 1/24 of the chunk = 2 MB of configs[2]'s features, 0.3 ms of
  // staging copy + PCIe instead of the 1.1 ms the first sixth took)
  if (srhost::corpus_upload_in_flight(c) && n >= 24 * 2048) { cuts[0] = f0 + n / 24; cuts[1] = f0 + n / 6; cuts[2] = f0 + n / 2; n_cuts = 4; }
  int rc = reserve_scoring(m, gmm_kernel, n_cuts == 4 ? n - n / 2 : n);
  if (rc) return rc;
  uint64_t a = f0;
  for (int i = 0; i < n_cuts; i++) {
    if ((rc = srhost::corpus_ready(c, a, cuts[i], m->s_gmm))) return rc;
    if ((rc = launch_scoring(m, c->feats.p + a * m->dim, cuts[i] - a, gmm_kernel, table + (a - f0) * m->ld))) return rc;
    a = cuts[i];
  }
  return SR_OK;
}

// the chunks of a pass over the corpus, with their score buffers (two when there is more than one chunk) and launch order
int prepare_chunks(sr_model* m, sr_corpus* c, std::vector<Chunk>* chunks) {
  *chunks = make_chunks(c, m->chunk_frames);
  uint64_t mx = 0;
  for (const Chunk& ch : *chunks) mx = std::max(mx, ch.f1 - ch.f0);
  const int nbuf = chunks->size() > 1 ? 2 : 1;
  for (int i = 0; i < nbuf; i++) HIP_TRY(m->scores[i].ensure((size_t)mx * m->ld));
  return ensure_utt_order(m, c, *chunks);
}

// The pass itself: chunk i is scored on s_gmm into buffer i & 1 while chunk i-1 is searched on s_search (on s_gmm after it with
// SRGPU_OVERLAP=0).  ev_scored hands a buffer to the search; ev_consumed hands it back to the scoring two chunks later.
//   score(const Chunk&, double* table)                           enqueues the chunk's scores on s_gmm
//   search(const Chunk&, const double* table, hipStream_t s)     enqueues its search on s (kind-1 profiling window)
//   tail(hipStream_t s)                                          enqueues what follows the last chunk's search on its stream, outside
//                                                                the profiling windows (the compaction of the words)
template <class Score, class Search, class Tail>
int run_chunks(sr_model* m, const std::vector<Chunk>& chunks, Score score, Search search, Tail tail) {
  const hipStream_t s_search = m->overlap ? m->s_search : m->s_gmm;
  int rc;
  for (size_t i = 0; i < chunks.size(); i++) {
    const int buf = (int)(i & 1);
    if (i >= 2) HIP_TRY(hipStreamWaitEvent(m->s_gmm, m->ev_consumed[buf], 0));
    if ((rc = score(chunks[i], m->scores[buf].p))) return rc;
    HIP_TRY(hipEventRecord(m->ev_scored[buf], m->s_gmm));
    HIP_TRY(hipStreamWaitEvent(s_search, m->ev_scored[buf], 0));
    EventPair ep{};
    if ((rc = prof_begin(m, s_search, 1, &ep))) return rc;
    if ((rc = search(chunks[i], m->scores[buf].p, s_search))) return rc;
    if ((rc = prof_end(m, s_search, &ep))) return rc;
    HIP_TRY(hipEventRecord(m->ev_consumed[buf], s_search));
  }
  if ((rc = tail(s_search))) return rc;
  HIP_TRY(hipStreamSynchronize(m->s_search));
  HIP_TRY(hipStreamSynchronize(m->s_gmm));
  return SR_OK;
}
template <class Score, class Search>
int run_chunks(sr_model* m, const std::vector<Chunk>& chunks, Score score, Search search) {
  return run_chunks(m, chunks, score, search, [](hipStream_t) { return (int)SR_OK; });
}

}  // namespace
namespace srhost {
static void swap_spare(sr_corpus* c, CorpusSpare& sp) {
  c->feats.swap(sp.feats); c->d_frame_off.swap(sp.d_frame_off); c->utt_order.swap(sp.utt_order); c->out_words.swap(sp.out_words);
  c->out_count.swap(sp.out_count); c->out_flags.swap(sp.out_flags); c->tb_score.swap(sp.tb_score); c->tb_word.swap(sp.tb_word);
  c->tb_bkp.swap(sp.tb_bkp); c->gather_off.swap(sp.gather_off); c->result.swap(sp.result);
}
void corpus_register(sr_corpus* c) {
  sr_model* m = c->model;
  std::lock_guard<std::mutex> lk(m->spare_mu);
  m->corpora.push_back(c);
}
void corpus_adopt_spare(sr_corpus* c) {
  sr_model* m = c->model;
  std::unique_ptr<CorpusSpare> sp;
  { std::lock_guard<std::mutex> lk(m->spare_mu); sp = std::move(m->spare); }
  if (sp) swap_spare(c, *sp);  // (whatever the new corpus held -- nothing -- goes away with sp)
  c->order_chunk_frames = 0;   // the launch order is rebuilt for the new utterances
}
size_t corpus_spare_cap_bytes() {
  static const size_t cap = [] {
    const char* e = getenv("SRGPU_SPARE_MB");
    const long mb = e ? atol(e) : 256;
    return (size_t)(mb < 0 ? 0 : mb) << 20;
  }();
  return cap;
}
void corpus_donate_spare(sr_corpus* c) {
  sr_model* m = c->model;  // (srgpu.h: a corpus is destroyed BEFORE its model)
  if (!m) return;
  std::unique_ptr<CorpusSpare> sp(new CorpusSpare());
  swap_spare(c, *sp);
  std::lock_guard<std::mutex> lk(m->spare_mu);
  m->corpora.erase(std::remove(m->corpora.begin(), m->corpora.end(), c), m->corpora.end());
  if (sp->bytes() > corpus_spare_cap_bytes()) {
    // too big to keep: freed on return -- all but the result block, 4 bytes per frame and, being pinned, the dearest to get again
    std::unique_ptr<CorpusSpare> small(new CorpusSpare());
    small->result.swap(sp->result); small->gather_off.swap(sp->gather_off);
    sp = std::move(small);
    if (sp->bytes() > corpus_spare_cap_bytes()) return;
  }
  if (!m->spare) m->spare = std::move(sp);  // (else: one spare set is kept, this one is freed on return)
}
}  // namespace srhost
namespace {

int check_model(const sr_model* m) {
  if (!m) return fail(SR_EINVAL, "null model handle");
  HIP_TRY(hipSetDevice(m->device));
  return SR_OK;
}
int check_corpus(const sr_model* m, const sr_corpus* c) {
  int rc = check_model(m);
  if (rc) return rc;
  if (!c || c->model != m) return fail(SR_EINVAL, "corpus does not belong to this model");
  return SR_OK;
}

}  // namespace

const char* sr_last_error(void) { return g_err; }

int sr_abi_version(void) { return SR_ABI_VERSION; }

int sr_device_count(int* count) {
  return guarded(__func__, [&]() -> int {
  if (!count) return fail(SR_EINVAL, "count is null");
  int n = 0;
  hipError_t e = hipGetDeviceCount(&n);
  if (e != hipSuccess) { *count = 0; return fail(SR_ENODEV, "hipGetDeviceCount: %s", hipGetErrorString(e)); }
  *count = n;
  return SR_OK;
  });
}

namespace srhost {

// A model handle with everything but the four parameter tables: device checks, streams, events, dens_off, chunk sizes.
// sr_model_create uploads host tables into it; the device-side finalize (em_finalize.hip) fills them where they are.
int model_shell(int device, uint32_t dim, uint32_t n_states, const uint32_t* dens_off, int max_approx, sr_model** out) {
  *out = nullptr;
  if (!dens_off) return fail(SR_EINVAL, "null model table");
  if (dim == 0 || n_states == 0) return fail(SR_EINVAL, "dim and n_states must be positive");
  // (0 beyond dimension 63: no dense FP64-MFMA instantiation -- SR_GMM_MFMA is then answered by the exact kernel, resolve_dense_kernel)
  const int ks = gmm_mfma_ksteps_for_dim(dim);
  if (dim > 160) return fail(SR_ELIMIT, "dim %u unsupported (max 160: the exact kernel keeps a workgroup's frames in LDS)", dim);
  if (dens_off[0] != 0) return fail(SR_EINVAL, "dens_off[0] must be 0");
  for (uint32_t s = 0; s < n_states; s++)
    if (dens_off[s + 1] < dens_off[s]) return fail(SR_EINVAL, "dens_off must be non-decreasing (state %u)", s);
  const uint64_t C = dens_off[n_states];
  if (C >= (1ull << 31)) return fail(SR_ELIMIT, "too many densities");
  int ndev = 0;
  if (hipGetDeviceCount(&ndev) != hipSuccess || ndev == 0) return fail(SR_ENODEV, "no HIP device visible");
  if (device < 0 || device >= ndev) return fail(SR_EINVAL, "device %d out of range (0..%d)", device, ndev - 1);
  hipDeviceProp_t prop;
  HIP_TRY(hipGetDeviceProperties(&prop, device));
  if (strncmp(prop.gcnArchName, "gfx950", 6) != 0)
    return fail(SR_ENODEV, "device %d is %s; libsrgpu is built for gfx950 (MI355X) only", device, prop.gcnArchName);
  HIP_TRY(hipSetDevice(device));
  sr_model* m = new sr_model();
  std::unique_ptr<sr_model, int (*)(sr_model*)> own(m, sr_model_destroy);  // released on success; an exception frees it
  m->device = device; m->dim = dim; m->n_states = n_states; m->n_dens = C; m->max_approx = max_approx != 0;
  m->ksteps = ks;
  m->ld = (n_states + 7u) & ~7u;  // 64-byte rows pieces for the kernels that write 8 states per thread
  hipError_t e;
  if ((e = hipStreamCreateWithFlags(&m->s_gmm, hipStreamNonBlocking)) != hipSuccess ||
      (e = hipStreamCreateWithFlags(&m->s_search, hipStreamNonBlocking)) != hipSuccess)
    return fail(SR_EHIP, "hipStreamCreate: %s", hipGetErrorString(e));
  for (int i = 0; i < 2; i++)
    if ((e = hipEventCreateWithFlags(&m->ev_scored[i], hipEventDisableTiming)) != hipSuccess ||
        (e = hipEventCreateWithFlags(&m->ev_consumed[i], hipEventDisableTiming)) != hipSuccess)
      return fail(SR_EHIP, "hipEventCreate: %s", hipGetErrorString(e));
  if ((e = m->dens_off.upload(dens_off, n_states + 1)) != hipSuccess) return fail(SR_EHIP, "model upload: %s", hipGetErrorString(e));
  uint32_t mx = 0;
  for (uint32_t s = 0; s < n_states; s++) mx = std::max(mx, dens_off[s + 1] - dens_off[s]);
  m->max_dens = std::max(1u, mx);
  m->h_dens_off.assign(dens_off, dens_off + n_states + 1);
  const char* env = getenv("SRGPU_SCORE_CHUNK_MB");
  // score workspace per chunk: 48 GiB by default, at most a sixth of the device's memory (two such buffers only when a
  // corpus needs more than one chunk, and the candidate masks of a chunk take up to as much again).  Bigger chunks mean
  // fewer, longer launches (configs[4]'s 19.4 GB table: 136.8 ms per step in one chunk, 147.1 in 16 + 3.4 GB) and MI355X has
  // 288 GB of HBM to spend.
  size_t chunk_bytes = (size_t)49152 << 20;
  {
    size_t free_b = 0, total_b = 0;
    if (hipMemGetInfo(&free_b, &total_b) == hipSuccess && total_b) chunk_bytes = std::min(chunk_bytes, total_b / 6);
  }
  if (env) chunk_bytes = (size_t)atol(env) << 20;
  m->chunk_frames = std::max<size_t>(1, chunk_bytes / ((size_t)m->ld * sizeof(double)));
  // the refinement kernel addresses the transposed feature copy of a chunk with 32-bit buffer offsets
  m->chunk_frames = std::min<size_t>(m->chunk_frames, ((size_t)1 << 32) / (4 * (size_t)dim) - 128);
  if (const char* ov = getenv("SRGPU_OVERLAP")) m->overlap = atoi(ov) != 0;
  if (const char* e = getenv("SRGPU_PREFILTER")) {  // which way round the fp16 prefilter runs (same masks; for measuring)
    if (!strcmp(e, "staged")) m->pf_route = kPfStaged;
    else if (!strcmp(e, "stationary")) m->pf_route = kPfStationary;
    else return fail(SR_EINVAL, "SRGPU_PREFILTER=%s: staged or stationary", e);
  }
  if (const char* e = getenv("SRGPU_GATHER")) {  // where a recognition call's words are compacted (same output; for measuring)
    if (!strcmp(e, "host")) m->gather_device = false;
    else if (!strcmp(e, "device")) m->gather_device = true;
    else return fail(SR_EINVAL, "SRGPU_GATHER=%s: host or device", e);
  }
  if (const char* e = getenv("SRGPU_DEFER_MB")) m->defer_budget = (size_t)strtoull(e, nullptr, 10) << 20;
  if (const char* e = getenv("SRGPU_FB_MB")) m->fb_budget = std::max<size_t>(1, (size_t)strtoull(e, nullptr, 10)) << 20;
  if (const char* e = getenv("SRGPU_MLLT_MB")) m->mllt_budget = std::max<size_t>(1, (size_t)strtoull(e, nullptr, 10)) << 20;
  if (const char* e = getenv("SRGPU_LDA_MB")) m->lda_budget = std::max<size_t>(1, (size_t)strtoull(e, nullptr, 10)) << 20;
  m->vtln_budget = chunk_bytes / 4;
  if (const char* e = getenv("SRGPU_VTLN_KB")) m->vtln_budget = (size_t)strtoull(e, nullptr, 10) << 10;  // (tests: several chunks of warps)
  m->vtln_timing = getenv("SRGPU_VTLN_TIMING") != nullptr;  // (tools/vtln_time.py, and the tests' count of chunks)
  if (const char* e = getenv("SRGPU_DEFER_CAP")) m->defer_cap_limit = std::max(1u, (uint32_t)strtoul(e, nullptr, 10));  // (tests: full segments)
  *out = own.release();
  return SR_OK;
}

// host copies of the parameter tables, for the kernel-specific packings: a model finalised on the device has none until
// a packing is asked for
int ensure_host_tables(sr_model* m) {
  const size_t C = m->n_dens, D = m->dim;
  if (m->h_norm.size() == C && m->h_means.size() == C * D) return SR_OK;
  m->h_means.resize(C * D); m->h_inv_vars.resize(C * D); m->h_norm.resize(C); m->h_logw.resize(C);
  if (C == 0) return SR_OK;
  HIP_TRY(hipMemcpy(m->h_means.data(), m->means.p, C * D * sizeof(double), hipMemcpyDeviceToHost));
  HIP_TRY(hipMemcpy(m->h_inv_vars.data(), m->inv_vars.p, C * D * sizeof(double), hipMemcpyDeviceToHost));
  HIP_TRY(hipMemcpy(m->h_norm.data(), m->norm.p, C * sizeof(double), hipMemcpyDeviceToHost));
  HIP_TRY(hipMemcpy(m->h_logw.data(), m->logw.p, C * sizeof(double), hipMemcpyDeviceToHost));
  return SR_OK;
}

// Can an emission cost of this model be negative (or not a number)?  The search kernels' collapsed word-boundary transition rests on
// costs >= 0 (Recognizer.cpp:143,173: the early-out is inert then); a model that can break it is searched by the variant that replays
// the early-out (viterbi_words.hip, NEG) instead of being flagged utterance by utterance.  A density's score is
// fl(fl(norm + dist / 2) - logw) with dist >= 0 whenever every inverse variance is >= 0, and rounding is monotone, so
// fl(norm - logw) >= 0 for every density rules negative costs out (a variance <= 0 or NaN makes norm -inf or NaN: caught).  Sum
// scoring (Mixtures.cpp:719-728) lies up to log(#densities) below the smallest density score.
int may_go_negative(sr_model* m, bool* out) {
  if (m->neg_possible < 0) {
    const size_t C = m->n_dens;
    std::vector<double> norm_l, logw_l;
    const double *norm = m->h_norm.data(), *logw = m->h_logw.data();
    if (m->h_norm.size() != C || m->h_logw.size() != C) {
      norm_l.resize(C); logw_l.resize(C);
      if (C) {
        HIP_TRY(hipMemcpy(norm_l.data(), m->norm.p, C * sizeof(double), hipMemcpyDeviceToHost));
        HIP_TRY(hipMemcpy(logw_l.data(), m->logw.p, C * sizeof(double), hipMemcpyDeviceToHost));
      }
      norm = norm_l.data(); logw = logw_l.data();
    }
    bool neg = false;
    for (uint32_t s = 0; s < m->n_states && !neg; s++) {
      const uint32_t c0 = m->h_dens_off[s], c1 = m->h_dens_off[s + 1];
      const double slack = m->max_approx ? 0.0 : std::log((double)std::max(1u, c1 - c0)) + 1e-6;
      for (uint32_t c = c0; c < c1; c++)
        if (!(norm[c] - logw[c] - slack >= 0.0)) { neg = true; break; }
    }
    // tables handed in through sr_model_create are taken as they are: a negative or NaN inverse variance there
    if (!neg && m->h_inv_vars.size() == C * (size_t)m->dim)
      for (double iv : m->h_inv_vars)
        if (!(iv >= 0.0)) { neg = true; break; }
    m->neg_possible = neg ? 1 : 0;
  }
  *out = m->neg_possible == 1;
  return SR_OK;
}

}  // namespace srhost

int sr_model_create(int device, uint32_t dim, uint32_t n_states, const uint32_t* dens_off, const double* means,
                    const double* inv_vars, const double* norm, const double* logw, int max_approx, sr_model** out) {
  return guarded(__func__, [&]() -> int {
  if (!out) return fail(SR_EINVAL, "out is null");
  *out = nullptr;
  if (!dens_off || !means || !inv_vars || !norm || !logw) return fail(SR_EINVAL, "null model table");
  sr_model* m = nullptr;
  int rc = srhost::model_shell(device, dim, n_states, dens_off, max_approx, &m);
  if (rc != SR_OK) return rc;
  std::unique_ptr<sr_model, int (*)(sr_model*)> own(m, sr_model_destroy);
  const uint64_t C = m->n_dens;
  hipError_t e;
  if ((e = m->means.upload(means, C * dim)) != hipSuccess || (e = m->inv_vars.upload(inv_vars, C * dim)) != hipSuccess ||
      (e = m->norm.upload(norm, C)) != hipSuccess || (e = m->logw.upload(logw, C)) != hipSuccess)
    return fail(SR_EHIP, "model upload: %s", hipGetErrorString(e));
  m->h_means.assign(means, means + C * dim);
  m->h_inv_vars.assign(inv_vars, inv_vars + C * dim);
  m->h_norm.assign(norm, norm + C);
  m->h_logw.assign(logw, logw + C);
  std::vector<uint32_t> ident(C);
  std::iota(ident.begin(), ident.end(), 0u);
  m->n_mean = m->n_var = (uint32_t)C;
  m->h_dens_mean = ident; m->h_dens_var = ident;
  if ((e = m->dens_mean.upload(ident.data(), C)) != hipSuccess || (e = m->dens_var.upload(ident.data(), C)) != hipSuccess)
    return fail(SR_EHIP, "tying upload: %s", hipGetErrorString(e));
  *out = own.release();
  return SR_OK;
  });
}

int sr_model_destroy(sr_model* m) {
  return guarded(__func__, [&]() -> int {
  if (!m) return SR_OK;
  (void)hipSetDevice(m->device);
  (void)hipDeviceSynchronize();
  for (auto& ep : m->events) { (void)hipEventDestroy(ep.a); (void)hipEventDestroy(ep.b); }
  {  // corpora that outlive the model (srgpu.h asks for the other order) must not reach into it when they are destroyed
    std::lock_guard<std::mutex> lk(m->spare_mu);
    for (sr_corpus* c : m->corpora) c->model = nullptr;
    m->corpora.clear();
  }
  m->dens_mean.release(); m->dens_var.release();
  m->dens_off.release(); m->means.release(); m->inv_vars.release(); m->norm.release(); m->logw.release();
  m->apack.release(); m->blk_meta.release(); m->grp_state.release();
  m->scores[0].release(); m->scores[1].release();
  for (int i = 0; i < 2; i++) {
    if (m->ev_scored[i]) (void)hipEventDestroy(m->ev_scored[i]);
    if (m->ev_consumed[i]) (void)hipEventDestroy(m->ev_consumed[i]);
  }
  for (int b = 0; b < 2; b++) {
    if (m->staging_free[b]) (void)hipEventDestroy(m->staging_free[b]);
    if (m->staging[b]) (void)hipHostFree(m->staging[b]);
  }
  if (m->s_copy) (void)hipStreamDestroy(m->s_copy);
  if (m->s_gmm) (void)hipStreamDestroy(m->s_gmm);
  if (m->s_search) (void)hipStreamDestroy(m->s_search);
  delete m;
  return SR_OK;
  });
}

int sr_model_info(const sr_model* m, uint32_t* dim, uint32_t* n_states, uint64_t* n_densities) {
  return guarded(__func__, [&]() -> int {
  if (!m) return fail(SR_EINVAL, "null model handle");
  if (dim) *dim = m->dim;
  if (n_states) *n_states = m->n_states;
  if (n_densities) *n_densities = m->n_dens;
  return SR_OK;
  });
}

int sr_corpus_upload(sr_model* m, const float* feats, const uint64_t* frame_off, uint32_t n_utts, sr_corpus** out) {
  return guarded(__func__, [&]() -> int {
  if (!out) return fail(SR_EINVAL, "out is null");
  *out = nullptr;
  int rc = check_model(m);
  if (rc) return rc;
  if (!frame_off) return fail(SR_EINVAL, "frame_off is null");
  if (frame_off[0] != 0) return fail(SR_EINVAL, "frame_off[0] must be 0");
  for (uint32_t u = 0; u < n_utts; u++) {
    if (frame_off[u + 1] < frame_off[u]) return fail(SR_EINVAL, "frame_off must be non-decreasing (utterance %u)", u);
    if (frame_off[u + 1] - frame_off[u] > 65535)
      return fail(SR_ELIMIT, "utterance %u has %llu frames; back pointers are 16 bit like the reference's Book::bkp (max 65535)",
                  u, (unsigned long long)(frame_off[u + 1] - frame_off[u]));
  }
  const uint64_t F = frame_off[n_utts];
  if (F > 0 && !feats) return fail(SR_EINVAL, "feats is null");
  sr_corpus* c = new sr_corpus();
  std::unique_ptr<sr_corpus, int (*)(sr_corpus*)> own(c, sr_corpus_destroy);
  c->model = m; c->n_utts = n_utts; c->n_frames = F;
  srhost::corpus_register(c);
  c->frame_off.assign(frame_off, frame_off + n_utts + 1);
  srhost::corpus_adopt_spare(c);
  hipError_t e;
  if ((e = c->feats.ensure((size_t)F * m->dim + 64)) != hipSuccess ||
      (F > 0 && (e = hipMemcpy(c->feats.p, feats, (size_t)F * m->dim * sizeof(float), hipMemcpyHostToDevice)) != hipSuccess) ||
      (e = c->d_frame_off.upload(frame_off, n_utts + 1)) != hipSuccess)
    return fail(SR_EHIP, "corpus upload: %s", hipGetErrorString(e));
  *out = own.release();
  return SR_OK;
  });
}

int sr_model_trim(sr_model* m) {
  return guarded(__func__, [&]() -> int {
  int rc = check_model(m);
  if (rc) return rc;
  HIP_TRY(hipDeviceSynchronize());
  std::unique_ptr<CorpusSpare> sp;
  { std::lock_guard<std::mutex> lk(m->spare_mu); sp = std::move(m->spare); }
  // ... and the refinement's deferred-leftover segments (23 GB at configs[4]); the next scoring call allocates them again
  m->pf_defer.release(); m->pf_defer_cnt.release();
  return SR_OK;  // (sp's buffers are freed here)
  });
}

int sr_corpus_destroy(sr_corpus* c) {
  return guarded(__func__, [&]() -> int {
  if (!c) return SR_OK;
  srhost::feeder_join(c);  // an upload still in flight borrows the caller's buffer and writes into c->feats
  if (c->model) { (void)hipSetDevice(c->model->device); (void)hipDeviceSynchronize(); }
  srhost::corpus_donate_spare(c);  // the search-path buffers stay with the model for its next corpus
  c->feats.release(); c->d_frame_off.release(); c->tb_score.release(); c->tb_word.release(); c->tb_bkp.release();
  c->out_words.release(); c->out_count.release(); c->out_flags.release(); c->automata.release(); c->out_states.release();
  c->aut_off.release(); c->bp_off.release(); c->al_blk_frame0.release(); c->al_list_off.release(); c->al_states.release();
  c->al_blk_frames.release(); c->al_blk_list.release(); c->backptr.release(); c->out_cost.release(); c->path_scores.release();
  c->pair_off.release(); c->pair_frame.release(); c->key_mean.release(); c->key_var.release(); c->iota.release();
  c->keys_sorted.release(); c->pairs_sorted.release(); c->row_begin.release(); c->pair_w.release(); c->acc_mean.release(); c->acc_var.release();
  c->w_mean.release(); c->w_var.release(); c->sort_temp.release();
  delete c;
  return SR_OK;
  });
}

int sr_score_corpus(sr_model* m, sr_corpus* c, int gmm_kernel, double* out) {
  return guarded(__func__, [&]() -> int {
  int rc = check_corpus(m, c);
  if (rc) return rc;
  if (!out && c->n_frames) return fail(SR_EINVAL, "out is null");
  // chunk over plain frame ranges; utterance boundaries do not matter for scoring
  const uint64_t F = c->n_frames;
  const size_t step = m->chunk_frames;
  HIP_TRY(m->scores[0].ensure((size_t)std::min<uint64_t>(F, step) * m->ld));
  for (uint64_t f = 0; f < F; f += step) {
    const uint64_t n = std::min<uint64_t>(step, F - f);
    if ((rc = srhost::corpus_ready(c, f, f + n, m->s_gmm))) return rc;
    if ((rc = launch_scoring(m, c->feats.p + f * m->dim, n, gmm_kernel, m->scores[0].p))) return rc;
    HIP_TRY(hipStreamSynchronize(m->s_gmm));
    HIP_TRY(hipMemcpy2D(out + f * m->n_states, (size_t)m->n_states * sizeof(double), m->scores[0].p,
                        (size_t)m->ld * sizeof(double), (size_t)m->n_states * sizeof(double), (size_t)n,
                        hipMemcpyDeviceToHost));
  }
  if (m->profiling) m->prof.frames += F;
  return SR_OK;
  });
}

int sr_score_frames(sr_model* m, const float* feats, uint64_t n_frames, int gmm_kernel, double* out) {
  return guarded(__func__, [&]() -> int {
  const uint64_t off[2] = {0, n_frames};
  int rc = check_model(m);
  if (rc) return rc;
  if (n_frames > 0 && (!feats || !out)) return fail(SR_EINVAL, "%s is null", feats ? "out" : "feats");
  if (n_frames > (std::numeric_limits<size_t>::max() / sizeof(float) - 64) / m->dim)
    return fail(SR_ELIMIT, "n_frames %llu x dim %u overflows the address space", (unsigned long long)n_frames, m->dim);
  // scoring has no 16-bit frame limit: bypass the per-utterance check by uploading directly
  sr_corpus* c = new sr_corpus();
  std::unique_ptr<sr_corpus, int (*)(sr_corpus*)> own(c, sr_corpus_destroy);
  c->model = m; c->n_utts = 1; c->n_frames = n_frames; c->frame_off.assign(off, off + 2);
  srhost::corpus_register(c);
  hipError_t e;
  if ((e = c->feats.ensure((size_t)n_frames * m->dim + 64)) != hipSuccess ||
      (n_frames > 0 && (e = hipMemcpy(c->feats.p, feats, (size_t)n_frames * m->dim * sizeof(float), hipMemcpyHostToDevice)) != hipSuccess))
    return fail(SR_EHIP, "feature upload: %s", hipGetErrorString(e));
  return sr_score_corpus(m, c, gmm_kernel, out);
  });
}

// test hook: the candidate masks of `feats` from the prefilter alone, by the given route (kPfStaged 0 / kPfStationary 1), as the
// kernel leaves them: [group][frame][4 state slots].  masks == null only reports the group count.  Nothing on a scoring path calls this.
int sr_prefilter_masks(sr_model* m, const float* feats, uint64_t n_frames, int route, uint32_t* n_groups, uint32_t* masks, uint64_t cap_words) {
  return guarded(__func__, [&]() -> int {
  int rc = check_model(m);
  if (rc) return rc;
  if (route != kPfStaged && route != kPfStationary) return fail(SR_EINVAL, "route %d: 0 (staged) or 1 (stationary)", route);
  if (!m->max_approx) return fail(SR_EINVAL, "the prefilter scores max-approx models only");
  if ((rc = reserve_scoring(m, SR_GMM_PREFILTER, n_frames, route))) return rc;
  if (m->pf_ks32 == 0) return fail(SR_EINVAL, "this model is not scored through the prefilter");
  if (n_groups) *n_groups = m->pf_groups;
  if (!masks || n_frames == 0) return SR_OK;
  if (!feats) return fail(SR_EINVAL, "feats is null");
  const uint64_t words = (uint64_t)m->pf_groups * n_frames * 4;
  if (cap_words < words) return fail(SR_EINVAL, "masks holds %llu words, %llu needed", (unsigned long long)cap_words, (unsigned long long)words);
  DevBuf<float> d_feats;
  HIP_TRY(d_feats.ensure((size_t)n_frames * m->dim + 64));
  HIP_TRY(hipMemcpy(d_feats.p, feats, (size_t)n_frames * m->dim * sizeof(float), hipMemcpyHostToDevice));
  GmmPrefilterArgs pa{};
  if ((rc = prefilter_args(m, d_feats.p, n_frames, &pa))) return rc;
  HIP_TRY(hipMemsetAsync(m->pf_mask.p, 0xA5, words * sizeof(uint32_t), m->s_gmm));  // a word no kernel wrote shows
  HIP_TRY(launch_gmm_prefilter(pa, m->pf_ks32, route, m->s_gmm));
  HIP_TRY(hipStreamSynchronize(m->s_gmm));
  HIP_TRY(hipMemcpy(masks, m->pf_mask.p, words * sizeof(uint32_t), hipMemcpyDeviceToHost));
  return SR_OK;
  });
}

// test hook: the refinement alone on candidate masks the caller supplies, in sr_prefilter_masks' layout [group][frame][4 state slots].
// Any mask word is in range for the kernel (it clears the bits beyond a pseudo-state's densities and ignores the slots beyond the last
// one); what the host checks is the array's size.  Nothing on a scoring path calls this.
int sr_refine_masks(sr_model* m, const float* feats, uint64_t n_frames, const uint32_t* masks, uint64_t n_words, double* out) {
  return guarded(__func__, [&]() -> int {
  int rc = check_model(m);
  if (rc) return rc;
  if (!m->max_approx) return fail(SR_EINVAL, "the refinement scores max-approx models only");
  if (n_frames >= (1ull << 30)) return fail(SR_ELIMIT, "n_frames %llu: the refinement's lists hold 30-bit frame numbers", (unsigned long long)n_frames);
  if ((rc = reserve_scoring(m, SR_GMM_PREFILTER, n_frames))) return rc;
  if (m->pf_ks32 == 0) return fail(SR_EINVAL, "this model is not scored through the prefilter");
  const uint64_t words = (uint64_t)m->pf_groups * n_frames * 4;
  if (n_words != words) return fail(SR_EINVAL, "masks holds %llu words, %u groups x %llu frames x 4 = %llu expected", (unsigned long long)n_words,
                                    m->pf_groups, (unsigned long long)n_frames, (unsigned long long)words);
  if (n_frames == 0) return SR_OK;
  if (!feats || !masks || !out) return fail(SR_EINVAL, "%s is null", !feats ? "feats" : !masks ? "masks" : "out");
  DevBuf<float> d_feats;
  DevBuf<double> d_out;
  HIP_TRY(d_feats.ensure((size_t)n_frames * m->dim + 64));
  HIP_TRY(d_out.ensure((size_t)n_frames * m->ld));
  HIP_TRY(hipMemcpy(d_feats.p, feats, (size_t)n_frames * m->dim * sizeof(float), hipMemcpyHostToDevice));
  const GmmRefineArgs ra = refine_args(m, d_feats.p, n_frames, d_out.p);
  // (the kernel reads group pairs: the pair's second half beyond an odd group count holds no pseudo-state)
  HIP_TRY(hipMemsetAsync(m->pf_mask.p, 0, (size_t)((m->pf_groups + 1u) & ~1u) * n_frames * 4 * sizeof(uint32_t), m->s_gmm));
  HIP_TRY(hipMemcpyAsync(m->pf_mask.p, masks, words * sizeof(uint32_t), hipMemcpyHostToDevice, m->s_gmm));
  HIP_TRY(launch_transpose_feats(d_feats.p, n_frames, m->dim, m->pf_dp, ra.n_frames_ld, m->featsT.p, m->pf_dp != m->dim ? m->featsP.p : nullptr, m->s_gmm));
  HIP_TRY(launch_gmm_refine(ra, m->s_gmm));
  HIP_TRY(hipStreamSynchronize(m->s_gmm));
  HIP_TRY(hipMemcpy2D(out, (size_t)m->n_states * sizeof(double), d_out.p, (size_t)m->ld * sizeof(double), (size_t)m->n_states * sizeof(double),
                      (size_t)n_frames, hipMemcpyDeviceToHost));
  return SR_OK;
  });
}

// test hook: the geometry launch_gmm_refine gives a launch over n_frames -- threads per workgroup, pseudo-states per workgroup, frames
// per workgroup (split of the frame range), chunks per state
int sr_refine_geometry(sr_model* m, uint64_t n_frames, uint32_t out[4]) {
  return guarded(__func__, [&]() -> int {
  int rc = check_model(m);
  if (rc) return rc;
  if (!out) return fail(SR_EINVAL, "out is null");
  if (!m->max_approx) return fail(SR_EINVAL, "the refinement scores max-approx models only");
  if ((rc = reserve_scoring(m, SR_GMM_PREFILTER, 0))) return rc;  // (packs the model on first use; no workspace for 0 frames)
  if (m->pf_ks32 == 0) return fail(SR_EINVAL, "this model is not scored through the prefilter");
  gmm_refine_geometry(refine_shape(m, n_frames), out);
  return SR_OK;
  });
}

int sr_prefilter_range_frames(uint32_t* frames) {
  return guarded(__func__, [&]() -> int {
  if (!frames) return fail(SR_EINVAL, "frames is null");
  *frames = (uint32_t)gmm_prefilter_stationary_range_frames();
  return SR_OK;
  });
}

int sr_lexicon_create(sr_model* m, uint32_t n_words, const uint32_t* word_off, const uint16_t* automaton,
                      uint32_t silence_idx, const double tdp[3], uint16_t silence_state, sr_lexicon** out) {
  return guarded(__func__, [&]() -> int {
  if (!out) return fail(SR_EINVAL, "out is null");
  *out = nullptr;
  int rc = check_model(m);
  if (rc) return rc;
  if (!word_off || !automaton || !tdp) return fail(SR_EINVAL, "null lexicon table");
  if (n_words == 0 || n_words > 65535) return fail(SR_ELIMIT, "n_words must be 1..65535 (Book::word is 16 bit)");
  if (silence_idx >= n_words) return fail(SR_EINVAL, "silence_idx out of range");
  if (word_off[0] != 0) return fail(SR_EINVAL, "word_off[0] must be 0");
  uint32_t max_pos = 0;
  for (uint32_t w = 0; w < n_words; w++) {
    if (word_off[w + 1] <= word_off[w]) return fail(SR_EINVAL, "word %u has no positions", w);
    max_pos = std::max(max_pos, word_off[w + 1] - word_off[w]);
  }
  // the reference addresses hypotheses as word*max_pos + pos and lets entry into position 1 alias the
  // next word's position 0 when every word has a single position (Recognizer.cpp:139); not reproduced
  if (max_pos < 2) return fail(SR_ELIMIT, "lexicon needs at least one word with two or more positions");
  const uint32_t P = word_off[n_words];
  if (P > decode_big_max_slots()) return fail(SR_ELIMIT, "%u trellis positions exceed the decoder's limit of %u", P, decode_big_max_slots());
  for (uint32_t w = 0; w < n_words; w++)
    for (uint32_t k = 0; k < word_off[w + 1] - word_off[w]; k++) {
      const uint32_t st = automaton[word_off[w] + k];
      if (st >= m->n_states) return fail(SR_EINVAL, "word %u position %u: state %u >= n_states %u", w, k, st, m->n_states);
    }
  std::vector<uint32_t> info, sword, wend, f_state, f_pred, f_orig, f_type, f_word, w_info, w_order;
  std::vector<uint2> w_states;
  sr_lexicon* l = new sr_lexicon();
  std::unique_ptr<sr_lexicon, int (*)(sr_lexicon*)> own(l, sr_lexicon_destroy);
  l->model = m;
  l->net = build_decode_net(n_words, word_off, automaton, silence_idx, silence_state, tdp, info, sword, wend);
  l->h_slot_info = info;
  l->h_word_off.assign(word_off, word_off + n_words + 1);
  l->fast = build_fast_net(info, sword, word_off, f_state, f_pred, f_orig, f_type, f_word);
  l->words = build_word_net(n_words, word_off, automaton, silence_idx, silence_state, w_info, w_states, w_order);
  hipError_t e;
  if ((e = l->slot_info.upload(info.data(), P)) != hipSuccess || (e = l->slot_word.upload(sword.data(), P)) != hipSuccess ||
      (e = l->word_end_slot.upload(wend.data(), n_words)) != hipSuccess || (e = l->f_state.upload(f_state.data(), f_state.size())) != hipSuccess ||
      (e = l->f_pred.upload(f_pred.data(), f_pred.size())) != hipSuccess || (e = l->f_orig.upload(f_orig.data(), f_orig.size())) != hipSuccess ||
      (e = l->f_type.upload(f_type.data(), f_type.size())) != hipSuccess || (e = l->f_word.upload(f_word.data(), f_word.size())) != hipSuccess ||
      (e = l->w_info.upload(w_info.data(), w_info.size())) != hipSuccess || (e = l->w_states.upload(w_states.data(), w_states.size())) != hipSuccess ||
      (e = l->w_order.upload(w_order.data(), w_order.size())) != hipSuccess)
    return fail(SR_EHIP, "lexicon upload: %s", hipGetErrorString(e));
  l->net.slot_info = l->slot_info.p; l->net.slot_word = l->slot_word.p; l->net.word_end_slot = l->word_end_slot.p;
  l->fast.state = l->f_state.p; l->fast.pred = l->f_pred.p; l->fast.orig = l->f_orig.p; l->fast.chunk_type = l->f_type.p; l->fast.word = l->f_word.p;
  l->words.info = w_info.empty() ? nullptr : l->w_info.p; l->words.states = l->w_states.p; l->words.order = l->w_order.p;
  *out = own.release();
  return SR_OK;
  });
}

// the lexicon's networks and the model's row stride: what decode_route decides from
static DecodeArgs lexicon_args(const sr_lexicon* l) {
  DecodeArgs da{};
  da.net = l->net; da.fast = l->fast; da.words = l->words;
  da.ld = l->model ? l->model->ld : 0;
  return da;
}

int sr_lexicon_describe(const sr_lexicon* l, char* out, size_t cap) {
  return guarded(__func__, [&]() -> int {
  if (!l || !out || cap == 0) return fail(SR_EINVAL, "null argument");
  const DecodeRoute r = decode_route(lexicon_args(l), false, false);
  const WordNet& w = l->words;
  if (r.first == DecodeFirst::kWords && r.big)
    snprintf(out, cap, "words %u x %u plain %u%s (replay: big, %u positions)", w.nw, w.nt, w.plain_len, w.has_general ? " general" : "", l->net.n_slots);
  else if (r.first == DecodeFirst::kWords) snprintf(out, cap, "words %u x %u plain %u%s", w.nw, w.nt, w.plain_len, w.has_general ? " general" : "");
  else if (r.big) snprintf(out, cap, "big (%u positions: hypotheses in device memory)", l->net.n_slots);
  else snprintf(out, cap, "slots (%u type-padded positions)", l->fast.n_slots);
  return SR_OK;
  });
}

int sr_lexicon_destroy(sr_lexicon* l) {
  return guarded(__func__, [&]() -> int {
  if (!l) return SR_OK;
  if (l->model) { (void)hipSetDevice(l->model->device); (void)hipDeviceSynchronize(); }
  delete l;  // (the buffers go with it)
  return SR_OK;
  });
}

// Words of utterance u start at out_words[frame_off[u]] on the device, out_count[u] of them; a kernel that could not walk an
// utterance's traceback (traceback.h) has raised kFlagCorrupt instead of reporting words: SR_ECORRUPT, naming the first one.
//
// The device packs them (gather_words.hip) into c->result, pinned host memory it writes directly: reserve_gather before the pass
// (allocation synchronises), enqueue_gather behind the last search on its stream, and after the pass's own synchronisation
// gather_words checks the block's header and copies offsets and words out.  SRGPU_GATHER=host keeps the earlier route for
// comparison: three pageable copies of everything and the loop on the host.
static int reserve_gather(sr_model* m, sr_corpus* c, uint32_t extra_slots, int n_arrays) {
  if (!m->gather_device) return SR_OK;
  HIP_TRY(c->result.ensure(gather_block_bytes(c->n_utts, c->n_frames + (uint64_t)c->n_utts * extra_slots, n_arrays)));
  HIP_TRY(c->gather_off.ensure((size_t)c->n_utts + 1));
  return SR_OK;
}
static int enqueue_gather(sr_model* m, sr_corpus* c, GatherArgs a, int n_arrays, hipStream_t s) {
  if (!m->gather_device) return SR_OK;
  a.frame_off = c->d_frame_off.p; a.n_utts = c->n_utts;
  a.dev_off = c->gather_off.p; a.block = c->result.p;
  HIP_TRY(launch_gather_words(a, n_arrays, s));
  return SR_OK;
}
static GatherArgs zerogram_gather(const sr_corpus* c) {
  GatherArgs a{};
  a.count = c->out_count.p; a.flags = c->out_flags.p; a.flag_mask = kFlagCorrupt; a.extra_slots = 0;
  a.src[0] = c->out_words.p;
  return a;
}
// the parts of a written block
struct GatherBlock {
  const GatherHeader* head;
  const uint64_t* off;
  const uint32_t* data;  // array k starts at data + k * head->n_words
};
static GatherBlock gather_block(const sr_corpus* c) {
  const uint64_t* off = reinterpret_cast<const uint64_t*>(c->result.p + sizeof(GatherHeader));
  return {reinterpret_cast<const GatherHeader*>(c->result.p), off, reinterpret_cast<const uint32_t*>(off + c->n_utts + 1)};
}

static int gather_words_host(sr_corpus* c, uint32_t* out_words, uint64_t* out_word_off);
static int gather_words(sr_corpus* c, uint32_t* out_words, uint64_t* out_word_off) {
  if (!c->model->gather_device) return gather_words_host(c, out_words, out_word_off);
  const GatherBlock b = gather_block(c);
  const GatherHeader& h = *b.head;
  // the serial loop's order: the lower utterance first, and the flag before the count in one utterance
  if (h.first_flagged != kGatherNone && h.first_flagged <= h.first_over)
    return fail(SR_ECORRUPT, "utterance %u: the traceback does not walk back to frame 0 (Recognizer.cpp:222-231)", h.first_flagged);
  if (h.first_over != kGatherNone) {
    const uint64_t T = c->frame_off[h.first_over + 1] - c->frame_off[h.first_over];
    return fail(SR_ECORRUPT, "utterance %u: %u words for %llu frames", h.first_over, h.over_count, (unsigned long long)T);
  }
  memcpy(out_word_off, b.off, sizeof(uint64_t) * ((size_t)c->n_utts + 1));
  if (h.n_words) memcpy(out_words, b.data, sizeof(uint32_t) * h.n_words);
  return SR_OK;
}
static int gather_words_host(sr_corpus* c, uint32_t* out_words, uint64_t* out_word_off) {
  const uint32_t U = c->n_utts;
  const uint64_t F = c->n_frames;
  std::vector<uint32_t> counts(U), flags(U), dev_words(F);
  if (U) HIP_TRY(hipMemcpy(counts.data(), c->out_count.p, sizeof(uint32_t) * U, hipMemcpyDeviceToHost));
  if (U) HIP_TRY(hipMemcpy(flags.data(), c->out_flags.p, sizeof(uint32_t) * U, hipMemcpyDeviceToHost));
  if (F) HIP_TRY(hipMemcpy(dev_words.data(), c->out_words.p, sizeof(uint32_t) * F, hipMemcpyDeviceToHost));
  uint64_t w = 0;
  out_word_off[0] = 0;
  for (uint32_t u = 0; u < U; u++) {
    if (flags[u] & kFlagCorrupt) return fail(SR_ECORRUPT, "utterance %u: the traceback does not walk back to frame 0 (Recognizer.cpp:222-231)", u);
    const uint64_t b = c->frame_off[u], T = c->frame_off[u + 1] - b;
    if (counts[u] > T) return fail(SR_ECORRUPT, "utterance %u: %u words for %llu frames", u, counts[u], (unsigned long long)T);
    for (uint32_t i = 0; i < counts[u]; i++) out_words[w++] = dev_words[b + i];
    out_word_off[u + 1] = w;
  }
  return SR_OK;
}

// The zerogram search of a corpus on `chunks` (prepare_chunks): the words and tracebacks stay in c->out_* / c->tb_*.
// score(chunk, table) enqueues the chunk's scores on m->s_gmm (score_chunk, but for the test hook sr_recognize_corpus_scores);
// exact_negative is DecodeArgs' (-1: asked of the model); after(chunk, table, stream) enqueues more work on a chunk's scores behind
// its search (a no-op for sr_recognize_corpus).
template <class Score, class After>
static int recognize_pass(sr_model* m, sr_corpus* c, sr_lexicon* l, const sr_search_params* p, const std::vector<Chunk>& chunks,
                          int exact_negative, Score score, After after) {
  const uint32_t U = c->n_utts;
  const uint64_t F = c->n_frames;
  HIP_TRY(c->tb_score.ensure(F + U));
  HIP_TRY(c->tb_word.ensure(F + U));
  HIP_TRY(c->tb_bkp.ensure(F + U));
  HIP_TRY(c->out_words.ensure(F));
  HIP_TRY(c->out_count.ensure(U));
  HIP_TRY(c->out_flags.ensure(U));
  int rc;
  if ((rc = reserve_gather(m, c, 0, 1))) return rc;
  HIP_TRY(hipMemsetAsync(c->out_flags.p, 0, sizeof(uint32_t) * std::max(1u, U), m->s_gmm));

  DecodeArgs da = lexicon_args(l);
  da.frame_off = c->d_frame_off.p; da.utt_order = c->utt_order.p;
  da.am_threshold = p->am_threshold; da.word_penalty = p->word_penalty;
  if (p->flags & ~(SR_SEARCH_GENERAL_KERNEL | SR_SEARCH_SLOT_KERNEL)) return fail(SR_EINVAL, "unknown sr_search_params.flags 0x%x", (unsigned)p->flags);
  const DecodeRoute route = decode_route(da, p->flags & SR_SEARCH_GENERAL_KERNEL, p->flags & SR_SEARCH_SLOT_KERNEL);
  if (route.big) {  // hypothesis arrays of the utterances in flight
    uint32_t most = 0;
    for (const Chunk& ch : chunks) most = std::max(most, ch.u1 - ch.u0);
    HIP_TRY(c->big_ws.ensure((size_t)most * decode_big_workspace(l->net.n_slots)));
  }
  if (exact_negative < 0) {
    bool neg = false;
    if ((rc = srhost::may_go_negative(m, &neg))) return rc;
    da.exact_negative = neg ? 1u : 0u;
  } else {
    da.exact_negative = exact_negative ? 1u : 0u;
  }
  da.tb_score = c->tb_score.p; da.tb_word = c->tb_word.p; da.tb_bkp = c->tb_bkp.p;
  da.out_words = c->out_words.p; da.out_count = c->out_count.p; da.out_flags = c->out_flags.p;

  rc = run_chunks(m, chunks, score,
      [&](const Chunk& ch, const double* table, hipStream_t s) -> int {
        da.scores = table; da.frame_base = ch.f0; da.utt_first = ch.u0; da.n_utts = ch.u1 - ch.u0;
        HIP_TRY(launch_decode(da, route, c->big_ws.p, s));
        if (m->profiling) m->prof.search_bytes += (8.0 * m->n_states + 4.0 * l->net.n_slots) * (double)(ch.f1 - ch.f0);
        return after(ch, table, s);
      },
      [&](hipStream_t s) { return enqueue_gather(m, c, zerogram_gather(c), 1, s); });
  if (rc) return rc;
  if (m->profiling) m->prof.frames += F;
  return SR_OK;
}
// ... with the model's scores, as every production pass takes it
template <class After>
static int recognize_pass(sr_model* m, sr_corpus* c, sr_lexicon* l, const sr_search_params* p, const std::vector<Chunk>& chunks,
                          After after) {
  return recognize_pass(m, c, l, p, chunks, -1,
                        [&](const Chunk& ch, double* table) { return score_chunk(m, c, ch.f0, ch.f1, p->gmm_kernel, table); }, after);
}

int sr_recognize_corpus(sr_model* m, sr_corpus* c, sr_lexicon* l, const sr_search_params* p, uint32_t* out_words,
                        uint64_t* out_word_off, double* tb_score, uint16_t* tb_word, uint16_t* tb_bkp) {
  return guarded(__func__, [&]() -> int {
  int rc = check_corpus(m, c);
  if (rc) return rc;
  if (!l || l->model != m) return fail(SR_EINVAL, "lexicon does not belong to this model");
  if (!p || !out_word_off || (!out_words && c->n_frames)) return fail(SR_EINVAL, "null argument");
  const uint32_t U = c->n_utts;
  const uint64_t F = c->n_frames;
  std::vector<Chunk> chunks;
  if ((rc = prepare_chunks(m, c, &chunks))) return rc;
  if ((rc = recognize_pass(m, c, l, p, chunks, [](const Chunk&, const double*, hipStream_t) { return (int)SR_OK; }))) return rc;
  if ((rc = gather_words(c, out_words, out_word_off))) return rc;
  if (tb_score) HIP_TRY(hipMemcpy(tb_score, c->tb_score.p, sizeof(double) * (F + U), hipMemcpyDeviceToHost));
  if (tb_word) HIP_TRY(hipMemcpy(tb_word, c->tb_word.p, sizeof(uint16_t) * (F + U), hipMemcpyDeviceToHost));
  if (tb_bkp) HIP_TRY(hipMemcpy(tb_bkp, c->tb_bkp.p, sizeof(uint16_t) * (F + U), hipMemcpyDeviceToHost));
  return SR_OK;
  });
}

int sr_traceback_corpus(sr_model* m, sr_corpus* c, sr_lexicon* l, const uint16_t* tb_word, const uint16_t* tb_bkp,
                        uint32_t* out_words, uint64_t* out_word_off) {
  return guarded(__func__, [&]() -> int {
  int rc = check_corpus(m, c);
  if (rc) return rc;
  if (!l || l->model != m) return fail(SR_EINVAL, "lexicon does not belong to this model");
  if (!tb_word || !tb_bkp || !out_word_off || (!out_words && c->n_frames)) return fail(SR_EINVAL, "null argument");
  const uint32_t U = c->n_utts;
  const uint64_t F = c->n_frames;
  HIP_TRY(c->tb_word.ensure(F + U));
  HIP_TRY(c->tb_bkp.ensure(F + U));
  HIP_TRY(c->out_words.ensure(F));
  HIP_TRY(c->out_count.ensure(U));
  HIP_TRY(c->out_flags.ensure(U));
  if ((rc = reserve_gather(m, c, 0, 1))) return rc;
  HIP_TRY(hipMemcpyAsync(c->tb_word.p, tb_word, sizeof(uint16_t) * (F + U), hipMemcpyHostToDevice, m->s_gmm));
  HIP_TRY(hipMemcpyAsync(c->tb_bkp.p, tb_bkp, sizeof(uint16_t) * (F + U), hipMemcpyHostToDevice, m->s_gmm));
  HIP_TRY(launch_traceback(c->d_frame_off.p, U, c->tb_word.p, c->tb_bkp.p, l->net.silence_word, l->net.n_words, c->out_words.p,
                           c->out_count.p, c->out_flags.p, m->s_gmm));
  if ((rc = enqueue_gather(m, c, zerogram_gather(c), 1, m->s_gmm))) return rc;
  HIP_TRY(hipStreamSynchronize(m->s_gmm));
  return gather_words(c, out_words, out_word_off);
  });
}

int sr_gather_words(sr_model* m, uint32_t n_utts, const uint64_t* frame_off, const uint32_t* counts, const uint32_t* flags,
                    const uint32_t* words, uint32_t* out_words, uint64_t* out_word_off) {
  return guarded(__func__, [&]() -> int {
  int rc = check_model(m);
  if (rc) return rc;
  if (!frame_off || !out_word_off || (n_utts && (!counts || !flags))) return fail(SR_EINVAL, "null argument");
  if (frame_off[0] != 0) return fail(SR_EINVAL, "frame_off[0] must be 0");
  for (uint32_t u = 0; u < n_utts; u++)
    if (frame_off[u + 1] < frame_off[u]) return fail(SR_EINVAL, "frame_off falls at utterance %u", u);
  sr_corpus c;  // (the search outputs of a corpus, filled by the caller instead of a search; its buffers go with it)
  c.model = m; c.n_utts = n_utts; c.n_frames = frame_off[n_utts];
  if (c.n_frames && (!words || !out_words)) return fail(SR_EINVAL, "null argument");
  c.frame_off.assign(frame_off, frame_off + n_utts + 1);
  HIP_TRY(c.d_frame_off.upload(frame_off, (size_t)n_utts + 1));
  HIP_TRY(c.out_count.upload(counts, n_utts));
  HIP_TRY(c.out_flags.upload(flags, n_utts));
  HIP_TRY(c.out_words.upload(words, c.n_frames));
  if ((rc = reserve_gather(m, &c, 0, 1))) return rc;
  if ((rc = enqueue_gather(m, &c, zerogram_gather(&c), 1, m->s_gmm))) return rc;
  HIP_TRY(hipStreamSynchronize(m->s_gmm));
  return gather_words(&c, out_words, out_word_off);
  });
}

// test hook: sr_recognize_corpus with the chunk's score step replaced by a copy of the caller's rows (padded to the table's row
// stride with +inf, the whole table once, so that a chunk is one copy)
int sr_recognize_corpus_scores(sr_model* m, sr_corpus* c, sr_lexicon* l, const sr_search_params* p, const double* scores,
                               uint64_t n_scores, int exact_negative, uint32_t* out_words, uint64_t* out_word_off, double* tb_score,
                               uint16_t* tb_word, uint16_t* tb_bkp, uint32_t* out_flags) {
  return guarded(__func__, [&]() -> int {
  int rc = check_corpus(m, c);
  if (rc) return rc;
  if (!l || l->model != m) return fail(SR_EINVAL, "lexicon does not belong to this model");
  if (!p || !out_word_off || !out_flags || (!out_words && c->n_frames) || (!scores && c->n_frames)) return fail(SR_EINVAL, "null argument");
  if (exact_negative != 0 && exact_negative != 1) return fail(SR_EINVAL, "exact_negative must be 0 or 1");
  const uint32_t U = c->n_utts;
  const uint64_t F = c->n_frames;
  if (n_scores != F * m->n_states)
    return fail(SR_EINVAL, "%llu scores for %llu frames x %u states", (unsigned long long)n_scores, (unsigned long long)F, m->n_states);
  const size_t S = m->n_states, ld = m->ld;
  std::vector<double> padded((size_t)F * ld, std::numeric_limits<double>::infinity());
  for (uint64_t t = 0; t < F; t++) memcpy(padded.data() + t * ld, scores + t * S, sizeof(double) * S);
  std::vector<Chunk> chunks;
  if ((rc = prepare_chunks(m, c, &chunks))) return rc;
  rc = recognize_pass(m, c, l, p, chunks, exact_negative,
                      [&](const Chunk& ch, double* table) -> int {
                        if (ch.f1 > ch.f0)
                          HIP_TRY(hipMemcpyAsync(table, padded.data() + ch.f0 * ld, sizeof(double) * (ch.f1 - ch.f0) * ld, hipMemcpyHostToDevice, m->s_gmm));
                        return SR_OK;
                      },
                      [](const Chunk&, const double*, hipStream_t) { return (int)SR_OK; });
  if (rc) {  // (a copy may still be reading `padded`)
    (void)hipStreamSynchronize(m->s_gmm);
    return rc;
  }
  if (U) HIP_TRY(hipMemcpy(out_flags, c->out_flags.p, sizeof(uint32_t) * U, hipMemcpyDeviceToHost));
  if ((rc = gather_words(c, out_words, out_word_off))) return rc;
  if (tb_score) HIP_TRY(hipMemcpy(tb_score, c->tb_score.p, sizeof(double) * (F + U), hipMemcpyDeviceToHost));
  if (tb_word) HIP_TRY(hipMemcpy(tb_word, c->tb_word.p, sizeof(uint16_t) * (F + U), hipMemcpyDeviceToHost));
  if (tb_bkp) HIP_TRY(hipMemcpy(tb_bkp, c->tb_bkp.p, sizeof(uint16_t) * (F + U), hipMemcpyDeviceToHost));
  return SR_OK;
  });
}

int sr_traceback_words(uint32_t n_frames, const uint16_t* tb_word, const uint16_t* tb_bkp, uint32_t silence_word, uint32_t n_words,
                       uint32_t* out_words, uint32_t* out_count) {
  return guarded(__func__, [&]() -> int {
  if (!tb_word || !tb_bkp || !out_count || (!out_words && n_frames)) return fail(SR_EINVAL, "null argument");
  *out_count = 0;
  const uint32_t n = walk_traceback(
      n_frames, silence_word, n_words, [&](uint32_t t) -> uint32_t { return tb_word[t]; },
      [&](uint32_t t) -> uint32_t { return tb_bkp[t]; }, out_words, n_frames);
  if (n == kTbCorrupt) return fail(SR_ECORRUPT, "not a traceback: a back pointer that does not fall, or a word outside the lexicon");
  *out_count = n;
  return SR_OK;
  });
}

int sr_bigram_create(sr_model* m, uint32_t n_words, const uint32_t* word_off, const uint16_t* mixtures,
                     uint32_t silence_word, const float* lm, const float tdp[8], sr_bigram** out) {
  return guarded(__func__, [&]() -> int {
  if (!out) return fail(SR_EINVAL, "out is null");
  *out = nullptr;
  int rc = check_model(m);
  if (rc) return rc;
  if (!word_off || !mixtures || !lm || !tdp) return fail(SR_EINVAL, "null argument");
  const uint32_t W = n_words;
  if (W == 0 || silence_word >= W) return fail(SR_EINVAL, "silence word %u out of range (%u words)", silence_word, W);
  if (W > bigram_max_words()) return fail(SR_ELIMIT, "%u words: the bigram search handles at most %u", W, bigram_max_words());
  if (word_off[0] != 0) return fail(SR_EINVAL, "word_off[0] must be 0");
  for (uint32_t w = 0; w < W; w++) {
    if (word_off[w + 1] <= word_off[w]) return fail(SR_EINVAL, "word %u has no states", w);
    for (uint32_t i = word_off[w]; i < word_off[w + 1]; i++)
      if (mixtures[i] >= m->n_states) return fail(SR_EINVAL, "word %u: mixture %u out of range", w, mixtures[i]);
  }
  // (slots: the words, then the silence copy of every word -- build_bigram_net)
  const uint32_t n_sil = word_off[silence_word + 1] - word_off[silence_word];
  if ((uint64_t)word_off[W] + (uint64_t)W * n_sil > bigram_max_positions())
    return fail(SR_ELIMIT, "%llu positions (words and their silence copies): the bigram search handles at most %u",
                (unsigned long long)word_off[W] + (unsigned long long)W * n_sil, bigram_max_positions());
  std::vector<uint32_t> slot_off, slot_mix, pos_info, pos_slot;
  std::vector<float> lmT, rowmin, rowmax;
  sr_bigram* b = new sr_bigram();
  std::unique_ptr<sr_bigram, int (*)(sr_bigram*)> own(b, sr_bigram_destroy);
  b->model = m;
  // (every lexicon within these limits has a layout: the register layout, the dense LDS image, or the state hypotheses in device
  // memory -- bigram_layout, viterbi_bigram.hip)
  b->net = build_bigram_net(W, word_off, mixtures, silence_word, lm, tdp, slot_off, slot_mix, pos_info, pos_slot, lmT, rowmin, rowmax);
  hipError_t e;
  if ((e = b->slot_off.upload(slot_off.data(), slot_off.size())) != hipSuccess ||
      (e = b->slot_mix.upload(slot_mix.data(), slot_mix.size())) != hipSuccess ||
      (e = b->mixtures.upload(mixtures, word_off[W])) != hipSuccess || (e = b->lmT.upload(lmT.data(), lmT.size())) != hipSuccess ||
      (e = b->lm_rowmin.upload(rowmin.data(), W)) != hipSuccess || (e = b->lm_rowmax.upload(rowmax.data(), W)) != hipSuccess ||
      (e = b->pos_info.upload(pos_info.data(), pos_info.size())) != hipSuccess ||
      (e = b->pos_slot.upload(pos_slot.data(), pos_slot.size())) != hipSuccess)
    return fail(SR_EHIP, "bigram upload: %s", hipGetErrorString(e));
  b->lm_min = std::numeric_limits<float>::infinity();  // (a NaN fails the comparison)
  for (uint32_t w = 0; w < W; w++)
    for (uint32_t h = 0; h < W && w != silence_word; h++) b->lm_min = std::min(b->lm_min, lm[(size_t)w * W + h]);
  BigramArgs& net = b->net;
  net.slot_off = b->slot_off.p; net.slot_mix = b->slot_mix.p; net.mixtures = b->mixtures.p; net.pos_info = b->pos_info.p;
  net.pos_slot = b->pos_slot.p; net.lmT = b->lmT.p; net.lm_rowmin = b->lm_rowmin.p; net.lm_rowmax = b->lm_rowmax.p;
  b->h_slot_off = std::move(slot_off); b->h_pos_info = std::move(pos_info); b->h_lmT = std::move(lmT);
  *out = own.release();
  return SR_OK;
  });
}

int sr_bigram_destroy(sr_bigram* b) {
  return guarded(__func__, [&]() -> int {
  if (!b) return SR_OK;
  if (b->model) { (void)hipSetDevice(b->model->device); (void)hipDeviceSynchronize(); }
  delete b;  // (the buffers go with it)
  return SR_OK;
  });
}

// The bigram search of a corpus (sr_recognize_bigram_corpus).  score(chunk, table) enqueues the chunk's scores on m->s_gmm (score_chunk,
// but for the test hook sr_recognize_bigram_corpus_scores); before(chunks) runs once the chunks are known; after(chunk, table,
// stream) is enqueued behind each chunk's search on the same score table (sr_recognize_bigram_confidence_corpus: the forward-backward).
template <class Score, class Before, class After>
static int bigram_recognize_pass(sr_model* m, sr_corpus* c, sr_bigram* b, const sr_bigram_params* p, uint32_t* out_word, float* out_score,
                                 uint32_t* out_time, uint64_t* out_off, Score score, Before before, After after) {
  int rc = check_corpus(m, c);
  if (rc) return rc;
  if (!b || b->model != m) return fail(SR_EINVAL, "bigram search net does not belong to this model");
  if (!p || !out_off || ((!out_word || !out_score || !out_time) && c->n_frames)) return fail(SR_EINVAL, "null argument");
  const uint32_t U = c->n_utts, W = b->net.n_words;
  const uint64_t F = c->n_frames;
  if (p->flags & ~(SR_BIGRAM_DENSE_STATES | SR_BIGRAM_GLOBAL_STATES)) return fail(SR_EINVAL, "unknown sr_bigram_params.flags 0x%x", (unsigned)p->flags);
  if ((p->flags & SR_BIGRAM_DENSE_STATES) && (p->flags & SR_BIGRAM_GLOBAL_STATES))
    return fail(SR_EINVAL, "SR_BIGRAM_DENSE_STATES and SR_BIGRAM_GLOBAL_STATES exclude each other");
  BigramArgs ba = b->net;
  ba.ld = m->ld;
  ba.dense_states = (p->flags & SR_BIGRAM_DENSE_STATES) ? 1u : 0u;
  ba.global_states = (p->flags & SR_BIGRAM_GLOBAL_STATES) ? 1u : 0u;
  const BigramLayout layout = bigram_layout(ba);
  if (layout == BigramLayout::kNone)
    return fail(SR_ELIMIT, "this lexicon's dense LDS image would take %zu bytes > 160 KiB (SR_BIGRAM_DENSE_STATES)", bigram_lds_bytes(W, ba.n_positions));
  std::vector<Chunk> chunks;
  if ((rc = prepare_chunks(m, c, &chunks))) return rc;
  if ((rc = before(chunks))) return rc;  // (behind every argument check: the hook may build and keep tables)
  // traceback book: 2 start entries + (word ends kept per frame <= W) * T per utterance
  const uint64_t per_frame = p->max_word_ends ? std::min<uint64_t>(p->max_word_ends, W) : W;
  std::vector<uint64_t> book_off(U + 1, 0);
  uint32_t max_chunk_utts = 0;
  for (uint32_t u = 0; u < U; u++) book_off[u + 1] = book_off[u] + 2 + per_frame * (c->frame_off[u + 1] - c->frame_off[u]);
  for (const Chunk& ch : chunks) max_chunk_utts = std::max(max_chunk_utts, ch.u1 - ch.u0);
  HIP_TRY(b->book.ensure(book_off[U]));
  HIP_TRY(b->book_off.upload(book_off.data(), book_off.size()));
  HIP_TRY(b->we_slot.ensure((size_t)max_chunk_utts * 4 * W));
  HIP_TRY(b->we_bp.ensure((size_t)max_chunk_utts * 4 * W));
  HIP_TRY(b->we_score.ensure((size_t)max_chunk_utts * 4 * W));
  HIP_TRY(b->out_word.ensure(F + U));
  HIP_TRY(b->out_time.ensure(F + U));
  HIP_TRY(b->out_score.ensure(F + U));
  HIP_TRY(b->out_count.ensure(U));
  HIP_TRY(b->out_flags.ensure(U));
  if ((rc = reserve_gather(m, c, 1, 3))) return rc;  // (utterance u's slots start at frame_off[u] + u, T_u + 1 of them)

  ba.frame_off = c->d_frame_off.p; ba.utt_order = c->utt_order.p;
  ba.ac_pruning = p->acoustic_pruning; ba.lm_pruning = p->lm_pruning;
  if (layout == BigramLayout::kGlobal) {
    // a bounded, persistent grid (two workgroups per CU at most, each looping over its utterances): the state images take
    // grid x gs_ws_words x 4 bytes whatever the corpus size -- and at most a quarter of the free device memory
    int dev_cus = 0;
    HIP_TRY(hipDeviceGetAttribute(&dev_cus, hipDeviceAttributeMultiprocessorCount, m->device));
    const uint64_t per_wg = bigram_gs_ws_words(W, ba.n_positions);
    size_t free_b = 0, total_b = 0;
    HIP_TRY(hipMemGetInfo(&free_b, &total_b));
    const uint64_t have = b->gs_ws.n / per_wg;  // (workgroups the workspace of an earlier call holds)
    const uint64_t cap = std::max<uint64_t>(have, (free_b / 4) / (per_wg * 4));
    const uint64_t grid = std::min<uint64_t>({(uint64_t)std::max(dev_cus, 1) * 2, (uint64_t)std::max(max_chunk_utts, 1u), cap});
    if (grid == 0) return fail(SR_ENOMEM, "bigram search: %llu bytes of device memory for one state image, %zu free",
                                (unsigned long long)(per_wg * 4), free_b);
    HIP_TRY(b->gs_ws.ensure(grid * per_wg));
    ba.gs_grid = (uint32_t)grid; ba.gs_ws = b->gs_ws.p; ba.gs_ws_words = per_wg;
    if (getenv("SRGPU_BIGRAM_STATS")) {
      HIP_TRY(b->gs_active.ensure(1));
      HIP_TRY(hipMemset(b->gs_active.p, 0, sizeof(unsigned long long)));
      HIP_TRY(hipDeviceSynchronize());
      ba.gs_active = b->gs_active.p;
    }
  }
  ba.we_slot = b->we_slot.p; ba.we_bp = b->we_bp.p; ba.we_score = b->we_score.p;
  ba.book = b->book.p; ba.book_off = b->book_off.p;
  ba.out_word = b->out_word.p; ba.out_score = b->out_score.p; ba.out_time = b->out_time.p;
  ba.out_count = b->out_count.p; ba.out_flags = b->out_flags.p;

  rc = run_chunks(m, chunks, score,
      [&](const Chunk& ch, const double* table, hipStream_t s) -> int {
        ba.scores = table; ba.frame_base = ch.f0; ba.utt_first = ch.u0; ba.n_utts = ch.u1 - ch.u0;
        HIP_TRY(launch_bigram(ba, s));  // (invalid value: a layout without the workspace it needs -- a bug here, not the caller's)
        // SURVEY 8(d)'s decoder model, 8 S + 4 P bytes per frame, with P = the bigram search's positions (words + their silence copies)
        if (m->profiling) m->prof.search_bytes += (8.0 * m->n_states + 4.0 * ba.n_positions) * (double)(ch.f1 - ch.f0);
        return after(ch, table, s);
      },
      [&](hipStream_t s) {
        GatherArgs ga{};
        ga.count = b->out_count.p; ga.flags = b->out_flags.p; ga.flag_mask = ~0u; ga.extra_slots = 1;
        ga.src[0] = b->out_word.p; ga.src[1] = b->out_time.p; ga.src[2] = reinterpret_cast<const uint32_t*>(b->out_score.p);
        return enqueue_gather(m, c, ga, 3, s);
      });
  if (rc) return rc;

  if (m->gather_device) {
    const GatherBlock g = gather_block(c);
    const GatherHeader& h = *g.head;
    if (h.first_flagged != kGatherNone && h.first_flagged <= h.first_over)
      return fail(SR_ELIMIT, "utterance %u: more than %llu word ends per frame (sr_bigram_params.max_word_ends)", h.first_flagged,
                  (unsigned long long)per_frame);
    // (the search writes at most T + 1 entries; a count beyond them would have made the host's loop read the next utterance's)
    if (h.first_over != kGatherNone) return fail(SR_ECORRUPT, "utterance %u: %u entries for its frames", h.first_over, h.over_count);
    memcpy(out_off, g.off, sizeof(uint64_t) * ((size_t)U + 1));
    if (h.n_words) {
      memcpy(out_word, g.data, sizeof(uint32_t) * h.n_words);
      memcpy(out_time, g.data + h.n_words, sizeof(uint32_t) * h.n_words);
      memcpy(out_score, g.data + 2 * h.n_words, sizeof(float) * h.n_words);
    }
  } else {
    std::vector<uint32_t> counts(U), flags(U), dw(F + U), dt(F + U);
    std::vector<float> ds(F + U);
    if (U) {
      HIP_TRY(hipMemcpy(counts.data(), b->out_count.p, sizeof(uint32_t) * U, hipMemcpyDeviceToHost));
      HIP_TRY(hipMemcpy(flags.data(), b->out_flags.p, sizeof(uint32_t) * U, hipMemcpyDeviceToHost));
      HIP_TRY(hipMemcpy(dw.data(), b->out_word.p, sizeof(uint32_t) * (F + U), hipMemcpyDeviceToHost));
      HIP_TRY(hipMemcpy(dt.data(), b->out_time.p, sizeof(uint32_t) * (F + U), hipMemcpyDeviceToHost));
      HIP_TRY(hipMemcpy(ds.data(), b->out_score.p, sizeof(float) * (F + U), hipMemcpyDeviceToHost));
    }
    uint64_t n = 0;
    out_off[0] = 0;
    for (uint32_t u = 0; u < U; u++) {
      if (flags[u]) return fail(SR_ELIMIT, "utterance %u: more than %llu word ends per frame (sr_bigram_params.max_word_ends)", u,
                                (unsigned long long)per_frame);
      const uint64_t o = c->frame_off[u] + u;
      for (uint32_t i = 0; i < counts[u]; i++, n++) { out_word[n] = dw[o + i]; out_score[n] = ds[o + i]; out_time[n] = dt[o + i]; }
      out_off[u + 1] = n;
    }
  }
  if (ba.gs_active) {  // diagnostic (tools/cliffs.py): positions the global-states search visited per frame
    unsigned long long visited = 0;
    HIP_TRY(hipMemcpy(&visited, ba.gs_active, sizeof visited, hipMemcpyDeviceToHost));
    fprintf(stderr, "srgpu bigram: global states, %llu frames, %.1f active positions per frame\n", (unsigned long long)F,
            F ? (double)visited / (double)F : 0.0);
  }
  if (m->profiling) m->prof.frames += F;
  return SR_OK;
}
// ... with the model's scores, as every production pass takes it
template <class Before, class After>
static int bigram_recognize_pass(sr_model* m, sr_corpus* c, sr_bigram* b, const sr_bigram_params* p, uint32_t* out_word, float* out_score,
                                 uint32_t* out_time, uint64_t* out_off, Before before, After after) {
  return bigram_recognize_pass(m, c, b, p, out_word, out_score, out_time, out_off,
                               [&](const Chunk& ch, double* table) { return score_chunk(m, c, ch.f0, ch.f1, p->gmm_kernel, table); }, before, after);
}

int sr_recognize_bigram_corpus(sr_model* m, sr_corpus* c, sr_bigram* b, const sr_bigram_params* p, uint32_t* out_word,
                               float* out_score, uint32_t* out_time, uint64_t* out_off) {
  return guarded(__func__, [&]() -> int {
  return bigram_recognize_pass(m, c, b, p, out_word, out_score, out_time, out_off, [](const std::vector<Chunk>&) { return SR_OK; },
                               [](const Chunk&, const double*, hipStream_t) { return SR_OK; });
  });
}

// test hook: sr_recognize_bigram_corpus with the chunk's score step replaced by a copy of the caller's rows (padded to the table's row
// stride with +inf, the whole table once, so that a chunk is one copy)
int sr_recognize_bigram_corpus_scores(sr_model* m, sr_corpus* c, sr_bigram* b, const sr_bigram_params* p, const double* scores,
                                      uint64_t n_scores, uint32_t* out_word, float* out_score, uint32_t* out_time, uint64_t* out_off) {
  return guarded(__func__, [&]() -> int {
  int rc = check_corpus(m, c);
  if (rc) return rc;
  if (!scores && c->n_frames) return fail(SR_EINVAL, "null argument");
  const uint64_t F = c->n_frames;
  if (n_scores != F * m->n_states)
    return fail(SR_EINVAL, "%llu scores for %llu frames x %u states", (unsigned long long)n_scores, (unsigned long long)F, m->n_states);
  const size_t S = m->n_states, ld = m->ld;
  std::vector<double> padded((size_t)F * ld, std::numeric_limits<double>::infinity());
  for (uint64_t t = 0; t < F; t++) memcpy(padded.data() + t * ld, scores + t * S, sizeof(double) * S);
  rc = bigram_recognize_pass(m, c, b, p, out_word, out_score, out_time, out_off,
                             [&](const Chunk& ch, double* table) -> int {
                               if (ch.f1 > ch.f0)
                                 HIP_TRY(hipMemcpyAsync(table, padded.data() + ch.f0 * ld, sizeof(double) * (ch.f1 - ch.f0) * ld, hipMemcpyHostToDevice, m->s_gmm));
                               return SR_OK;
                             },
                             [](const std::vector<Chunk>&) { return SR_OK; }, [](const Chunk&, const double*, hipStream_t) { return SR_OK; });
  if (rc) (void)hipStreamSynchronize(m->s_gmm);  // (a copy may still be reading `padded`)
  return rc;
  });
}

int sr_bigram_route(const sr_bigram* b, uint32_t flags, char* out, size_t cap) {
  return guarded(__func__, [&]() -> int {
  if (!b || !out || cap == 0) return fail(SR_EINVAL, "null argument");
  if (flags & ~(SR_BIGRAM_DENSE_STATES | SR_BIGRAM_GLOBAL_STATES)) return fail(SR_EINVAL, "unknown sr_bigram_params.flags 0x%x", (unsigned)flags);
  if ((flags & SR_BIGRAM_DENSE_STATES) && (flags & SR_BIGRAM_GLOBAL_STATES))
    return fail(SR_EINVAL, "SR_BIGRAM_DENSE_STATES and SR_BIGRAM_GLOBAL_STATES exclude each other");
  BigramArgs ba = b->net;
  ba.ld = b->model ? b->model->ld : 0;
  ba.dense_states = (flags & SR_BIGRAM_DENSE_STATES) ? 1u : 0u;
  ba.global_states = (flags & SR_BIGRAM_GLOBAL_STATES) ? 1u : 0u;
  bigram_route_text(bigram_route_of(ba), out, cap);
  return SR_OK;
  });
}

int sr_bigram_describe(const sr_bigram* b, char* out, size_t cap) {
  return guarded(__func__, [&]() -> int {
  if (!b || !out || cap == 0) return fail(SR_EINVAL, "null argument");
  BigramArgs ba = b->net;
  ba.ld = b->model ? b->model->ld : 0;
  const BigramLayout layout = bigram_layout(ba);
  snprintf(out, cap, "%s", layout == BigramLayout::kRegisters ? "registers" : layout == BigramLayout::kLds ? "lds" : "global");
  return SR_OK;
  });
}

int sr_recognize_batch(sr_model* m, sr_lexicon* l, const sr_search_params* p, const float* feats,
                       const uint64_t* frame_off, uint32_t n_utts, uint32_t* out_words, uint64_t* out_word_off) {
  return guarded(__func__, [&]() -> int {
  // the feeder copies while the first chunks are being scored (feeder.cpp); the corpus goes away with `own`, which also
  // ends the borrowing of the caller's buffer
  sr_corpus* c = nullptr;
  int rc = sr_corpus_upload_async(m, feats, frame_off, n_utts, &c);
  if (rc) return rc;
  std::unique_ptr<sr_corpus, int (*)(sr_corpus*)> own(c, sr_corpus_destroy);
  return sr_recognize_corpus(m, c, l, p, out_words, out_word_off, nullptr, nullptr, nullptr);
  });
}

// The score side of a pass over per-utterance automata (the aligner, the forward-backward): automata on the device, the corpus'
// chunks with their score buffers and, with a bit-exact kernel requested, the listed tables -- such a pass reads scores of its
// automaton's states only (N of S), so just those (frame, state) pairs are scored: the direct-form kernel in listed mode, the
// same bits as the dense table would hold.  (SR_GMM_MFMA keeps the dense FP64-MFMA table: its rounding differs.)
struct AutomatonScoring {
  std::vector<Chunk> chunks;
  std::vector<uint32_t> blk_first_of_utt;
  bool listed = false;
  int gmm_kernel = SR_GMM_PREFILTER;
};

static int automaton_scoring_setup(sr_model* m, sr_corpus* c, const uint16_t* automata, const uint64_t* aut_off, int gmm_kernel,
                                   AutomatonScoring* p) {
  const uint32_t U = c->n_utts;
  if (gmm_kernel == SR_GMM_DEFAULT) gmm_kernel = SR_GMM_PREFILTER;  // scores of the automaton's states only: listed, bit-exact
  p->gmm_kernel = gmm_kernel;
  HIP_TRY(c->automata.upload(automata, aut_off[U]));
  HIP_TRY(c->aut_off.upload(aut_off, U + 1));
  int rc = prepare_chunks(m, c, &p->chunks);
  if (rc) return rc;
  p->listed = gmm_kernel != SR_GMM_MFMA;
  p->blk_first_of_utt.assign(U + 1, 0);
  if (p->listed) {
    const uint32_t fpb = (uint32_t)gmm_exact_frames_per_block();
    std::vector<uint32_t> list_off(U + 1, 0), list_states, blk_frames, blk_list;
    std::vector<uint64_t> blk_frame0;
    for (uint32_t u = 0; u < U; u++) {
      std::vector<uint32_t> st(automata + aut_off[u], automata + aut_off[u + 1]);
      std::sort(st.begin(), st.end());
      st.erase(std::unique(st.begin(), st.end()), st.end());
      list_states.insert(list_states.end(), st.begin(), st.end());
      list_off[u + 1] = (uint32_t)list_states.size();
      for (uint64_t f = c->frame_off[u]; f < c->frame_off[u + 1]; f += fpb) {
        blk_frame0.push_back(f);
        blk_frames.push_back((uint32_t)std::min<uint64_t>(fpb, c->frame_off[u + 1] - f));
        blk_list.push_back(u);
      }
      p->blk_first_of_utt[u + 1] = (uint32_t)blk_frame0.size();
    }
    HIP_TRY(c->al_list_off.upload(list_off.data(), list_off.size()));
    HIP_TRY(c->al_states.upload(list_states.data(), list_states.size()));
    HIP_TRY(c->al_blk_frame0.upload(blk_frame0.data(), blk_frame0.size()));
    HIP_TRY(c->al_blk_frames.upload(blk_frames.data(), blk_frames.size()));
    HIP_TRY(c->al_blk_list.upload(blk_list.data(), blk_list.size()));
  }
  return SR_OK;
}

// run_chunks' score step of such a pass
static int automaton_scoring_chunk(sr_model* m, sr_corpus* c, const AutomatonScoring& p, const Chunk& ch, double* table) {
  int r = srhost::corpus_ready(c, ch.f0, ch.f1, m->s_gmm);
  if (r) return r;
  if (!p.listed) return launch_scoring(m, c->feats.p + ch.f0 * m->dim, ch.f1 - ch.f0, p.gmm_kernel, table);
  GmmExactArgs ga{};
  ga.feats = c->feats.p; ga.n_frames = c->n_frames; ga.dim = m->dim; ga.n_states = m->n_states;
  ga.dens_off = m->dens_off.p; ga.means = m->means.p; ga.inv_vars = m->inv_vars.p; ga.norm = m->norm.p; ga.logw = m->logw.p;
  ga.out = table; ga.ld = m->ld;
  GmmExactList gl{};
  gl.blk_frame0 = c->al_blk_frame0.p; gl.blk_frames = c->al_blk_frames.p; gl.blk_list = c->al_blk_list.p;
  gl.list_off = c->al_list_off.p; gl.states = c->al_states.p;
  gl.blk_first = p.blk_first_of_utt[ch.u0]; gl.frame_base = ch.f0;
  EventPair eg{};
  if ((r = prof_begin(m, m->s_gmm, 0, &eg))) return r;
  HIP_TRY(launch_gmm_exact_listed(ga, !m->max_approx, gl, p.blk_first_of_utt[ch.u1] - p.blk_first_of_utt[ch.u0], m->s_gmm));
  return prof_end(m, m->s_gmm, &eg);
}

static int check_automaton(const sr_model* m, const uint16_t* automata, const uint64_t* aut_off, uint32_t u) {
  for (uint64_t i = aut_off[u]; i < aut_off[u + 1]; i++)
    if (automata[i] >= m->n_states) return fail(SR_EINVAL, "utterance %u: automaton state %u >= n_states", u, automata[i]);
  return SR_OK;
}

// The score step of an automaton pass (align_common, fb_pass): score(scoring, chunk, table) enqueues the chunk's scores on m->s_gmm --
// automaton_scoring_chunk for every production pass; the test hooks sr_align_corpus_scores / sr_state_posteriors_corpus_scores copy
// the caller's rows instead (ScoreTable below).
static auto model_scores(sr_model* m, sr_corpus* c) {
  return [m, c](const AutomatonScoring& sc, const Chunk& ch, double* table) -> int { return automaton_scoring_chunk(m, c, sc, ch, table); };
}

// The score step of a pass over the recognition network (the word posteriors, occ_pass, smbr_accuracies): score_chunk with the caller's
// kernel for every production pass; the test hooks sr_*_corpus_scores pass a ScoreTable.
static auto gmm_scores(sr_model* m, sr_corpus* c, int gmm_kernel) {
  return [m, c, gmm_kernel](const Chunk& ch, double* table) -> int { return score_chunk(m, c, ch.f0, ch.f1, gmm_kernel, table); };
}

// A caller's score table [F x n_states] as the hooks' score step: the rows padded to the chunk tables' stride m->ld with +inf, the
// whole table once, so that a chunk is one copy.
struct ScoreTable {
  sr_model* m = nullptr;
  std::vector<double> padded;
  int set(sr_model* model, const sr_corpus* c, const double* scores, uint64_t n_scores) {
    m = model;
    const uint64_t F = c->n_frames;
    const size_t S = m->n_states, ld = m->ld;
    if (n_scores != F * S)
      return fail(SR_EINVAL, "%llu scores for %llu frames x %u states", (unsigned long long)n_scores, (unsigned long long)F, m->n_states);
    if (!scores && F) return fail(SR_EINVAL, "null argument");
    padded.assign((size_t)F * ld, std::numeric_limits<double>::infinity());
    for (uint64_t t = 0; t < F; t++) memcpy(padded.data() + t * ld, scores + t * S, sizeof(double) * S);
    return SR_OK;
  }
  // the bigram-network hooks: their word entry is a product in the linear domain, where a cost of -inf (exp(+inf)) has no meaning
  int refuse_neg_inf(const double* scores, uint64_t n_scores) const {
    for (uint64_t i = 0; i < n_scores; i++)
      if (scores[i] == -std::numeric_limits<double>::infinity())
        return fail(SR_EINVAL, "score %llu (frame %llu, state %llu) is -inf", (unsigned long long)i, (unsigned long long)(i / m->n_states),
                    (unsigned long long)(i % m->n_states));
    return SR_OK;
  }
  int operator()(const AutomatonScoring&, const Chunk& ch, double* table) const { return (*this)(ch, table); }
  int operator()(const Chunk& ch, double* table) const {  // (the network passes' score step: run_chunks' own signature)
    if (ch.f1 > ch.f0)
      HIP_TRY(hipMemcpyAsync(table, padded.data() + ch.f0 * m->ld, sizeof(double) * (ch.f1 - ch.f0) * m->ld, hipMemcpyHostToDevice, m->s_gmm));
    return SR_OK;
  }
  // after a pass over the table, failed or not: no copy still reads `padded`
  int done(int rc) const {
    const hipError_t e = hipStreamSynchronize(m->s_gmm);
    if (rc) return rc;
    HIP_TRY(e);
    return SR_OK;
  }
};

template <class Score>
static int align_common(sr_model* m, sr_corpus* c, const uint16_t* automata, const uint64_t* aut_off, const double tdp[3],
                        uint16_t silence_state, double thr, bool pruned, int gmm_kernel, Score score, uint16_t* out_states,
                        double* out_cost) {
  int rc = check_corpus(m, c);
  if (rc) return rc;
  if (!automata || !aut_off || !tdp || !out_states || !out_cost) return fail(SR_EINVAL, "null argument");
  // (a negative threshold prunes a frame's best node with the rest: no node is left, and neither the kernel's nor the reference's
  // back-trace has anything to follow; -0.0, +inf and NaN prune nothing or strict losers only)
  if (pruned && thr < 0.0) return fail(SR_EINVAL, "pruning_threshold must not be negative (got %g)", thr);
  const uint32_t max_pos = pruned ? kAlignPrunedMaxPositions : kAlignMaxPositions;
  static_assert(kAlignPrunedMaxPositions <= kAlignMaxPositions, "");
  const uint32_t U = c->n_utts;
  const uint64_t F = c->n_frames;
  std::vector<uint64_t> bp_off(U + 1, 0);
  uint32_t max_n = 1;
  for (uint32_t u = 0; u < U; u++) {
    const uint64_t N = aut_off[u + 1] - aut_off[u], T = c->frame_off[u + 1] - c->frame_off[u];
    if (N < 1 || T < 1) return fail(SR_EINVAL, "utterance %u: automaton and utterance must be non-empty", u);
    if (!pruned && N > T)
      return fail(SR_EINVAL, "utterance %u: automaton length %llu exceeds %llu frames (Aligner::align_sequence_full indexes "
                  "its T-sized cost arrays by position)", u, (unsigned long long)N, (unsigned long long)T);
    if (N > max_pos)
      return fail(SR_ELIMIT, "utterance %u: automaton length %llu exceeds %u%s", u, (unsigned long long)N, max_pos,
                  pruned ? " (the pruned aligner keeps 20 bytes per position in the 160 KiB LDS)" : "");
    if ((rc = check_automaton(m, automata, aut_off, u))) return rc;
    max_n = std::max<uint32_t>(max_n, (uint32_t)N);
    bp_off[u + 1] = bp_off[u] + N * T;
  }
  HIP_TRY(c->bp_off.upload(bp_off.data(), U + 1));
  HIP_TRY(c->backptr.ensure(bp_off[U]));
  HIP_TRY(c->out_states.ensure(F));
  HIP_TRY(c->out_cost.ensure(U));
  AutomatonScoring sc;
  if ((rc = automaton_scoring_setup(m, c, automata, aut_off, gmm_kernel, &sc))) return rc;
  AlignArgs aa{};
  aa.ld = m->ld; aa.frame_off = c->d_frame_off.p; aa.utt_order = c->utt_order.p; aa.automata = c->automata.p; aa.aut_off = c->aut_off.p;
  aa.tdp_loop = tdp[0]; aa.tdp_forward = tdp[1]; aa.tdp_skip = tdp[2]; aa.silence_state = silence_state;
  aa.pruning_threshold = thr; aa.backptr = c->backptr.p; aa.bp_off = c->bp_off.p; aa.max_positions = max_n;
  aa.out_states = c->out_states.p; aa.out_cost = c->out_cost.p;
  rc = run_chunks(m, sc.chunks,
      [&](const Chunk& ch, double* table) -> int { return score(sc, ch, table); },
      [&](const Chunk& ch, const double* table, hipStream_t s) -> int {
        aa.scores = table; aa.frame_base = ch.f0; aa.utt_first = ch.u0; aa.n_utts = ch.u1 - ch.u0;
        HIP_TRY(pruned ? launch_align_pruned(aa, s) : launch_align_full(aa, s));
        return SR_OK;
      });
  if (rc) return rc;
  if (F) HIP_TRY(hipMemcpy(out_states, c->out_states.p, sizeof(uint16_t) * F, hipMemcpyDeviceToHost));
  if (U) HIP_TRY(hipMemcpy(out_cost, c->out_cost.p, sizeof(double) * U, hipMemcpyDeviceToHost));
  if (m->profiling) {
    m->prof.frames += F;
    for (uint32_t u = 0; u < U; u++) m->prof.search_bytes += 9.0 * (double)bp_off[u + 1] - 9.0 * (double)bp_off[u];
  }
  return SR_OK;
}

int sr_align_corpus(sr_model* m, sr_corpus* c, const uint16_t* automata, const uint64_t* aut_off, const double tdp[3],
                    uint16_t silence_state, int gmm_kernel, uint16_t* out_states, double* out_cost) {
  return guarded(__func__, [&]() -> int {
  return align_common(m, c, automata, aut_off, tdp, silence_state, 0.0, false, gmm_kernel, model_scores(m, c), out_states, out_cost);
  });
}

int sr_align_corpus_pruned(sr_model* m, sr_corpus* c, const uint16_t* automata, const uint64_t* aut_off,
                           const double tdp[3], uint16_t silence_state, double pruning_threshold, int gmm_kernel,
                           uint16_t* out_states, double* out_cost) {
  return guarded(__func__, [&]() -> int {
  return align_common(m, c, automata, aut_off, tdp, silence_state, pruning_threshold, true, gmm_kernel, model_scores(m, c), out_states,
                      out_cost);
  });
}

// test hook: sr_align_corpus / sr_align_corpus_pruned with the chunk's score step replaced by a copy of the caller's rows
int sr_align_corpus_scores(sr_model* m, sr_corpus* c, const uint16_t* automata, const uint64_t* aut_off, const double tdp[3],
                           uint16_t silence_state, int pruned, double pruning_threshold, const double* scores, uint64_t n_scores,
                           uint16_t* out_states, double* out_cost) {
  return guarded(__func__, [&]() -> int {
  int rc = check_corpus(m, c);
  if (rc) return rc;
  if (pruned != 0 && pruned != 1) return fail(SR_EINVAL, "pruned must be 0 or 1");
  ScoreTable table;
  if ((rc = table.set(m, c, scores, n_scores))) return rc;
  // (SR_GMM_MFMA: no listed tables to set up for scores nobody computes)
  return table.done(align_common(m, c, automata, aut_off, tdp, silence_state, pruned ? pruning_threshold : 0.0, pruned != 0, SR_GMM_MFMA,
                                 std::cref(table), out_states, out_cost));
  });
}

int sr_path_scores_corpus(sr_model* m, sr_corpus* c, const uint16_t* states, int gmm_kernel, double* out) {
  return guarded(__func__, [&]() -> int {
  int rc = check_corpus(m, c);
  if (rc) return rc;
  if (gmm_kernel == SR_GMM_DEFAULT) gmm_kernel = SR_GMM_PREFILTER;  // (frame, state) pairs scored directly, bit-exact
  const uint64_t F = c->n_frames;
  if (F == 0) return SR_OK;
  if (!states || !out) return fail(SR_EINVAL, "null argument");
  for (uint64_t f = 0; f < F; f++)
    if (states[f] >= m->n_states) return fail(SR_EINVAL, "frame %llu: state %u >= n_states", (unsigned long long)f, states[f]);
  if ((rc = srhost::corpus_ready(c, 0, F, m->s_gmm))) return rc;
  HIP_TRY(c->out_states.upload(states, F));
  HIP_TRY(c->path_scores.ensure(F));
  if (gmm_kernel != SR_GMM_MFMA) {  // bit-exact kernels: score the F (frame, state) pairs directly, no dense table
    EmArgs a{};
    a.feats = c->feats.p; a.n_frames = F; a.dim = m->dim; a.states = c->out_states.p;
    a.dens_off = m->dens_off.p; a.means = m->means.p; a.inv_vars = m->inv_vars.p; a.norm = m->norm.p; a.logw = m->logw.p;
    a.max_approx = m->max_approx;
    HIP_TRY(launch_path_scores_direct(a, c->path_scores.p, m->s_gmm));
    HIP_TRY(hipStreamSynchronize(m->s_gmm));
    HIP_TRY(hipMemcpy(out, c->path_scores.p, sizeof(double) * F, hipMemcpyDeviceToHost));
    if (m->profiling) m->prof.frames += F;
    return SR_OK;
  }
  const size_t step = m->chunk_frames;
  HIP_TRY(m->scores[0].ensure((size_t)std::min<uint64_t>(F, step) * m->ld));
  for (uint64_t f = 0; f < F; f += step) {
    const uint64_t n = std::min<uint64_t>(step, F - f);
    if ((rc = launch_scoring(m, c->feats.p + f * m->dim, n, gmm_kernel, m->scores[0].p))) return rc;
    HIP_TRY(launch_path_scores(m->scores[0].p, m->ld, f, f, f + n, c->out_states.p, c->path_scores.p, m->s_gmm));
  }
  HIP_TRY(hipStreamSynchronize(m->s_gmm));
  HIP_TRY(hipMemcpy(out, c->path_scores.p, sizeof(double) * F, hipMemcpyDeviceToHost));
  if (m->profiling) m->prof.frames += F;
  return SR_OK;
  });
}

int sr_model_set_tying(sr_model* m, uint32_t n_mean, uint32_t n_var, const uint32_t* dens_mean, const uint32_t* dens_var) {
  return guarded(__func__, [&]() -> int {
  int rc = check_model(m);
  if (rc) return rc;
  if (!dens_mean || !dens_var) return fail(SR_EINVAL, "null tying table");
  for (uint64_t c = 0; c < m->n_dens; c++)
    if (dens_mean[c] >= n_mean || dens_var[c] >= n_var) return fail(SR_EINVAL, "density %llu: tying index out of range", (unsigned long long)c);
  HIP_TRY(m->dens_mean.upload(dens_mean, m->n_dens));
  HIP_TRY(m->dens_var.upload(dens_var, m->n_dens));
  m->n_mean = n_mean; m->n_var = n_var;
  m->h_dens_mean.assign(dens_mean, dens_mean + m->n_dens);
  m->h_dens_var.assign(dens_var, dens_var + m->n_dens);
  return SR_OK;
  });
}

int sr_model_topology(const sr_model* m, uint32_t* dens_off, uint32_t* dens_mean, uint32_t* dens_var) {
  return guarded(__func__, [&]() -> int {
  if (!m) return fail(SR_EINVAL, "null model handle");
  if (dens_off) std::copy(m->h_dens_off.begin(), m->h_dens_off.end(), dens_off);
  if (dens_mean) std::copy(m->h_dens_mean.begin(), m->h_dens_mean.end(), dens_mean);
  if (dens_var) std::copy(m->h_dens_var.begin(), m->h_dens_var.end(), dens_var);
  return SR_OK;
  });
}

int sr_model_tying_info(const sr_model* m, uint32_t* n_mean, uint32_t* n_var) {
  return guarded(__func__, [&]() -> int {
  if (!m) return fail(SR_EINVAL, "null model handle");
  if (n_mean) *n_mean = m->n_mean;
  if (n_var) *n_var = m->n_var;
  return SR_OK;
  });
}

// The (frame, density, weight) pairs of an alignment (em_assign_kernel): checks the states, sizes and uploads what the assignment reads
// and fills `*out` with everything but the accumulators' side (sort workspace, rows); *pair_off_out = the F + 1 pair offsets it uploads
// (the last one is the pair count, which the fMLLR fold reads as the end of the last frame's pairs).  No pair at all: SR_EINVAL.
static int alignment_pairs(sr_model* m, sr_corpus* c, const uint16_t* states, int first_pass, int max_approx, EmArgs* out,
                           std::vector<uint64_t>* pair_off_out) {
  const uint64_t F = c->n_frames;
  const uint32_t D = m->dim;
  int rc;
  if (!states) return fail(SR_EINVAL, "states is null");
  const bool soft = !first_pass && !max_approx;
  std::vector<uint64_t>& pair_off = *pair_off_out;
  pair_off.assign(F + 1, 0);
  uint64_t n_pairs = 0;
  for (uint64_t f = 0; f < F; f++) {
    if (states[f] >= m->n_states) return fail(SR_EINVAL, "frame %llu: state %u >= n_states", (unsigned long long)f, states[f]);
    pair_off[f] = n_pairs;
    n_pairs += soft ? (m->h_dens_off[states[f] + 1] - m->h_dens_off[states[f]]) : 1;
  }
  pair_off[F] = n_pairs;
  if (n_pairs >= (1ull << 31)) return fail(SR_ELIMIT, "too many (frame, density) pairs");
  if (n_pairs == 0) return fail(SR_EINVAL, "no (frame, density) pairs to accumulate");
  if ((rc = srhost::corpus_ready(c, 0, F, m->s_gmm))) return rc;
  HIP_TRY(c->out_states.upload(states, F));
  HIP_TRY(c->pair_off.upload(pair_off.data(), F + 1));
  HIP_TRY(c->pair_frame.ensure(n_pairs)); HIP_TRY(c->key_mean.ensure(n_pairs)); HIP_TRY(c->key_var.ensure(n_pairs));
  HIP_TRY(c->pair_w.ensure(n_pairs));
  EmArgs a{};
  a.feats = c->feats.p; a.n_frames = F; a.n_pairs = n_pairs; a.dim = D; a.states = c->out_states.p; a.pair_off = c->pair_off.p;
  a.dens_off = m->dens_off.p; a.means = m->means.p; a.inv_vars = m->inv_vars.p; a.norm = m->norm.p; a.logw = m->logw.p;
  a.dens_mean = m->dens_mean.p; a.dens_var = m->dens_var.p; a.n_mean = m->n_mean; a.n_var = m->n_var;
  a.first_pass = first_pass; a.max_approx = max_approx;
  a.pair_frame = c->pair_frame.p; a.pair_w = c->pair_w.p; a.key_mean = c->key_mean.p; a.key_var = c->key_var.p;
  *out = a;
  return SR_OK;
}

int sr_accumulate_corpus(sr_model* m, sr_corpus* c, const uint16_t* states, int first_pass, int max_approx, double* mean_acc,
                         double* mean_w, double* var_acc, double* var_w) {
  return guarded(__func__, [&]() -> int {
  int rc = check_corpus(m, c);
  if (rc) return rc;
  const bool to_host = mean_acc || mean_w || var_acc || var_w;  // all NULL: the statistics stay on the device
  if (to_host && (!mean_acc || !mean_w || !var_acc || !var_w)) return fail(SR_EINVAL, "null output (pass all four arrays, or none)");
  const uint64_t F = c->n_frames;
  const uint32_t D = m->dim;
  c->acc_valid = false;
  if (F == 0) {  // empty result = reset_accumulators()
    if (to_host) {
      std::fill(mean_acc, mean_acc + (size_t)m->n_mean * D, 0.0);
      std::fill(mean_w, mean_w + m->n_mean, 0.0);
      std::fill(var_acc, var_acc + (size_t)m->n_var * D, 1e-4);
      std::fill(var_w, var_w + m->n_var, 0.0);
    }
    return to_host ? SR_OK : fail(SR_EINVAL, "empty corpus: nothing to keep on the device");
  }
  EmArgs a{};
  std::vector<uint64_t> pair_off;
  if ((rc = alignment_pairs(m, c, states, first_pass, max_approx, &a, &pair_off))) return rc;
  const uint64_t n_pairs = a.n_pairs;
  HIP_TRY(c->keys_sorted.ensure(n_pairs)); HIP_TRY(c->pairs_sorted.ensure(n_pairs));
  {
    std::vector<uint32_t> iota(n_pairs);
    std::iota(iota.begin(), iota.end(), 0u);
    HIP_TRY(c->iota.upload(iota.data(), n_pairs));
  }
  const size_t temp = em_sort_temp_bytes(n_pairs);
  HIP_TRY(c->sort_temp.ensure(temp));
  HIP_TRY(c->row_begin.ensure((size_t)std::max(m->n_mean, m->n_var) + 1));
  HIP_TRY(c->acc_mean.ensure((size_t)m->n_mean * D)); HIP_TRY(c->w_mean.ensure(m->n_mean));
  HIP_TRY(c->acc_var.ensure((size_t)m->n_var * D)); HIP_TRY(c->w_var.ensure(m->n_var));
  EventPair ep{};
  if ((rc = prof_begin(m, m->s_gmm, 1, &ep))) return rc;
  HIP_TRY(launch_em_accumulate(a, c->sort_temp.p, temp, c->iota.p, c->keys_sorted.p, c->pairs_sorted.p, c->row_begin.p, c->acc_mean.p, c->w_mean.p,
                               c->acc_var.p, c->w_var.p, m->s_gmm));
  if ((rc = prof_end(m, m->s_gmm, &ep))) return rc;
  HIP_TRY(hipStreamSynchronize(m->s_gmm));
  c->acc_valid = true; c->acc_n_mean = m->n_mean; c->acc_n_var = m->n_var;
  if (to_host) {
    HIP_TRY(hipMemcpy(mean_acc, c->acc_mean.p, sizeof(double) * (size_t)m->n_mean * D, hipMemcpyDeviceToHost));
    HIP_TRY(hipMemcpy(mean_w, c->w_mean.p, sizeof(double) * m->n_mean, hipMemcpyDeviceToHost));
    HIP_TRY(hipMemcpy(var_acc, c->acc_var.p, sizeof(double) * (size_t)m->n_var * D, hipMemcpyDeviceToHost));
    HIP_TRY(hipMemcpy(var_w, c->w_var.p, sizeof(double) * m->n_var, hipMemcpyDeviceToHost));
  }
  return SR_OK;
  });
}

int sr_model_create_from_accumulated(sr_model* m, sr_corpus* c, int pooling, int max_approx, sr_model** out) {
  return guarded(__func__, [&]() -> int {
  if (!out) return fail(SR_EINVAL, "out is null");
  *out = nullptr;
  int rc = check_corpus(m, c);
  if (rc) return rc;
  if (pooling < 0 || pooling > 2) return fail(SR_EINVAL, "pooling must be 0 (global), 1 (mixture) or 2 (none)");
  return srhost::finalize_accumulated(m, c, pooling, max_approx, out);
  });
}

// ---- what the forward-backward style passes below share: fb_plan.h plans; these check, size and copy -----------------------------
using srplan::Group;

// An utterance's workspace against m->fb_budget: a launch group takes its first utterance whatever it costs (fb_plan.h), so every
// utterance has to fit alone.  tables: the lattices' word-end tables in place of a trellis.
static int check_fits(const sr_model* m, uint32_t u, uint64_t bytes, bool tables = false) {
  if (bytes <= m->fb_budget) return SR_OK;
  return fail(SR_ELIMIT, "utterance %u: %s of %llu bytes %s the forward-backward workspace of %llu (SRGPU_FB_MB)", u,
              tables ? "word-end tables" : "trellis", (unsigned long long)bytes, tables ? "exceed" : "exceeds",
              (unsigned long long)m->fb_budget);
}
// ... for every utterance of the cost prefix a pass cuts its launch groups with
static int check_fits(const sr_model* m, const std::vector<uint64_t>& cost) {
  for (uint32_t u = 0; u + 1 < cost.size(); u++)
    if (int rc = check_fits(m, u, cost[u + 1] - cost[u])) return rc;
  return SR_OK;
}
// the launch groups of trellises at tr_off[U + 1], 8 bytes per cell, with the offsets on the device and room for the largest group's
static int trellis_groups(sr_model* m, sr_corpus* c, const std::vector<Chunk>& chunks, const std::vector<uint64_t>& tr_off,
                          srplan::Groups* groups) {
  std::vector<uint64_t> cost(tr_off);
  for (uint64_t& x : cost) x *= 8;
  *groups = srplan::launch_groups(chunks, cost.data(), m->fb_budget);
  HIP_TRY(c->fb_trellis_off.upload(tr_off.data(), tr_off.size()));
  HIP_TRY(c->fb_trellis.ensure(std::max<uint64_t>(1, groups->max_span(tr_off.data()))));
  return SR_OK;
}
// an entry point's output arrays: is one of them missing
static bool any_null(std::initializer_list<const void*> ps) { return std::find(ps.begin(), ps.end(), nullptr) != ps.end(); }

// The item path (launch_items, posterior_items.hip): a launch group of at most max_gf frames counts, scans and appends its items to
// the corpus' c->fb_item_* (at most item_bound) behind the counter c->fb_base.
static int ensure_items(sr_corpus* c, uint64_t max_gf, uint64_t F, uint64_t item_bound, size_t* scan_bytes) {
  *scan_bytes = items_scan_temp_bytes(max_gf);
  HIP_TRY(c->fb_scan_temp.ensure(*scan_bytes));
  HIP_TRY(c->fb_cnt.ensure(max_gf)); HIP_TRY(c->fb_scan.ensure(max_gf)); HIP_TRY(c->fb_base.ensure(1));
  HIP_TRY(c->fb_item_off.ensure(F + 1));
  HIP_TRY(c->fb_item_frame.ensure(item_bound)); HIP_TRY(c->fb_item_mix.ensure(item_bound)); HIP_TRY(c->fb_item_w.ensure(item_bound));
  return SR_OK;
}
// What every pass' ItemArgs share over the uploaded lists (upload_mix_lists; the positions in `slot_pos`); serial_limit as ItemArgs'
static void set_slot_pos(ItemArgs* a, const uint16_t* p) { a->slot_pos16 = p; }
static void set_slot_pos(ItemArgs* a, const uint32_t* p) { a->slot_pos32 = p; }
template <class Pos>
static void item_fields(ItemArgs* a, sr_corpus* c, const DevBuf<Pos>& slot_pos, uint32_t serial_limit, double floor) {
  a->frame_off = c->d_frame_off.p; a->trellis = c->fb_trellis.p; a->mix = c->fb_mix.p; a->slot_beg = c->fb_slot_beg.p;
  set_slot_pos(a, slot_pos.p); a->serial_limit = serial_limit; a->floor = floor;
  a->group_cnt = c->fb_cnt.p; a->item_base = c->fb_base.p; a->item_off = c->fb_item_off.p;
  a->item_frame = c->fb_item_frame.p; a->item_mix = c->fb_item_mix.p; a->item_w = c->fb_item_w.p;
}
// a launch group's utterances [u0, u1) in the item arguments; returns its frames
static uint64_t item_group(ItemArgs* a, const sr_corpus* c, uint32_t u0, uint32_t u1) {
  a->utt_first = u0; a->n_utts = u1 - u0; a->group_f0 = c->frame_off[u0];
  return c->frame_off[u1] - c->frame_off[u0];
}
// The mixture lists of a pass' items on the device: c->fb_mix and c->fb_slot_beg, the positions in `slot_pos` (16-bit: c->fb_slot_pos,
// 32-bit: c->bgmmi_slot_pos) and -- per_utt: a set per utterance -- c->fb_mix_off
template <class Pos>
static int upload_mix_lists(sr_corpus* c, const srplan::MixLists<Pos>& ml, bool per_utt, DevBuf<Pos>& slot_pos) {
  if (per_utt) HIP_TRY(c->fb_mix_off.upload(ml.mix_off.data(), ml.mix_off.size()));
  HIP_TRY(c->fb_mix.upload(ml.mix.data(), ml.mix.size()));
  HIP_TRY(c->fb_slot_beg.upload(ml.slot_beg.data(), ml.slot_beg.size()));
  HIP_TRY(slot_pos.upload(ml.slot_pos.data(), ml.slot_pos.size()));
  return SR_OK;
}
// The item arguments of a network pass over the uploaded lists `ml`: the free network's rows of P positions, or -- chain -- the
// transcripts' chains (upload_chains, trellis_groups)
template <class Pos>
static void occ_item_fields(ItemArgs* a, sr_corpus* c, const srplan::MixLists<Pos>& ml, bool chain, uint64_t P, const DevBuf<Pos>& slot_pos,
                            uint32_t serial_limit, const double* gate, double floor) {
  item_fields(a, c, slot_pos, serial_limit, floor);
  a->n_cols = a->row_stride = (uint32_t)P; a->n_mix = chain ? 0u : (uint32_t)ml.mix.size(); a->gate = gate;
  if (chain) { a->trellis_off = c->fb_trellis_off.p; a->chain_off = c->mmi_chain_off.p; a->mix_off = c->fb_mix_off.p; }
}
// the transcripts' chains of either network (chains.cpp) on the device
static int upload_chains(sr_corpus* c, const chain_host::Chains& ch) {
  HIP_TRY(c->mmi_chain_off.upload(ch.off.data(), ch.off.size()));
  HIP_TRY(c->mmi_info.upload(ch.info.data(), ch.info.size()));
  HIP_TRY(c->mmi_src.upload(ch.src.data(), ch.src.size()));
  HIP_TRY(c->mmi_dst.upload(ch.dst.data(), ch.dst.size()));
  return SR_OK;
}
// ahead of a pass' first launch group, on its stream
static hipError_t reset_item_count(DevBuf<uint32_t>& base, hipStream_t s) { return hipMemsetAsync(base.p, 0, sizeof(uint32_t), s); }
static int read_item_count(const DevBuf<uint32_t>& base, uint64_t* n_items) {
  uint32_t n = 0;
  HIP_TRY(hipMemcpy(&n, base.p, sizeof(uint32_t), hipMemcpyDeviceToHost));
  *n_items = n;
  return SR_OK;
}

// The top items per frame an entry point may give out: all three arrays or none (*post), at most max_items a frame.
static int top_items_arguments(const void* out_count, const void* out_id, const void* out_weight, const char* id_name, uint32_t max_items,
                               bool* post) {
  *post = out_count || out_id || out_weight;
  if (*post && (!out_count || !out_id || !out_weight))
    return fail(SR_EINVAL, "null output (pass out_count, %s and out_weight, or none)", id_name);
  if (*post && (max_items == 0 || max_items > 65535)) return fail(SR_EINVAL, "max_items must be 1 .. 65535 (got %u)", max_items);
  return SR_OK;
}
template <class Id>
static int ensure_top_items(uint64_t F, uint32_t max_items, DevBuf<uint16_t>& count, DevBuf<Id>& id, DevBuf<double>& weight) {
  HIP_TRY(count.ensure(F));
  HIP_TRY(id.ensure((size_t)F * max_items));
  HIP_TRY(weight.ensure((size_t)F * max_items));
  return SR_OK;
}
template <class Id>
static int copy_top_items(uint64_t F, uint32_t max_items, const DevBuf<uint16_t>& count, const DevBuf<Id>& id, const DevBuf<double>& weight,
                          uint16_t* out_count, Id* out_id, double* out_weight) {
  HIP_TRY(hipMemcpy(out_count, count.p, sizeof(uint16_t) * F, hipMemcpyDeviceToHost));
  HIP_TRY(hipMemcpy(out_id, id.p, sizeof(Id) * F * max_items, hipMemcpyDeviceToHost));
  HIP_TRY(hipMemcpy(out_weight, weight.p, sizeof(double) * F * max_items, hipMemcpyDeviceToHost));
  return SR_OK;
}
// the top items of the items a pass left in c->fb_item_* (launch_items_top), to the host
static int top_of_items(sr_model* m, sr_corpus* c, uint32_t max_items, uint16_t* out_count, uint16_t* out_state, double* out_weight) {
  const uint64_t F = c->n_frames;
  if (F == 0) return SR_OK;
  int rc = ensure_top_items(F, max_items, c->fb_count, c->fb_state, c->fb_weight);
  if (rc) return rc;
  HIP_TRY(launch_items_top(c->fb_item_off.p, c->fb_item_mix.p, c->fb_item_w.p, F, max_items, c->fb_count.p, c->fb_state.p,
                           c->fb_weight.p, m->s_gmm));
  HIP_TRY(hipStreamSynchronize(m->s_gmm));
  return copy_top_items(F, max_items, c->fb_count, c->fb_state, c->fb_weight, out_count, out_state, out_weight);
}

// ---- forward-backward (viterbi_fb.hip) -----------------------------------------------------------------------------------
// The argument checks both entry points share: the aligner's, with N_u <= 2 T_u - 1 (a path must exist) in place of N_u <= T_u.
static int fb_check(sr_model* m, sr_corpus* c, const uint16_t* automata, const uint64_t* aut_off, const double tdp[3],
                    double posterior_floor, const double* out_cost) {
  int rc = check_corpus(m, c);
  if (rc) return rc;
  if (!automata || !aut_off || !tdp || !out_cost) return fail(SR_EINVAL, "null argument");
  if (!(posterior_floor >= 0.0)) return fail(SR_EINVAL, "posterior_floor must be >= 0 (got %g)", posterior_floor);
  for (uint32_t u = 0; u < c->n_utts; u++) {
    const uint64_t N = aut_off[u + 1] - aut_off[u], T = c->frame_off[u + 1] - c->frame_off[u];
    if (N < 1 || T < 1) return fail(SR_EINVAL, "utterance %u: automaton and utterance must be non-empty", u);
    if (N > align_max_positions()) return fail(SR_ELIMIT, "utterance %u: automaton length %llu exceeds %u", u, (unsigned long long)N, align_max_positions());
    if (N > 2 * T - 1)
      return fail(SR_EINVAL, "utterance %u: automaton length %llu: no path through it in %llu frames (at most 2 T - 1 positions)", u,
                  (unsigned long long)N, (unsigned long long)T);
    if ((rc = check_automaton(m, automata, aut_off, u))) return rc;
    if ((rc = check_fits(m, u, 8 * N * T))) return rc;
  }
  return SR_OK;
}

// One pass over the corpus on the aligner's scoring chunks; inside a chunk, consecutive utterances whose trellises fit m->fb_budget
// together (8 B per frame and position) run forward, backward and -- want_items -- the posterior items.  Leaves F_u in c->out_cost
// and, with want_items, *n_items items in c->fb_item_* (frame order, ascending mixture id) with c->fb_item_off[F + 1].
template <class Score>
static int fb_pass(sr_model* m, sr_corpus* c, const uint16_t* automata, const uint64_t* aut_off, const double tdp[3],
                   uint16_t silence_state, int gmm_kernel, double posterior_floor, bool want_items, uint64_t* n_items, Score score) {
  const uint32_t U = c->n_utts;
  const uint64_t F = c->n_frames;
  *n_items = 0;
  HIP_TRY(c->out_cost.ensure(U));
  if (U == 0) return SR_OK;
  // per utterance: trellis offset; its automaton's distinct mixtures (ascending) and the positions carrying each
  std::vector<uint64_t> tr_off(U + 1, 0);
  srplan::MixLists<uint16_t> ml;
  uint64_t item_bound = 0;
  for (uint32_t u = 0; u < U; u++) {
    const uint64_t N = aut_off[u + 1] - aut_off[u], T = c->frame_off[u + 1] - c->frame_off[u];
    tr_off[u + 1] = tr_off[u] + N * T;
    ml.add(automata + aut_off[u], N);
    item_bound += T * ml.n_mix(u);
  }
  if (want_items && item_bound >= (1ull << 31)) return fail(SR_ELIMIT, "too many (frame, mixture) posteriors");
  AutomatonScoring sc;
  int rc = automaton_scoring_setup(m, c, automata, aut_off, gmm_kernel, &sc);
  if (rc) return rc;
  srplan::Groups groups;
  if ((rc = trellis_groups(m, c, sc.chunks, tr_off, &groups))) return rc;
  FbArgs fa{};
  size_t scan_bytes = 0;
  if (want_items && ((rc = upload_mix_lists(c, ml, true, c->fb_slot_pos)) ||
                     (rc = ensure_items(c, std::max<uint64_t>(1, groups.max_span(c->frame_off.data())), F, item_bound, &scan_bytes))))
    return rc;
  fa.ld = m->ld; fa.frame_off = c->d_frame_off.p; fa.automata = c->automata.p; fa.aut_off = c->aut_off.p;
  fa.tdp_loop = tdp[0]; fa.tdp_forward = tdp[1]; fa.tdp_skip = tdp[2]; fa.silence_state = silence_state;
  fa.trellis = c->fb_trellis.p; fa.trellis_off = c->fb_trellis_off.p; fa.out_cost = c->out_cost.p;
  ItemArgs ia{};  // the automata as chains, every mixture summed in position order
  item_fields(&ia, c, c->fb_slot_pos, 0, posterior_floor);
  ia.trellis_off = c->fb_trellis_off.p; ia.chain_off = c->aut_off.p; ia.mix_off = c->fb_mix_off.p; ia.by_frame = true;
  size_t ci = 0;  // run_chunks searches the chunks in order
  rc = run_chunks(m, sc.chunks,
      [&](const Chunk& ch, double* table) -> int { return score(sc, ch, table); },
      [&](const Chunk& ch, const double* table, hipStream_t s) -> int {
        if (want_items && ci == 0) HIP_TRY(reset_item_count(c->fb_base, s));
        for (const Group& g : groups.of_chunk[ci]) {
          fa.scores = table; fa.frame_base = ch.f0; fa.utt_first = g.u0; fa.n_utts = g.u1 - g.u0;
          fa.max_positions = srplan::max_positions(g, aut_off);
          HIP_TRY(launch_fb_forward(fa, s));
          HIP_TRY(launch_fb_backward(fa, s));
          if (want_items) {
            const uint64_t n = item_group(&ia, c, g.u0, g.u1);
            HIP_TRY(launch_items(ia, +1, n, c->fb_scan_temp.p, scan_bytes, c->fb_scan.p, s));
          }
        }
        ci++;
        return SR_OK;
      });
  if (rc) return rc;
  if (want_items && (rc = read_item_count(c->fb_base, n_items))) return rc;
  if (m->profiling) {  // trellis traffic per (frame, position): alpha out, alpha in + gamma out, gamma in (items)
    m->prof.frames += F;
    m->prof.search_bytes += (want_items ? 32.0 : 24.0) * (double)tr_off[U];
  }
  return SR_OK;
}

// ... with the model's scores, as every production pass takes it
static int fb_pass(sr_model* m, sr_corpus* c, const uint16_t* automata, const uint64_t* aut_off, const double tdp[3],
                   uint16_t silence_state, int gmm_kernel, double posterior_floor, bool want_items, uint64_t* n_items) {
  return fb_pass(m, c, automata, aut_off, tdp, silence_state, gmm_kernel, posterior_floor, want_items, n_items, model_scores(m, c));
}

// sr_state_posteriors_corpus and its test hook: the checks, the pass on `score`'s scores, F_u and the top items to the host
template <class Score>
static int state_posteriors(sr_model* m, sr_corpus* c, const uint16_t* automata, const uint64_t* aut_off, const double tdp[3],
                            uint16_t silence_state, int gmm_kernel, double posterior_floor, uint32_t max_items, Score score,
                            double* out_cost, uint16_t* out_count, uint16_t* out_state, double* out_weight) {
  int rc = fb_check(m, c, automata, aut_off, tdp, posterior_floor, out_cost);
  if (rc) return rc;
  bool post = false;
  if ((rc = top_items_arguments(out_count, out_state, out_weight, "out_state", max_items, &post))) return rc;
  const uint32_t U = c->n_utts;
  uint64_t n_items = 0;
  if ((rc = fb_pass(m, c, automata, aut_off, tdp, silence_state, gmm_kernel, posterior_floor, post, &n_items, score))) return rc;
  if (U) HIP_TRY(hipMemcpy(out_cost, c->out_cost.p, sizeof(double) * U, hipMemcpyDeviceToHost));
  return post ? top_of_items(m, c, max_items, out_count, out_state, out_weight) : SR_OK;
}

int sr_state_posteriors_corpus(sr_model* m, sr_corpus* c, const uint16_t* automata, const uint64_t* aut_off, const double tdp[3],
                               uint16_t silence_state, int gmm_kernel, double posterior_floor, uint32_t max_items, double* out_cost,
                               uint16_t* out_count, uint16_t* out_state, double* out_weight) {
  return guarded(__func__, [&]() -> int {
  return state_posteriors(m, c, automata, aut_off, tdp, silence_state, gmm_kernel, posterior_floor, max_items, model_scores(m, c), out_cost,
                          out_count, out_state, out_weight);
  });
}

// test hook: sr_state_posteriors_corpus with the chunk's score step replaced by a copy of the caller's rows
int sr_state_posteriors_corpus_scores(sr_model* m, sr_corpus* c, const uint16_t* automata, const uint64_t* aut_off, const double tdp[3],
                                      uint16_t silence_state, const double* scores, uint64_t n_scores, double posterior_floor,
                                      uint32_t max_items, double* out_cost, uint16_t* out_count, uint16_t* out_state,
                                      double* out_weight) {
  return guarded(__func__, [&]() -> int {
  int rc = check_corpus(m, c);
  if (rc) return rc;
  ScoreTable table;
  if ((rc = table.set(m, c, scores, n_scores))) return rc;
  return table.done(state_posteriors(m, c, automata, aut_off, tdp, silence_state, SR_GMM_MFMA, posterior_floor, max_items, std::cref(table),
                                     out_cost, out_count, out_state, out_weight));
  });
}

// The pairs of the n_items items a pass left in c->fb_item_* (fb_pass, occ_pass; em_assign_weighted_kernel): counts them, sizes what
// the assignment writes and fills `a` with everything but the accumulators' side.  a->n_pairs = 0: nothing above the floor.
static int item_pairs(sr_model* m, sr_corpus* c, uint64_t n_items, int first_pass, int max_approx, EmArgs* out) {
  EmArgs a{};
  a.feats = c->feats.p; a.n_frames = c->n_frames; a.dim = m->dim;
  a.dens_off = m->dens_off.p; a.means = m->means.p; a.inv_vars = m->inv_vars.p; a.norm = m->norm.p; a.logw = m->logw.p;
  a.dens_mean = m->dens_mean.p; a.dens_var = m->dens_var.p; a.n_mean = m->n_mean; a.n_var = m->n_var;
  a.first_pass = first_pass; a.max_approx = max_approx;
  a.n_items = n_items; a.item_frame = c->fb_item_frame.p; a.item_mix = c->fb_item_mix.p; a.item_w = c->fb_item_w.p;
  uint64_t n_pairs = 0;
  if (n_items) {
    HIP_TRY(c->fb_pair_cnt.ensure(n_items));
    HIP_TRY(c->fb_pair_end.ensure(n_items));
    a.item_pair_end = c->fb_pair_end.p;
    const size_t scan = em_item_scan_temp_bytes(n_items);
    HIP_TRY(c->fb_scan_temp.ensure(scan));
    HIP_TRY(launch_em_item_pairs(a, c->fb_scan_temp.p, scan, c->fb_pair_cnt.p, m->s_gmm));
    HIP_TRY(hipStreamSynchronize(m->s_gmm));
    HIP_TRY(hipMemcpy(&n_pairs, c->fb_pair_end.p + (n_items - 1), sizeof(uint64_t), hipMemcpyDeviceToHost));
  }
  if (n_pairs >= (1ull << 31)) return fail(SR_ELIMIT, "too many (frame, density) pairs");
  a.n_pairs = n_pairs;
  if (n_pairs) {
    HIP_TRY(c->pair_frame.ensure(n_pairs)); HIP_TRY(c->key_mean.ensure(n_pairs)); HIP_TRY(c->key_var.ensure(n_pairs));
    HIP_TRY(c->pair_w.ensure(n_pairs));
    a.pair_frame = c->pair_frame.p; a.pair_w = c->pair_w.p; a.key_mean = c->key_mean.p; a.key_var = c->key_var.p;
  }
  *out = a;
  return SR_OK;
}

// The posterior-weighted statistics of the n_items items a pass left in c->fb_item_* (fb_pass, occ_pass), in c->acc_* and -- to_host --
// the four arrays.
static int accumulate_items(sr_model* m, sr_corpus* c, uint64_t n_items, int first_pass, int max_approx, bool to_host, double* mean_acc,
                            double* mean_w, double* var_acc, double* var_w) {
  const uint32_t D = m->dim;
  int rc;
  EmArgs a{};
  if ((rc = item_pairs(m, c, n_items, first_pass, max_approx, &a))) return rc;
  const uint64_t n_pairs = a.n_pairs;
  if (n_pairs == 0) {  // nothing above the floor: reset_accumulators()
    if (to_host) {
      std::fill(mean_acc, mean_acc + (size_t)m->n_mean * D, 0.0);
      std::fill(mean_w, mean_w + m->n_mean, 0.0);
      std::fill(var_acc, var_acc + (size_t)m->n_var * D, 1e-4);
      std::fill(var_w, var_w + m->n_var, 0.0);
    }
    return to_host ? SR_OK : fail(SR_EINVAL, "no posterior above the floor: nothing to keep on the device");
  }
  HIP_TRY(c->keys_sorted.ensure(n_pairs)); HIP_TRY(c->pairs_sorted.ensure(n_pairs));
  HIP_TRY(c->iota.ensure(n_pairs));
  const size_t temp = em_sort_temp_bytes(n_pairs);
  HIP_TRY(c->sort_temp.ensure(temp));
  HIP_TRY(c->row_begin.ensure((size_t)std::max(m->n_mean, m->n_var) + 1));
  HIP_TRY(c->acc_mean.ensure((size_t)m->n_mean * D)); HIP_TRY(c->w_mean.ensure(m->n_mean));
  HIP_TRY(c->acc_var.ensure((size_t)m->n_var * D)); HIP_TRY(c->w_var.ensure(m->n_var));
  EventPair ep{};
  if ((rc = prof_begin(m, m->s_gmm, 1, &ep))) return rc;
  HIP_TRY(launch_em_accumulate_weighted(a, c->sort_temp.p, temp, c->iota.p, c->keys_sorted.p, c->pairs_sorted.p, c->row_begin.p,
                                        c->acc_mean.p, c->w_mean.p, c->acc_var.p, c->w_var.p, m->s_gmm));
  if ((rc = prof_end(m, m->s_gmm, &ep))) return rc;
  HIP_TRY(hipStreamSynchronize(m->s_gmm));
  c->acc_valid = true; c->acc_n_mean = m->n_mean; c->acc_n_var = m->n_var;
  if (to_host) {
    HIP_TRY(hipMemcpy(mean_acc, c->acc_mean.p, sizeof(double) * (size_t)m->n_mean * D, hipMemcpyDeviceToHost));
    HIP_TRY(hipMemcpy(mean_w, c->w_mean.p, sizeof(double) * m->n_mean, hipMemcpyDeviceToHost));
    HIP_TRY(hipMemcpy(var_acc, c->acc_var.p, sizeof(double) * (size_t)m->n_var * D, hipMemcpyDeviceToHost));
    HIP_TRY(hipMemcpy(var_w, c->w_var.p, sizeof(double) * m->n_var, hipMemcpyDeviceToHost));
  }
  return SR_OK;
}

int sr_baum_welch_corpus(sr_model* m, sr_corpus* c, const uint16_t* automata, const uint64_t* aut_off, const double tdp[3],
                         uint16_t silence_state, int gmm_kernel, double posterior_floor, int first_pass, int max_approx,
                         double* out_cost, double* mean_acc, double* mean_w, double* var_acc, double* var_w) {
  return guarded(__func__, [&]() -> int {
  int rc = fb_check(m, c, automata, aut_off, tdp, posterior_floor, out_cost);
  if (rc) return rc;
  const bool to_host = mean_acc || mean_w || var_acc || var_w;  // all NULL: the statistics stay on the device
  if (to_host && (!mean_acc || !mean_w || !var_acc || !var_w)) return fail(SR_EINVAL, "null output (pass all four arrays, or none)");
  const uint32_t U = c->n_utts;
  c->acc_valid = false;
  uint64_t n_items = 0;
  if ((rc = fb_pass(m, c, automata, aut_off, tdp, silence_state, gmm_kernel, posterior_floor, true, &n_items))) return rc;
  if (U) HIP_TRY(hipMemcpy(out_cost, c->out_cost.p, sizeof(double) * U, hipMemcpyDeviceToHost));
  return accumulate_items(m, c, n_items, first_pass, max_approx, to_host, mean_acc, mean_w, var_acc, var_w);
  });
}

// ---- what fMLLR and MLLR share ahead of their statistics ---------------------------------------------------------------------------
// every utterance's speaker is one of n_speakers (> 0: the caller's check), and the dimension fits; `what` names the call in the message
// (null: a call without the contraction's dimension limit -- the MAP statistics)
static int speaker_check(const sr_model* m, const sr_corpus* c, const uint32_t* utt_speaker, uint32_t n_speakers, const char* what) {
  if (!utt_speaker && c->n_utts) return fail(SR_EINVAL, "utt_speaker is null");
  for (uint32_t u = 0; u < c->n_utts; u++)
    if (utt_speaker[u] >= n_speakers) return fail(SR_EINVAL, "utterance %u: speaker %u >= n_speakers %u", u, utt_speaker[u], n_speakers);
  if (what && m->dim > fmllr_max_dim()) return fail(SR_ELIMIT, "dimension %u exceeds %u (%s)", m->dim, fmllr_max_dim(), what);
  return SR_OK;
}

// no frame, or nothing above the floor: the statistics of `groups` speakers or (speaker, class) pairs are 0
static int adapt_zero(uint32_t D, uint64_t groups, double* out_beta, double* out_k, double* out_G) {
  const size_t nk = (size_t)groups * D * (D + 1);
  std::fill(out_beta, out_beta + groups, 0.0);
  std::fill(out_k, out_k + nk, 0.0);
  std::fill(out_G, out_G + nk * (D + 1), 0.0);
  return SR_OK;
}

// The (frame, density, weight) pairs of the adaptation statistics, formed on the device with the density id beside the keys, from an
// alignment or from a Baum-Welch pass (which also gives out_cost).  e->n_pairs = 0: no frame, or nothing above the floor.
static int adapt_pairs(sr_model* m, sr_corpus* c, const uint16_t* states, int max_approx, EmArgs* e) {
  *e = EmArgs{};
  if (c->n_frames == 0) return SR_OK;
  std::vector<uint64_t> pair_off;
  int rc = alignment_pairs(m, c, states, 0, max_approx, e, &pair_off);
  if (rc) return rc;
  HIP_TRY(c->fm_pair_dens.ensure(e->n_pairs));
  e->pair_dens = c->fm_pair_dens.p;
  HIP_TRY(launch_em_pairs(*e, m->s_gmm));
  return SR_OK;
}
static int adapt_pairs_bw(sr_model* m, sr_corpus* c, const uint16_t* automata, const uint64_t* aut_off, const double tdp[3],
                          uint16_t silence_state, int gmm_kernel, double posterior_floor, int max_approx, double* out_cost, EmArgs* e) {
  int rc = fb_check(m, c, automata, aut_off, tdp, posterior_floor, out_cost);
  if (rc) return rc;
  uint64_t n_items = 0;
  if ((rc = fb_pass(m, c, automata, aut_off, tdp, silence_state, gmm_kernel, posterior_floor, true, &n_items))) return rc;
  if (c->n_utts) HIP_TRY(hipMemcpy(out_cost, c->out_cost.p, sizeof(double) * c->n_utts, hipMemcpyDeviceToHost));
  if ((rc = item_pairs(m, c, n_items, 0, max_approx, e)) || e->n_pairs == 0) return rc;
  HIP_TRY(c->fm_pair_dens.ensure(e->n_pairs));
  e->pair_dens = c->fm_pair_dens.p;
  HIP_TRY(launch_em_pairs_weighted(*e, m->s_gmm));
  return SR_OK;
}

// What the fMLLR and MLLR statistics end with: the segments of the groups (g->shape is the caller's) to the device, the partials'
// workspace and the results sized, `launch` under the profile events, the results to the host
template <class Launch>
static int grouped_statistics(sr_model* m, sr_corpus* c, const srplan::Segments& seg, uint32_t n_groups, GroupedStats* g, Launch launch,
                              double* out_beta, double* out_k, double* out_G) {
  const uint32_t D = m->dim;
  int rc;
  g->n_groups = n_groups; g->n_segs = (uint32_t)seg.begin.size();
  HIP_TRY(c->fm_seg_begin.upload(seg.begin.data(), seg.begin.size())); HIP_TRY(c->fm_seg_len.upload(seg.len.data(), seg.len.size()));
  HIP_TRY(c->fm_spk_seg_off.upload(seg.off.data(), seg.off.size()));
  HIP_TRY(c->fm_partial.ensure((size_t)g->n_segs * g->shape.rows * g->shape.cols));
  const size_t nk = (size_t)n_groups * D * (D + 1), nG = nk * (D + 1);
  HIP_TRY(c->fm_beta.ensure(n_groups)); HIP_TRY(c->fm_k.ensure(nk)); HIP_TRY(c->fm_G.ensure(nG));
  g->seg_begin = c->fm_seg_begin.p; g->seg_len = c->fm_seg_len.p; g->grp_seg_off = c->fm_spk_seg_off.p; g->partial = c->fm_partial.p;
  g->out_beta = c->fm_beta.p; g->out_k = c->fm_k.p; g->out_G = c->fm_G.p;
  EventPair ep{};
  if ((rc = prof_begin(m, m->s_gmm, 1, &ep))) return rc;
  HIP_TRY(launch());
  if ((rc = prof_end(m, m->s_gmm, &ep))) return rc;
  HIP_TRY(hipStreamSynchronize(m->s_gmm));
  HIP_TRY(hipMemcpy(out_beta, c->fm_beta.p, sizeof(double) * n_groups, hipMemcpyDeviceToHost));
  HIP_TRY(hipMemcpy(out_k, c->fm_k.p, sizeof(double) * nk, hipMemcpyDeviceToHost));
  HIP_TRY(hipMemcpy(out_G, c->fm_G.p, sizeof(double) * nG, hipMemcpyDeviceToHost));
  return SR_OK;
}

// ---- fMLLR speaker adaptation (fmllr_stats.hip; the estimate itself is host code, fmllr.cpp) ---------------------------------------
// The checks every statistics call makes before any launch
static int fmllr_check(sr_model* m, sr_corpus* c, const uint32_t* utt_speaker, uint32_t n_speakers, const double* out_beta,
                       const double* out_k, const double* out_G) {
  int rc = check_corpus(m, c);
  if (rc) return rc;
  if (!out_beta || !out_k || !out_G) return fail(SR_EINVAL, "null output");
  if (n_speakers == 0) return fail(SR_EINVAL, "n_speakers is 0");
  if ((rc = speaker_check(m, c, utt_speaker, n_speakers, "fMLLR statistics"))) return rc;
  const uint32_t D = m->dim;
  size_t free_b = 0, total_b = 0;
  HIP_TRY(hipMemGetInfo(&free_b, &total_b));
  const double g_bytes = 8.0 * (double)n_speakers * D * (D + 1) * (D + 1);
  if (g_bytes > (double)free_b / 4)
    return fail(SR_ELIMIT, "G of %u speakers (%.0f bytes) exceeds a quarter of the free device memory (%llu bytes)", n_speakers, g_bytes,
                (unsigned long long)free_b);
  return SR_OK;
}

// fold, contraction and reduction over the pairs `e` describes (formed already: frame t's at [pair_off[t], pair_off[t + 1])), per
// speaker; the results to the host
static int fmllr_statistics(sr_model* m, sr_corpus* c, const EmArgs& e, const uint64_t* d_frame_pair_off, const uint32_t* utt_speaker,
                            uint32_t S, double* out_beta, double* out_k, double* out_G) {
  const uint32_t D = m->dim, U = c->n_utts;
  const uint64_t F = c->n_frames;
  int rc;
  // every speaker's frames in corpus order, cut into segments
  std::vector<uint32_t> spk_frames(S + 1, 0), frame_list(F);
  for (uint32_t u = 0; u < U; u++) spk_frames[utt_speaker[u] + 1] += (uint32_t)(c->frame_off[u + 1] - c->frame_off[u]);
  for (uint32_t s = 0; s < S; s++) spk_frames[s + 1] += spk_frames[s];
  {
    std::vector<uint32_t> fill(spk_frames.begin(), spk_frames.end() - 1);
    for (uint32_t u = 0; u < U; u++)
      for (uint64_t f = c->frame_off[u]; f < c->frame_off[u + 1]; f++) frame_list[fill[utt_speaker[u]]++] = (uint32_t)f;
  }
  const srplan::Segments seg(spk_frames.data(), S, fmllr_seg_frames());
  FmllrArgs a{};
  a.feats = c->feats.p; a.n_frames = F; a.dim = D; a.g.shape = fmllr_shape(D);
  a.means = m->means.p; a.inv_vars = m->inv_vars.p;
  a.frame_pair_off = d_frame_pair_off; a.pair_dens = e.pair_dens; a.pair_key = e.key_mean; a.pair_w = e.pair_w;
  HIP_TRY(c->fm_fold_a.ensure((size_t)F * a.g.shape.rows)); HIP_TRY(c->fm_fold_c.ensure((size_t)F * a.g.shape.rows));
  HIP_TRY(c->fm_frame_list.upload(frame_list.data(), F));
  a.fold_a = c->fm_fold_a.p; a.fold_c = c->fm_fold_c.p; a.frame_list = c->fm_frame_list.p;
  if ((rc = grouped_statistics(m, c, seg, S, &a.g, [&] { return launch_fmllr_statistics(a, m->s_gmm); }, out_beta, out_k, out_G))) return rc;
  if (m->profiling) {  // per frame: the fold's two rows out and in, the features; the partials out and in
    m->prof.frames += F;
    m->prof.search_bytes += (double)F * (32.0 * a.g.shape.rows + 4.0 * D) + 16.0 * (double)a.g.n_segs * a.g.shape.rows * a.g.shape.cols;
  }
  return SR_OK;
}

int sr_fmllr_statistics_corpus(sr_model* m, sr_corpus* c, const uint16_t* states, const uint32_t* utt_speaker, uint32_t n_speakers,
                               int max_approx, double* out_beta, double* out_k, double* out_G) {
  return guarded(__func__, [&]() -> int {
  int rc = fmllr_check(m, c, utt_speaker, n_speakers, out_beta, out_k, out_G);
  if (rc) return rc;
  EmArgs e{};
  if ((rc = adapt_pairs(m, c, states, max_approx, &e))) return rc;
  if (e.n_pairs == 0) return adapt_zero(m->dim, n_speakers, out_beta, out_k, out_G);
  return fmllr_statistics(m, c, e, c->pair_off.p, utt_speaker, n_speakers, out_beta, out_k, out_G);
  });
}

int sr_fmllr_statistics_bw_corpus(sr_model* m, sr_corpus* c, const uint16_t* automata, const uint64_t* aut_off, const double tdp[3],
                                  uint16_t silence_state, int gmm_kernel, double posterior_floor, const uint32_t* utt_speaker,
                                  uint32_t n_speakers, int max_approx, double* out_cost, double* out_beta, double* out_k, double* out_G) {
  return guarded(__func__, [&]() -> int {
  int rc = fmllr_check(m, c, utt_speaker, n_speakers, out_beta, out_k, out_G);
  if (rc) return rc;
  EmArgs e{};
  if ((rc = adapt_pairs_bw(m, c, automata, aut_off, tdp, silence_state, gmm_kernel, posterior_floor, max_approx, out_cost, &e))) return rc;
  if (e.n_pairs == 0) return adapt_zero(m->dim, n_speakers, out_beta, out_k, out_G);
  HIP_TRY(c->fm_frame_pair_off.ensure(c->n_frames + 1));
  HIP_TRY(launch_fmllr_item_frames(c->fb_item_off.p, c->fb_pair_end.p, c->n_frames, c->fm_frame_pair_off.p, m->s_gmm));
  return fmllr_statistics(m, c, e, c->fm_frame_pair_off.p, utt_speaker, n_speakers, out_beta, out_k, out_G);
  });
}

int sr_corpus_transform(sr_model* m, sr_corpus* c, const uint32_t* utt_speaker, uint32_t n_speakers, const double* W, sr_corpus** out) {
  return guarded(__func__, [&]() -> int {
  if (!out) return fail(SR_EINVAL, "out is null");
  *out = nullptr;
  int rc = check_corpus(m, c);
  if (rc) return rc;
  if (n_speakers == 0) return fail(SR_EINVAL, "n_speakers is 0");
  if (!W) return fail(SR_EINVAL, "W is null");
  if ((rc = speaker_check(m, c, utt_speaker, n_speakers, "fMLLR transform"))) return rc;
  const uint32_t D = m->dim;
  const uint64_t F = c->n_frames;
  if ((rc = srhost::corpus_ready(c, 0, F, m->s_gmm))) return rc;  // an asynchronous upload of c: wait for all of it
  sr_corpus* t = new sr_corpus();
  std::unique_ptr<sr_corpus, int (*)(sr_corpus*)> own(t, sr_corpus_destroy);
  t->model = m; t->n_utts = c->n_utts; t->n_frames = F;
  srhost::corpus_register(t);
  t->frame_off = c->frame_off;
  HIP_TRY(t->feats.ensure((size_t)F * D + 64));
  HIP_TRY(t->d_frame_off.upload(t->frame_off.data(), t->frame_off.size()));
  DevBuf<uint32_t> d_spk;
  DevBuf<double> d_W;
  HIP_TRY(d_spk.upload(utt_speaker, c->n_utts));
  HIP_TRY(d_W.upload(W, (size_t)n_speakers * D * (D + 1)));
  EventPair ep{};
  if ((rc = prof_begin(m, m->s_gmm, 1, &ep))) return rc;
  HIP_TRY(launch_fmllr_transform(c->feats.p, t->d_frame_off.p, t->n_utts, d_spk.p, d_W.p, D, t->feats.p, m->s_gmm));
  if ((rc = prof_end(m, m->s_gmm, &ep))) return rc;
  HIP_TRY(hipStreamSynchronize(m->s_gmm));
  if (m->profiling) {  // a row in, a row out
    m->prof.frames += F;
    m->prof.search_bytes += 8.0 * (double)F * D;
  }
  *out = own.release();
  return SR_OK;
  });
}

// ---- MLLR of the means (mllr_stats.hip; the estimate itself is host code, mllr.cpp) -------------------------------------------------
// The checks every statistics call makes before any launch
static int mllr_check(sr_model* m, sr_corpus* c, const uint32_t* utt_speaker, uint32_t n_speakers, const uint32_t* dens_class,
                      uint32_t n_classes, const double* out_beta, const double* out_k, const double* out_G) {
  int rc = check_corpus(m, c);
  if (rc) return rc;
  if (!out_beta || !out_k || !out_G) return fail(SR_EINVAL, "null output");
  if (n_speakers == 0) return fail(SR_EINVAL, "n_speakers is 0");
  if (n_classes == 0) return fail(SR_EINVAL, "n_classes is 0");
  if (!dens_class && m->n_dens) return fail(SR_EINVAL, "dens_class is null");
  for (uint64_t d = 0; d < m->n_dens; d++)
    if (dens_class[d] >= n_classes) return fail(SR_EINVAL, "density %llu: class %u >= n_classes %u", (unsigned long long)d, dens_class[d], n_classes);
  if ((rc = speaker_check(m, c, utt_speaker, n_speakers, "MLLR statistics"))) return rc;
  const uint32_t D = m->dim;
  if ((uint64_t)n_speakers * m->n_dens >= 0xFFFFFFFFull)
    return fail(SR_ELIMIT, "n_speakers * densities = %llu does not fit the 32-bit (speaker, density) keys", (unsigned long long)n_speakers * m->n_dens);
  size_t free_b = 0, total_b = 0;
  HIP_TRY(hipMemGetInfo(&free_b, &total_b));
  const double groups = (double)n_speakers * n_classes, out_bytes = 8.0 * groups * (1.0 + (double)D * (D + 1) * (D + 2));
  if (out_bytes > (double)free_b / 4 || groups >= 4294967295.0)
    return fail(SR_ELIMIT, "the statistics of %u speakers x %u classes (%.0f bytes) exceed a quarter of the free device memory (%llu bytes)",
                n_speakers, n_classes, out_bytes, (unsigned long long)free_b);
  return SR_OK;
}

// entries, contraction and reduction over the pairs `e` describes (formed already), per (speaker, class); the results to the host
static int mllr_statistics(sr_model* m, sr_corpus* c, const EmArgs& e, const uint32_t* utt_speaker, uint32_t S, const uint32_t* dens_class,
                           uint32_t R, double* out_beta, double* out_k, double* out_G) {
  const uint32_t D = m->dim, U = c->n_utts, E = D + 1, n_groups = S * R;
  const uint64_t F = c->n_frames, n_pairs = e.n_pairs;
  int rc;
  std::vector<uint32_t> frame_speaker(F);
  for (uint32_t u = 0; u < U; u++) std::fill(frame_speaker.begin() + c->frame_off[u], frame_speaker.begin() + c->frame_off[u + 1], utt_speaker[u]);
  MllrArgs a{};
  a.feats = c->feats.p; a.dim = D; a.g.shape = fmllr_shape(D); a.means = m->means.p; a.inv_vars = m->inv_vars.p;
  a.n_pairs = n_pairs; a.pair_frame = e.pair_frame; a.pair_dens = e.pair_dens; a.pair_key = e.key_mean; a.pair_w = e.pair_w;
  a.n_dens = (uint32_t)m->n_dens; a.n_speakers = S; a.n_classes = R;
  HIP_TRY(c->ml_frame_speaker.upload(frame_speaker.data(), F)); HIP_TRY(c->ml_dens_class.upload(dens_class, m->n_dens));
  HIP_TRY(c->ml_key.ensure(n_pairs)); HIP_TRY(c->iota.ensure(n_pairs)); HIP_TRY(c->keys_sorted.ensure(n_pairs));
  HIP_TRY(c->pairs_sorted.ensure(n_pairs)); HIP_TRY(c->ml_run_key.ensure(n_pairs)); HIP_TRY(c->ml_run_len.ensure(n_pairs));
  HIP_TRY(c->ml_run_begin.ensure(n_pairs)); HIP_TRY(c->ml_n_runs.ensure(1));
  a.sort_temp_bytes = mllr_temp_bytes(n_pairs);
  HIP_TRY(c->sort_temp.ensure(a.sort_temp_bytes));
  a.frame_speaker = c->ml_frame_speaker.p; a.dens_class = c->ml_dens_class.p; a.key = c->ml_key.p; a.iota = c->iota.p;
  a.keys_sorted = c->keys_sorted.p; a.pairs_sorted = c->pairs_sorted.p; a.run_key = c->ml_run_key.p; a.run_len = c->ml_run_len.p;
  a.run_begin = c->ml_run_begin.p; a.n_runs = c->ml_n_runs.p; a.sort_temp = c->sort_temp.p;
  EventPair ep{};
  if ((rc = prof_begin(m, m->s_gmm, 1, &ep))) return rc;
  HIP_TRY(launch_mllr_runs(a, m->s_gmm));
  if ((rc = prof_end(m, m->s_gmm, &ep))) return rc;
  HIP_TRY(hipStreamSynchronize(m->s_gmm));
  uint32_t n_runs = 0, last_key = 0;
  HIP_TRY(hipMemcpy(&n_runs, c->ml_n_runs.p, sizeof(uint32_t), hipMemcpyDeviceToHost));
  if (n_runs == 0 || n_runs > n_pairs) return fail(SR_EINTERNAL, "MLLR statistics: %u runs of %llu pairs", n_runs, (unsigned long long)n_pairs);
  HIP_TRY(hipMemcpy(&last_key, c->ml_run_key.p + (n_runs - 1), sizeof(uint32_t), hipMemcpyDeviceToHost));
  a.n_entries = n_runs - (last_key == 0xFFFFFFFFu ? 1u : 0u);  // the dropped pairs sort behind every key
  const size_t ne = std::max<uint32_t>(1, a.n_entries);
  HIP_TRY(c->ml_gkey.ensure(ne)); HIP_TRY(c->ml_gkey_sorted.ensure(ne)); HIP_TRY(c->ml_ent_order.ensure(ne));
  HIP_TRY(c->ml_grp_begin.ensure((size_t)n_groups + 1)); HIP_TRY(c->ml_ent_dens.ensure(ne)); HIP_TRY(c->ml_ent_occ.ensure(ne));
  HIP_TRY(c->ml_ent_x.ensure(ne * D));
  a.gkey = c->ml_gkey.p; a.gkey_sorted = c->ml_gkey_sorted.p; a.ent_order = c->ml_ent_order.p; a.grp_begin = c->ml_grp_begin.p;
  a.ent_dens = c->ml_ent_dens.p; a.ent_occ = c->ml_ent_occ.p; a.ent_x = c->ml_ent_x.p;
  if ((rc = prof_begin(m, m->s_gmm, 1, &ep))) return rc;
  HIP_TRY(launch_mllr_groups(a, m->s_gmm));
  if ((rc = prof_end(m, m->s_gmm, &ep))) return rc;
  HIP_TRY(hipStreamSynchronize(m->s_gmm));
  // every group's entries, cut into segments
  std::vector<uint32_t> grp_begin((size_t)n_groups + 1);
  HIP_TRY(hipMemcpy(grp_begin.data(), c->ml_grp_begin.p, sizeof(uint32_t) * grp_begin.size(), hipMemcpyDeviceToHost));
  if (grp_begin[0] != 0 || grp_begin[n_groups] != a.n_entries) return fail(SR_EINTERNAL, "MLLR statistics: the groups do not cover the entries");
  if (!std::is_sorted(grp_begin.begin(), grp_begin.end())) return fail(SR_EINTERNAL, "MLLR statistics: group bounds out of order");
  const srplan::Segments seg(grp_begin.data(), n_groups, fmllr_seg_frames());
  if ((rc = grouped_statistics(m, c, seg, n_groups, &a.g, [&] { return launch_mllr_statistics(a, m->s_gmm); }, out_beta, out_k, out_G))) return rc;
  if (m->profiling) {  // per pair: keys and sort, weight, frame, a feature row; per entry: its sums out and in; the partials out and in
    m->prof.frames += F;
    m->prof.search_bytes += (double)n_pairs * (40.0 + 4.0 * D) + 16.0 * (double)a.n_entries * E +
                            16.0 * (double)a.g.n_segs * a.g.shape.rows * a.g.shape.cols;
  }
  return SR_OK;
}

int sr_mllr_statistics_corpus(sr_model* m, sr_corpus* c, const uint16_t* states, const uint32_t* utt_speaker, uint32_t n_speakers,
                              const uint32_t* dens_class, uint32_t n_classes, int max_approx, double* out_beta, double* out_k,
                              double* out_G) {
  return guarded(__func__, [&]() -> int {
  int rc = mllr_check(m, c, utt_speaker, n_speakers, dens_class, n_classes, out_beta, out_k, out_G);
  if (rc) return rc;
  EmArgs e{};
  if ((rc = adapt_pairs(m, c, states, max_approx, &e))) return rc;
  if (e.n_pairs == 0) return adapt_zero(m->dim, (uint64_t)n_speakers * n_classes, out_beta, out_k, out_G);
  return mllr_statistics(m, c, e, utt_speaker, n_speakers, dens_class, n_classes, out_beta, out_k, out_G);
  });
}

int sr_mllr_statistics_bw_corpus(sr_model* m, sr_corpus* c, const uint16_t* automata, const uint64_t* aut_off, const double tdp[3],
                                 uint16_t silence_state, int gmm_kernel, double posterior_floor, const uint32_t* utt_speaker,
                                 uint32_t n_speakers, const uint32_t* dens_class, uint32_t n_classes, int max_approx, double* out_cost,
                                 double* out_beta, double* out_k, double* out_G) {
  return guarded(__func__, [&]() -> int {
  int rc = mllr_check(m, c, utt_speaker, n_speakers, dens_class, n_classes, out_beta, out_k, out_G);
  if (rc) return rc;
  EmArgs e{};
  if ((rc = adapt_pairs_bw(m, c, automata, aut_off, tdp, silence_state, gmm_kernel, posterior_floor, max_approx, out_cost, &e))) return rc;
  if (e.n_pairs == 0) return adapt_zero(m->dim, (uint64_t)n_speakers * n_classes, out_beta, out_k, out_G);
  return mllr_statistics(m, c, e, utt_speaker, n_speakers, dens_class, n_classes, out_beta, out_k, out_G);
  });
}

// What a speaker-adapted model (sr_model_transform_means, sr_model_map_adapt) takes over from its prior `m`: the topology, the tying
// tables on device and host, and the inverse variances and norms, copied on the device.  means and logw are sized; the caller fills them.
static int adapted_model_shell(sr_model* m, std::unique_ptr<sr_model, int (*)(sr_model*)>& own) {
  const uint64_t C = m->n_dens, D = m->dim;
  sr_model* o = nullptr;
  int rc = srhost::model_shell(m->device, m->dim, m->n_states, m->h_dens_off.data(), m->max_approx ? 1 : 0, &o);
  if (rc) return rc;
  own.reset(o);
  HIP_TRY(o->dens_mean.upload(m->h_dens_mean.data(), C)); HIP_TRY(o->dens_var.upload(m->h_dens_var.data(), C));
  o->n_mean = m->n_mean; o->n_var = m->n_var; o->h_dens_mean = m->h_dens_mean; o->h_dens_var = m->h_dens_var;
  HIP_TRY(o->means.ensure(C * D)); HIP_TRY(o->inv_vars.ensure(C * D)); HIP_TRY(o->norm.ensure(C)); HIP_TRY(o->logw.ensure(C));
  if (C) {
    HIP_TRY(hipMemcpy(o->inv_vars.p, m->inv_vars.p, sizeof(double) * C * D, hipMemcpyDeviceToDevice));
    HIP_TRY(hipMemcpy(o->norm.p, m->norm.p, sizeof(double) * C, hipMemcpyDeviceToDevice));
  }
  return SR_OK;
}

int sr_model_transform_means(sr_model* m, const uint32_t* dens_class, uint32_t n_classes, const double* W, sr_model** out) {
  return guarded(__func__, [&]() -> int {
  if (!out) return fail(SR_EINVAL, "out is null");
  *out = nullptr;
  int rc = check_model(m);
  if (rc) return rc;
  if (n_classes == 0) return fail(SR_EINVAL, "n_classes is 0");
  if (!W) return fail(SR_EINVAL, "W is null");
  if (!dens_class && m->n_dens) return fail(SR_EINVAL, "dens_class is null");
  const uint64_t C = m->n_dens;
  const uint32_t D = m->dim;
  if (m->h_dens_mean.size() != C || m->h_dens_var.size() != C) return fail(SR_EINTERNAL, "the model has no tying tables");
  std::vector<uint32_t> row_class(m->n_mean, 0xFFFFFFFFu), class_off((size_t)n_classes + 1, 0);
  for (uint64_t d = 0; d < C; d++) {
    if (dens_class[d] >= n_classes) return fail(SR_EINVAL, "density %llu: class %u >= n_classes %u", (unsigned long long)d, dens_class[d], n_classes);
    uint32_t& rc_ = row_class[m->h_dens_mean[d]];
    if (rc_ != 0xFFFFFFFFu && rc_ != dens_class[d])
      return fail(SR_EINVAL, "density %llu: its mean row %u is shared with a density of class %u, not %u", (unsigned long long)d,
                  m->h_dens_mean[d], rc_, dens_class[d]);
    rc_ = dens_class[d];
    class_off[dens_class[d] + 1]++;
  }
  if (D > fmllr_max_dim()) return fail(SR_ELIMIT, "dimension %u exceeds %u (MLLR mean transform)", D, fmllr_max_dim());
  // the densities by (class, id); a workgroup takes at most mllr_dens_per_block() of one class
  for (uint32_t r = 0; r < n_classes; r++) class_off[r + 1] += class_off[r];
  std::vector<uint32_t> order(std::max<uint64_t>(1, C)), blk;
  {
    std::vector<uint32_t> fill(class_off.begin(), class_off.end() - 1);
    for (uint64_t d = 0; d < C; d++) order[fill[dens_class[d]]++] = (uint32_t)d;
  }
  const uint32_t per = mllr_dens_per_block();
  for (uint32_t r = 0; r < n_classes; r++)
    for (uint32_t b = class_off[r]; b < class_off[r + 1]; b += per) {
      blk.push_back(r); blk.push_back(b); blk.push_back(std::min(class_off[r + 1], b + per));
    }
  std::unique_ptr<sr_model, int (*)(sr_model*)> own(nullptr, sr_model_destroy);
  if ((rc = adapted_model_shell(m, own))) return rc;
  sr_model* o = own.get();
  if (C) HIP_TRY(hipMemcpy(o->logw.p, m->logw.p, sizeof(double) * C, hipMemcpyDeviceToDevice));
  DevBuf<uint32_t> d_order, d_blk;
  DevBuf<double> d_W;
  HIP_TRY(d_order.upload(order.data(), order.size())); HIP_TRY(d_blk.upload(blk.data(), blk.size()));
  HIP_TRY(d_W.upload(W, (size_t)n_classes * D * (D + 1)));
  HIP_TRY(launch_mllr_transform_means(m->means.p, d_order.p, d_blk.p, (uint32_t)(blk.size() / 3), d_W.p, D, o->means.p, o->s_gmm));
  HIP_TRY(hipStreamSynchronize(o->s_gmm));
  *out = own.release();
  return SR_OK;
  });
}

// ---- MAP adaptation of the means (map_stats.hip; checks, the mean rows' plan and the weight update are host code, map.cpp) -----------
// The checks every statistics call makes before any launch
static int map_check(sr_model* m, sr_corpus* c, const uint32_t* utt_speaker, uint32_t n_speakers, const uint64_t* out_ent_off,
                     const uint32_t* out_dens, const double* out_occ, const double* out_x) {
  int rc = check_corpus(m, c);
  if (rc) return rc;
  if (!out_ent_off) return fail(SR_EINVAL, "out_ent_off is null");
  const int given = (out_dens ? 1 : 0) + (out_occ ? 1 : 0) + (out_x ? 1 : 0);
  if (given != 0 && given != 3) return fail(SR_EINVAL, "null output (pass all three entry arrays, or none)");
  if (n_speakers == 0) return fail(SR_EINVAL, "n_speakers is 0");
  if ((rc = speaker_check(m, c, utt_speaker, n_speakers, nullptr))) return rc;
  if ((uint64_t)n_speakers * m->n_dens >= 0xFFFFFFFFull)
    return fail(SR_ELIMIT, "n_speakers * densities = %llu does not fit the 32-bit (speaker, density) keys", (unsigned long long)n_speakers * m->n_dens);
  return SR_OK;
}

// runs, plan and sums over the pairs `e` describes (formed already); the counts, and the entries where asked for, to the host
static int map_statistics(sr_model* m, sr_corpus* c, const EmArgs& e, const uint32_t* utt_speaker, uint32_t S, uint64_t cap,
                          uint64_t* out_ent_off, uint32_t* out_dens, double* out_occ, double* out_x) {
  const uint32_t D = m->dim, U = c->n_utts;
  const uint64_t F = c->n_frames, n_pairs = e.n_pairs;
  int rc;
  if (n_pairs == 0) {  // no frame, or nothing above the floor: no entry
    std::fill(out_ent_off, out_ent_off + S + 1, (uint64_t)0);
    return SR_OK;
  }
  std::vector<uint32_t> frame_speaker(F);
  for (uint32_t u = 0; u < U; u++) std::fill(frame_speaker.begin() + c->frame_off[u], frame_speaker.begin() + c->frame_off[u + 1], utt_speaker[u]);
  MllrArgs r{};  // launch_mllr_runs' share
  r.n_pairs = n_pairs; r.pair_frame = e.pair_frame; r.pair_dens = e.pair_dens; r.pair_key = e.key_mean; r.pair_w = e.pair_w;
  r.n_dens = (uint32_t)m->n_dens; r.n_speakers = S;
  HIP_TRY(c->ml_frame_speaker.upload(frame_speaker.data(), F));
  HIP_TRY(c->ml_key.ensure(n_pairs)); HIP_TRY(c->iota.ensure(n_pairs)); HIP_TRY(c->keys_sorted.ensure(n_pairs));
  HIP_TRY(c->pairs_sorted.ensure(n_pairs)); HIP_TRY(c->ml_run_key.ensure(n_pairs)); HIP_TRY(c->ml_run_len.ensure(n_pairs));
  HIP_TRY(c->ml_n_runs.ensure(1));
  r.sort_temp_bytes = map_temp_bytes(n_pairs);
  HIP_TRY(c->sort_temp.ensure(r.sort_temp_bytes));
  r.frame_speaker = c->ml_frame_speaker.p; r.key = c->ml_key.p; r.iota = c->iota.p; r.keys_sorted = c->keys_sorted.p;
  r.pairs_sorted = c->pairs_sorted.p; r.run_key = c->ml_run_key.p; r.run_len = c->ml_run_len.p; r.n_runs = c->ml_n_runs.p;
  r.sort_temp = c->sort_temp.p;
  MapArgs a{};
  a.feats = c->feats.p; a.dim = D; a.n_pairs = n_pairs; a.pair_frame = e.pair_frame; a.pair_w = e.pair_w;
  a.pairs_sorted = r.pairs_sorted; a.run_key = r.run_key; a.run_len = r.run_len; a.n_runs = r.n_runs;
  a.n_dens = r.n_dens; a.n_speakers = S;
  HIP_TRY(c->map_cnt.ensure(n_pairs + 1)); HIP_TRY(c->map_scan.ensure(n_pairs + 1));
  HIP_TRY(c->map_seg_ent.ensure(n_pairs + n_pairs / map_seg_pairs() + 1));
  HIP_TRY(c->map_counts.ensure(2)); HIP_TRY(c->map_ent_off.ensure((size_t)S + 1));
  a.cnt = c->map_cnt.p; a.scan = c->map_scan.p; a.seg_ent = c->map_seg_ent.p; a.counts = c->map_counts.p; a.ent_off = c->map_ent_off.p;
  a.temp = r.sort_temp; a.temp_bytes = r.sort_temp_bytes;
  EventPair ep{};
  if ((rc = prof_begin(m, m->s_gmm, 1, &ep))) return rc;
  HIP_TRY(launch_mllr_runs(r, m->s_gmm));
  HIP_TRY(launch_map_plan(a, m->s_gmm));
  if ((rc = prof_end(m, m->s_gmm, &ep))) return rc;
  HIP_TRY(hipStreamSynchronize(m->s_gmm));
  uint32_t counts[2] = {0, 0};
  std::vector<uint32_t> ent_off((size_t)S + 1);
  HIP_TRY(hipMemcpy(counts, c->map_counts.p, sizeof counts, hipMemcpyDeviceToHost));
  HIP_TRY(hipMemcpy(ent_off.data(), c->map_ent_off.p, sizeof(uint32_t) * ent_off.size(), hipMemcpyDeviceToHost));
  a.n_entries = counts[0]; a.n_segs = counts[1];
  if (a.n_entries > n_pairs || a.n_segs < a.n_entries || a.n_segs > a.n_entries + n_pairs / map_seg_pairs())
    return fail(SR_EINTERNAL, "MAP statistics: %u entries in %u segments of %llu pairs", a.n_entries, a.n_segs, (unsigned long long)n_pairs);
  if (ent_off[0] != 0 || ent_off[S] != a.n_entries || !std::is_sorted(ent_off.begin(), ent_off.end()))
    return fail(SR_EINTERNAL, "MAP statistics: the speakers do not cover the entries");
  std::copy(ent_off.begin(), ent_off.end(), out_ent_off);
  if (m->profiling) {  // per pair: keys and sort
    m->prof.frames += F;
    m->prof.search_bytes += (double)n_pairs * 40.0;
  }
  if (!out_dens) return SR_OK;  // the sizing call
  if (a.n_entries > cap)
    return fail(SR_EINVAL, "%u entries exceed the capacity of %llu (out_ent_off holds the counts)", a.n_entries, (unsigned long long)cap);
  if (a.n_entries == 0) return SR_OK;  // every pair was dropped
  const size_t ne = a.n_entries;
  HIP_TRY(c->ml_ent_dens.ensure(ne)); HIP_TRY(c->ml_ent_occ.ensure(ne)); HIP_TRY(c->ml_ent_x.ensure(ne * D));
  HIP_TRY(c->map_partial.ensure(a.n_segs > a.n_entries ? (size_t)a.n_segs * (D + 1) : 1));
  a.partial = c->map_partial.p; a.out_dens = c->ml_ent_dens.p; a.out_occ = c->ml_ent_occ.p; a.out_x = c->ml_ent_x.p;
  if ((rc = prof_begin(m, m->s_gmm, 1, &ep))) return rc;
  HIP_TRY(launch_map_sums(a, m->s_gmm));
  if ((rc = prof_end(m, m->s_gmm, &ep))) return rc;
  HIP_TRY(hipStreamSynchronize(m->s_gmm));
  HIP_TRY(hipMemcpy(out_dens, a.out_dens, sizeof(uint32_t) * ne, hipMemcpyDeviceToHost));
  HIP_TRY(hipMemcpy(out_occ, a.out_occ, sizeof(double) * ne, hipMemcpyDeviceToHost));
  HIP_TRY(hipMemcpy(out_x, a.out_x, sizeof(double) * ne * D, hipMemcpyDeviceToHost));
  if (m->profiling)  // per pair: weight, frame, a feature row; per entry: its sums out; the partials out and in
    m->prof.search_bytes += (double)n_pairs * (16.0 + 4.0 * D) + 8.0 * (double)ne * (D + 2) +
                            (a.n_segs > a.n_entries ? 16.0 * (double)a.n_segs * (D + 1) : 0.0);
  return SR_OK;
}

int sr_map_statistics_corpus(sr_model* m, sr_corpus* c, const uint16_t* states, const uint32_t* utt_speaker, uint32_t n_speakers,
                             int max_approx, uint64_t cap, uint64_t* out_ent_off, uint32_t* out_dens, double* out_occ, double* out_x) {
  return guarded(__func__, [&]() -> int {
  int rc = map_check(m, c, utt_speaker, n_speakers, out_ent_off, out_dens, out_occ, out_x);
  if (rc) return rc;
  EmArgs e{};
  if ((rc = adapt_pairs(m, c, states, max_approx, &e))) return rc;
  return map_statistics(m, c, e, utt_speaker, n_speakers, cap, out_ent_off, out_dens, out_occ, out_x);
  });
}

int sr_map_statistics_bw_corpus(sr_model* m, sr_corpus* c, const uint16_t* automata, const uint64_t* aut_off, const double tdp[3],
                                uint16_t silence_state, int gmm_kernel, double posterior_floor, const uint32_t* utt_speaker,
                                uint32_t n_speakers, int max_approx, double* out_cost, uint64_t cap, uint64_t* out_ent_off,
                                uint32_t* out_dens, double* out_occ, double* out_x) {
  return guarded(__func__, [&]() -> int {
  int rc = map_check(m, c, utt_speaker, n_speakers, out_ent_off, out_dens, out_occ, out_x);
  if (rc) return rc;
  EmArgs e{};
  if ((rc = adapt_pairs_bw(m, c, automata, aut_off, tdp, silence_state, gmm_kernel, posterior_floor, max_approx, out_cost, &e))) return rc;
  return map_statistics(m, c, e, utt_speaker, n_speakers, cap, out_ent_off, out_dens, out_occ, out_x);
  });
}

int sr_model_map_adapt(sr_model* prior, uint64_t n_entries, const uint32_t* dens, const double* occ, const double* x, double tau,
                       int update_weights, double tau_w, sr_model** out) {
  return guarded(__func__, [&]() -> int {
  if (!out) return fail(SR_EINVAL, "out is null");
  *out = nullptr;
  sr_model* m = prior;
  int rc = check_model(m);
  if (rc) return rc;
  const uint64_t C = m->n_dens;
  const uint32_t D = m->dim;
  if (m->h_dens_mean.size() != C || m->h_dens_var.size() != C) return fail(SR_EINTERNAL, "the model has no tying tables");
  if ((rc = map_host::validate(C, D, n_entries, dens, occ, x, tau, update_weights, tau_w))) return rc;
  map_host::Plan plan;
  map_host::plan(C, m->n_mean, m->h_dens_mean.data(), n_entries, dens, &plan);
  std::vector<double> logw;
  if (update_weights && n_entries) {  // C doubles from the device where the model keeps no host copy
    logw.resize(C);
    if (m->h_logw.size() == C) logw = m->h_logw;
    else HIP_TRY(hipMemcpy(logw.data(), m->logw.p, sizeof(double) * C, hipMemcpyDeviceToHost));
    map_host::update_weights(m->n_states, m->h_dens_off.data(), n_entries, dens, occ, tau_w, logw.data());
  }
  std::unique_ptr<sr_model, int (*)(sr_model*)> own(nullptr, sr_model_destroy);
  if ((rc = adapted_model_shell(m, own))) return rc;
  sr_model* o = own.get();
  if (C) {
    if (logw.empty()) HIP_TRY(hipMemcpy(o->logw.p, m->logw.p, sizeof(double) * C, hipMemcpyDeviceToDevice));
    else HIP_TRY(hipMemcpy(o->logw.p, logw.data(), sizeof(double) * C, hipMemcpyHostToDevice));
  }
  DevBuf<uint32_t> d_slot, d_off, d_ent, d_rep;
  DevBuf<double> d_occ, d_x;
  const size_t ne = std::max<uint64_t>(1, n_entries);
  HIP_TRY(d_slot.upload(plan.row_slot.data(), plan.row_slot.size())); HIP_TRY(d_off.upload(plan.row_off.data(), plan.row_off.size()));
  HIP_TRY(d_ent.ensure(ne)); HIP_TRY(d_rep.ensure(ne)); HIP_TRY(d_occ.ensure(ne)); HIP_TRY(d_x.ensure(ne * D));
  if (n_entries) {
    HIP_TRY(hipMemcpy(d_ent.p, plan.row_ent.data(), sizeof(uint32_t) * n_entries, hipMemcpyHostToDevice));
    HIP_TRY(hipMemcpy(d_rep.p, plan.row_rep.data(), sizeof(uint32_t) * plan.row_rep.size(), hipMemcpyHostToDevice));
    HIP_TRY(hipMemcpy(d_occ.p, occ, sizeof(double) * n_entries, hipMemcpyHostToDevice));
    HIP_TRY(hipMemcpy(d_x.p, x, sizeof(double) * n_entries * D, hipMemcpyHostToDevice));
  }
  MapMeansArgs a{};
  a.means = m->means.p; a.dens_mean = o->dens_mean.p; a.row_slot = d_slot.p; a.row_off = d_off.p; a.row_ent = d_ent.p; a.row_rep = d_rep.p;
  a.occ = d_occ.p; a.x = d_x.p; a.tau = tau; a.dim = D; a.n_dens = C; a.out = o->means.p;
  HIP_TRY(launch_map_means(a, o->s_gmm));
  HIP_TRY(hipStreamSynchronize(o->s_gmm));
  *out = own.release();
  return SR_OK;
  });
}

// ---- MLLT, the global semi-tied covariance transform (mllt_stats.hip; the estimate itself is host code, mllt.cpp) -------------------
// The checks every statistics call makes before any launch
static int mllt_check(sr_model* m, sr_corpus* c, const double* out_beta, const double* out_G) {
  int rc = check_corpus(m, c);
  if (rc) return rc;
  if (!out_beta || !out_G) return fail(SR_EINVAL, "null output");
  if (m->dim > mllt_max_dim()) return fail(SR_ELIMIT, "dimension %u exceeds %u (MLLT statistics)", m->dim, mllt_max_dim());
  const MlltShape s = mllt_shape(m->dim);
  const size_t seg_bytes = sizeof(double) * s.rows * s.cols;
  if (seg_bytes > m->mllt_budget)
    return fail(SR_ELIMIT, "one segment's partial sums (%llu bytes) exceed the MLLT workspace of %llu (SRGPU_MLLT_MB)",
                (unsigned long long)seg_bytes, (unsigned long long)m->mllt_budget);
  return SR_OK;
}

// contraction and reduction over the pairs `e` describes (formed already), in rounds of as many consecutive segments as the workspace
// holds; the results to the host
static int mllt_statistics(sr_model* m, sr_corpus* c, const EmArgs& e, double* out_beta, double* out_G) {
  const uint32_t D = m->dim;
  const size_t nG = (size_t)D * D * D;
  if (e.n_pairs == 0) {  // no frame, or nothing above the floor
    *out_beta = 0.0;
    std::fill(out_G, out_G + nG, 0.0);
    return SR_OK;
  }
  int rc;
  MlltArgs a{};
  a.feats = c->feats.p; a.dim = D; a.shape = mllt_shape(D); a.means = m->means.p; a.inv_vars = m->inv_vars.p;
  a.n_pairs = e.n_pairs; a.pair_frame = e.pair_frame; a.pair_dens = e.pair_dens; a.pair_key = e.key_mean; a.pair_w = e.pair_w;
  const uint64_t n_segs = (e.n_pairs + mllt_seg_pairs() - 1) / mllt_seg_pairs();
  const size_t seg_doubles = (size_t)a.shape.rows * a.shape.cols;
  const uint64_t per_round = std::min<uint64_t>(n_segs, m->mllt_budget / (sizeof(double) * seg_doubles));
  if (n_segs > 0xFFFFFFFFull || per_round == 0) return fail(SR_EINTERNAL, "MLLT statistics: %llu segments", (unsigned long long)n_segs);
  HIP_TRY(c->fm_partial.ensure((size_t)per_round * seg_doubles));
  HIP_TRY(c->fm_beta.ensure(1)); HIP_TRY(c->fm_G.ensure(nG));
  a.partial = c->fm_partial.p; a.out_beta = c->fm_beta.p; a.out_G = c->fm_G.p;
  EventPair ep{};
  if ((rc = prof_begin(m, m->s_gmm, 1, &ep))) return rc;
  for (uint64_t s0 = 0; s0 < n_segs; s0 += per_round) {
    a.seg0 = (uint32_t)s0; a.n_segs = (uint32_t)std::min<uint64_t>(per_round, n_segs - s0);
    HIP_TRY(launch_mllt_round(a, m->s_gmm));
  }
  if ((rc = prof_end(m, m->s_gmm, &ep))) return rc;
  HIP_TRY(hipStreamSynchronize(m->s_gmm));
  HIP_TRY(hipMemcpy(out_beta, c->fm_beta.p, sizeof(double), hipMemcpyDeviceToHost));
  HIP_TRY(hipMemcpy(out_G, c->fm_G.p, sizeof(double) * nG, hipMemcpyDeviceToHost));
  if (m->profiling) {  // per pair: key, weight, frame, density; a feature row, a mean row and a variance row; the partials out and in
    m->prof.frames += c->n_frames;
    m->prof.search_bytes += (double)e.n_pairs * (20.0 + 20.0 * D) + 16.0 * (double)n_segs * seg_doubles;
  }
  return SR_OK;
}

int sr_mllt_statistics_corpus(sr_model* m, sr_corpus* c, const uint16_t* states, int max_approx, double* out_beta, double* out_G) {
  return guarded(__func__, [&]() -> int {
  int rc = mllt_check(m, c, out_beta, out_G);
  if (rc) return rc;
  EmArgs e{};
  if ((rc = adapt_pairs(m, c, states, max_approx, &e))) return rc;
  return mllt_statistics(m, c, e, out_beta, out_G);
  });
}

int sr_mllt_statistics_bw_corpus(sr_model* m, sr_corpus* c, const uint16_t* automata, const uint64_t* aut_off, const double tdp[3],
                                 uint16_t silence_state, int gmm_kernel, double posterior_floor, int max_approx, double* out_cost,
                                 double* out_beta, double* out_G) {
  return guarded(__func__, [&]() -> int {
  int rc = mllt_check(m, c, out_beta, out_G);
  if (rc) return rc;
  EmArgs e{};
  if ((rc = adapt_pairs_bw(m, c, automata, aut_off, tdp, silence_state, gmm_kernel, posterior_floor, max_approx, out_cost, &e))) return rc;
  return mllt_statistics(m, c, e, out_beta, out_G);
  });
}

// ---- LDA with frame splicing (lda_stats.hip; the estimate itself is host code, lda.cpp) ---------------------------------------------
// [a, b) of every frame's utterance, for the clamping of the spliced vector
static int lda_upload_spans(sr_corpus* c) {
  std::vector<uint32_t> span(2 * (size_t)c->n_frames);
  for (uint32_t u = 0; u < c->n_utts; u++)
    for (uint64_t f = c->frame_off[u]; f < c->frame_off[u + 1]; f++) { span[2 * f] = (uint32_t)c->frame_off[u]; span[2 * f + 1] = (uint32_t)c->frame_off[u + 1]; }
  HIP_TRY(c->lda_span.upload(span.data(), span.size()));
  return SR_OK;
}

int sr_lda_statistics_corpus(sr_model* m, sr_corpus* c, const uint16_t* states, uint32_t context, const uint32_t* class_of_state,
                             uint32_t n_classes, double* out_count, double* out_sum, double* out_scatter) {
  return guarded(__func__, [&]() -> int {
  int rc = check_corpus(m, c);
  if (rc) return rc;
  if (!out_count || !out_sum || !out_scatter) return fail(SR_EINVAL, "null output");
  if (n_classes == 0) return fail(SR_EINVAL, "n_classes is 0");
  const uint32_t D = m->dim;
  const uint64_t F = c->n_frames, E64 = (2 * (uint64_t)context + 1) * D;
  if (E64 > lda_max_e()) return fail(SR_ELIMIT, "spliced dimension (2 x %u + 1) x %u exceeds %u (LDA statistics)", context, D, lda_max_e());
  const uint32_t E = (uint32_t)E64;
  if (F >= 0xFFFFFFFFull) return fail(SR_ELIMIT, "%llu frames do not fit the 32-bit frame lists", (unsigned long long)F);
  if (F && !states) return fail(SR_EINVAL, "states is null");
  size_t free_b = 0, total_b = 0;
  HIP_TRY(hipMemGetInfo(&free_b, &total_b));
  const double out_bytes = 8.0 * ((double)n_classes * E + (double)E * E);
  if (out_bytes > (double)free_b / 4)
    return fail(SR_ELIMIT, "the statistics of %u classes (%.0f bytes) exceed a quarter of the free device memory (%llu bytes)", n_classes,
                out_bytes, (unsigned long long)free_b);
  if ((uint64_t)n_classes * ((E + 255) / 256) > 0x7FFFFFFFull)  // lda_class_reduce_kernel's grid
    return fail(SR_ELIMIT, "%u classes x %u columns exceed the class sums' launch grid", n_classes, E);
  if (class_of_state)
    for (uint32_t s = 0; s < m->n_states; s++)
      if (class_of_state[s] >= n_classes && class_of_state[s] != SR_LDA_SKIP)
        return fail(SR_EINVAL, "state %u: class %u is neither < n_classes %u nor SR_LDA_SKIP", s, class_of_state[s], n_classes);
  std::vector<uint32_t> bounds((size_t)n_classes + 1, 0), items;
  items.reserve(F);
  for (uint64_t t = 0; t < F; t++) {
    if (states[t] >= m->n_states) return fail(SR_EINVAL, "frame %llu: state %u >= n_states %u", (unsigned long long)t, states[t], m->n_states);
    const uint32_t k = class_of_state ? class_of_state[states[t]] : states[t];
    if (k == SR_LDA_SKIP) continue;
    if (k >= n_classes) return fail(SR_EINVAL, "frame %llu: class %u >= n_classes %u", (unsigned long long)t, k, n_classes);
    bounds[k + 1]++;
    items.push_back((uint32_t)t);
  }
  const size_t seg_doubles = (size_t)lda_pairs(E) * lda_block() * lda_block();
  // ---- the checks are done: the outputs are written from here on
  const uint64_t n_items = items.size();
  for (uint32_t k = 0; k < n_classes; k++) out_count[k] = (double)bounds[k + 1];
  if (n_items == 0) {  // no frame, or none kept
    std::fill(out_sum, out_sum + (size_t)n_classes * E, 0.0);
    std::fill(out_scatter, out_scatter + (size_t)E * E, 0.0);
    return SR_OK;
  }
  // the kept frames grouped stably by class, every class cut into segments
  for (uint32_t k = 0; k < n_classes; k++) bounds[k + 1] += bounds[k];
  std::vector<uint32_t> class_items(n_items);
  {
    std::vector<uint32_t> fill(bounds.begin(), bounds.end() - 1);
    for (uint32_t t : items) class_items[fill[class_of_state ? class_of_state[states[t]] : states[t]]++] = t;
  }
  const srplan::Segments seg(bounds.data(), n_classes, lda_seg_items());
  if ((rc = srhost::corpus_ready(c, 0, F, m->s_gmm))) return rc;  // an asynchronous upload of c: wait for all of it
  if ((rc = lda_upload_spans(c))) return rc;
  LdaArgs a{};
  a.feats = c->feats.p; a.frame_span = c->lda_span.p; a.dim = D; a.context = context; a.E = E;
  {
    std::vector<uint32_t> triples(3 * (size_t)n_items);  // (frame, first and end frame of its utterance)
    uint32_t u = 0;
    for (size_t i = 0; i < n_items; i++) {
      while (c->frame_off[u + 1] <= items[i]) u++;
      triples[3 * i] = items[i]; triples[3 * i + 1] = (uint32_t)c->frame_off[u]; triples[3 * i + 2] = (uint32_t)c->frame_off[u + 1];
    }
    HIP_TRY(c->lda_items.upload(triples.data(), triples.size()));
  }
  HIP_TRY(c->lda_class_items.upload(class_items.data(), n_items));
  HIP_TRY(c->lda_cseg_begin.upload(seg.begin.data(), seg.begin.size())); HIP_TRY(c->lda_cseg_len.upload(seg.len.data(), seg.len.size()));
  HIP_TRY(c->lda_class_seg_off.upload(seg.off.data(), seg.off.size()));
  a.items = c->lda_items.p; a.n_items = n_items; a.class_items = c->lda_class_items.p;
  a.cseg_begin = c->lda_cseg_begin.p; a.cseg_len = c->lda_cseg_len.p; a.class_seg_off = c->lda_class_seg_off.p;
  a.n_csegs = (uint32_t)seg.begin.size(); a.n_classes = n_classes;
  const uint64_t n_segs = (n_items + lda_seg_items() - 1) / lda_seg_items();
  // (at least one segment a round: at most 36 blocks of 32 KiB, whatever SRGPU_LDA_MB says)
  const uint64_t per_round = std::min<uint64_t>(n_segs, std::max<uint64_t>(1, m->lda_budget / (sizeof(double) * seg_doubles)));
  HIP_TRY(c->fm_partial.ensure((size_t)per_round * seg_doubles));
  HIP_TRY(c->lda_cpartial.ensure((size_t)a.n_csegs * E));
  HIP_TRY(c->lda_sum.ensure((size_t)n_classes * E)); HIP_TRY(c->lda_scatter.ensure((size_t)E * E));
  a.partial = c->fm_partial.p; a.cpartial = c->lda_cpartial.p; a.out_sum = c->lda_sum.p; a.out_scatter = c->lda_scatter.p;
  EventPair ep{};
  if ((rc = prof_begin(m, m->s_gmm, 1, &ep))) return rc;
  HIP_TRY(launch_lda_class_sums(a, m->s_gmm));
  for (uint64_t s0 = 0; s0 < n_segs; s0 += per_round) {
    a.seg0 = (uint32_t)s0; a.n_segs = (uint32_t)std::min<uint64_t>(per_round, n_segs - s0);
    HIP_TRY(launch_lda_round(a, m->s_gmm));
  }
  if ((rc = prof_end(m, m->s_gmm, &ep))) return rc;
  HIP_TRY(hipStreamSynchronize(m->s_gmm));
  HIP_TRY(hipMemcpy(out_sum, c->lda_sum.p, sizeof(double) * n_classes * E, hipMemcpyDeviceToHost));
  HIP_TRY(hipMemcpy(out_scatter, c->lda_scatter.p, sizeof(double) * E * E, hipMemcpyDeviceToHost));
  if (m->profiling) {  // per kept frame: its spliced row for the class sums and once per panel pair's side; the partials out and in
    m->prof.frames += F;
    m->prof.search_bytes += (double)n_items * 4.0 * E * (1.0 + lda_panels(E)) + 16.0 * (double)n_segs * seg_doubles;
  }
  return SR_OK;
  });
}

int sr_corpus_splice_transform(sr_model* m, sr_corpus* c, sr_model* target, uint32_t context, const double* M, sr_corpus** out) {
  return guarded(__func__, [&]() -> int {
  if (!out) return fail(SR_EINVAL, "out is null");
  *out = nullptr;
  int rc = check_corpus(m, c);
  if (rc) return rc;
  if (!target) return fail(SR_EINVAL, "target is null");
  if (!M) return fail(SR_EINVAL, "M is null");
  if (target->device != m->device) return fail(SR_EINVAL, "the target model is on device %d, the corpus on device %d", target->device, m->device);
  const uint32_t D = m->dim, p = target->dim;
  const uint64_t F = c->n_frames, E64 = (2 * (uint64_t)context + 1) * D;
  if (E64 > lda_max_e()) return fail(SR_ELIMIT, "spliced dimension (2 x %u + 1) x %u exceeds %u (splice transform)", context, D, lda_max_e());
  if (F >= 0xFFFFFFFFull) return fail(SR_ELIMIT, "%llu frames do not fit the 32-bit frame lists", (unsigned long long)F);
  const uint32_t E = (uint32_t)E64;
  if ((rc = srhost::corpus_ready(c, 0, F, m->s_gmm))) return rc;  // an asynchronous upload of c: wait for all of it
  if ((rc = lda_upload_spans(c))) return rc;
  sr_corpus* t = new sr_corpus();
  std::unique_ptr<sr_corpus, int (*)(sr_corpus*)> own(t, sr_corpus_destroy);
  t->model = target; t->n_utts = c->n_utts; t->n_frames = F;
  srhost::corpus_register(t);
  t->frame_off = c->frame_off;
  HIP_TRY(t->feats.ensure((size_t)F * p + 64));
  HIP_TRY(t->d_frame_off.upload(t->frame_off.data(), t->frame_off.size()));
  DevBuf<double> d_M;
  HIP_TRY(d_M.upload(M, (size_t)p * (E + 1)));
  EventPair ep{};
  if ((rc = prof_begin(m, m->s_gmm, 1, &ep))) return rc;
  HIP_TRY(launch_lda_project(c->feats.p, c->lda_span.p, F, D, context, d_M.p, p, t->feats.p, m->s_gmm));
  if ((rc = prof_end(m, m->s_gmm, &ep))) return rc;
  HIP_TRY(hipStreamSynchronize(m->s_gmm));
  if (m->profiling) {  // a row in, a row out
    m->prof.frames += F;
    m->prof.search_bytes += 4.0 * (double)F * (D + p);
  }
  *out = own.release();
  return SR_OK;
  });
}

// ---- forward-backward over the recognition network (viterbi_netfb.hip) ----------------------------------------------------
// 8 B per (frame, position)
static std::vector<uint64_t> netfb_cost(const sr_corpus* c, const sr_lexicon* l) {
  return srplan::linear_cost(c->frame_off.data(), c->n_utts, 8ull * l->net.n_slots);
}

static int netfb_check(sr_model* m, sr_corpus* c, sr_lexicon* l, const sr_search_params* p, double scale, double posterior_floor) {
  int rc = check_corpus(m, c);
  if (rc) return rc;
  if (!l || l->model != m) return fail(SR_EINVAL, "lexicon does not belong to this model");
  if (!p) return fail(SR_EINVAL, "null argument");
  if (p->flags != 0) return fail(SR_EINVAL, "sr_search_params.flags must be 0 (got 0x%x)", (unsigned)p->flags);
  if (!(scale > 0.0) || !std::isfinite(scale)) return fail(SR_EINVAL, "scale must be finite and > 0 (got %g)", scale);
  if (!(posterior_floor >= 0.0)) return fail(SR_EINVAL, "posterior_floor must be >= 0 (got %g)", posterior_floor);
  const uint64_t P = l->net.n_slots;
  if (P > netfb_max_slots())
    return fail(SR_ELIMIT, "%llu lexicon positions exceed the network forward-backward's %llu", (unsigned long long)P,
                (unsigned long long)netfb_max_slots());
  return check_fits(m, netfb_cost(c, l));
}

// The launch groups of a pass -- consecutive utterances of a chunk whose trellises (8 B per frame and position) fit m->fb_budget
// together (netfb_check: every utterance fits alone) -- and their workspace.  run() enqueues a chunk's groups in order: forward,
// backward, word posteriors, then per_group(args, frames of the group).
struct NetFbPass {
  srplan::Groups groups;
  NetFbArgs a{};
  size_t ci = 0;  // run_chunks searches the chunks in order

  int setup(sr_model* m, sr_corpus* c, sr_lexicon* l, const sr_search_params* p, double scale, const std::vector<Chunk>& chunks) {
    const uint64_t P = l->net.n_slots;
    groups = srplan::launch_groups(chunks, netfb_cost(c, l).data(), m->fb_budget);
    const uint64_t max_gf = std::max<uint64_t>(1, groups.max_span(c->frame_off.data()));
    HIP_TRY(c->fb_trellis.ensure(max_gf * P));
    HIP_TRY(c->nf_post.ensure(max_gf * l->net.n_words));
    HIP_TRY(c->out_cost.ensure(c->n_utts));
    a.net = l->net; a.ld = m->ld; a.frame_off = c->d_frame_off.p;
    a.scale = scale; a.word_penalty = p->word_penalty;
    a.trellis = c->fb_trellis.p; a.out_cost = c->out_cost.p; a.post = c->nf_post.p;
    // trellis traffic per (frame, position): alpha out, alpha in + gamma out, gamma in (word posteriors)
    if (m->profiling) m->prof.search_bytes += 32.0 * (double)P * (double)c->n_frames;
    return SR_OK;
  }
  template <class PerGroup>
  int run(sr_corpus* c, const Chunk& ch, const double* table, hipStream_t s, PerGroup per_group) {
    for (const Group& g : groups.of_chunk[ci]) {
      a.scores = table; a.frame_base = ch.f0; a.utt_first = g.u0; a.n_utts = g.u1 - g.u0; a.group_f0 = c->frame_off[g.u0];
      const uint64_t n = c->frame_off[g.u1] - c->frame_off[g.u0];
      HIP_TRY(launch_netfb_forward(a, s));
      HIP_TRY(launch_netfb_backward(a, s));
      HIP_TRY(launch_netfb_words(a, n, s));
      int rc = per_group(a, n);
      if (rc) return rc;
    }
    ci++;
    return SR_OK;
  }
};

// kappa F_u on the device -> F_u
static int netfb_costs(sr_corpus* c, double scale, double* out_cost) {
  const uint32_t U = c->n_utts;
  if (U) HIP_TRY(hipMemcpy(out_cost, c->out_cost.p, sizeof(double) * U, hipMemcpyDeviceToHost));
  for (uint32_t u = 0; u < U; u++) out_cost[u] /= scale;
  return SR_OK;
}

// sr_word_posteriors_corpus and its test hook: the checks, the pass on `score`'s scores, F_u and the top words to the host
template <class Score>
static int word_posteriors(sr_model* m, sr_corpus* c, sr_lexicon* l, const sr_search_params* p, double scale, double posterior_floor,
                           uint32_t max_items, Score score, double* out_cost, uint16_t* out_count, uint32_t* out_word,
                           double* out_weight) {
  int rc = netfb_check(m, c, l, p, scale, posterior_floor);
  if (rc) return rc;
  if (!out_cost) return fail(SR_EINVAL, "null argument");
  bool post = false;
  if ((rc = top_items_arguments(out_count, out_word, out_weight, "out_word", max_items, &post))) return rc;
  const uint64_t F = c->n_frames;
  std::vector<Chunk> chunks;
  if ((rc = prepare_chunks(m, c, &chunks))) return rc;
  NetFbPass fp;
  if ((rc = fp.setup(m, c, l, p, scale, chunks))) return rc;
  if (post && (rc = ensure_top_items(F, max_items, c->nf_count, c->nf_word, c->nf_weight))) return rc;
  rc = run_chunks(m, chunks, [&](const Chunk& ch, double* table) -> int { return score(ch, table); },
      [&](const Chunk& ch, const double* table, hipStream_t s) -> int {
        return fp.run(c, ch, table, s, [&](const NetFbArgs& a, uint64_t n) -> int {
          if (post) HIP_TRY(launch_netfb_top(a, n, max_items, posterior_floor, c->nf_count.p, c->nf_word.p, c->nf_weight.p, s));
          return SR_OK;
        });
      });
  if (rc) return rc;
  if (m->profiling) m->prof.frames += F;
  if ((rc = netfb_costs(c, scale, out_cost))) return rc;
  if (!post || F == 0) return SR_OK;
  return copy_top_items(F, max_items, c->nf_count, c->nf_word, c->nf_weight, out_count, out_word, out_weight);
}

int sr_word_posteriors_corpus(sr_model* m, sr_corpus* c, sr_lexicon* l, const sr_search_params* p, double scale, double posterior_floor,
                              uint32_t max_items, double* out_cost, uint16_t* out_count, uint32_t* out_word, double* out_weight) {
  return guarded(__func__, [&]() -> int {
  if (!p) return fail(SR_EINVAL, "null argument");
  return word_posteriors(m, c, l, p, scale, posterior_floor, max_items, gmm_scores(m, c, p->gmm_kernel), out_cost, out_count, out_word,
                         out_weight);
  });
}

// test hook: sr_word_posteriors_corpus with the chunk's score step replaced by a copy of the caller's rows (p->gmm_kernel is not read)
int sr_word_posteriors_corpus_scores(sr_model* m, sr_corpus* c, sr_lexicon* l, const sr_search_params* p, double scale,
                                     double posterior_floor, uint32_t max_items, const double* scores, uint64_t n_scores, double* out_cost,
                                     uint16_t* out_count, uint32_t* out_word, double* out_weight) {
  return guarded(__func__, [&]() -> int {
  int rc = check_corpus(m, c);
  if (rc) return rc;
  ScoreTable table;
  if ((rc = table.set(m, c, scores, n_scores))) return rc;
  return table.done(word_posteriors(m, c, l, p, scale, posterior_floor, max_items, std::cref(table), out_cost, out_count, out_word,
                                    out_weight));
  });
}

int sr_recognize_confidence_corpus(sr_model* m, sr_corpus* c, sr_lexicon* l, const sr_search_params* p, double scale,
                                   uint32_t* out_words, uint64_t* out_word_off, double* out_conf, uint32_t* out_first,
                                   uint32_t* out_last) {
  return guarded(__func__, [&]() -> int {
  int rc = netfb_check(m, c, l, p, scale, 0.0);
  if (rc) return rc;
  const uint64_t F = c->n_frames;
  if (!out_word_off || (F && (!out_words || !out_conf || !out_first || !out_last))) return fail(SR_EINVAL, "null argument");
  std::vector<Chunk> chunks;
  if ((rc = prepare_chunks(m, c, &chunks))) return rc;
  NetFbPass fp;
  if ((rc = fp.setup(m, c, l, p, scale, chunks))) return rc;
  HIP_TRY(c->nf_conf.ensure(F));
  HIP_TRY(c->nf_first.ensure(F));
  HIP_TRY(c->nf_last.ensure(F));
  rc = recognize_pass(m, c, l, p, chunks, [&](const Chunk& ch, const double* table, hipStream_t s) -> int {
    return fp.run(c, ch, table, s, [&](const NetFbArgs& a, uint64_t) -> int {
      HIP_TRY(launch_netfb_conf(a, c->tb_word.p, c->tb_bkp.p, c->out_count.p, c->nf_conf.p, c->nf_first.p, c->nf_last.p, s));
      return SR_OK;
    });
  });
  if (rc) return rc;
  if ((rc = gather_words(c, out_words, out_word_off))) return rc;
  // the device holds word k of utterance u at frame_off[u] + k, like out_words
  std::vector<double> conf(F);
  std::vector<uint32_t> first(F), last(F);
  if (F) {
    HIP_TRY(hipMemcpy(conf.data(), c->nf_conf.p, sizeof(double) * F, hipMemcpyDeviceToHost));
    HIP_TRY(hipMemcpy(first.data(), c->nf_first.p, sizeof(uint32_t) * F, hipMemcpyDeviceToHost));
    HIP_TRY(hipMemcpy(last.data(), c->nf_last.p, sizeof(uint32_t) * F, hipMemcpyDeviceToHost));
  }
  for (uint32_t u = 0; u < c->n_utts; u++)
    for (uint64_t i = out_word_off[u]; i < out_word_off[u + 1]; i++) {
      const uint64_t d = c->frame_off[u] + (i - out_word_off[u]);
      out_conf[i] = conf[d]; out_first[i] = first[d]; out_last[i] = last[d];
    }
  return SR_OK;
  });
}

// ---- forward-backward over the bigram search network (viterbi_bigram_fb.hip) -----------------------------------------------------
// bytes of one group's workspace beside the trellis, per utterance: vec, prod, wend (Kp each), the two x rows, m
static uint64_t bgfb_utt_bytes(const sr_bigram* b) { return 24ull * bgfb_padded(b->net.n_words) + 16ull * b->net.n_positions + 8; }
// 8 B per (frame, position) and the vectors
static std::vector<uint64_t> bgfb_cost(const sr_corpus* c, const sr_bigram* b) {
  return srplan::linear_cost(c->frame_off.data(), c->n_utts, 8ull * b->net.n_positions, bgfb_utt_bytes(b));
}

static int bgfb_check(sr_model* m, sr_corpus* c, sr_bigram* b, double scale, double posterior_floor) {
  int rc = check_corpus(m, c);
  if (rc) return rc;
  if (!b || b->model != m) return fail(SR_EINVAL, "bigram search net does not belong to this model");
  if (!(scale > 0.0) || !std::isfinite(scale)) return fail(SR_EINVAL, "scale must be finite and > 0 (got %g)", scale);
  if (!(posterior_floor >= 0.0)) return fail(SR_EINVAL, "posterior_floor must be >= 0 (got %g)", posterior_floor);
  if (b->lm_min == -std::numeric_limits<float>::infinity()) return fail(SR_EINVAL, "the language model has a score of -inf");
  if (-scale * (double)b->lm_min > 700.0)
    return fail(SR_ELIMIT, "scale %g x LM score %g: exp(%g) is not representable", scale, (double)b->lm_min, -scale * (double)b->lm_min);
  return check_fits(m, bgfb_cost(c, b));
}

// exp(-kappa lm) and its transpose in b->fb_lk / b->fb_lkT: built once per (net, kappa)
static int bgfb_tables(sr_model* m, sr_bigram* b, double scale) {
  if (b->fb_kappa == scale && b->fb_lk.p) return SR_OK;
  const uint32_t W = b->net.n_words, Kp = bgfb_padded(W);
  b->fb_kappa = 0.0;
  HIP_TRY(b->fb_lk.ensure((size_t)Kp * Kp));
  HIP_TRY(b->fb_lkT.ensure((size_t)Kp * Kp));
  HIP_TRY(launch_bgfb_table(b->lmT.p, W, Kp, b->net.silence, scale, b->fb_lk.p, b->fb_lkT.p, m->s_search));
  HIP_TRY(hipStreamSynchronize(m->s_search));
  b->fb_kappa = scale;
  return SR_OK;
}

// The search net's fields of a BgFbArgs or a BgLatArgs (both name them alike), with the model's row length and the corpus' offsets
template <class Args>
static void bg_net_args(const sr_model* m, const sr_corpus* c, const sr_bigram* b, Args* a) {
  a->n_words = b->net.n_words; a->silence = b->net.silence; a->n_positions = (uint32_t)b->net.n_positions;
  a->Kp = bgfb_padded(b->net.n_words);
  a->slot_off = b->slot_off.p; a->pos_info = b->pos_info.p; a->pos_slot = b->pos_slot.p; a->lmT = b->lmT.p;
  memcpy(a->tdp, b->net.tdp, sizeof(a->tdp));
  a->ld = m->ld; a->frame_off = c->d_frame_off.p;
}

// The time-step recursion over the bigram search network with `mult` operand vectors per utterance (1: BgFbPass; 2: BgSmbrPass, the
// accuracy side beside every cost).  The launch groups are cut like NetFbPass' on a cost prefix that counts the per-utterance vectors
// in, each with its utterances ordered longest first.  run_groups() enqueues a chunk's groups: per frame the step and the product,
// forward then backward, then after(group).
struct BgStepPass {
  srplan::Groups groups;
  srplan::StepOrder steps;                 // each group's range, longest first
  const double *lk = nullptr, *lkT = nullptr;
  const uint32_t* d_order = nullptr;       // `order` on the device
  uint64_t max_gf = 1;                     // frames of the largest group
  uint32_t mult = 1;
  size_t ci = 0;  // run_chunks searches the chunks in order

  // plans the groups on `cost`, sizes and clears the workspace, and fills `a` with everything but the launch's own fields and `post`
  int workspace(sr_model* m, sr_corpus* c, sr_bigram* b, double scale, uint32_t mult_, const std::vector<uint64_t>& cost,
                const std::vector<Chunk>& chunks, BgFbArgs* a) {
    const uint64_t P = b->net.n_positions;
    const uint32_t W = b->net.n_words, Kp = bgfb_padded(W), U = c->n_utts;
    mult = mult_;
    groups = srplan::launch_groups(chunks, cost.data(), m->fb_budget);
    steps = srplan::StepOrder(groups, c->frame_off.data(), U);
    max_gf = std::max<uint64_t>(1, groups.max_span(c->frame_off.data()));
    const uint32_t max_gu = std::max(1u, groups.max_utts());
    int rc = bgfb_tables(m, b, scale);
    if (rc) return rc;
    lk = b->fb_lk.p; lkT = b->fb_lkT.p;
    const size_t rows = ((size_t)mult * max_gu + 63) & ~(size_t)63;  // the product reads whole 16-column tiles of vec
    HIP_TRY(c->fb_trellis.ensure(max_gf * mult * P));
    HIP_TRY(c->out_cost.ensure(U));
    HIP_TRY(c->bgfb_vec.ensure(rows * Kp));
    HIP_TRY(c->bgfb_prod.ensure(rows * Kp));
    HIP_TRY(c->bgfb_wend.ensure(rows * Kp));
    HIP_TRY(c->bgfb_m.ensure(rows));
    HIP_TRY(c->bgfb_xb.ensure(2 * (size_t)mult * max_gu * P));
    HIP_TRY(c->bgfb_order.upload(steps.order.data(), steps.order.size()));
    d_order = c->bgfb_order.p;
    HIP_TRY(hipMemset(c->bgfb_vec.p, 0, rows * Kp * sizeof(double)));  // (the padding columns h >= W stay 0 from here on)
    if (U) HIP_TRY(hipMemset(c->out_cost.p, 0, sizeof(double) * U));  // T_u = 0: F_u = 0, the start hypothesis is a word end
    HIP_TRY(hipDeviceSynchronize());
    bg_net_args(m, c, b, a);
    a->scale = scale;
    a->trellis = c->fb_trellis.p; a->vec = c->bgfb_vec.p; a->prod = c->bgfb_prod.p; a->wend = c->bgfb_wend.p; a->m = c->bgfb_m.p; a->xb = c->bgfb_xb.p;
    a->out_cost = c->out_cost.p;
    return SR_OK;
  }
  // forward() and backward() launch frame a->t of the first a->n_alive utterances from the arguments `a` is part of
  template <class Forward, class Backward, class After>
  int run_groups(sr_corpus* c, const Chunk& ch, const double* table, hipStream_t s, BgFbArgs* a, Forward forward, Backward backward,
                 After after) {
    for (const Group& g : groups.of_chunk[ci]) {
      a->scores = table; a->frame_base = ch.f0; a->group_f0 = c->frame_off[g.u0];
      a->order = d_order + g.u0; a->n_group = g.u1 - g.u0;
      const uint32_t t_max = steps.t_max(g);
      for (uint32_t t = 0; t < t_max; t++) {
        a->t = t; a->n_alive = steps.alive(g, t);
        HIP_TRY(forward());
        const uint32_t next = steps.alive(g, t + 1);  // only those that go on need their entries
        HIP_TRY(launch_bgfb_product(lk, a->vec, a->prod, a->Kp, mult * next, s));
      }
      for (uint32_t t = t_max; t-- > 0;) {
        a->t = t; a->n_alive = steps.alive(g, t);
        HIP_TRY(backward());
        if (t) HIP_TRY(launch_bgfb_product(lkT, a->vec, a->prod, a->Kp, mult * a->n_alive, s));
      }
      int rc = after(g);
      if (rc) return rc;
    }
    ci++;
    return SR_OK;
  }
};

// BgStepPass at multiplicity 1 with the word posteriors: run() enqueues a chunk's groups, after each recursion the word posteriors
// (want_words) and per_group(args, frames of the group).
struct BgFbPass : BgStepPass {
  BgFbArgs a{};
  bool want_words = true;  // the word posteriors of every group (the MMI passes read gamma itself)

  int setup(sr_model* m, sr_corpus* c, sr_bigram* b, double scale, const std::vector<Chunk>& chunks) {
    int rc = workspace(m, c, b, scale, 1, bgfb_cost(c, b), chunks, &a);
    if (rc) return rc;
    HIP_TRY(c->nf_post.ensure(max_gf * b->net.n_words));
    a.post = c->nf_post.p;
    // trellis traffic per (frame, position) as NetFbPass; the product reads the table once per frame step and direction
    if (m->profiling) m->prof.search_bytes += 32.0 * (double)b->net.n_positions * (double)c->n_frames;
    return SR_OK;
  }
  template <class PerGroup>
  int run(sr_corpus* c, const Chunk& ch, const double* table, hipStream_t s, PerGroup per_group) {
    return run_groups(c, ch, table, s, &a, [&] { return launch_bgfb_forward(a, s); }, [&] { return launch_bgfb_backward(a, s); },
                      [&](const Group& g) -> int {
                        const uint64_t n = c->frame_off[g.u1] - c->frame_off[g.u0];
                        if (want_words) HIP_TRY(launch_bgfb_words(a, n, s));
                        return per_group(a, n);
                      });
  }
};

// the top items of a group's frames through netfb_top_kernel (it reads the word count, the posteriors and the group's first frame)
static int bgfb_top(const BgFbArgs& a, uint64_t n, uint32_t max_items, double floor, sr_corpus* c, hipStream_t s) {
  NetFbArgs t{};
  t.net.n_words = a.n_words; t.post = a.post; t.group_f0 = a.group_f0;
  HIP_TRY(launch_netfb_top(t, n, max_items, floor, c->nf_count.p, c->nf_word.p, c->nf_weight.p, s));
  return SR_OK;
}

// sr_bigram_word_posteriors_corpus and its test hook: the pass on `score`'s scores once bgfb_check has passed, F_u and the top words
// to the host
template <class Score>
static int bigram_word_posteriors(sr_model* m, sr_corpus* c, sr_bigram* b, double scale, double posterior_floor, uint32_t max_items,
                                  Score score, double* out_cost, uint16_t* out_count, uint32_t* out_word, double* out_weight) {
  int rc;
  if (!out_cost) return fail(SR_EINVAL, "null argument");
  bool post = false;
  if ((rc = top_items_arguments(out_count, out_word, out_weight, "out_word", max_items, &post))) return rc;
  const uint64_t F = c->n_frames;
  std::vector<Chunk> chunks;
  if ((rc = prepare_chunks(m, c, &chunks))) return rc;
  BgFbPass fp;
  if ((rc = fp.setup(m, c, b, scale, chunks))) return rc;
  if (post && (rc = ensure_top_items(F, max_items, c->nf_count, c->nf_word, c->nf_weight))) return rc;
  rc = run_chunks(m, chunks, [&](const Chunk& ch, double* table) -> int { return score(ch, table); },
      [&](const Chunk& ch, const double* table, hipStream_t s) -> int {
        return fp.run(c, ch, table, s, [&](const BgFbArgs& a, uint64_t n) -> int {
          return post ? bgfb_top(a, n, max_items, posterior_floor, c, s) : SR_OK;
        });
      });
  if (rc) return rc;
  if (m->profiling) m->prof.frames += F;
  if ((rc = netfb_costs(c, scale, out_cost))) return rc;
  if (!post || F == 0) return SR_OK;
  return copy_top_items(F, max_items, c->nf_count, c->nf_word, c->nf_weight, out_count, out_word, out_weight);
}

int sr_bigram_word_posteriors_corpus(sr_model* m, sr_corpus* c, sr_bigram* b, int gmm_kernel, double scale, double posterior_floor,
                                     uint32_t max_items, double* out_cost, uint16_t* out_count, uint32_t* out_word, double* out_weight) {
  return guarded(__func__, [&]() -> int {
  int rc = bgfb_check(m, c, b, scale, posterior_floor);
  if (rc) return rc;
  return bigram_word_posteriors(m, c, b, scale, posterior_floor, max_items, gmm_scores(m, c, gmm_kernel), out_cost, out_count, out_word,
                                out_weight);
  });
}

// test hook: sr_bigram_word_posteriors_corpus with the chunk's score step replaced by a copy of the caller's rows
int sr_bigram_word_posteriors_corpus_scores(sr_model* m, sr_corpus* c, sr_bigram* b, double scale, double posterior_floor,
                                            uint32_t max_items, const double* scores, uint64_t n_scores, double* out_cost,
                                            uint16_t* out_count, uint32_t* out_word, double* out_weight) {
  return guarded(__func__, [&]() -> int {
  int rc = bgfb_check(m, c, b, scale, posterior_floor);
  if (rc) return rc;
  ScoreTable table;
  if ((rc = table.set(m, c, scores, n_scores)) || (rc = table.refuse_neg_inf(scores, n_scores))) return rc;
  return table.done(bigram_word_posteriors(m, c, b, scale, posterior_floor, max_items, std::cref(table), out_cost, out_count, out_word,
                                           out_weight));
  });
}

int sr_recognize_bigram_confidence_corpus(sr_model* m, sr_corpus* c, sr_bigram* b, const sr_bigram_params* p, double scale,
                                          uint32_t* out_word, float* out_score, uint32_t* out_time, uint64_t* out_off, double* out_conf) {
  return guarded(__func__, [&]() -> int {
  int rc = bgfb_check(m, c, b, scale, 0.0);
  if (rc) return rc;
  if (!out_conf && c->n_frames) return fail(SR_EINVAL, "null argument");
  const uint64_t F = c->n_frames;
  const uint32_t U = c->n_utts;
  BgFbPass fp;
  rc = bigram_recognize_pass(m, c, b, p, out_word, out_score, out_time, out_off,
      [&](const std::vector<Chunk>& chunks) -> int {
        int r = fp.setup(m, c, b, scale, chunks);
        if (r) return r;
        HIP_TRY(c->bgfb_conf.ensure(F + U));
        return SR_OK;
      },
      [&](const Chunk& ch, const double* table, hipStream_t s) -> int {
        return fp.run(c, ch, table, s, [&](const BgFbArgs& a, uint64_t) -> int {
          HIP_TRY(launch_bgfb_conf(a, a.n_group, b->out_word.p, b->out_time.p, b->out_count.p, c->bgfb_conf.p, s));
          return SR_OK;
        });
      });
  if (rc) return rc;
  // the device holds item i of utterance u at frame_off[u] + u + i, like the search's items
  std::vector<double> conf(F + U);
  if (U) HIP_TRY(hipMemcpy(conf.data(), c->bgfb_conf.p, sizeof(double) * (F + U), hipMemcpyDeviceToHost));
  for (uint32_t u = 0; u < U; u++)
    for (uint64_t i = out_off[u]; i < out_off[u + 1]; i++) out_conf[i] = conf[c->frame_off[u] + u + (i - out_off[u])];
  return SR_OK;
  });
}

// ---- MMI training over the recognition network (viterbi_mmi.hip) -----------------------------------------------------------------
// The transcripts' chains of this network and of the bigram search network: chain_host::build_chains and build_bgchains
#include "chains.cpp"
using chain_host::Chains;

// netfb_check plus the transcript's: *constrained = a transcript pair is given
static int occ_check(sr_model* m, sr_corpus* c, sr_lexicon* l, const sr_search_params* p, double scale, double posterior_floor,
                     const uint32_t* trans, const uint64_t* trans_off, bool* constrained) {
  int rc = netfb_check(m, c, l, p, scale, posterior_floor);
  if (rc) return rc;
  if ((trans_off == nullptr) != (trans == nullptr))
    return fail(SR_EINVAL, "partial transcript (pass trans and trans_off, or neither)");
  *constrained = trans_off != nullptr;
  if (!*constrained) return SR_OK;
  if (l->net.silence_word != 0) return fail(SR_EINVAL, "the transcript-constrained network needs the silence word to be word 0 (it is %u)", l->net.silence_word);
  if (trans_off[0] != 0) return fail(SR_EINVAL, "trans_off[0] must be 0");
  const uint64_t sil = l->h_word_off[1];
  for (uint32_t u = 0; u < c->n_utts; u++) {
    if (trans_off[u + 1] < trans_off[u]) return fail(SR_EINVAL, "trans_off must be non-decreasing (utterance %u)", u);
    const uint64_t n = trans_off[u + 1] - trans_off[u], T = c->frame_off[u + 1] - c->frame_off[u];
    if (n > netfb_max_slots()) return fail(SR_ELIMIT, "utterance %u: transcript of %llu words", u, (unsigned long long)n);
    uint64_t N = sil * (n + 1);
    for (uint64_t i = trans_off[u]; i < trans_off[u + 1]; i++) {
      const uint32_t w = trans[i];
      if (w >= l->net.n_words || w == 0)
        return fail(SR_EINVAL, "utterance %u: transcript word %u is not a lexicon word other than silence", u, w);
      N += l->h_word_off[w + 1] - l->h_word_off[w];
    }
    if (N > netfb_max_slots())
      return fail(SR_ELIMIT, "utterance %u: chain of %llu positions exceeds the network forward-backward's %llu", u, (unsigned long long)N,
                  (unsigned long long)netfb_max_slots());
    if ((rc = check_fits(m, u, 8 * N * T))) return rc;
  }
  return SR_OK;
}

// One occupancy pass over the corpus on the search's scoring chunks: the free network (trans_off null) or the transcripts' chains.
// Inside a chunk, consecutive utterances whose trellises fit m->fb_budget together (8 B per frame and position) run forward, backward and
// -- want_items -- the occupancy items.  Leaves kappa F_u in c->out_cost and, with want_items, *n_items items in c->fb_item_* (frame
// order, ascending mixture id) with c->fb_item_off[F + 1]; utterances whose gate (device, optional) is +inf give no items.
template <class Score>
static int occ_pass(sr_model* m, sr_corpus* c, sr_lexicon* l, const sr_search_params* p, double scale, double posterior_floor,
                    const uint32_t* trans, const uint64_t* trans_off, bool want_items, const double* gate, uint64_t* n_items,
                    Score score) {
  const uint32_t U = c->n_utts;
  const uint64_t F = c->n_frames, P = l->net.n_slots;
  const bool chain = trans_off != nullptr;
  *n_items = 0;
  HIP_TRY(c->out_cost.ensure(U));
  if (U == 0) return SR_OK;
  Chains ch;
  if (chain) chain_host::build_chains(l->h_word_off.data(), l->h_slot_info.data(), U, trans, trans_off, &ch);
  // the mixture lists: the distinct mixtures (ascending) of the lexicon, or of each chain, and the positions carrying each
  const srplan::OccPlan<uint16_t> pl(c->frame_off.data(), U, chain ? ch.off.data() : nullptr, chain ? ch.info.data() : l->h_slot_info.data(), P,
                                     true);
  if (want_items && pl.item_bound >= (1ull << 31)) return fail(SR_ELIMIT, "too many (frame, mixture) occupancies");
  std::vector<Chunk> chunks;
  int rc = prepare_chunks(m, c, &chunks);
  if (rc) return rc;
  srplan::Groups groups;
  if ((rc = trellis_groups(m, c, chunks, pl.tr_off, &groups))) return rc;
  const uint64_t max_gf = std::max<uint64_t>(1, groups.max_span(c->frame_off.data()));
  if (chain) {
    if ((rc = upload_chains(c, ch))) return rc;
  } else {
    HIP_TRY(c->nf_ends.ensure(max_gf));
  }
  size_t scan_bytes = 0;
  if (want_items && ((rc = upload_mix_lists(c, pl.ml, chain, c->fb_slot_pos)) || (rc = ensure_items(c, max_gf, F, pl.item_bound, &scan_bytes))))
    return rc;
  NetFbArgs na{};
  na.net = l->net; na.ld = m->ld; na.frame_off = c->d_frame_off.p; na.scale = scale; na.word_penalty = p->word_penalty;
  na.trellis = c->fb_trellis.p; na.out_cost = c->out_cost.p; na.ends = c->nf_ends.p;
  ChainArgs ca{};
  ca.ld = m->ld; ca.frame_off = c->d_frame_off.p; ca.scale = scale; ca.word_penalty = p->word_penalty;
  ca.tdp_loop = l->net.tdp_loop; ca.tdp_forward = l->net.tdp_forward; ca.tdp_skip = l->net.tdp_skip;
  ca.chain_off = c->mmi_chain_off.p; ca.info = c->mmi_info.p; ca.src = c->mmi_src.p; ca.dst = c->mmi_dst.p; ca.sil_len = ch.sil_len;
  ca.trellis = c->fb_trellis.p; ca.trellis_off = c->fb_trellis_off.p; ca.out_cost = c->out_cost.p;
  ItemArgs ia{};
  occ_item_fields(&ia, c, pl.ml, chain, P, c->fb_slot_pos, 0, gate, posterior_floor);
  size_t ci = 0;  // run_chunks searches the chunks in order
  rc = run_chunks(m, chunks, [&](const Chunk& k, double* table) -> int { return score(k, table); },
      [&](const Chunk& k, const double* table, hipStream_t s) -> int {
        if (want_items && ci == 0) HIP_TRY(reset_item_count(c->fb_base, s));
        for (const Group& g : groups.of_chunk[ci]) {
          if (chain) {
            ca.scores = table; ca.frame_base = k.f0; ca.utt_first = g.u0; ca.n_utts = g.u1 - g.u0;
            ca.max_positions = srplan::max_positions(g, ch.off.data());
            HIP_TRY(launch_chain_forward(ca, s));
            HIP_TRY(launch_chain_backward(ca, s));
          } else {
            na.scores = table; na.frame_base = k.f0; na.utt_first = g.u0; na.n_utts = g.u1 - g.u0; na.group_f0 = c->frame_off[g.u0];
            HIP_TRY(launch_netfb_forward(na, s));
            HIP_TRY(launch_netocc_backward(na, s));
          }
          if (want_items) {
            const uint64_t n = item_group(&ia, c, g.u0, g.u1);
            HIP_TRY(launch_items(ia, +1, n, c->fb_scan_temp.p, scan_bytes, c->fb_scan.p, s));
          }
        }
        ci++;
        return SR_OK;
      });
  if (rc) return rc;
  if (want_items && (rc = read_item_count(c->fb_base, n_items))) return rc;
  if (m->profiling) {  // trellis traffic per (frame, position) as the network pass counts it: alpha out, alpha in + part out, part in
    m->prof.frames += F;
    m->prof.search_bytes += 32.0 * (double)pl.tr_off[U];
  }
  return SR_OK;
}

// ... with the model's scores, as every production pass takes it
static int occ_pass(sr_model* m, sr_corpus* c, sr_lexicon* l, const sr_search_params* p, double scale, double posterior_floor,
                    const uint32_t* trans, const uint64_t* trans_off, bool want_items, const double* gate, uint64_t* n_items) {
  return occ_pass(m, c, l, p, scale, posterior_floor, trans, trans_off, want_items, gate, n_items, gmm_scores(m, c, p->gmm_kernel));
}

// Numerator and denominator statistics of MMI training, for sr_mmi_statistics_corpus and sr_bigram_mmi_statistics_corpus:
// pass(numerator, gate, &n_items) is the entry point's occupancy pass over the transcripts' chains (numerator) or the free network.
template <class Pass>
static int mmi_statistics(sr_model* m, sr_corpus* c, double scale, int max_approx, double* out_num_cost, double* out_den_cost,
                          double* num_mean_acc, double* num_mean_w, double* num_var_acc, double* num_var_w, double* den_mean_acc,
                          double* den_mean_w, double* den_var_acc, double* den_var_w, Pass pass) {
  if (any_null({out_num_cost, out_den_cost, num_mean_acc, num_mean_w, num_var_acc, num_var_w, den_mean_acc, den_mean_w, den_var_acc,
                den_var_w}))
    return fail(SR_EINVAL, "null output");
  const uint32_t U = c->n_utts;
  int rc;
  c->acc_valid = false;
  // numerator: the transcripts' chains.  Its costs stay on the device as the denominator's gate: an utterance without a path through
  // its transcript (F_num = +inf) contributes to neither side.
  uint64_t n_items = 0;
  if ((rc = pass(true, nullptr, &n_items))) return rc;
  if ((rc = netfb_costs(c, scale, out_num_cost))) return rc;
  HIP_TRY(c->mmi_num_cost.ensure(U));
  if (U) HIP_TRY(hipMemcpy(c->mmi_num_cost.p, c->out_cost.p, sizeof(double) * U, hipMemcpyDeviceToDevice));
  if ((rc = accumulate_items(m, c, n_items, 0, max_approx, true, num_mean_acc, num_mean_w, num_var_acc, num_var_w))) return rc;
  // denominator: the free network
  if ((rc = pass(false, c->mmi_num_cost.p, &n_items))) return rc;
  if ((rc = netfb_costs(c, scale, out_den_cost))) return rc;
  rc = accumulate_items(m, c, n_items, 0, max_approx, true, den_mean_acc, den_mean_w, den_var_acc, den_var_w);
  c->acc_valid = false;  // (the handle holds one side only: nothing for sr_model_create_from_accumulated)
  return rc;
}

// sr_net_occupancies_corpus and its test hook: the checks, the pass on `score`'s scores, F_u and the top items to the host
template <class Score>
static int net_occupancies(sr_model* m, sr_corpus* c, sr_lexicon* l, const sr_search_params* p, double scale, double posterior_floor,
                           uint32_t max_items, const uint32_t* trans, const uint64_t* trans_off, Score score, double* out_cost,
                           uint16_t* out_count, uint16_t* out_state, double* out_weight) {
  bool constrained = false;
  int rc = occ_check(m, c, l, p, scale, posterior_floor, trans, trans_off, &constrained);
  if (rc) return rc;
  if (!out_cost) return fail(SR_EINVAL, "null argument");
  bool post = false;
  if ((rc = top_items_arguments(out_count, out_state, out_weight, "out_state", max_items, &post))) return rc;
  uint64_t n_items = 0;
  if ((rc = occ_pass(m, c, l, p, scale, posterior_floor, trans, constrained ? trans_off : nullptr, post, nullptr, &n_items, score)))
    return rc;
  if ((rc = netfb_costs(c, scale, out_cost))) return rc;
  return post ? top_of_items(m, c, max_items, out_count, out_state, out_weight) : SR_OK;
}

int sr_net_occupancies_corpus(sr_model* m, sr_corpus* c, sr_lexicon* l, const sr_search_params* p, double scale, double posterior_floor,
                              uint32_t max_items, const uint32_t* trans, const uint64_t* trans_off, double* out_cost,
                              uint16_t* out_count, uint16_t* out_state, double* out_weight) {
  return guarded(__func__, [&]() -> int {
  if (!p) return fail(SR_EINVAL, "null argument");
  return net_occupancies(m, c, l, p, scale, posterior_floor, max_items, trans, trans_off, gmm_scores(m, c, p->gmm_kernel), out_cost,
                         out_count, out_state, out_weight);
  });
}

// test hook: sr_net_occupancies_corpus with the chunk's score step replaced by a copy of the caller's rows (p->gmm_kernel is not read)
int sr_net_occupancies_corpus_scores(sr_model* m, sr_corpus* c, sr_lexicon* l, const sr_search_params* p, double scale,
                                     double posterior_floor, uint32_t max_items, const uint32_t* trans, const uint64_t* trans_off,
                                     const double* scores, uint64_t n_scores, double* out_cost, uint16_t* out_count, uint16_t* out_state,
                                     double* out_weight) {
  return guarded(__func__, [&]() -> int {
  int rc = check_corpus(m, c);
  if (rc) return rc;
  ScoreTable table;
  if ((rc = table.set(m, c, scores, n_scores))) return rc;
  return table.done(net_occupancies(m, c, l, p, scale, posterior_floor, max_items, trans, trans_off, std::cref(table), out_cost, out_count,
                                    out_state, out_weight));
  });
}

int sr_mmi_statistics_corpus(sr_model* m, sr_corpus* c, sr_lexicon* l, const sr_search_params* p, double scale, double posterior_floor,
                             int max_approx, const uint32_t* trans, const uint64_t* trans_off, double* out_num_cost, double* out_den_cost,
                             double* num_mean_acc, double* num_mean_w, double* num_var_acc, double* num_var_w, double* den_mean_acc,
                             double* den_mean_w, double* den_var_acc, double* den_var_w) {
  return guarded(__func__, [&]() -> int {
  bool constrained = false;
  int rc = occ_check(m, c, l, p, scale, posterior_floor, trans, trans_off, &constrained);
  if (rc) return rc;
  if (!constrained) return fail(SR_EINVAL, "null argument (MMI statistics need the transcripts)");
  return mmi_statistics(m, c, scale, max_approx, out_num_cost, out_den_cost, num_mean_acc, num_mean_w, num_var_acc, num_var_w, den_mean_acc,
                        den_mean_w, den_var_acc, den_var_w, [&](bool numerator, const double* gate, uint64_t* n_items) {
    return occ_pass(m, c, l, p, scale, posterior_floor, numerator ? trans : nullptr, numerator ? trans_off : nullptr, true, gate, n_items);
  });
  });
}

int sr_model_create_from_mmi_statistics(sr_model* m, const double* num_mean_acc, const double* num_mean_w, const double* num_var_acc,
                                        const double* num_var_w, const double* den_mean_acc, const double* den_mean_w,
                                        const double* den_var_acc, const double* den_var_w, double E, double tau, double var_floor,
                                        sr_model** out) {
  return guarded(__func__, [&]() -> int {
  if (!out) return fail(SR_EINVAL, "out is null");
  *out = nullptr;
  int rc = check_model(m);
  if (rc) return rc;
  if (!num_mean_acc || !num_mean_w || !num_var_acc || !num_var_w || !den_mean_acc || !den_mean_w || !den_var_acc || !den_var_w)
    return fail(SR_EINVAL, "null statistics");
  if (!(E > 0.0) || !std::isfinite(E)) return fail(SR_EINVAL, "E must be finite and > 0 (got %g)", E);
  if (!(tau >= 0.0) || !std::isfinite(tau)) return fail(SR_EINVAL, "tau must be finite and >= 0 (got %g)", tau);
  if (!(var_floor > 0.0) || !std::isfinite(var_floor)) return fail(SR_EINVAL, "var_floor must be finite and > 0 (got %g)", var_floor);
  const uint64_t C = m->n_dens;
  const uint32_t D = m->dim;
  // untied: every density owns a mean row and a variance row
  if (m->n_mean != C || m->n_var != C) return fail(SR_EINVAL, "the EBW update needs an untied model (%u mean and %u variance rows for %llu densities)", m->n_mean, m->n_var, (unsigned long long)C);
  {
    std::vector<uint8_t> seen_m(C, 0), seen_v(C, 0);
    for (uint64_t d = 0; d < C; d++) {
      if (seen_m[m->h_dens_mean[d]] || seen_v[m->h_dens_var[d]]) return fail(SR_EINVAL, "the EBW update needs an untied model (density %llu shares a row)", (unsigned long long)d);
      seen_m[m->h_dens_mean[d]] = seen_v[m->h_dens_var[d]] = 1;
    }
  }
  DevBuf<double> d_nma, d_nmw, d_nva, d_dma, d_dmw, d_dva, d_means, d_vars, d_ivars;
  HIP_TRY(d_nma.upload(num_mean_acc, C * D)); HIP_TRY(d_nmw.upload(num_mean_w, C)); HIP_TRY(d_nva.upload(num_var_acc, C * D));
  HIP_TRY(d_dma.upload(den_mean_acc, C * D)); HIP_TRY(d_dmw.upload(den_mean_w, C)); HIP_TRY(d_dva.upload(den_var_acc, C * D));
  HIP_TRY(d_means.ensure(C * D)); HIP_TRY(d_vars.ensure(C * D)); HIP_TRY(d_ivars.ensure(C * D));
  EbwArgs a{};
  a.n_dens = C; a.dim = D; a.dens_mean = m->dens_mean.p; a.dens_var = m->dens_var.p; a.old_means = m->means.p; a.old_inv_vars = m->inv_vars.p;
  a.num_mean_acc = d_nma.p; a.num_mean_w = d_nmw.p; a.num_var_acc = d_nva.p; a.den_mean_acc = d_dma.p; a.den_mean_w = d_dmw.p; a.den_var_acc = d_dva.p;
  a.E = E; a.tau = tau; a.var_floor = var_floor; a.means = d_means.p; a.vars = d_vars.p; a.inv_vars = d_ivars.p;
  HIP_TRY(launch_ebw_combine(a, m->s_gmm));
  HIP_TRY(hipStreamSynchronize(m->s_gmm));
  std::vector<double> means(C * D), vars(C * D), ivars(C * D), norm(C), logw(C);
  if (C) {
    HIP_TRY(hipMemcpy(means.data(), d_means.p, sizeof(double) * C * D, hipMemcpyDeviceToHost));
    HIP_TRY(hipMemcpy(vars.data(), d_vars.p, sizeof(double) * C * D, hipMemcpyDeviceToHost));
    HIP_TRY(hipMemcpy(ivars.data(), d_ivars.p, sizeof(double) * C * D, hipMemcpyDeviceToHost));
    HIP_TRY(hipMemcpy(logw.data(), m->logw.p, sizeof(double) * C, hipMemcpyDeviceToHost));  // the mixture weights stay
  }
  for (uint64_t d = 0; d < C; d++) {  // the host's log, in finalize_core's order (em_finalize.hip)
    double acc = D * log(2 * M_PI);
    for (uint32_t k = 0; k < D; k++) acc = acc + log(vars[d * D + k]);
    norm[d] = acc / 2;
  }
  sr_model* nm = nullptr;
  if ((rc = sr_model_create(m->device, D, m->n_states, m->h_dens_off.data(), means.data(), ivars.data(), norm.data(), logw.data(),
                            m->max_approx ? 1 : 0, &nm)))
    return rc;
  if ((rc = sr_model_set_tying(nm, m->n_mean, m->n_var, m->h_dens_mean.data(), m->h_dens_var.data()))) {
    sr_model_destroy(nm);
    return rc;
  }
  *out = nm;
  return SR_OK;
  });
}

// ---- sMBR training over the recognition network (viterbi_smbr.hip) ----------------------------------------------------------------
int sr_smbr_max_positions(uint32_t* out) {
  if (!out) return fail(SR_EINVAL, "out is null");
  *out = (uint32_t)smbr_max_slots();
  return SR_OK;
}

// 16 B per (frame, position)
static std::vector<uint64_t> smbr_cost(const sr_corpus* c, const sr_lexicon* l) {
  return srplan::linear_cost(c->frame_off.data(), c->n_utts, 16ull * l->net.n_slots);
}

// netfb_check with the accuracy pass' position limit and 16 B per (frame, position), plus the references
static int smbr_check(sr_model* m, sr_corpus* c, sr_lexicon* l, const sr_search_params* p, double scale, double posterior_floor,
                      const uint16_t* ref_states) {
  int rc = netfb_check(m, c, l, p, scale, posterior_floor);
  if (rc) return rc;
  if (!ref_states) return fail(SR_EINVAL, "null argument (ref_states)");
  const uint64_t P = l->net.n_slots;
  if (P > smbr_max_slots())
    return fail(SR_ELIMIT, "%llu lexicon positions exceed the accuracy forward-backward's %llu", (unsigned long long)P,
                (unsigned long long)smbr_max_slots());
  return check_fits(m, smbr_cost(c, l));
}

// kappa F_u, Abar_u on the device -> F_u, Abar_u
static int smbr_costs(sr_corpus* c, double scale, double* out_cost, double* out_acc) {
  int rc = netfb_costs(c, scale, out_cost);
  if (rc) return rc;
  if (c->n_utts) HIP_TRY(hipMemcpy(out_acc, c->smbr_acc.p, sizeof(double) * c->n_utts, hipMemcpyDeviceToHost));
  return SR_OK;
}

// NetFbPass for the accuracy recursions: the launch groups are consecutive utterances of a chunk whose trellises (16 B per frame and
// position) fit m->fb_budget together (smbr_check: every utterance fits alone).  run() enqueues a chunk's groups in order: forward,
// backward, then per_group(item arguments of the group, frames of the group).  want_items: the item path is ready (ensure_items) and
// `ia` writes to c->fb_item_*.
struct SmbrPass {
  srplan::Groups groups;
  SmbrArgs a{};
  ItemArgs ia{};  // the free network's mixture lists
  uint64_t item_bound = 0;
  size_t scan_bytes = 0;
  size_t ci = 0;  // run_chunks searches the chunks in order

  int setup(sr_model* m, sr_corpus* c, sr_lexicon* l, const sr_search_params* p, double scale, double floor, const uint16_t* ref_states,
            bool want_items, const std::vector<Chunk>& chunks) {
    const uint64_t P = l->net.n_slots, F = c->n_frames;
    groups = srplan::launch_groups(chunks, smbr_cost(c, l).data(), m->fb_budget);
    const uint64_t max_gf = std::max<uint64_t>(1, groups.max_span(c->frame_off.data()));
    // the lexicon's distinct mixtures (ascending) and the positions carrying each, as occ_pass lists them
    srplan::MixLists<uint16_t> ml;
    ml.add(l->h_slot_info.data(), P, 0xFFFFu);
    item_bound = F * ml.n_mix(0);
    if (item_bound >= (1ull << 31)) return fail(SR_ELIMIT, "too many (frame, mixture) weights");
    HIP_TRY(c->fb_trellis.ensure(max_gf * 2 * P));
    HIP_TRY(c->smbr_ends.ensure(max_gf * 2));
    HIP_TRY(c->out_cost.ensure(c->n_utts));
    HIP_TRY(c->smbr_acc.ensure(c->n_utts));
    HIP_TRY(c->smbr_ref.upload(ref_states, F));
    int rc = upload_mix_lists(c, ml, false, c->fb_slot_pos);
    if (rc) return rc;
    if (want_items && (rc = ensure_items(c, max_gf, F, item_bound, &scan_bytes))) return rc;
    a.net = l->net; a.ld = m->ld; a.frame_off = c->d_frame_off.p; a.scale = scale; a.word_penalty = p->word_penalty;
    a.ref = c->smbr_ref.p; a.trellis = c->fb_trellis.p; a.ends = c->smbr_ends.p; a.out_cost = c->out_cost.p; a.out_acc = c->smbr_acc.p;
    occ_item_fields(&ia, c, ml, false, P, c->fb_slot_pos, 0, nullptr, floor);
    ia.row_stride = (uint32_t)(2 * P);
    // trellis traffic per (frame, position): (alpha, abar) out, both in + the part out, the part in (items)
    if (m->profiling) m->prof.search_bytes += 48.0 * (double)P * (double)F;
    return SR_OK;
  }
  template <class PerGroup>
  int run(sr_corpus* c, const Chunk& ch, const double* table, hipStream_t s, PerGroup per_group) {
    for (const Group& g : groups.of_chunk[ci]) {
      a.scores = table; a.frame_base = ch.f0; a.utt_first = g.u0; a.n_utts = g.u1 - g.u0; a.group_f0 = c->frame_off[g.u0];
      HIP_TRY(launch_smbr_forward(a, s));
      HIP_TRY(launch_smbr_backward(a, s));
      const uint64_t n = item_group(&ia, c, g.u0, g.u1);
      int rc = per_group(ia, n);
      if (rc) return rc;
    }
    ci++;
    return SR_OK;
  }
};

// What the accuracy and sMBR statistics calls of either network do once their check has passed.  Pass is the network's pass (SmbrPass,
// BgSmbrPass), setup(pass, chunks, want_items) its set-up.
template <class Pass, class Setup, class Score>
static int smbr_accuracies(sr_model* m, sr_corpus* c, Score score, double scale, uint32_t max_items, double* out_cost, double* out_acc,
                           uint16_t* out_count, uint16_t* out_state, double* out_weight, Setup setup) {
  if (!out_cost || !out_acc) return fail(SR_EINVAL, "null argument");
  bool post = false;
  int rc = top_items_arguments(out_count, out_state, out_weight, "out_state", max_items, &post);
  if (rc) return rc;
  std::vector<Chunk> chunks;
  if ((rc = prepare_chunks(m, c, &chunks))) return rc;
  Pass sp;
  if ((rc = setup(sp, chunks, post))) return rc;
  rc = run_chunks(m, chunks, [&](const Chunk& ch, double* table) -> int { return score(ch, table); },
      [&](const Chunk& ch, const double* table, hipStream_t s) -> int {
        if (post && sp.ci == 0) HIP_TRY(reset_item_count(c->fb_base, s));
        return sp.run(c, ch, table, s, [&](const ItemArgs& ia, uint64_t n) -> int {
          if (post) HIP_TRY(launch_items(ia, 0, n, c->fb_scan_temp.p, sp.scan_bytes, c->fb_scan.p, s));
          return SR_OK;
        });
      });
  if (rc) return rc;
  if (m->profiling) m->prof.frames += c->n_frames;
  if ((rc = smbr_costs(c, scale, out_cost, out_acc))) return rc;
  return post ? top_of_items(m, c, max_items, out_count, out_state, out_weight) : SR_OK;
}

template <class Pass, class Setup>
static int smbr_statistics(sr_model* m, sr_corpus* c, int gmm_kernel, double scale, int max_approx, double* out_cost, double* out_acc,
                           double* num_mean_acc, double* num_mean_w, double* num_var_acc, double* num_var_w, double* den_mean_acc,
                           double* den_mean_w, double* den_var_acc, double* den_var_w, Setup setup) {
  if (any_null({out_cost, out_acc, num_mean_acc, num_mean_w, num_var_acc, num_var_w, den_mean_acc, den_mean_w, den_var_acc, den_var_w}))
    return fail(SR_EINVAL, "null output");
  const uint64_t F = c->n_frames;
  int rc;
  c->acc_valid = false;
  std::vector<Chunk> chunks;
  if ((rc = prepare_chunks(m, c, &chunks))) return rc;
  Pass sp;
  if ((rc = setup(sp, chunks, true))) return rc;
  // one pass, the items of both signs: the positive ones in the fb_item_* buffers, the negative ones beside them
  const uint64_t nb = sp.item_bound;
  HIP_TRY(c->smbr_base.ensure(1)); HIP_TRY(c->smbr_item_off.ensure(F + 1));
  HIP_TRY(c->smbr_item_frame.ensure(nb)); HIP_TRY(c->smbr_item_mix.ensure(nb)); HIP_TRY(c->smbr_item_w.ensure(nb));
  rc = run_chunks(m, chunks, [&](const Chunk& ch, double* table) { return score_chunk(m, c, ch.f0, ch.f1, gmm_kernel, table); },
      [&](const Chunk& ch, const double* table, hipStream_t s) -> int {
        if (sp.ci == 0) {
          HIP_TRY(reset_item_count(c->fb_base, s));
          HIP_TRY(reset_item_count(c->smbr_base, s));
        }
        return sp.run(c, ch, table, s, [&](const ItemArgs& pos, uint64_t n) -> int {
          ItemArgs neg = pos;
          neg.item_base = c->smbr_base.p; neg.item_off = c->smbr_item_off.p;
          neg.item_frame = c->smbr_item_frame.p; neg.item_mix = c->smbr_item_mix.p; neg.item_w = c->smbr_item_w.p;
          HIP_TRY(launch_items(pos, +1, n, c->fb_scan_temp.p, sp.scan_bytes, c->fb_scan.p, s));
          HIP_TRY(launch_items(neg, -1, n, c->fb_scan_temp.p, sp.scan_bytes, c->fb_scan.p, s));
          return SR_OK;
        });
      });
  if (rc) return rc;
  if (m->profiling) m->prof.frames += F;
  if ((rc = smbr_costs(c, scale, out_cost, out_acc))) return rc;
  uint64_t n_pos = 0, n_neg = 0;
  if (c->n_utts && ((rc = read_item_count(c->fb_base, &n_pos)) || (rc = read_item_count(c->smbr_base, &n_neg)))) return rc;
  if ((rc = accumulate_items(m, c, n_pos, 0, max_approx, true, num_mean_acc, num_mean_w, num_var_acc, num_var_w))) return rc;
  if (n_neg) {  // the negative side through the same buffers
    HIP_TRY(hipMemcpy(c->fb_item_frame.p, c->smbr_item_frame.p, sizeof(uint32_t) * n_neg, hipMemcpyDeviceToDevice));
    HIP_TRY(hipMemcpy(c->fb_item_mix.p, c->smbr_item_mix.p, sizeof(uint16_t) * n_neg, hipMemcpyDeviceToDevice));
    HIP_TRY(hipMemcpy(c->fb_item_w.p, c->smbr_item_w.p, sizeof(double) * n_neg, hipMemcpyDeviceToDevice));
  }
  rc = accumulate_items(m, c, n_neg, 0, max_approx, true, den_mean_acc, den_mean_w, den_var_acc, den_var_w);
  c->acc_valid = false;  // (the handle holds one side only: nothing for sr_model_create_from_accumulated)
  return rc;
}

int sr_net_accuracies_corpus(sr_model* m, sr_corpus* c, sr_lexicon* l, const sr_search_params* p, double scale, double posterior_floor,
                             uint32_t max_items, const uint16_t* ref_states, double* out_cost, double* out_acc, uint16_t* out_count,
                             uint16_t* out_state, double* out_weight) {
  return guarded(__func__, [&]() -> int {
  int rc = smbr_check(m, c, l, p, scale, posterior_floor, ref_states);
  if (rc) return rc;
  return smbr_accuracies<SmbrPass>(m, c, gmm_scores(m, c, p->gmm_kernel), scale, max_items, out_cost, out_acc, out_count, out_state,
                                   out_weight, [&](SmbrPass& sp, const std::vector<Chunk>& chunks, bool want_items) {
    return sp.setup(m, c, l, p, scale, posterior_floor, ref_states, want_items, chunks);
  });
  });
}

// test hook: sr_net_accuracies_corpus with the chunk's score step replaced by a copy of the caller's rows (p->gmm_kernel is not read)
int sr_net_accuracies_corpus_scores(sr_model* m, sr_corpus* c, sr_lexicon* l, const sr_search_params* p, double scale,
                                    double posterior_floor, uint32_t max_items, const uint16_t* ref_states, const double* scores,
                                    uint64_t n_scores, double* out_cost, double* out_acc, uint16_t* out_count, uint16_t* out_state,
                                    double* out_weight) {
  return guarded(__func__, [&]() -> int {
  int rc = smbr_check(m, c, l, p, scale, posterior_floor, ref_states);
  if (rc) return rc;
  ScoreTable table;
  if ((rc = table.set(m, c, scores, n_scores))) return rc;
  return table.done(smbr_accuracies<SmbrPass>(m, c, std::cref(table), scale, max_items, out_cost, out_acc, out_count, out_state, out_weight,
                                              [&](SmbrPass& sp, const std::vector<Chunk>& chunks, bool want_items) {
    return sp.setup(m, c, l, p, scale, posterior_floor, ref_states, want_items, chunks);
  }));
  });
}

int sr_smbr_statistics_corpus(sr_model* m, sr_corpus* c, sr_lexicon* l, const sr_search_params* p, double scale, double posterior_floor,
                              int max_approx, const uint16_t* ref_states, double* out_cost, double* out_acc, double* num_mean_acc,
                              double* num_mean_w, double* num_var_acc, double* num_var_w, double* den_mean_acc, double* den_mean_w,
                              double* den_var_acc, double* den_var_w) {
  return guarded(__func__, [&]() -> int {
  int rc = smbr_check(m, c, l, p, scale, posterior_floor, ref_states);
  if (rc) return rc;
  return smbr_statistics<SmbrPass>(m, c, p->gmm_kernel, scale, max_approx, out_cost, out_acc, num_mean_acc, num_mean_w, num_var_acc, num_var_w,
                                   den_mean_acc, den_mean_w, den_var_acc, den_var_w,
                                   [&](SmbrPass& sp, const std::vector<Chunk>& chunks, bool want_items) {
    return sp.setup(m, c, l, p, scale, posterior_floor, ref_states, want_items, chunks);
  });
  });
}

// ---- MMI training over the bigram search network (viterbi_bigram_mmi.hip) ---------------------------------------------------------
// bgfb_check plus the transcript's: *constrained = a transcript pair is given.  free_items: the call makes items of the free network
static int bgocc_check(sr_model* m, sr_corpus* c, sr_bigram* b, double scale, double posterior_floor, const uint32_t* trans,
                       const uint64_t* trans_off, bool free_items, bool* constrained) {
  int rc = bgfb_check(m, c, b, scale, posterior_floor);
  if (rc) return rc;
  if (free_items) {
    std::vector<uint8_t> seen(65536, 0);
    uint64_t n_mix = 0;
    for (uint32_t i : b->h_pos_info) n_mix += !seen[i & 0xFFFFu]++;
    if (n_mix * c->n_frames >= (1ull << 31)) return fail(SR_ELIMIT, "too many (frame, mixture) occupancies");
  }
  if ((trans_off == nullptr) != (trans == nullptr))
    return fail(SR_EINVAL, "partial transcript (pass trans and trans_off, or neither)");
  *constrained = trans_off != nullptr;
  if (!*constrained) return SR_OK;
  if (trans_off[0] != 0) return fail(SR_EINVAL, "trans_off[0] must be 0");
  const uint32_t W = b->net.n_words, sil = b->net.silence;
  const uint64_t sil_len = b->net.silence_states;
  for (uint32_t u = 0; u < c->n_utts; u++) {
    if (trans_off[u + 1] < trans_off[u]) return fail(SR_EINVAL, "trans_off must be non-decreasing (utterance %u)", u);
    const uint64_t n = trans_off[u + 1] - trans_off[u], T = c->frame_off[u + 1] - c->frame_off[u];
    uint64_t N = sil_len * (n + 1);
    for (uint64_t i = trans_off[u]; i < trans_off[u + 1]; i++) {
      const uint32_t w = trans[i];
      if (w >= W || w == sil) return fail(SR_EINVAL, "utterance %u: transcript word %u is not a lexicon word other than silence", u, w);
      N += b->h_slot_off[w + 1] - b->h_slot_off[w];
    }
    if (N > bgchain_max_positions())
      return fail(SR_ELIMIT, "utterance %u: chain of %llu positions exceeds the transcript network's %u", u, (unsigned long long)N,
                  bgchain_max_positions());
    if ((rc = check_fits(m, u, 8 * N * T))) return rc;
  }
  return SR_OK;
}

// the items of the bigram passes: most positions of a mixture a lane sums alone (a silence mixture has W + 1: summed wave-wide)
static constexpr uint32_t kBgItemsSerial = 16;

// One occupancy pass over the corpus on the search's scoring chunks: the free network (trans_off null; BgFbPass' launch groups, workspace
// and table cache) or the transcripts' chains (consecutive utterances whose trellises fit m->fb_budget together).  Leaves kappa F_u in
// c->out_cost and, with want_items, *n_items items in c->fb_item_* (frame order, ascending mixture id) with c->fb_item_off[F + 1];
// utterances whose gate (device, optional) is +inf give no items.
template <class Score>
static int bgocc_pass(sr_model* m, sr_corpus* c, sr_bigram* b, double scale, double posterior_floor, const uint32_t* trans,
                      const uint64_t* trans_off, bool want_items, const double* gate, uint64_t* n_items, Score score) {
  const uint32_t U = c->n_utts;
  const uint64_t F = c->n_frames, P = b->net.n_positions;
  const bool chain = trans_off != nullptr;
  *n_items = 0;
  HIP_TRY(c->out_cost.ensure(U));
  if (U == 0) return SR_OK;
  Chains ch;
  if (chain)
    chain_host::build_bgchains(b->h_slot_off.data(), b->h_pos_info.data(), b->net.n_words, b->net.silence, b->h_lmT.data(), scale, U, trans,
                               trans_off, &ch);
  // the mixture lists only where items are wanted
  const srplan::OccPlan<uint32_t> pl(c->frame_off.data(), U, chain ? ch.off.data() : nullptr, chain ? ch.info.data() : b->h_pos_info.data(), P,
                                     want_items);
  if (want_items && pl.item_bound >= (1ull << 31)) return fail(SR_ELIMIT, "too many (frame, mixture) occupancies");
  std::vector<Chunk> chunks;
  int rc = prepare_chunks(m, c, &chunks);
  if (rc) return rc;
  // the chains' launch groups (bgocc_check: every utterance fits alone); the free network's are BgFbPass'
  srplan::Groups groups;
  BgFbPass fp;
  fp.want_words = false;
  if (chain) {
    if ((rc = trellis_groups(m, c, chunks, pl.tr_off, &groups)) || (rc = upload_chains(c, ch))) return rc;
    HIP_TRY(c->bgmmi_lmc.upload(ch.lmc.data(), ch.lmc.size()));
  } else {
    if ((rc = fp.setup(m, c, b, scale, chunks))) return rc;
  }
  size_t scan_bytes = 0;
  if (want_items) {
    const uint64_t max_gf = std::max<uint64_t>(1, (chain ? groups : fp.groups).max_span(c->frame_off.data()));
    if ((rc = upload_mix_lists(c, pl.ml, chain, c->bgmmi_slot_pos)) || (rc = ensure_items(c, max_gf, F, pl.item_bound, &scan_bytes))) return rc;
  }
  BgChainArgs ca{};
  ca.ld = m->ld; ca.frame_off = c->d_frame_off.p; ca.scale = scale;
  memcpy(ca.tdp, b->net.tdp, sizeof(ca.tdp));
  ca.chain_off = c->mmi_chain_off.p; ca.info = c->mmi_info.p; ca.src = c->mmi_src.p; ca.dst = c->mmi_dst.p; ca.lmc = c->bgmmi_lmc.p;
  ca.sil_len = b->net.silence_states;
  ca.trellis = c->fb_trellis.p; ca.trellis_off = c->fb_trellis_off.p; ca.out_cost = c->out_cost.p;
  ItemArgs ia{};
  occ_item_fields(&ia, c, pl.ml, chain, P, c->bgmmi_slot_pos, kBgItemsSerial, gate, posterior_floor);
  auto items = [&](uint32_t u0, uint32_t u1, hipStream_t s) -> int {
    if (!want_items) return SR_OK;
    const uint64_t n = item_group(&ia, c, u0, u1);
    HIP_TRY(launch_items(ia, +1, n, c->fb_scan_temp.p, scan_bytes, c->fb_scan.p, s));
    return SR_OK;
  };
  size_t ci = 0;  // run_chunks searches the chunks in order
  rc = run_chunks(m, chunks, [&](const Chunk& k, double* table) -> int { return score(k, table); },
      [&](const Chunk& k, const double* table, hipStream_t s) -> int {
        if (want_items && ci == 0) HIP_TRY(reset_item_count(c->fb_base, s));
        if (!chain) {
          ci++;
          return fp.run(c, k, table, s, [&](const BgFbArgs& a, uint64_t) -> int {
            const uint32_t u0 = (uint32_t)(a.order - fp.d_order);
            return items(u0, u0 + a.n_group, s);
          });
        }
        for (const Group& g : groups.of_chunk[ci]) {
          ca.scores = table; ca.frame_base = k.f0; ca.utt_first = g.u0; ca.n_utts = g.u1 - g.u0;
          ca.max_positions = srplan::max_positions(g, ch.off.data());
          HIP_TRY(launch_bgchain_forward(ca, s));
          HIP_TRY(launch_bgchain_backward(ca, s));
          int r = items(g.u0, g.u1, s);
          if (r) return r;
        }
        ci++;
        return SR_OK;
      });
  if (rc) return rc;
  if (want_items && (rc = read_item_count(c->fb_base, n_items))) return rc;
  if (m->profiling) {
    // per (frame, position): alpha out, alpha in + gamma out (the free network: counted by BgFbPass, whose word-posterior read of gamma
    // is the items' count pass here); the items' write pass reads gamma once more
    m->prof.frames += F;
    if (chain) m->prof.search_bytes += (want_items ? 40.0 : 24.0) * (double)pl.tr_off[U];
    else if (want_items) m->prof.search_bytes += 8.0 * (double)P * (double)F;
  }
  return SR_OK;
}

// bgocc_check as sr_bigram_occupancies_corpus and its test hook call it
static int bigram_occupancies_check(sr_model* m, sr_corpus* c, sr_bigram* b, double scale, double posterior_floor, const uint32_t* trans,
                                    const uint64_t* trans_off, const uint16_t* out_count, const uint16_t* out_state,
                                    const double* out_weight, bool* constrained) {
  return bgocc_check(m, c, b, scale, posterior_floor, trans, trans_off, !trans_off && (out_count || out_state || out_weight), constrained);
}

// sr_bigram_occupancies_corpus and its test hook: the pass on `score`'s scores once the check has passed, F_u and the top items to the
// host
template <class Score>
static int bigram_occupancies(sr_model* m, sr_corpus* c, sr_bigram* b, double scale, double posterior_floor, uint32_t max_items,
                              const uint32_t* trans, const uint64_t* trans_off, bool constrained, Score score, double* out_cost,
                              uint16_t* out_count, uint16_t* out_state, double* out_weight) {
  int rc;
  if (!out_cost) return fail(SR_EINVAL, "null argument");
  bool post = false;
  if ((rc = top_items_arguments(out_count, out_state, out_weight, "out_state", max_items, &post))) return rc;
  uint64_t n_items = 0;
  if ((rc = bgocc_pass(m, c, b, scale, posterior_floor, trans, constrained ? trans_off : nullptr, post, nullptr, &n_items, score))) return rc;
  if ((rc = netfb_costs(c, scale, out_cost))) return rc;
  return post ? top_of_items(m, c, max_items, out_count, out_state, out_weight) : SR_OK;
}

int sr_bigram_occupancies_corpus(sr_model* m, sr_corpus* c, sr_bigram* b, int gmm_kernel, double scale, double posterior_floor,
                                 uint32_t max_items, const uint32_t* trans, const uint64_t* trans_off, double* out_cost,
                                 uint16_t* out_count, uint16_t* out_state, double* out_weight) {
  return guarded(__func__, [&]() -> int {
  bool constrained = false;
  int rc = bigram_occupancies_check(m, c, b, scale, posterior_floor, trans, trans_off, out_count, out_state, out_weight, &constrained);
  if (rc) return rc;
  return bigram_occupancies(m, c, b, scale, posterior_floor, max_items, trans, trans_off, constrained, gmm_scores(m, c, gmm_kernel), out_cost,
                            out_count, out_state, out_weight);
  });
}

// test hook: sr_bigram_occupancies_corpus with the chunk's score step replaced by a copy of the caller's rows
int sr_bigram_occupancies_corpus_scores(sr_model* m, sr_corpus* c, sr_bigram* b, double scale, double posterior_floor, uint32_t max_items,
                                        const uint32_t* trans, const uint64_t* trans_off, const double* scores, uint64_t n_scores,
                                        double* out_cost, uint16_t* out_count, uint16_t* out_state, double* out_weight) {
  return guarded(__func__, [&]() -> int {
  bool constrained = false;
  int rc = bigram_occupancies_check(m, c, b, scale, posterior_floor, trans, trans_off, out_count, out_state, out_weight, &constrained);
  if (rc) return rc;
  ScoreTable table;
  if ((rc = table.set(m, c, scores, n_scores)) || (rc = table.refuse_neg_inf(scores, n_scores))) return rc;
  return table.done(bigram_occupancies(m, c, b, scale, posterior_floor, max_items, trans, trans_off, constrained, std::cref(table), out_cost,
                                       out_count, out_state, out_weight));
  });
}

int sr_bigram_mmi_statistics_corpus(sr_model* m, sr_corpus* c, sr_bigram* b, int gmm_kernel, double scale, double posterior_floor,
                                    int max_approx, const uint32_t* trans, const uint64_t* trans_off, double* out_num_cost,
                                    double* out_den_cost, double* num_mean_acc, double* num_mean_w, double* num_var_acc, double* num_var_w,
                                    double* den_mean_acc, double* den_mean_w, double* den_var_acc, double* den_var_w) {
  return guarded(__func__, [&]() -> int {
  bool constrained = false;
  int rc = bgocc_check(m, c, b, scale, posterior_floor, trans, trans_off, true, &constrained);
  if (rc) return rc;
  if (!constrained) return fail(SR_EINVAL, "null argument (MMI statistics need the transcripts)");
  return mmi_statistics(m, c, scale, max_approx, out_num_cost, out_den_cost, num_mean_acc, num_mean_w, num_var_acc, num_var_w, den_mean_acc,
                        den_mean_w, den_var_acc, den_var_w, [&](bool numerator, const double* gate, uint64_t* n_items) {
    return bgocc_pass(m, c, b, scale, posterior_floor, numerator ? trans : nullptr, numerator ? trans_off : nullptr, true, gate, n_items,
                      gmm_scores(m, c, gmm_kernel));
  });
  });
}

// ---- sMBR training over the bigram search network (viterbi_bigram_smbr.hip) -------------------------------------------------------
// 16 B per (frame, position) and twice BgFbPass' vectors per utterance
static std::vector<uint64_t> bgsmbr_cost(const sr_corpus* c, const sr_bigram* b) {
  return srplan::linear_cost(c->frame_off.data(), c->n_utts, 16ull * b->net.n_positions, 2 * bgfb_utt_bytes(b));
}

// bgocc_check's free pass with items, at the accuracy pass' bytes, plus the references
static int bgsmbr_check(sr_model* m, sr_corpus* c, sr_bigram* b, double scale, double posterior_floor, const uint16_t* ref_states) {
  bool constrained = false;
  int rc = bgocc_check(m, c, b, scale, posterior_floor, nullptr, nullptr, true, &constrained);
  if (rc) return rc;
  if (!ref_states) return fail(SR_EINVAL, "null argument (ref_states)");
  return check_fits(m, bgsmbr_cost(c, b));
}

// BgStepPass at multiplicity 2 for the accuracy recursions: the groups cut on 16 B per (frame, position) and twice the vectors, the
// items' mixture lists bgocc_pass' free ones.  run() enqueues a chunk's groups: the recursion on both operand vectors, then
// per_group(item arguments of the group, frames of the group).  `ia` writes to c->fb_item_*.
struct BgSmbrPass : BgStepPass {
  BgSmbrArgs a{};
  ItemArgs ia{};
  uint64_t item_bound = 0;
  size_t scan_bytes = 0;

  int setup(sr_model* m, sr_corpus* c, sr_bigram* b, double scale, double floor, const uint16_t* ref_states,
            const std::vector<Chunk>& chunks) {
    const uint64_t P = b->net.n_positions, F = c->n_frames;
    const uint32_t U = c->n_utts;
    srplan::MixLists<uint32_t> ml;
    ml.add(b->h_pos_info.data(), P, 0xFFFFu);
    item_bound = F * ml.n_mix(0);  // (bgsmbr_check: below 2^31)
    // what this pass clears and uploads goes ahead of the workspace's synchronisation.  T_u = 0: Abar_u = 0
    HIP_TRY(c->smbr_acc.ensure(U));
    if (U) HIP_TRY(hipMemset(c->smbr_acc.p, 0, sizeof(double) * U));
    HIP_TRY(c->smbr_ref.upload(ref_states, F));
    int rc = upload_mix_lists(c, ml, false, c->bgmmi_slot_pos);
    if (rc) return rc;
    if ((rc = workspace(m, c, b, scale, 2, bgsmbr_cost(c, b), chunks, &a.fb))) return rc;
    if ((rc = ensure_items(c, max_gf, F, item_bound, &scan_bytes))) return rc;
    a.ref = c->smbr_ref.p; a.out_acc = c->smbr_acc.p;
    occ_item_fields(&ia, c, ml, false, P, c->bgmmi_slot_pos, kBgItemsSerial, nullptr, floor);
    ia.row_stride = (uint32_t)(2 * P);
    // trellis traffic per (frame, position): (alpha, abar) out, the previous row's pair in; both in + gamma out; the items read gamma
    if (m->profiling) m->prof.search_bytes += 64.0 * (double)P * (double)F;
    return SR_OK;
  }
  template <class PerGroup>
  int run(sr_corpus* c, const Chunk& ch, const double* table, hipStream_t s, PerGroup per_group) {
    return run_groups(c, ch, table, s, &a.fb, [&] { return launch_bgsmbr_forward(a, s); }, [&] { return launch_bgsmbr_backward(a, s); },
                      [&](const Group& g) -> int {
                        const uint64_t n = item_group(&ia, c, g.u0, g.u1);
                        return per_group(ia, n);
                      });
  }
};

int sr_bigram_accuracies_corpus(sr_model* m, sr_corpus* c, sr_bigram* b, int gmm_kernel, double scale, double posterior_floor,
                                uint32_t max_items, const uint16_t* ref_states, double* out_cost, double* out_acc, uint16_t* out_count,
                                uint16_t* out_state, double* out_weight) {
  return guarded(__func__, [&]() -> int {
  int rc = bgsmbr_check(m, c, b, scale, posterior_floor, ref_states);
  if (rc) return rc;
  return smbr_accuracies<BgSmbrPass>(m, c, gmm_scores(m, c, gmm_kernel), scale, max_items, out_cost, out_acc, out_count, out_state, out_weight,
                                     [&](BgSmbrPass& sp, const std::vector<Chunk>& chunks, bool) {
    return sp.setup(m, c, b, scale, posterior_floor, ref_states, chunks);
  });
  });
}

// test hook: sr_bigram_accuracies_corpus with the chunk's score step replaced by a copy of the caller's rows
int sr_bigram_accuracies_corpus_scores(sr_model* m, sr_corpus* c, sr_bigram* b, double scale, double posterior_floor, uint32_t max_items,
                                       const uint16_t* ref_states, const double* scores, uint64_t n_scores, double* out_cost,
                                       double* out_acc, uint16_t* out_count, uint16_t* out_state, double* out_weight) {
  return guarded(__func__, [&]() -> int {
  int rc = bgsmbr_check(m, c, b, scale, posterior_floor, ref_states);
  if (rc) return rc;
  ScoreTable table;
  if ((rc = table.set(m, c, scores, n_scores)) || (rc = table.refuse_neg_inf(scores, n_scores))) return rc;
  return table.done(smbr_accuracies<BgSmbrPass>(m, c, std::cref(table), scale, max_items, out_cost, out_acc, out_count, out_state, out_weight,
                                                [&](BgSmbrPass& sp, const std::vector<Chunk>& chunks, bool) {
    return sp.setup(m, c, b, scale, posterior_floor, ref_states, chunks);
  }));
  });
}

int sr_bigram_smbr_statistics_corpus(sr_model* m, sr_corpus* c, sr_bigram* b, int gmm_kernel, double scale, double posterior_floor,
                                     int max_approx, const uint16_t* ref_states, double* out_cost, double* out_acc, double* num_mean_acc,
                                     double* num_mean_w, double* num_var_acc, double* num_var_w, double* den_mean_acc, double* den_mean_w,
                                     double* den_var_acc, double* den_var_w) {
  return guarded(__func__, [&]() -> int {
  int rc = bgsmbr_check(m, c, b, scale, posterior_floor, ref_states);
  if (rc) return rc;
  return smbr_statistics<BgSmbrPass>(m, c, gmm_kernel, scale, max_approx, out_cost, out_acc, num_mean_acc, num_mean_w, num_var_acc, num_var_w,
                                     den_mean_acc, den_mean_w, den_var_acc, den_var_w,
                                     [&](BgSmbrPass& sp, const std::vector<Chunk>& chunks, bool) {
    return sp.setup(m, c, b, scale, posterior_floor, ref_states, chunks);
  });
  });
}

// ---- word lattices over the recognition network (viterbi_lattice.hip) ---------------------------------------------------------
// Per frame the word-end tables take 8 W (fwd) + 2 W (first) + 16 (E, Bend) bytes, and the emit step's count and scan 16 more.
static uint64_t lattice_frame_bytes(const sr_lexicon* l) { return 10ull * l->net.n_words + 32; }
static std::vector<uint64_t> lattice_cost(const sr_corpus* c, const sr_lexicon* l) {
  return srplan::linear_cost(c->frame_off.data(), c->n_utts, lattice_frame_bytes(l));
}

// What both lattice entry points do once their pass has run: the arc offsets per utterance from the frames' (c->lat_frame_arc, the
// total in c->lat_base), the best costs, and -- the caller wants the arcs, and the arrays of `cap` hold them -- *n_arcs for
// copy_arcs.  *n_arcs = 0: nothing to copy.
static int lattice_offsets(sr_corpus* c, uint64_t cap, bool fill, uint64_t* out_arc_off, double* out_best, uint64_t* n_arcs) {
  const uint32_t U = c->n_utts;
  const uint64_t F = c->n_frames;
  *n_arcs = 0;
  uint64_t total = 0;
  HIP_TRY(hipMemcpy(&total, c->lat_base.p, sizeof(uint64_t), hipMemcpyDeviceToHost));
  std::vector<uint64_t> frame_arc(F + 1);
  if (F) HIP_TRY(hipMemcpy(frame_arc.data(), c->lat_frame_arc.p, sizeof(uint64_t) * F, hipMemcpyDeviceToHost));
  frame_arc[F] = total;
  for (uint32_t u = 0; u <= U; u++) out_arc_off[u] = frame_arc[c->frame_off[u]];
  if (U) HIP_TRY(hipMemcpy(out_best, c->out_cost.p, sizeof(double) * U, hipMemcpyDeviceToHost));
  if (!fill) return SR_OK;
  if (total > cap) return fail(SR_EINVAL, "the lattices hold %llu arcs, the arrays %llu", (unsigned long long)total, (unsigned long long)cap);
  *n_arcs = total;
  return SR_OK;
}
template <class T>
static hipError_t copy_arcs(T* out, const DevBuf<T>& arcs, uint64_t n_arcs) {
  return n_arcs ? hipMemcpy(out, arcs.p, sizeof(T) * n_arcs, hipMemcpyDeviceToHost) : hipSuccess;
}

// The emit side of both lattice passes (lattice_emit.h).  setup(): the count / scan workspace for launch groups of at most max_gf frames,
// the arc counter cleared, the shared arc arrays for arc_cap arcs (0: the sizing call, none) bound into either args struct.
struct LatticeEmit {
  size_t scan_bytes = 0;
  uint64_t cap = 0;

  template <class Args>
  int setup(sr_corpus* c, uint64_t max_gf, uint64_t arc_cap, Args* a, double*& arc_cost) {  // arc_cost: a->arc_cost or a->arc_am
    HIP_TRY(c->lat_cnt.ensure(max_gf)); HIP_TRY(c->lat_scan.ensure(max_gf)); HIP_TRY(c->lat_base.ensure(1));
    HIP_TRY(c->lat_frame_arc.ensure(c->n_frames + 1));
    scan_bytes = lattice_scan_temp_bytes(max_gf);
    HIP_TRY(c->fb_scan_temp.ensure(scan_bytes));
    HIP_TRY(hipMemset(c->lat_base.p, 0, sizeof(uint64_t)));
    cap = arc_cap;
    if (!cap) return SR_OK;
    HIP_TRY(c->lat_arc_word.ensure(cap)); HIP_TRY(c->lat_arc_first.ensure(cap)); HIP_TRY(c->lat_arc_last.ensure(cap));
    HIP_TRY(c->lat_arc_fwd.ensure(cap)); HIP_TRY(c->lat_arc_bwd.ensure(cap)); HIP_TRY(c->lat_arc_cost.ensure(cap));
    a->arc_word = c->lat_arc_word.p; a->arc_first = c->lat_arc_first.p; a->arc_last = c->lat_arc_last.p;
    a->arc_fwd = c->lat_arc_fwd.p; a->arc_bwd = c->lat_arc_bwd.p; arc_cost = c->lat_arc_cost.p;
    return SR_OK;
  }
  template <class Args, class Emit>
  hipError_t launch(Emit emit, const Args& a, sr_corpus* c, const Group& g, hipStream_t s) {
    return emit(a, c->frame_off[g.u1] - c->frame_off[g.u0], c->fb_scan_temp.p, scan_bytes, c->lat_cnt.p, c->lat_scan.p, c->lat_base.p,
                c->lat_frame_arc.p, cap, s);
  }
};

// Both lattice entry points after their own argument checks, with their pass `lp`, its bytes per utterance (`cost`, prefix sums) and slots
// per frame: limits, chunks, setup(device cap, chunks), the pass, the offsets and the shared arrays.  *n_arcs: arcs to copy besides (0: none).
struct LatticeOut {  // the caller's arrays both lattices have: offsets and best costs, then the six per arc (all null: the sizing call)
  uint64_t* arc_off; double* best; uint32_t *word, *first, *last; double *fwd, *bwd, *cost;
};
template <class Pass, class Setup>
static int lattice_corpus(sr_model* m, sr_corpus* c, int gmm_kernel, const std::vector<uint64_t>& cost, uint64_t slots, uint64_t cap,
                          bool fill, Pass& lp, Setup setup, const LatticeOut& out, uint64_t* n_arcs) {
  int rc;
  for (uint32_t u = 0; u < c->n_utts; u++) {
    const uint64_t T = c->frame_off[u + 1] - c->frame_off[u];
    if (T > 65535) return fail(SR_ELIMIT, "utterance %u: %llu frames exceed the lattice's 65535", u, (unsigned long long)T);
    if ((rc = check_fits(m, u, cost[u + 1] - cost[u], true))) return rc;
  }
  std::vector<Chunk> chunks;
  if ((rc = prepare_chunks(m, c, &chunks))) return rc;
  const uint64_t dev_cap = fill ? std::min<uint64_t>(cap, c->n_frames * slots) : 0;  // (no lattice has more arcs than that)
  if ((rc = setup(dev_cap, chunks))) return rc;
  rc = run_chunks(m, chunks, [&](const Chunk& ch, double* table) { return score_chunk(m, c, ch.f0, ch.f1, gmm_kernel, table); },
                  [&](const Chunk& ch, const double* table, hipStream_t s) -> int { return lp.run(c, ch, table, s); });
  if (rc) return rc;
  if (m->profiling) m->prof.frames += c->n_frames;
  if ((rc = lattice_offsets(c, cap, fill, out.arc_off, out.best, n_arcs))) return rc;
  HIP_TRY(copy_arcs(out.word, c->lat_arc_word, *n_arcs));
  HIP_TRY(copy_arcs(out.first, c->lat_arc_first, *n_arcs));
  HIP_TRY(copy_arcs(out.last, c->lat_arc_last, *n_arcs));
  HIP_TRY(copy_arcs(out.fwd, c->lat_arc_fwd, *n_arcs));
  HIP_TRY(copy_arcs(out.bwd, c->lat_arc_bwd, *n_arcs));
  HIP_TRY(copy_arcs(out.cost, c->lat_arc_cost, *n_arcs));
  return SR_OK;
}

// The launch groups of a lattice pass -- NetFbPass' grouping on the lattice's bytes per frame: consecutive utterances of a chunk
// whose word-end tables fit m->fb_budget together (every utterance fits alone: checked by the entry point).  run() enqueues a
// chunk's groups in order: forward, backward, emit.
struct LatticePass {
  srplan::Groups groups;
  LatticeArgs a{};
  LatticeEmit emit;
  size_t ci = 0;

  int setup(sr_model* m, sr_corpus* c, sr_lexicon* l, const sr_search_params* p, double beam, uint64_t arc_cap,
            const std::vector<Chunk>& chunks) {
    const uint64_t W = l->net.n_words;
    groups = srplan::launch_groups(chunks, lattice_cost(c, l).data(), m->fb_budget);
    const uint64_t max_gf = std::max<uint64_t>(1, groups.max_span(c->frame_off.data()));
    if (max_gf >= (1ull << 31)) return fail(SR_ELIMIT, "too many frames in one launch group");
    HIP_TRY(c->lat_fwd.ensure(max_gf * W));
    HIP_TRY(c->lat_first.ensure(max_gf * W));
    HIP_TRY(c->lat_ends.ensure(max_gf));
    HIP_TRY(c->lat_bend.ensure(max_gf));
    HIP_TRY(c->out_cost.ensure(c->n_utts));
    if (int rc = emit.setup(c, max_gf, arc_cap, &a, a.arc_cost)) return rc;
    a.net = l->net; a.ld = m->ld; a.frame_off = c->d_frame_off.p;
    a.word_penalty = p->word_penalty; a.beam = beam;
    a.fwd = c->lat_fwd.p; a.first = c->lat_first.p; a.ends = c->lat_ends.p; a.bend = c->lat_bend.p; a.out_best = c->out_cost.p;
    // word-end tables per frame: fwd, first, E and Bend out, then in again for the count and for the write
    if (m->profiling) m->prof.search_bytes += (30.0 * (double)W + 48.0) * (double)c->n_frames;
    return SR_OK;
  }
  int run(sr_corpus* c, const Chunk& ch, const double* table, hipStream_t s) {
    for (const Group& g : groups.of_chunk[ci]) {
      a.scores = table; a.frame_base = ch.f0; a.utt_first = g.u0; a.n_utts = g.u1 - g.u0; a.group_f0 = c->frame_off[g.u0];
      HIP_TRY(launch_lattice_forward(a, s));
      HIP_TRY(launch_lattice_backward(a, s));
      HIP_TRY(emit.launch(launch_lattice_emit, a, c, g, s));
    }
    ci++;
    return SR_OK;
  }
};

int sr_word_lattice_corpus(sr_model* m, sr_corpus* c, sr_lexicon* l, const sr_search_params* p, double lattice_beam, uint64_t cap,
                           uint64_t* out_arc_off, double* out_best, uint32_t* out_word, uint32_t* out_first, uint32_t* out_last,
                           double* out_fwd, double* out_bwd, double* out_cost) {
  return guarded(__func__, [&]() -> int {
  int rc = check_corpus(m, c);
  if (rc) return rc;
  if (!l || l->model != m) return fail(SR_EINVAL, "lexicon does not belong to this model");
  if (!p || !out_arc_off || !out_best) return fail(SR_EINVAL, "null argument");
  if (p->flags != 0) return fail(SR_EINVAL, "sr_search_params.flags must be 0 (got 0x%x)", (unsigned)p->flags);
  if (!(lattice_beam >= 0.0)) return fail(SR_EINVAL, "lattice_beam must be >= 0 (got %g)", lattice_beam);
  const bool fill = out_word || out_first || out_last || out_fwd || out_bwd || out_cost;
  if (fill && (!out_word || !out_first || !out_last || !out_fwd || !out_bwd || !out_cost))
    return fail(SR_EINVAL, "null output (pass all six arc arrays, or none)");
  const uint64_t P = l->net.n_slots;
  if (P > lattice_max_slots())
    return fail(SR_ELIMIT, "%llu lexicon positions exceed the word lattice's %llu", (unsigned long long)P,
                (unsigned long long)lattice_max_slots());
  LatticePass lp;
  uint64_t n = 0;
  return lattice_corpus(m, c, p->gmm_kernel, lattice_cost(c, l), l->net.n_words, cap, fill, lp,
                        [&](uint64_t dev_cap, const std::vector<Chunk>& chunks) { return lp.setup(m, c, l, p, lattice_beam, dev_cap, chunks); },
                        LatticeOut{out_arc_off, out_best, out_word, out_first, out_last, out_fwd, out_bwd, out_cost}, &n);
  });
}

// ---- word lattices over the bigram search network (viterbi_bigram_lattice.hip) -----------------------------------------------------
// Workspace counted in SRGPU_FB_MB: per (frame, slot) fwd 8 + bwd 8 + first 2 + pred 4 bytes over 2 W slots, and the emit step's count
// and scan; per utterance the vectors vec / prod / wend (8 Kp each) and arg (4 Kp), the two rows of cost 8 + first 2 + pred 4 per position
static uint64_t bglat_frame_bytes(const sr_bigram* b) { return 44ull * b->net.n_words + 16; }
static uint64_t bglat_utt_bytes(const sr_bigram* b) { return 28ull * bgfb_padded(b->net.n_words) + 28ull * b->net.n_positions; }
static std::vector<uint64_t> bglat_cost(const sr_corpus* c, const sr_bigram* b) {
  return srplan::linear_cost(c->frame_off.data(), c->n_utts, bglat_frame_bytes(b), bglat_utt_bytes(b));
}

// The launch groups of a pass, cut like BgFbPass' on the lattice's bytes, each with its utterances ordered longest first.  run()
// enqueues a chunk's groups: per frame the in-word step and the min-plus entry, forward then backward, then the arcs.
struct BgLatPass {
  srplan::Groups groups;
  srplan::StepOrder steps;                 // each group's range, longest first
  BgLatArgs a{};
  const float *tab_fwd = nullptr, *tab_bwd = nullptr;
  const uint32_t* d_order = nullptr;
  LatticeEmit emit;
  size_t ci = 0;
  uint32_t rows = 0;
  int argmin = 0;

  int setup(sr_model* m, sr_corpus* c, sr_bigram* b, double beam, uint64_t arc_cap, const std::vector<Chunk>& chunks) {
    const uint64_t P = b->net.n_positions;
    const uint32_t W = b->net.n_words, Kp = bgfb_padded(W), U = c->n_utts;
    groups = srplan::launch_groups(chunks, bglat_cost(c, b).data(), m->fb_budget);
    steps = srplan::StepOrder(groups, c->frame_off.data(), U);
    const uint64_t max_gf = std::max<uint64_t>(1, groups.max_span(c->frame_off.data()));
    const uint32_t max_gu = std::max(1u, groups.max_utts());
    if (max_gf >= (1ull << 31)) return fail(SR_ELIMIT, "too many frames in one launch group");
    // the table in the other orientation: built once per net
    if (!b->lat_lm_built) {
      HIP_TRY(b->lat_lm.ensure((size_t)W * W));
      HIP_TRY(launch_bglat_transpose(b->lmT.p, W, b->lat_lm.p, m->s_search));
      HIP_TRY(hipStreamSynchronize(m->s_search));
      b->lat_lm_built = true;
    }
    tab_fwd = b->lmT.p; tab_bwd = b->lat_lm.p;
    const char* env = getenv("SRGPU_BGLAT_ARGMIN");  // "rescan": the min-only loop with an equality rescan (same bits; for measuring)
    argmin = env && !strcmp(env, "rescan") ? 1 : 0;
    rows = max_gu;
    const size_t S = 2 * (size_t)W;
    HIP_TRY(c->bglat_fwd.ensure(max_gf * S));
    HIP_TRY(c->bglat_bwd.ensure(max_gf * S));
    HIP_TRY(c->bglat_first.ensure(max_gf * S));
    HIP_TRY(c->bglat_pred.ensure(max_gf * S));
    HIP_TRY(c->bgfb_vec.ensure((size_t)rows * Kp));
    HIP_TRY(c->bgfb_prod.ensure((size_t)rows * Kp));
    HIP_TRY(c->bgfb_wend.ensure((size_t)rows * Kp));
    HIP_TRY(c->bglat_arg.ensure((size_t)rows * Kp));
    HIP_TRY(c->bgfb_xb.ensure(2 * (size_t)max_gu * P));
    HIP_TRY(c->bglat_row_first.ensure(2 * (size_t)max_gu * P));
    HIP_TRY(c->bglat_row_pred.ensure(2 * (size_t)max_gu * P));
    HIP_TRY(c->bgfb_order.upload(steps.order.data(), steps.order.size()));
    d_order = c->bgfb_order.p;
    HIP_TRY(c->out_cost.ensure(U));
    if (int rc = emit.setup(c, max_gf, arc_cap, &a, a.arc_am)) return rc;
    if (U) HIP_TRY(hipMemset(c->out_cost.p, 0, sizeof(double) * U));  // T_u = 0: the empty path ends at the start's word end
    HIP_TRY(hipDeviceSynchronize());
    bg_net_args(m, c, b, &a);
    a.beam = beam;
    a.fwd = c->bglat_fwd.p; a.bwd = c->bglat_bwd.p; a.first = c->bglat_first.p; a.pred = c->bglat_pred.p;
    a.vec = c->bgfb_vec.p; a.prod = c->bgfb_prod.p; a.wend = c->bgfb_wend.p; a.arg = c->bglat_arg.p;
    a.row = c->bgfb_xb.p; a.row_first = c->bglat_row_first.p; a.row_pred = c->bglat_row_pred.p;
    a.out_best = c->out_cost.p;
    if (arc_cap) {
      HIP_TRY(c->bglat_arc_hist.ensure(arc_cap)); HIP_TRY(c->bglat_arc_pred.ensure(arc_cap));
      a.arc_hist = c->bglat_arc_hist.p; a.arc_pred = c->bglat_arc_pred.p;
    }
    // per frame: the rows of both walks (cost, first, pred in and out forward: 28, e + beta in and out backward: 16 per position) and
    // the word-end tables (22 per slot out, fwd and bwd in again for the count, all of it for the write: 60 per slot, 2 W slots)
    if (m->profiling) m->prof.search_bytes += (44.0 * (double)P + 120.0 * (double)W) * (double)c->n_frames;
    return SR_OK;
  }
  int run(sr_corpus* c, const Chunk& ch, const double* table, hipStream_t s) {
    for (const Group& g : groups.of_chunk[ci]) {
      a.scores = table; a.frame_base = ch.f0; a.group_f0 = c->frame_off[g.u0];
      a.order = d_order + g.u0; a.utt_first = g.u0; a.n_group = g.u1 - g.u0;
      const uint32_t t_max = steps.t_max(g);
      HIP_TRY(launch_bglat_init(a, rows, s));
      HIP_TRY(launch_bglat_entry(tab_fwd, a.vec, a.prod, a.arg, a.n_words, a.Kp, steps.alive(g, 0), argmin, s));
      for (uint32_t t = 0; t < t_max; t++) {
        a.t = t; a.n_alive = steps.alive(g, t);
        HIP_TRY(launch_bglat_forward(a, s));
        HIP_TRY(launch_bglat_entry(tab_fwd, a.vec, a.prod, a.arg, a.n_words, a.Kp, steps.alive(g, t + 1), argmin, s));
      }
      for (uint32_t t = t_max; t-- > 0;) {
        a.t = t; a.n_alive = steps.alive(g, t);
        HIP_TRY(launch_bglat_backward(a, s));
        if (t) HIP_TRY(launch_bglat_entry(tab_bwd, a.vec, a.prod, nullptr, a.n_words, a.Kp, a.n_alive, argmin, s));
      }
      HIP_TRY(emit.launch(launch_bglat_emit, a, c, g, s));
    }
    ci++;
    return SR_OK;
  }
};

int sr_bigram_word_lattice_corpus(sr_model* m, sr_corpus* c, sr_bigram* b, int gmm_kernel, double lattice_beam, uint64_t cap,
                                  uint64_t* out_arc_off, double* out_best, uint32_t* out_word, uint32_t* out_hist, uint32_t* out_pred,
                                  uint32_t* out_first, uint32_t* out_last, double* out_fwd, double* out_bwd, double* out_am) {
  return guarded(__func__, [&]() -> int {
  int rc = check_corpus(m, c);
  if (rc) return rc;
  if (!b || b->model != m) return fail(SR_EINVAL, "bigram search net does not belong to this model");
  if (!out_arc_off || !out_best) return fail(SR_EINVAL, "null argument");
  if (!(lattice_beam >= 0.0)) return fail(SR_EINVAL, "lattice_beam must be >= 0 (got %g)", lattice_beam);
  const bool fill = out_word || out_hist || out_pred || out_first || out_last || out_fwd || out_bwd || out_am;
  if (fill && (!out_word || !out_hist || !out_pred || !out_first || !out_last || !out_fwd || !out_bwd || !out_am))
    return fail(SR_EINVAL, "null output (pass all eight arc arrays, or none)");
  if (b->lm_min == -std::numeric_limits<float>::infinity()) return fail(SR_EINVAL, "the language model has a score of -inf");
  BgLatPass lp;
  uint64_t n = 0;
  rc = lattice_corpus(m, c, gmm_kernel, bglat_cost(c, b), 2ull * b->net.n_words, cap, fill, lp,
                      [&](uint64_t dev_cap, const std::vector<Chunk>& chunks) { return lp.setup(m, c, b, lattice_beam, dev_cap, chunks); },
                      LatticeOut{out_arc_off, out_best, out_word, out_first, out_last, out_fwd, out_bwd, out_am}, &n);
  if (rc) return rc;
  HIP_TRY(copy_arcs(out_hist, c->bglat_arc_hist, n));
  HIP_TRY(copy_arcs(out_pred, c->bglat_arc_pred, n));
  return SR_OK;
  });
}

// ---- N-best lists from either kind of lattice: sr_lattice_nbest, sr_bigram_lattice_nbest (host code on the caller's arrays) ----------
#include "nbest.cpp"

int sr_probe_fp16_accumulation(int device, int* within_model, double* worst_ratio) {
  return guarded(__func__, [&]() -> int {
  if (!within_model) return fail(SR_EINVAL, "within_model is null");
  HIP_TRY(hipSetDevice(device));
  bool ok = false, ok4 = false;
  double worst = 0.0, worst4 = 0.0;
  HIP_TRY(probe_fp16_accumulation(nullptr, 3, &ok, &worst));    // K = 96: models of dimension <= 46
  HIP_TRY(probe_fp16_accumulation(nullptr, 4, &ok4, &worst4));  // K = 128: dimension 47 .. 62 (allowed: 132)
  *within_model = (ok && ok4) ? 1 : 0;
  if (worst_ratio) *worst_ratio = std::max(worst, worst4 * (87.0 / 132.0));  // on the K = 96 scale
  return SR_OK;
  });
}

int sr_probe_fp16_denormals(int device, int* preserved) {
  return guarded(__func__, [&]() -> int {
  if (!preserved) return fail(SR_EINVAL, "preserved is null");
  HIP_TRY(hipSetDevice(device));
  bool ok = false;
  HIP_TRY(probe_fp16_denormals(nullptr, &ok));
  *preserved = ok ? 1 : 0;
  return SR_OK;
  });
}

// ---- streaming recognition: sr_stream_*, sr_bigram_stream_*, sr_commit_points ------------------------------------------------------
#include "stream_api.cpp"

int sr_profile_enable(sr_model* m, int on) {
  return guarded(__func__, [&]() -> int {
  if (!m) return fail(SR_EINVAL, "null model handle");
  m->profiling = on != 0;
  return SR_OK;
  });
}

int sr_profile_reset(sr_model* m) {
  return guarded(__func__, [&]() -> int {
  int rc = check_model(m);
  if (rc) return rc;
  HIP_TRY(hipDeviceSynchronize());
  for (auto& ep : m->events) { (void)hipEventDestroy(ep.a); (void)hipEventDestroy(ep.b); }
  m->events.clear();
  m->prof = sr_profile{};
  HIP_TRY(m->pf_counter.ensure(1));
  HIP_TRY(hipMemset(m->pf_counter.p, 0, sizeof(unsigned long long)));
  return SR_OK;
  });
}

int sr_profile_read(sr_model* m, sr_profile* out) {
  return guarded(__func__, [&]() -> int {
  int rc = check_model(m);
  if (rc) return rc;
  if (!out) return fail(SR_EINVAL, "out is null");
  HIP_TRY(hipDeviceSynchronize());
  for (auto& ep : m->events) {
    float ms = 0.f;
    HIP_TRY(hipEventElapsedTime(&ms, ep.a, ep.b));
    if (ep.kind == 0) { m->prof.gmm_ms += ms; m->prof.gmm_launches++; }
    else if (ep.kind == 1) { m->prof.search_ms += ms; m->prof.search_launches++; }
    else if (ep.kind == 2) m->prof.prefilter_ms += ms;
    else m->prof.refine_ms += ms;
    (void)hipEventDestroy(ep.a);
    (void)hipEventDestroy(ep.b);
  }
  m->events.clear();
  if (m->pf_counter.p) {
    unsigned long long n = 0;
    HIP_TRY(hipMemcpy(&n, m->pf_counter.p, sizeof(n), hipMemcpyDeviceToHost));
    m->prof.refined_densities = n;
  }
  *out = m->prof;
  return SR_OK;
  });
}
