// fmllr.cpp -- the fMLLR transform estimate from per-speaker statistics (Gales 1998, "Maximum likelihood linear transformations for
// HMM-based speech recognition", section 3.2: the row-by-row update of a constrained transform).  Host code, no device.
//
// For a speaker with statistics beta, k_i (row i, D + 1 long) and G_i ((D + 1) x (D + 1), symmetric positive definite), W = [A b]:
//   Q(W) = beta log|det A| - 1/2 sum_i (w_i G_i w_i^T - 2 w_i k_i^T)
// A sweep updates rows i = 0 .. D - 1 in order; with p_i = (row i of the cofactor matrix of the current A, 0):
//   w_i = (alpha p_i + k_i) G_i^-1,   alpha a root of   alpha^2 (p_i G_i^-1 p_i^T) + alpha (p_i G_i^-1 k_i^T) - beta = 0,
// the root with the larger beta log|alpha p_i G_i^-1 p_i^T + p_i G_i^-1 k_i^T| - 1/2 w_i G_i w_i^T + w_i k_i^T.  Each row update
// maximises Q over that row, so Q is nondecreasing.  The cofactor row is det(A) times column i of A^-1, both from one Gauss-Jordan
// elimination with partial pivoting of the current A.
#include <cmath>
#include <cstring>
#include <vector>

#include "host_util.h"

namespace {

using srhost::chol_solve;  // (host_util.h: shared with mllr.cpp)
using srhost::cholesky;
using srhost::invert;
using srhost::set_error;

double dot(const double* a, const double* b, uint32_t n) {
  double s = 0.0;
  for (uint32_t i = 0; i < n; i++) s += a[i] * b[i];
  return s;
}

// w G w^T for the symmetric (D+1) x (D+1) matrix G
double quad(const double* w, const double* G, uint32_t E) {
  double s = 0.0;
  for (uint32_t j = 0; j < E; j++) s += w[j] * dot(G + (size_t)j * E, w, E);
  return s;
}

// Q(W); false: A singular
bool auxiliary(uint32_t D, double beta, const double* k, const double* G, const double* W, double* q, double* logdet) {
  const uint32_t E = D + 1;
  std::vector<double> inv;
  double sg, la;
  if (!invert(W, D, inv, &sg, &la)) return false;
  double s = 0.0;
  for (uint32_t i = 0; i < D; i++) {
    const double* w = W + (size_t)i * E;
    s += quad(w, G + (size_t)i * E * E, E) - 2.0 * dot(w, k + (size_t)i * E, E);
  }
  *q = beta * la - 0.5 * s;
  *logdet = la;
  return std::isfinite(*q);
}

// one speaker: 0 estimated, 2 failed (W then holds garbage: the caller restores it)
int estimate_speaker(uint32_t D, double beta, const double* k, const double* G, uint32_t n_sweeps, double* W, double* aux, double* logdet) {
  const uint32_t E = D + 1;
  std::vector<std::vector<double>> L(D);
  for (uint32_t i = 0; i < D; i++) {
    L[i].assign(G + (size_t)i * E * E, G + (size_t)(i + 1) * E * E);
    if (!cholesky(L[i], E)) return 2;
  }
  double q = 0.0, ld = 0.0;
  if (!auxiliary(D, beta, k, G, W, &q, &ld)) return 2;
  if (aux) aux[0] = q;
  std::vector<double> inv, p(E), gp(E), gk(E), w(E), best(E);
  for (uint32_t sweep = 0; sweep < n_sweeps; sweep++) {
    for (uint32_t i = 0; i < D; i++) {
      double sg, la;
      if (!invert(W, D, inv, &sg, &la)) return 2;
      const double det = sg * std::exp(la);
      if (!std::isfinite(det) || det == 0.0) return 2;
      for (uint32_t j = 0; j < D; j++) p[j] = det * inv[(size_t)j * D + i];  // cofactor_ij = det(A) (A^-1)_ji
      p[D] = 0.0;
      const double* ki = k + (size_t)i * E;
      const double* Gi = G + (size_t)i * E * E;
      chol_solve(L[i], E, p.data(), gp.data());   // G_i^-1 p_i^T
      chol_solve(L[i], E, ki, gk.data());         // G_i^-1 k_i^T
      const double a = dot(p.data(), gp.data(), E), b = dot(p.data(), gk.data(), E);
      if (!(a > 0.0)) return 2;
      const double disc = std::sqrt(b * b + 4.0 * a * beta);
      // the two roots without cancellation: the one of b's sign side through the product of the roots, -beta / a
      const double r1 = b >= 0.0 ? (-b - disc) / (2.0 * a) : (-b + disc) / (2.0 * a);
      const double roots[2] = {r1, r1 != 0.0 ? (-beta / a) / r1 : 0.0};
      double best_f = -HUGE_VAL;
      bool any = false;
      for (double alpha : roots) {
        for (uint32_t j = 0; j < E; j++) w[j] = alpha * gp[j] + gk[j];
        const double f = beta * std::log(std::fabs(alpha * a + b)) - 0.5 * quad(w.data(), Gi, E) + dot(w.data(), ki, E);
        if (std::isfinite(f) && (!any || f > best_f)) { best_f = f; best = w; any = true; }
      }
      if (!any) return 2;
      std::memcpy(W + (size_t)i * E, best.data(), sizeof(double) * E);
    }
    if (!auxiliary(D, beta, k, G, W, &q, &ld)) return 2;
    if (aux) aux[sweep + 1] = q;
  }
  *logdet = ld;
  return 0;
}

}  // namespace

extern "C" SR_API int sr_fmllr_estimate(uint32_t dim, uint32_t n_speakers, const double* beta, const double* k, const double* G,
                                        uint32_t n_sweeps, double min_count, double* W, double* out_aux, double* out_logdet,
                                        int32_t* out_status) {
  return srhost::guarded(__func__, [&]() -> int {
  if (dim == 0) return set_error(SR_EINVAL, "sr_fmllr_estimate: dim is 0");
  if (!beta || !k || !G || !W || !out_status) return set_error(SR_EINVAL, "sr_fmllr_estimate: null argument");
  if (!(min_count >= 0.0)) return set_error(SR_EINVAL, "sr_fmllr_estimate: min_count must be >= 0");
  if (n_sweeps == 0) return set_error(SR_EINVAL, "sr_fmllr_estimate: n_sweeps is 0");
  const uint32_t D = dim, E = D + 1;
  const size_t nW = (size_t)D * E;
  std::vector<double> keep(nW), aux(n_sweeps + 1);
  for (uint32_t s = 0; s < n_speakers; s++) {
    double* Ws = W + s * nW;
    const double *ks = k + s * nW, *Gs = G + s * nW * E;
    std::memcpy(keep.data(), Ws, sizeof(double) * nW);
    double ld = NAN;
    int st = 1;
    if (beta[s] >= min_count) {
      st = estimate_speaker(D, beta[s], ks, Gs, n_sweeps, Ws, aux.data(), &ld);
      if (st) std::memcpy(Ws, keep.data(), sizeof(double) * nW);
    }
    if (st) {  // W as given: its Q (NaN where it has none) at every sweep
      double q = NAN;
      if (!auxiliary(D, beta[s], ks, Gs, Ws, &q, &ld)) { q = NAN; std::vector<double> inv; double sg; if (!invert(Ws, D, inv, &sg, &ld)) ld = NAN; }
      std::fill(aux.begin(), aux.end(), q);
    }
    out_status[s] = st;
    if (out_aux) std::memcpy(out_aux + (size_t)s * (n_sweeps + 1), aux.data(), sizeof(double) * (n_sweeps + 1));
    if (out_logdet) out_logdet[s] = ld;
  }
  return SR_OK;
  });
}

#include "mllr.cpp"  // sr_mllr_estimate: the MLLR mean transforms (see the note at its top)
#include "mllt.cpp"  // sr_mllt_estimate: the MLLT transform, likewise
#include "lda.cpp"   // sr_lda_estimate: the LDA projection, likewise
#include "map.cpp"   // the host part of sr_model_map_adapt: checks, the mean rows' plan, the weight update, likewise

// sr_vtln_choose: a speaker's warp from the warp search's costs (vtln_tables.h); host code like the estimates above
#include "vtln_tables.h"

extern "C" SR_API int sr_vtln_choose(uint32_t n_speakers, uint32_t n_warps, const double* cost, const uint64_t* frames, uint64_t min_frames,
                                     uint32_t fallback_warp, uint32_t* out_warp) {
  return srhost::guarded(__func__, [&]() -> int {
  if (n_warps == 0) return set_error(SR_EINVAL, "sr_vtln_choose: n_warps is 0");
  if (fallback_warp >= n_warps) return set_error(SR_EINVAL, "sr_vtln_choose: fallback_warp >= n_warps");
  if (n_speakers == 0) return SR_OK;
  if (!cost || !frames || !out_warp) return set_error(SR_EINVAL, "sr_vtln_choose: null argument");
  srplan::vtln_choose(n_speakers, n_warps, cost, frames, min_frames, fallback_warp, out_warp);
  return SR_OK;
  });
}
