// mllt.cpp -- the MLLT / global semi-tied covariance transform from the statistics of mllt_stats.hip (Gales 1999, "Semi-tied
// covariance matrices for hidden Markov models", section III with one transform class).  Host code, no device.
//
// With beta and G_i (D x D, symmetric positive definite) per row i:
//   Q(A) = beta log|det A| - 1/2 sum_i a_i G_i a_i^T
// A sweep updates rows i = 0 .. D - 1 in order; with p_i = row i of the cofactor matrix of the current A:
//   a_i = alpha p_i G_i^-1,   alpha = +sqrt(beta / (p_i G_i^-1 p_i^T)).
// Each row update maximises Q over that row, so Q is nondecreasing.  Both roots give the same Q; the positive one makes
// det A = a_i p_i^T > 0 after every update, which fixes the result's sign.  a_i does not change when p_i is scaled by a positive
// number, so the code takes c_i = p_i / |det A| = sign(det A) (column i of A^-1) from one Gauss-Jordan elimination of the current A
// and never forms the determinant itself.
//
// Compiled as part of fmllr.cpp's translation unit like mllr.cpp (see the note there); complete by itself -- host_util.h and the
// standard library.
#include <cmath>
#include <cstring>
#include <vector>

#include "host_util.h"

namespace mllt_host {

using srhost::chol_solve;
using srhost::cholesky;
using srhost::invert;
using srhost::set_error;

// W = [A 0]: srhost::invert reads the first D columns of D + 1 long rows

// Q(W); false: A singular
static bool auxiliary(uint32_t D, double beta, const double* G, const double* W, double* q, double* logdet) {
  const uint32_t E = D + 1;
  std::vector<double> inv;
  double sg, la;
  if (!invert(W, D, inv, &sg, &la)) return false;
  double s = 0.0;
  for (uint32_t i = 0; i < D; i++) {
    const double* a = W + (size_t)i * E;
    const double* Gi = G + (size_t)i * D * D;
    for (uint32_t j = 0; j < D; j++) {
      double r = 0.0;
      for (uint32_t k = 0; k < D; k++) r += Gi[(size_t)j * D + k] * a[k];
      s += a[j] * r;
    }
  }
  *q = beta * la - 0.5 * s;
  *logdet = la;
  return std::isfinite(*q);
}

// 0 estimated, 2 failed (W then holds garbage: the caller restores it)
static int estimate(uint32_t D, double beta, const double* G, uint32_t n_sweeps, double* W, double* aux, double* logdet) {
  const uint32_t E = D + 1;
  std::vector<std::vector<double>> L(D);
  for (uint32_t i = 0; i < D; i++) {
    L[i].assign(G + (size_t)i * D * D, G + (size_t)(i + 1) * D * D);
    if (!cholesky(L[i], D)) return 2;
  }
  double q = 0.0, ld = 0.0;
  if (!auxiliary(D, beta, G, W, &q, &ld)) return 2;
  aux[0] = q;
  std::vector<double> inv, c(D), gc(D);
  for (uint32_t sweep = 0; sweep < n_sweeps; sweep++) {
    for (uint32_t i = 0; i < D; i++) {
      double sg, la;
      if (!invert(W, D, inv, &sg, &la)) return 2;
      for (uint32_t j = 0; j < D; j++) c[j] = sg * inv[(size_t)j * D + i];  // cofactor_ij = det(A) (A^-1)_ji
      chol_solve(L[i], D, c.data(), gc.data());                             // G_i^-1 c_i^T
      double cgc = 0.0;
      for (uint32_t j = 0; j < D; j++) cgc += c[j] * gc[j];
      if (!(cgc > 0.0) || !std::isfinite(cgc)) return 2;
      const double alpha = std::sqrt(beta / cgc);
      if (!std::isfinite(alpha)) return 2;
      for (uint32_t j = 0; j < D; j++) W[(size_t)i * E + j] = alpha * gc[j];
    }
    if (!auxiliary(D, beta, G, W, &q, &ld)) return 2;
    aux[sweep + 1] = q;
  }
  *logdet = ld;
  return 0;
}

}  // namespace mllt_host

extern "C" SR_API int sr_mllt_estimate(uint32_t dim, double beta, const double* G, uint32_t n_sweeps, double min_count, double* A,
                                       double* out_aux, double* out_logdet, int32_t* out_status) {
  using namespace mllt_host;
  return srhost::guarded(__func__, [&]() -> int {
  if (dim == 0) return set_error(SR_EINVAL, "sr_mllt_estimate: dim is 0");
  if (!G || !A || !out_status) return set_error(SR_EINVAL, "sr_mllt_estimate: null argument");
  if (!(min_count >= 0.0)) return set_error(SR_EINVAL, "sr_mllt_estimate: min_count must be >= 0");
  if (n_sweeps == 0) return set_error(SR_EINVAL, "sr_mllt_estimate: n_sweeps is 0");
  const uint32_t D = dim, E = D + 1;
  std::vector<double> W((size_t)D * E, 0.0), given, aux(n_sweeps + 1);
  for (uint32_t i = 0; i < D; i++) std::memcpy(W.data() + (size_t)i * E, A + (size_t)i * D, sizeof(double) * D);
  given = W;
  double ld = NAN;
  int st = 1;
  if (beta >= min_count) st = estimate(D, beta, G, n_sweeps, W.data(), aux.data(), &ld);
  if (st) {  // A as given: its Q (NaN where it has none) at every sweep
    double q = NAN;
    if (!auxiliary(D, beta, G, given.data(), &q, &ld)) { q = NAN; std::vector<double> inv; double sg; if (!invert(given.data(), D, inv, &sg, &ld)) ld = NAN; }
    std::fill(aux.begin(), aux.end(), q);
  } else {
    for (uint32_t i = 0; i < D; i++) std::memcpy(A + (size_t)i * D, W.data() + (size_t)i * E, sizeof(double) * D);
  }
  *out_status = st;
  if (out_aux) std::memcpy(out_aux, aux.data(), sizeof(double) * (n_sweeps + 1));
  if (out_logdet) *out_logdet = ld;
  return SR_OK;
  });
}
