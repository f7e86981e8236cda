// lda.cpp -- the LDA projection from the statistics of lda_stats.hip (Fisher's discriminant over spliced frames; Haeb-Umbach & Ney
// 1992, "Linear discriminant analysis for improved large vocabulary continuous speech recognition").  Host code, no device.
//
// With count_k, sum_k per class and the scatter S = sum z z^T of the kept frames, N = sum count:
//   mu_k = sum_k / count_k (count_k > 0),  mu = sum_k sum_k / N
//   W = (S - sum_k count_k mu_k mu_k^T) / N                     within-class covariance
//   B = sum_k count_k mu_k mu_k^T / N - mu mu^T                 between-class covariance
// W = L L^T (Cholesky); C = L^-1 B L^-T is symmetric, C = Q diag(lambda) Q^T with lambda descending; A = the first p columns of Q, as
// rows, times L^-1.  Then A W A^T = I_p and A B A^T = diag(lambda_0 .. lambda_p-1).  Every row's sign makes its entry of largest
// magnitude (the first of them on a tie) positive.  M = [A b], b = -A mu with remove_mean, else 0.
//
// The eigendecomposition is written out here: Householder reflections bring C to tridiagonal form T = Qt C Qt^T, implicit QR steps
// with Wilkinson's shift (Givens rotations, the bulge chased down the unreduced block) bring T to diagonal form; both are applied to
// the rows of Qt as they go, so the eigenvectors end up as Qt's rows.
//
// Compiled as part of fmllr.cpp's translation unit like mllt.cpp (see the note there); complete by itself -- host_util.h and the
// standard library.
#include <algorithm>
#include <cmath>
#include <cstring>
#include <numeric>
#include <vector>

#include "host_util.h"

namespace lda_host {

using srhost::cholesky;
using srhost::set_error;

// c (n x n, symmetric, destroyed) -> d[n] eigenvalues (unsorted), qt[n x n] the eigenvectors as rows; false: no convergence
static bool eigh(std::vector<double>& c, uint32_t n, std::vector<double>& d, std::vector<double>& qt) {
  qt.assign((size_t)n * n, 0.0);
  for (uint32_t i = 0; i < n; i++) qt[(size_t)i * n + i] = 1.0;
  std::vector<double> v(n), pv(n), wv(n), e(n, 0.0);
  // tridiagonal form: step k reflects column k's part below the subdiagonal away
  for (uint32_t k = 0; k + 2 < n; k++) {
    const uint32_t m = n - k - 1;  // v lives on indices k + 1 .. n - 1
    double tail = 0.0;
    for (uint32_t i = 1; i < m; i++) tail += c[(size_t)(k + 1 + i) * n + k] * c[(size_t)(k + 1 + i) * n + k];
    if (tail == 0.0) continue;
    const double x0 = c[(size_t)(k + 1) * n + k], norm = std::sqrt(x0 * x0 + tail), alpha = x0 > 0.0 ? -norm : norm;
    for (uint32_t i = 0; i < m; i++) v[i] = c[(size_t)(k + 1 + i) * n + k];
    v[0] -= alpha;
    double vv = 0.0;
    for (uint32_t i = 0; i < m; i++) vv += v[i] * v[i];
    const double beta = 2.0 / vv;
    // S = c[k+1.., k+1..]:  p = beta S v,  w = p - (beta v.p / 2) v,  S -= v w^T + w v^T
    double vp = 0.0;
    for (uint32_t i = 0; i < m; i++) {
      const double* row = c.data() + (size_t)(k + 1 + i) * n + (k + 1);
      double s = 0.0;
      for (uint32_t j = 0; j < m; j++) s += row[j] * v[j];
      pv[i] = beta * s;
      vp += v[i] * pv[i];
    }
    const double K = 0.5 * beta * vp;
    for (uint32_t i = 0; i < m; i++) wv[i] = pv[i] - K * v[i];
    for (uint32_t i = 0; i < m; i++) {
      double* row = c.data() + (size_t)(k + 1 + i) * n + (k + 1);
      const double vi = v[i], wi = wv[i];
      for (uint32_t j = 0; j < m; j++) row[j] -= vi * wv[j] + wi * v[j];
    }
    c[(size_t)(k + 1) * n + k] = c[(size_t)k * n + k + 1] = alpha;
    for (uint32_t i = 1; i < m; i++) c[(size_t)(k + 1 + i) * n + k] = c[(size_t)k * n + k + 1 + i] = 0.0;
    // Qt <- H Qt: rows k + 1 .. n - 1
    std::fill(pv.begin(), pv.begin() + n, 0.0);
    for (uint32_t i = 0; i < m; i++) {
      const double* row = qt.data() + (size_t)(k + 1 + i) * n;
      const double vi = v[i];
      for (uint32_t j = 0; j < n; j++) pv[j] += vi * row[j];
    }
    for (uint32_t i = 0; i < m; i++) {
      double* row = qt.data() + (size_t)(k + 1 + i) * n;
      const double bv = beta * v[i];
      for (uint32_t j = 0; j < n; j++) row[j] -= bv * pv[j];
    }
  }
  d.resize(n);
  for (uint32_t i = 0; i < n; i++) d[i] = c[(size_t)i * n + i];
  for (uint32_t i = 0; i + 1 < n; i++) e[i] = c[(size_t)(i + 1) * n + i];  // couples i and i + 1
  // implicit QR steps on the trailing unreduced block [lo, hi]
  const double eps = std::ldexp(1.0, -52);
  for (uint64_t step = 0, limit = 60ull * n + 60;; step++) {
    for (uint32_t i = 0; i + 1 < n; i++)
      if (std::fabs(e[i]) <= eps * (std::fabs(d[i]) + std::fabs(d[i + 1]))) e[i] = 0.0;
    uint32_t hi = n ? n - 1 : 0;
    while (hi > 0 && e[hi - 1] == 0.0) hi--;
    if (hi == 0) return true;
    if (step >= limit) return false;
    uint32_t lo = hi - 1;
    while (lo > 0 && e[lo - 1] != 0.0) lo--;
    const double dd = 0.5 * (d[hi - 1] - d[hi]), eh = e[hi - 1];
    const double mu = dd == 0.0 ? d[hi] - std::fabs(eh) : d[hi] - eh * eh / (dd + (dd > 0.0 ? 1.0 : -1.0) * std::hypot(dd, eh));
    double x = d[lo] - mu, z = e[lo];
    for (uint32_t k = lo; k < hi; k++) {
      // the rotation R = [c s; -s c] of the plane (k, k + 1) with R (x, z) = (r, 0):  T <- R T R^T,  Qt <- R Qt
      const double r = std::hypot(x, z);
      const double cs = r == 0.0 ? 1.0 : x / r, sn = r == 0.0 ? 0.0 : z / r;
      if (k > lo) e[k - 1] = r;
      const double a = d[k], b = e[k], g = d[k + 1];
      d[k] = cs * cs * a + 2.0 * cs * sn * b + sn * sn * g;
      d[k + 1] = sn * sn * a - 2.0 * cs * sn * b + cs * cs * g;
      e[k] = cs * sn * (g - a) + (cs * cs - sn * sn) * b;
      x = e[k];
      if (k + 1 < hi) {
        z = sn * e[k + 1];  // the bulge at (k, k + 2)
        e[k + 1] = cs * e[k + 1];
      }
      double* rk = qt.data() + (size_t)k * n;
      double* rk1 = rk + n;
      for (uint32_t j = 0; j < n; j++) {
        const double u = rk[j], w = rk1[j];
        rk[j] = cs * u + sn * w;
        rk1[j] = cs * w - sn * u;
      }
    }
  }
}

static bool all_finite(const double* p, size_t n) {
  for (size_t i = 0; i < n; i++)
    if (!std::isfinite(p[i])) return false;
  return true;
}

// 0 estimated (A [p x E], b [p], eig [E] filled), 1 too little data, 2 failed
static int estimate(uint32_t E, uint32_t n_classes, const double* count, const double* sum, const double* scatter, uint32_t p,
                    bool remove_mean, double min_count, std::vector<double>& A, std::vector<double>& bvec, std::vector<double>& eig) {
  if (!all_finite(count, n_classes) || !all_finite(sum, (size_t)n_classes * E) || !all_finite(scatter, (size_t)E * E)) return 2;
  double N = 0.0;
  uint32_t live = 0;
  for (uint32_t k = 0; k < n_classes; k++) {
    if (count[k] < 0.0) return 2;
    N += count[k];
    live += count[k] > 0.0;
  }
  if (N < min_count || live < 2) return 1;
  std::vector<double> mu(E, 0.0), muk(E), between((size_t)E * E, 0.0);
  for (uint32_t k = 0; k < n_classes; k++) {
    if (!(count[k] > 0.0)) continue;
    for (uint32_t j = 0; j < E; j++) { mu[j] += sum[(size_t)k * E + j]; muk[j] = sum[(size_t)k * E + j] / count[k]; }
    for (uint32_t j = 0; j < E; j++) {
      const double cj = count[k] * muk[j];
      for (uint32_t l = 0; l < E; l++) between[(size_t)j * E + l] += cj * muk[l];
    }
  }
  for (uint32_t j = 0; j < E; j++) mu[j] /= N;
  std::vector<double> L((size_t)E * E), C((size_t)E * E);
  for (uint32_t j = 0; j < E; j++)
    for (uint32_t l = 0; l < E; l++) {
      L[(size_t)j * E + l] = (scatter[(size_t)j * E + l] - between[(size_t)j * E + l]) / N;
      C[(size_t)j * E + l] = between[(size_t)j * E + l] / N - mu[j] * mu[l];
    }
  if (!cholesky(L, E)) return 2;  // (reads and writes the lower triangle)
  // C <- L^-1 C (a forward substitution down every column), then C <- C L^-T (the same along every row)
  for (uint32_t i = 0; i < E; i++) {
    double* ci = C.data() + (size_t)i * E;
    for (uint32_t k = 0; k < i; k++) {
      const double f = L[(size_t)i * E + k];
      const double* ck = C.data() + (size_t)k * E;
      for (uint32_t j = 0; j < E; j++) ci[j] -= f * ck[j];
    }
    const double dinv = L[(size_t)i * E + i];
    for (uint32_t j = 0; j < E; j++) ci[j] /= dinv;
  }
  for (uint32_t i = 0; i < E; i++) {
    double* ci = C.data() + (size_t)i * E;
    for (uint32_t j = 0; j < E; j++) {
      double s = ci[j];
      for (uint32_t k = 0; k < j; k++) s -= ci[k] * L[(size_t)j * E + k];
      ci[j] = s / L[(size_t)j * E + j];
    }
  }
  for (uint32_t i = 0; i < E; i++)
    for (uint32_t j = i + 1; j < E; j++) C[(size_t)i * E + j] = C[(size_t)j * E + i] = 0.5 * (C[(size_t)i * E + j] + C[(size_t)j * E + i]);
  if (!all_finite(C.data(), C.size())) return 2;
  std::vector<double> d, qt;
  if (!eigh(C, E, d, qt) || !all_finite(d.data(), E)) return 2;
  std::vector<uint32_t> order(E);
  std::iota(order.begin(), order.end(), 0u);
  std::stable_sort(order.begin(), order.end(), [&](uint32_t a, uint32_t b) { return d[a] > d[b]; });
  eig.resize(E);
  for (uint32_t i = 0; i < E; i++) eig[i] = d[order[i]];
  A.assign((size_t)p * E, 0.0);
  bvec.assign(p, 0.0);
  for (uint32_t i = 0; i < p; i++) {
    const double* q = qt.data() + (size_t)order[i] * E;
    double* a = A.data() + (size_t)i * E;
    for (uint32_t j = E; j-- > 0;) {  // a L = q:  L^T a^T = q^T, from the last entry up
      double s = q[j];
      for (uint32_t k = j + 1; k < E; k++) s -= L[(size_t)k * E + j] * a[k];
      a[j] = s / L[(size_t)j * E + j];
    }
    uint32_t big = 0;
    for (uint32_t j = 1; j < E; j++)
      if (std::fabs(a[j]) > std::fabs(a[big])) big = j;
    if (a[big] < 0.0)
      for (uint32_t j = 0; j < E; j++) a[j] = -a[j];
    if (remove_mean) {
      double s = 0.0;
      for (uint32_t j = 0; j < E; j++) s += a[j] * mu[j];
      bvec[i] = -s;
    }
  }
  if (!all_finite(A.data(), A.size()) || !all_finite(bvec.data(), p)) return 2;
  return 0;
}

}  // namespace lda_host

extern "C" SR_API int sr_lda_estimate(uint32_t E, uint32_t n_classes, const double* count, const double* sum, const double* scatter,
                                      uint32_t p, int remove_mean, double min_count, double* M, double* out_eig, int32_t* out_status) {
  using namespace lda_host;
  return srhost::guarded(__func__, [&]() -> int {
  if (E == 0) return set_error(SR_EINVAL, "sr_lda_estimate: E is 0");
  if (p == 0 || p > E) return set_error(SR_EINVAL, "sr_lda_estimate: p must be 1 .. E");
  if (n_classes == 0) return set_error(SR_EINVAL, "sr_lda_estimate: n_classes is 0");
  if (!count || !sum || !scatter || !M || !out_status) return set_error(SR_EINVAL, "sr_lda_estimate: null argument");
  if (!(min_count >= 0.0)) return set_error(SR_EINVAL, "sr_lda_estimate: min_count must be >= 0");
  std::vector<double> A, b, eig;
  const int st = estimate(E, n_classes, count, sum, scatter, p, remove_mean != 0, min_count, A, b, eig);
  if (st == 0) {  // (otherwise M, and out_eig, stay as given)
    for (uint32_t i = 0; i < p; i++) {
      std::memcpy(M + (size_t)i * (E + 1), A.data() + (size_t)i * E, sizeof(double) * E);
      M[(size_t)i * (E + 1) + E] = b[i];
    }
    if (out_eig) std::memcpy(out_eig, eig.data(), sizeof(double) * E);
  }
  *out_status = st;
  return SR_OK;
  });
}
