// mllr.cpp -- the MLLR mean transforms from per-(speaker, regression class) statistics (Leggetter & Woodland 1995, "Maximum
// likelihood linear regression for speaker adaptation of continuous density hidden Markov models"; the regression-class tree of
// Gales 1996, "The generation and use of regression class trees for MLLR adaptation").  Host code, no device.
//
// For a node with statistics beta, k_i (row i, D + 1 long) and G_i ((D + 1) x (D + 1), symmetric), W = [A b]:
//   Q(W) = -1/2 sum_i (w_i G_i w_i^T - 2 w_i k_i^T),   maximised row by row at w_i = k_i G_i^-1: one Cholesky solve per row.
// The tree: nodes 0 .. n_classes - 1 are the leaves (the base classes), parent[v] > v or -1.  A node's statistics are the sum of its
// leaves', added in ascending leaf id.  A leaf takes the transform of its lowest ancestor (itself first) whose beta >= min_count
// and whose every G_i factorises.
//
// Compiled as part of fmllr.cpp's translation unit (its last line includes this file): the library's host units are listed by name
// where the host side is built under the sanitizers, and the adaptation estimates stay one unit there.  The file is complete by
// itself -- host_util.h and the standard library -- which is how tests/cpp/mllr_driver.cpp builds it.
#include <cmath>
#include <cstring>
#include <vector>

#include "host_util.h"

namespace mllr_host {

using srhost::chol_solve;
using srhost::cholesky;
using srhost::set_error;

static double dot(const double* a, const double* b, uint32_t n) {
  double s = 0.0;
  for (uint32_t i = 0; i < n; i++) s += a[i] * b[i];
  return s;
}

// Q(W) of one node
static double auxiliary(uint32_t D, const double* k, const double* G, const double* W) {
  const uint32_t E = D + 1;
  double s = 0.0;
  for (uint32_t i = 0; i < D; i++) {
    const double* w = W + (size_t)i * E;
    const double* Gi = G + (size_t)i * E * E;
    double q = 0.0;
    for (uint32_t j = 0; j < E; j++) q += w[j] * dot(Gi + (size_t)j * E, w, E);
    s += q - 2.0 * dot(w, k + (size_t)i * E, E);
  }
  return -0.5 * s;
}

// a node of one speaker: its statistics (a leaf's are the caller's), whether it qualifies and its transform
struct Node {
  int state = 0;  // 0 not looked at, 1 estimated, 2 does not qualify
  double beta = 0.0;
  const double *k = nullptr, *G = nullptr;
  std::vector<double> k_sum, G_sum, W;
};

}  // namespace mllr_host

extern "C" SR_API int sr_mllr_estimate(uint32_t dim, uint32_t n_speakers, uint32_t n_classes, uint32_t n_nodes, const int32_t* parent,
                                       const double* beta, const double* k, const double* G, double min_count, double* W,
                                       int32_t* out_node, double* out_aux) {
  using namespace mllr_host;
  return srhost::guarded(__func__, [&]() -> int {
  if (dim == 0) return set_error(SR_EINVAL, "sr_mllr_estimate: dim is 0");
  if (!parent || !beta || !k || !G || !W || !out_node) return set_error(SR_EINVAL, "sr_mllr_estimate: null argument");
  if (!(min_count >= 0.0)) return set_error(SR_EINVAL, "sr_mllr_estimate: min_count must be >= 0");
  if (n_classes == 0 || n_nodes < n_classes || n_nodes > 0x7FFFFFFFu) return set_error(SR_EINVAL, "sr_mllr_estimate: need 1 <= n_classes <= n_nodes < 2^31");
  for (uint32_t v = 0; v < n_nodes; v++) {
    if (parent[v] == -1) continue;
    // a parent comes after its children and is no leaf
    if (parent[v] < 0 || (uint32_t)parent[v] <= v || (uint32_t)parent[v] >= n_nodes || (uint32_t)parent[v] < n_classes)
      return set_error(SR_EINVAL, "sr_mllr_estimate: malformed tree (parent[v] must be -1 or an inner node > v)");
  }
  const uint32_t D = dim, E = D + 1, R = n_classes;
  const size_t nW = (size_t)D * E, nG = nW * E;
  // every inner node's leaves, ascending
  std::vector<std::vector<uint32_t>> leaves(n_nodes);
  for (uint32_t r = 0; r < R; r++)
    for (int32_t v = parent[r]; v != -1; v = parent[v]) leaves[v].push_back(r);
  std::vector<Node> nodes(n_nodes);
  std::vector<double> L, x(E);
  for (uint32_t s = 0; s < n_speakers; s++) {
    const double* beta_s = beta + (size_t)s * R;
    const double *k_s = k + (size_t)s * R * nW, *G_s = G + (size_t)s * R * nG;
    for (Node& n : nodes) n.state = 0;
    // the node's statistics and, where it qualifies, its transform
    auto look = [&](uint32_t v) {
      Node& n = nodes[v];
      if (v < R) {
        n.beta = beta_s[v]; n.k = k_s + v * nW; n.G = G_s + v * nG;
      } else {
        n.beta = 0.0;
        n.k_sum.assign(nW, 0.0); n.G_sum.assign(nG, 0.0);
        for (uint32_t r : leaves[v]) {
          n.beta += beta_s[r];
          for (size_t e = 0; e < nW; e++) n.k_sum[e] += k_s[r * nW + e];
          for (size_t e = 0; e < nG; e++) n.G_sum[e] += G_s[r * nG + e];
        }
        n.k = n.k_sum.data(); n.G = n.G_sum.data();
      }
      n.state = 2;
      if (!(n.beta >= min_count)) return;
      n.W.assign(nW, 0.0);
      for (uint32_t i = 0; i < D; i++) {
        L.assign(n.G + (size_t)i * E * E, n.G + (size_t)(i + 1) * E * E);
        if (!cholesky(L, E)) return;
        chol_solve(L, E, n.k + (size_t)i * E, x.data());
        for (uint32_t j = 0; j < E; j++) {
          if (!std::isfinite(x[j])) return;
          n.W[(size_t)i * E + j] = x[j];
        }
      }
      n.state = 1;
    };
    for (uint32_t r = 0; r < R; r++) {
      int32_t used = -1;
      for (int32_t v = (int32_t)r; v != -1; v = parent[v]) {
        if (nodes[v].state == 0) look((uint32_t)v);
        if (nodes[v].state == 1) { used = v; break; }
      }
      double* Wr = W + ((size_t)s * R + r) * nW;
      out_node[(size_t)s * R + r] = used;
      double q0 = NAN, q1 = NAN;
      if (used >= 0) {
        const Node& n = nodes[used];
        if (out_aux) { q0 = auxiliary(D, n.k, n.G, Wr); q1 = auxiliary(D, n.k, n.G, n.W.data()); }
        std::memcpy(Wr, n.W.data(), sizeof(double) * nW);
      }
      if (out_aux) { out_aux[((size_t)s * R + r) * 2] = q0; out_aux[((size_t)s * R + r) * 2 + 1] = q1; }
    }
  }
  return SR_OK;
  });
}
