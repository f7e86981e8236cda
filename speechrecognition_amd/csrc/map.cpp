// map.cpp -- the host part of MAP adaptation (Gauvain & Lee 1994, "Maximum a posteriori estimation for multivariate Gaussian mixture
// observations of Markov chains", the relevance form): the argument checks of sr_model_map_adapt, the plan that names every occupied
// mean row's entries, and the update of the mixture weights.  Host code, no device; the means themselves are map_stats.hip's.
//
// One speaker's entries (dens strictly ascending, occ > 0, x [n_entries x D]) against a prior model:
//   mean row r:   O_r = sum occ, X_ri = sum x_i over the row's entries in ascending density id;  mu'_ri = (tau mu_ri + X_ri) / (tau + O_r)
//   mixture s with an entry:  n_d = tau_w exp(logw_d) + occ_d (0 without an entry), N = sum n_d in mixture order, logw'_d = log(n_d / N)
// exp and log are the host's libm, one call per density (sr_model_eliminate's rule for where the logarithm is taken); the
// multiplication and the addition of n_d are rounded one after the other (no FMA: the host units are built for baseline x86-64).
//
// Compiled as part of fmllr.cpp's translation unit (its last lines include this file), like mllr.cpp.  The file is complete by itself --
// host_util.h and the standard library -- which is how tests/cpp/map_driver.cpp builds it.
#include <cmath>
#include <cstdio>
#include <vector>

#include "host_util.h"

namespace map_host {

static int bad(const char* fmt, unsigned long long i) {
  char msg[160];
  snprintf(msg, sizeof msg, fmt, i);
  return srhost::set_error(SR_EINVAL, msg);
}

int validate(uint64_t n_dens, uint32_t dim, uint64_t n_entries, const uint32_t* dens, const double* occ, const double* x, double tau,
             int update_weights, double tau_w) {
  if (!(tau >= 0.0) || !std::isfinite(tau)) return srhost::set_error(SR_EINVAL, "sr_model_map_adapt: tau must be finite and >= 0");
  if (update_weights && (!(tau_w > 0.0) || !std::isfinite(tau_w))) return srhost::set_error(SR_EINVAL, "sr_model_map_adapt: tau_w must be finite and > 0");
  if (n_entries && (!dens || !occ || !x)) return bad("sr_model_map_adapt: null array with %llu entries", n_entries);
  for (uint64_t e = 0; e < n_entries; e++) {
    if (dens[e] >= n_dens) return bad("sr_model_map_adapt: entry %llu: density beyond the model's", e);
    if (e && dens[e] <= dens[e - 1]) return bad("sr_model_map_adapt: entry %llu: dens must be strictly ascending", e);
    if (!(occ[e] > 0.0) || !std::isfinite(occ[e])) return bad("sr_model_map_adapt: entry %llu: occ must be finite and > 0", e);
    for (uint32_t i = 0; i < dim; i++)
      if (!std::isfinite(x[e * dim + i])) return bad("sr_model_map_adapt: entry %llu: x is not finite", e);
  }
  return SR_OK;
}

void plan(uint64_t n_dens, uint32_t n_mean, const uint32_t* dens_mean, uint64_t n_entries, const uint32_t* dens, Plan* out) {
  out->row_slot.assign(n_mean, 0xFFFFFFFFu);
  out->row_off.assign(1, 0);
  out->row_ent.assign(n_entries, 0);
  out->row_rep.clear();
  // slots in the order of their first entry; counts, then offsets
  for (uint64_t e = 0; e < n_entries; e++) {
    uint32_t& slot = out->row_slot[dens_mean[dens[e]]];
    if (slot == 0xFFFFFFFFu) { slot = (uint32_t)out->row_off.size() - 1; out->row_off.push_back(0); }
    out->row_off[slot + 1]++;
  }
  const size_t slots = out->row_off.size() - 1;
  for (size_t s = 0; s < slots; s++) out->row_off[s + 1] += out->row_off[s];
  std::vector<uint32_t> fill(out->row_off.begin(), out->row_off.end() - 1);
  for (uint64_t e = 0; e < n_entries; e++) out->row_ent[fill[out->row_slot[dens_mean[dens[e]]]]++] = (uint32_t)e;  // ascending density id
  out->row_rep.assign(slots, 0xFFFFFFFFu);
  for (uint64_t d = 0; d < n_dens && slots; d++) {
    const uint32_t slot = out->row_slot[dens_mean[d]];
    if (slot != 0xFFFFFFFFu && out->row_rep[slot] == 0xFFFFFFFFu) out->row_rep[slot] = (uint32_t)d;
  }
}

void update_weights(uint32_t n_states, const uint32_t* dens_off, uint64_t n_entries, const uint32_t* dens, const double* occ, double tau_w,
                    double* logw) {
  std::vector<double> n;
  uint64_t e = 0;
  for (uint32_t s = 0; s < n_states && e < n_entries; s++) {
    const uint32_t c0 = dens_off[s], c1 = dens_off[s + 1];
    if (dens[e] >= c1) continue;  // no entry in this mixture: its weights keep their bits
    n.assign(c1 - c0, 0.0);
    double N = 0.0;
    for (uint32_t d = c0; d < c1; d++) {
      double o = 0.0;
      if (e < n_entries && dens[e] == d) o = occ[e++];
      const double w = std::exp(logw[d]);
      const double prod = tau_w * w;
      n[d - c0] = prod + o;
      N = N + n[d - c0];
    }
    for (uint32_t d = c0; d < c1; d++) logw[d] = std::log(n[d - c0] / N);
  }
}

}  // namespace map_host
