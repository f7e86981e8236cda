// model_structure.hip -- the operations that change a model's shape: sr_model_split (every density with enough observations
// becomes two, moved apart along every dimension by a fraction of its standard deviation) and sr_model_eliminate (densities with too
// few observations go), and sr_model_tables, which reads a model's per-density tables back.  They follow the schedule of the
// reference trainer (Trainer::train, Training.cpp:44-235: split / accumulate / finalize / eliminate / accumulate / finalize), not
// the bits of its MixtureModel::split / eliminate: the operations are specified in include/srgpu.h.
//
// The integer work -- which densities split or survive, dens_off, parents, tying, row renumbering -- is host code
// (structure_plan.h).  One kernel then writes the new per-density tables from the old ones where they are, in HBM, one thread per
// (density, dimension):
//   sign  0: means, inv_vars, norm are the parent's bits
//   sign -1: mean - epsilon * sqrt(1.0 / inv_var);  sign +1: mean + epsilon * sqrt(1.0 / inv_var)     (FP64, no contraction:
//            -ffp-contract=off; the device's FP64 division and square root are correctly rounded, so a host loop in this order
//            gives the same bits)
// The log weights are host work like finalize_core's (em_finalize.hip): one subtraction of M_LN2 per child, or the host's log of
// the survivors' renormalised weights.  No atomics: two identical calls give identical bits.  C x D doubles never cross the bus.
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <memory>
#include <vector>

#include "handles.h"
#include "structure_plan.h"

#pragma clang fp contract(off)

using srhost::fail;
using srhost::guarded;

namespace {

__global__ void structure_expand_kernel(const double* means, const double* ivars, const double* norm, const uint32_t* parent,
                                        const int8_t* sign, double epsilon, uint64_t n_dens, uint32_t D, double* means_o,
                                        double* ivars_o, double* norm_o) {
  const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n_dens * D) return;
  const uint64_t c = i / D;
  const uint32_t d = (uint32_t)(i % D);
  const uint64_t src = (uint64_t)parent[c] * D + d;
  const double iv = ivars[src], mu = means[src];
  const int sg = sign[c];
  ivars_o[i] = iv;
  if (d == 0) norm_o[c] = norm[parent[c]];
  if (sg == 0) { means_o[i] = mu; return; }
  const double sd = sqrt(1.0 / iv);
  const double delta = epsilon * sd;
  means_o[i] = sg > 0 ? mu + delta : mu - delta;
}

int open_model(const sr_model* m) {
  if (!m) return fail(SR_EINVAL, "null model handle");
  HIP_TRY(hipSetDevice(m->device));
  return SR_OK;
}

bool finite_nonneg(double v) { return v >= 0.0 && v < INFINITY; }  // false for NaN

// the per mean row observation weights: the caller's host array, or the ones sr_accumulate_corpus left in the corpus handle
int fetch_weights(sr_model* m, sr_corpus* c, const double* mean_w, std::vector<double>* own, const double** w) {
  if ((c != nullptr) == (mean_w != nullptr))
    return fail(SR_EINVAL, "pass the weights either as mean_w or as a corpus holding statistics, not %s", c ? "both" : "neither");
  if (mean_w) { *w = mean_w; return SR_OK; }
  if (c->model != m) return fail(SR_EINVAL, "corpus does not belong to this model");
  if (!c->acc_valid || c->acc_n_mean != m->n_mean || c->acc_n_var != m->n_var)
    return fail(SR_EINVAL, "the corpus holds no statistics of this model: call sr_accumulate_corpus first");
  own->assign(std::max(1u, m->n_mean), 0.0);
  if (m->n_mean) HIP_TRY(hipMemcpy(own->data(), c->w_mean.p, sizeof(double) * m->n_mean, hipMemcpyDeviceToHost));
  *w = own->data();
  return SR_OK;
}

int host_logw(sr_model* m, std::vector<double>* out) {
  out->assign(std::max<uint64_t>(1, m->n_dens), 0.0);
  if (m->h_logw.size() == m->n_dens) { std::copy(m->h_logw.begin(), m->h_logw.end(), out->begin()); return SR_OK; }
  if (m->n_dens) HIP_TRY(hipMemcpy(out->data(), m->logw.p, sizeof(double) * m->n_dens, hipMemcpyDeviceToHost));
  return SR_OK;
}

// the new model of a plan: shell, tying, the expansion kernel over m's device tables, the log weights from the host
int build_from_plan(sr_model* m, const srplan::Plan& plan, const std::vector<double>& logw, double epsilon, sr_model** out,
                    uint32_t* out_parent) {
  sr_model* o = nullptr;
  int rc = srhost::model_shell(m->device, m->dim, m->n_states, plan.dens_off.data(), m->max_approx ? 1 : 0, &o);
  if (rc != SR_OK) return rc;
  std::unique_ptr<sr_model, int (*)(sr_model*)> own(o, sr_model_destroy);
  const uint64_t C = plan.n_dens;
  const uint32_t D = m->dim;
  DevBuf<uint32_t> d_parent;
  DevBuf<int8_t> d_sign;
  hipError_t e;
  if ((e = o->dens_mean.upload(plan.dens_mean.data(), C)) != hipSuccess || (e = o->dens_var.upload(plan.dens_var.data(), C)) != hipSuccess ||
      (e = d_parent.upload(plan.parent.data(), C)) != hipSuccess || (e = d_sign.upload(plan.sign.data(), C)) != hipSuccess ||
      (e = o->means.ensure(C * D)) != hipSuccess || (e = o->inv_vars.ensure(C * D)) != hipSuccess ||
      (e = o->norm.ensure(C)) != hipSuccess || (e = o->logw.upload(logw.data(), C)) != hipSuccess)
    return fail(SR_EHIP, "model structure upload: %s", hipGetErrorString(e));
  o->n_mean = plan.n_mean; o->n_var = plan.n_var;
  o->h_dens_mean = plan.dens_mean;
  o->h_dens_var = plan.dens_var;
  static const bool timing = getenv("SRGPU_STRUCT_TIMING") != nullptr;  // the kernel's HIP-event time to stderr (tools/structure_time.py)
  hipEvent_t ev[2] = {nullptr, nullptr};
  if (timing) { HIP_TRY(hipEventCreate(&ev[0])); HIP_TRY(hipEventCreate(&ev[1])); HIP_TRY(hipEventRecord(ev[0], o->s_gmm)); }
  if (C) {
    const uint64_t n = C * D;
    hipLaunchKernelGGL(structure_expand_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, o->s_gmm, m->means.p, m->inv_vars.p,
                       m->norm.p, d_parent.p, d_sign.p, epsilon, C, D, o->means.p, o->inv_vars.p, o->norm.p);
    HIP_TRY(hipGetLastError());
  }
  if (timing) HIP_TRY(hipEventRecord(ev[1], o->s_gmm));
  HIP_TRY(hipStreamSynchronize(o->s_gmm));
  if (timing) {
    float ms = 0.f;
    HIP_TRY(hipEventElapsedTime(&ms, ev[0], ev[1]));
    fprintf(stderr, "[structure] expand kernel %.4f ms\n", ms);
    (void)hipEventDestroy(ev[0]); (void)hipEventDestroy(ev[1]);
  }
  if (out_parent) std::copy(plan.parent.begin(), plan.parent.end(), out_parent);
  *out = own.release();
  return SR_OK;
}

}  // namespace

extern "C" {

int sr_model_split(sr_model* m, sr_corpus* c, const double* mean_w, double min_obs, double epsilon, int pooling, sr_model** out,
                   uint32_t* out_parent) {
  return guarded(__func__, [&]() -> int {
  if (!out) return fail(SR_EINVAL, "out is null");
  *out = nullptr;
  int rc = open_model(m);
  if (rc) return rc;
  if (!finite_nonneg(min_obs)) return fail(SR_EINVAL, "min_obs must be finite and >= 0");
  if (!finite_nonneg(epsilon)) return fail(SR_EINVAL, "epsilon must be finite and >= 0");
  if (pooling < 0 || pooling > 2) return fail(SR_EINVAL, "pooling must be 0 (global), 1 (mixture) or 2 (none)");
  std::vector<double> own_w, logw_old;
  const double* w = nullptr;
  if ((rc = fetch_weights(m, c, mean_w, &own_w, &w))) return rc;
  srplan::Plan plan;
  if (!srplan::split_plan(m->n_states, m->h_dens_off.data(), m->n_mean, m->n_var, m->h_dens_mean.data(), m->h_dens_var.data(), w, min_obs,
                          pooling, &plan))
    return fail(SR_ELIMIT, "the split model would have %llu densities (max 2^31 - 1)", (unsigned long long)plan.n_dens);
  if ((rc = host_logw(m, &logw_old))) return rc;
  std::vector<double> logw(std::max<uint64_t>(1, plan.n_dens));
  for (uint64_t k = 0; k < plan.n_dens; k++) logw[k] = plan.sign[k] ? logw_old[plan.parent[k]] - M_LN2 : logw_old[plan.parent[k]];
  return build_from_plan(m, plan, logw, epsilon, out, out_parent);
  });
}

int sr_model_eliminate(sr_model* m, sr_corpus* c, const double* mean_w, double min_obs, sr_model** out, uint32_t* out_parent) {
  return guarded(__func__, [&]() -> int {
  if (!out) return fail(SR_EINVAL, "out is null");
  *out = nullptr;
  int rc = open_model(m);
  if (rc) return rc;
  if (!finite_nonneg(min_obs)) return fail(SR_EINVAL, "min_obs must be finite and >= 0");
  std::vector<double> own_w;
  const double* w = nullptr;
  if ((rc = fetch_weights(m, c, mean_w, &own_w, &w))) return rc;
  srplan::Plan plan;
  srplan::eliminate_plan(m->n_states, m->h_dens_off.data(), m->n_mean, m->n_var, m->h_dens_mean.data(), m->h_dens_var.data(), w, min_obs,
                         &plan);
  std::vector<double> logw(std::max<uint64_t>(1, plan.n_dens));
  for (uint32_t s = 0; s < m->n_states; s++) {  // the survivors' weights, added in mixture order
    double total = 0.0;
    for (uint32_t k = plan.dens_off[s]; k < plan.dens_off[s + 1]; k++) total += w[m->h_dens_mean[plan.parent[k]]];
    for (uint32_t k = plan.dens_off[s]; k < plan.dens_off[s + 1]; k++) logw[k] = log(w[m->h_dens_mean[plan.parent[k]]] / total);
  }
  return build_from_plan(m, plan, logw, 0.0, out, out_parent);
  });
}

int sr_model_tables(const sr_model* m, double* means, double* inv_vars, double* norm, double* logw) {
  return guarded(__func__, [&]() -> int {
  int rc = open_model(m);
  if (rc) return rc;
  const size_t C = m->n_dens, D = m->dim;
  if (C == 0) return SR_OK;
  if (means) HIP_TRY(hipMemcpy(means, m->means.p, C * D * sizeof(double), hipMemcpyDeviceToHost));
  if (inv_vars) HIP_TRY(hipMemcpy(inv_vars, m->inv_vars.p, C * D * sizeof(double), hipMemcpyDeviceToHost));
  if (norm) HIP_TRY(hipMemcpy(norm, m->norm.p, C * sizeof(double), hipMemcpyDeviceToHost));
  if (logw) HIP_TRY(hipMemcpy(logw, m->logw.p, C * sizeof(double), hipMemcpyDeviceToHost));
  return SR_OK;
  });
}

}  // extern "C"
