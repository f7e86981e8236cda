// structure_plan.h -- the integer side of sr_model_split / sr_model_eliminate (model_structure.hip): which densities split or
// survive, the new dens_off, the density of the old model every new density comes from, the new tying and the renumbering of the
// accumulator rows.  Host code over plain arrays, no HIP include: tests/cpp/structure_plan_driver.cpp compiles it with the host
// compiler alone and tests/structure_reference.py restates it in numpy.
//
// Split (the schedule of MixtureModel::split, not its bits): density k with mean row r = dens_mean[k] splits iff
// mean_w[r] >= min_obs (a NaN weight does not).  A mixture keeps its densities in their slots -- a density that splits becomes its
// lower child there, with the parent's (mean row, var row) -- and the upper children follow, in the order of their parents.  The
// j-th upper child, counted in mixture order over the whole model, gets mean row n_mean + j and, without pooling, var row
// n_var + j; with mixture or global pooling it shares the parent's var row.
//
// Eliminate: a density survives iff its weight is >= min_obs; a non-empty mixture that would lose every density keeps its heaviest
// one (ties: the lowest index; NaN ranks below everything; all NaN: the first).  Survivors keep their order.  Rows that no survivor
// references are dropped and the rest renumbered in ascending old index (write_mixset_file's rule, mixset.cpp).
#pragma once
#include <cstdint>
#include <vector>

namespace srplan {

constexpr int kPoolGlobal = 0, kPoolMixture = 1, kPoolNone = 2;  // SRHOST_POOL_* (host_util.h)
constexpr uint32_t kDropped = 0xFFFFFFFFu;

struct Plan {
  uint64_t n_dens = 0;                 // C'
  uint32_t n_mean = 0, n_var = 0;      // rows of the new tying
  std::vector<uint32_t> dens_off;      // [n_states + 1]
  std::vector<uint32_t> parent;        // [C'] density of the old model
  std::vector<int8_t> sign;            // [C'] -1 lower child, +1 upper child, 0 copy
  std::vector<uint32_t> dens_mean, dens_var;  // [C'] rows of the new tying
  std::vector<uint32_t> mean_map, var_map;    // eliminate: new index of every old row, kDropped where it is gone
};

inline bool splits(double w, double min_obs) { return w >= min_obs; }  // false for NaN

// false (and nothing else in *out but n_dens) when the new model would have 2^31 densities or more
inline bool split_plan(uint32_t n_states, const uint32_t* dens_off, uint32_t n_mean, uint32_t n_var, const uint32_t* dens_mean,
                       const uint32_t* dens_var, const double* mean_w, double min_obs, int pooling, Plan* out) {
  const uint64_t C = dens_off[n_states];
  uint64_t n_up = 0;
  for (uint64_t k = 0; k < C; k++) n_up += splits(mean_w[dens_mean[k]], min_obs) ? 1 : 0;
  *out = Plan();
  out->n_dens = C + n_up;
  if (out->n_dens >= (1ull << 31)) return false;
  out->n_mean = n_mean + (uint32_t)n_up;
  out->n_var = pooling == kPoolNone ? n_var + (uint32_t)n_up : n_var;
  out->dens_off.assign(1, 0u);
  out->parent.reserve(out->n_dens); out->sign.reserve(out->n_dens);
  out->dens_mean.reserve(out->n_dens); out->dens_var.reserve(out->n_dens);
  uint32_t j = 0;
  for (uint32_t s = 0; s < n_states; s++) {
    for (uint32_t k = dens_off[s]; k < dens_off[s + 1]; k++) {
      out->parent.push_back(k);
      out->sign.push_back(splits(mean_w[dens_mean[k]], min_obs) ? -1 : 0);
      out->dens_mean.push_back(dens_mean[k]);
      out->dens_var.push_back(dens_var[k]);
    }
    for (uint32_t k = dens_off[s]; k < dens_off[s + 1]; k++) {
      if (!splits(mean_w[dens_mean[k]], min_obs)) continue;
      out->parent.push_back(k);
      out->sign.push_back(1);
      out->dens_mean.push_back(n_mean + j);
      out->dens_var.push_back(pooling == kPoolNone ? n_var + j : dens_var[k]);
      j++;
    }
    out->dens_off.push_back((uint32_t)out->parent.size());
  }
  return true;
}

inline void eliminate_plan(uint32_t n_states, const uint32_t* dens_off, uint32_t n_mean, uint32_t n_var, const uint32_t* dens_mean,
                           const uint32_t* dens_var, const double* mean_w, double min_obs, Plan* out) {
  *out = Plan();
  out->dens_off.assign(1, 0u);
  out->mean_map.assign(n_mean, kDropped);
  out->var_map.assign(n_var, kDropped);
  for (uint32_t s = 0; s < n_states; s++) {
    const uint32_t k0 = dens_off[s], k1 = dens_off[s + 1];
    const size_t before = out->parent.size();
    for (uint32_t k = k0; k < k1; k++)
      if (splits(mean_w[dens_mean[k]], min_obs)) out->parent.push_back(k);
    if (out->parent.size() == before && k1 > k0) {  // the heaviest stays
      uint32_t best = k0;
      double bw = mean_w[dens_mean[k0]];
      for (uint32_t k = k0 + 1; k < k1; k++) {
        const double w = mean_w[dens_mean[k]];
        if (w > bw || (bw != bw && w == w)) { best = k; bw = w; }
      }
      out->parent.push_back(best);
    }
    out->dens_off.push_back((uint32_t)out->parent.size());
  }
  out->n_dens = out->parent.size();
  out->sign.assign(out->n_dens, 0);
  for (uint32_t k : out->parent) { out->mean_map[dens_mean[k]] = 0; out->var_map[dens_var[k]] = 0; }
  for (uint32_t r = 0; r < n_mean; r++)
    if (out->mean_map[r] != kDropped) out->mean_map[r] = out->n_mean++;
  for (uint32_t r = 0; r < n_var; r++)
    if (out->var_map[r] != kDropped) out->var_map[r] = out->n_var++;
  out->dens_mean.reserve(out->n_dens); out->dens_var.reserve(out->n_dens);
  for (uint32_t k : out->parent) {
    out->dens_mean.push_back(out->mean_map[dens_mean[k]]);
    out->dens_var.push_back(out->var_map[dens_var[k]]);
  }
}

}  // namespace srplan
