// host_util.h -- small host-side helpers shared by the C-ABI translation units.
#pragma once
#include <stdint.h>

#include <algorithm>
#include <cmath>
#include <exception>
#include <mutex>
#include <new>
#include <stdexcept>
#include <string>
#include <system_error>
#include <thread>
#include <vector>

#include "../../include/srgpu.h"

#define SRHOST_POOL_GLOBAL 0   // MixtureModel::GLOBAL_POOLING  (sietill/Mixtures.hpp:20-24)
#define SRHOST_POOL_MIXTURE 1  // MixtureModel::MIXTURE_POOLING
#define SRHOST_POOL_NONE 2     // MixtureModel::NO_POOLING

namespace srhost {

// finalised tables, one row per density in mixture order (what sr_model_create consumes)
struct MixsetTables {
  uint32_t dim = 0;
  std::vector<uint32_t> dens_off;
  std::vector<double> means, inv_vars, norm, logw;
  std::vector<uint32_t> dens_mean, dens_var;  // accumulator rows (MixtureDensity{mean_idx, var_idx}) per density
  uint32_t n_mean = 0, n_var = 0;
};

// returns nullptr on success or the reference's error text (sietill/Mixtures.cpp:753-825)
const char* load_mixset(const char* path, uint32_t dim, int pooling, MixsetTables* out);

// stores the message for sr_last_error() and returns `code`
int set_error(int code, const char* msg);

// Exception barrier of the C ABI (include/srgpu.h: "No exceptions cross this boundary"): every extern "C" entry runs its
// body through this, so that a failed host allocation (std::bad_alloc from new / std::vector), an over-long container
// (std::length_error), a refused std::thread (std::system_error) or anything else becomes an SR_E* code plus
// sr_last_error() text instead of std::terminate -> SIGABRT in the caller's process.
template <typename F>
int guarded(const char* entry, F&& body) noexcept {
  try {
    return body();
  } catch (const std::bad_alloc&) {
    return set_error(SR_ENOMEM, (std::string(entry) + ": out of host memory").c_str());
  } catch (const std::length_error& e) {
    return set_error(SR_ELIMIT, (std::string(entry) + ": size too large for a host container (" + e.what() + ")").c_str());
  } catch (const std::exception& e) {
    return set_error(SR_EINTERNAL, (std::string(entry) + ": unexpected exception: " + e.what()).c_str());
  } catch (...) {
    return set_error(SR_EINTERNAL, (std::string(entry) + ": unexpected exception").c_str());
  }
}

// in-place Cholesky factor (lower) of the n x n matrix g; false: not positive definite  (fmllr.cpp, mllr.cpp)
inline bool cholesky(std::vector<double>& g, uint32_t n) {
  for (uint32_t j = 0; j < n; j++) {
    double d = g[(size_t)j * n + j];
    for (uint32_t k = 0; k < j; k++) d -= g[(size_t)j * n + k] * g[(size_t)j * n + k];
    if (!(d > 0.0) || !std::isfinite(d)) return false;
    d = std::sqrt(d);
    g[(size_t)j * n + j] = d;
    for (uint32_t i = j + 1; i < n; i++) {
      double s = g[(size_t)i * n + j];
      for (uint32_t k = 0; k < j; k++) s -= g[(size_t)i * n + k] * g[(size_t)j * n + k];
      g[(size_t)i * n + j] = s / d;
    }
  }
  return true;
}

// x = G^-1 b from the factor l (G = l l^T)
inline void chol_solve(const std::vector<double>& l, uint32_t n, const double* b, double* x) {
  for (uint32_t i = 0; i < n; i++) {
    double s = b[i];
    for (uint32_t k = 0; k < i; k++) s -= l[(size_t)i * n + k] * x[k];
    x[i] = s / l[(size_t)i * n + i];
  }
  for (uint32_t i = n; i-- > 0;) {
    double s = x[i];
    for (uint32_t k = i + 1; k < n; k++) s -= l[(size_t)k * n + i] * x[k];
    x[i] = s / l[(size_t)i * n + i];
  }
}

// Gauss-Jordan elimination with partial pivoting: inv = A^-1 (D x D, A = the first D columns of W's D + 1 long rows), *sign and
// *logabs of det A; false: singular  (fmllr.cpp, mllt.cpp)
inline bool invert(const double* W, uint32_t D, std::vector<double>& inv, double* sign, double* logabs) {
  const uint32_t E = D + 1;
  std::vector<double> a((size_t)D * D);
  for (uint32_t i = 0; i < D; i++)
    for (uint32_t j = 0; j < D; j++) a[(size_t)i * D + j] = W[(size_t)i * E + j];
  inv.assign((size_t)D * D, 0.0);
  for (uint32_t i = 0; i < D; i++) inv[(size_t)i * D + i] = 1.0;
  double sg = 1.0, la = 0.0;
  for (uint32_t c = 0; c < D; c++) {
    uint32_t piv = c;
    for (uint32_t r = c + 1; r < D; r++)
      if (std::fabs(a[(size_t)r * D + c]) > std::fabs(a[(size_t)piv * D + c])) piv = r;
    const double pv = a[(size_t)piv * D + c];
    if (pv == 0.0 || !std::isfinite(pv)) return false;
    if (piv != c) {
      for (uint32_t j = 0; j < D; j++) {
        std::swap(a[(size_t)piv * D + j], a[(size_t)c * D + j]);
        std::swap(inv[(size_t)piv * D + j], inv[(size_t)c * D + j]);
      }
      sg = -sg;
    }
    if (pv < 0.0) sg = -sg;
    la += std::log(std::fabs(pv));
    for (uint32_t j = 0; j < D; j++) { a[(size_t)c * D + j] /= pv; inv[(size_t)c * D + j] /= pv; }
    for (uint32_t r = 0; r < D; r++) {
      if (r == c) continue;
      const double f = a[(size_t)r * D + c];
      if (f == 0.0) continue;
      for (uint32_t j = 0; j < D; j++) { a[(size_t)r * D + j] -= f * a[(size_t)c * D + j]; inv[(size_t)r * D + j] -= f * inv[(size_t)c * D + j]; }
    }
  }
  *sign = sg;
  *logabs = la;
  return std::isfinite(la);
}

// Worker threads that cannot outlive their scope and cannot take the process down: the destructor joins (a joinable
// std::thread that is destroyed calls std::terminate -- what an exception thrown between emplace_back and join used to do),
// a worker's exception is kept and rethrown by wait() on the caller's thread (where `guarded` turns it into an SR_E* code),
// and a thread the system refuses (std::system_error) runs its work on the calling thread instead.
class ThreadGroup {
 public:
  explicit ThreadGroup(size_t expected) { pool_.reserve(expected); }  // (no reallocation while threads exist)
  ThreadGroup(const ThreadGroup&) = delete;
  ThreadGroup& operator=(const ThreadGroup&) = delete;
  ~ThreadGroup() { join_all(); }
  template <typename F>
  void run(F fn) {
    auto body = [this, fn]() mutable {
      try {
        fn();
      } catch (...) {
        std::lock_guard<std::mutex> g(mu_);
        if (!first_) first_ = std::current_exception();
      }
    };
    if (pool_.size() < pool_.capacity()) {
      try {
        pool_.emplace_back(body);
        return;
      } catch (const std::system_error&) {  // refused: below, on this thread
      }
    }
    body();
  }
  // the calling thread's own share: exceptions are kept like a worker's, so that wait() reports the first of all
  template <typename F>
  void run_here(F fn) {
    try {
      fn();
    } catch (...) {
      std::lock_guard<std::mutex> g(mu_);
      if (!first_) first_ = std::current_exception();
    }
  }
  void wait() {
    join_all();
    if (first_) { std::exception_ptr e = first_; first_ = nullptr; std::rethrow_exception(e); }
  }

 private:
  void join_all() noexcept {
    for (std::thread& t : pool_)
      if (t.joinable()) t.join();
  }
  std::vector<std::thread> pool_;
  std::mutex mu_;
  std::exception_ptr first_;
};

// fn(i0, i1) over [0, n) on up to `max_threads` (default 16) host threads; one call on the caller's thread when n is small
template <typename F>
inline void parallel_ranges(size_t n, size_t min_per_thread, F&& fn, size_t max_threads = 16) {
  const unsigned hw = std::thread::hardware_concurrency();
  size_t nt = std::min<size_t>(max_threads, hw ? hw : 1);
  if (min_per_thread) nt = std::min(nt, n / min_per_thread);
  if (nt <= 1) { fn((size_t)0, n); return; }
  ThreadGroup g(nt - 1);
  for (size_t t = 0; t + 1 < nt; t++) {
    const size_t a = n * t / nt, b = n * (t + 1) / nt;
    g.run([&fn, a, b]() { fn(a, b); });
  }
  g.run_here([&]() { fn(n * (nt - 1) / nt, n); });
  g.wait();
}

}  // namespace srhost

// The host part of sr_model_map_adapt (map.cpp, compiled within fmllr.cpp's unit; the device part is map_stats.hip)
namespace map_host {

// the occupied mean rows as CSR: what map_means_kernel walks
struct Plan {
  std::vector<uint32_t> row_slot;  // [n_mean] the row's slot, 0xFFFFFFFF: no entry
  std::vector<uint32_t> row_off;   // [slots + 1]
  std::vector<uint32_t> row_ent;   // [n_entries] a slot's entries, ascending density id
  std::vector<uint32_t> row_rep;   // [slots] the lowest density of the row
};
// SR_OK, or SR_EINVAL with the message set: the argument checks of sr_model_map_adapt that need no handle
int validate(uint64_t n_dens, uint32_t dim, uint64_t n_entries, const uint32_t* dens, const double* occ, const double* x, double tau,
             int update_weights, double tau_w);
void plan(uint64_t n_dens, uint32_t n_mean, const uint32_t* dens_mean, uint64_t n_entries, const uint32_t* dens, Plan* out);
// logw [n_dens] in/out: the mixtures with an entry get log(n_d / N), n_d = tau_w * exp(logw_d) + occ_d, N their sum in mixture order
void update_weights(uint32_t n_states, const uint32_t* dens_off, uint64_t n_entries, const uint32_t* dens, const double* occ, double tau_w,
                    double* logw);

}  // namespace map_host

// The transcripts' chains of the MMI passes (chains.cpp, compiled within srgpu_api.cpp's unit; ChainArgs and BgChainArgs of kernels.h)
namespace chain_host {

struct Chains {
  std::vector<uint64_t> off;            // [U + 1] an utterance's chain positions
  std::vector<uint32_t> info, src, dst; // per chain position
  std::vector<double> lmc;              // per chain position, the bigram network's chains alone
  uint32_t sil_len = 0;                 // positions of the silence word
};
// The recognition network: segment g of utterance u is the silence word 0 (g even) or w_{(g+1)/2} (g odd), each with the slot_info of
// its lexicon word (word w: slots word_off[w] .. word_off[w + 1]).  trans: words other than 0, utterance u's at trans_off[u] ..
void build_chains(const uint32_t* word_off, const uint32_t* slot_info, uint32_t U, const uint32_t* trans, const uint64_t* trans_off,
                  Chains* ch);
// The bigram search network: segment 0 is the silence word S = slot `sil`, segment 2 i - 1 the word w_i (slot w_i) and segment 2 i its
// silence copy c_i (slot w_i + W), each with the pos_info of its slot; lmc = scale * lmT[history * W + word] at a word's entry (+inf
// where the entry is +inf or NaN), 0 elsewhere
void build_bgchains(const uint32_t* slot_off, const uint32_t* pos_info, uint32_t W, uint32_t sil, const float* lmT, double scale, uint32_t U,
                    const uint32_t* trans, const uint64_t* trans_off, Chains* ch);

}  // namespace chain_host
