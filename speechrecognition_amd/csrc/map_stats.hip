// map_stats.hip -- MAP adaptation of the means (Gauvain & Lee 1994, relevance form): the per-(speaker, density) sums of a set of
// (frame, density, weight) pairs, and a model's means interpolated with one speaker's sums.
//
// The pairs, their keys speaker * n_dens + density, the stable sort and the runs of equal keys are launch_mllr_runs' (mllr_stats.hip):
// run e is the "entry" e, the runs come out in ascending (speaker, density), a last run of key 0xFFFFFFFF holds the dropped pairs.
//   occ[e] = sum gamma,   x[e][i] = sum gamma * (double) x_ti        over the entry's pairs in the order they were formed
// The order of summation is the specification (include/srgpu.h): an entry's pairs are cut into segments of kSeg = 1024; within a segment
// one chain per value from 0.0, sum = sum + gamma * x (the product rounded, then the addition); the segments' partials are added in
// ascending order to a total from 0.0.  Only the additions of one chain are serial: the segments of a long entry (silence: thousands
// of frames of one density) run on different waves, which is what this file has over mllr_entry_kernel's one wave per entry.
//
//   1. map_count_kernel    per run: (segments << 32 | pairs), 0 for the dropped run and past the last run; an exclusive scan of those
//                          gives every entry's first pair (low word) and first segment (high word) at once
//   2. map_plan_kernel     the entry and segment counts, the segment list seg_ent[segment] = entry, every speaker's first entry:
//                          all on the device, the host reads back the counts and the speakers' offsets only
//   3. map_partial_kernel  one wave per segment, a lane per dimension (D > 64: lanes loop over the dimensions); an entry of one segment
//                          is written to the outputs directly (0.0 + partial = partial, and a chain from +0.0 is never -0.0)
//   4. map_reduce_kernel   an entry's partials in ascending order into the outputs
// No atomics: two identical calls return identical bits.
//
//   map_means_kernel       mu'_ri = (tau * mu_ri + X_ri) / (tau + O_r), O_r and X_ri chains from 0.0 over the row's entries in ascending
//                          density id; a row without an entry keeps the prior's bits
#include <hip/hip_runtime.h>
#include <hipcub/hipcub.hpp>
#include <stdint.h>

#include <algorithm>

#include "kernels.h"

namespace srgpu {

#pragma clang fp contract(off)

static constexpr uint32_t kSeg = 1024;  // pairs per segment: the unit of the fixed summation order

uint32_t map_seg_pairs() { return kSeg; }

__device__ static inline uint32_t map_entries(const MapArgs& a) {
  const uint32_t runs = *a.n_runs;  // > 0: there is at least one pair
  return runs - (a.run_key[runs - 1] == 0xFFFFFFFFu ? 1u : 0u);  // the dropped pairs sort behind every key
}

// cnt[e] for e = 0 .. n_pairs (the runs are at most n_pairs; the element past them closes the scan)
__global__ __launch_bounds__(256) void map_count_kernel(MapArgs a) {
  const uint64_t e = (uint64_t)blockIdx.x * 256 + threadIdx.x;
  if (e > a.n_pairs) return;
  const uint64_t len = e < map_entries(a) ? a.run_len[e] : 0u;
  a.cnt[e] = ((len + kSeg - 1) / kSeg) << 32 | len;
}

// thread e: the segments of entry e; thread s <= n_speakers: ent_off[s] = the first entry whose key is >= s * n_dens
__global__ __launch_bounds__(256) void map_plan_kernel(MapArgs a) {
  const uint64_t e = (uint64_t)blockIdx.x * 256 + threadIdx.x;
  const uint32_t n = map_entries(a);
  if (e == 0) { a.counts[0] = n; a.counts[1] = (uint32_t)(a.scan[n] >> 32); }
  if (e <= a.n_speakers) {
    const uint64_t want = e * a.n_dens;
    uint32_t lo = 0, hi = n;
    while (lo < hi) { const uint32_t mid = (lo + hi) >> 1; if (a.run_key[mid] < want) lo = mid + 1; else hi = mid; }
    a.ent_off[e] = lo;
  }
  if (e < n) {
    const uint32_t s0 = (uint32_t)(a.scan[e] >> 32), s1 = (uint32_t)(a.scan[e + 1] >> 32);
    for (uint32_t s = s0; s < s1; s++) a.seg_ent[s] = (uint32_t)e;
  }
}

// One WAVE per segment, a lane per dimension.  em_sum_kernel's batches (em_accumulate.hip): the (frame, weight) metadata of 64 pairs
// one lane each, the next batch's on its way while this one is summed, handed round through a wave-private LDS slot array (broadcast
// reads); 32 feature rows (D consecutive floats each) in flight, their products formed before the chain of additions takes them.
__global__ __launch_bounds__(256) void map_partial_kernel(MapArgs a) {
  const uint32_t D = a.dim, lane = threadIdx.x & 63u;
  const uint32_t seg = blockIdx.x * 4u + (threadIdx.x >> 6);
  constexpr int kF = 32;  // feature rows in flight
  __shared__ ulonglong2 slots[4][64];
  if (seg >= a.n_segs) return;  // wave-uniform
  ulonglong2* slot = slots[threadIdx.x >> 6];  // wave-private: (feature row offset, weight) of the batch's pairs
  const uint32_t ent = a.seg_ent[seg];
  const uint64_t sc = a.scan[ent];
  const uint32_t k = seg - (uint32_t)(sc >> 32), len = a.run_len[ent];
  const uint32_t lo = (uint32_t)sc + k * kSeg, e = lo + (len - k * kSeg < kSeg ? len - k * kSeg : kSeg);
  const bool direct = len <= kSeg;  // the entry's only segment: no partial
  double* dst = direct ? a.out_x + (uint64_t)ent * D : a.partial + (uint64_t)seg * (D + 1);
  for (uint32_t d0 = 0; d0 < D; d0 += 64) {  // (one pass for D <= 64)
    const uint32_t d = d0 + lane;
    const bool act = d < D;
    const float* col = a.feats + (act ? d : 0u);
    double sum = 0.0, w = 0.0;
    auto meta = [&](uint32_t i, double& pw, uint32_t& fr) {  // this lane's pair of the batch at i
      const uint32_t pr = a.pairs_sorted[(i + lane < e) ? i + lane : e - 1];
      pw = a.pair_w[pr];
      fr = a.pair_frame[pr];
    };
    double pw = 0.0, pw_n = 0.0;
    uint32_t fr = 0, fr_n = 0;
    meta(lo, pw, fr);  // (a segment holds at least one pair)
    for (uint32_t i = lo; i < e; i += 64) {
      const uint32_t n = (e - i < 64u) ? e - i : 64u;
      if (i + 64 < e) meta(i + 64, pw_n, fr_n);
      // (wave-scope release / acquire around the exchange, as in em_sum_kernel: one lane writes a slot, all read it, the next batch
      // overwrites it)
      __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
      slot[lane] = make_ulonglong2((unsigned long long)fr * D, (unsigned long long)__double_as_longlong(pw));
      __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
      __builtin_amdgcn_wave_barrier();
      __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
      for (uint32_t j0 = 0; j0 < n; j0 += kF) {  // wave-uniform
        double yy[kF];
#pragma unroll
        for (int j = 0; j < kF; j++) yy[j] = (double)col[slot[(j0 + j < n) ? j0 + j : j0].x];
#pragma unroll
        for (int j = 0; j < kF; j++) yy[j] = __longlong_as_double((long long)slot[(j0 + j < n) ? j0 + j : j0].y) * yy[j];
#pragma unroll
        for (int j = 0; j < kF; j++) {
          if (j0 + j < n) {  // wave-uniform
            sum = sum + yy[j];
            w = w + __longlong_as_double((long long)slot[j0 + j].y);
          }
        }
      }
      pw = pw_n; fr = fr_n;
    }
    if (act) dst[d] = sum;
    if (d0 == 0 && lane == 0) {
      if (direct) a.out_occ[ent] = w; else dst[D] = w;
    }
  }
  if (k == 0 && lane == 0) {
    const uint32_t key = a.run_key[ent];
    a.out_dens[ent] = key - (key / a.n_dens) * a.n_dens;
  }
}

// thread (entry, column i <= D; column D is occ): the partials of an entry of more than one segment, ascending, onto 0.0
__global__ __launch_bounds__(256) void map_reduce_kernel(MapArgs a) {
  const uint32_t E = a.dim + 1;
  const uint64_t idx = (uint64_t)blockIdx.x * 256 + threadIdx.x, ent = idx / E;
  const uint32_t i = (uint32_t)(idx - ent * E);
  if (ent >= a.n_entries) return;
  const uint32_t s0 = (uint32_t)(a.scan[ent] >> 32), s1 = (uint32_t)(a.scan[ent + 1] >> 32);
  if (s1 - s0 < 2) return;  // written by its segment
  double total = 0.0;
  for (uint32_t s = s0; s < s1; s++) total = total + a.partial[(uint64_t)s * E + i];
  if (i < a.dim) a.out_x[ent * a.dim + i] = total; else a.out_occ[ent] = total;
}

size_t map_temp_bytes(uint64_t n_pairs) {
  size_t scan = 0;
  (void)hipcub::DeviceScan::ExclusiveSum(nullptr, scan, (const unsigned long long*)nullptr, (unsigned long long*)nullptr, (int)(n_pairs + 1));
  return std::max(scan, mllr_temp_bytes(n_pairs));
}

hipError_t launch_map_plan(const MapArgs& a, hipStream_t stream) {
  const uint64_t n = std::max<uint64_t>(a.n_pairs, a.n_speakers) + 1;
  hipLaunchKernelGGL(map_count_kernel, dim3((unsigned)((a.n_pairs + 256) / 256)), dim3(256), 0, stream, a);
  hipError_t e = hipGetLastError();
  if (e != hipSuccess) return e;
  size_t bytes = a.temp_bytes;
  e = hipcub::DeviceScan::ExclusiveSum(a.temp, bytes, (const unsigned long long*)a.cnt, (unsigned long long*)a.scan, (int)(a.n_pairs + 1), stream);
  if (e != hipSuccess) return e;
  hipLaunchKernelGGL(map_plan_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, stream, a);
  return hipGetLastError();
}

hipError_t launch_map_sums(const MapArgs& a, hipStream_t stream) {
  if (a.n_segs == 0) return hipSuccess;
  hipLaunchKernelGGL(map_partial_kernel, dim3((a.n_segs + 3) / 4), dim3(256), 0, stream, a);
  if (a.n_segs > a.n_entries)  // some entry has more than one segment
    hipLaunchKernelGGL(map_reduce_kernel, dim3((unsigned)(((uint64_t)a.n_entries * (a.dim + 1) + 255) / 256)), dim3(256), 0, stream, a);
  return hipGetLastError();
}

// thread (density d, dimension i)
__global__ __launch_bounds__(256) void map_means_kernel(MapMeansArgs a) {
  const uint64_t idx = (uint64_t)blockIdx.x * 256 + threadIdx.x, d = idx / a.dim;
  const uint32_t i = (uint32_t)(idx - d * a.dim);
  if (d >= a.n_dens) return;
  const uint32_t slot = a.row_slot[a.dens_mean[d]];
  if (slot == 0xFFFFFFFFu) { a.out[idx] = a.means[idx]; return; }
  double O = 0.0, X = 0.0;
  for (uint32_t q = a.row_off[slot]; q < a.row_off[slot + 1]; q++) {
    const uint32_t ent = a.row_ent[q];
    O = O + a.occ[ent];
    X = X + a.x[(uint64_t)ent * a.dim + i];
  }
  // every density of the row reads the prior mean of the row's lowest density: the same bits for all of them
  a.out[idx] = (a.tau * a.means[(uint64_t)a.row_rep[slot] * a.dim + i] + X) / (a.tau + O);
}

hipError_t launch_map_means(const MapMeansArgs& a, hipStream_t stream) {
  if (a.n_dens == 0) return hipSuccess;
  hipLaunchKernelGGL(map_means_kernel, dim3((unsigned)((a.n_dens * a.dim + 255) / 256)), dim3(256), 0, stream, a);
  return hipGetLastError();
}

}  // namespace srgpu
