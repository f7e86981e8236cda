// gather_words.hip -- the tail of a recognition call: the search leaves utterance u's words in slots of its own
// (out_words[frame_off[u] ..], out_count[u] of them); the caller wants them back to back with their offsets.  Two small launches
// behind the last search pack them into one result block, which the entry point hands in as mapped pinned host memory: the
// stores travel to the host as they are made, and the host reads the block after the one synchronisation it needs anyway.
//
//   block = GatherHeader | word_off[n_utts + 1] (uint64) | n_arrays runs of n_words 32-bit elements
//
// gather_scan_kernel (one workgroup) makes the checks the host loop used to make -- a flag raised, more words than slots -- and the
// prefix sum of the counts; gather_copy_kernel moves the elements, a group of utterances per workgroup, its output range walked in
// order so that the stores coalesce.  A count beyond its slots is reported in the header and clamped, so nothing is read past an
// utterance's slots whatever the counts say.
#include <hip/hip_runtime.h>

#include "kernels.h"

namespace srgpu {

constexpr uint32_t kScanThreads = 1024, kScanWaves = kScanThreads / 64;
constexpr uint32_t kCopyThreads = 256;
constexpr uint32_t kCopyGroup = 8;  // utterances per workgroup (a power of two: the search below halves it)

static __device__ inline uint64_t* block_off(const GatherArgs& a) { return reinterpret_cast<uint64_t*>(a.block + sizeof(GatherHeader)); }

__global__ __launch_bounds__(kScanThreads) void gather_scan_kernel(GatherArgs a) {
  __shared__ unsigned long long wave_sum[kScanWaves];
  __shared__ uint32_t first_flagged, first_over;
  const uint32_t tid = threadIdx.x, lane = tid & 63u, wave = tid >> 6;
  if (tid == 0) { first_flagged = kGatherNone; first_over = kGatherNone; }
  uint64_t* off = block_off(a);
  unsigned long long carry = 0;  // words of the tiles before this one (the same in every thread)
  uint32_t my_flagged = kGatherNone, my_over = kGatherNone, my_over_count = 0;  // this thread's first: its utterances ascend
  for (uint32_t base = 0; base < a.n_utts; base += kScanThreads) {
    const uint32_t u = base + tid;
    const bool live = u < a.n_utts;
    uint32_t n = 0;
    if (live) {
      const uint64_t slots = a.frame_off[u + 1] - a.frame_off[u] + a.extra_slots;
      n = a.count[u];
      if ((a.flags[u] & a.flag_mask) && my_flagged == kGatherNone) my_flagged = u;
      if (n > slots) {
        if (my_over == kGatherNone) { my_over = u; my_over_count = n; }
        n = (uint32_t)slots;
      }
    }
    unsigned long long x = n;  // inclusive scan: inside the wave by shuffles, across the waves through wave_sum
    for (uint32_t d = 1; d < 64; d <<= 1) {
      const unsigned long long y = __shfl_up(x, d, 64);
      if (lane >= d) x += y;
    }
    if (lane == 63) wave_sum[wave] = x;
    __syncthreads();
    unsigned long long before = 0, tile = 0;
    for (uint32_t w = 0; w < kScanWaves; w++) {
      const unsigned long long s = wave_sum[w];
      if (w < wave) before += s;
      tile += s;
    }
    __syncthreads();  // (the next tile writes wave_sum again)
    if (live) {
      const uint64_t end = carry + before + x;
      a.dev_off[u + 1] = end;
      off[u + 1] = end;
    }
    carry += tile;
  }
  __syncthreads();  // (first_* are set, also when there was no tile)
  if (my_flagged != kGatherNone) atomicMin(&first_flagged, my_flagged);
  if (my_over != kGatherNone) atomicMin(&first_over, my_over);
  __syncthreads();
  GatherHeader* h = reinterpret_cast<GatherHeader*>(a.block);
  if (my_over != kGatherNone && my_over == first_over) h->over_count = my_over_count;
  if (tid == 0) {
    h->n_words = carry;
    h->first_flagged = first_flagged;
    h->first_over = first_over;
    if (first_over == kGatherNone) h->over_count = 0;
    a.dev_off[0] = 0;
    off[0] = 0;
  }
}

template <int N>
__global__ __launch_bounds__(kCopyThreads) void gather_copy_kernel(GatherArgs a) {
  __shared__ uint64_t s_off[kCopyGroup + 1], s_src[kCopyGroup];
  const uint32_t tid = threadIdx.x;
  const uint32_t u0 = blockIdx.x * kCopyGroup, nu = min(kCopyGroup, a.n_utts - u0);
  if (tid <= nu) s_off[tid] = a.dev_off[u0 + tid];
  if (tid < nu) s_src[tid] = a.frame_off[u0 + tid] + (uint64_t)(u0 + tid) * a.extra_slots;
  __syncthreads();
  const uint64_t total = a.dev_off[a.n_utts];
  uint32_t* dst = reinterpret_cast<uint32_t*>(block_off(a) + a.n_utts + 1);
  const uint64_t hi = s_off[nu];
  for (uint64_t j = s_off[0] + tid; j < hi; j += kCopyThreads) {
    // the utterance that output element j belongs to: the last one of the group that starts at or before j (so one without
    // words, whose start is its successor's, is never chosen)
    uint32_t i = 0;
    for (uint32_t step = kCopyGroup / 2; step; step >>= 1)
      if (i + step < nu && s_off[i + step] <= j) i += step;
    const uint64_t s = s_src[i] + (j - s_off[i]);
#pragma unroll
    for (int k = 0; k < N; k++) dst[(uint64_t)k * total + j] = a.src[k][s];
  }
}

size_t gather_block_bytes(uint32_t n_utts, uint64_t n_slots, int n_arrays) {
  return sizeof(GatherHeader) + sizeof(uint64_t) * ((size_t)n_utts + 1) + sizeof(uint32_t) * (size_t)n_slots * (size_t)n_arrays;
}

hipError_t launch_gather_words(const GatherArgs& a, int n_arrays, hipStream_t stream) {
  if (n_arrays < 1 || n_arrays > kGatherMaxArrays || !a.block || !a.dev_off) return hipErrorInvalidValue;
  hipLaunchKernelGGL(gather_scan_kernel, dim3(1), dim3(kScanThreads), 0, stream, a);
  hipError_t e = hipGetLastError();
  if (e != hipSuccess || a.n_utts == 0) return e;
  const dim3 grid((a.n_utts + kCopyGroup - 1) / kCopyGroup), block(kCopyThreads);
  switch (n_arrays) {
    case 1: hipLaunchKernelGGL(gather_copy_kernel<1>, grid, block, 0, stream, a); break;
    case 2: hipLaunchKernelGGL(gather_copy_kernel<2>, grid, block, 0, stream, a); break;
    default: hipLaunchKernelGGL(gather_copy_kernel<3>, grid, block, 0, stream, a); break;
  }
  return hipGetLastError();
}

}  // namespace srgpu
