// posterior_items.hip -- the step every training pass ends with (Baum-Welch, MMI and sMBR over the recognition network and over the
// bigram search network): from a trellis of per-position weights to the items (frame, mixture, weight) of the EM accumulation
// (em_accumulate.hip), and the largest of them per frame.
//
//   items_kernel          one wave per frame, lanes over the utterance's distinct mixtures (ascending): the weight of a mixture is the
//                         sum of its positions' trellis entries, kept against the floor -- count pass, device scan, write pass.  A lane
//                         sums a mixture alone, in position order; with ItemArgs::serial_limit set, a mixture of more positions than
//                         that (the bigram net's silence mixtures: W + 1 positions each) is summed by the whole wave, lane l its
//                         positions l, l + 64, .., then a butterfly over the lanes.
//   items_by_frame_kernel the same for Baum-Welch's automata of few mixtures: a thread per frame
//   items_advance_kernel  the launch's items added to the device counter
//   items_top_kernel      per frame the items of largest |weight| in AlignmentItem shape
//
// sign = +1 / -1 keeps the mixtures with sign * sum > 0 and >= floor at that weight, sign = 0 those with sum != 0 and |sum| >= floor
// at the signed sum.  Posteriors and occupancies are never negative, so their passes are sign = +1.  No atomics and a fixed summation
// order: two identical calls return identical bits.
#include <hip/hip_runtime.h>
#include <hipcub/hipcub.hpp>
#include <stdint.h>

#include "dpp_util.h"
#include "kernels.h"

namespace srgpu {

static constexpr double kInf = __builtin_huge_val();
static constexpr int kItemsSplit = 8;  // workgroups (of four waves) per utterance

// Workgroup (u, y): its waves take every (4 * kItemsSplit)-th frame of utterance u; lane l of round r owns the utterance's mixture
// 64 r + l.  WRITE = false counts the items of each frame, WRITE = true stores them at *item_base + the exclusive scan of the counts,
// a frame's items in ascending mixture order.  Pos: the width of the position lists.
template <bool WRITE, class Pos>
__global__ __launch_bounds__(256) void items_kernel(ItemArgs a, int sign) {
  const uint32_t u = a.utt_first + blockIdx.x, lane = threadIdx.x & 63;
  const uint64_t f0 = a.frame_off[u];
  const int T = (int)(a.frame_off[u + 1] - f0);
  const uint32_t ld = a.chain_off ? (uint32_t)(a.chain_off[u + 1] - a.chain_off[u]) : a.row_stride;
  const double* tr = a.trellis + (a.chain_off ? a.trellis_off[u] - a.trellis_off[a.utt_first] : (f0 - a.group_f0) * ld);
  const uint32_t j0 = a.chain_off ? a.mix_off[u] : 0u, j1 = a.chain_off ? a.mix_off[u + 1] : a.n_mix;
  const Pos* pos = sizeof(Pos) == 2 ? (const Pos*)a.slot_pos16 : (const Pos*)a.slot_pos32;
  const bool gated = a.gate && !(a.gate[u] < kInf);
  const double fl = a.floor;
  const uint32_t base = WRITE ? *a.item_base : 0u;
  for (int t = blockIdx.y * 4 + (threadIdx.x >> 6); t < T; t += 4 * kItemsSplit) {
    const double* g = tr + (size_t)t * ld;
    const uint64_t gf = f0 + (uint64_t)t - a.group_f0;  // frame within the launch
    const uint32_t o = WRITE ? base + a.group_scan[gf] : 0u;
    uint32_t n = 0;
    for (uint32_t jr = j0; jr < j1 && !gated; jr += 64) {
      const uint32_t j = jr + lane;
      const uint32_t b0 = j < j1 ? a.slot_beg[j] : 0u, b1 = j < j1 ? a.slot_beg[j + 1] : 0u;
      const bool wide = a.serial_limit && b1 - b0 > a.serial_limit;
      double p = 0.0;
      if (!wide)
        for (uint32_t i = b0; i < b1; i++) p += g[pos[i]];
      for (uint64_t todo = __ballot(wide); todo; todo &= todo - 1) {  // (wave-uniform) the round's wide mixtures, one after the other
        const int l = __ffsll((unsigned long long)todo) - 1;
        const uint32_t w0 = (uint32_t)__shfl((int)b0, l), w1 = (uint32_t)__shfl((int)b1, l);
        double q = 0.0;
        for (uint32_t i = w0 + lane; i < w1; i += 64) q += g[pos[i]];
#pragma unroll
        for (int k = 1; k < 64; k <<= 1) q += shfl_xor_f64(q, k);  // (both partners add the same two values: every lane the same bits)
        if ((int)lane == l) p = q;
      }
      if (sign < 0) p = -p;
      const double mag = sign == 0 ? fabs(p) : p;
      const bool keep = j < j1 && mag > 0.0 && mag >= fl;
      const uint64_t votes = __ballot(keep);
      if (WRITE && keep) {
        const uint32_t k = o + n + (uint32_t)__popcll(votes & ((1ull << lane) - 1));
        a.item_frame[k] = (uint32_t)(f0 + t);
        a.item_mix[k] = a.mix[j];
        a.item_w[k] = p;
      }
      n += (uint32_t)__popcll(votes);
    }
    if (lane == 0) {
      if (WRITE) a.item_off[f0 + t] = o;
      else a.group_cnt[gf] = n;
    }
  }
}

// ItemArgs::by_frame (Baum-Welch: chains, 16-bit positions, no gate, sign +1): one workgroup per utterance, one thread per frame, which
// sums every mixture of the automaton itself -- the same sums in the same order, the same items.  A transcript's automaton has a handful
// of mixtures, so a wave per frame leaves most lanes idle and takes twice as long (profiles/items_refactor.txt).
template <bool WRITE>
__global__ __launch_bounds__(256) void items_by_frame_kernel(ItemArgs a, int) {
  const uint32_t u = a.utt_first + blockIdx.x;
  const uint64_t f0 = a.frame_off[u];
  const int T = (int)(a.frame_off[u + 1] - f0);
  const uint32_t N = (uint32_t)(a.chain_off[u + 1] - a.chain_off[u]);
  const double* tr = a.trellis + (a.trellis_off[u] - a.trellis_off[a.utt_first]);
  const uint32_t j0 = a.mix_off[u], j1 = a.mix_off[u + 1];
  const double fl = a.floor;
  const uint32_t base = WRITE ? *a.item_base : 0u;
  for (int t = threadIdx.x; t < T; t += blockDim.x) {
    const double* g = tr + (size_t)t * N;
    const uint64_t gf = f0 + (uint64_t)t - a.group_f0;  // frame within the launch
    const uint32_t o = WRITE ? base + a.group_scan[gf] : 0u;
    uint32_t n = 0;
    for (uint32_t j = j0; j < j1; j++) {
      double p = 0.0;
      for (uint32_t i = a.slot_beg[j]; i < a.slot_beg[j + 1]; i++) p += g[a.slot_pos16[i]];
      if (p > 0.0 && p >= fl) {
        if (WRITE) {
          a.item_frame[o + n] = (uint32_t)(f0 + t);
          a.item_mix[o + n] = a.mix[j];
          a.item_w[o + n] = p;
        }
        n++;
      }
    }
    if (WRITE) a.item_off[f0 + t] = o;
    else a.group_cnt[gf] = n;
  }
}

// *item_base += the launch's items; item_off[first frame after the launch] = *item_base (overwritten by the next launch with
// the same value, the corpus' total after the last one)
__global__ void items_advance_kernel(ItemArgs a, uint64_t n_frames) {
  const uint32_t total = *a.item_base + a.group_scan[n_frames - 1] + a.group_cnt[n_frames - 1];
  *a.item_base = total;
  a.item_off[a.group_f0 + n_frames] = total;
}

size_t items_scan_temp_bytes(uint64_t n_frames) {
  size_t bytes = 0;
  (void)hipcub::DeviceScan::ExclusiveSum(nullptr, bytes, (const uint32_t*)nullptr, (uint32_t*)nullptr, (int)n_frames);
  return bytes;
}

hipError_t launch_items(const ItemArgs& args, int sign, uint64_t n_frames, void* scan_temp, size_t scan_temp_bytes, uint32_t* scan_out,
                        hipStream_t stream) {
  if (args.n_utts == 0 || n_frames == 0) return hipSuccess;
  const bool chain = args.chain_off != nullptr;
  if ((args.slot_pos16 != nullptr) == (args.slot_pos32 != nullptr) || (args.trellis_off != nullptr) != chain ||
      (args.mix_off != nullptr) != chain || (!chain && args.row_stride < args.n_cols) ||
      (args.by_frame && (!chain || !args.slot_pos16 || args.serial_limit || args.gate || sign != 1)))
    return hipErrorInvalidValue;
  ItemArgs a = args;
  a.group_scan = scan_out;
  const auto count = a.by_frame ? items_by_frame_kernel<false> : a.slot_pos16 ? items_kernel<false, uint16_t> : items_kernel<false, uint32_t>;
  const auto write = a.by_frame ? items_by_frame_kernel<true> : a.slot_pos16 ? items_kernel<true, uint16_t> : items_kernel<true, uint32_t>;
  const dim3 grid(a.n_utts, a.by_frame ? 1 : kItemsSplit);
  hipLaunchKernelGGL(count, grid, dim3(256), 0, stream, a, sign);
  hipError_t e = hipGetLastError();
  if (e != hipSuccess) return e;
  e = hipcub::DeviceScan::ExclusiveSum(scan_temp, scan_temp_bytes, a.group_cnt, scan_out, (int)n_frames, stream);
  if (e != hipSuccess) return e;
  hipLaunchKernelGGL(write, grid, dim3(256), 0, stream, a, sign);
  hipLaunchKernelGGL(items_advance_kernel, dim3(1), dim3(1), 0, stream, a, n_frames);
  return hipGetLastError();
}

// one thread per frame: max_items rounds of "the best item ranked after the previous pick" (|weight| descending, then id ascending)
__global__ __launch_bounds__(256) void items_top_kernel(const uint32_t* item_off, const uint16_t* item_mix, const double* item_w,
                                                        uint64_t n_frames, uint32_t K, uint16_t* out_count, uint16_t* out_state,
                                                        double* out_weight) {
  const uint64_t f = (uint64_t)blockIdx.x * 256 + threadIdx.x;
  if (f >= n_frames) return;
  const uint32_t b = item_off[f], e = item_off[f + 1];
  double pw = kInf;
  uint32_t pid = 0, r = 0;
  for (; r < K; r++) {
    double bw = -1.0, bs = 0.0;
    uint32_t bid = 0xFFFFFFFFu;
    for (uint32_t i = b; i < e; i++) {
      const double s = item_w[i], w = fabs(s);
      const uint32_t id = item_mix[i];
      if (r > 0 && !(w < pw || (w == pw && id > pid))) continue;  // ranked at or before the previous pick
      if (w > bw || (w == bw && id < bid)) { bw = w; bs = s; bid = id; }
    }
    if (bid == 0xFFFFFFFFu) break;
    out_state[f * K + r] = (uint16_t)bid;
    out_weight[f * K + r] = bs;
    pw = bw; pid = bid;
  }
  out_count[f] = (uint16_t)r;
  for (uint32_t q = r; q < K; q++) {
    out_state[f * K + q] = 0;
    out_weight[f * K + q] = 0.0;
  }
}

hipError_t launch_items_top(const uint32_t* item_off, const uint16_t* item_mix, const double* item_w, uint64_t n_frames,
                            uint32_t max_items, uint16_t* out_count, uint16_t* out_state, double* out_weight, hipStream_t stream) {
  if (n_frames == 0) return hipSuccess;
  hipLaunchKernelGGL(items_top_kernel, dim3((unsigned)((n_frames + 255) / 256)), dim3(256), 0, stream, item_off, item_mix, item_w,
                     n_frames, max_items, out_count, out_state, out_weight);
  return hipGetLastError();
}

}  // namespace srgpu
