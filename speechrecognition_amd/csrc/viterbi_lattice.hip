// viterbi_lattice.hip -- word lattices over the recognition network: the two walks of viterbi_netfb.hip (the paths the zerogram
// decoder searches, slots = the lexicon's (word, position) pairs in DecodeNet order) in the MIN semiring, without a beam and with
// the decoder's own order of additions: ((h + wp) + tdp) + e and (h + tdp) + e (orc_decode_pruned, Recognizer.cpp:103-232).
//
//   lattice_forward_kernel   A_t(s) = the cheapest path from the start hypothesis to slot s at frame t, and beside it b_t(s) = the
//                            frame at which that path entered its current word (an entry at frame t sets t, an in-word move carries
//                            its source's, the start hypothesis has 0).  Candidates are compared on their final values in the order
//                            the decoder meets them (source slots ascending, the first of equal ones stays): the entry before the
//                            in-word moves if the best word end of the frame before -- the lowest slot among equal ones -- lies
//                            below the destination, after them otherwise; in-word from position pos - 2, pos - 1, pos.  Only the
//                            word ends leave the workgroup: fwd[t][w] = A_t(end of w), first[t][w] = b_t(end of w), E_t = their min.
//   lattice_backward_kernel  B_t(s) = the cheapest continuation from slot s after frame t to a word end at frame T - 1, rolling
//                            rows only; one value per frame leaves: Bend_t = B_t(any word end) = the min over every entry at t + 1,
//                            additions in the order ((wp + tdp) + e) + B and (tdp + e) + B; Bend_{T-1} = 0.
//   lattice_count_kernel /   per frame the arcs (word w ending at t, fwd finite) with fwd + bwd <= E_{T-1} + beam, an exclusive scan
//   lattice_write_kernel     over the launch's frames (hipcub), and the arcs compacted in (frame, word) order behind those of the
//                            launches before: word, first, last, fwd, bwd = Bend_t, cost = fwd - E_{first-1} (E_{-1} = 0).  The
//                            stage is lattice_emit.h's, shared with viterbi_bigram_lattice.hip; here its policy, LatEmit.
//
// One workgroup per utterance, slots strided over the threads, FP64.  The forward's two cost rows and two 16-bit start rows live in
// LDS (20 B per slot), the backward's two rows likewise (16 B per slot).  The min over the word ends is one block-wide reduction per
// frame of (cost, slot) pairs, the lower slot winning among equal costs: a total order, so every lane and every call get the same
// bits.  No atomics.  min and + only: +inf stays +inf and never turns into NaN (costs are never subtracted, except fwd - E of a
// reachable arc, both finite).
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "dpp_util.h"
#include "kernels.h"
#include "lattice_emit.h"

namespace srgpu {

static constexpr double kInf = __builtin_huge_val();
static constexpr int kLatThreads = 512;
static constexpr int kLatWaves = kLatThreads / 64;
static constexpr uint32_t kNoSlot = 0xFFFFFFFFu;

struct LatCosts {
  double tl, tf, ts, wp;
};
__device__ inline LatCosts lat_costs(const LatticeArgs& a) {
  return LatCosts{a.net.tdp_loop, a.net.tdp_forward, a.net.tdp_skip, a.word_penalty};
}
// penalty of a jump of j positions INTO a slot with flags f (keyed on the destination's state; silence: always forward)
__device__ inline double lat_tdp_into(uint32_t f, int j, const LatCosts& c) {
  if (f & kSlotSilState) return c.tf;
  return j == 0 ? c.tl : (j == 1 ? c.tf : c.ts);
}
__device__ inline double lat_wp(uint32_t f, const LatCosts& c) { return (f & kSlotSilWord) ? 0.0 : c.wp; }
// tdp(first state, init + 1) of an entry into the slot (position 0 or 1 of its word)
__device__ inline double lat_tinit(uint32_t f, const LatCosts& c) {
  return (f & kSlotPos0) ? c.tf : ((f & kSlotFirstSil) ? c.tf : c.ts);
}

// LDS: cost[2][P] f64, red cost[2][kLatWaves] f64, red slot[2][kLatWaves] u32, start[2][P] u16
__global__ __launch_bounds__(kLatThreads) void lattice_forward_kernel(LatticeArgs a) {
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  const uint32_t u = a.utt_first + blockIdx.x, tid = threadIdx.x;
  const uint32_t P = a.net.n_slots, W = a.net.n_words;
  const uint64_t f0 = a.frame_off[u];
  const int T = (int)(a.frame_off[u + 1] - f0);
  double* al = reinterpret_cast<double*>(smem);
  double* red_v = al + 2 * (size_t)P;
  uint32_t* red_i = reinterpret_cast<uint32_t*>(red_v + 2 * kLatWaves);
  uint16_t* st = reinterpret_cast<uint16_t*>(red_i + 2 * kLatWaves);
  const uint64_t g0 = f0 - a.group_f0;  // the utterance's first frame within the launch
  double* fwd = a.fwd + g0 * W;
  uint16_t* first = a.first + g0 * W;
  double* ends = a.ends + g0;
  const double* row0 = a.scores + (f0 - a.frame_base) * a.ld;
  const uint32_t* info = a.net.slot_info;
  const uint32_t* slot_word = a.net.slot_word;
  const LatCosts c = lat_costs(a);
  if (T == 0) {
    if (tid == 0) a.out_best[u] = kInf;
    return;
  }
  // the virtual row before frame 0 (parity 1): the start hypothesis at slot 0, cost 0, word start 0
  for (uint32_t s = tid; s < P; s += kLatThreads) {
    al[P + s] = s == 0 ? 0.0 : kInf;
    st[P + s] = 0;
  }
  double E = (info[0] & kSlotEnd) ? 0.0 : kInf;
  uint32_t Eslot = (info[0] & kSlotEnd) ? 0u : kNoSlot;
  __syncthreads();
  for (int t = 0; t < T; t++) {
    const double* prev = al + (size_t)((t + 1) & 1) * P;
    double* cur = al + (size_t)(t & 1) * P;
    const uint16_t* pst = st + (size_t)((t + 1) & 1) * P;
    uint16_t* cst = st + (size_t)(t & 1) * P;
    const double* row = row0 + (uint64_t)t * a.ld;
    double my = kInf;
    uint32_t my_slot = kNoSlot;
    for (uint32_t s = tid; s < P; s += kLatThreads) {
      const uint32_t f = info[s];
      const double e = row[f & 0xFFFFu];
      const bool entry = f & (kSlotPos0 | kSlotPos1);
      double v = kInf, xe = kInf;
      uint32_t b = (uint32_t)t;
      if (entry) {
        const double ee = (f & kSlotPos0) ? e : row[info[s - 1] & 0xFFFFu];  // position 1 emits the word's FIRST state on entry
        xe = ((E + lat_wp(f, c)) + lat_tinit(f, c)) + ee;
        if (Eslot < s) v = xe;  // the decoder meets the best word end before the slot's in-word sources
      }
      if (!entry) {
        const double x2 = (prev[s - 2] + lat_tdp_into(f, 2, c)) + e;
        if (x2 < v) { v = x2; b = pst[s - 2]; }
      }
      if (!(f & kSlotPos0)) {
        const double x1 = (prev[s - 1] + lat_tdp_into(f, 1, c)) + e;
        if (x1 < v) { v = x1; b = pst[s - 1]; }
      }
      if (!(f & kSlotEnd)) {
        const double x0 = (prev[s] + lat_tdp_into(f, 0, c)) + e;
        if (x0 < v) { v = x0; b = pst[s]; }
      }
      if (xe < v) { v = xe; b = (uint32_t)t; }  // the entry met after the in-word sources (an earlier one is not below itself)
      cur[s] = v;
      cst[s] = (uint16_t)b;
      if (f & kSlotEnd) {
        const uint32_t w = slot_word[s];
        fwd[(size_t)t * W + w] = v;
        first[(size_t)t * W + w] = (uint16_t)b;
        if (v < my) { my = v; my_slot = s; }  // (slots ascend within a thread: the first of equal costs stays)
      }
    }
#pragma unroll
    for (int k = 1; k < 64; k <<= 1) {
      const double ov = shfl_xor_f64(my, k);
      const uint32_t os = (uint32_t)__shfl_xor((int)my_slot, k);
      if (ov < my || (ov == my && os < my_slot)) { my = ov; my_slot = os; }
    }
    double* rv = red_v + (t & 1) * kLatWaves;
    uint32_t* ri = red_i + (t & 1) * kLatWaves;
    if ((tid & 63) == 0) { rv[tid >> 6] = my; ri[tid >> 6] = my_slot; }
    __syncthreads();
    E = rv[0]; Eslot = ri[0];
#pragma unroll
    for (int w = 1; w < kLatWaves; w++) {
      const double ov = rv[w];
      const uint32_t os = ri[w];
      if (ov < E || (ov == E && os < Eslot)) { E = ov; Eslot = os; }
    }
    if (!(E < kInf)) Eslot = kNoSlot;
    if (tid == 0) ends[t] = E;
  }
  if (tid == 0) a.out_best[u] = E;
}

// LDS: beta[2][P] f64, red[2][kLatWaves] f64
__global__ __launch_bounds__(kLatThreads) void lattice_backward_kernel(LatticeArgs a) {
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  const uint32_t u = a.utt_first + blockIdx.x, tid = threadIdx.x;
  const uint32_t P = a.net.n_slots;
  const uint64_t f0 = a.frame_off[u];
  const int T = (int)(a.frame_off[u + 1] - f0);
  if (T == 0) return;
  double* be = reinterpret_cast<double*>(smem);
  double* red = be + 2 * (size_t)P;
  double* bend = a.bend + (f0 - a.group_f0);
  const double* row0 = a.scores + (f0 - a.frame_base) * a.ld;
  const uint32_t* info = a.net.slot_info;
  const LatCosts c = lat_costs(a);

  // the slot's term of Bend_{t-1}: the entry into it at frame t (penalties, the entry's emission at t, B_t(s))
  auto entry_term = [&](uint32_t s, uint32_t f, double b, const double* row) -> double {
    if (!(f & (kSlotPos0 | kSlotPos1))) return kInf;
    const uint32_t fs = (f & kSlotPos0) ? f : info[s - 1];
    return ((lat_wp(f, c) + lat_tinit(f, c)) + row[fs & 0xFFFFu]) + b;
  };
  auto block_min_store = [&](double v, int t) {
#pragma unroll
    for (int k = 1; k < 64; k <<= 1) {
      const double o = shfl_xor_f64(v, k);
      v = o < v ? o : v;
    }
    if ((tid & 63) == 0) red[(t & 1) * kLatWaves + (tid >> 6)] = v;
  };
  {  // frame T - 1: B = 0 at the word ends
    double* cur = be + (size_t)((T - 1) & 1) * P;
    const double* row = row0 + (uint64_t)(T - 1) * a.ld;
    double m = kInf;
    for (uint32_t s = tid; s < P; s += kLatThreads) {
      const uint32_t f = info[s];
      const double b = (f & kSlotEnd) ? 0.0 : kInf;
      cur[s] = b;
      const double x = entry_term(s, f, b, row);
      m = x < m ? x : m;
    }
    if (tid == 0) bend[T - 1] = 0.0;
    block_min_store(m, T - 1);
    __syncthreads();
  }
  for (int t = T - 2; t >= 0; t--) {
    const double* nxt = be + (size_t)((t + 1) & 1) * P;
    double* cur = be + (size_t)(t & 1) * P;
    const double* rn = row0 + (uint64_t)(t + 1) * a.ld;  // emissions of the successors
    const double* row = row0 + (uint64_t)t * a.ld;
    double B = red[((t + 1) & 1) * kLatWaves];
#pragma unroll
    for (int w = 1; w < kLatWaves; w++) {
      const double o = red[((t + 1) & 1) * kLatWaves + w];
      B = o < B ? o : B;
    }
    if (tid == 0) bend[t] = B;
    double m = kInf;
    for (uint32_t s = tid; s < P; s += kLatThreads) {
      const uint32_t f = info[s];
      double b;
      if (f & kSlotEnd) {
        b = B;
      } else {
        const uint32_t f1 = info[s + 1];  // (s is not its word's last position: s + 1 is in the word)
        b = (lat_tdp_into(f, 0, c) + rn[f & 0xFFFFu]) + nxt[s];
        const double x1 = (lat_tdp_into(f1, 1, c) + rn[f1 & 0xFFFFu]) + nxt[s + 1];
        b = x1 < b ? x1 : b;
        if (!(f1 & kSlotEnd)) {
          const uint32_t f2 = info[s + 2];
          const double x2 = (lat_tdp_into(f2, 2, c) + rn[f2 & 0xFFFFu]) + nxt[s + 2];
          b = x2 < b ? x2 : b;
        }
      }
      cur[s] = b;
      const double x = entry_term(s, f, b, row);
      m = x < m ? x : m;
    }
    block_min_store(m, t);
    __syncthreads();
  }
}

static size_t lattice_fwd_smem(uint32_t P) { return (size_t)P * (2 * 8 + 2 * 2) + 2 * kLatWaves * (8 + 4); }
static size_t lattice_bwd_smem(uint32_t P) { return (size_t)P * 2 * 8 + 2 * kLatWaves * 8; }
// 20 B per slot and 192 B for the reduction in the 160 KiB (163 840 B) LDS of a CU
size_t lattice_max_slots() { return 8176; }

hipError_t launch_lattice_forward(const LatticeArgs& a, hipStream_t stream) {
  if (a.n_utts == 0) return hipSuccess;
  if (a.net.n_slots > lattice_max_slots()) return hipErrorInvalidValue;
  const size_t smem = lattice_fwd_smem(a.net.n_slots);
  hipError_t e = hipFuncSetAttribute((const void*)lattice_forward_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)smem);
  if (e != hipSuccess) return e;
  hipLaunchKernelGGL(lattice_forward_kernel, dim3(a.n_utts), dim3(kLatThreads), smem, stream, a);
  return hipGetLastError();
}

hipError_t launch_lattice_backward(const LatticeArgs& a, hipStream_t stream) {
  if (a.n_utts == 0) return hipSuccess;
  if (a.net.n_slots > lattice_max_slots()) return hipErrorInvalidValue;
  const size_t smem = lattice_bwd_smem(a.net.n_slots);
  hipError_t e = hipFuncSetAttribute((const void*)lattice_backward_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)smem);
  if (e != hipSuccess) return e;
  hipLaunchKernelGGL(lattice_backward_kernel, dim3(a.n_utts), dim3(kLatThreads), smem, stream, a);
  return hipGetLastError();
}

// ---- the arcs (lattice_emit.h) ----------------------------------------------------------------------------------------------
struct LatEmit {
  const LatticeArgs& a;
  __device__ uint32_t n_utts() const { return a.n_utts; }
  __device__ uint32_t slots() const { return a.net.n_words; }
  __device__ bool keep(uint64_t g, uint32_t w, double limit) const {
    const double f = a.fwd[g * a.net.n_words + w];
    const double tot = f + a.bend[g];
    return f < kInf && tot < kInf && tot <= limit;
  }
  __device__ double frame(uint64_t g) const { return a.bend[g]; }
  __device__ void write(uint64_t i, uint64_t g, uint32_t w, uint64_t uf, double bwd) const {
    const uint32_t W = a.net.n_words;
    const double f = a.fwd[g * W + w];
    const uint32_t b = a.first[g * W + w];
    a.arc_word[i] = w;
    a.arc_first[i] = b;
    a.arc_last[i] = (uint32_t)(g - uf);
    a.arc_fwd[i] = f;
    a.arc_bwd[i] = bwd;
    a.arc_cost[i] = f - (b ? a.ends[uf + b - 1] : 0.0);
  }
};

__global__ __launch_bounds__(256) void lattice_count_kernel(LatticeArgs a, uint64_t n_frames, uint64_t* cnt) {
  emit_count(LatEmit{a}, n_frames, cnt);
}
__global__ __launch_bounds__(256) void lattice_write_kernel(LatticeArgs a, uint64_t n_frames, const uint64_t* scan,
                                                            const uint64_t* arc_base, uint64_t* frame_arc, uint64_t cap) {
  emit_write(LatEmit{a}, n_frames, scan, arc_base, frame_arc, cap);
}
__global__ void lattice_advance_kernel(const uint64_t* cnt, const uint64_t* scan, uint64_t n_frames, uint64_t* arc_base) {
  emit_advance(cnt, scan, n_frames, arc_base);
}

size_t lattice_scan_temp_bytes(uint64_t n_frames) {
  size_t bytes = 0;
  (void)hipcub::DeviceScan::ExclusiveSum(nullptr, bytes, (const uint64_t*)nullptr, (uint64_t*)nullptr, (int)n_frames);
  return bytes;
}

hipError_t launch_lattice_emit(const LatticeArgs& a, uint64_t n_frames, void* scan_temp, size_t scan_temp_bytes, uint64_t* cnt,
                               uint64_t* scan, uint64_t* arc_base, uint64_t* frame_arc, uint64_t cap, hipStream_t stream) {
  return launch_emit(lattice_count_kernel, lattice_write_kernel, lattice_advance_kernel, a, a.n_utts, n_frames, scan_temp,
                     scan_temp_bytes, cnt, scan, arc_base, frame_arc, cap, stream);
}

}  // namespace srgpu
