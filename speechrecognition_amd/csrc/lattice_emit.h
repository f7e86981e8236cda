// lattice_emit.h -- the arc-emission stage both word lattices end with (viterbi_lattice.hip, viterbi_bigram_lattice.hip): per frame of
// a launch the arcs inside the beam are counted, an exclusive scan over the launch's frames (hipcub) places them, and they are
// compacted in (frame, slot) order behind the arcs of the launches before.
// What differs between the two networks is a policy type E around the launch's arguments e.a (LatticeArgs or BgLatArgs; both name
// frame_off, utt_first, group_f0, out_best, beam and arc_word alike, and the bodies read those directly; arc_word null = sizing call):
//   e.n_utts(), e.slots()   utterances of the launch; slots per frame (W, or 2W)
//   e.keep(g, x, limit)     is (slot x, frame g of the launch) an arc inside the beam?  limit = best + beam of the frame's utterance
//   e.frame(g)              a value of frame g for write(), read once before the slot loop: the zerogram's Bend_t, which inside write()
//                           is loaded again for every arc (the arc stores may alias it); the bigram network has none and returns a dummy
//   e.write(i, g, x, uf, fr)  the fields of arc i = (slot x, frame g); uf = its utterance's first frame in the launch, fr = e.frame(g)
// Each file keeps its own __global__ kernels, a line around the bodies here.  Nothing here multiplies, so the code means the same with
// -ffp-contract=off (viterbi_bigram_lattice.hip) and without (viterbi_lattice.hip); it has to stay that way.
#pragma once
#include <hip/hip_runtime.h>
#include <hipcub/hipcub.hpp>
#include <stdint.h>

namespace srgpu {

// the utterance of the launch that owns corpus frame gf: the last u with frame_off[u] <= gf
template <class E>
__device__ inline uint32_t emit_utt_of(const E& e, uint64_t gf) {
  uint32_t lo = e.a.utt_first, hi = e.a.utt_first + e.n_utts();  // frame_off[lo] <= gf < frame_off[hi]
  while (hi - lo > 1) {
    const uint32_t mid = lo + (hi - lo) / 2;
    if (e.a.frame_off[mid] <= gf) lo = mid; else hi = mid;
  }
  return lo;
}

// one wave per frame of the launch (workgroups of 256): cnt[g] = its arcs inside the beam
template <class E>
__device__ inline void emit_count(const E& e, uint64_t n_frames, uint64_t* cnt) {
  const uint64_t g = (uint64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (g >= n_frames) return;
  const uint32_t lane = threadIdx.x & 63, S = e.slots();
  const uint32_t u = emit_utt_of(e, e.a.group_f0 + g);
  const double limit = e.a.out_best[u] + e.a.beam;
  uint32_t n = 0;
  for (uint32_t x0 = 0; x0 < S; x0 += 64) {
    const uint32_t x = x0 + lane;
    const bool keep = x < S && e.keep(g, x, limit);
    n += (uint32_t)__popcll(__ballot(keep));
  }
  if (lane == 0) cnt[g] = n;
}

// one wave per frame of the launch: the frame's arcs at arc_base[0] + scan[g] ..., in slot order; frame_arc[corpus frame] = that
// position (the per-utterance offsets are read from it).  Nothing is written at or beyond cap.
template <class E>
__device__ inline void emit_write(const E& e, uint64_t n_frames, const uint64_t* scan, const uint64_t* arc_base, uint64_t* frame_arc,
                                  uint64_t cap) {
  const uint64_t g = (uint64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (g >= n_frames) return;
  const uint32_t lane = threadIdx.x & 63, S = e.slots();
  const uint64_t gf = e.a.group_f0 + g;
  const uint32_t u = emit_utt_of(e, gf);
  const uint64_t uf = e.a.frame_off[u] - e.a.group_f0;  // the utterance's first frame within the launch
  const double limit = e.a.out_best[u] + e.a.beam;
  uint64_t pos = arc_base[0] + scan[g];
  if (lane == 0) frame_arc[gf] = pos;
  if (!e.a.arc_word) return;  // the sizing call
  const auto fr = e.frame(g);
  for (uint32_t x0 = 0; x0 < S; x0 += 64) {
    const uint32_t x = x0 + lane;
    const bool keep = x < S && e.keep(g, x, limit);
    const uint64_t mask = __ballot(keep);
    if (keep) {
      const uint64_t i = pos + (uint64_t)__popcll(mask & ((1ull << lane) - 1ull));
      if (i < cap) e.write(i, g, x, uf, fr);
    }
    pos += (uint64_t)__popcll(mask);
  }
}

// arc_base[0] += the launch's arcs (one thread)
__device__ inline void emit_advance(const uint64_t* cnt, const uint64_t* scan, uint64_t n_frames, uint64_t* arc_base) {
  arc_base[0] += scan[n_frames - 1] + cnt[n_frames - 1];
}

// count, scan, write, advance of one launch (the file's three kernels) on `stream`; cnt / scan [n_frames] workspace
template <class Count, class Write, class Advance, class Args>
hipError_t launch_emit(Count count, Write write, Advance advance, const Args& a, uint32_t n_utts, uint64_t n_frames, void* scan_temp,
                       size_t scan_temp_bytes, uint64_t* cnt, uint64_t* scan, uint64_t* arc_base, uint64_t* frame_arc, uint64_t cap,
                       hipStream_t stream) {
  if (n_utts == 0 || n_frames == 0) return hipSuccess;
  const dim3 grid((unsigned)((n_frames + 3) / 4));
  hipLaunchKernelGGL(count, grid, dim3(256), 0, stream, a, n_frames, cnt);
  hipError_t e = hipGetLastError();
  if (e != hipSuccess) return e;
  e = hipcub::DeviceScan::ExclusiveSum(scan_temp, scan_temp_bytes, cnt, scan, (int)n_frames, stream);
  if (e != hipSuccess) return e;
  hipLaunchKernelGGL(write, grid, dim3(256), 0, stream, a, n_frames, scan, arc_base, frame_arc, cap);
  hipLaunchKernelGGL(advance, dim3(1), dim3(1), 0, stream, cnt, scan, n_frames, arc_base);
  return hipGetLastError();
}

}  // namespace srgpu
