// commit_point.h -- the nearest common ancestor of a workgroup's worth of nodes in an append-only tree, for the stable prefix of a
// streaming result (sr_stream_stable; stream_commit_kernel in viterbi_decode.hip) and for the fold alone (sr_commit_points).
//
// The tree is given by a parent lookup: node 0 is the root, the parent of node c > 0 is parent(c) < c (a search's traceback:
// tb_bkp[c], the frame before the word that ended at frame c started).  Because a parent's index is below its child's,
//
//     lca(a, b):  while (a != b) replace the larger of the two by its parent
//
// ends at the nearest common ancestor: the larger index cannot be an ancestor of the smaller, so stepping it up loses no common
// ancestor, and every step lowers it.  lca is associative and commutative (the nearest common ancestor of a set does not depend
// on how the set is split), so a workgroup folds its candidates in any order: a thread its own, a wave by xor shuffles, the
// waves through LDS.  Equal operands -- the common case: most hypotheses alive in a frame started their word at the same few
// frames -- return at once.  No atomics, and no memory beyond one word of LDS per wave.
//
// `floor` is an ancestor of every candidate (the previous commit point: a commit point never moves back),
// so no walk passes below it; a walk that does reach it with the operands still apart stops there.  The work of one fold is
// therefore bounded by the nodes above the previous commit point.  The walk takes nothing on trust (traceback.h): a parent that
// is not below its child ends the fold with kCommitCorrupt.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace srgpu {

static constexpr uint32_t kCommitNone = 0xFFFFFFFFu;     // no candidate: the fold's identity
static constexpr uint32_t kCommitCorrupt = 0xFFFFFFFEu;  // a parent not below its child: absorbing

template <class Parent>
__device__ inline uint32_t commit_lca(uint32_t a, uint32_t b, uint32_t floor, Parent parent) {
  if (a == b) return a;
  if (a == kCommitCorrupt || b == kCommitCorrupt) return kCommitCorrupt;
  if (a == kCommitNone) return b;
  if (b == kCommitNone) return a;
  while (a != b) {
    const uint32_t hi = a > b ? a : b, lo = a > b ? b : a;
    if (hi <= floor) return floor;
    const uint32_t p = parent(hi);
    if (p >= hi) return kCommitCorrupt;
    a = p; b = lo;
  }
  return a;
}

// Every thread of the workgroup (NT threads, whole waves) brings the fold of its own candidates (kCommitNone: it has none) and
// returns the workgroup's; red: NT / 64 words of LDS.  Two barriers; red may be reused after the call.
template <int NT, class Parent>
__device__ inline uint32_t commit_fold(uint32_t mine, uint32_t floor, uint32_t* red, Parent parent) {
  static_assert(NT % 64 == 0, "whole waves");
#pragma unroll
  for (int m = 1; m < 64; m <<= 1) mine = commit_lca(mine, (uint32_t)__shfl_xor((int)mine, m), floor, parent);
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = mine;
  __syncthreads();
  uint32_t all = red[0];
#pragma unroll
  for (int w = 1; w < NT / 64; w++) all = commit_lca(all, red[w], floor, parent);
  __syncthreads();
  return all;
}

}  // namespace srgpu
