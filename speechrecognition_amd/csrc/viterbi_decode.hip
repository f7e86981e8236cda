// viterbi_decode.hip -- time-synchronous beam Viterbi over whole-word linear HMMs with a zerogram
// LM, bit-compatible with Recognizer::recognizeSequence_pruned (sietill/Recognizer.cpp:103-232).
//
// One workgroup decodes one utterance.  The reference's hypothesis array (Book[word*max_pos+pos],
// Recognizer.cpp:116-117) becomes P = sum_w n_pos(w) "slots" in the same (word, position) order;
// a slot's word and position are static, so per slot only {score f64, bkp u16} live in LDS and
// each thread keeps its slots' constants in registers.  Per frame:
//
//   A  every slot gathers its candidates -- skip/forward/loop inside the word (keyed on the
//      DESTINATION state, TdpModel.cpp:19-29; word-end slots do not expand, Recognizer.cpp:131) and,
//      for positions 0 and 1, the word-boundary candidate -- and replays the reference's merge
//      (`new > target -> continue; new += am; target > new -> replace`, :143-157, :173-186) in
//      ascending source-slot order, which is the order the reference visits hypotheses in (:126).
//      The O(#word-ends x W) boundary loop (:133-158) collapses to one min over word-end slots
//      plus a broadcast: all boundary candidates of a target write identical fields and FP addition
//      of a constant is monotone, so only their minimum and the FIRST slot index attaining it (per
//      (word-penalty, tdp) class, for exact ties against in-word candidates) matter.  That shortcut
//      needs the pre-AM early-out (:143) to be inert, i.e. emission costs >= 0; a slot whose
//      candidates involve a negative emission cost replays the boundary loop sequentially instead
//      (exact, O(W), rare: flagged in out_flags bit 0).
//   B  block-wide min of the new scores (= best_score, :155,184; it includes the dead
//      position-1 slot of one-position words such as silence) and min over word-end slots.
//   C  prune `score > best + am_threshold` (:194), record traceback[t] = first minimal surviving
//      word end (:199-205), publish the word-end minimum and first-index per class for frame t+1.
//
// This file holds the GENERAL kernel: slots in reference order, every per-slot decision taken per lane, the
// sequential boundary replay inline.  Production launches run a fast kernel first (viterbi_words.hip or viterbi_fast.hip:
// same results, ~5x fewer instructions per frame) and decode_kernel only for the utterances it hands back (out_flags
// kFlagReplay: a negative emission cost was seen); decode_route, at the end of this file, picks the kernels.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <stdlib.h>

#include "commit_point.h"
#include "kernels.h"
#include "traceback.h"

namespace srgpu {

// slot_info: the kSlot* bits of kernels.h, built by build_decode_net (end of this file)
static constexpr double kInf = __builtin_huge_val();

struct Merge {  // one target hypothesis being built (Book, Recognizer.hpp:75-89; word/pos are static)
  double score;
  uint32_t bkp;
  __device__ Merge() : score(kInf), bkp(0) {}
  // Recognizer.cpp:143-157 / :173-186
  __device__ void offer(double pre_am, double am, uint32_t cand_bkp) {
    const double n = pre_am + am;
    const bool take = !(pre_am > score) && (score > n);  // `continue` on the early-out, then strict improvement
    score = take ? n : score;
    bkp = take ? cand_bkp : bkp;
  }
};

// (value, index) lexicographic minimum across the wave: every lane ends with the result
__device__ inline void wave_min_idx(double& v, uint32_t& idx) {
#pragma unroll
  for (int m = 1; m < 64; m <<= 1) {
    const int lo = __shfl_xor(__double2loint(v), m), hi = __shfl_xor(__double2hiint(v), m);
    const double ov = __hiloint2double(hi, lo);
    const uint32_t oi = __shfl_xor(idx, m);
    if (ov < v || (ov == v && oi < idx)) { v = ov; idx = oi; }
  }
}
__device__ inline double wave_min(double v) {
#pragma unroll
  for (int m = 1; m < 64; m <<= 1) {
    const int lo = __shfl_xor(__double2loint(v), m), hi = __shfl_xor(__double2hiint(v), m);
    const double ov = __hiloint2double(hi, lo);
    v = ov < v ? ov : v;
  }
  return v;
}

// Sequential replay of the word-boundary loop (Recognizer.cpp:133-158) for ONE target slot whose
// candidates involve a negative emission cost: sources in ascending slot order -- word ends of the
// words before this one, the in-word sources, then the remaining word ends.  Rare; reached only through a
// wave-uniform branch.
__device__ inline Merge replay_boundary(const uint32_t* word_end_slot, uint32_t W, const double* sc,
                                                           const uint16_t* bk, uint32_t p, bool pos1, bool has_loop,
                                                           bool in_word, double wp, double t_b, double am_b, double am,
                                                           double t_fwd, double t_loop, uint32_t bkp_new) {
  Merge mg;
  const uint32_t base = pos1 ? p - 1 : p;  // slot of position 0 of this word
  uint32_t v = 0;
  for (; v < W; v++) {
    const uint32_t e = word_end_slot[v];
    if (e >= base) break;
    const double s = sc[e];
    if (s != kInf) mg.offer((s + wp) + t_b, am_b, bkp_new);
  }
  if (in_word) {
    if (pos1) mg.offer(sc[p - 1] + t_fwd, am, bk[p - 1]);
    if (has_loop) mg.offer(sc[p] + t_loop, am, bk[p]);
  }
  for (; v < W; v++) {
    const double s = sc[word_end_slot[v]];
    if (s != kInf) mg.offer((s + wp) + t_b, am_b, bkp_new);
  }
  return mg;
}

// B: the block minimum of the frame's new scores and the first minimal word end (score, slot) from every lane's partials.  Its
// barrier also ends every read of the previous frame's hypotheses.
template <int NT>
__device__ __forceinline__ void block_minima(double my_best, double my_we, uint32_t my_we_idx, double* red_best, double* red_we,
                                             uint32_t* red_idx, double& best, double& we, uint32_t& we_idx) {
  constexpr uint32_t kWavesPerWg = NT / 64;
  const uint32_t wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  my_best = wave_min(my_best);
  wave_min_idx(my_we, my_we_idx);
  if (lane == 0) { red_best[wave] = my_best; red_we[wave] = my_we; red_idx[wave] = my_we_idx; }
  __syncthreads();
  best = red_best[0]; we = red_we[0];
  we_idx = red_idx[0];
#pragma unroll
  for (uint32_t w = 1; w < kWavesPerWg; w++) {
    const double ob = red_best[w];
    best = ob < best ? ob : best;
    const double ow = red_we[w];
    const uint32_t oi = red_idx[w];
    if (ow < we || (ow == we && oi < we_idx)) { we = ow; we_idx = oi; }
  }
}
// C: the first slot (in index order) whose boundary candidate equals the minimum's, per (word penalty, tdp) class -- for word end p
// of score v near the surviving minimum m_we, into the next frame's ef_nxt (reset in phase A)
__device__ __forceinline__ void publish_word_end(uint32_t* ef_nxt, uint32_t p, double v, double m_we, double wp_word, double tf, double ts) {
  if (v + 0.0 + tf == m_we + 0.0 + tf) atomicMin(&ef_nxt[0], p);
  if (v + 0.0 + ts == m_we + 0.0 + ts) atomicMin(&ef_nxt[1], p);
  if (v + wp_word + tf == m_we + wp_word + tf) atomicMin(&ef_nxt[2], p);
  if (v + wp_word + ts == m_we + wp_word + ts) atomicMin(&ef_nxt[3], p);
}

// Launched right after a fast kernel on the same stream (launch_decode): workgroups of unflagged utterances exit at once, flagged
// utterances are decoded again from frame 1 with the replay inline (exact, slower).  Without a fast kernel: every utterance.
template <int NT, int SPT>
__global__ __launch_bounds__(NT) void decode_kernel(DecodeArgs a) {
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  const uint32_t P = a.net.n_slots;
  const uint32_t tid = threadIdx.x;
  constexpr uint32_t PP = NT * SPT;                                // slot arrays are padded to the thread grid
  double* sc = reinterpret_cast<double*>(smem);                    // [PP] hypothesis scores
  double* am_l = sc + PP;                                          // [PP] this frame's emission cost per slot (for position-1 slots' neighbours)
  double* red_best = am_l + PP;                                    // [16]
  double* red_we = red_best + 16;                                  // [16]
  uint32_t* red_idx = reinterpret_cast<uint32_t*>(red_we + 16);    // [16]
  uint32_t* e_first = red_idx + 16;                                // [2][4] first word-end slot per class, by frame parity; [4] unused
  uint16_t* bk = reinterpret_cast<uint16_t*>(e_first + 12);         // [PP] back pointers (start frame of the word)

  const uint32_t u = a.utt_order ? a.utt_order[a.utt_first + blockIdx.x] : a.utt_first + blockIdx.x;
  if (a.only_flagged && !(a.out_flags[u] & kFlagReplay)) return;  // wave-uniform: nothing to redo for this utterance
  const uint64_t f0 = a.frame_off[u];
  const uint32_t T = (uint32_t)(a.frame_off[u + 1] - f0);
  const double* row0 = a.scores + (f0 - a.frame_base) * a.ld;
  const uint64_t tb0 = f0 + u;  // traceback[0] of this utterance
  const double tl = a.net.tdp_loop, tf = a.net.tdp_forward, ts = a.net.tdp_skip;
  const double wp_word = a.word_penalty, thr = a.am_threshold;

  // ---- static per-slot constants: info | first_state of the word (for position-1 slots) ------------
  uint32_t info[SPT], pk[SPT];  // pk = bkp of the hypothesis being built
#pragma unroll
  for (int i = 0; i < SPT; i++) {
    const uint32_t p = tid + i * NT;
    info[i] = p < P ? a.net.slot_info[p] : 0u;
    pk[i] = 0;
    sc[p] = kInf; bk[p] = 0;
  }
  if (tid < 8) e_first[tid] = 0xFFFFFFFFu;
  __syncthreads();
  // initial hypothesis: word 0, position 0, score 0 (Recognizer.cpp:120)
  const bool init_is_end = a.net.slot_info[0] & kSlotEnd;
  double m_we = init_is_end ? 0.0 : kInf;  // min over live word-end slots of the previous frame
  if (tid == 0) {
    sc[0] = 0.0;
    a.tb_score[tb0] = 0.0; a.tb_word[tb0] = 0; a.tb_bkp[tb0] = 0;  // traceback[0] = Book(0.0,0,0,0), :118
  }
  if (tid < 4 && init_is_end) e_first[4 + tid] = 0;  // frame t = 1 reads parity buffer 1
  // Emission costs are gathered TWO frames ahead into two register sets (set f&1 holds frame f, frames are
  // 1-based) and mirrored into am_l one frame ahead, so neither the frame body nor its barriers ever wait on
  // HBM: the gathers of frame t+2 are issued at the top of frame t and first touched in phase C of frame t+1.
  double am_s0[SPT], am_s1[SPT];
#pragma unroll
  for (int i = 0; i < SPT; i++) {
    const uint32_t p = tid + i * NT;
    am_s1[i] = T > 0 ? row0[info[i] & 0xFFFFu] : 0.0;  // padding slots carry state 0: a valid address, result unused
    am_l[p] = am_s1[i];
    am_s0[i] = T > 1 ? row0[a.ld + (info[i] & 0xFFFFu)] : 0.0;
  }
  __syncthreads();
  uint32_t slow_taken = 0;

  auto frame = [&](const uint32_t t, double (&am_issue)[SPT], double (&am_consume)[SPT]) {
    const uint32_t* ef_cur = e_first + 4 * (t & 1);
    uint32_t* ef_nxt = e_first + 4 * ((t + 1) & 1);
    const uint32_t bkp_new = (t - 1) & 0xFFFFu;  // merge_hypothesis(.., t - 1, ..) truncated to uint16 (:154, Recognizer.hpp:79)
    if (t + 2 <= T) {
      const double* rown = row0 + (uint64_t)(t + 1) * a.ld;  // frame t+2
#pragma unroll
      for (int i = 0; i < SPT; i++) am_issue[i] = rown[info[i] & 0xFFFFu];
    }

    // ---- A: build the new hypotheses in registers ------------------------------------------------
    // Branch-free: every slot makes the same five offers in ascending source order -- [boundary], skip,
    // forward, loop, [boundary] -- where a candidate that does not exist for this slot is +inf, which
    // Merge::offer ignores exactly like the reference ignores an absent hypothesis (:127-129).
    double nv[SPT];
    double my_best = kInf, my_we = kInf;
    uint32_t my_we_idx = 0xFFFFFFFFu;
    bool any_slow = false;
#pragma unroll
    for (int i = 0; i < SPT; i++) {
      uint32_t p = tid + i * NT;
      const bool live = p < P;
      asm volatile("" : "+v"(p));  // keep p*8 / p*2 address math out of loop-invariant registers
      // launder the slot constants: otherwise LICM hoists every derived per-slot value (tdp selects, word
      // penalty, class: ~12 VGPRs per slot) out of the frame loop and occupancy drops to 1 wave/SIMD
      uint32_t inf = info[i];
      asm volatile("" : "+v"(inf));
      const double am = am_l[p];
      const bool pos0 = inf & kSlotPos0, pos1 = inf & kSlotPos1, entry = pos0 || pos1;
      const bool sil_state = inf & kSlotSilState;
      const double t_loop = sil_state ? tf : tl, t_fwd = tf, t_skip = sil_state ? tf : ts;
      // unconditional LDS reads at clamped addresses; the selects below discard what does not apply
      const uint32_t p1 = p - (pos0 ? 0u : 1u), p2 = p - (entry ? 0u : 2u);
      const double s0 = sc[p], s1 = sc[p1], s2 = sc[p2], a1 = am_l[p1];
      const uint32_t b_loop_ = bk[p], b_fwd_ = bk[p1], b_skip_ = bk[p2];
      const double c_skip = entry ? kInf : s2 + t_skip;
      const double c_fwd = pos0 ? kInf : s1 + t_fwd;
      const double c_loop = (inf & kSlotEnd) ? kInf : s0 + t_loop;  // word ends do not expand in-word (:131)
      // word-boundary candidate (positions 0 and 1 only)
      const double am_b = pos1 ? a1 : am;  // emission of the word's position 0, even when entering position 1 (:136,148-151)
      const double wp = (inf & kSlotSilWord) ? 0.0 : wp_word;
      const bool b_skip = pos1 && !(inf & kSlotFirstSil);  // tdp(first_state, init + 1)
      const double t_b = b_skip ? ts : tf;
      const uint32_t cls = ((inf & kSlotSilWord) ? 0u : 2u) + (b_skip ? 1u : 0u);
      const double c_b = entry ? (m_we + wp) + t_b : kInf;  // cur_hyp->score + word_penalty + tdp, :140
      const uint32_t e_b = ef_cur[cls];                     // first word-end slot attaining c_b
      const bool b_first = e_b < p1;                        // is that source visited before the in-word ones? (p1 == p for position 0)
      Merge mg;
      mg.offer(b_first ? c_b : kInf, am_b, bkp_new);
      mg.offer(c_skip, am, b_skip_);
      mg.offer(c_fwd, am, b_fwd_);
      mg.offer(c_loop, am, b_loop_);
      mg.offer(b_first ? kInf : c_b, am_b, bkp_new);
      double extra = kInf;  // one-position word: boundary candidates with init = 1 land in a slot past the word's
                            // end (Recognizer.cpp:139); it never expands but feeds best_score (:155)
      if (live && (inf & kSlotSingle)) extra = ((m_we + wp) + ((inf & kSlotFirstSil) ? tf : ts)) + am;
      // the collapsed boundary candidate is only exact while the pre-AM early-out (:143) is inert
      const bool slow = live && (entry && (am_b < 0.0 || am < 0.0));
      any_slow |= slow;
      nv[i] = live ? mg.score : kInf; pk[i] = mg.bkp | (slow ? 0x80000000u : 0u);
      const double lo = extra < nv[i] ? extra : nv[i];
      my_best = lo < my_best ? lo : my_best;
      // keep the slots' live ranges apart (otherwise every slot's LDS reads are hoisted to the top: +60 VGPRs)
      __builtin_amdgcn_sched_barrier(0);
    }
    if (__any(any_slow)) {  // wave-uniform: some lane has a negative emission cost on an entry slot
      slow_taken = 1;
      my_best = kInf;
#pragma unroll
      for (int i = 0; i < SPT; i++) {
        const uint32_t p = tid + i * NT;
        const uint32_t inf = info[i];
        if (pk[i] & 0x80000000u) {
          const bool pos1 = inf & kSlotPos1;
          const double am = am_l[p], am_b = pos1 ? am_l[p - 1] : am;
          const double wp = (inf & kSlotSilWord) ? 0.0 : wp_word;
          const bool sil_state = inf & kSlotSilState;
          const double t_b = (pos1 && !(inf & kSlotFirstSil)) ? ts : tf;
          const Merge mg = replay_boundary(a.net.word_end_slot, a.net.n_words, sc, bk, p, pos1, !(inf & kSlotEnd), true, wp, t_b, am_b, am, tf,
                                           sil_state ? tf : tl, bkp_new);
          nv[i] = mg.score; pk[i] = mg.bkp;
        }
        double extra = kInf;
        if (p < P && (inf & kSlotSingle)) {
          const double am = am_l[p];
          const double wp = (inf & kSlotSilWord) ? 0.0 : wp_word;
          const double t_d = (inf & kSlotFirstSil) ? tf : ts;
          if (am >= 0.0) extra = ((m_we + wp) + t_d) + am;
          else extra = replay_boundary(a.net.word_end_slot, a.net.n_words, sc, bk, p, false, false, false, wp, t_d, am, am, tf, tf, bkp_new).score;
        }
        const double lo = extra < nv[i] ? extra : nv[i];
        my_best = lo < my_best ? lo : my_best;
      }
    }
#pragma unroll
    for (int i = 0; i < SPT; i++) {
      const uint32_t p = tid + i * NT;
      pk[i] &= 0xFFFFu;
      if (p < P && (info[i] & kSlotEnd) && (nv[i] < my_we || (nv[i] == my_we && p < my_we_idx))) { my_we = nv[i]; my_we_idx = p; }
    }
    if (tid < 4) ef_nxt[tid] = 0xFFFFFFFFu;

    // ---- B: block reductions -----------------------------------------------------------------------
    double best, we;
    uint32_t we_idx;
    block_minima<NT>(my_best, my_we, my_we_idx, red_best, red_we, red_idx, best, we, we_idx);

    // ---- C: prune, traceback, publish word-end minimum ------------------------------------------------
    const double limit = best + thr;
    const bool we_alive = !(we > limit) && we != kInf;
    m_we = we_alive ? we : kInf;
    // a word end other than we_idx can only tie the boundary candidate of the minimum if it rounds to
    // the same sum: its score is within a few ulps of the minimum (cheap, safe pre-filter)
    const double near = m_we + (fabs(m_we) + fabs(wp_word) + fabs(tf) + fabs(ts) + 1.0) * 1e-9;
#pragma unroll
    for (int i = 0; i < SPT; i++) {
      const uint32_t p = tid + i * NT;
      double v = nv[i];
      if (v > limit) v = kInf;  // :194-196
      sc[p] = v;
      bk[p] = (uint16_t)pk[i];
      am_l[p] = am_consume[i];  // next frame's emission costs (gathered two frames ago)
      if ((info[i] & kSlotEnd) && we_alive && v <= near) {
        if (p == we_idx) {  // first minimal surviving word end -> traceback[t] (:199-205)
          a.tb_score[tb0 + t] = v; a.tb_word[tb0 + t] = (uint16_t)p; a.tb_bkp[tb0 + t] = (uint16_t)pk[i];  // slot now, word after the loop
        }
        publish_word_end(ef_nxt, p, v, m_we, wp_word, tf, ts);
      }
    }
    if (!we_alive && tid == 0) { a.tb_score[tb0 + t] = kInf; a.tb_word[tb0 + t] = 0xFFFFu; a.tb_bkp[tb0 + t] = 0; }
    __syncthreads();
  };

  for (uint32_t t = 1; t <= T; t += 2) {
    frame(t, am_s1, am_s0);  // odd frame: refill set 1 (frame t+2), mirror set 0 (frame t+1)
    if (t + 1 <= T) frame(t + 1, am_s0, am_s1);
  }

  // ---- traceback (Recognizer.cpp:222-231; traceback.h) ------------------------------------------------------
  __threadfence();
  __syncthreads();
  traceback_slots_to_words<NT>(a, u, tb0, T, a.net.slot_word, P);
  traceback_walk(a, u, f0, tb0, T, slow_taken);
}

// ---- the same search for lexicons whose hypothesis arrays do not fit the LDS (more than 8192 slots) -----------------------
// Scores and back pointers of the two frames in flight live in a per-workgroup global workspace (20 bytes per slot: L2
// resident), emission costs are gathered where they are used, and a thread walks its slots in a loop instead of keeping them in
// registers.  Phases, merge order and the exactness argument are decode_kernel's (the sequential boundary replay is inline,
// per lane); slot ids stay 16 bit in the traceback, so P <= 65534.  A capacity path: measured 12.3 ms for
// 256 utterances at 9001 slots against 5.3 ms at 8000 slots in the type-sorted LDS kernel (2 x per slot).
//
// big_frame is one frame t of that search, shared by decode_big_kernel (a whole utterance) and decode_stream_kernel (k frames
// of an open utterance, from state a previous launch left).  Everything frame t + 1 needs is what it leaves behind: the
// pruned scores and back pointers in scn / bkn, m_we, and ef_nxt (the first word-end slot per boundary class).  Its traceback
// entry goes through `record(score, slot, bkp)`: slot 0xFFFF when no word end survives.
template <int NT, class Record>
__device__ __forceinline__ void big_frame(const DecodeNet& net, double wp_word, double thr, const double* row, uint32_t t,
                                          const double* sc, const uint16_t* bk, double* scn, uint16_t* bkn, const uint32_t* ef_cur,
                                          uint32_t* ef_nxt, double* red_best, double* red_we, uint32_t* red_idx, double& m_we,
                                          uint32_t& slow_taken, Record record) {
  const uint32_t P = net.n_slots;
  const uint32_t tid = threadIdx.x;
  const double tl = net.tdp_loop, tf = net.tdp_forward, ts = net.tdp_skip;
  const uint32_t bkp_new = (t - 1) & 0xFFFFu;
  // ---- A: the new hypotheses, unpruned, into the other buffer ---------------------------------------------------
  double my_best = kInf, my_we = kInf;
  uint32_t my_we_idx = 0xFFFFFFFFu;
  for (uint32_t p = tid; p < P; p += NT) {
    const uint32_t inf = net.slot_info[p];
    const double am = row[inf & 0xFFFFu];
    const bool pos0 = inf & kSlotPos0, pos1 = inf & kSlotPos1, entry = pos0 || pos1;
    const bool sil_state = inf & kSlotSilState;
    const double t_loop = sil_state ? tf : tl, t_skip = sil_state ? tf : ts;
    const uint32_t p1 = p - (pos0 ? 0u : 1u), p2 = p - (entry ? 0u : 2u);
    const double c_skip = entry ? kInf : sc[p2] + t_skip;
    const double c_fwd = pos0 ? kInf : sc[p1] + tf;
    const double c_loop = (inf & kSlotEnd) ? kInf : sc[p] + t_loop;  // word ends do not expand in-word (:131)
    const double am_b = pos1 ? row[net.slot_info[p1] & 0xFFFFu] : am;  // emission of the word's position 0 (:136,148-151)
    const double wp = (inf & kSlotSilWord) ? 0.0 : wp_word;
    const bool b_skip = pos1 && !(inf & kSlotFirstSil);
    const double t_b = b_skip ? ts : tf;
    const uint32_t cls = ((inf & kSlotSilWord) ? 0u : 2u) + (b_skip ? 1u : 0u);
    Merge mg;
    if (entry && (am_b < 0.0 || am < 0.0)) {  // the collapsed boundary candidate is only exact while the pre-AM early-out is inert
      mg = replay_boundary(net.word_end_slot, net.n_words, sc, bk, p, pos1, !(inf & kSlotEnd), true, wp, t_b, am_b, am, tf, t_loop, bkp_new);
      slow_taken = 1;
    } else {
      const double c_b = entry ? (m_we + wp) + t_b : kInf;  // cur_hyp->score + word_penalty + tdp, :140
      const bool b_first = ef_cur[cls] < p1;                // is that source visited before the in-word ones?
      mg.offer(b_first ? c_b : kInf, am_b, bkp_new);
      mg.offer(c_skip, am, bk[p2]);
      mg.offer(c_fwd, am, bk[p1]);
      mg.offer(c_loop, am, bk[p]);
      mg.offer(b_first ? kInf : c_b, am_b, bkp_new);
    }
    double lo = mg.score;
    if (inf & kSlotSingle) {  // one-position word: its dead position-1 slot still feeds best_score (:139,155)
      const double t_d = (inf & kSlotFirstSil) ? tf : ts;
      double extra;
      if (am >= 0.0) extra = ((m_we + wp) + t_d) + am;
      else { extra = replay_boundary(net.word_end_slot, net.n_words, sc, bk, p, false, false, false, wp, t_d, am, am, tf, tf, bkp_new).score; slow_taken = 1; }
      lo = extra < lo ? extra : lo;
    }
    my_best = lo < my_best ? lo : my_best;
    scn[p] = mg.score;
    bkn[p] = (uint16_t)mg.bkp;
    if ((inf & kSlotEnd) && (mg.score < my_we || (mg.score == my_we && p < my_we_idx))) { my_we = mg.score; my_we_idx = p; }
  }
  if (tid < 4) ef_nxt[tid] = 0xFFFFFFFFu;
  // ---- B ---------------------------------------------------------------------------------------------------------
  double best, we;
  uint32_t we_idx;
  block_minima<NT>(my_best, my_we, my_we_idx, red_best, red_we, red_idx, best, we, we_idx);
  // ---- C: prune, traceback, publish the word-end minimum -----------------------------------------------------------
  const double limit = best + thr;
  const bool we_alive = !(we > limit) && we != kInf;
  m_we = we_alive ? we : kInf;
  const double near = m_we + (fabs(m_we) + fabs(wp_word) + fabs(tf) + fabs(ts) + 1.0) * 1e-9;
  for (uint32_t p = tid; p < P; p += NT) {  // (a thread prunes the slots it wrote)
    const double v = scn[p];
    if (v > limit) { scn[p] = kInf; continue; }  // :194-196
    if ((net.slot_info[p] & kSlotEnd) && we_alive && v <= near) {
      if (p == we_idx) record(v, p, (uint32_t)bkn[p]);
      publish_word_end(ef_nxt, p, v, m_we, wp_word, tf, ts);
    }
  }
  if (!we_alive && tid == 0) record(kInf, 0xFFFFu, 0u);
  __syncthreads();  // workgroup-scope release/acquire: the pruned scores are visible to every thread of the next frame
}

template <int NT>
__global__ __launch_bounds__(NT) void decode_big_kernel(DecodeArgs a, unsigned char* ws_all, size_t ws_stride) {
  constexpr uint32_t kWavesPerWg = NT / 64;
  __shared__ double red_best[kWavesPerWg], red_we[kWavesPerWg];
  __shared__ uint32_t red_idx[kWavesPerWg], e_first[8];
  const uint32_t P = a.net.n_slots;
  const uint32_t tid = threadIdx.x;
  const uint32_t u = a.utt_order ? a.utt_order[a.utt_first + blockIdx.x] : a.utt_first + blockIdx.x;
  if (a.only_flagged && !(a.out_flags[u] & kFlagReplay)) return;  // workgroup-uniform: nothing to redo for this utterance
  const uint64_t f0 = a.frame_off[u];
  const uint32_t T = (uint32_t)(a.frame_off[u + 1] - f0);
  const double* row0 = a.scores + (f0 - a.frame_base) * a.ld;
  const uint64_t tb0 = f0 + u;
  unsigned char* ws = ws_all + (size_t)blockIdx.x * ws_stride;
  double* scb[2] = {reinterpret_cast<double*>(ws), reinterpret_cast<double*>(ws) + P};
  uint16_t* bkb[2] = {reinterpret_cast<uint16_t*>(ws + (size_t)P * 16), reinterpret_cast<uint16_t*>(ws + (size_t)P * 16) + P};

  for (uint32_t p = tid; p < P; p += NT) { scb[0][p] = kInf; bkb[0][p] = 0; }
  if (tid < 8) e_first[tid] = 0xFFFFFFFFu;
  __syncthreads();
  const bool init_is_end = a.net.slot_info[0] & kSlotEnd;
  double m_we = init_is_end ? 0.0 : kInf;
  if (tid == 0) {
    scb[0][0] = 0.0;  // initial hypothesis: word 0, position 0, score 0 (Recognizer.cpp:120)
    a.tb_score[tb0] = 0.0; a.tb_word[tb0] = 0; a.tb_bkp[tb0] = 0;
  }
  if (tid < 4 && init_is_end) e_first[4 + tid] = 0;
  __syncthreads();
  uint32_t slow_taken = 0;

  for (uint32_t t = 1; t <= T; t++) {
    // the winning word-end SLOT now, its word after the loop
    big_frame<NT>(a.net, a.word_penalty, a.am_threshold, row0 + (uint64_t)(t - 1) * a.ld, t, scb[(t - 1) & 1], bkb[(t - 1) & 1],
                  scb[t & 1], bkb[t & 1], e_first + 4 * (t & 1), e_first + 4 * ((t + 1) & 1), red_best, red_we, red_idx, m_we,
                  slow_taken, [&](double v, uint32_t slot, uint32_t bkp) {
                    a.tb_score[tb0 + t] = v; a.tb_word[tb0 + t] = (uint16_t)slot; a.tb_bkp[tb0 + t] = (uint16_t)bkp;
                  });
  }

  // ---- traceback (Recognizer.cpp:222-231; traceback.h) ------------------------------------------------------
  __threadfence();
  __syncthreads();
  traceback_slots_to_words<NT>(a, u, tb0, T, a.net.slot_word, P);
  traceback_walk(a, u, f0, tb0, T, slow_taken);
}

// ---- streaming (sr_stream_push): k more frames of each of n open utterances --------------------------------------------
// One workgroup per stream in the push.  The stream's state lives in device memory between launches: the double-buffered
// scores and back pointers (decode_big_workspace bytes; the current buffer is the frame parity), its StreamState (m_we and
// e_first for the next frame, flags, the partial word count) and its traceback of max_frames + 1 entries.  A stream whose first
// frame is in this push starts from decode_big_kernel's initial state, so a reused slot carries nothing over.  Traceback entries
// are written as WORDS at the frame they are produced, so the guarded walk at the end of the push can run at any frame; the walk
// reads the state and changes none of it.
template <int NT>
__global__ __launch_bounds__(NT) void decode_stream_kernel(StreamArgs a) {
  constexpr uint32_t kWavesPerWg = NT / 64;
  __shared__ double red_best[kWavesPerWg], red_we[kWavesPerWg];
  __shared__ uint32_t red_idx[kWavesPerWg], e_first[8];
  const StreamJob job = a.jobs[blockIdx.x];
  const uint32_t P = a.net.n_slots;
  const uint32_t tid = threadIdx.x;
  StreamState* st = a.state + job.slot;
  unsigned char* ws = a.ws + (size_t)job.slot * a.ws_stride;
  double* scb[2] = {reinterpret_cast<double*>(ws), reinterpret_cast<double*>(ws) + P};
  uint16_t* bkb[2] = {reinterpret_cast<uint16_t*>(ws + (size_t)P * 16), reinterpret_cast<uint16_t*>(ws + (size_t)P * 16) + P};
  const uint64_t tb0 = (uint64_t)job.slot * a.tb_stride;
  const uint32_t t0 = job.t0, t1 = job.t0 + job.k;

  double m_we;
  uint32_t flags;
  if (t0 == 0) {  // decode_big_kernel's initial state (Recognizer.cpp:116-120)
    for (uint32_t p = tid; p < P; p += NT) { scb[0][p] = kInf; bkb[0][p] = 0; }
    if (tid < 8) e_first[tid] = 0xFFFFFFFFu;
    __syncthreads();
    const bool init_is_end = a.net.slot_info[0] & kSlotEnd;
    m_we = init_is_end ? 0.0 : kInf;
    flags = 0;
    if (tid == 0) {
      scb[0][0] = 0.0;
      a.tb_score[tb0] = 0.0; a.tb_word[tb0] = 0; a.tb_bkp[tb0] = 0;
    }
    if (tid < 4 && init_is_end) e_first[4 + tid] = 0;
  } else {  // what the last push left (the other half of e_first is reset by the first frame before it is read)
    m_we = st->m_we;
    flags = st->flags;
    if (tid < 4) e_first[4 * ((t0 + 1) & 1) + tid] = st->e_first[tid];
  }
  __syncthreads();
  uint32_t slow_taken = 0;

  for (uint32_t t = t0 + 1; t <= t1; t++) {
    const double* row = a.scores + (job.row0 + (uint64_t)(t - t0 - 1)) * a.ld;
    big_frame<NT>(a.net, a.word_penalty, a.am_threshold, row, t, scb[(t - 1) & 1], bkb[(t - 1) & 1], scb[t & 1], bkb[t & 1],
                  e_first + 4 * (t & 1), e_first + 4 * ((t + 1) & 1), red_best, red_we, red_idx, m_we, slow_taken,
                  [&](double v, uint32_t slot, uint32_t bkp) {  // no surviving word end -> word 0 (:118,191)
                    a.tb_score[tb0 + t] = v;
                    a.tb_word[tb0 + t] = slot == 0xFFFFu ? (uint16_t)0 : (uint16_t)a.net.slot_word[slot];
                    a.tb_bkp[tb0 + t] = (uint16_t)bkp;
                  });
  }

  // ---- the state for the next push, and the partial result: the guarded walk from frame t1 (traceback.h) --------------
  __threadfence();
  const bool slow = __syncthreads_or((int)slow_taken) != 0;
  if (tid < 4) st->e_first[tid] = e_first[4 * ((t1 + 1) & 1) + tid];
  if (tid == 0) {
    st->m_we = m_we;
    const uint32_t n = walk_traceback(
        t1, a.net.silence_word, a.net.n_words,
        [&](uint32_t t) -> uint32_t { return __hip_atomic_load(&a.tb_word[tb0 + t], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); },
        [&](uint32_t t) -> uint32_t { return __hip_atomic_load(&a.tb_bkp[tb0 + t], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); },
        a.words + (uint64_t)job.slot * a.words_stride, t1);
    flags = (flags & kFlagSlowPath) | (slow ? kFlagSlowPath : 0u) | (n == kTbCorrupt ? kFlagCorrupt : 0u);
    st->flags = flags;
    st->count = n == kTbCorrupt ? 0u : n;
  }
}

uint32_t decode_big_max_slots() { return 65534; }  // slot ids are 16 bit in the traceback, 0xFFFF = no surviving word end
size_t decode_big_workspace(uint32_t n_slots) { return (((size_t)n_slots * 20) + 255) & ~(size_t)255; }  // per utterance in flight
static hipError_t launch_decode_big(const DecodeArgs& a, unsigned char* ws, hipStream_t stream) {
  if (a.net.n_slots > decode_big_max_slots() || !ws) return hipErrorInvalidValue;
  hipLaunchKernelGGL((decode_big_kernel<1024>), dim3(a.n_utts), dim3(1024), 0, stream, a, ws, decode_big_workspace(a.net.n_slots));
  return hipGetLastError();
}
hipError_t launch_decode_stream(const StreamArgs& a, uint32_t n_jobs, hipStream_t stream) {
  if (n_jobs == 0) return hipSuccess;
  if (a.net.n_slots > decode_big_max_slots()) return hipErrorInvalidValue;
  hipLaunchKernelGGL((decode_stream_kernel<1024>), dim3(n_jobs), dim3(1024), 0, stream, a);
  return hipGetLastError();
}

// ---- the stable prefix of an open utterance (sr_stream_stable) ---------------------------------------------------------------
// One workgroup per requested stream, launched on demand; the search's state is read, never written.  After t frames the current
// buffer is the frame parity t & 1 (big_frame wrote frame t's pruned hypotheses there): B = { bk[p] : sc[p] finite } are the
// traceback nodes a later traceback can still run through, and their nearest common ancestor under parent(c) = tb_bkp[c] is the
// commit point (commit_point.h).  The same pass keeps the alive hypothesis of least score (ties: the
// smaller slot) for the trailing silence.  Thread 0 then walks from the commit point with traceback.h's guards into the slot's
// own word buffer, and the workgroup copies the words into the call's result block.
// The scan both stream_commit_kernel and stream_trim_kernel start with, by every thread of the workgroup: the fold of the alive
// hypotheses' back pointers (-> the return value: kCommitNone where none is alive, kCommitCorrupt) and, per wave, the alive hypothesis
// of least score in red_sc / red_idx (commit_best reads them).  Ends behind a barrier.
template <int NT, class Parent>
__device__ __forceinline__ uint32_t commit_scan(uint32_t P, uint32_t t, const double* sc, const uint16_t* bk, uint32_t floor, Parent parent,
                                                uint32_t* red, double* red_sc, uint32_t* red_idx) {
  const uint32_t tid = threadIdx.x;
  uint32_t mine = kCommitNone, my_p = 0xFFFFFFFFu;
  double my_v = kInf;
  if (t == 0) {  // nothing searched yet (the buffers are not initialised): B = {0}
    if (tid == 0) mine = 0;
  } else {
    for (uint32_t p = tid; p < P; p += NT) {
      const double v = sc[p];
      if (!(v < kInf)) continue;  // pruned or never reached
      const uint32_t b = bk[p];
      mine = commit_lca(mine, b < t ? b : kCommitCorrupt, floor, parent);
      if (v < my_v) { my_v = v; my_p = p; }
    }
  }
  const uint32_t all = commit_fold<NT>(mine, floor, red, parent);
  wave_min_idx(my_v, my_p);
  if ((tid & 63) == 0) { red_sc[tid >> 6] = my_v; red_idx[tid >> 6] = my_p; }
  __syncthreads();
  return all;
}

template <int NT>
__global__ __launch_bounds__(NT) void stream_commit_kernel(StableArgs a) {
  constexpr uint32_t kWavesPerWg = NT / 64;
  __shared__ double red_sc[kWavesPerWg];
  __shared__ uint32_t red[kWavesPerWg], red_idx[kWavesPerWg], n_out;
  const StableJob job = a.jobs[blockIdx.x];
  const uint32_t P = a.net.n_slots;
  const uint32_t tid = threadIdx.x;
  const uint32_t t = job.t;
  const unsigned char* ws = a.ws + (size_t)job.slot * a.ws_stride;
  const double* sc = reinterpret_cast<const double*>(ws) + (size_t)(t & 1) * P;
  const uint16_t* bk = reinterpret_cast<const uint16_t*>(ws + (size_t)P * 16) + (size_t)(t & 1) * P;
  const uint64_t tb0 = (uint64_t)job.slot * a.tb_stride;
  const uint32_t floor = job.fresh ? 0u : a.commit[job.slot];
  auto parent = [&](uint32_t c) -> uint32_t { return a.tb_bkp[tb0 + c]; };

  const uint32_t all = commit_scan<NT>(P, t, sc, bk, floor, parent, red, red_sc, red_idx);
  uint32_t* words = a.words + (uint64_t)job.slot * a.words_stride;
  if (tid == 0) {
    double best = red_sc[0];
    uint32_t best_p = red_idx[0];
    for (uint32_t w = 1; w < kWavesPerWg; w++)
      if (red_sc[w] < best || (red_sc[w] == best && red_idx[w] < best_p)) { best = red_sc[w]; best_p = red_idx[w]; }
    StableResult r{floor, 0u, 0u, 0u};
    const uint32_t c = all == kCommitNone ? floor : all;  // no hypothesis alive: the commit point stays where it was
    if (c == kCommitCorrupt || c > t) r.flags = kStableCorrupt;
    else {
      const uint32_t n = walk_traceback(
          c, a.net.silence_word, a.net.n_words, [&](uint32_t f) -> uint32_t { return a.tb_word[tb0 + f]; },
          [&](uint32_t f) -> uint32_t { return a.tb_bkp[tb0 + f]; }, words, c);
      if (n == kTbCorrupt) r.flags = kStableCorrupt;
      else { r.commit = c; r.count = n; }
    }
    if (best_p < P && (a.net.slot_info[best_p] & kSlotSilWord)) {
      const uint32_t b = bk[best_p];
      r.silence = b < t ? t - b : 0u;
    }
    if (!r.flags) a.commit[job.slot] = r.commit;
    a.out_res[blockIdx.x] = r;
    n_out = r.count;
  }
  __syncthreads();  // workgroup-scope release/acquire: thread 0's words are visible to the copy
  const uint32_t n = n_out;
  for (uint32_t i = tid; i < n; i += NT) a.out_words[job.word_off + i] = words[i];
}

hipError_t launch_stream_commit(const StableArgs& a, uint32_t n_jobs, hipStream_t stream) {
  if (n_jobs == 0) return hipSuccess;
  if (a.net.n_slots > decode_big_max_slots()) return hipErrorInvalidValue;
  hipLaunchKernelGGL((stream_commit_kernel<256>), dim3(n_jobs), dim3(256), 0, stream, a);
  return hipGetLastError();
}

// ---- dropping the committed frames of an open utterance (sr_stream_trim) ---------------------------------
// One workgroup per requested stream.  The commit point c is stream_commit_kernel's (commit_scan, the same floor).  Nothing below
// c is read again except to spell out the words on the way to it, so: thread 0 walks from c into the committed-walk buffer, the
// workgroup copies those words out, and what the search left is renumbered with c as the new frame 0.
//   (1) checks, before anything is written: c is a node below t (a hypothesis entered at frame t carries bkp = t - 1, so c <= t - 1
//       and the window keeps a frame), every alive back pointer is >= c, the walk from c passes its guards.
//   (2) traceback entries (c, t] move to (0, t - c] in tiles of NT entries, ascending.  The move overlaps itself (destination
//       i, source c + i), so a tile is READ INTO REGISTERS, then a BARRIER, then WRITTEN: within a tile no thread's write can land
//       on an entry another thread has yet to read; across tiles the sources of tile k + 1 (> c + (k + 1) NT) lie above every
//       destination written so far (<= (k + 1) NT), and tile k + 1's writes follow its own barrier, which no thread reaches before
//       its reads of tile k are done.  A back pointer below c belongs to the no-word-end record (inf, word 0, bkp 0) or to a dead
//       node, which no walk from a later finite entry reaches (section 4.5c(1)): it becomes 0.  Entry 0 becomes (0.0, 0, 0).
//   (3) the alive hypotheses' back pointers lose c.  big_frame and stream_commit_kernel take the current buffer from the frame
//       parity, so with c odd scores (unchanged: they stay absolute) and back pointers go to the other buffer, with c even the back
//       pointers are rewritten in place.  A thread touches only its own slots p: no ordering needed.
//   (4) commit[slot] = 0, and thread 0 redoes the partial result's walk from frame t - c behind a barrier.
template <int NT>
__global__ __launch_bounds__(NT) void stream_trim_kernel(TrimArgs a) {
  constexpr uint32_t kWavesPerWg = NT / 64;
  __shared__ double red_sc[kWavesPerWg];
  __shared__ uint32_t red[kWavesPerWg], red_idx[kWavesPerWg], n_out;
  const StableJob job = a.jobs[blockIdx.x];
  const uint32_t P = a.net.n_slots;
  const uint32_t tid = threadIdx.x;
  const uint32_t t = job.t;
  unsigned char* ws = a.ws + (size_t)job.slot * a.ws_stride;
  double* sc0 = reinterpret_cast<double*>(ws);                           // the two buffers of scores, then of back pointers
  uint16_t* bk0 = reinterpret_cast<uint16_t*>(ws + (size_t)P * 16);
  const double* sc = sc0 + (size_t)(t & 1) * P;
  const uint16_t* bk = bk0 + (size_t)(t & 1) * P;
  const uint64_t tb0 = (uint64_t)job.slot * a.tb_stride;
  const uint32_t floor = job.fresh ? 0u : a.commit[job.slot];
  auto parent = [&](uint32_t c) -> uint32_t { return a.tb_bkp[tb0 + c]; };

  const uint32_t all = commit_scan<NT>(P, t, sc, bk, floor, parent, red, red_sc, red_idx);
  const uint32_t c = all == kCommitNone ? floor : all;  // no hypothesis alive: the commit point stays where it was
  // ---- (1) ----
  bool bad = c == kCommitCorrupt || (t == 0 ? c != 0 : c >= t);
  if (!bad && t)
    for (uint32_t p = tid; p < P; p += NT)
      if (sc[p] < kInf && bk[p] < c) bad = true;
  uint32_t* walk_words = a.walk_words + (uint64_t)job.slot * a.words_stride;
  if (tid == 0) {
    uint32_t n = 0;
    if (!bad) {
      n = walk_traceback(
          c, a.net.silence_word, a.net.n_words, [&](uint32_t f) -> uint32_t { return a.tb_word[tb0 + f]; },
          [&](uint32_t f) -> uint32_t { return a.tb_bkp[tb0 + f]; }, walk_words, c);
      if (n == kTbCorrupt) bad = true;
    }
    n_out = n;
  }
  bad = __syncthreads_or((int)bad) != 0;  // (also: thread 0's words and n_out are visible to the workgroup)
  if (bad) {
    if (tid == 0) a.out_res[blockIdx.x] = StableResult{0u, 0u, 0u, kStableCorrupt};
    return;
  }
  const uint32_t n_words = n_out;
  for (uint32_t i = tid; i < n_words; i += NT) a.out_words[job.word_off + i] = walk_words[i];
  if (tid == 0) {
    a.commit[job.slot] = 0;
    a.out_res[blockIdx.x] = StableResult{c, 0u, n_words, 0u};
  }
  if (c == 0) return;  // nothing to drop (workgroup-uniform): the state stays as it is, bit for bit
  // ---- (2) ----
  const uint32_t n_keep = t - c;
  for (uint32_t i0 = 1; i0 <= n_keep; i0 += NT) {  // (a uniform trip count: every thread meets every barrier)
    const uint32_t i = i0 + tid;
    double v = 0.0;
    uint16_t w = 0, b = 0;
    if (i <= n_keep) { v = a.tb_score[tb0 + c + i]; w = a.tb_word[tb0 + c + i]; b = a.tb_bkp[tb0 + c + i]; }
    __syncthreads();
    if (i <= n_keep) {
      a.tb_score[tb0 + i] = v; a.tb_word[tb0 + i] = w;
      a.tb_bkp[tb0 + i] = b >= c ? (uint16_t)(b - c) : (uint16_t)0;
    }
  }
  if (tid == 0) { a.tb_score[tb0] = 0.0; a.tb_word[tb0] = 0; a.tb_bkp[tb0] = 0; }  // (entry 0 is no tile's source: sources are > c)
  // ---- (3) ----
  double* scn = sc0 + (size_t)(n_keep & 1) * P;
  uint16_t* bkn = bk0 + (size_t)(n_keep & 1) * P;
  const bool moved = (c & 1) != 0;
  for (uint32_t p = tid; p < P; p += NT) {
    const double v = sc[p];
    const uint16_t b = bk[p];
    if (moved) scn[p] = v;
    if (v < kInf) bkn[p] = (uint16_t)(b - c);
    else if (moved) bkn[p] = b;
  }
  // ---- (4) ----
  __threadfence();
  __syncthreads();
  if (tid == 0) {
    StreamState* st = a.state + job.slot;
    const uint32_t n = walk_traceback(
        n_keep, a.net.silence_word, a.net.n_words,
        [&](uint32_t f) -> uint32_t { return __hip_atomic_load(&a.tb_word[tb0 + f], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); },
        [&](uint32_t f) -> uint32_t { return __hip_atomic_load(&a.tb_bkp[tb0 + f], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); },
        a.words + (uint64_t)job.slot * a.words_stride, n_keep);
    st->flags = (st->flags & kFlagSlowPath) | (n == kTbCorrupt ? kFlagCorrupt : 0u);
    st->count = n == kTbCorrupt ? 0u : n;
  }
}

hipError_t launch_stream_trim(const TrimArgs& a, uint32_t n_jobs, hipStream_t stream) {
  if (n_jobs == 0) return hipSuccess;
  if (a.net.n_slots > decode_big_max_slots()) return hipErrorInvalidValue;
  hipLaunchKernelGGL((stream_trim_kernel<256>), dim3(n_jobs), dim3(256), 0, stream, a);
  return hipGetLastError();
}

// the fold alone (sr_commit_points): one workgroup per set of nodes of a forest the caller supplies
template <int NT>
__global__ __launch_bounds__(NT) void commit_points_kernel(CommitPointsArgs a) {
  __shared__ uint32_t red[NT / 64];
  const uint64_t n0 = a.node_off[blockIdx.x], s0 = a.set_off[blockIdx.x];
  const uint64_t n_nodes = a.node_off[blockIdx.x + 1] - n0, n_set = a.set_off[blockIdx.x + 1] - s0;
  const uint32_t* par = a.parent + n0;
  const uint32_t floor = a.floor[blockIdx.x];
  auto parent = [&](uint32_t c) -> uint32_t { return par[c]; };  // c is a candidate or above one: below n_nodes
  uint32_t mine = kCommitNone;
  for (uint64_t j = threadIdx.x; j < n_set; j += NT) {
    const uint32_t x = a.set[s0 + j];
    mine = commit_lca(mine, x < n_nodes ? x : kCommitCorrupt, floor, parent);
  }
  const uint32_t all = commit_fold<NT>(mine, floor, red, parent);
  if (threadIdx.x == 0) a.out[blockIdx.x] = all;
}

hipError_t launch_commit_points(const CommitPointsArgs& a, uint32_t n_sets, hipStream_t stream) {
  if (n_sets == 0) return hipSuccess;
  hipLaunchKernelGGL((commit_points_kernel<256>), dim3(n_sets), dim3(256), 0, stream, a);
  return hipGetLastError();
}

uint32_t decode_max_slots() { return 8192; }

static size_t decode_smem(uint32_t PP) { return (size_t)PP * 16 + 16 * 8 * 2 + 16 * 4 + 12 * 4 + (size_t)PP * 2 + 16; }

static hipError_t launch_decode_lds(const DecodeArgs& a, hipStream_t stream) {
  const uint32_t P = a.net.n_slots;
  const dim3 grid(a.n_utts);
#define SR_LAUNCH(NT, SPT)                                                                                   \
  do {                                                                                                       \
    const size_t smem = decode_smem((NT) * (SPT));                                                           \
    hipError_t e = hipFuncSetAttribute((const void*)decode_kernel<NT, SPT>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)smem); \
    if (e != hipSuccess) return e;                                                                           \
    hipLaunchKernelGGL((decode_kernel<NT, SPT>), grid, dim3(NT), smem, stream, a);                           \
    return hipGetLastError();                                                                                \
  } while (0)
  if (P <= 64) SR_LAUNCH(64, 1);
  if (P <= 256) SR_LAUNCH(64, 4);
  if (P <= 1024) SR_LAUNCH(256, 4);
  if (P <= 2048) SR_LAUNCH(256, 8);
  if (P <= 4096) SR_LAUNCH(512, 8);
  if (P <= 8192) SR_LAUNCH(1024, 8);
#undef SR_LAUNCH
  return hipErrorInvalidValue;
}

// The one place that decides which kernels search a lexicon (kernels.h: DecodeRoute):
//   flags      word net applies   first kernel   replay kernel (decode_kernel; decode_big_kernel without a FastNet)
//   GENERAL    -                  none           every utterance
//   SLOT       -                  slots          flagged ones  (a big lexicon: none, every utterance)
//   none       yes                words          flagged ones
//   none       no                 slots          flagged ones  (a big lexicon: none, every utterance)
DecodeRoute decode_route(const DecodeArgs& a, bool general, bool slots) {
  const bool big = a.fast.n_slots == 0;
  DecodeFirst first = DecodeFirst::kNone;
  if (!general && !slots && decode_words_applies(a)) first = DecodeFirst::kWords;
  else if (!general && !big) first = DecodeFirst::kSlots;
  return DecodeRoute{first, big};
}

hipError_t launch_decode(DecodeArgs a, const DecodeRoute& r, unsigned char* big_ws, hipStream_t stream) {
  if (a.n_utts == 0) return hipSuccess;
  if (r.first != DecodeFirst::kNone) {
    hipError_t e = r.first == DecodeFirst::kWords ? launch_decode_words(a, stream) : launch_decode_fast(a, stream);
    if (e != hipSuccess) return e;
  }
  // the replay kernel, whose workgroups exit at once unless the fast one flagged their utterance (negative emission cost)
  a.only_flagged = r.first != DecodeFirst::kNone ? 1u : 0u;
  return r.big ? launch_decode_big(a, big_ws, stream) : launch_decode_lds(a, stream);
}

DecodeNet build_decode_net(uint32_t n_words, const uint32_t* word_off, const uint16_t* automaton, uint32_t silence_word,
                           uint32_t silence_state, const double tdp[3], std::vector<uint32_t>& slot_info,
                           std::vector<uint32_t>& slot_word, std::vector<uint32_t>& word_end_slot) {
  const uint32_t P = word_off[n_words];
  slot_info.assign(P, 0); slot_word.assign(P, 0); word_end_slot.assign(n_words, 0);
  for (uint32_t w = 0; w < n_words; w++) {
    const uint32_t b = word_off[w], n = word_off[w + 1] - b;
    for (uint32_t k = 0; k < n; k++) {
      const uint32_t st = automaton[b + k];
      uint32_t f = st;
      if (k == 0) f |= kSlotPos0;
      if (k == 1) f |= kSlotPos1;
      if (k == n - 1) f |= kSlotEnd;
      if (st == silence_state) f |= kSlotSilState;
      if (w == silence_word) f |= kSlotSilWord;
      if (automaton[b] == silence_state) f |= kSlotFirstSil;
      if (n == 1) f |= kSlotSingle;
      slot_info[b + k] = f;
      slot_word[b + k] = w;
    }
    word_end_slot[w] = b + n - 1;
  }
  DecodeNet net{};
  net.n_slots = P; net.n_words = n_words; net.silence_word = silence_word; net.silence_state = silence_state;
  net.tdp_loop = tdp[0]; net.tdp_forward = tdp[1]; net.tdp_skip = tdp[2];
  return net;
}

}  // namespace srgpu

// ---- the walk alone (sr_traceback_corpus): traceback arrays supplied by the caller, one thread per utterance ------------
namespace srgpu {
__global__ void traceback_kernel(const uint64_t* frame_off, uint32_t n_utts, const uint16_t* tb_word, const uint16_t* tb_bkp,
                                 uint32_t silence_word, uint32_t n_words, uint32_t* out_words, uint32_t* out_count,
                                 uint32_t* out_flags) {
  const uint32_t u = blockIdx.x * blockDim.x + threadIdx.x;
  if (u >= n_utts) return;
  const uint64_t f0 = frame_off[u], tb0 = f0 + u;
  const uint32_t T = (uint32_t)(frame_off[u + 1] - f0);
  const uint32_t n = walk_traceback(
      T, silence_word, n_words, [&](uint32_t t) -> uint32_t { return tb_word[tb0 + t]; },
      [&](uint32_t t) -> uint32_t { return tb_bkp[tb0 + t]; }, out_words + f0, T);
  out_flags[u] = n == kTbCorrupt ? kFlagCorrupt : 0u;
  out_count[u] = n == kTbCorrupt ? 0u : n;
}

hipError_t launch_traceback(const uint64_t* frame_off, uint32_t n_utts, const uint16_t* tb_word, const uint16_t* tb_bkp,
                            uint32_t silence_word, uint32_t n_words, uint32_t* out_words, uint32_t* out_count,
                            uint32_t* out_flags, hipStream_t stream) {
  if (n_utts == 0) return hipSuccess;
  hipLaunchKernelGGL(traceback_kernel, dim3((n_utts + 63) / 64), dim3(64), 0, stream, frame_off, n_utts, tb_word, tb_bkp,
                     silence_word, n_words, out_words, out_count, out_flags);
  return hipGetLastError();
}
}  // namespace srgpu
