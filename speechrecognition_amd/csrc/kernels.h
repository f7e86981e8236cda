// kernels.h -- argument blocks and launchers of the gfx950 kernels behind libsrgpu.so.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <vector>

#include "bigram_route.h"
#include "vtln_tables.h"

namespace srgpu {

// ---- GMM scoring, FP64 MFMA contraction (gmm_mfma.hip) ------------------------------------------
struct GmmMfmaArgs {
  const float* feats;           // [n_frames x dim] float32
  uint64_t n_frames;
  uint32_t dim;
  const double* apack;          // [n_blocks][KSTEPS][64] model rows in MFMA A-fragment order
  const uint32_t* blk_meta;     // [n_blocks] (group << 1) | last-block-of-group
  const uint32_t* grp_state;    // [n_groups*4] state written by slot g of a group, 0xFFFFFFFF = padding
  const uint32_t* split_begin;  // [ny+1] block range of each state-range split (group aligned)
  double* out;                  // [n_frames x ld]
  uint32_t ld;
  uint32_t nx, ny;              // frame tiles x state-range splits
};
int gmm_mfma_ksteps_for_dim(uint32_t dim);   // 0 if dim unsupported
int gmm_mfma_frames_per_tile(int ksteps);
hipError_t launch_gmm_mfma(const GmmMfmaArgs& a, int ksteps, bool sum, hipStream_t stream);

// ---- GMM scoring, direct form, bit-exact with the reference (gmm_exact.hip) ----------------------
struct GmmExactArgs {
  const float* feats;
  uint64_t n_frames;
  uint32_t dim;
  uint32_t n_states;
  const uint32_t* dens_off;  // [n_states+1]
  const double* means;       // [C x dim]
  const double* inv_vars;    // [C x dim]
  const double* norm;        // [C]
  const double* logw;        // [C]
  double* out;               // [n_frames x ld]
  uint32_t ld;
  uint32_t states_per_split; // grid.y splits the state range
};
hipError_t launch_gmm_exact(const GmmExactArgs& a, bool sum, uint32_t n_splits, hipStream_t stream);
// listed mode: only the (frame, state) pairs a forced alignment can touch.  Block b covers blk_frames[b] (<= 256) frames
// of one utterance starting at absolute frame blk_frame0[b] (a.feats = the corpus' first frame) and scores the states
// states[list_off[blk_list[b]] .. list_off[blk_list[b] + 1]) into out[(frame - frame_base) * ld + state].
struct GmmExactList {
  const uint64_t* blk_frame0;
  const uint32_t* blk_frames;
  const uint32_t* blk_list;
  const uint32_t* list_off;
  const uint32_t* states;   // null: dense mode
  uint32_t blk_first;
  uint64_t frame_base;
};
hipError_t launch_gmm_exact_listed(const GmmExactArgs& a, bool sum, const GmmExactList& L, uint32_t n_blocks, hipStream_t stream);
int gmm_exact_frames_per_block();

// ---- exact GMM scoring through an fp16 prefilter (gmm_prefilter.hip) ------------------------------------------------
struct GmmPrefilterArgs {
  const float* feats;
  uint64_t n_frames;
  uint32_t dim;
  const unsigned char* apack;   // [n_groups][8 blocks][KS32][64 lanes][8 fp16], scaled by a power of two
  const float* grp_lim;         // [n_groups*4][4] candidate limit of the state in that slot: 2 eps = [1] |b^ - b| + [0] |b| + [2]
                                // (pf_bound, gmm_prefilter.hip header; [3] unused)
  const uint32_t* split_begin;  // [ny+1] group ranges
  uint32_t* mask;               // [group][frame][4 state slots] candidate densities of (frame, state)
  uint32_t nx, ny;
  uint32_t chunks;              // 1, 2 or 4 consecutive state slots (of 32 densities) make up one state
  // the group-stationary route (gmm_prefilter_stationary_kernel): the launch's frame operands, built once per launch
  uint32_t n_groups;
  uint4* bfrag;                 // [16-frame block][k-step][lane][8 fp16] B fragments, gmm_prefilter_operand_sizes() entries
  float2* bnorm;                // [frame] (|b|, |b^ - b|), both rounded up, the second capped (gmm_prefilter.hip header)
};
enum { kPfStaged = 0, kPfStationary = 1 };  // routes of launch_gmm_prefilter
// Constants of the prefilter's error bound (derivation: gmm_prefilter.hip header), by k-steps of 32; the host folds them into grp_lim.
struct PfBound { float kappa, acc, abs, sub; };
constexpr float kPfRes16 = 4.8835e-4f;  // cap of |b^ - b| / |b|: one fp16 rounding of a normal fp32 x^2 or x
inline constexpr PfBound pf_bound(int ks32) {
  return ks32 == 4 ? PfBound{1.05e-3f, 1.6e-5f, 7.0e-7f, 3.38e-7f} : PfBound{1.05e-3f, 1.1e-5f, 6.0e-7f, 2.92e-7f};
}
struct GmmRefineArgs {
  // dim = the PADDED, odd dimension gmm_refine_padded_dim(model dimension): pair dimensions, zeros, the odd tail last (gmm_prefilter.hip)
  const float* feats;           // [n_frames x dim] row-major features in that order (batches of unrelated frames): the corpus' own
                                // rows when its dimension IS dim, else the padded copy launch_transpose_feats writes
  const float* featsT;          // [dim x n_frames_ld] transposed features (main pass: 64 consecutive frames per wave)
  uint64_t n_frames, n_frames_ld;
  uint32_t dim, n_pstates, chunks;  // pseudo-states = states x chunks (a state of up to 32*chunks densities)
  const uint32_t* n_dens_ps;    // [n_pstates] densities in each pseudo-state (0..32)
  const double* rows;           // [state][2*dim + 2 planes][n_slots]: mu_0, 1/var_0, ..., norm, logw per density slot;
                                // 1 KB of slack after the last state
  uint32_t n_slots;             // gmm_refine_slots(max_dens): 8, 16 or 32
  const uint32_t* mask;         // as written by the prefilter
  double* out; uint32_t ld;
  uint64_t frames_per_split;    // set by the launcher
  unsigned long long* n_refined;  // optional: += densities evaluated (profiling)
  uint32_t* ring;               // workspace, gmm_refine_ring_words() u32: wave-private lists of pairs with further candidates
  uint32_t* tickets;            // set by the launcher (the workspace's tail): per workgroup the next 64-frame block to hand out
  // deferred leftovers (mixtures of more than 32 densities, gmm_refine_defer_layout): per wave and panel a segment of defer_cap 16-byte
  // entries + its count; null: the lists are worked off inside the refinement kernel (rounds 2-4)
  void* defer;
  uint32_t* defer_cnt;
  uint32_t defer_cap;
};
// workspace of the deferred-leftover route for this launch: entries per segment (0: the route does not apply -- one chunk per state, a
// padded dimension beyond 39, or more than `budget_bytes`), at most `cap_limit` when that is not 0; total 16-byte entries, total counters
void gmm_refine_defer_layout(const GmmRefineArgs& a, size_t budget_bytes, uint32_t cap_limit, uint32_t* cap, size_t* n_entries,
                             size_t* n_counts);
size_t gmm_refine_ring_words(const GmmRefineArgs& a);  // needs n_frames, n_pstates, dim, n_slots
// the grid launch_gmm_refine gives this shape (same fields): threads per workgroup, pseudo-states per workgroup, frames per workgroup,
// chunks per state -- the workgroup over split y takes frames y * out[2] .. in blocks of 64, one block per wave at a time: on the deferred
// route thread (wave, lane) takes frame y * out[2] + wave * 64 + it * out[0] + lane in iteration it, on every other route a wave draws its
// next block when it starts one (in that order when the waves keep pace)
void gmm_refine_geometry(const GmmRefineArgs& a, uint32_t out[4]);
// route: kPfStaged -- frames stationary, the model streamed through LDS (needs split_begin, nx, ny); kPfStationary -- a 4-state group
// stationary in a wave's registers, the frames' ready-made operands streamed past it (needs n_groups, bfrag, bnorm; builds the
// operands first).  ks32 = 4 has no stationary instantiation (its A operand alone is 128 registers) and takes the staged kernel on
// either route: gmm_prefilter_route() says which kernel a launch runs.  Both routes write the same masks, bit for bit.
hipError_t launch_gmm_prefilter(const GmmPrefilterArgs& a, int ks32, int route, hipStream_t stream);
int gmm_prefilter_route(int ks32, int route);
int gmm_prefilter_frames_per_tile();
// the stationary route cuts the frames into ranges of a multiple of 32 frames; a launch of more frames than this has at least two
int gmm_prefilter_stationary_range_frames();
// entries of bfrag / bnorm for a launch over n_frames on that route
void gmm_prefilter_operand_sizes(int ks32, uint64_t n_frames, size_t* n_frag, size_t* n_norm);
// does the fp16 MFMA keep subnormal inputs on this device / in this build (an assumption of the prefilter's error bound)?
hipError_t probe_fp16_denormals(hipStream_t stream, bool* preserved);
// does the fp16 MFMA chain accumulate within the bound's model (|error| <= 87 (K = 96: ks32 3) / 132 (K = 128: ks32 4) * 2^-24 *
// sum |a_k b_k| on adversarial dot products)?
hipError_t probe_fp16_accumulation(hipStream_t stream, int ks32, bool* ok, double* worst_ratio);
uint32_t gmm_refine_padded_dim(uint32_t dim);               // odd, >= dim; 0: no refinement instantiation (dim > 62)
int gmm_refine_slots(uint32_t max_dens, uint32_t padded_dim);  // density slots per panel: 8, 16 or 32 (always 32 beyond padded dimension 39)
hipError_t launch_gmm_refine(const GmmRefineArgs& a, hipStream_t stream);
// featsT [dp x ldT] in the padded order and, when dp != dim, featsP [n_frames x dp] row-major in the same order (else unused)
hipError_t launch_transpose_feats(const float* feats, uint64_t n_frames, uint32_t dim, uint32_t dp, uint64_t ldT, float* out, float* featsP,
                                  hipStream_t stream);

// ---- beam Viterbi decoder (viterbi_decode.hip) ---------------------------------------------------
// Search network flattened to "slots" = (word, position) pairs in (word, position) order, which is
// the iteration order of the reference's hypothesis array (Recognizer.cpp:126).
struct DecodeNet {
  uint32_t n_slots;             // P
  uint32_t n_words;
  const uint32_t* slot_info;    // [P] emission state (bits 0-15) | the kSlot* flags below
  const uint32_t* slot_word;    // [P] word index of the slot
  const uint32_t* word_end_slot;// [W] slot index of each word's last position
  uint32_t silence_word;
  double tdp_loop, tdp_forward, tdp_skip;
  uint32_t silence_state;
};
static constexpr uint32_t kSlotPos0 = 1u << 16;      // position 0 of its word
static constexpr uint32_t kSlotPos1 = 1u << 17;      // position 1
static constexpr uint32_t kSlotEnd = 1u << 18;       // last position (word end): no in-word expansion
static constexpr uint32_t kSlotSilState = 1u << 19;  // its state is the silence state: tdp is always `forward`
static constexpr uint32_t kSlotSilWord = 1u << 20;   // word is the silence word: no word penalty
static constexpr uint32_t kSlotFirstSil = 1u << 21;  // word's first state is the silence state
static constexpr uint32_t kSlotSingle = 1u << 22;    // one-position word: owns the virtual dead slot (w, 1)
// The same network with slots sorted by type for the fast kernel (viterbi_fast.hip); ids below are positions in
// the sorted order, every type padded to a multiple of 64 slots.
struct FastNet {
  uint32_t n_slots;             // padded total (multiple of 64); 0: not built -- more than decode_max_slots(), a `big` lexicon
  const uint32_t* state;        // [n] emission state of the slot
  const uint32_t* pred;         // [n] sorted id of the slot one position back | two positions back << 16
  const uint32_t* orig;         // [n] original slot index | original index of the word's position 0 << 16; 0xFFFFFFFF = padding
  const uint32_t* chunk_type;   // [n/64] kind | flags (viterbi_fast.hip)
  const uint32_t* word;         // [n] word index of the slot
  uint32_t init_slot;           // sorted id of original slot 0
  uint32_t init_is_end;         // original slot 0 is a word end
};
// The same network word by word for the word-per-lane kernel (viterbi_words.hip): lexica whose words all have <= 4 positions
struct WordNet {
  const uint32_t* info;         // [W] positions (bits 0-2) | silence word (8) | first state is silence (16) | position p's state is silence << (8 + p); null: not built
  const uint2* states;          // [W] emission state of positions 0..3, 16 bits each
  const uint32_t* order;        // [nw * nt] word of lane slot tid + k * nt; every group of 64 slots holds one kind of word, 0xFFFFFFFF = padding
  uint32_t nw, nt;              // words per lane, lanes per workgroup (whole waves)
  uint32_t plain_len;           // positions of a plain word (2, 3 or 4): the commonest length among the words without silence flags
  uint32_t has_general;         // some word is neither plain nor a one-position word
  uint32_t init_is_end;         // word 0 has one position: the initial hypothesis is a word end
};
struct DecodeArgs {
  DecodeNet net;
  FastNet fast;
  WordNet words;
  const double* scores;         // [frames x ld] dense emission costs of this launch's frames
  uint32_t ld;
  const uint64_t* frame_off;    // [n_utts+1] global frame offsets of the corpus
  uint64_t frame_base;          // scores row 0 is global frame `frame_base`
  uint32_t utt_first, n_utts;   // utterances handled by this launch
  const uint32_t* utt_order;    // [n_utts_total] workgroup utt_first + b decodes utterance utt_order[utt_first + b]: the launch's range,
                                // longest first (the tail of a launch is then its shortest utterances); null = identity
  double am_threshold, word_penalty;
  // traceback arrays, entry frame_off[u] + u + t  (t = 0..T_u)
  double* tb_score;
  uint16_t* tb_word;
  uint16_t* tb_bkp;
  uint32_t* out_words;          // utterance u writes its words at out_words[frame_off[u] ...]
  uint32_t* out_count;          // [n_utts_total]
  uint32_t* out_flags;          // [n_utts_total] kFlagSlowPath | kFlagReplay | kFlagCorrupt (traceback.h)
  uint32_t only_flagged;        // the replay kernel redoes only the utterances a fast kernel flagged kFlagReplay (set by launch_decode)
  uint32_t exact_negative;      // the model's emission costs can be negative (some density has norm - log weight < 0): the word-per-lane kernel
                                // runs its NEG variant, which replays the reference's early-out instead of flagging the utterance
};
// The zerogram search of a lexicon: a fast kernel first, if any -- word per lane (viterbi_words.hip) or slot per lane
// (viterbi_fast.hip) --, then the replay kernel -- decode_kernel (LDS) or, for a lexicon without a FastNet, decode_big_kernel
// (hypotheses in device memory) -- on the utterances the fast kernel flagged, or on every utterance when there is none.
enum class DecodeFirst { kNone, kWords, kSlots };
struct DecodeRoute {
  DecodeFirst first;
  bool big;                     // the replay kernel is decode_big_kernel: a workspace of n_utts * decode_big_workspace(P) bytes
};
// from the networks, the model's ld and the search flags (SR_SEARCH_GENERAL_KERNEL, SR_SEARCH_SLOT_KERNEL)
DecodeRoute decode_route(const DecodeArgs& a, bool general, bool slots);
hipError_t launch_decode(DecodeArgs a, const DecodeRoute& r, unsigned char* big_ws, hipStream_t stream);
uint32_t decode_max_slots();          // what the LDS-resident kernels hold
uint32_t decode_big_max_slots();
size_t decode_big_workspace(uint32_t n_slots);
uint32_t decode_words_max_words();
// launch_decode's pieces
hipError_t launch_decode_fast(const DecodeArgs& a, hipStream_t stream);
bool decode_words_applies(const DecodeArgs& a);                          // short-word lexicon whose score rows fit the LDS twice
hipError_t launch_decode_words(const DecodeArgs& a, hipStream_t stream);
// The networks, built on the host beside the kernels that read them from a lexicon of n_words words, word w's emission states
// automaton[word_off[w] .. word_off[w + 1]).  A builder fills the net's scalars and writes its arrays into the vectors;
// sr_lexicon_create uploads those and sets the net's pointers.
DecodeNet build_decode_net(uint32_t n_words, const uint32_t* word_off, const uint16_t* automaton, uint32_t silence_word,
                           uint32_t silence_state, const double tdp[3], std::vector<uint32_t>& slot_info,
                           std::vector<uint32_t>& slot_word, std::vector<uint32_t>& word_end_slot);
FastNet build_fast_net(const std::vector<uint32_t>& slot_info, const std::vector<uint32_t>& slot_word, const uint32_t* word_off,
                       std::vector<uint32_t>& state, std::vector<uint32_t>& pred, std::vector<uint32_t>& orig,
                       std::vector<uint32_t>& chunk_type, std::vector<uint32_t>& word);
WordNet build_word_net(uint32_t n_words, const uint32_t* word_off, const uint16_t* automaton, uint32_t silence_word,
                       uint32_t silence_state, std::vector<uint32_t>& info, std::vector<uint2>& states, std::vector<uint32_t>& order);
// streaming (sr_stream_push): decode_stream_kernel advances each of n open utterances by k frames from the state the last push
// left in device memory.  Per stream slot: decode_big_workspace(P) bytes of hypotheses, a StreamState, max_frames + 1 traceback
// entries (words, not slots) and max_frames words of partial result.
struct StreamState {
  double m_we;            // word-end minimum of the last frame searched (+inf: none survived)
  uint32_t e_first[4];    // first word-end slot attaining it per boundary class, for the next frame
  uint32_t flags;         // kFlagSlowPath | kFlagCorrupt (traceback.h), the latter for the last walk
  uint32_t count;         // words of the partial result, at words + slot * words_stride
  uint32_t pad[2];
};
struct StreamJob {        // one workgroup of a push
  uint32_t slot;          // stream slot
  uint32_t t0, k;         // frames searched before this push, frames in it
  uint32_t pad;
  uint64_t row0;          // its first frame's row in the push's score table
};
struct StreamArgs {
  DecodeNet net;
  double am_threshold, word_penalty;
  const double* scores;   // [push frames x ld]
  uint32_t ld;
  const StreamJob* jobs;  // [workgroups]
  unsigned char* ws;      // [slots x ws_stride]
  size_t ws_stride;
  StreamState* state;     // [slots]
  double* tb_score;       // [slots x tb_stride], entry t = traceback[t]
  uint16_t* tb_word;
  uint16_t* tb_bkp;
  uint64_t tb_stride;     // max_frames + 1
  uint32_t* words;        // [slots x words_stride]
  uint64_t words_stride;  // max_frames
};
hipError_t launch_decode_stream(const StreamArgs& a, uint32_t n_jobs, hipStream_t stream);
// the stable prefix (sr_stream_stable): stream_commit_kernel, one workgroup per requested stream, reads what the last push left
// -- the current buffer's scores and back pointers, the traceback -- and changes none of it.  It folds the back pointers of the
// alive hypotheses into their nearest common ancestor in the traceback (commit_point.h), walks from there (traceback.h) into the
// slot's own word buffer, and copies the words and a StableResult into the call's result block.
static constexpr uint32_t kStableCorrupt = 1u;  // StableResult::flags: a parent not below its child, or the walk failed its guards
struct StableJob {         // one workgroup of a call
  uint32_t slot;           // stream slot
  uint32_t t;              // frames searched so far
  uint32_t fresh;          // no commit point computed for this utterance yet: the floor is 0, commit[slot] is not read
  uint32_t pad;
  uint64_t word_off;       // its words' place in the block's word area (t slots: the walk returns at most one word per frame)
};
struct StableResult {
  uint32_t commit;         // the commit point c(t): a frame
  uint32_t silence;        // trailing silence in frames
  uint32_t count;          // stable words
  uint32_t flags;
};
struct StableArgs {
  DecodeNet net;
  const StableJob* jobs;    // [workgroups]
  const unsigned char* ws;  // [slots x ws_stride]: the search's hypotheses, read only
  size_t ws_stride;
  const uint16_t* tb_word;  // [slots x tb_stride], read only
  const uint16_t* tb_bkp;
  uint64_t tb_stride;
  uint32_t* commit;         // [slots] the previous commit point, carried from call to call
  uint32_t* words;          // [slots x words_stride] the walk's buffer
  uint64_t words_stride;    // max_frames
  StableResult* out_res;    // [workgroups]
  uint32_t* out_words;      // the block's word area
};
hipError_t launch_stream_commit(const StableArgs& a, uint32_t n_jobs, hipStream_t stream);
// the trim (sr_stream_trim): stream_trim_kernel, one workgroup per requested stream, finds the commit point c as stream_commit_kernel
// does (a StableJob; the same floor), hands the words of the walk from c to the call's result block (StableResult::commit = c, the
// frames dropped; ::count, the words; ::silence unused), and renumbers what the search left: traceback entries (c, t] move to
// (0, t - c], the alive hypotheses' back pointers lose c and land in the buffer of parity (t - c) & 1 with their scores, commit[slot]
// becomes 0, and the walk from frame t - c refreshes the slot's partial result.  A result flagged kStableCorrupt has written nothing.
struct TrimArgs {
  DecodeNet net;
  const StableJob* jobs;    // [workgroups]
  unsigned char* ws;        // [slots x ws_stride]: the search's hypotheses
  size_t ws_stride;
  StreamState* state;       // [slots]: flags and count of the partial result
  double* tb_score;         // [slots x tb_stride]
  uint16_t* tb_word;
  uint16_t* tb_bkp;
  uint64_t tb_stride;
  uint32_t* commit;         // [slots]
  uint32_t* walk_words;     // [slots x words_stride] the committed walk's buffer (sr_stream_stable's)
  uint32_t* words;          // [slots x words_stride] the slots' partial results
  uint64_t words_stride;    // max_frames
  StableResult* out_res;    // [workgroups]
  uint32_t* out_words;      // the block's word area
};
hipError_t launch_stream_trim(const TrimArgs& a, uint32_t n_jobs, hipStream_t stream);
// the fold alone (sr_commit_points): set i's nodes set[set_off[i] .. set_off[i + 1]) in the tree parent[node_off[i] ..], out[i] their
// nearest common ancestor (kCommitCorrupt of commit_point.h where a parent is not below its child)
struct CommitPointsArgs {
  const uint64_t* node_off;  // [n_sets + 1]
  const uint32_t* parent;
  const uint64_t* set_off;   // [n_sets + 1]
  const uint32_t* set;
  const uint32_t* floor;     // [n_sets]
  uint32_t* out;             // [n_sets]
};
hipError_t launch_commit_points(const CommitPointsArgs& a, uint32_t n_sets, hipStream_t stream);
// the traceback walk alone (traceback.h) on arrays in the traceback layout above; out_flags[u] = kFlagCorrupt where it does not walk
hipError_t launch_traceback(const uint64_t* frame_off, uint32_t n_utts, const uint16_t* tb_word, const uint16_t* tb_bkp,
                            uint32_t silence_word, uint32_t n_words, uint32_t* out_words, uint32_t* out_count,
                            uint32_t* out_flags, hipStream_t stream);

// ---- compaction of a search's words into one result block (gather_words.hip) -----------------------
constexpr uint32_t kGatherNone = 0xFFFFFFFFu;
constexpr int kGatherMaxArrays = 3;
struct GatherHeader {       // the head of the block: what the host checks before it copies
  uint64_t n_words;         // all utterances' words (a count beyond its slots counted as the slots)
  uint32_t first_flagged;   // the first utterance with flags & flag_mask, kGatherNone: none
  uint32_t first_over;      // the first utterance with more words than slots, kGatherNone: none ...
  uint32_t over_count;      // ... and its count
  uint32_t reserved[3];
};
static_assert(sizeof(GatherHeader) == 32, "word_off follows the header, 8-byte aligned");
struct GatherArgs {
  const uint32_t* count;      // [n_utts]
  const uint32_t* flags;      // [n_utts]
  const uint64_t* frame_off;  // [n_utts+1]; utterance u owns slots frame_off[u] + u * extra_slots .. of each array, T_u + extra_slots of them
  uint32_t n_utts, extra_slots, flag_mask;
  const uint32_t* src[kGatherMaxArrays];  // arrays of 32-bit elements, moved as bits
  uint64_t* dev_off;          // [n_utts+1] workspace: the offsets for the second launch
  unsigned char* block;       // GatherHeader, word_off[n_utts+1] (uint64), then n_arrays runs of n_words elements; gather_block_bytes()
};
size_t gather_block_bytes(uint32_t n_utts, uint64_t n_slots, int n_arrays);  // n_slots: all utterances' slots, the most n_words can be
hipError_t launch_gather_words(const GatherArgs& a, int n_arrays, hipStream_t stream);

// ---- forced aligners (viterbi_align.hip) ----------------------------------------------------------
struct AlignArgs {
  const double* scores;         // [frames x ld]
  uint32_t ld;
  const uint64_t* frame_off;    // [n_utts+1]
  uint64_t frame_base;
  uint32_t utt_first, n_utts;
  const uint32_t* utt_order;    // as in DecodeArgs
  const uint16_t* automata;     // concatenated reference automata
  const uint64_t* aut_off;      // [n_utts_total+1]
  double tdp_loop, tdp_forward, tdp_skip;
  uint32_t silence_state;
  double pruning_threshold;     // pruned variant only
  uint8_t* backptr;             // workspace: [sum_u T_u * N_u] taken transition (0/1/2, 3 = none)
  const uint64_t* bp_off;       // [n_utts_total+1] offsets into backptr
  uint32_t max_positions;       // max N_u over the launch (sizes the LDS cost buffers)
  uint16_t* out_states;         // [total frames]
  double* out_cost;             // [n_utts_total]
};
hipError_t launch_align_full(const AlignArgs& a, hipStream_t stream);
hipError_t launch_align_pruned(const AlignArgs& a, hipStream_t stream);
uint32_t align_max_positions();
// The LDS bytes of an aligner launch whose longest automaton has max_positions positions -- the kernels' layouts: cost[2][N] f64 and
// ref[N] u16; the pruned kernel's alive[2][N] u8 and red[4] f64 beside them; 16 for the alignment of the base -- against the 160 KiB
// a workgroup can have (gfx950).  The launchers size their launches with these, align_common refuses what does not fit.
constexpr size_t kAlignLdsLimit = 160 * 1024;
constexpr size_t align_full_lds_bytes(uint32_t max_positions) { return (size_t)max_positions * (2 * 8 + 2) + 16; }
constexpr size_t align_pruned_lds_bytes(uint32_t max_positions) { return (size_t)max_positions * (2 * 8 + 2 + 2) + 4 * 8 + 16; }
constexpr uint32_t kAlignMaxPositions = 8192;        // align_max_positions(): sr_align_corpus, the forward-backward passes
constexpr uint32_t kAlignPrunedMaxPositions = 8189;  // sr_align_corpus_pruned: 20 bytes a position
static_assert(align_full_lds_bytes(kAlignMaxPositions) <= kAlignLdsLimit, "align_full_kernel at the position limit");
static_assert(align_pruned_lds_bytes(kAlignPrunedMaxPositions) <= kAlignLdsLimit &&
              align_pruned_lds_bytes(kAlignPrunedMaxPositions + 1) > kAlignLdsLimit, "align_pruned_kernel at the position limit");

// ---- forward-backward over the aligner's automata and topology (viterbi_fb.hip) --------------------------------------
// A launch covers utterances [utt_first, utt_first + n_utts) of one score chunk whose trellises fit the workspace together.
struct FbArgs {
  const double* scores;         // [frames x ld], row 0 = frame frame_base (as AlignArgs)
  uint32_t ld;
  uint64_t frame_base;
  const uint64_t* frame_off;    // [n_utts_total+1]
  uint32_t utt_first, n_utts;
  const uint16_t* automata;     // concatenated automata
  const uint64_t* aut_off;      // [n_utts_total+1]
  double tdp_loop, tdp_forward, tdp_skip;
  uint32_t silence_state;
  uint32_t max_positions;       // max N_u over the launch (sizes the LDS)
  double* trellis;              // workspace: [T_u][N_u] per utterance at trellis_off[u] - trellis_off[utt_first]; alpha, then gamma
  const uint64_t* trellis_off;  // [n_utts_total+1] prefix sums of T_u * N_u
  double* out_cost;             // [n_utts_total] forward cost F_u
};
hipError_t launch_fb_forward(const FbArgs& a, hipStream_t stream);
hipError_t launch_fb_backward(const FbArgs& a, hipStream_t stream);

// ---- the items of a training pass (posterior_items.hip) ------------------------------------------------------------------------
// Items (frame, mixture, weight) from a trellis of per-position weights, in frame order then ascending mixture id: the weight of a
// mixture is the sum over the positions that carry it.  Either per-utterance trellises [T_u][N_u] with a mixture list each (chains:
// trellis_off, chain_off and mix_off set), or rows of row_stride doubles per frame of the launch and one list for every utterance.
struct ItemArgs {
  const uint64_t* frame_off;    // [n_utts_total+1]
  uint32_t utt_first, n_utts;
  uint64_t group_f0;            // first frame of the launch
  const double* trellis;
  const uint64_t* trellis_off;  // chains: [n_utts_total+1] prefix sums of T_u * N_u, utterance u at trellis_off[u] - trellis_off[utt_first]
  const uint64_t* chain_off;    // chains: [n_utts_total+1] prefix sums of N_u (FbArgs::aut_off, ChainArgs::chain_off)
  uint32_t n_cols, n_mix;       // rows: positions, distinct mixtures
  uint32_t row_stride;          // rows: doubles between the rows (the weights are the first n_cols), frame f at (f - group_f0) * row_stride
  uint32_t serial_limit;        // 0: a lane sums every mixture alone, in position order; else one of more positions is summed wave-wide
  const uint32_t* mix_off;      // chains: [n_utts_total+1] range of utterance u in mix[] / slot_beg[]
  const uint16_t* mix;          // distinct mixtures, ascending
  const uint32_t* slot_beg;     // positions of mixture j: slot_pos[slot_beg[j] .. slot_beg[j+1])
  const uint16_t* slot_pos16;   // positions grouped by mixture, ascending within: exactly one of the two widths is set
  const uint32_t* slot_pos32;
  const double* gate;           // optional [n_utts_total]: an utterance whose gate is +inf gives no items
  bool by_frame;                // chains of few mixtures (16-bit, no gate, sign +1): a thread instead of a wave per frame; the same items
  double floor;                 // items: weight > 0 and >= floor (launch_items' sign)
  uint32_t* group_cnt;          // [frames of the launch] items per frame (count pass)
  const uint32_t* group_scan;   // [frames of the launch] exclusive prefix sum of group_cnt (write pass; set by launch_items)
  uint32_t* item_base;          // device scalar: items written so far
  uint32_t* item_off;           // [n_frames_total+1] first item of each frame
  uint32_t* item_frame; uint16_t* item_mix; double* item_w;
};
// items of the launch's frames (count pass, device scan, write pass), appended at *item_base; scan_temp from items_scan_temp_bytes.
// sign = +1 / -1: the items with sign * sum > 0 and >= floor, weight sign * sum; 0: sum != 0 and |sum| >= floor, weight sum
size_t items_scan_temp_bytes(uint64_t n_frames);
hipError_t launch_items(const ItemArgs& a, int sign, uint64_t n_frames, void* scan_temp, size_t scan_temp_bytes, uint32_t* scan_out,
                        hipStream_t stream);
// per frame the max_items items of largest |weight| (ties: smaller mixture id first), the weights signed; entries past out_count are zero
hipError_t launch_items_top(const uint32_t* item_off, const uint16_t* item_mix, const double* item_w, uint64_t n_frames,
                            uint32_t max_items, uint16_t* out_count, uint16_t* out_state, double* out_weight, hipStream_t stream);

// ---- forward-backward over the recognition network (viterbi_netfb.hip) ------------------------------------------------
// A launch covers utterances [utt_first, utt_first + n_utts) of one score chunk whose trellises fit the workspace together.
struct NetFbArgs {
  DecodeNet net;                // the lexicon's slot tables (build_decode_net); n_slots <= netfb_max_slots()
  const double* scores;         // [frames x ld], row 0 = frame frame_base (as DecodeArgs)
  uint32_t ld;
  uint64_t frame_base;
  const uint64_t* frame_off;    // [n_utts_total+1]
  uint32_t utt_first, n_utts;
  double scale, word_penalty;   // kappa > 0 multiplies every cost
  uint64_t group_f0;            // first frame of the launch
  double* trellis;              // [frames of the launch][P]: alpha, then gamma
  double* out_cost;             // [n_utts_total] kappa F_u
  double* post;                 // [frames of the launch][W] word posteriors p_t(w)
  double* ends;                 // [frames of the launch] the word-end sums E_t, kept for netocc_backward_kernel; null: not kept
};
size_t netfb_max_slots();
hipError_t launch_netfb_forward(const NetFbArgs& a, hipStream_t stream);
hipError_t launch_netfb_backward(const NetFbArgs& a, hipStream_t stream);
hipError_t launch_netfb_words(const NetFbArgs& a, uint64_t n_frames, hipStream_t stream);
// per frame of the launch the max_items largest p_t(w) > 0 and >= floor (ties: smaller word first), at out_*[corpus frame]; entries
// past out_count are zero
hipError_t launch_netfb_top(const NetFbArgs& a, uint64_t n_frames, uint32_t max_items, double floor, uint16_t* out_count,
                            uint32_t* out_word, double* out_weight, hipStream_t stream);
// the recognised words of the launch's utterances (decoder traceback in DecodeArgs' layout, out_count from its walk): frames and
// max p_t(word) over them at out_*[frame_off[u] + k]
hipError_t launch_netfb_conf(const NetFbArgs& a, const uint16_t* tb_word, const uint16_t* tb_bkp, const uint32_t* out_count,
                             double* out_conf, uint32_t* out_first, uint32_t* out_last, hipStream_t stream);

// ---- MMI training over the recognition network (viterbi_mmi.hip) ------------------------------------------------------------------
// netfb_backward_kernel's twin that leaves mixture-occupancy parts instead of gamma in the trellis (a.ends = the E_t of the forward pass)
hipError_t launch_netocc_backward(const NetFbArgs& a, hipStream_t stream);
// The network restricted to a transcript: utterance u's chain of segments sil_0 w_1 sil_1 .. w_n sil_n, its positions at
// chain_off[u] .. chain_off[u + 1] (at most netfb_max_slots()).  A launch covers utterances [utt_first, utt_first + n_utts) of one score
// chunk whose trellises fit the workspace together.
struct ChainArgs {
  const double* scores;         // [frames x ld], row 0 = frame frame_base (as DecodeArgs)
  uint32_t ld;
  uint64_t frame_base;
  const uint64_t* frame_off;    // [n_utts_total+1]
  uint32_t utt_first, n_utts;
  double scale, word_penalty;   // as NetFbArgs
  double tdp_loop, tdp_forward, tdp_skip;
  const uint64_t* chain_off;    // [n_utts_total+1]
  const uint32_t* info;         // per chain position: the slot_info of its lexicon slot
  const uint32_t* src;          // positions 0 and 1 of a segment: the (up to two) word ends that enter it, chain position | chain position << 16, 0xFFFF = none
  const uint32_t* dst;          // word ends: position 0 of the (up to two) segments they enter, packed the same way
  uint32_t sil_len;             // positions of the silence word: the word end of w_n is that far before the chain's last position
  uint32_t max_positions;       // longest chain of the launch (sizes the LDS)
  double* trellis;              // [T_u][N_u] per utterance at trellis_off[u] - trellis_off[utt_first]: alpha, then the occupancy parts
  const uint64_t* trellis_off;  // [n_utts_total+1] prefix sums of T_u * N_u
  double* out_cost;             // [n_utts_total] kappa F_u
};
hipError_t launch_chain_forward(const ChainArgs& a, hipStream_t stream);
hipError_t launch_chain_backward(const ChainArgs& a, hipStream_t stream);
// Extended Baum-Welch: numerator and denominator statistics (accumulator rows as EmArgs) + the old tables -> new means, variances and
// inverse variances per density
struct EbwArgs {
  uint64_t n_dens;
  uint32_t dim;
  const uint32_t* dens_mean; const uint32_t* dens_var;
  const double* old_means; const double* old_inv_vars;  // [C x dim]
  const double *num_mean_acc, *num_mean_w, *num_var_acc, *den_mean_acc, *den_mean_w, *den_var_acc;
  double E, tau, var_floor;
  double* means; double* vars; double* inv_vars;          // [C x dim]
};
hipError_t launch_ebw_combine(const EbwArgs& a, hipStream_t stream);

// ---- sMBR training over the recognition network (viterbi_smbr.hip) ----------------------------------------------------------------
// NetFbArgs' launch with the expected frame accuracy beside every cost.
struct SmbrArgs {
  DecodeNet net;                // the lexicon's slot tables; n_slots <= smbr_max_slots()
  const double* scores;         // [frames x ld], row 0 = frame frame_base (as DecodeArgs)
  uint32_t ld;
  uint64_t frame_base;
  const uint64_t* frame_off;    // [n_utts_total+1]
  uint32_t utt_first, n_utts;
  double scale, word_penalty;   // as NetFbArgs
  uint64_t group_f0;            // first frame of the launch
  const uint16_t* ref;          // [n_frames_total] the reference mixture of every frame; >= the state count: none
  double* trellis;              // [frames of the launch][2][P]: (alpha, abar), then the signed parts over alpha
  double* ends;                 // [frames of the launch][2]: the word-end sum E_t and its expected accuracy
  double* out_cost;             // [n_utts_total] kappa F_u
  double* out_acc;              // [n_utts_total] Abar_u
};
size_t smbr_max_slots();
hipError_t launch_smbr_forward(const SmbrArgs& a, hipStream_t stream);
hipError_t launch_smbr_backward(const SmbrArgs& a, hipStream_t stream);

// ---- word lattices over the recognition network (viterbi_lattice.hip) --------------------------------------------------
// A launch covers utterances [utt_first, utt_first + n_utts) of one score chunk whose word-end tables fit the workspace together.
struct LatticeArgs {
  DecodeNet net;                // the lexicon's slot tables; n_slots <= lattice_max_slots()
  const double* scores;         // [frames x ld], row 0 = frame frame_base (as DecodeArgs)
  uint32_t ld;
  uint64_t frame_base;
  const uint64_t* frame_off;    // [n_utts_total+1]
  uint32_t utt_first, n_utts;
  double word_penalty, beam;    // beam >= 0 (+inf: every arc on a complete path)
  uint64_t group_f0;            // first frame of the launch
  double* fwd;                  // [frames of the launch][W] A_t(end slot of w)
  uint16_t* first;              // [frames of the launch][W] the frame at which that path entered w
  double* ends;                 // [frames of the launch] E_t = min over w of fwd
  double* bend;                 // [frames of the launch] Bend_t
  double* out_best;             // [n_utts_total] E_{T-1} (+inf for T = 0)
  uint32_t *arc_word, *arc_first, *arc_last;  // the compacted arcs (null: count only)
  double *arc_fwd, *arc_bwd, *arc_cost;
};
size_t lattice_max_slots();
hipError_t launch_lattice_forward(const LatticeArgs& a, hipStream_t stream);
hipError_t launch_lattice_backward(const LatticeArgs& a, hipStream_t stream);
size_t lattice_scan_temp_bytes(uint64_t n_frames);
// after forward and backward: cnt / scan [n_frames] workspace; the launch's arcs go to arc_*[arc_base[0] + ...] (only below cap),
// frame_arc[corpus frame] = the position of the frame's first arc, arc_base[0] += the launch's arcs
hipError_t launch_lattice_emit(const LatticeArgs& a, uint64_t n_frames, void* scan_temp, size_t scan_temp_bytes, uint64_t* cnt,
                               uint64_t* scan, uint64_t* arc_base, uint64_t* frame_arc, uint64_t cap, hipStream_t stream);

// ---- bigram-LM beam search over a linear lexicon (viterbi_bigram.hip; Teaching::LinearSearch) -----------------------
struct BigramArgs {
  const double* scores;         // [frames x ld]
  uint32_t ld;
  const uint64_t* frame_off;    // [n_utts_total+1]
  uint64_t frame_base;
  uint32_t utt_first, n_utts;
  const uint32_t* utt_order;    // as in DecodeArgs
  uint32_t n_words, silence, n_positions;  // W; silence word; sum of state counts over the 2W slots (words + silence copies)
  const uint32_t* slot_off;     // [2W+1] first dense position of every slot
  const uint32_t* slot_mix;     // [2W] offset of the slot's acoustic word in `mixtures`
  const uint16_t* mixtures;     // emission state per lexicon position
  const uint32_t* pos_info;     // [n_positions] per dense position (slots back to back): emission state | flags << 16
                                //   flags: 1 = first state of its slot, 2 = second, 4 = last, 8 = silence (copy)
  const uint32_t* pos_slot;     // [n_positions] its slot
  const float* lmT;             // [W x W] transposed: lmT[h*W + w] = -log p(w | h)
  const float *lm_rowmin, *lm_rowmax;  // [W] min / max over w != silence of lmT[h][w]
  float tdp[2][4];              // [isSilence][loop, forward, skip, exit]
  float ac_pruning, lm_pruning; // >= FLT_MAX: off
  uint32_t *we_slot, *we_bp; float* we_score;  // workspace [n_utts][2][2W]
  uint4* book;                  // traceback book; utterance u owns [book_off[u], book_off[u+1])
  const uint64_t* book_off;     // [n_utts_total+1]
  uint32_t* out_word; float* out_score; uint32_t* out_time;  // [frames + utts]: utterance u at frame_off[u] + u
  uint32_t *out_count, *out_flags;  // [n_utts_total]; flag 1 = book capacity exceeded
  uint32_t max_slot_states;     // most states of any slot
  uint32_t silence_states;      // states of the silence word (= of every silence copy)
  uint32_t dense_states;        // keep the state hypotheses in the dense LDS image even where the register layout applies
  uint32_t row4_mask;           // register layout: bit k = slot row k (words k * 1024 ...) holds a word of four states (the other rows keep three)
  uint32_t global_states;       // keep the state hypotheses in device memory (bigram_gs_kernel) even where another layout applies
  uint32_t gs_grid;             // global states: workgroups of the persistent grid (each decodes every gs_grid-th utterance)
  uint32_t* gs_ws;              // global states: [gs_grid][gs_ws_words] workspace, the state image of every workgroup
  uint64_t gs_ws_words;         //   >= bigram_gs_ws_words(n_words, n_positions)
  unsigned long long* gs_active;  // global states, optional: += the positions step 3 visits, every frame
};
// bigram_route.h: BigramLayout, BigramRoute, bigram_route() -- the one place that chooses the kernel -- and the LDS / workspace size
// formulas (bigram_lds_bytes, bigram_gs_ws_words)
BigramRoute bigram_route_of(const BigramArgs& a);  // what launch_bigram runs for these arguments (n_words .. global_states, ld)
inline BigramLayout bigram_layout(const BigramArgs& a) { return bigram_route_of(a).layout; }
uint32_t bigram_max_positions();
hipError_t launch_bigram(const BigramArgs& a, hipStream_t stream);
uint32_t bigram_max_words();
// The search net, built on the host beside the kernels that read it (as build_decode_net) from a lexicon of n_words words, word w's
// emission states mixtures[word_off[w] .. word_off[w + 1]), the dense [W x W] table lm[w * W + h] = -log p(w | h) and tdp
// [isSilence][loop, forward, skip, exit].  Returns a BigramArgs with only the network's scalars set (n_words, silence, n_positions, tdp,
// max_slot_states, silence_states, row4_mask) and writes its arrays into the vectors; sr_bigram_create uploads those and mixtures and
// sets the pointers.
BigramArgs build_bigram_net(uint32_t n_words, const uint32_t* word_off, const uint16_t* mixtures, uint32_t silence_word, const float* lm,
                            const float tdp[8], std::vector<uint32_t>& slot_off, std::vector<uint32_t>& slot_mix,
                            std::vector<uint32_t>& pos_info, std::vector<uint32_t>& pos_slot, std::vector<float>& lmT,
                            std::vector<float>& lm_rowmin, std::vector<float>& lm_rowmax);
// streaming (sr_bigram_stream_push): bigram_stream_kernel advances each of n open utterances by k frames on the global-states layout,
// from the state the last push left in device memory.  Per stream slot: the state image (a.gs_ws, bigram_gs_ws_words each), the two
// word-end lists (a.we_*, 2 x 2W entries each), the active list (lsave, 2W), a BigramStreamState, the book (its own allocation, grown by
// the host between pushes; back pointers are indices into it) and items_stride partial-result items.
static constexpr uint32_t kBgStreamOverflow = 1u, kBgStreamCorrupt = 2u;  // BigramStreamState::flags
struct BigramStreamState {
  uint32_t n_book, n_we, n_L;  // book entries, word ends of the last frame, slots on the active list
  uint32_t lcur, gs_cur;       // which half of the active-list double buffer / of the image holds the current hypotheses
  uint32_t flags;              // kBgStreamOverflow: an append would have passed book_cap; kBgStreamCorrupt: the partial walk failed
  uint32_t count;              // items of the partial result
  uint32_t pad;
};
struct BigramStreamJob {       // one workgroup of a push
  uint32_t slot, t0, k, pad;   // stream slot, frames searched before this push, frames in it
  uint64_t row0;               // its first frame's row in the push's score table
  uint4* book;                 // the slot's book and its capacity (entries)
  uint64_t book_cap;
};
struct BigramStreamArgs {
  BigramArgs a;                // lexicon, LM, penalties, beams, scores = the push's table; gs_ws, we_* per slot (frame_off etc. unused)
  const BigramStreamJob* jobs; // [workgroups]
  BigramStreamState* state;    // [slots]
  uint16_t* lsave;             // [slots x 2W] the active list between pushes
  uint32_t* out_word; float* out_score; uint32_t* out_time;  // [slots x items_stride] the partial result
  uint64_t items_stride;       // max_frames + 1
};
hipError_t launch_bigram_stream(const BigramStreamArgs& s, uint32_t n_jobs, hipStream_t stream);
// the stable prefix (sr_bigram_stream_stable): bigram_stream_commit_kernel, one workgroup per requested stream, reads what the last
// push left -- the state record, the saved active list, the image's current buffer, the merged word-end list, the book -- and changes
// none of it.  The nearest common ancestor (commit_point.h; parent(b) = book[b].z) of the entries a later word end can start from is
// the commit entry; the items from the start entry to it go straight into the call's result block (StableResult::commit = its time).
struct BigramStableJob {       // one workgroup of a call
  uint32_t slot, t, fresh, pad;  // stream slot, frames searched so far, no commit entry computed for this utterance yet
  const uint4* book;           // the slot's book (NULL while t == 0)
  uint64_t item_off;           // its items' place in each of the block's three item areas (t slots: an item steps back a frame at least)
};
struct BigramStableArgs {
  uint32_t n_words, silence, n_positions;
  const uint32_t* slot_off;    // [2W + 1]
  const uint32_t* gs_ws;       // [slots x gs_ws_words], read only
  uint64_t gs_ws_words;
  const uint32_t* we_bp;       // [slots x 2 x 2W], read only: list 0 is the merged one
  const uint16_t* lsave;       // [slots x 2W]
  const BigramStreamState* state;  // [slots]
  const BigramStableJob* jobs; // [workgroups]
  uint32_t* commit;            // [slots] the previous commit entry (a book index), carried from call to call
  StableResult* out_res;       // [workgroups]
  uint32_t* out_word; float* out_score; uint32_t* out_time;  // the block's item areas
};
hipError_t launch_bigram_stream_commit(const BigramStableArgs& a, uint32_t n_jobs, hipStream_t stream);

// ---- forward-backward over the bigram search network (viterbi_bigram_fb.hip) -------------------------------------------------------
// A launch group = utterances of one score chunk whose trellises fit the workspace together, walked frame by frame: `order` lists them
// longest first, so the n_alive utterances with more than t frames are its first entries.  Per utterance of the group (index j in
// `order`) the vectors vec / prod / wend [Kp] and m, Kp = bgfb_padded(W); vec has rows up to the next multiple of 64.
struct BgFbArgs {
  uint32_t n_words, silence, n_positions, Kp;
  const uint32_t *slot_off, *pos_info, *pos_slot;  // the search net's tables (BigramArgs)
  const float* lmT;             // [W x W] as BigramArgs (frame 0 is entered from the silence history alone)
  float tdp[2][4];
  double scale;                 // kappa > 0 multiplies every cost
  const double* scores;         // [frames x ld], row 0 = frame frame_base
  uint32_t ld;
  uint64_t frame_base;
  const uint64_t* frame_off;    // [n_utts_total+1]
  const uint32_t* order;        // [n_group] the group's utterances, longest first
  uint32_t n_group, n_alive, t; // utterances of the group / with more than t frames; the frame index of this launch
  uint64_t group_f0;            // first frame of the group
  double* trellis;              // [frames of the group][n_positions]: alpha, then gamma
  double* vec;                  // forward a[h, u] = exp(m_u - hist_h); backward b[w, u] = exp(m_u - entry cost of word w)
  double* prod;                 // the product's result X[w, u] / Y[h, u]
  double* wend;                 // forward: the word-end cost of word h itself; backward: the entry cost of its copy (silence: of itself)
  double* m;                    // [n_group] the offset of vec
  double* xb;                   // [2][n_group][n_positions] kappa e_t + beta_t of the last two frames
  double* out_cost;             // [n_utts_total] kappa F_u
  double* post;                 // [frames of the group][W] word posteriors
};
inline uint32_t bgfb_padded(uint32_t n_words) { return (n_words + 63u) & ~63u; }
// lk[w][h] = exp(-kappa lm[w, h]) (0: NaN, +inf, the silence row, padding) and its transpose, both [Kp x Kp]
hipError_t launch_bgfb_table(const float* lmT, uint32_t W, uint32_t Kp, uint32_t silence, double kappa, double* lk, double* lkT,
                             hipStream_t stream);
hipError_t launch_bgfb_forward(const BgFbArgs& a, hipStream_t stream);   // frame a.t of the first a.n_alive utterances
hipError_t launch_bgfb_backward(const BgFbArgs& a, hipStream_t stream);
// out[n][m] = sum_k table[m][k] v[n][k], n < n_alive (v_mfma_f64_16x16x4_f64; fixed summation order)
hipError_t launch_bgfb_product(const double* table, const double* v, double* out, uint32_t Kp, uint32_t n_alive, hipStream_t stream);
hipError_t launch_bgfb_words(const BgFbArgs& a, uint64_t n_frames, hipStream_t stream);
// per item of the search's result (BigramArgs' out_* layout) the max of p_t(word) over its frames, at out_conf[frame_off[u] + u + i]
hipError_t launch_bgfb_conf(const BgFbArgs& a, uint32_t n_utts, const uint32_t* it_word, const uint32_t* it_time,
                            const uint32_t* it_count, double* out_conf, hipStream_t stream);

// ---- MMI training over the bigram search network (viterbi_bigram_mmi.hip) ----------------------------------------------------------
// The network restricted to a transcript w_1 .. w_n: utterance u's chain of segments S w_1 c_1 .. w_n c_n (S = the silence word, c_i =
// the silence copy after w_i), its positions at chain_off[u] .. chain_off[u + 1] (at most bgchain_max_positions()).  A launch covers
// utterances [utt_first, utt_first + n_utts) of one score chunk whose trellises fit the workspace together.
struct BgChainArgs {
  const double* scores;         // [frames x ld], row 0 = frame frame_base
  uint32_t ld;
  uint64_t frame_base;
  const uint64_t* frame_off;    // [n_utts_total+1]
  uint32_t utt_first, n_utts;
  double scale;                 // kappa
  float tdp[2][4];              // as BgFbArgs
  const uint64_t* chain_off;    // [n_utts_total+1]
  const uint32_t* info;         // per chain position: the pos_info of its position in the search net
  const uint32_t* src;          // first and second state of a segment: the (up to two) word ends that enter it, chain position | chain position << 16,
                                // 0xFFFF = none; the start's word end counts as that of S (the low half of S' and w_1's link)
  const uint32_t* dst;          // word ends: the first state of the (up to two) segments they enter, packed the same way
  const double* lmc;            // first and second state of a segment: kappa lm of the entry (0: S and the copies; +inf: forbidden)
  uint32_t sil_len;             // states of the silence word: the word end of w_n is that far before the chain's last position
  uint32_t max_positions;       // longest chain of the launch (sizes the LDS and the workgroup)
  double* trellis;              // [T_u][N_u] per utterance at trellis_off[u] - trellis_off[utt_first]: alpha, then gamma
  const uint64_t* trellis_off;  // [n_utts_total+1] prefix sums of T_u * N_u
  double* out_cost;             // [n_utts_total] kappa F_u
};
inline uint32_t bgchain_max_positions() { return 8192; }
hipError_t launch_bgchain_forward(const BgChainArgs& a, hipStream_t stream);
hipError_t launch_bgchain_backward(const BgChainArgs& a, hipStream_t stream);

// ---- sMBR training over the bigram search network (viterbi_bigram_smbr.hip) --------------------------------------------------------
// BgFbArgs' launch with the expected frame accuracy beside every cost: the trellis has rows [alpha[P], abar[P]] (2 n_positions doubles
// per frame; the signed gamma goes over alpha), vec / prod / wend two rows [Kp] per utterance (index j: rows 2 j and 2 j + 1, the
// second the accuracy side; vec has rows up to the next multiple of 64), xb is [2][n_group][2][n_positions].  post is unused.
struct BgSmbrArgs {
  BgFbArgs fb;
  const uint16_t* ref;          // [n_frames_total] the reference mixture of every frame; >= the state count: none
  double* out_acc;              // [n_utts_total] Abar_u
};
hipError_t launch_bgsmbr_forward(const BgSmbrArgs& a, hipStream_t stream);   // frame a.fb.t of the first a.fb.n_alive utterances
hipError_t launch_bgsmbr_backward(const BgSmbrArgs& a, hipStream_t stream);

// ---- word lattices over the bigram search network (viterbi_bigram_lattice.hip) -----------------------------------------------------
// The launch groups are BgFbArgs' (utterances [utt_first, utt_first + n_group) of one score chunk, `order` = longest first); what a
// group keeps are the word ends per (frame, slot): fwd, bwd, first, pred [frames of the group][2W].
struct BgLatArgs {
  uint32_t n_words, silence, n_positions, Kp;
  const uint32_t *slot_off, *pos_info, *pos_slot;  // the search net's tables (BigramArgs)
  const float* lmT;             // [W x W] as BigramArgs
  float tdp[2][4];
  const double* scores;         // [frames x ld], row 0 = frame frame_base
  uint32_t ld;
  uint64_t frame_base;
  const uint64_t* frame_off;    // [n_utts_total+1]
  const uint32_t* order;        // [n_group] the group's utterances, longest first
  uint32_t utt_first, n_group, n_alive, t;  // n_alive: utterances with more than t frames; t: the frame index of this launch
  uint64_t group_f0;            // first frame of the group
  double beam;                  // >= 0 (+inf: every arc on a complete path)
  double *fwd, *bwd;            // [frames of the group][2W] WE_t(x); the cheapest continuation from that word end
  uint16_t* first;              // [frames of the group][2W] the frame at which the cheapest path to the word end entered the slot
  uint32_t* pred;               // [frames of the group][2W] the history it was entered from
  double *vec, *prod, *wend;    // per utterance of the group [Kp]: the min-plus entry's operand and result; backward: the entry cost of
                                // the word's own copy (silence: of itself)
  uint32_t* arg;                // [Kp] per utterance: the entry's arg-min history
  double* row;                  // [2][n_group][n_positions] forward: the cost rows of two frames; backward: e_t + beta_t
  uint16_t* row_first;          // [2][n_group][n_positions] forward: first / pred beside the cost
  uint32_t* row_pred;
  double* out_best;             // [n_utts_total] min over x of WE_{T-1}(x) (preset to 0: T = 0)
  uint32_t *arc_word, *arc_hist, *arc_pred, *arc_first, *arc_last;  // the compacted arcs (arc_word null: count only)
  double *arc_fwd, *arc_bwd, *arc_am;
};
hipError_t launch_bglat_transpose(const float* in, uint32_t W, float* out, hipStream_t stream);  // out[h * W + w] = in[w * W + h]
hipError_t launch_bglat_init(const BgLatArgs& a, uint32_t rows, hipStream_t stream);  // vec rows: the histories before frame 0
// out[n][i] = min_k (vec[n][k] + (double) tab[k * W + i]) for n < n_alive, i < Kp; arg (null: not wanted) = the smallest such k.
// argmin: 0 = compare-and-select in the loop, 1 = a min-only loop and an equality rescan (the same bits)
hipError_t launch_bglat_entry(const float* tab, const double* vec, double* out, uint32_t* arg, uint32_t W, uint32_t Kp, uint32_t n_alive,
                              int argmin, hipStream_t stream);
hipError_t launch_bglat_forward(const BgLatArgs& a, hipStream_t stream);   // frame a.t of the first a.n_alive utterances
hipError_t launch_bglat_backward(const BgLatArgs& a, hipStream_t stream);
// as launch_lattice_emit, 2W slots per frame
hipError_t launch_bglat_emit(const BgLatArgs& a, uint64_t n_frames, void* scan_temp, size_t scan_temp_bytes, uint64_t* cnt, uint64_t* scan,
                             uint64_t* arc_base, uint64_t* frame_arc, uint64_t cap, hipStream_t stream);

// out[f] = scores[(f - frame_base) * ld + states[f]] for f in [f0, f1)  (Trainer::calc_am_score, Training.cpp:605)
hipError_t launch_path_scores(const double* scores, uint32_t ld, uint64_t frame_base, uint64_t f0, uint64_t f1,
                              const uint16_t* states, double* out, hipStream_t stream);

// ---- EM accumulation (em_accumulate.hip) ------------------------------------------------------------------------
struct EmArgs {
  const float* feats;
  uint64_t n_frames, n_pairs;
  uint32_t dim;
  const uint16_t* states;      // [n_frames] aligned mixture per frame
  const uint64_t* pair_off;    // [n_frames] first pair of each frame
  const uint32_t* dens_off;    // model (per density, mixture order)
  const double* means; const double* inv_vars; const double* norm; const double* logw;
  const uint32_t* dens_mean; const uint32_t* dens_var;  // accumulator row of each density
  uint32_t n_mean, n_var;
  int first_pass, max_approx;
  uint32_t* pair_frame; double* pair_w; uint32_t* key_mean; uint32_t* key_var;  // [n_pairs] workspace
  uint32_t* pair_dens;         // optional [n_pairs]: the density of each pair (fMLLR statistics; a dropped pair's keys are 0xFFFFFFFF)
  // posterior-weighted pairs (Baum-Welch): item i = (item_frame[i], mixture item_mix[i], gamma item_w[i]); its pairs end at item_pair_end[i]
  uint64_t n_items;
  const uint32_t* item_frame; const uint16_t* item_mix; const double* item_w;
  uint64_t* item_pair_end;
};
size_t em_sort_temp_bytes(uint64_t n_pairs);
// out[t] = score(frame t, a.states[t]); uses feats, n_frames, dim, states, dens_off, means, inv_vars, norm, logw, max_approx
hipError_t launch_path_scores_direct(const EmArgs& a, double* out, hipStream_t stream);
hipError_t launch_em_accumulate(const EmArgs& a, void* sort_temp, size_t sort_temp_bytes, uint32_t* iota, uint32_t* keys_sorted,
                                uint32_t* pairs_sorted, uint32_t* row_begin /* [max(n_mean, n_var) + 1] */, double* mean_acc,
                                double* mean_w, double* var_acc, double* var_w, hipStream_t stream);
// step 1 alone: the (frame, density, weight) pairs into a.pair_* / key_* (launch_em_accumulate's / launch_em_accumulate_weighted's)
hipError_t launch_em_pairs(const EmArgs& a, hipStream_t stream);
hipError_t launch_em_pairs_weighted(const EmArgs& a, hipStream_t stream);
// Baum-Welch: pair counts of the items, then their inclusive device scan into a.item_pair_end (scan_temp from em_item_scan_temp_bytes) ...
size_t em_item_scan_temp_bytes(uint64_t n_items);
hipError_t launch_em_item_pairs(const EmArgs& a, void* scan_temp, size_t scan_temp_bytes, uint64_t* cnt, hipStream_t stream);
// ... and, with a.n_pairs = item_pair_end[n_items - 1]: (frame, density, gamma * p_d) pairs into the same sort and row sums
hipError_t launch_em_accumulate_weighted(const EmArgs& a, void* sort_temp, size_t sort_temp_bytes, uint32_t* iota, uint32_t* keys_sorted,
                                         uint32_t* pairs_sorted, uint32_t* row_begin, double* mean_acc, double* mean_w, double* var_acc,
                                         double* var_w, hipStream_t stream);

// ---- fMLLR: per-speaker statistics of a set of pairs, the adapted corpus (fmllr_stats.hip) --------------------------------------------
// The contraction's shape for a dimension: rows = D + 1 padded to 16 (row D of the k block is beta); columns = the (D+1)(D+2)/2 pairs
// j <= k of G padded to 16, then the D + 1 columns of k padded to 16.
struct FmllrShape { uint32_t rows, g_cols, g_tiles, k_tiles, cols; };
FmllrShape fmllr_shape(uint32_t dim);
uint32_t fmllr_seg_frames();   // frames per segment: the unit of the fixed summation order
uint32_t fmllr_max_dim();
// What the fMLLR and MLLR contractions share (sym_contract.h): the items of every group, group after group, are cut into segments;
// segment s = items [seg_begin[s], + seg_len[s]) of one group (at most fmllr_seg_frames()), group q owns segments [grp_seg_off[q],
// grp_seg_off[q + 1]); G below stands for n_groups
struct GroupedStats {
  FmllrShape shape;
  uint32_t n_groups, n_segs;
  const uint32_t* seg_begin; const uint32_t* seg_len; const uint32_t* grp_seg_off;
  double* partial;                   // workspace [n_segs][rows][cols]
  double *out_beta, *out_k, *out_G;  // device: [G], [G x D x (D+1)], [G x D x (D+1) x (D+1)]
};
hipError_t launch_grouped_reduce(const GroupedStats& a, uint32_t dim, hipStream_t stream);  // fmllr_stats.hip: partial -> out_*
struct FmllrArgs {
  const float* feats;
  uint64_t n_frames;
  uint32_t dim;
  const double* means; const double* inv_vars;  // [C x dim] per density
  // the pairs, in frame order: frame t's are [frame_pair_off[t], frame_pair_off[t + 1])
  const uint64_t* frame_pair_off;  // [n_frames + 1]
  const uint32_t* pair_dens; const uint32_t* pair_key; const double* pair_w;  // key 0xFFFFFFFF: dropped
  double *fold_a, *fold_c;         // workspace [n_frames x rows]
  const uint32_t* frame_list;      // every speaker's frames in corpus order, speaker after speaker: the items of g (group = speaker)
  GroupedStats g;
};
hipError_t launch_fmllr_item_frames(const uint32_t* item_off, const uint64_t* item_pair_end, uint64_t n_frames, uint64_t* frame_pair_off,
                                    hipStream_t stream);
hipError_t launch_fmllr_statistics(const FmllrArgs& a, hipStream_t stream);  // fold, contraction, reduction
// out[t][i] = (float)(W_s[i][D] + sum_j W_s[i][j] (double) feats[t][j]), j ascending, s = utt_speaker[utterance of t]
hipError_t launch_fmllr_transform(const float* feats, const uint64_t* frame_off, uint32_t n_utts, const uint32_t* utt_speaker, const double* W,
                                  uint32_t dim, float* out, hipStream_t stream);

// ---- MLLR of the means: per-(speaker, regression class) statistics of a set of pairs, the adapted means (mllr_stats.hip) ----------------
// The pairs are EmArgs' (pair_frame, pair_dens, pair_w; key_mean 0xFFFFFFFF: dropped).  Three steps with two host reads between them:
//   launch_mllr_runs     keys speaker * n_dens + density, stable sort, the runs of equal keys           -> *n_runs, run_key[*n_runs - 1]
//   launch_mllr_groups   the runs ("entries") ordered by (speaker, class, density), the groups' bounds  -> grp_begin[n_groups + 1]
//   launch_mllr_statistics  entry sums, contraction over the segments the host cut from grp_begin, reduction
// The contraction has fmllr_shape(dim)'s rows and columns and segments of fmllr_seg_frames() entries (GroupedStats).
struct MllrArgs {
  const float* feats;
  uint32_t dim;
  const double* means; const double* inv_vars;  // [n_dens x dim]
  uint64_t n_pairs;
  const uint32_t* pair_frame; const uint32_t* pair_dens; const uint32_t* pair_key; const double* pair_w;
  const uint32_t* frame_speaker;   // [n_frames]
  const uint32_t* dens_class;      // [n_dens]
  uint32_t n_dens, n_speakers, n_classes;
  // the pairs by key (all [n_pairs]): key / iota in, keys_sorted / pairs_sorted out; runs of equal keys (a last run of 0xFFFFFFFF holds
  // the dropped pairs): run_key, run_len, run_begin [n_pairs], n_runs [1]
  uint32_t *key, *iota, *keys_sorted, *pairs_sorted, *run_key, *run_len, *run_begin, *n_runs;
  void* sort_temp; size_t sort_temp_bytes;  // mllr_temp_bytes(n_pairs)
  // entries = the runs with a key: gkey = speaker * n_classes + class per run, ent_order = the runs in stable gkey order, grp_begin
  // [n_groups + 1] the first position of every group; per position: the density, occ and x_acc [n_entries x dim]
  uint32_t n_entries;
  uint32_t *gkey, *gkey_sorted, *ent_order, *grp_begin, *ent_dens;
  double *ent_occ, *ent_x;
  GroupedStats g;                  // the items: the entry positions; group = speaker * n_classes + class
};
size_t mllr_temp_bytes(uint64_t n_pairs);
hipError_t launch_mllr_runs(const MllrArgs& a, hipStream_t stream);
hipError_t launch_mllr_groups(const MllrArgs& a, hipStream_t stream);
hipError_t launch_mllr_statistics(const MllrArgs& a, hipStream_t stream);
// out[d][i] = acc, acc starting at W_r[i][D] and taking acc = acc + W_r[i][j] * means[d][j] for j ascending, r the class of density d.
// order: the densities by (class, id); block b transforms order[blk[3b + 1] .. blk[3b + 2]) with W[blk[3b]]
uint32_t mllr_dens_per_block();
hipError_t launch_mllr_transform_means(const double* means, const uint32_t* order, const uint32_t* blk, uint32_t n_blocks, const double* W,
                                       uint32_t dim, double* out, hipStream_t stream);

// ---- MAP adaptation of the means: per-(speaker, density) sums of a set of pairs, the adapted means (map_stats.hip) ---------------------
// After launch_mllr_runs (keys, stable sort, runs: run e is entry e, in ascending (speaker, density)):
//   launch_map_plan   per entry its first pair and first segment (segments of map_seg_pairs() pairs), the segment list, every speaker's
//                     first entry                                                            -> counts[2] = entries, segments; ent_off
//   launch_map_sums   a wave per segment, then the partials of the entries of several segments in ascending order -> out_*
struct MapArgs {
  const float* feats;
  uint32_t dim;
  uint64_t n_pairs;
  const uint32_t* pair_frame; const double* pair_w;
  const uint32_t *pairs_sorted, *run_key, *run_len, *n_runs;  // launch_mllr_runs' results
  uint32_t n_dens, n_speakers;
  uint64_t *cnt, *scan;    // [n_pairs + 1] per run (segments << 32 | pairs) and its exclusive scan: (first segment << 32 | first pair)
  uint32_t* seg_ent;       // [n_pairs + n_pairs / map_seg_pairs() + 1] the entry of every segment
  uint32_t* counts;        // [2] entries, segments
  uint32_t* ent_off;       // [n_speakers + 1] every speaker's first entry
  void* temp; size_t temp_bytes;  // map_temp_bytes(n_pairs): launch_mllr_runs' workspace as well
  uint32_t n_entries, n_segs;     // launch_map_sums: what counts held
  double* partial;         // workspace [n_segs][dim + 1]: x, then occ
  uint32_t* out_dens; double *out_occ, *out_x;  // device: [n_entries], [n_entries], [n_entries x dim]
};
uint32_t map_seg_pairs();   // pairs per segment: the unit of the fixed summation order
size_t map_temp_bytes(uint64_t n_pairs);
hipError_t launch_map_plan(const MapArgs& a, hipStream_t stream);
hipError_t launch_map_sums(const MapArgs& a, hipStream_t stream);
// out[d][i] = (tau * means[rep][i] + X) / (tau + O) for a density whose mean row has entries (slot = row_slot[dens_mean[d]], its entries
// row_ent[row_off[slot] .. row_off[slot + 1]) in ascending density id, O and X chains from 0.0 over them, rep = row_rep[slot] the row's
// lowest density); means[d][i] where row_slot is 0xFFFFFFFF.  No contraction.
struct MapMeansArgs {
  const double* means;       // [n_dens x dim] the prior's
  const uint32_t* dens_mean; // [n_dens]
  const uint32_t *row_slot, *row_off, *row_ent, *row_rep;
  const double *occ, *x;     // the entries: [n_entries], [n_entries x dim]
  double tau;
  uint32_t dim;
  uint64_t n_dens;
  double* out;               // [n_dens x dim]
};
hipError_t launch_map_means(const MapMeansArgs& a, hipStream_t stream);

// ---- MLLT: the global semi-tied covariance statistics of a set of pairs (mllt_stats.hip) ------------------------------------------------
// The pairs are EmArgs' (pair_frame, pair_dens, pair_w; key_mean 0xFFFFFFFF: dropped), taken in pair order and cut into segments of
// mllt_seg_pairs().  The contraction's shape: rows = D + 1 padded to 16 (row D carries gamma alone); columns = the D (D + 1) / 2 pairs
// j <= k, then one "ones" column (its row D is beta), padded to 16.
struct MlltShape { uint32_t rows, tri, tiles, cols; };
MlltShape mllt_shape(uint32_t dim);
uint32_t mllt_seg_pairs();   // pairs per segment: the unit of the fixed summation order
uint32_t mllt_max_dim();
struct MlltArgs {
  const float* feats;
  uint32_t dim;
  MlltShape shape;
  const double* means; const double* inv_vars;  // [C x dim] per density
  uint64_t n_pairs;
  const uint32_t* pair_frame; const uint32_t* pair_dens; const uint32_t* pair_key; const double* pair_w;
  // one round: segments [seg0, seg0 + n_segs) into partial; the reduction adds them, ascending, onto the running sums in out_G / out_beta
  // (seg0 == 0: onto 0)
  uint32_t seg0, n_segs;
  double* partial;              // workspace [n_segs][rows][cols]
  double *out_beta, *out_G;     // device: [1], [D x D x D]
};
hipError_t launch_mllt_round(const MlltArgs& a, hipStream_t stream);  // contraction and reduction of one round

// ---- LDA with frame splicing: the scatter and class sums of the spliced frames, the projected corpus (lda_stats.hip) -------------------
// z_t[(o + c) D + j] = (double) x[clamp(t + o, a, b - 1)][j], o = -c .. c, [a, b) = frame_span[2t], frame_span[2t + 1] the frames of
// t's utterance; E = (2c + 1) D <= lda_max_e().  The items (kept frames, corpus order) are cut into segments of lda_seg_items(); a
// segment's partial scatter is stored as the lda_pairs(E) blocks (I <= J) of lda_block() x lda_block() doubles of the upper triangle.
uint32_t lda_seg_items();
uint32_t lda_max_e();
uint32_t lda_block();
inline uint32_t lda_panels(uint32_t E) { return (E + lda_block() - 1) / lda_block(); }
inline uint32_t lda_pairs(uint32_t E) { return lda_panels(E) * (lda_panels(E) + 1) / 2; }
struct LdaArgs {
  const float* feats;
  const uint32_t* frame_span;   // [2 x n_frames]
  uint32_t dim, context, E;
  // the scatter: items [3 x n_items] = (frame, a, b) of the kept frames in corpus order, [a, b) the frame's utterance.  One round: segments [seg0, seg0 + n_segs) into partial; the
  // reduction adds them, ascending, onto the running sums in out_scatter (seg0 == 0: onto 0)
  const uint32_t* items; uint64_t n_items;
  uint32_t seg0, n_segs;
  double* partial;              // workspace [n_segs][lda_pairs(E)][lda_block()][lda_block()]
  double* out_scatter;          // device [E x E]
  // the class sums: class_items = the kept frames grouped stably by class; segment g = positions [cseg_begin[g], + cseg_len[g]) of one
  // class, class k owns segments [class_seg_off[k], class_seg_off[k + 1])
  const uint32_t* class_items; const uint32_t* cseg_begin; const uint32_t* cseg_len; const uint32_t* class_seg_off;
  uint32_t n_csegs, n_classes;
  double* cpartial;             // workspace [n_csegs][E]
  double* out_sum;              // device [n_classes x E]
};
hipError_t launch_lda_round(const LdaArgs& a, hipStream_t stream);       // scatter and reduction of one round
hipError_t launch_lda_class_sums(const LdaArgs& a, hipStream_t stream);  // segment sums and their reduction
// out[t][i] = (float) acc, acc starting at M[i][E] and taking acc = acc + M[i][n] * z_t[n] for n ascending; M [p x (E + 1)]
hipError_t launch_lda_project(const float* feats, const uint32_t* frame_span, uint64_t n_frames, uint32_t dim, uint32_t context,
                              const double* M, uint32_t p, float* out, hipStream_t stream);

// ---- the audio front end (frontend.hip) -------------------------------------------------------------------------------------------
// MFCC: one workgroup per span of at most span_frames consecutive frames of one utterance, one wave64 per frame at a time.
struct MfccArgs {
  const int16_t* samples; const uint64_t* sample_off;  // device: the utterances' samples, back to back
  const uint64_t* frame_off;                           // device [n_utts + 1]
  const uint2* spans; uint32_t n_spans;                // device: (utterance, first frame) of every workgroup
  uint32_t span_frames;                                // frames a workgroup covers: (span_frames - 1) shift + window <= mfcc_span_cap()
  uint32_t window, shift, n_fft, n_mel, n_cepstra;
  float preemphasis, energy_floor;
  // tables, device, computed on the host in double and stored as float
  const float* win;                                    // [window]
  const float2* twiddle;                               // [n_fft] (cos, -sin)(2 pi n / n_fft)
  const uint32_t* mel_first; const uint32_t* mel_count; const uint32_t* mel_off;  // [n_mel] a filter's bins and where its weights begin
  const float* mel_w;                                  // the filters' weights, filter by filter, bins ascending
  const float* dct;                                    // [n_cepstra][n_mel], sqrt(2 / n_mel) folded in
  float* out;                                          // [frames][n_cepstra]; mfcc_warps_kernel: [n_warps][frames][n_cepstra]
  // a warped front end's filters (sr_frontend_create_warped): one CSR over (warp, filter), warp by warp; warp_off indexes warp_w
  const uint32_t* warp_first; const uint32_t* warp_count; const uint32_t* warp_off;  // [n_warps][n_mel]
  const float* warp_w;
  uint32_t n_warps;                                    // mfcc_warps_kernel: the warps it applies, from the first of the CSR given
  uint64_t n_frames;                                   // mfcc_warps_kernel: the corpus's frames, the stride between two warps' cepstra
  const uint32_t* utt_warp;                            // mfcc_kernel, device [n_utts]: the utterance's warp; NULL: the unwarped filters above
};
// (mfcc_span_cap(), mfcc_waves() and the warp search's LDS rule -- mfcc_warps_pair_floats(), mfcc_warps_lds_bytes(),
// mfcc_warps_waves() -- are in vtln_tables.h, host-only, so that tests/cpp/vtln_tables_driver.cpp checks the functions the launch uses)
hipError_t launch_mfcc(const MfccArgs& a, hipStream_t stream);
// The warp search's MFCC stage: mfcc_kernel's spans and workgroups, but a frame's power spectrum is computed once and all n_warps
// filterbanks are applied to it.  A wave keeps, beside its two transform buffers, the n_warps x n_mel logarithms.
hipError_t launch_mfcc_warps(const MfccArgs& a, hipStream_t stream);
// The warp search's sums (sr_vtln_costs_corpus), in their defined order and without atomics: vtln_reduce_kernel, a thread per (row,
// warp), adds src[warp src_stride + j] for the row's j in ascending position -- j = off[row] .. off[row + 1] - 1 itself (items NULL) or
// items[that position] -- taking the first addend as is; an empty sum is +0.  -> out[row out_row + warp out_warp].
//   utterances  rows = utterances, off = the frame offsets, src = path scores [n_warps][frames]      -> [n_warps][n_utts]
//   speakers    rows = speakers, items = a speaker's utterances ascending, src = the utterances' sums -> [n_speakers][n_warps]
struct VtlnReduceArgs {
  const double* src; uint64_t src_stride;
  const uint64_t* off; const uint32_t* items;
  uint32_t n_rows, n_warps;
  double* out; uint64_t out_row, out_warp;
};
hipError_t launch_vtln_reduce(const VtlnReduceArgs& a, hipStream_t stream);
// FeaturePostProcessor::process_features on every utterance: static | delta | delta-delta, mean / deviation (NULL: none), then the
// energy maximum of component 0.  cepstra [frames][n_static] -> out [frames][n_static + n_first + n_second]
struct FeaturePostArgs {
  const float* cepstra; const uint64_t* frame_off; uint32_t n_utts; uint64_t n_frames;
  uint32_t n_static, n_first, n_second, step;
  const double* mean; const double* stddev;
  int energy_max_norm;
  float* out;
};
hipError_t launch_feature_post(const FeaturePostArgs& a, hipStream_t stream);
// Streaming (sr_stream_push_audio): stream_frontend_kernel, one workgroup per pushed utterance, takes its piece of samples to the
// rows that became ready, through the slot's state -- the last 2 step statics and the running energy maximum, 2 step n_static + 1
// floats.  A job: the utterance had S statics before the push and gains k; its piece (the sample before it first) begins at
// samples[sample0]; its staging rows -- 2 step of history, then the k new statics -- begin at row stage0 of `stage`; it emits
// `rows` rows from row0 of the utterance into row out0 of `out`, clamped by T (kStreamFrontendOpen: the count is not known yet).
// warp (sr_stream_set_warp): the utterance's filters are warp `warp` of the front end's warped CSR, as mfcc_kernel takes them by
// utt_warp; kStreamNoWarp (== SR_STREAM_NO_WARP): the unwarped filters.  The jobs of one launch may carry any mix of warps.
constexpr uint32_t kStreamFrontendOpen = 0xFFFFFFFFu;
constexpr uint32_t kStreamNoWarp = 0xFFFFFFFFu;
struct StreamFrontendJob {
  uint32_t slot, S, k, T;
  uint32_t row0, rows, warp;
  uint64_t sample0, stage0, out0;
};
struct StreamFrontendArgs {
  MfccArgs mfcc;                 // samples: the push's pieces; window .. dct and warp_first .. warp_w as for mfcc_kernel (sample_off,
                                 // frame_off, spans, out, utt_warp unused; warp_* are NULL for a front end without warps)
  const StreamFrontendJob* jobs;
  uint32_t n_static, n_first, n_second, step;
  const double* mean; const double* stddev;
  int energy_max_norm;
  float* state;                  // [slots][2 step n_static + 1]
  float* stage;                  // per push
  float* out;                    // the push's feature rows [rows][n_static + n_first + n_second]
};
hipError_t launch_stream_frontend(const StreamFrontendArgs& a, uint32_t n_jobs, hipStream_t stream);

// The pipeline of a stream set (stream_pipeline.hip; sr_stream_set_projection, sr_stream_set_transform): stream_pipeline_kernel, one
// workgroup per pushed utterance, splices and projects the rows that became ready and applies the slot's transform.  A job: the
// utterance had R input rows before the push and gains k, which begin at row in0 of `in`; it emits `rows` rows from row0 of the
// utterance into row out0 of `out`, clamped by R + k (before the finish no emitted row reaches that far); has_w: the slot's W applies.
struct StreamPipelineJob {
  uint32_t slot, has_w, R, k;
  uint32_t row0, rows;
  uint64_t in0, out0;
};
struct StreamPipelineArgs {
  const StreamPipelineJob* jobs;
  uint32_t in_dim, context, dim;  // D, c, p; without a projection (M == nullptr) in_dim == dim and context == 0
  const double* M;                // [p][(2c + 1) D + 1] or nullptr
  const double* W;                // [slots][p][p + 1] or nullptr (no slot has a transform)
  uint32_t w_doubles, y_floats;   // the kernel's LDS parts: p (p + 1) with W, stream_pipeline_group_rows() x p with M and W, else 0
  float* hist;                    // [slots][2c][D]: input row g of a slot at ring position g mod 2c
  const float* in;                // the push's new input rows [.][D]
  float* out;                     // the push's rows [.][p], what the scoring reads
};
uint32_t stream_pipeline_group_rows();
size_t stream_pipeline_lds_bytes(uint32_t in_dim, uint32_t context, uint32_t dim, bool projection, bool transforms);
hipError_t launch_stream_pipeline(const StreamPipelineArgs& a, uint32_t n_jobs, hipStream_t stream);

}  // namespace srgpu
