// handles.h -- the opaque handle types of the C ABI (include/srgpu.h) and the small helpers the translation units that
// implement it share (srgpu_api.cpp: compute entry points; feeder.cpp: frame-batch feeder and multi-device driver).
#pragma once
#include <hip/hip_runtime.h>

#include <atomic>
#include <condition_variable>
#include <cstdint>
#include <map>
#include <memory>
#include <mutex>
#include <string>
#include <thread>
#include <vector>

#include "../../include/srgpu.h"
#include "host_util.h"
#include "kernels.h"
#include "stream_audio_plan.h"
#include "stream_pipeline_plan.h"
#include "stream_set_plan.h"
#include "vtln_tables.h"

namespace srhost {
// stores a printf-style message for sr_last_error() (thread-local) and returns `code`
int fail(int code, const char* fmt, ...) __attribute__((format(printf, 2, 3)));
}  // namespace srhost

#define HIP_TRY(expr)                                                                             \
  do {                                                                                            \
    hipError_t e_ = (expr);                                                                       \
    if (e_ != hipSuccess) return srhost::fail(SR_EHIP, "%s: %s (%s:%d)", #expr, hipGetErrorString(e_), __FILE__, __LINE__); \
  } while (0)

template <typename T>
struct DevBuf {
  T* p = nullptr;
  size_t n = 0;
  hipError_t ensure(size_t count) {
    if (count <= n && p) return hipSuccess;
    if (p) { hipError_t e = hipFree(p); if (e != hipSuccess) return e; p = nullptr; n = 0; }
    if (count == 0) count = 1;
    hipError_t e = hipMalloc(reinterpret_cast<void**>(&p), count * sizeof(T));
    if (e == hipSuccess) n = count;
    return e;
  }
  hipError_t upload(const T* src, size_t count) {
    hipError_t e = ensure(count);
    if (e != hipSuccess || count == 0) return e;
    return hipMemcpy(p, src, count * sizeof(T), hipMemcpyHostToDevice);
  }
  void release() { if (p) (void)hipFree(p); p = nullptr; n = 0; }
  void swap(DevBuf& o) { T* tp = p; p = o.p; o.p = tp; size_t tn = n; n = o.n; o.n = tn; }
  // handles own their buffers: whatever a destroy function does not release by name goes with the object
  DevBuf() = default;
  DevBuf(const DevBuf&) = delete;
  DevBuf& operator=(const DevBuf&) = delete;
  ~DevBuf() { release(); }
};

// Pinned host memory the device writes straight into (hipHostMalloc, mapped and coherent): same idiom as DevBuf
template <typename T>
struct PinnedBuf {
  T* p = nullptr;
  size_t n = 0;
  hipError_t ensure(size_t count) {
    if (count <= n && p) return hipSuccess;
    if (p) { hipError_t e = hipHostFree(p); if (e != hipSuccess) return e; p = nullptr; n = 0; }
    if (count == 0) count = 1;
    hipError_t e = hipHostMalloc(reinterpret_cast<void**>(&p), count * sizeof(T), hipHostMallocMapped | hipHostMallocCoherent);
    if (e == hipSuccess) n = count;
    return e;
  }
  void release() { if (p) (void)hipHostFree(p); p = nullptr; n = 0; }
  void swap(PinnedBuf& o) { T* tp = p; p = o.p; o.p = tp; size_t tn = n; n = o.n; o.n = tn; }
  PinnedBuf() = default;
  PinnedBuf(const PinnedBuf&) = delete;
  PinnedBuf& operator=(const PinnedBuf&) = delete;
  ~PinnedBuf() { release(); }
};

struct EventPair { hipEvent_t a, b; int kind; };  // kind 0 = gmm, 1 = search, 2 = prefilter pass, 3 = refinement (inside 0)


struct sr_feeder;  // feeder.cpp: the asynchronous upload of a corpus


// The device buffers of a destroyed corpus that its model keeps for the next one (sr_recognize_batch creates and destroys a corpus
// per call: nine hipMalloc / hipFree pairs, about a millisecond of the 1.5 ms a boundary step used to lose against a resident one)
struct CorpusSpare {
  DevBuf<float> feats;
  DevBuf<uint64_t> d_frame_off;
  DevBuf<uint32_t> utt_order, out_words, out_count, out_flags;
  DevBuf<double> tb_score;
  DevBuf<uint16_t> tb_word, tb_bkp;
  DevBuf<uint64_t> gather_off;
  PinnedBuf<unsigned char> result;  // (pinning a result block per sr_recognize_batch call would cost more than the compaction saves)
  size_t bytes() const {
    return feats.n * 4 + d_frame_off.n * 8 + (utt_order.n + out_words.n + out_count.n + out_flags.n) * 4 + tb_score.n * 8 + (tb_word.n + tb_bkp.n) * 2 +
           gather_off.n * 8 + result.n;
  }
};
// ... kept only up to this size (SRGPU_SPARE_MB, default 256): a one-shot call on a huge corpus must not leave the model holding
// a corpus-sized allocation; sr_model_trim() releases it at any time
size_t corpus_spare_cap_bytes();

struct sr_model {
  int device = 0;
  uint32_t dim = 0, n_states = 0, ld = 0;
  uint64_t n_dens = 0;
  bool max_approx = true;
  // exact-kernel tables (finalised, per density)
  DevBuf<uint32_t> dens_off;
  DevBuf<double> means, inv_vars, norm, logw;
  // EM tying (accumulator rows)
  DevBuf<uint32_t> dens_mean, dens_var;
  std::vector<uint32_t> h_dens_off, h_dens_mean, h_dens_var;
  // host copies of the finalised tables: the kernel-specific packings are built on first use of that kernel
  std::vector<double> h_means, h_inv_vars, h_norm, h_logw;
  bool mfma_packed = false, pf_packed = false;
  uint32_t n_mean = 0, n_var = 0;
  // MFMA packing
  int ksteps = 0;
  uint32_t n_blocks = 0, n_groups = 0;
  DevBuf<double> apack;
  DevBuf<uint32_t> blk_meta, grp_state;
  std::vector<uint32_t> group_first_block;  // host: [n_groups+1]
  std::map<uint32_t, std::unique_ptr<DevBuf<uint32_t>>> split_tabs, pf_split_tabs;  // state-range split tables by split count
  const uint32_t *split_cur = nullptr, *pf_split_cur = nullptr;
  uint32_t split_ny = 0;
  // fp16 prefilter + FP64 refinement (gmm_prefilter.hip); pf_ks32 == 0: model not eligible
  int pf_ks32 = 0;
  uint32_t pf_groups = 0, pf_ny = 0, max_dens = 0, pf_slots = 0, pf_chunks = 1, pf_pstates = 0;
  DevBuf<unsigned char> pf_apack;
  DevBuf<float> pf_lim, featsT, featsP;  // featsP: row-major features in the refinement's padded order (only when pf_dp != dim)
  DevBuf<uint4> pf_defer;                  // deferred leftovers of the refinement (mixtures of more than 32 densities): segments ...
  DevBuf<uint32_t> pf_defer_cnt;           // ... and their counts (gmm_refine_defer_layout)
  int neg_possible = -1;                   // can an emission cost of this model be negative?  -1: not looked at yet (srhost::may_go_negative)
  uint32_t pf_dp = 0;                      // gmm_refine_padded_dim(dim): the odd dimension the refinement planes / featsT are laid out in
  DevBuf<uint32_t> pf_mask, pf_ndens, pf_ring;
  DevBuf<uint4> pf_bfrag;                  // the launch's frames as fp16 B fragments and ...
  DevBuf<float2> pf_bnorm;                 // ... their norms: the stationary prefilter route's operands, rebuilt by every launch
  int pf_route = srgpu::kPfStationary;            // SRGPU_PREFILTER=staged|stationary, read once per model (launch_gmm_prefilter)
  bool gather_device = true;               // SRGPU_GATHER=host|device, read once per model: where the search's words are compacted (gather_words.hip)
  DevBuf<double> pf_rows;
  DevBuf<unsigned long long> pf_counter;
  // feeder resources (feeder.cpp), created by the first asynchronous upload and kept: pinning 2 x 8 MiB costs milliseconds
  hipStream_t s_copy = nullptr;
  float* staging[2] = {nullptr, nullptr};
  hipEvent_t staging_free[2] = {nullptr, nullptr};
  std::atomic<bool> staging_busy{false};
  std::mutex spare_mu;
  std::unique_ptr<CorpusSpare> spare;  // of the last corpus destroyed while none was kept
  std::vector<sr_corpus*> corpora;     // live corpora of this model (under spare_mu): sr_model_destroy clears their `model` links, so that a
                                       // corpus destroyed AFTER its model -- against srgpu.h -- frees its buffers without touching the freed model
  // streams / workspace
  hipStream_t s_gmm = nullptr, s_search = nullptr;
  DevBuf<double> scores[2];
  hipEvent_t ev_scored[2] = {nullptr, nullptr}, ev_consumed[2] = {nullptr, nullptr};
  size_t chunk_frames = 0;
  bool overlap = true;  // search of chunk i on its own stream while chunk i+1 is scored (SRGPU_OVERLAP=0: one stream)
  size_t defer_budget = (size_t)32 << 30;  // most bytes for the refinement's deferred-leftover segments (SRGPU_DEFER_MB; 0: route off)
  uint32_t defer_cap_limit = 0;            // most entries per segment, 0: no limit (SRGPU_DEFER_CAP, tests: full segments)
  size_t fb_budget = (size_t)1 << 30;      // most bytes for the forward-backward trellises of one launch (SRGPU_FB_MB)
  size_t mllt_budget = (size_t)256 << 20;  // most bytes for the segment partials of one round of the MLLT statistics (SRGPU_MLLT_MB)
  size_t lda_budget = (size_t)256 << 20;   // likewise for the segment partials of the LDA scatter (SRGPU_LDA_MB)
  size_t vtln_budget = 0;                  // most bytes for the cepstra, rows, states and scores of one chunk of warps of the warp search: a
                                           // quarter of the score workspace (SRGPU_VTLN_KB; a chunk takes at least one warp)
  bool vtln_timing = false;                // SRGPU_VTLN_TIMING: sr_vtln_costs_corpus prints its chunk count and its stages' HIP-event times to stderr
  // profiling
  bool profiling = false;
  std::vector<EventPair> events;
  sr_profile prof{};
};

struct sr_corpus {
  sr_model* model = nullptr;
  sr_feeder* feeder = nullptr;      // sr_corpus_upload_async: pieces still on their way (feeder.cpp)
  uint32_t n_utts = 0;
  uint64_t n_frames = 0;
  std::vector<uint64_t> frame_off;  // host copy
  DevBuf<float> feats;
  DevBuf<uint64_t> d_frame_off;
  DevBuf<uint32_t> utt_order;       // per launch range (chunk), its utterances longest first; built for order_chunk_frames
  size_t order_chunk_frames = 0;    // 0 = not built
  // search outputs (device)
  DevBuf<double> tb_score;
  DevBuf<uint16_t> tb_word, tb_bkp;
  DevBuf<uint32_t> out_words, out_count, out_flags;
  // the packed result of a recognition call (gather_words.hip): the block the compaction writes and the host reads, the word offsets' device copy
  PinnedBuf<unsigned char> result;
  DevBuf<uint64_t> gather_off;
  DevBuf<unsigned char> big_ws;     // decode_big_kernel: hypothesis arrays of the utterances in flight
  // aligner workspace
  DevBuf<uint16_t> automata, out_states;
  DevBuf<uint64_t> aut_off, bp_off, al_blk_frame0;
  DevBuf<uint32_t> al_list_off, al_states, al_blk_frames, al_blk_list;
  DevBuf<uint8_t> backptr;
  DevBuf<double> out_cost, path_scores;
  // EM accumulation workspace
  DevBuf<uint64_t> pair_off;
  DevBuf<uint32_t> pair_frame, key_mean, key_var, iota, keys_sorted, pairs_sorted, row_begin;
  DevBuf<double> pair_w, acc_mean, acc_var, w_mean, w_var;
  bool acc_valid = false;           // acc_* hold the statistics of the last sr_accumulate_corpus (for sr_model_create_from_accumulated)
  uint32_t acc_n_mean = 0, acc_n_var = 0;
  DevBuf<unsigned char> sort_temp;
  // forward-backward workspace (viterbi_fb.hip): the trellis of one launch group, the automata's distinct mixtures, the items
  DevBuf<double> fb_trellis, fb_item_w, fb_weight;
  DevBuf<uint64_t> fb_trellis_off, fb_pair_cnt, fb_pair_end;
  DevBuf<uint32_t> fb_mix_off, fb_slot_beg, fb_cnt, fb_scan, fb_base, fb_item_off, fb_item_frame;
  DevBuf<uint16_t> fb_mix, fb_slot_pos, fb_item_mix, fb_count, fb_state;
  DevBuf<unsigned char> fb_scan_temp;
  // recognition-network forward-backward (viterbi_netfb.hip; the trellis is fb_trellis): word posteriors of one launch group, outputs
  DevBuf<double> nf_post, nf_weight, nf_conf;
  DevBuf<uint32_t> nf_word, nf_first, nf_last;
  DevBuf<uint16_t> nf_count;
  // MMI training (viterbi_mmi.hip; trellis, mixture lists and items are the fb_* buffers): the word-end sums of one launch group, the
  // transcripts' chains, the numerator's costs (the gate of the denominator's statistics)
  DevBuf<double> nf_ends, mmi_num_cost;
  DevBuf<uint64_t> mmi_chain_off;
  DevBuf<uint32_t> mmi_info, mmi_src, mmi_dst;
  // sMBR training (viterbi_smbr.hip; trellis, mixture lists and the items of one sign are the fb_* buffers): the word-end sums and
  // accuracies of one launch group, the references, Abar_u, the items of the other sign
  DevBuf<double> smbr_ends, smbr_acc, smbr_item_w;
  DevBuf<uint16_t> smbr_ref, smbr_item_mix;
  DevBuf<uint32_t> smbr_base, smbr_item_off, smbr_item_frame;
  // forward-backward over the bigram search network (viterbi_bigram_fb.hip; trellis, posteriors and items are the buffers above):
  // the launch groups' vectors and utterance orders, the items' confidences.  The sMBR pass over the same network
  // (viterbi_bigram_smbr.hip) uses them at twice the size, with smbr_ref / smbr_acc and the smbr_item_* set above
  DevBuf<double> bgfb_vec, bgfb_prod, bgfb_wend, bgfb_m, bgfb_xb, bgfb_conf;
  DevBuf<uint32_t> bgfb_order;
  // MMI training over the bigram search network (viterbi_bigram_mmi.hip; chains, mixture lists, items and the gate are the mmi_* / fb_*
  // buffers above): the 32-bit position lists, the chains' entry LM costs
  DevBuf<uint32_t> bgmmi_slot_pos;
  DevBuf<double> bgmmi_lmc;
  // word lattices (viterbi_lattice.hip): the word-end tables of one launch group, the scan's workspace, the compacted arcs
  DevBuf<double> lat_fwd, lat_ends, lat_bend, lat_arc_fwd, lat_arc_bwd, lat_arc_cost;
  DevBuf<uint16_t> lat_first;
  DevBuf<uint64_t> lat_cnt, lat_scan, lat_base, lat_frame_arc;
  DevBuf<uint32_t> lat_arc_word, lat_arc_first, lat_arc_last;
  // word lattices over the bigram search network (viterbi_bigram_lattice.hip; vectors, rows and order are the bgfb_* buffers, the
  // scan's workspace and the arcs the lat_* ones): the word-end tables of one launch group, the rolling rows' first / pred, more arc fields
  DevBuf<double> bglat_fwd, bglat_bwd;
  DevBuf<uint16_t> bglat_first, bglat_row_first;
  DevBuf<uint32_t> bglat_pred, bglat_arg, bglat_row_pred, bglat_arc_hist, bglat_arc_pred;
  // fMLLR statistics (fmllr_stats.hip; the pairs are the EM workspace above): the pairs' densities, the per-frame folds, the speakers'
  // frame lists and segments, the segments' partial sums, the results
  DevBuf<uint32_t> fm_pair_dens, fm_frame_list, fm_seg_begin, fm_seg_len, fm_spk_seg_off;
  DevBuf<uint64_t> fm_frame_pair_off;
  DevBuf<double> fm_fold_a, fm_fold_c, fm_partial, fm_beta, fm_k, fm_G;
  // MLLR statistics (mllr_stats.hip; pairs, sort workspace, segments, partial sums and results are the EM and fm_* buffers above): the
  // frames' speakers and the densities' classes, the pairs' keys and their runs, the entries' groups, order and sums
  DevBuf<uint32_t> ml_frame_speaker, ml_dens_class, ml_key, ml_run_key, ml_run_len, ml_run_begin, ml_n_runs, ml_gkey, ml_gkey_sorted,
      ml_ent_order, ml_grp_begin, ml_ent_dens;
  DevBuf<double> ml_ent_occ, ml_ent_x;
  // MAP statistics (map_stats.hip; pairs, keys, sort workspace and runs are the EM and ml_* buffers above, the entries' sums ml_ent_*):
  // the runs' (segments, pairs) counts and their scan, the segment list, the counts and the speakers' first entries, the partial sums
  DevBuf<uint64_t> map_cnt, map_scan;
  DevBuf<uint32_t> map_seg_ent, map_counts, map_ent_off;
  DevBuf<double> map_partial;
  // LDA statistics and projection (lda_stats.hip; the scatter's segment partials are fm_partial): the frames' utterance bounds, the kept
  // frames in corpus order and grouped by class, the classes' segments, their partial sums, the results
  DevBuf<uint32_t> lda_span, lda_items, lda_class_items, lda_cseg_begin, lda_cseg_len, lda_class_seg_off;
  DevBuf<double> lda_cpartial, lda_sum, lda_scatter;
};

struct sr_lexicon {
  sr_model* model = nullptr;
  // the search networks (kernels.h; build_decode_net, build_fast_net, build_word_net), pointing into the buffers below
  srgpu::DecodeNet net{};
  std::vector<uint32_t> h_slot_info, h_word_off;  // host copies of net.slot_info and the words' first slots [W + 1] (transcript chains)
  srgpu::FastNet fast{};    // n_slots = 0: none -- more slots than the LDS kernels hold, decode_big_kernel
  srgpu::WordNet words{};   // info = null: none -- some word has more than 4 positions, or the words do not fit a workgroup
  DevBuf<uint32_t> slot_info, slot_word, word_end_slot;
  DevBuf<uint32_t> f_state, f_pred, f_orig, f_type, f_word;
  DevBuf<uint32_t> w_info, w_order;
  DevBuf<uint2> w_states;
};

// The audio front end of a model (sr_frontend_*, frontend.cpp): the parameters as checked and the MFCC stage's tables
struct sr_frontend {
  sr_model* model = nullptr;
  bool has_mfcc = false;            // false: cepstra in only
  sr_mfcc_params mfcc{};
  sr_feature_post_params post{};    // (mean / stddev point at nothing: the device copies below are what is used)
  bool normalise = false;
  uint32_t span_frames = 1;         // frames per workgroup of mfcc_kernel
  DevBuf<float> win, mel_w, dct;
  DevBuf<float2> twiddle;
  DevBuf<uint32_t> mel_first, mel_count, mel_off;
  DevBuf<double> mean, stddev;
  // a warped front end (sr_frontend_create_warped): the warps' filters, one CSR over (warp, filter); the tables above stay the unwarped ones
  uint32_t n_warps = 0;             // 0: not warped
  DevBuf<float> warp_w;
  DevBuf<uint32_t> warp_first, warp_count, warp_off;
};

struct sr_bigram {
  sr_model* model = nullptr;
  srgpu::BigramArgs net{};  // the search net (kernels.h; build_bigram_net): only its network fields set, pointing into the buffers below
  DevBuf<uint32_t> slot_off, slot_mix;
  DevBuf<uint16_t> mixtures;
  DevBuf<uint32_t> pos_info, pos_slot;
  DevBuf<float> lmT, lm_rowmin, lm_rowmax;
  std::vector<uint32_t> h_slot_off, h_pos_info;  // host copies of slot_off, pos_info and lmT (transcript chains, mixture lists)
  std::vector<float> h_lmT;
  // workspace
  DevBuf<uint32_t> we_slot, we_bp, out_word, out_time, out_count, out_flags;
  DevBuf<float> we_score, out_score;
  DevBuf<uint4> book;
  DevBuf<uint64_t> book_off;
  DevBuf<uint32_t> gs_ws;               // global-states layout: the persistent workgroups' state images (viterbi_bigram.hip)
  DevBuf<unsigned long long> gs_active; // ... and the SRGPU_BIGRAM_STATS counter
  // forward-backward over the search network (viterbi_bigram_fb.hip): exp(-kappa lm) and its transpose, built for fb_kappa and kept
  // (0: not built).  lm_min: the smallest LM score into a word other than silence (NaN entries aside), from sr_bigram_create
  double fb_kappa = 0.0;
  float lm_min = 0.f;
  DevBuf<double> fb_lk, fb_lkT;
  // word lattices (viterbi_bigram_lattice.hip): the table in the caller's orientation, lm[w * W + h], built from lmT on first use
  DevBuf<float> lat_lm;
  bool lat_lm_built = false;
};

// The slots of a stream set (sr_stream_*, sr_bigram_stream_*) and their ids: stream_set_plan.h
using srplan::StreamSlots;

// The audio side of a stream set (sr_stream_set_frontend, _push_audio, _finish_audio and the bigram twins): the front end, what
// kind of input each slot's utterance takes, the host carry of an audio utterance (stream_audio_plan.h) and the device state
// stream_frontend_kernel keeps per slot.
enum : uint8_t { kStreamFresh = 0, kStreamRows = 1, kStreamAudio = 2, kStreamAudioFinished = 3 };
struct StreamAudio {
  sr_frontend* fe = nullptr;
  std::vector<uint8_t> kind;               // [max_streams] kStream*, kStreamFresh from begin to the first push that names the id
  std::vector<srplan::AudioCarry> carry;   // [max_streams]
  std::vector<uint32_t> warp;              // [max_streams] the utterance's VTLN warp (sr_stream_set_warp), SR_STREAM_NO_WARP from begin and after end
  DevBuf<float> state;                     // [max_streams][2 step n_static + 1]: the last 2 step statics, the running maximum
  // per push, sized by the largest push so far
  DevBuf<int16_t> samples;
  DevBuf<float> stage;
  DevBuf<srgpu::StreamFrontendJob> jobs;
  void open(uint32_t max_streams) {
    kind.assign(max_streams, kStreamFresh); carry.assign(max_streams, srplan::AudioCarry()); warp.assign(max_streams, SR_STREAM_NO_WARP);
  }
  void begin(uint32_t slot) { kind[slot] = kStreamFresh; carry[slot] = srplan::AudioCarry(); warp[slot] = SR_STREAM_NO_WARP; }
  void end(uint32_t slot) { warp[slot] = SR_STREAM_NO_WARP; }
};

// The pipeline of a stream set (sr_stream_set_projection, _set_transform, _push_rows and the bigram twins): the projection, the
// slots' transforms, the host carry of every utterance (stream_pipeline_plan.h) and the history stream_pipeline_kernel keeps per slot.
struct StreamPipeline {
  bool projection = false;
  uint32_t in_dim = 0, context = 0;        // D, c (0, 0 without a projection)
  DevBuf<double> M;                        // [p][(2c + 1) D + 1]
  DevBuf<float> hist;                      // [max_streams][2c][D]
  DevBuf<double> W;                        // [max_streams][p][p + 1], allocated by the first sr_stream_set_transform
  std::vector<uint8_t> has_w;              // [max_streams] the slot's utterance has a transform
  std::vector<srplan::PipelineCarry> carry;  // [max_streams]
  // per push, sized by the largest push so far
  DevBuf<float> in;
  DevBuf<srgpu::StreamPipelineJob> jobs;
  void open(uint32_t max_streams) { has_w.assign(max_streams, 0); carry.assign(max_streams, srplan::PipelineCarry()); }
  void begin(uint32_t slot) { has_w[slot] = 0; carry[slot] = srplan::PipelineCarry(); }
};

// What the two kinds of stream set share (stream_api.cpp): everything but the search.  The device state of a slot is a window on its
// utterance: base = the frames dropped so far (window frame f is the utterance's frame base + f; slots.frames counts the window's
// searched frames).  Reset by every begin; only sr_stream_trim moves it, so it stays 0 in the bigram set.
struct StreamSet {
  sr_model* model = nullptr;
  StreamSlots slots;
  StreamAudio audio;
  StreamPipeline pipe;
  DevBuf<float> feats;                // the rows a push searches, sized by the largest push so far
  // the stable and trim calls, allocated by their first call: the previous commit point (zerogram: a frame; bigram: a book index) per
  // slot (a separate array: the state records are the search kernels'), and the call's pinned block -- its jobs in, its results and
  // items out (stream_set_plan.h: block_layout)
  std::vector<uint8_t> commit_fresh;  // [max_streams] no commit point computed for the slot's utterance yet
  DevBuf<uint32_t> commit;
  PinnedBuf<unsigned char> stable_block;
  std::vector<uint64_t> base;         // [max_streams]
  virtual ~StreamSet() = default;     // (sr_stream_destroy and its twin delete through this type)
};

// A set of concurrently open utterances on one (model, lexicon) (sr_stream_*).  The device state of slot i's utterance
// (decode_stream_kernel) lives in the per-slot buffers below.
struct sr_stream : StreamSet {
  sr_lexicon* lex = nullptr;
  sr_search_params params{};
  // per slot, device
  DevBuf<unsigned char> ws;         // decode_big_workspace(P) each
  DevBuf<srgpu::StreamState> state;
  DevBuf<double> tb_score;          // max_frames + 1 each
  DevBuf<uint16_t> tb_word, tb_bkp;
  DevBuf<uint32_t> words;           // max_frames each
  DevBuf<srgpu::StreamJob> jobs;    // per push, sized by the largest push so far
  DevBuf<uint32_t> stable_words;    // sr_stream_stable, sr_stream_trim: the walk's words (max_frames each)
  // sr_stream_trim: the committed words of the frames dropped (base).  Reset by sr_stream_begin; an id that is never trimmed keeps an
  // empty archive.
  std::vector<std::vector<uint32_t>> archive;   // [max_streams] grows with words, not frames
};

// A set of concurrently open utterances on one (model, bigram search net) (sr_bigram_stream_*).  The device state of slot i's
// utterance (bigram_stream_kernel, global-states layout) lives in the per-slot buffers below, a copy of its BigramStreamState (read
// back after every push) on the host.
struct sr_bigram_stream : StreamSet {
  sr_bigram* bigram = nullptr;
  sr_bigram_params params{};
  std::vector<srgpu::BigramStreamState> host_state;  // [max_streams] as of the slot's last push
  std::vector<uint8_t> failed;      // [max_streams] a push flagged the slot (SR_EINTERNAL until it ends)
  // per slot, device
  DevBuf<uint32_t> gs_ws;           // bigram_gs_ws_words each
  DevBuf<uint32_t> we_slot, we_bp;  // 4W each
  DevBuf<float> we_score;
  DevBuf<uint16_t> lsave;           // 2W each
  DevBuf<srgpu::BigramStreamState> state;
  DevBuf<uint32_t> out_word, out_time;  // max_frames + 1 each
  DevBuf<float> out_score;
  std::vector<std::unique_ptr<DevBuf<uint4>>> book;  // [max_streams] grown before a push to n_book + W x (its frames)
  DevBuf<srgpu::BigramStreamJob> jobs;               // per push, sized by the largest push so far
};

namespace srhost {
// (srgpu_api.cpp) handle without parameter tables / lazily fetched host copies of them
int model_shell(int device, uint32_t dim, uint32_t n_states, const uint32_t* dens_off, int max_approx, sr_model** out);
int ensure_host_tables(sr_model* m);
int may_go_negative(sr_model* m, bool* out);  // can an emission cost of this model be negative or NaN? (cached)
// (em_finalize.hip) MixtureModel::finalize on the device: statistics (host arrays) -> new model whose tables are built in HBM
int finalize_on_device(int device, uint32_t dim, uint32_t n_states, const uint32_t* dens_off, uint32_t n_mean, uint32_t n_var,
                       const uint32_t* dens_mean, const uint32_t* dens_var, const double* mean_acc, const double* mean_w,
                       const double* var_acc, const double* var_w, int pooling, int max_approx, sr_model** out);
int finalize_accumulated(sr_model* m, sr_corpus* c, int pooling, int max_approx, sr_model** out);
// (feeder.cpp) make frames [f0, f1) of the corpus visible to work queued on `stream` afterwards: returns at once for a
// synchronously uploaded corpus; for sr_corpus_upload_async it waits (host) until the feeder has issued the pieces that
// cover the range and makes the stream wait for their copy events.  Returns the feeder's error, if any.
int corpus_ready(sr_corpus* c, uint64_t f0, uint64_t f1, hipStream_t stream);
bool corpus_upload_in_flight(const sr_corpus* c);
void feeder_join(sr_corpus* c);  // blocks until the feeder thread (if any) has finished, frees its staging buffers
// (srgpu_api.cpp) a new corpus takes over the buffers its model kept from the last destroyed one / a dying corpus leaves them
void corpus_register(sr_corpus* c);     // after c->model is set
void corpus_adopt_spare(sr_corpus* c);
void corpus_donate_spare(sr_corpus* c);
}  // namespace srhost
