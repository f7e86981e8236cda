/*
 * srgpu.h -- C ABI of libsrgpu.so: MI355X (gfx950) GMM acoustic scorer + Viterbi decoder/aligner.
 *
 * Drop-in boundary for the hot path of kkromberg/SpeechRecognition's `sietill` recogniser.
 * Every entry point names the reference interface it replaces (paths relative to the reference
 * repository root, src/sietill/...).  Plain pointers and sizes only; no C++/torch types; all
 * functions return 0 on success or a negative SR_E* code, with a thread-local message in
 * sr_last_error().  No exceptions cross this boundary.
 *
 * Conventions (same as the reference):
 *   scores   negative natural-log likelihoods (costs, lower is better), IEEE double
 *   features float32, row-major [frames x dim], utterances concatenated (Corpus layout,
 *            Corpus.cpp:89-111); offsets here are in FRAMES, not floats
 *   states   mixture (= HMM state) indices; words are indices into the lexicon
 *
 * Ownership: the caller owns every host buffer; handles own their device memory.  Model and
 * lexicon are immutable after creation.  A handle is bound to one HIP device and must be used by
 * one host thread at a time (one handle per GPU; utterance batches shard across GPUs with no
 * collective, Recognizer.cpp:46-47).
 */
#ifndef SRGPU_H
#define SRGPU_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#if defined(__GNUC__)
#define SR_API __attribute__((visibility("default")))
#else
#define SR_API
#endif

/* ABI version of this header.  Bumped whenever a struct below grows or changes layout or an entry point changes its signature
 * (4: sr_bigram_params gained `flags` in round 3 -- a caller compiled against the 16-byte struct of version 3 would be read 4 bytes
 * past its end; sr_model_trim, SR_GMM_DEFAULT).  A binding checks `sr_abi_version() == SR_ABI_VERSION` once after loading the
 * library (capi.py and sr_sietill.hpp do) and zero-initialises the parameter structs field by field. */
#define SR_ABI_VERSION 4
SR_API int sr_abi_version(void);

#define SR_OK 0
#define SR_EINVAL (-1)   /* bad argument (message says which) */
#define SR_EHIP (-2)     /* HIP runtime error */
#define SR_ENODEV (-3)   /* no usable gfx950 device */
#define SR_ELIMIT (-4)   /* size outside what the kernels support (message says which) */
#define SR_ENOMEM (-5)   /* host allocation failed (std::bad_alloc caught at the boundary) */
#define SR_EINTERNAL (-6) /* any other C++ exception caught at the boundary (message carries what()) */
#define SR_ECORRUPT (-7) /* a traceback that does not walk back to frame 0 (a back pointer that does not fall, a word outside the
                           lexicon): no words are reported for the call */

/* GMM scoring kernels (MixtureModel::score, Mixtures.cpp:737-744) */
#define SR_GMM_MFMA 0   /* dense FP64 MFMA contraction + fused min / -log-sum-exp epilogue (<= 1e-9 relative, ~1e-15 on
                           well-conditioned models; what SR_GMM_DEFAULT picks for sum scoring).  Dimension <= 63; a model of
                           dimension 64 .. 160 (the largest the library takes) is scored by SR_GMM_EXACT's kernel instead */
#define SR_GMM_EXACT 1  /* direct form replaying density_score_sse's operation order (Mixtures.cpp:645-690): bit-exact */
#define SR_GMM_PREFILTER 2  /* bit-exact like SR_GMM_EXACT: a 16-bit MFMA prefilter selects the densities that can be the
                               minimum, FP64 replays only those.  Max-approx models with <= 128 densities per mixture and
                               dim <= 62; any other model is scored by SR_GMM_EXACT's kernel instead (same bits). */

#define SR_GMM_DEFAULT 3  /* what a drop-in caller wants: the fastest kernel that reproduces MixtureModel::score for THIS model --
                             SR_GMM_PREFILTER (bit-exact) for max-approx models; for sum scoring (max-approx false,
                             Mixtures.cpp:719-728) the FP64-MFMA kernel with its fused -log sum exp, i.e. SR_GMM_MFMA's bound:
                             <= 1e-9 relative (measured 6e-16 on synthetic models, 2.3e-9 worst on a trained real-speech model;
                             the direct form SR_GMM_EXACT is 1e-12 from the reference's libm in sum mode and 3x slower -- a
                             caller that wants those three digits passes SR_GMM_EXACT).  Words and tracebacks through this
                             selector are held to the reference on the sum-mode goldens (tests/test_gpu_parity.py).
                             The aligner / path-score entry points score only the states they need with the bit-exact kernel. */

typedef struct sr_model sr_model;     /* replaces MixtureModel as a FeatureScorer (Mixtures.hpp:18, FeatureScorer.hpp:12-16) */
typedef struct sr_corpus sr_corpus;   /* replaces Corpus' feature store (Corpus.hpp:79-84, Corpus.cpp:141-144) */
typedef struct sr_lexicon sr_lexicon; /* replaces Lexicon + TdpModel as search network (Lexicon.hpp:16-33, TdpModel.hpp:13-29) */

SR_API const char* sr_last_error(void);
SR_API int sr_device_count(int* count);

/* ---- model ------------------------------------------------------------------------------------
 * Finalised tables as MixtureModel holds them after read()+finalize() (Mixtures.cpp:374-461,
 * Mixtures.hpp:71-84), expanded per density (tied variances repeated):
 *   dens_off[n_states+1]  densities of state s are rows dens_off[s] .. dens_off[s+1]-1
 *   means, inv_vars       [C x dim] doubles (means_, vars_inv_);  norm, logw  [C] (norm_, mean_weights_log_)
 *   max_approx            1: min_score (Mixtures.cpp:696-713), 0: sum_score (:719-728)
 * Limits: dim <= 160 (the matrix-core kernels end at 63 and 62: the exact kernel scores what lies beyond), C < 2^31.  (The reference
 * itself stops at 65535 densities, Mixtures.cpp:766.) */
SR_API int sr_model_create(int device, uint32_t dim, uint32_t n_states, const uint32_t* dens_off,
                    const double* means, const double* inv_vars, const double* norm, const double* logw,
                    int max_approx, sr_model** out);
/* MixtureModel(config, dim, ...) with "load-mixtures-from" (Mixtures.cpp:156-174): reads a MIXSET v2
 * file (read(), :748-830), derives the tables (finalize(), :374-461) on the host and creates the
 * device model.  pooling: 0 global, 1 mixture, 2 none (MixtureModel::VarianceModel, Mixtures.hpp:20-24).
 * Malformed files return SR_EINVAL with the reference's message instead of abort() (Mixtures.cpp:97-102). */
SR_API int sr_model_load_mixset(const char* path, uint32_t dim, int pooling, int max_approx, int device, sr_model** out);
/* MixtureModel::finalize (Mixtures.cpp:374-461) on in-memory statistics -- the model update of an EM iteration:
 * accumulators as sr_accumulate_corpus returns them (+ the topology: dens_off, accumulator rows per density) ->
 * new device model.  The divisions, variances and per-density tables are computed on the device, in the reference's
 * operation order; the logarithms (norm_, mean_weights_log_) go through the host's libm so that the tables carry the
 * reference's bits (the variances come back to the host for that).  sr_mixset_write stores the same statistics as a MIXSET v2 file exactly like
 * MixtureModel::write (Mixtures.cpp:834-878: unreferenced rows dropped and renumbered). */
SR_API int sr_model_create_from_statistics(int device, uint32_t dim, uint32_t n_states, const uint32_t* dens_off,
                                           uint32_t n_mean, uint32_t n_var, const uint32_t* dens_mean, const uint32_t* dens_var,
                                           const double* mean_acc, const double* mean_w, const double* var_acc, const double* var_w,
                                           int pooling, int max_approx, sr_model** out);
SR_API int sr_mixset_write(const char* path, uint32_t dim, uint32_t n_states, const uint32_t* dens_off, uint32_t n_mean,
                           uint32_t n_var, const uint32_t* dens_mean, const uint32_t* dens_var, const double* mean_acc,
                           const double* mean_w, const double* var_acc, const double* var_w);
SR_API int sr_model_destroy(sr_model* m);
SR_API int sr_model_info(const sr_model* m, uint32_t* dim, uint32_t* n_states, uint64_t* n_densities);

/* ---- corpus / frame-batch feeder (Corpus.cpp:89-111) --------------------------------------------
 * Copies n_utts concatenated utterances to the device. frame_off[n_utts+1], frame_off[0] == 0.
 * The host buffer is borrowed for the duration of the call only. */
SR_API int sr_corpus_upload(sr_model* m, const float* feats, const uint64_t* frame_off, uint32_t n_utts, sr_corpus** out);
/* The frame-batch feeder proper: like sr_corpus_upload, but it returns as soon as the handle exists.  A feeder thread copies
 * the host buffer in 2 MiB pieces through two pinned staging buffers on the corpus' own copy stream; the compute entry
 * points below wait -- on the device, per score chunk -- only for the pieces a chunk needs, so the transfer of later
 * utterances overlaps the scoring of earlier ones.  The host buffer is borrowed until sr_corpus_wait() has returned (or
 * the corpus has been destroyed); sr_corpus_wait returns the feeder's status.  sr_recognize_batch feeds this way. */
SR_API int sr_corpus_upload_async(sr_model* m, const float* feats, const uint64_t* frame_off, uint32_t n_utts, sr_corpus** out);
SR_API int sr_corpus_wait(sr_corpus* c);
/* A corpus must be destroyed BEFORE the model it was uploaded to.  Its search-path device buffers (features, frame offsets, word and
 * traceback outputs) are not freed but parked on the model for the next corpus -- sr_recognize_batch creates and destroys one per
 * call, and nine allocations per batch cost about a millisecond -- if they hold at most SRGPU_SPARE_MB MiB together (default 256;
 * 0 keeps nothing); one set is kept, until the next upload adopts it, sr_model_trim() or sr_model_destroy(). */
SR_API int sr_corpus_destroy(sr_corpus* c);
/* Releases what the model keeps for reuse between calls: the parked buffers above, and the scoring path's deferred-leftover segments
 * (models of more than 32 densities per mixture; up to SRGPU_DEFER_MB, 23 GB at 8000 states x 64 densities / 302 685 frames) --
 * the next scoring call allocates them again. */
SR_API int sr_model_trim(sr_model* m);

/* ---- scoring: FeatureScorer::prepare_sequence + score (FeatureScorer.hpp:14-15) -------------------
 * Dense table out[total_frames x n_states] (row-major, host memory): out[t*n_states+s] is what
 * MixtureModel::score(frame t, s) returns.  This is the table a `GpuMixtureScorer::prepare_sequence`
 * fills, exactly like NeuralNetwork::prepare_sequence does (NeuralNetwork.cpp:184-199). */
SR_API int sr_score_corpus(sr_model* m, sr_corpus* c, int gmm_kernel, double* out);
/* one-shot convenience over host features of a single sequence */
SR_API int sr_score_frames(sr_model* m, const float* feats, uint64_t n_frames, int gmm_kernel, double* out);

/* ---- search network ---------------------------------------------------------------------------
 * Linear whole-word lexicon as Lexicon::add_word builds it (Lexicon.cpp:11-22): word w owns
 * automaton[word_off[w] .. word_off[w+1]) (state ids with repetitions expanded,
 * MarkovAutomaton.hpp:22-28).  tdp = {loop, forward, skip} (TdpModel.cpp:5-7); silence_state as
 * TdpModel::silence_state.  The initial hypothesis sits at position 0 of word 0 like the
 * reference's (Recognizer.cpp:120), which is a word end when word 0 (normally silence) has one
 * position.  Limits: <= 65535 words, <= 65534 positions in total (beyond 8192 type-padded positions the search keeps its
 * hypotheses in device memory instead of LDS: same results, slower), some word with >= 2 positions. */
SR_API int sr_lexicon_create(sr_model* m, uint32_t n_words, const uint32_t* word_off, const uint16_t* automaton,
                      uint32_t silence_idx, const double tdp[3], uint16_t silence_state, sr_lexicon** out);
SR_API int sr_lexicon_destroy(sr_lexicon* l);
/* Which search kernel sr_recognize_corpus runs on this lexicon, as text (for logs and benchmark reports): "words <nw> x <lanes>
 * plain <L> [general]" = the word-per-lane kernel (viterbi_words.hip), "slots" = the slot-per-lane kernel (viterbi_fast.hip),
 * "big" = hypotheses in device memory.  out is NUL-terminated within cap bytes. */
SR_API int sr_lexicon_describe(const sr_lexicon* l, char* out, size_t cap);

typedef struct {
  double am_threshold; /* "am-threshold", Recognizer.cpp:31 (beam) */
  double word_penalty; /* "word-penalty", Recognizer.cpp:32 */
  int gmm_kernel;      /* SR_GMM_DEFAULT, or SR_GMM_MFMA / SR_GMM_EXACT / SR_GMM_PREFILTER */
  int flags;           /* 0, SR_SEARCH_GENERAL_KERNEL or SR_SEARCH_SLOT_KERNEL (was `reserved`, must be 0 otherwise) */
} sr_search_params;
/* Decode every utterance with the general kernel (slots in reference order, sequential boundary replay inline,
 * viterbi_decode.hip) instead of the type-sorted fast kernel: same results, several times slower.  The fast kernel hands
 * an utterance to it by itself when it meets a negative emission cost; this flag is for cross-checking the two. */
#define SR_SEARCH_GENERAL_KERNEL 1
/* Lexica whose words all have at most four positions (and at most 3072 words, score rows that fit the LDS twice) are searched
 * by the word-per-lane kernel (viterbi_words.hip: a word's hypotheses live in registers) -- also where they have more than the
 * 8192 type-padded positions the slot-per-lane kernel holds (2 731 .. 3 072 three-state words; round 4); this flag keeps them on the
 * slot-per-lane kernel that serves every other lexicon (viterbi_fast.hip).  Same results; for cross-checking the two. */
#define SR_SEARCH_SLOT_KERNEL 2

/* ---- decoder: Recognizer::recognize / recognizeSequence_pruned (Recognizer.cpp:38-92, :103-232) ---
 * Scores every frame of the resident corpus and runs the beam Viterbi per utterance, all on the
 * device.  out_words (capacity: total frames, a safe upper bound) receives the recognised word
 * indices of all utterances back to back, silence removed; utterance u owns
 * out_words[out_word_off[u] .. out_word_off[u+1]).
 * Optional traceback dump (may be NULL), each [total_frames + n_utts]: entry frame_off[u]+u+t is
 * traceback[t] of utterance u, t = 0..T_u (Recognizer.cpp:118,191-208). */
SR_API int sr_recognize_corpus(sr_model* m, sr_corpus* c, sr_lexicon* l, const sr_search_params* p,
                        uint32_t* out_words, uint64_t* out_word_off,
                        double* tb_score, uint16_t* tb_word, uint16_t* tb_bkp);
/* The traceback loop alone (Recognizer.cpp:222-231: `t = T; while (t > 0) { push word unless silence; t = traceback[t].bkp }`,
 * reversed), with the checks every search kernel here applies before it follows an entry: bkp < t (the reference writes
 * bkp = t - 1 of an earlier frame, :140,170, so t falls strictly), word < n_words, at most T words.  SR_ECORRUPT otherwise.
 * sr_traceback_corpus walks caller-supplied dumps in sr_recognize_corpus' layout ([total_frames + n_utts], words not slots)
 * on the device, with the kernels' own walker; sr_traceback_words walks one utterance's T + 1 entries on the host. */
SR_API int sr_traceback_corpus(sr_model* m, sr_corpus* c, sr_lexicon* l, const uint16_t* tb_word, const uint16_t* tb_bkp,
                               uint32_t* out_words, uint64_t* out_word_off);
SR_API int sr_traceback_words(uint32_t n_frames, const uint16_t* tb_word, const uint16_t* tb_bkp, uint32_t silence_word,
                              uint32_t n_words, uint32_t* out_words, uint32_t* out_count);
/* one-shot convenience: upload + recognise + free */
SR_API int sr_recognize_batch(sr_model* m, sr_lexicon* l, const sr_search_params* p, const float* feats,
                       const uint64_t* frame_off, uint32_t n_utts, uint32_t* out_words, uint64_t* out_word_off);

/* ---- streaming recognition: Recognizer::recognizeSequence_pruned (Recognizer.cpp:103-232) fed frame by frame -------------
 * The frame-at-a-time shape of Mm::FeatureScorer::addFeature / OfflineRecognizer::processFeature (RWTH ASR): an utterance is
 * begun, its frames are pushed as they arrive, the best words so far can be read after any push, and ending it returns exactly
 * what sr_recognize_corpus returns for the whole utterance (same gmm_kernel): words and traceback, bit for bit.  After t frames
 * the partial result is what sr_recognize_corpus returns for the first t frames as a complete utterance (the reference's
 * traceback[1..t] does not depend on later frames); a later frame can still change which words the final result holds.
 *
 * sr_stream_open     a set of up to max_streams concurrently open utterances of up to max_frames frames (<= 65535, the 16-bit
 *                    back pointers) on (m, l).  p->flags must be 0; p->gmm_kernel as for sr_recognize_corpus.  Device memory:
 *                    max_streams x (20 P + 12 (max_frames + 1) + 4 max_frames + 40) bytes (P = the lexicon's positions; 20 P
 *                    rounded up to 256), plus staging for the largest push: 4 dim + 8 n_states bytes per frame and the scoring
 *                    kernel's own workspaces.  The search always keeps its hypotheses in device memory (decode_stream_kernel).
 *                    An utterance that is trimmed (sr_stream_trim, below) may be longer than max_frames: the limit then bounds
 *                    the frames since the last one dropped.
 * sr_stream_begin    a fresh utterance (the initial hypothesis of Recognizer.cpp:116-120); *id names it until sr_stream_end.  Ids
 *                    are not reused soon after their utterance ended: an ended id is refused, not confused with a newer one.
 * sr_stream_push     n utterances, ids[n], each at most once; their new frames back to back in feats ([frames x dim] float32),
 *                    utterance i owning rows [frame_off[i], frame_off[i+1]) (frame_off[0] == 0; an empty range is allowed).
 *                    Every frame of the push is scored in one launch, then one search launch advances every utterance; returns
 *                    when both have finished.  Everything is checked before anything is launched: a refused push changes no
 *                    utterance.
 * sr_stream_partial  the words after the frames pushed so far (*frames); cap = capacity of out_words (may be NULL if cap is 0).
 * sr_stream_end      the final words and, optionally (each may be NULL), the utterance's T + 1 traceback entries in
 *                    sr_recognize_corpus' per-utterance layout (words, not slots); frees the id (also on SR_ECORRUPT).  An
 *                    utterance ended after 0 frames reports what sr_recognize_corpus reports for an empty utterance: no words,
 *                    traceback[0] = (0.0, 0, 0).
 * sr_stream_destroy  before its lexicon and its model.
 * Errors: SR_EINVAL for an unknown or ended id, an id repeated within one push, max_streams == 0, max_frames == 0, p->flags != 0, a
 * malformed frame_off, and a cap below the word count (*count then holds the count needed; the id stays open); SR_ELIMIT for a
 * push that would take an utterance past max_frames, sr_stream_begin with every id in use, max_frames > 65535 and a lexicon of
 * more than 65534 positions; SR_ECORRUPT as for sr_recognize_corpus.  Threading: like the model, one host thread at a time. */
typedef struct sr_stream sr_stream;   /* a set of concurrently open utterances on one (model, lexicon) */
SR_API int sr_stream_open(sr_model* m, sr_lexicon* l, const sr_search_params* p, uint32_t max_streams, uint64_t max_frames,
                          sr_stream** out);
SR_API int sr_stream_begin(sr_stream* s, uint32_t* id);
SR_API int sr_stream_push(sr_stream* s, uint32_t n, const uint32_t* ids, const float* feats, const uint64_t* frame_off);
SR_API int sr_stream_partial(sr_stream* s, uint32_t id, uint32_t* out_words, uint32_t cap, uint32_t* count, uint64_t* frames);
SR_API int sr_stream_end(sr_stream* s, uint32_t id, uint32_t* out_words, uint32_t cap, uint32_t* count, double* tb_score,
                         uint16_t* tb_word, uint16_t* tb_bkp);
SR_API int sr_stream_destroy(sr_stream* s);

/* ---- the stable prefix of a streaming result, and a trailing-silence count -----------------------------------------------
 * sr_stream_partial's words can still change with later frames; sr_stream_stable returns the leading part of them that cannot.
 * After t pushed frames of an utterance:
 *   B           the set { bk[p] : sc[p] finite } over the trellis positions p of the search's current hypotheses (bk: the frame
 *               before the hypothesis' word started, the reference's Book::bkp); for t = 0, B = {0}.
 *   the tree    node c > 0 (a frame) has the parent tb_bkp[c] < c, the traceback entry sr_stream_end returns; node 0 is the root.
 *   commit      c(t) = the nearest common ancestor of B in that tree.  Every traceback a later frame can produce runs through a
 *               member of B, hence through c(t): no later frame can move it, and c(t + 1) is c(t) or a descendant of it.  With no
 *               hypothesis alive the commit point stays where it was.
 *   stable      the words the guarded walk of sr_stream_partial returns when started at frame c(t) instead of t, silence removed.
 *               They are a prefix of sr_stream_partial at this and at every later frame t' whose tb_score[t'] is finite, and of
 *               sr_stream_end under the same condition.  (A frame at which no word end survives records (inf, word 0, bkp 0):
 *               ending there returns no words at all -- the reference's behaviour, stated, not changed.)
 *   silence     on the alive hypothesis of least score (ties: the smaller position): t - bk if its position belongs to the silence
 *               word, else 0; 0 with no alive hypothesis.  An endpointer ends the utterance when this passes its threshold.
 * sr_stream_stable  n utterances, ids[n], each at most once, in ONE launch (stream_commit_kernel: one workgroup per utterance, started
 *                   only by this call -- sr_stream_push does no work for it) whose results land in one pinned block.  out_words:
 *                   the stable words back to back, utterance i's at [out_word_off[i], out_word_off[i + 1]) (cap = capacity of
 *                   out_words, which may be NULL if cap is 0); out_commit[i] = c(t); out_silence[i] (the array may be NULL) = the
 *                   trailing silence.  The call reads the search's state and changes none of it; it keeps the commit point per
 *                   utterance, so that a call's walk is bounded by the traceback nodes above the previous call's commit point.
 *                   First call: 4 + 4 max_frames bytes of device memory per stream.
 * Errors, everything checked before the launch: SR_EINVAL for an unknown, ended or repeated id; SR_EINVAL for a cap below the
 * word count (out_word_off then holds the offsets needed, nothing else is written); SR_ECORRUPT for a walk that fails its guards
 * (nothing is written). */
SR_API int sr_stream_stable(sr_stream* s, uint32_t n, const uint32_t* ids, uint32_t* out_words, uint64_t cap, uint64_t* out_word_off,
                            uint32_t* out_commit, uint32_t* out_silence);

/* ---- endless streams: dropping the committed frames of an open utterance --------------------------------------------------
 * Nothing below the commit point c(t) is read again except to spell out the words on the way to it.  sr_stream_trim moves those
 * words to the host and drops the frames up to c(t) on the device; the search goes on bit for bit as if nothing had been dropped.
 * After a trim the device state of the utterance is a WINDOW on it:
 *   base        the frames dropped so far, a 64-bit host count.  Window frame f is the utterance's frame base + f; window frame 0
 *               stands for the last commit point trimmed at and carries the entry (0.0, 0, 0).
 *   archive     the words of the guarded walks from every commit point trimmed at down to the one before it, silence removed: a
 *               host array per utterance that grows with words, not frames, and is reset by sr_stream_begin.
 *   max_frames  bounds the WINDOW, not the utterance: a push is SR_ELIMIT when the rows received since the last dropped frame
 *               would pass it (for an audio id: the frames its samples make).  An utterance that is trimmed as often as its commit
 *               point moves runs on without limit in a set opened for the largest uncommitted stretch.  Only the utterance's own
 *               row counts stay 32 bit: a push that would take one past 2^32 - 1 is SR_ELIMIT.
 * sr_stream_trim     n utterances, ids[n], each at most once, in ONE launch (stream_trim_kernel: one workgroup per utterance).
 *                    Per id: c = c(t) exactly as sr_stream_stable computes it (the same fold, the same floor; with no hypothesis
 *                    alive it stays at the previous commit point); the words of the walk from c go to the archive; d = c frames
 *                    are dropped: traceback entries (c, t] become (0, t - c] with their back pointers rebased (one below c -- the
 *                    no-word-end record, or a dead node no later walk reaches -- becomes 0), the alive hypotheses' back pointers
 *                    lose c, the commit point becomes 0, and the partial result is walked anew.  out_dropped[i] = d (the array may
 *                    be NULL); d == 0 is a valid answer and changes nothing.  c <= t - 1 always: the window keeps a frame.  Feature,
 *                    row and audio ids all trim: the front end's and the pipeline's own counters stay absolute.
 * On a trimmed utterance
 *   sr_stream_partial  returns archive + window words, *frames counts from the utterance's start.  Where the last searched frame
 *                      has no surviving word end the result is the window walk's alone -- no archived word: ending there returns
 *                      no earlier word at all, the reference's behaviour (above).
 *   sr_stream_stable   returns archive + the window's stable words, out_commit = base + c (SR_ELIMIT if past 2^32 - 1).
 *   sr_stream_end      returns the words sr_recognize_corpus returns for the whole utterance.  Its traceback arrays must be NULL:
 *                      the dropped entries are gone, and a non-NULL array is SR_EINVAL and leaves the id open.
 * An id that is never trimmed has base 0 and behaves as before.  The bigram stream set does not trim.
 * Errors, everything checked before the launch: SR_EINVAL for an unknown, ended or repeated id (nothing is written); SR_ECORRUPT
 * for an id whose walk fails its guards or with an alive back pointer below c -- that id is left as it was, on the device and
 * here; the other ids of the call are trimmed and their out_dropped written. */
SR_API int sr_stream_trim(sr_stream* s, uint32_t n, const uint32_t* ids, uint32_t* out_dropped);

/* ---- several devices: the `#pragma omp parallel for` over segments of Recognizer::recognize (Recognizer.cpp:46-47) -------
 * Utterances are independent, so a batch shards across devices with no collective: sr_shard_utterances deals them by
 * greedy longest-processing-time on frame counts (decreasing length, each to the lightest shard so far; deterministic);
 * shard_of_utt[n_utts] receives the shard of every utterance, shard_frames[n_shards] (may be NULL) the frames per shard.
 * sr_recognize_batch_multi runs one host thread per (model, lexicon) replica -- models[d] on its own device, or several
 * replicas on one device -- which feeds (sr_corpus_upload_async, straight from the caller's buffer) and recognises its
 * shard; the word sequences come back in corpus order, exactly what sr_recognize_batch returns on one device. */
SR_API int sr_shard_utterances(const uint64_t* frame_off, uint32_t n_utts, uint32_t n_shards, uint32_t* shard_of_utt,
                               uint64_t* shard_frames);
SR_API int sr_recognize_batch_multi(sr_model* const* models, sr_lexicon* const* lexica, uint32_t n_devices,
                                    const sr_search_params* p, const float* feats, const uint64_t* frame_off, uint32_t n_utts,
                                    uint32_t* out_words, uint64_t* out_word_off, uint64_t* shard_frames);

/* ---- forced aligner: Aligner::align_sequence_full (Alignment.cpp:50-144) --------------------------
 * Utterance u is aligned against automata[aut_off[u] .. aut_off[u+1]) (N_u state ids; training
 * builds `sil w1 sil ... sil`, Training.cpp:239-253).  Requires 1 <= N_u <= T_u (the reference
 * indexes T-sized cost arrays by position).  out_states[total_frames] receives
 * AlignmentItem::state per frame (count = 1, weight = 1 implied, Alignment.cpp:131-134);
 * out_cost[n_utts] the returned path cost.  Limits: N_u <= 8192 (SR_ELIMIT; 18 bytes per position in the
 * 160 KiB LDS).  An utterance with no path of finite cost (emission costs or penalties of +inf) gets
 * that cost (+inf, or NaN) and, from the frame at which the reference's back-trace would leave the
 * cells it has computed, the position the walk stands on. */
SR_API int sr_align_corpus(sr_model* m, sr_corpus* c, const uint16_t* automata, const uint64_t* aut_off,
                    const double tdp[3], uint16_t silence_state, int gmm_kernel,
                    uint16_t* out_states, double* out_cost);

/* Aligner::align_sequence_pruned (Alignment.cpp:149-288): beam `pruning_threshold` on the per-frame
 * best, transition penalty keyed on the destination state, ends at the highest position reached.
 * pruning_threshold must not be negative (SR_EINVAL): a negative beam prunes a frame's best node with
 * the others and leaves the back-trace nothing to follow, in the reference as here.  -0.0, +inf and NaN
 * are legal (they prune strict losers only, or nothing).  N_u > T_u is allowed.  Limits: N_u <= 8189
 * (SR_ELIMIT; 20 bytes per position and 48 more in the 160 KiB LDS, where sr_align_corpus and the
 * forward-backward passes take 8192). */
SR_API int sr_align_corpus_pruned(sr_model* m, sr_corpus* c, const uint16_t* automata, const uint64_t* aut_off,
                           const double tdp[3], uint16_t silence_state, double pruning_threshold, int gmm_kernel,
                           uint16_t* out_states, double* out_cost);

/* ---- training-side caller of the scorer: Trainer::calc_am_score (Training.cpp:585-612) -----------------------
 * out[t] = MixtureModel::score(frame t, states[t]) for every frame of the corpus, i.e. the emission cost along
 * a given state path (an alignment from sr_align_corpus*).  The reference's average AM score is the sequential
 * sum of out[] divided by the frame count; the sum is left to the host so that it keeps the reference's order. */
SR_API int sr_path_scores_corpus(sr_model* m, sr_corpus* c, const uint16_t* states, int gmm_kernel, double* out);

/* ---- EM statistics: MixtureModel::accumulate (Mixtures.cpp:278-372) after reset_accumulators (:235-247) --------
 * Tying: accumulator row of every density (mixture order), as MixtureDensity{mean_idx, var_idx} (Types.hpp:19-27).
 * sr_model_load_mixset installs the file's own; models from sr_model_create default to one row per density. */
SR_API int sr_model_set_tying(sr_model* m, uint32_t n_mean, uint32_t n_var, const uint32_t* dens_mean, const uint32_t* dens_var);
SR_API int sr_model_tying_info(const sr_model* m, uint32_t* n_mean, uint32_t* n_var);
/* The topology a trainer needs to turn sr_accumulate_corpus' statistics into a MIXSET file (sr_mixset_write) or the next model
 * (sr_model_create_from_statistics): dens_off[n_states + 1], and the accumulator rows dens_mean[C], dens_var[C] of every density
 * in mixture order (MixtureModel::mixtures_, Mixtures.hpp:88).  Any pointer may be NULL. */
SR_API int sr_model_topology(const sr_model* m, uint32_t* dens_off, uint32_t* dens_mean, uint32_t* dens_var);
/* states[total_frames]: aligned mixture per frame (an alignment from sr_align_corpus*).  first_pass: density 0 of
 * the mixture gets every frame; else max_approx: the arg-min density; else soft memberships.  Outputs (host):
 * mean_acc[n_mean*dim], mean_w[n_mean], var_acc[n_var*dim] (starts at 1e-4 like the reference), var_w[n_var].
 * Rows are summed in frame order, so max-approx / first-pass results are bit-identical to the reference's; with
 * several GPUs every rank accumulates its shard and the four arrays are all-reduced (sum) by the caller. */
SR_API int sr_accumulate_corpus(sr_model* m, sr_corpus* c, const uint16_t* states, int first_pass, int max_approx,
                                double* mean_acc, double* mean_w, double* var_acc, double* var_w);
/* The single-device EM iteration without the PCIe round trip: call sr_accumulate_corpus with all four output arrays NULL -- the
 * statistics then stay in the corpus handle on the device -- and finalise them here into the next model (MixtureModel::finalize,
 * Mixtures.cpp:374-461; same topology and tying as `m`).  The tables are built in HBM; only the 2 x n weights and the variances
 * (for the host-side logarithms, see sr_model_create_from_statistics) cross the bus. */
SR_API int sr_model_create_from_accumulated(sr_model* m, sr_corpus* c, int pooling, int max_approx, sr_model** out);

/* ---- growing and pruning mixtures: the split and eliminate steps of Trainer::train (Training.cpp:44-235) ----------------------
 * These follow the reference's SCHEDULE (split / accumulate / finalize / eliminate / accumulate / finalize), not the bits of its
 * MixtureModel::split / eliminate: the operations are the ones specified here.  Both take the per mean row observation weights
 * [n_mean] from exactly one source: the host array mean_w as sr_accumulate_corpus returns it (c NULL), or the statistics a call of
 * sr_accumulate_corpus / sr_baum_welch_corpus with NULL outputs left in c (mean_w NULL).  `m` and `c` are untouched; *out is a
 * model in its own right (every scoring route works on it) with its own tying, which sr_model_topology / sr_model_tying_info report
 * and the next sr_accumulate_corpus fills.  out_parent (optional) [C']: the density of m every density of *out came from.  The
 * topology is host integer work; the per-density tables are written on the device from m's (FP64, no contraction), so C x D
 * doubles never cross the bus.  No atomics: two identical calls return identical bits.
 *
 * sr_model_split: density k with mean row r = dens_mean[k] splits iff mean_w[r] >= min_obs (a NaN weight does not).  A mixture
 * keeps its densities in their slots and the upper children of those that split follow, in their parents' order.  The lower child
 * keeps the parent's (mean row, var row); the j-th upper child, counted in mixture order over the whole model, gets mean row
 * n_mean + j and var row n_var + j (pooling 2, none) or the parent's var row (pooling 0 global, 1 mixture).  Per dimension i:
 * delta_i = epsilon * sqrt(1.0 / inv_var_i); lower child mean_i - delta_i, upper child mean_i + delta_i; both children get
 * logw - M_LN2 (host); inv_vars and norm of both, and every table of a density that does not split, are the parent's bits.  The
 * tables are a seed: the accumulate / finalize pass that follows re-estimates everything.
 *
 * sr_model_eliminate: a density survives iff its weight is >= min_obs; a non-empty mixture that would lose every density keeps its
 * heaviest one (ties: the lowest index; NaN ranks below everything; all NaN: the first); empty mixtures stay empty.  Survivors keep
 * their order and the bits of their means, inv_vars and norm; logw' = log(w_k / sum of the mixture's surviving weights, added in
 * mixture order) through the host's log.  Mean and var rows no survivor references are dropped, the rest renumbered in ascending
 * old index (sr_mixset_write's rule).
 *
 * Errors, all before any launch, *out left NULL: SR_EINVAL for a NULL m or out, min_obs or epsilon negative, NaN or infinite, an
 * unknown pooling, both weight sources or neither, a corpus of another model or one that holds no statistics of m; SR_ELIMIT for
 * a split model of 2^31 densities or more. */
SR_API int sr_model_split(sr_model* m, sr_corpus* c, const double* mean_w, double min_obs, double epsilon, int pooling,
                          sr_model** out, uint32_t* out_parent);
SR_API int sr_model_eliminate(sr_model* m, sr_corpus* c, const double* mean_w, double min_obs, sr_model** out, uint32_t* out_parent);
/* The per-density tables in sr_model_create's shape: means, inv_vars [C x dim], norm, logw [C]; any pointer may be NULL.  A model
 * from sr_model_create fed with them (plus sr_model_set_tying) scores bit-identically.  For checkpoints: a split model has no
 * statistics to write until the next E-step. */
SR_API int sr_model_tables(const sr_model* m, double* means, double* inv_vars, double* norm, double* logw);

/* ---- Baum-Welch: forward-backward over the aligner's automata and topology ---------------------------------------
 * Same automata, 0-1-2 topology and transition penalties as sr_align_corpus (keyed on the SOURCE position; any jump out of
 * silence costs `forward`), summed over all paths instead of minimised.  F_u = -log sum_paths exp(-cost), so
 * V_u - log(#paths) <= F_u <= V_u for the Viterbi cost V_u.  Requires 1 <= N_u <= 2 T_u - 1 (a path must exist; unlike
 * sr_align_corpus N_u > T_u is allowed) and N_u <= 8192 (SR_ELIMIT).  T_u = 1 gives F_u = e(0, automaton[0]), where
 * sr_align_corpus returns +inf.  Forbidden jumps (+inf penalties) and unreachable cells stay +inf, never NaN.
 * gamma_t(k) = sum over the positions s carrying mixture k of P(s_t = s | X).  Workspace: 8 bytes per (frame, position) for
 * the utterances processed together, at most SRGPU_FB_MB MiB (default 1024); an utterance that alone needs more: SR_ELIMIT.
 * gmm_kernel resolves as in sr_align_corpus (SR_GMM_DEFAULT: listed exact scoring, the reference's bits).  SR_EINVAL also for
 * posterior_floor negative or NaN, max_items outside 1 .. 65535 with posterior outputs, and a partial set of optional outputs. */

/* out_cost[n_utts] = F_u (required).  Posteriors in AlignmentItem shape, all three optional (all or none): out_count[total_frames],
 * out_state[total_frames * max_items], out_weight[total_frames * max_items] -- per frame the mixtures of the utterance's automaton
 * with gamma > 0 and gamma >= posterior_floor, largest first (ties: smaller id first), at most max_items, not renormalised;
 * entries past out_count are 0. */
SR_API int sr_state_posteriors_corpus(sr_model* m, sr_corpus* c, const uint16_t* automata, const uint64_t* aut_off,
                                      const double tdp[3], uint16_t silence_state, int gmm_kernel, double posterior_floor,
                                      uint32_t max_items, double* out_cost, uint16_t* out_count, uint16_t* out_state,
                                      double* out_weight);

/* One Baum-Welch E-step: forward-backward + posterior-weighted statistics in one device pass, no posteriors crossing the bus.
 * Accumulators, seeds and formulas as sr_accumulate_corpus; every frame contributes, for each mixture k with gamma_t(k) > 0 and
 * >= posterior_floor, each density d of k with weight gamma_t(k) * p_d (p_d: density 0 on first_pass, else the arg-min with
 * max_approx, else the soft membership with its < 1e-8 drop).  Every accumulator row is summed frames in order, then mixtures in
 * ascending id, then densities in mixture order, without atomics: two identical calls return identical bits.  Statistics of
 * corpus shards add up like sr_accumulate_corpus'.  Output arrays as sr_accumulate_corpus: all four, or all NULL to keep the
 * statistics in the corpus handle for sr_model_create_from_accumulated. */
SR_API int sr_baum_welch_corpus(sr_model* m, sr_corpus* c, const uint16_t* automata, const uint64_t* aut_off,
                                const double tdp[3], uint16_t silence_state, int gmm_kernel, double posterior_floor,
                                int first_pass, int max_approx, double* out_cost, double* mean_acc, double* mean_w,
                                double* var_acc, double* var_w);

/* ---- fMLLR speaker adaptation (constrained MLLR, Gales 1998) -----------------------------------------------------------
 * One affine feature transform W_s = [A_s b_s] (D x (D+1), row-major) per speaker, estimated by maximum likelihood from an
 * alignment or from posteriors; the model is untouched.  With xi_t = (x_t1 .. x_tD, 1), iv = 1/var and mu of density d, speaker s
 * collects over the pairs (t, d, gamma) of its utterances (utt_speaker[u] < n_speakers names utterance u's speaker; a speaker's
 * utterances need not be contiguous), everything in FP64:
 *   out_beta[s]          = sum gamma
 *   out_k[s][i][j]       = sum gamma mu_di iv_di xi_tj              (D x (D+1))
 *   out_G[s][i][j][k]    = sum gamma iv_di xi_tj xi_tk              (D x (D+1) x (D+1): full storage, both triangles written from one
 *                                                                    sum, exactly symmetric)
 * sr_fmllr_statistics_corpus takes exactly the pairs sr_accumulate_corpus forms with first_pass = 0 (the arg-min density of
 * states[t] at weight 1 with max_approx, else the soft memberships with their < 1e-8 drop); sr_fmllr_statistics_bw_corpus exactly
 * those of sr_baum_welch_corpus (gamma_t(k) x membership, the same floor rule; out_cost[n_utts] = F_u).  A frame's pairs are folded in
 * pair order into two D-vectors; G and k are then contractions over the speaker's frames on the FP64 matrix cores, the products
 * xi_tj xi_tk formed in FP64 from the float features.  Determinism: no atomics; a speaker's frames are summed in corpus order, cut
 * into segments of 1024 frames whose partial sums are added in ascending order; the order does not depend on the launch, so two
 * identical calls return identical bits.  A speaker without frames gets zeros; statistics of corpus shards add up like
 * sr_accumulate_corpus'.  Device memory: the three outputs, 2 x 8 bytes per (frame, D+1 rounded up to 16) and 8 bytes per (segment,
 * that row count, (D+1)(D+2)/2 + D+1 columns each rounded up to 16).
 * Errors, all before any launch: SR_ELIMIT for a dimension above 63 and for n_speakers * D * (D+1)^2 * 8 bytes beyond a quarter of
 * the free device memory; SR_EINVAL for utt_speaker[u] >= n_speakers, n_speakers == 0 or a NULL output; otherwise the errors of
 * sr_accumulate_corpus / sr_baum_welch_corpus. */
SR_API int sr_fmllr_statistics_corpus(sr_model* m, sr_corpus* c, const uint16_t* states, const uint32_t* utt_speaker,
                                      uint32_t n_speakers, int max_approx, double* out_beta, double* out_k, double* out_G);
SR_API int sr_fmllr_statistics_bw_corpus(sr_model* m, sr_corpus* c, const uint16_t* automata, const uint64_t* aut_off,
                                         const double tdp[3], uint16_t silence_state, int gmm_kernel, double posterior_floor,
                                         const uint32_t* utt_speaker, uint32_t n_speakers, int max_approx, double* out_cost,
                                         double* out_beta, double* out_k, double* out_G);

/* The transforms from the statistics; host code, no device.  W[n_speakers x D x (D+1)] is in/out: the estimate starts from the caller's
 * value (identity [I 0] is the usual start).  Auxiliary function Q(W) = beta log|det A| - 1/2 sum_i (w_i G_i w_i^T - 2 w_i k_i^T).
 * One sweep updates rows i = 0 .. D-1 in order: with p_i = (row i of the cofactor matrix of the current A, 0),
 *   w_i = (alpha p_i + k_i) G_i^-1,  alpha a root of alpha^2 (p_i G_i^-1 p_i^T) + alpha (p_i G_i^-1 k_i^T) - beta = 0,
 * the root with the larger beta log|alpha p_i G_i^-1 p_i^T + p_i G_i^-1 k_i^T| - 1/2 w_i G_i w_i^T + w_i k_i^T; every row update
 * maximises Q over its row, so Q never falls.  Optional outputs: out_aux[s * (n_sweeps+1) + j] = Q_s after j sweeps (j = 0: the
 * start), out_logdet[s] = log|det A_s| of the result.  out_status[s]: 0 estimated; 1 beta_s < min_count, W_s left as given; 2 some
 * G_i not positive definite (its Cholesky factorisation fails) or A singular on the way, W_s restored to the value given.  With
 * status 1 or 2 out_aux holds Q of the W given at every j (NaN where it has none) and out_logdet its log|det A|.
 * SR_EINVAL for dim == 0, a NULL input or out_status, min_count negative or NaN, n_sweeps == 0. */
SR_API int sr_fmllr_estimate(uint32_t dim, uint32_t n_speakers, const double* beta, const double* k, const double* G,
                             uint32_t n_sweeps, double min_count, double* W, double* out_aux, double* out_logdet,
                             int32_t* out_status);

/* The adapted corpus: a new resident corpus with c's frame offsets whose row t is (float) acc_i, acc_i starting at b_i and taking
 * acc_i = acc_i + A_ij * (double) x_tj for j ascending, no fused multiply-add (the order of operations is the specification: a loop
 * over j in FP64 reproduces it bit for bit), with [A b] = W[utt_speaker[u]] of t's utterance.  `c` stays valid (an asynchronous
 * upload of it is waited for first); *out belongs to the same model, is accepted by every entry point that takes a corpus and is
 * destroyed with sr_corpus_destroy like any other: it allocates its own buffers rather than adopting the ones the model parked from
 * its last destroyed corpus, and parks its own on destruction.  SR_EINVAL / SR_ELIMIT as for the statistics (W NULL: SR_EINVAL). */
SR_API int sr_corpus_transform(sr_model* m, sr_corpus* c, const uint32_t* utt_speaker, uint32_t n_speakers, const double* W,
                               sr_corpus** out);

/* ---- MLLR of the means with regression classes (Leggetter & Woodland 1995) ----------------------------------------------------
 * One affine transform of the means W_{s,r} = [A b] (D x (D+1), row-major, the layout of sr_fmllr_estimate) per speaker s and
 * regression class r; dens_class[n_densities] (mixture order, < n_classes) names every density's class.  With the extended mean
 * xi_d = (mu_d1 .. mu_dD, 1), iv_d = 1/var_d, the adapted mean is mu'_d = W_{s,r} xi_d.  Over the pairs (t, d, gamma) of speaker s'
 * utterances, everything in FP64:
 *   occ[s][d]           = sum_t gamma             x_acc[s][d][i] = sum_t gamma x_ti       (the pairs of (s, d), frames ascending)
 *   out_beta[s][r]      = sum_{d in r} occ[s][d]
 *   out_k[s][r][i][j]   = sum_{d in r} (iv_di x_acc[s][d][i]) xi_dj                       (D x (D+1))
 *   out_G[s][r][i][j][k] = sum_{d in r} (occ[s][d] iv_di) xi_dj xi_dk                     (D x (D+1) x (D+1): full storage, both
 *                                                                                          triangles from one sum, exactly symmetric)
 * the densities of a group (s, r) in ascending density id.  Q(W) = -1/2 sum_i (w_i G_i w_i^T - 2 w_i k_i^T), maximised at
 * w_i = k_i G_i^-1 per row.  sr_mllr_statistics_corpus takes exactly the pairs of sr_fmllr_statistics_corpus,
 * sr_mllr_statistics_bw_corpus exactly those of sr_fmllr_statistics_bw_corpus (out_cost[n_utts] = F_u).  Outputs: [S x R],
 * [S x R x D x (D+1)], [S x R x D x (D+1) x (D+1)], S = n_speakers, R = n_classes; a group without pairs gets zeros, a class without
 * densities is allowed.  Determinism: no atomics.  The pairs are sorted stably by speaker * n_densities + density, so that occ and x_acc
 * add a (speaker, density)'s pairs in the order they were formed (frames ascending); the occupied (speaker, density) entries of a
 * group, in ascending density id, are cut into segments of 1024 whose partial sums -- chains of FP64 matrix-core accumulations, the
 * products xi_dj xi_dk formed in FP64 -- are added in ascending order.  Two identical calls return identical bits; statistics of corpus
 * shards add up.  Device memory: the three outputs, 36 bytes per pair, 8 (D + 4) bytes per entry and 8 bytes per (segment, D+1 rounded
 * up to 16, (D+1)(D+2)/2 + D+1 columns each rounded up to 16).
 * Errors, all before any launch: SR_EINVAL for dens_class[d] >= n_classes, n_classes == 0, a NULL output or dens_class, and the
 * SR_EINVAL cases of the fMLLR calls; SR_ELIMIT for a dimension above 63, for n_speakers * n_densities >= 2^32 - 1 (the 32-bit keys)
 * and for outputs (8 S R (1 + D (D+1) (D+2)) bytes) beyond a quarter of the free device memory; otherwise the errors of
 * sr_accumulate_corpus / sr_baum_welch_corpus. */
SR_API int sr_mllr_statistics_corpus(sr_model* m, sr_corpus* c, const uint16_t* states, const uint32_t* utt_speaker,
                                     uint32_t n_speakers, const uint32_t* dens_class, uint32_t n_classes, int max_approx,
                                     double* out_beta, double* out_k, double* out_G);
SR_API int sr_mllr_statistics_bw_corpus(sr_model* m, sr_corpus* c, const uint16_t* automata, const uint64_t* aut_off,
                                        const double tdp[3], uint16_t silence_state, int gmm_kernel, double posterior_floor,
                                        const uint32_t* utt_speaker, uint32_t n_speakers, const uint32_t* dens_class,
                                        uint32_t n_classes, int max_approx, double* out_cost, double* out_beta, double* out_k,
                                        double* out_G);

/* The transforms from the statistics over a regression-class tree; host code, no device.  parent[n_nodes]: nodes 0 .. n_classes-1 are
 * the leaves (the base classes of the statistics), parent[v] is -1 for a root or an inner node (>= n_classes) with parent[v] > v;
 * n_nodes == n_classes with every parent -1 means no tree.  A node's statistics are the sum of its leaves', added in ascending leaf
 * id.  Every leaf r of speaker s takes the transform w_i = k_i G_i^-1 (a Cholesky factorisation and two triangular solves per row) of
 * its lowest ancestor, itself first, whose beta >= min_count and whose every G_i factorises (positive definite, finite solution);
 * out_node[s * n_classes + r] is that node, or -1 where none qualifies: W[s][r] is then left as given, bit for bit.
 * W[n_speakers x n_classes x D x (D+1)] is in/out like sr_fmllr_estimate's (the value given only enters out_aux).  Optional
 * out_aux[(s * n_classes + r) * 2 + {0, 1}] = Q of the node used, at the W given and at the result (NaN for node -1).
 * SR_EINVAL for dim == 0, a NULL input or out_node, min_count negative or NaN, n_classes == 0, n_nodes < n_classes or a malformed
 * tree (a parent that is not -1, or not above its child, or a leaf, or >= n_nodes). */
SR_API int sr_mllr_estimate(uint32_t dim, uint32_t n_speakers, uint32_t n_classes, uint32_t n_nodes, const int32_t* parent,
                            const double* beta, const double* k, const double* G, double min_count, double* W, int32_t* out_node,
                            double* out_aux);

/* The adapted model of one speaker: a new device model with m's topology and tying whose means are mu'_di = acc, acc starting at b_i
 * and taking acc = acc + A_ij * mu_dj for j ascending in FP64, no fused multiply-add (the loop is the specification), with
 * [A b] = W[dens_class[d]], W[n_classes x D x (D+1)].  inv_vars, norm and logw keep m's bits; the scoring kernels' packed tables are
 * built on first use like those of sr_model_split's result.  W = [I 0] gives m's means bit for bit (finite means; a mean of -0.0
 * comes out as +0.0).  The features of that speaker are then uploaded to the new model (a corpus belongs to one model).
 * SR_EINVAL for a NULL argument, n_classes == 0, dens_class[d] >= n_classes, or two densities that share a mean row (sr_model_set_tying)
 * in different classes; SR_ELIMIT for a dimension above 63. */
SR_API int sr_model_transform_means(sr_model* m, const uint32_t* dens_class, uint32_t n_classes, const double* W, sr_model** out);

/* ---- MAP adaptation of the means and weights (Gauvain & Lee 1994, relevance form) ---------------------------------------------
 * Every density that a speaker's data reached moves towards that data, every other density stays where it was; nothing ties one
 * density's update to another's.  The statistics are the per-(speaker, density) sums that the MLLR statistics form on the way:
 * Pairs.  The (frame, density, gamma) pairs are exactly those of sr_mllr_statistics_corpus / sr_mllr_statistics_bw_corpus; a dropped
 *   pair stays dropped.
 * Entries.  An entry is a (speaker, density) with at least one kept pair.  Entries come out in ascending (speaker, density); speaker
 *   s owns entries out_ent_off[s] .. out_ent_off[s + 1]; out_dens is the density id in mixture order.
 * Values.  Everything is FP64 with no fused multiply-add: occ = sum gamma, x[i] = sum gamma * (double) x_ti.
 * Order of summation (this is the specification).  An entry's pairs are in the order they were formed, frames ascending.  They are cut
 *   into segments of 1024 pairs.  Within a segment there is one chain per value, starting at 0.0: sum = sum + gamma * (double) x, the
 *   product rounded, then the addition.  The segments' partials are then added in ascending order to a total that starts at 0.0.  The
 *   order depends on the pairs alone, never on the launch; no atomics, so two identical calls return identical bits.  Statistics of
 *   corpus shards add up, as sr_accumulate_corpus' do.
 * Sizing (the convention of sr_word_lattice_corpus).  out_ent_off[n_speakers + 1] is required and always written.  The three entry
 *   arrays -- out_dens[cap], out_occ[cap], out_x[cap x D] -- are given all or none.  None: the sizing call, SR_OK with the counts in
 *   out_ent_off.  Given but the total exceeds cap: nothing is written to the arrays, out_ent_off still holds the counts needed,
 *   SR_EINVAL.  With max_approx and an alignment every frame forms one pair, so cap = total_frames always suffices.
 * Errors, all before any launch: SR_EINVAL for a NULL m, c or out_ent_off, a partial set of arrays, n_speakers == 0,
 *   utt_speaker[u] >= n_speakers; SR_ELIMIT for n_speakers * n_densities >= 2^32 - 1 (the 32-bit keys, as MLLR); otherwise the errors of
 *   sr_accumulate_corpus / sr_baum_welch_corpus.  There is no dimension limit beyond the model's own 160: nothing here uses the matrix
 *   cores.  Device memory: 52 bytes per pair, 8 (D + 2) bytes per entry and 8 (D + 1) per segment of an entry of more than one. */
SR_API int sr_map_statistics_corpus(sr_model* m, sr_corpus* c, const uint16_t* states, const uint32_t* utt_speaker,
                                    uint32_t n_speakers, int max_approx, uint64_t cap, uint64_t* out_ent_off /*[n_speakers+1]*/,
                                    uint32_t* out_dens /*[cap]*/, double* out_occ /*[cap]*/, double* out_x /*[cap*D]*/);
SR_API int sr_map_statistics_bw_corpus(sr_model* m, sr_corpus* c, const uint16_t* automata, const uint64_t* aut_off,
                                       const double tdp[3], uint16_t silence_state, int gmm_kernel, double posterior_floor,
                                       const uint32_t* utt_speaker, uint32_t n_speakers, int max_approx, double* out_cost,
                                       uint64_t cap, uint64_t* out_ent_off, uint32_t* out_dens, double* out_occ, double* out_x);

/* The adapted model from one speaker's slice of the statistics (dens strictly ascending): a new device model with prior's topology
 * and tying, built like sr_model_transform_means' result (the scoring kernels' packed tables on first use).
 * Means.  For a mean row r (sr_model_set_tying): O_r is the sum of occ over the row's entries, X_ri the sum of x_i over the same
 *   entries, both in ascending density id, each a chain from 0.0.  mu'_ri = (tau * mu_ri + X_ri) / (tau + O_r): one multiplication,
 *   two additions and one division, each rounded, no contraction.  Every density of the row gets those bits.  A row without an entry
 *   keeps prior's bits exactly.
 * inv_vars and norm are always prior's bits; without update_weights, logw is too.
 * Weights.  With update_weights, for every mixture that has at least one entry: w_d = exp(logw_d) through the host's libm,
 *   n_d = tau_w * w_d + occ_d (occ_d = 0.0 where there is no entry), logw'_d = log(n_d / N) with N the sum of n_d in mixture order,
 *   through the host's log (sr_model_eliminate's rule for where the logarithm is taken).  Mixtures without an entry keep their bits.
 * prior may be any model of the right topology -- the result of sr_model_transform_means gives MAP with an MLLR-adapted prior.
 * n_entries == 0 is valid: every table equals prior's, bit for bit.
 * Errors, all before any launch, *out left NULL: SR_EINVAL for a NULL prior or out, NULL arrays with n_entries > 0, dens not strictly
 * ascending or >= n_densities, an occ that is not finite or not > 0, an x that is not finite, tau negative, NaN or infinite, and with
 * update_weights a tau_w that is not finite or not > 0. */
SR_API int sr_model_map_adapt(sr_model* prior, uint64_t n_entries, const uint32_t* dens, const double* occ, const double* x,
                              double tau, int update_weights, double tau_w, sr_model** out);

/* ---- MLLT: the global semi-tied covariance transform (Gales 1999, one transform class) --------------------------------------------
 * One square matrix A for the feature space, y = A x with the means following by mu' = A mu, chosen so that the model's diagonal
 * covariances fit as well as they can: the "MLLT" of the LDA + MLLT + fMLLR pipeline.  With z = (double) x_t - mu_d and iv = 1/var of
 * density d, the pairs (t, d, gamma) -- exactly those of the fMLLR statistics above, from an alignment or from a Baum-Welch pass --
 * collect, everything in FP64,
 *   beta       = sum gamma
 *   G[i][j][k] = sum (gamma iv_di) z_j z_k                    i, j, k < D      (out_G[D x D x D], full storage)
 * z is formed with one rounding, z_j z_k with one more, the product with gamma iv_di inside the matrix instruction.
 * Summation order: the pairs in pair order (frames ascending, a frame's densities in mixture order; a dropped pair -- membership below
 * 1e-8, empty mixture -- keeps its place with weight 0) are cut into segments of 1024; within a segment one chain of
 * v_mfma_f64_16x16x4_f64 accumulations per output, pairs ascending; then the segments' partial sums, ascending.  No atomics: two
 * identical calls return identical bits, and G is exactly symmetric in (j, k) (both triangles are written from one sum).
 * Limits: D <= 63 (SR_ELIMIT).  Memory: the partial sums of a segment are R x C doubles, R = D + 1 rounded up to 16,
 * C = D (D + 1) / 2 + 1 rounded up to 16 (0.3 MB at D = 39, i.e. 300 MB per million pairs); they live in a workspace of SRGPU_MLLT_MB
 * MiB (default 256, read when the model is made), and when the segments do not fit, the call runs in rounds of consecutive segments
 * whose reduction continues the same chain of additions: the result's bits do not depend on the workspace.  One segment that does not
 * fit: SR_ELIMIT (none does at D <= 63: at most 64 x 2032 doubles, below 1 MiB).  SR_EINVAL for a NULL output; otherwise the
 * errors of sr_accumulate_corpus / sr_baum_welch_corpus.  All errors are found before any launch and leave the outputs untouched.
 * Statistics of corpus shards add up; a corpus without live pairs gives zeros.
 *
 * Applying it needs no call of its own: with W = [A 0] (D x (D+1)), the adapted corpus is sr_corpus_transform with one speaker
 * (utt_speaker all 0), the adapted means are sr_model_transform_means with one class (dens_class all 0); upload or transform the
 * features for the adapted model, and let the next sr_accumulate_corpus / sr_baum_welch_corpus pass re-estimate the variances in the
 * new basis.  Costs of the adapted pair compare with the original's after subtracting log|det A| per frame. */
SR_API int sr_mllt_statistics_corpus(sr_model* m, sr_corpus* c, const uint16_t* states, int max_approx, double* out_beta /*[1]*/,
                                     double* out_G /*[D*D*D]*/);
/* out_cost[n_utts] as sr_baum_welch_corpus */
SR_API int sr_mllt_statistics_bw_corpus(sr_model* m, sr_corpus* c, const uint16_t* automata, const uint64_t* aut_off,
                                        const double tdp[3], uint16_t silence_state, int gmm_kernel, double posterior_floor,
                                        int max_approx, double* out_cost /*[n_utts]*/, double* out_beta, double* out_G);

/* The estimate (host code, no device).  Q(A) = beta log|det A| - 1/2 sum_i a_i G_i a_i^T.  A sweep updates rows i = 0 .. D-1 in
 * order: a_i = alpha p_i G_i^-1 with p_i row i of the cofactor matrix of the current A and alpha = +sqrt(beta / (p_i G_i^-1 p_i^T)).
 * Every row update maximises Q over its row, so Q never falls; both roots give the same Q, and the positive one makes det A > 0
 * after every update, which makes the result unique.  A[D x D] holds the start (usually I) and receives the result.
 * out_aux[n_sweeps + 1] (optional): Q after j sweeps (j = 0: the A given).  out_logdet (optional): log|det A| of the result.
 * *out_status: 0 estimated; 1 beta < min_count, A left as given; 2 some G_i not positive definite or A singular on the way, A restored
 * bit for bit.  With status 1 or 2 out_aux holds Q of the A given at every j (NaN where it has none).
 * SR_EINVAL for dim == 0, a NULL G, A or out_status, min_count negative or NaN, n_sweeps == 0. */
SR_API int sr_mllt_estimate(uint32_t dim, double beta, const double* G, uint32_t n_sweeps, double min_count, double* A /*[D*D] in/out*/,
                            double* out_aux /*[n_sweeps+1], optional*/, double* out_logdet /*optional*/, int32_t* out_status);

/* ---- LDA with frame splicing: the step the LDA + MLLT + fMLLR pipeline starts with -----------------------------------------------
 * A frame is stacked with its `context` neighbours on either side and the stack is projected to p dimensions so that the classes
 * (usually the aligned states, silence left out) are separated as well as a linear map can.  With D = m's dimension, c = context,
 * E = (2c + 1) D, the spliced vector of frame t in an utterance whose frames are [a, b) is
 *   z_t[(o + c) D + j] = (double) x[min(max(t + o, a), b - 1)][j]          o = -c .. c, j < D
 * (edge frames repeated; a one-frame utterance splices 2c + 1 copies of its frame).  It is never stored: the kernels gather it from
 * the resident float corpus.
 *
 * Statistics.  The class of frame t is class_of_state[states[t]], or states[t] itself when class_of_state is NULL; a frame of class
 * SR_LDA_SKIP is left out of everything.  The kept frames, in corpus order, are the items:
 *   out_count[k]       = the number of items of class k (exact)
 *   out_sum[k][j]      = sum z_tj over the items of class k                   [n_classes x E]
 *   out_scatter[j][k]  = sum z_tj z_tk over all items                         [E x E], full storage, both triangles written from one
 *                                                                              sum: exactly symmetric
 * Both factors of a product are floats widened to double, so every product is exact in FP64 and only the additions round.
 * Summation order, fixed by the item order alone: the items are cut into segments of 1024; within a segment one chain of
 * v_mfma_f64_16x16x4_f64 accumulations per output, items ascending; then the segments' partial sums, ascending.  The class sums do
 * the same over a class's own items (a stable grouping by class keeps them in corpus order), with plain FP64 additions within a
 * segment.  No atomics: two identical calls return identical bits.  A class without items, and a call without kept frames, gives
 * zeros; statistics of corpus shards add up.
 * Limits: E <= 512 (SR_ELIMIT); D itself may be anything a model allows (the statistic never touches the model's tables).  Memory:
 * a segment's partial sums are the (P (P + 1) / 2) blocks of 64 x 64 doubles of the upper triangle, P = E / 64 rounded up (0.7 MB at
 * E = 351); they live in a workspace of SRGPU_LDA_MB MiB (default 256, read when the model is made), and when the segments do not fit,
 * the call runs in rounds of consecutive segments whose reduction continues the same chain of additions: the result's bits do not
 * depend on the workspace.  A round holds at least one segment (at most 1.2 MB), however small the variable.
 * Errors, all before any launch and with the outputs untouched: SR_EINVAL for a NULL output, n_classes == 0, a state >= n_states, a
 * class that is neither < n_classes nor SR_LDA_SKIP; SR_ELIMIT for E > 512, for outputs beyond a quarter of the free device
 * memory and for n_classes x (E / 256 rounded up) beyond 2^31 - 1; otherwise the errors of any corpus call (a corpus of another model). */
#define SR_LDA_SKIP 0xFFFFFFFFu
SR_API int sr_lda_statistics_corpus(sr_model* m, sr_corpus* c, const uint16_t* states, uint32_t context,
                                    const uint32_t* class_of_state /*[n_states] or NULL = identity*/, uint32_t n_classes,
                                    double* out_count /*[n_classes]*/, double* out_sum /*[n_classes x E]*/, double* out_scatter /*[E x E]*/);

/* The estimate (host code, no device).  N = sum count; mu_k = sum_k / count_k over the classes with count > 0; mu = (sum of all
 * sums) / N;  W = (scatter - sum_k count_k mu_k mu_k^T) / N;  B = sum_k count_k mu_k mu_k^T / N - mu mu^T.  With the Cholesky
 * factor W = L L^T and the symmetric eigendecomposition of L^-1 B L^-T (Householder tridiagonalisation, implicit QR), eigenvalues
 * descending into out_eig[E] (optional), A = the first p eigenvectors, as rows, times L^-1; every row's sign makes its entry of
 * largest magnitude positive (the first such entry on a tie).  M = [A b] (p x (E+1), row-major): b_i = -(sum_j A_ij mu_j, j
 * ascending) with remove_mean, else 0.  The result satisfies A W A^T = I_p and A B A^T = diag(eig[0 .. p-1]).  Rows beyond the rank
 * of B (classes - 1) and rows of equal eigenvalues are one choice among many.
 * *out_status: 0 estimated; 1 N < min_count or fewer than two classes with frames; 2 W not positive definite (fewer frames than E,
 * for one) or something non-finite.  With status 1 or 2 M is left as given, bit for bit, and out_eig is not written.
 * SR_EINVAL for E == 0, p == 0 or p > E, n_classes == 0, a NULL input, M or out_status, min_count negative or NaN. */
SR_API int sr_lda_estimate(uint32_t E, uint32_t n_classes, const double* count, const double* sum, const double* scatter, uint32_t p,
                           int remove_mean, double min_count, double* M /*[p x (E+1)] in/out*/, double* out_eig /*[E], optional*/,
                           int32_t* out_status);

/* The projected corpus: a new resident corpus of `target` -- any model of dimension p on m's device -- with c's frame offsets whose
 * row t, column i is (float) acc, acc starting at M[i][E] and taking acc = acc + M[i][n] * z_tn for n ascending in FP64, no fused
 * multiply-add (the loop is the specification, as for sr_corpus_transform).  A placeholder model from sr_model_create (p dimensions,
 * the states of the alignment with one density each, any finite tables) is enough to hold the corpus for a first-pass
 * sr_accumulate_corpus and sr_model_create_from_accumulated, which give the first model of the projected space.  `c` stays valid
 * (an asynchronous upload of it is waited for first); *out is accepted by every entry point that takes a corpus of `target`, allocates
 * its own buffers like sr_corpus_transform's result, is destroyed with sr_corpus_destroy, and must be destroyed before `target`.
 * SR_EINVAL for a NULL M, out or target and a target on another device; SR_ELIMIT for E > 512. */
SR_API int sr_corpus_splice_transform(sr_model* m, sr_corpus* c, sr_model* target, uint32_t context, const double* M /*[p x (E+1)]*/,
                                      sr_corpus** out);

/* ---- the audio front end: PCM samples or static cepstra in, a resident corpus out -------------------------------------------------
 * What SignalAnalysis does before the recogniser sees a frame (SignalAnalysis.cpp: pre-emphasis, Hamming window, FFT, mel filterbank,
 * DCT; then process_features: deltas, normalisation), on the device.  A front end hangs on a model -- for its device and its
 * dimension, like a lexicon -- and is destroyed before it.  mfcc == NULL makes one that takes cepstra only.
 *
 * The MFCC stage.  The reference's source is not what is matched here; this definition is (tests/frontend_reference.py restates it in
 * float64).  An utterance of N samples has T = 0 frames if N < window, else T = 1 + (N - window) / shift (integer division); frame t
 * covers samples [t shift, t shift + window), no padding.
 *   pre-emphasis   y[n] = x[n] - preemphasis * x[n - 1] over the utterance, x[-1] = 0 before the utterance's first sample only
 *   window         w[i] = 0.54 - 0.46 cos(2 pi i / (window - 1)); the frame is zero-extended to n_fft
 *   power          P[k] = |X[k]|^2, k = 0 .. n_fft / 2, X the DFT of the windowed frame
 *   filterbank     n_mel triangles whose n_mel + 2 edge frequencies are equally spaced in mel(f) = 2595 log10(1 + f / 700) between f_low
 *                  and f_high; bin k (f_k = k sample_rate / n_fft) has the weight max(0, min((f_k - l) / (c - l), (r - f_k) / (r - c))) in
 *                  the filter of edges l < c < r;  E_m = sum_k weight P[k]
 *   logarithm      L_m = log(max(E_m, energy_floor))
 *   DCT-II         c_i = sqrt(2 / n_mel) sum_m L_m cos(pi i (m + 1/2) / n_mel), i = 0 .. n_cepstra - 1; c_0 is the energy-like component
 * Window, twiddles, filter weights and the DCT matrix (the factor folded in) are computed on the host in double and stored as float;
 * the device works in FP32 on them, in an order of its own (a half-length complex transform of radix-4 stages; a filter's bins and a
 * cepstrum's filters ascending).  No atomics: two identical calls return identical bits, and an utterance gives the same bits alone
 * as inside any batch.
 * Limits (SR_ELIMIT): n_fft a power of two in 64 .. 2048, window <= n_fft, n_mel <= 64, an utterance of more than 65535 frames.
 * SR_EINVAL: shift == 0, window < 2, n_cepstra == 0 or > n_mel, a sample rate that is not positive and finite, f_low < 0,
 * f_high > sample_rate / 2, f_low >= f_high, a filter without a bin of positive weight, energy_floor not positive and finite, a
 * pre-emphasis that is not finite, flags != 0, n_cepstra != n_static.
 *
 * The post-processing stage is sr::FeaturePostProcessor::process_features (include/sr_sietill.hpp) bit for bit, utterance by utterance:
 * the n_static statics; the deltas of the first n_first of them, frame a = min(max(t, deriv_step), T - 1) minus frame a - deriv_step (frame
 * 0 if a < deriv_step); the delta-deltas of the first n_second deltas, the delta at frame min(t, T - 1 - deriv_step) + deriv_step (frame
 * T - 1 where T <= deriv_step) minus the delta at t; with mean / stddev, (float)((double)x - mean[k]) and then (float)((double)x /
 * stddev[k]); with energy_max_norm, component 0 minus its maximum over the utterance.  Float subtraction, FP64 subtraction and
 * division are correctly rounded and a maximum has no order, so the device's rows carry the host loop's bits.
 * SR_EINVAL: the model's dimension != n_static + n_first + n_second, n_static == 0, n_first > n_static, n_second > n_first,
 * deriv_step == 0, only one of mean and stddev given.
 *
 * Every check comes before any launch; a refused call leaves *out NULL and the host outputs untouched.  An utterance without frames
 * is allowed, and so is a corpus of none. */
typedef struct {
  double sample_rate;            /* Hz */
  uint32_t window, shift;        /* samples */
  uint32_t n_fft, n_mel, n_cepstra;
  double f_low, f_high;          /* Hz: the filterbank's outer edges */
  float preemphasis, energy_floor;
  uint32_t flags;                /* 0 */
} sr_mfcc_params;
typedef struct {
  uint32_t n_static, n_first, n_second, deriv_step;  /* SignalAnalysis.cpp:53-56: 12, 12, 1, 3 */
  int32_t energy_max_norm;
  const double* mean;            /* [n_static + n_first + n_second] each, or both NULL: no mean / deviation normalisation */
  const double* stddev;
} sr_feature_post_params;
typedef struct sr_frontend sr_frontend;
SR_API int sr_frontend_create(sr_model* m, const sr_mfcc_params* mfcc /*NULL: cepstra in only*/, const sr_feature_post_params* post,
                              sr_frontend** out);
SR_API int sr_frontend_destroy(sr_frontend* fe);
/* *frames = T of an utterance of n_samples (SR_EINVAL for a front end without an MFCC stage) */
SR_API int sr_frontend_frames(const sr_frontend* fe, uint64_t n_samples, uint64_t* frames);
/* samples of utterance u: samples[sample_off[u] .. sample_off[u + 1]), sample_off[0] == 0 and non-decreasing (else SR_EINVAL).  *out: a
 * resident corpus of the front end's model, both stages applied, with buffers of its own like sr_corpus_transform's result: accepted
 * wherever a corpus of that model is, destroyed with sr_corpus_destroy before the model.  out_frame_off[n_utts + 1]: its frame offsets. */
SR_API int sr_corpus_from_audio(sr_frontend* fe, const int16_t* samples, const uint64_t* sample_off, uint32_t n_utts, sr_corpus** out,
                                uint64_t* out_frame_off /*[n_utts+1]*/);
/* the post-processing stage alone, on static cepstra [frames x n_static] with sr_corpus_upload's frame_off (the reference's .mm2 files) */
SR_API int sr_corpus_from_cepstra(sr_frontend* fe, const float* cepstra, const uint64_t* frame_off, uint32_t n_utts, sr_corpus** out);
/* the MFCC stage alone, back to the host: out_cepstra [frames x n_cepstra] -- room for sum_u sr_frontend_frames(N_u) rows -- and the frame
 * offsets; what a caller writes as .mm2 and estimates the normalisation's mean and deviation from */
SR_API int sr_mfcc_corpus(sr_frontend* fe, const int16_t* samples, const uint64_t* sample_off, uint32_t n_utts, float* out_cepstra,
                          uint64_t* out_frame_off /*[n_utts+1]*/);

/* ---- vocal-tract-length normalisation (VTLN): warped filterbanks, the warp search, warped corpora --------------------------------------
 * The one speaker normalisation that lives inside the front end.  A warped front end holds, beside the unwarped filterbank, one
 * filterbank per warp factor alpha[a]; a speaker's warp is found by scoring its utterances under every warp along an alignment
 * (sr_vtln_costs_corpus, sr_vtln_choose), and a corpus is then made with a warp per utterance (sr_corpus_from_audio_warped).
 *
 * The warp has one break point and is piecewise linear.  For a warp factor alpha > 0 and break_frac in (0, 1):
 *   f0 = break_frac * f_high * min(1, 1 / alpha)
 *   g_alpha(f) = alpha * f                                                             for f <= f0
 *              = alpha * f0 + (f_high - alpha * f0) / (f_high - f0) * (f - f0)           for f >  f0
 * so g is continuous and monotone and g(f_high) = f_high.  alpha == 1.0 is the identity by definition: g(f) = f exactly, with no
 * arithmetic.  The filters' edges stay where the MFCC stage's definition puts them; bin k has, in filter m of warp alpha, the weight of
 * the unwarped triangle evaluated at g_alpha(f_k): max(0, min((g(f_k) - l) / (c - l), (r - g(f_k)) / (r - c))), computed in double and
 * stored as float like the unwarped weights.  Window, twiddles and DCT are shared by all warps, so the filterbank of alpha == 1.0 is
 * the unwarped front end's, bit for bit, and so are its cepstra.  (tests/vtln_reference.py restates all of this in float64.)
 * NO JACOBIAN TERM is applied anywhere: the costs below are plain emission costs.  A caller who wants a per-warp penalty adds
 * frames[s] * penalty[a] to the returned costs before choosing.
 *
 * sr_frontend_create_warped   a front end with n_warps filterbanks.  It checks everything sr_frontend_create checks, and: SR_EINVAL for
 *     mfcc == NULL, vtln == NULL, n_warps == 0, alpha == NULL, an alpha that is not finite and positive, break_frac outside (0, 1), and --
 *     naming warp and filter -- a filter of any warp without a bin of positive weight; SR_ELIMIT for n_warps > 32 or n_warps * n_mel >
 *     1024 (the logarithms of one frame under every warp are kept in 4 KiB of a wave's LDS; 13 warps of 40 filters are 520).  The
 *     unwarped filterbank is always built, whether or not 1.0 is among the alphas, and every entry point that takes a front end --
 *     sr_corpus_from_audio, sr_mfcc_corpus, sr_corpus_from_cepstra, sr_stream_set_frontend and its bigram twin -- accepts a warped one
 *     and behaves exactly as on an unwarped front end of the same parameters.  Streaming has no per-stream warp.
 * sr_frontend_warps           *n_warps: the warps of the front end, 0 for an unwarped one.
 * sr_corpus_from_audio_warped sr_corpus_from_audio with utterance u through the filters of warp utt_warp[u].  An index >= n_warps, a NULL
 *     utt_warp and an unwarped front end are SR_EINVAL, before any launch.  The result is a corpus like sr_corpus_from_audio's, and an
 *     utterance's rows depend on its samples and its warp alone, not on the batch.
 * sr_vtln_costs_corpus        the warp search.  states [frames] is an alignment of the UNWARPED corpus: one state per frame, the frame
 *     offsets being the front end's own (sr_frontend_frames; sr_corpus_from_audio's out_frame_off).  For every warp a, every utterance
 *     goes through warp a's filters and the post-processing stage, and row t is scored against states[t]: MixtureModel::score(row,
 *     states[t]), the value sr_path_scores_corpus returns on sr_corpus_from_audio_warped's corpus with every utterance on warp a, bit
 *     for bit.  The order of summation is the definition: an utterance's sum is the sequential FP64 sum of its frames' scores in
 *     ascending order; out_cost[s * n_warps + a] is the sequential FP64 sum of the sums of speaker s's utterances (utt_speaker[u] == s,
 *     utterances without frames included) in ascending index.  The first addend of each sum is taken as is and an empty sum is +0.
 *     No atomics: two calls give the same bits, and the bits do not depend on how the warps are processed in chunks.  A chunk is as
 *     many warps as keep the buffers that grow with warps x frames -- cepstra, rows, the alignment's copies, scores -- within a
 *     budget, a quarter of the score workspace (SRGPU_VTLN_KB, read when the model is made, sets it in KiB), and at least one warp;
 *     the samples, the offsets and the n_warps x n_utts utterance sums are not counted, so the budget bounds the chunks, not the
 *     call's whole device memory.  sr_vtln_chunks tells how many chunks a call on that many frames and utterances takes.
 *     SRGPU_VTLN_TIMING, read with the budget, makes every call print one line to stderr, `vtln_timing chunks N mfcc_warps_ms ..
 *     post_ms .. score_ms .. reduce_ms ..`, its stages' HIP-event times for tools/vtln_time.py (five event records per chunk more).
 *     out_frames[s]: the speaker's frames.  Costs are costs: smaller is better.  A frame's power spectrum is computed once for all
 *     warps (mfcc_warps_kernel).  Checked before any launch (SR_EINVAL): an unwarped front end, the offsets, a
 *     state >= n_states, a speaker >= n_speakers, NULL arguments; SR_ELIMIT as for sr_corpus_from_audio.
 * sr_vtln_choose              host only.  out_warp[s]: the first warp of smallest cost of speaker s -- or fallback_warp where the
 *     speaker has fewer than min_frames frames, where its smallest cost is not finite, or where any of its costs is NaN.  SR_EINVAL
 *     for n_warps == 0, fallback_warp >= n_warps, a NULL argument with n_speakers > 0.
 * A refused call leaves *out NULL and the host outputs untouched. */
typedef struct {
  uint32_t n_warps;
  const double* alpha;           /* [n_warps] warp factors, each finite and > 0 */
  double break_frac;             /* in (0, 1): the break point as a fraction of f_high (0.875 is common) */
} sr_vtln_params;
SR_API int sr_frontend_create_warped(sr_model* m, const sr_mfcc_params* mfcc, const sr_vtln_params* vtln, const sr_feature_post_params* post,
                                     sr_frontend** out);
SR_API int sr_frontend_warps(const sr_frontend* fe, uint32_t* n_warps);
SR_API int sr_corpus_from_audio_warped(sr_frontend* fe, const int16_t* samples, const uint64_t* sample_off, uint32_t n_utts,
                                       const uint32_t* utt_warp /*[n_utts]*/, sr_corpus** out, uint64_t* out_frame_off /*[n_utts+1]*/);
SR_API int sr_vtln_costs_corpus(sr_frontend* fe, const int16_t* samples, const uint64_t* sample_off, uint32_t n_utts,
                                const uint16_t* states /*[frames]: an alignment*/, const uint32_t* utt_speaker /*[n_utts]*/,
                                uint32_t n_speakers, double* out_cost /*[n_speakers][n_warps]*/, uint64_t* out_frames /*[n_speakers]*/);
/* *out_chunks: the chunks of warps sr_vtln_costs_corpus takes for n_frames frames in n_utts utterances (host only; SR_EINVAL for an
 * unwarped front end or a NULL argument, SR_ELIMIT where the call itself would return it) */
SR_API int sr_vtln_chunks(const sr_frontend* fe, uint64_t n_frames, uint32_t n_utts, uint32_t* out_chunks);
SR_API int sr_vtln_choose(uint32_t n_speakers, uint32_t n_warps, const double* cost, const uint64_t* frames, uint64_t min_frames,
                          uint32_t fallback_warp, uint32_t* out_warp /*[n_speakers]*/);

/* ---- streaming from audio: PCM samples into a stream set, the front end on the device ------------------------------------------------
 * With a front end attached, a stream set takes an utterance's samples as they arrive, in pieces of any size, instead of finished
 * feature rows.  step = deriv_step.  An utterance fed as audio has received N samples so far and has S = sr_frontend_frames(N) static
 * frames.
 *   before the finish  frames 0 .. S - 1 - step have been searched (none while S <= step): row t needs the statics t - step .. t + step
 *                      and nothing else, and every clamp of the post-processing that involves T is inactive while static t + step exists;
 *   after the finish   all T = S frames have been searched, the last up to `step` rows with the clamped windows of the now-known T.
 * The rows.  With energy_max_norm == 0, row t is exactly row t of sr_corpus_from_audio on the whole utterance, bit for bit, for every
 * way of cutting the samples into pushes -- one sample at a time, pushes that complete no frame, and shift > window (the samples between
 * two frames are passed over, but the pre-emphasis still reads the one before a frame's first) included.  So the words and the
 * traceback are sr_recognize_corpus' (sr_recognize_bigram_corpus') on that corpus.
 * The energy maximum, with energy_max_norm != 0.  Only this needs the whole utterance; it has a causal replacement.  Component 0 of
 * row t is the value the front end produces without the maximum (the static, mean / stddev applied) minus m(t): the maximum of that
 * same value over frames 0 .. min(t + step, T - 1), kept the way the host loop keeps it -- replaced on `<` alone, so the first frame
 * that reaches it wins and -0 is told from +0.  One float subtraction; it does not depend on how the samples were cut.  It equals the
 * batch's bits whenever the utterance's maximum lies in its first step + 1 frames.  Otherwise it is NOT the batch's value: rows before
 * frame (argmax - step) carry a smaller maximum than sr_corpus_from_audio subtracts.
 *
 * sr_stream_set_frontend   attaches `fe` (NULL detaches) -- only while no id is open; the front end must belong to the stream set's model
 *                          (with a projection attached: see sr_stream_set_projection) and have an MFCC stage; it is destroyed after the stream set.  Device memory: max_streams x (2 step n_static + 1)
 *                          floats, the last 2 step statics and the running maximum of every slot.
 * sr_stream_push_audio     n utterances, ids[n], each at most once; their new samples back to back, entry i's at samples[sample_off[i] ..
 *                          sample_off[i + 1]), sample_off[0] == 0, an empty range allowed.  The rows that became ready are searched
 *                          before it returns (one launch of stream_frontend_kernel, then the scoring and the search of sr_stream_push; a
 *                          push that readies no row launches neither of those).  out_feats (may be NULL): those rows, [rows x dim], entry
 *                          i's at out_frame_off[i] .. out_frame_off[i + 1] (out_frame_off [n + 1], may be NULL); cap_rows: the rows
 *                          out_feats holds -- fewer than the push readies is SR_EINVAL, with the count in the error text and in
 *                          out_frame_off[n] (it is sum_i of max(S_i' - step, 0) - max(S_i - step, 0), computable on the host).
 * sr_stream_finish_audio   emits the last rows of the n utterances; afterwards the ids take no more audio.  sr_stream_partial, _stable
 *                          and _end work as before on what has been searched (_partial's *frames is max(S - step, 0) before the finish).
 * An id is an audio id from its first sr_stream_push_audio (or _finish_audio) and a feature id from its first sr_stream_push: the other
 * kind of push on it is SR_EINVAL.  sr_stream_end on an audio id that was not finished is SR_EINVAL and leaves the id open.  max_frames
 * bounds T (SR_ELIMIT).  Every check comes before any launch; a refused call changes no utterance, its carried samples included.
 * Other errors (SR_EINVAL): no front end attached, an unknown, ended or finished id, an id twice in one call, sample_off[0] != 0 or
 * falling.  The host keeps fewer than `window` samples (and the one before them) per utterance between pushes and uploads them in
 * front of the new ones.  Threading as for the stream set.  Stream sets without a front end, and ids fed with rows, behave as before. */
SR_API int sr_stream_set_frontend(sr_stream* s, sr_frontend* fe);
SR_API int sr_stream_push_audio(sr_stream* s, uint32_t n, const uint32_t* ids, const int16_t* samples, const uint64_t* sample_off,
                                float* out_feats /*optional*/, uint64_t cap_rows, uint64_t* out_frame_off /*[n+1], optional*/);
SR_API int sr_stream_finish_audio(sr_stream* s, uint32_t n, const uint32_t* ids, float* out_feats /*optional*/, uint64_t cap_rows,
                                  uint64_t* out_frame_off /*[n+1], optional*/);
/* the same for the bigram stream set (declared below) */
struct sr_bigram_stream;
SR_API int sr_bigram_stream_set_frontend(struct sr_bigram_stream* s, sr_frontend* fe);
SR_API int sr_bigram_stream_push_audio(struct sr_bigram_stream* s, uint32_t n, const uint32_t* ids, const int16_t* samples,
                                       const uint64_t* sample_off, float* out_feats /*optional*/, uint64_t cap_rows,
                                       uint64_t* out_frame_off /*[n+1], optional*/);
SR_API int sr_bigram_stream_finish_audio(struct sr_bigram_stream* s, uint32_t n, const uint32_t* ids, float* out_feats /*optional*/,
                                         uint64_t cap_rows, uint64_t* out_frame_off /*[n+1], optional*/);
/* ---- streaming: splice, projection and per-utterance transform on the device ------------------------------------------
 * A stream set of a model of dimension p may carry a pipeline of two optional stages, applied on the device (stream_pipeline_kernel,
 * one launch per push, one workgroup per pushed utterance) to every row before it is scored.
 *   1. projection  set for the whole stream set: in_dim = D, context = c, M [p x (E + 1)] doubles, E = (2c + 1) D.  Row t of an utterance
 *                  of T input rows is sr_corpus_splice_transform's row, bit for bit:
 *                    z_t[(o + c) D + j] = (double) x[min(max(t + o, 0), T - 1)][j], o = -c .. c;
 *                    acc = M[i][E];  acc = acc + M[i][n] * z_t[n] for n ascending, FP64, no fused multiply-add;  the row is (float) acc.
 *   2. transform   set per utterance: W [p x (p + 1)] = [A b], applied to the float row stage 1 produced (to the pushed row without a
 *                  projection); sr_corpus_transform's row, bit for bit:
 *                    acc = b_i;  acc = acc + A_ij * (double) y_j for j ascending, no FMA;  the row is (float) acc.
 * The intermediate row is rounded to float between the stages, as it is when the batch calls run one after the other.  So, for every
 * way of cutting an utterance into pushes, the rows searched are bit-identical to sr_corpus_upload (or sr_corpus_from_audio without
 * the energy maximum), then sr_corpus_splice_transform, then sr_corpus_transform on the whole utterance, and the words and the
 * traceback are sr_recognize_corpus' (sr_recognize_bigram_corpus') on that corpus.
 * Delay.  An utterance has received R input rows so far.
 *   before the finish  rows 0 .. R - 1 - c have been searched (none while R <= c): row t needs the input rows t - c .. t + c; the left clamp
 *                      is known at once, the right clamp involves T;
 *   after the finish   all T rows have been searched, the last up to c of them with the clamp of the now-known T (a one-row utterance
 *                      splices 2c + 1 copies of its row).
 * With c == 0, or without a projection, there is no delay and nothing to finish.  For audio ids R is the number of rows the front end
 * has readied: the total delay is deriv_step + c frames, and sr_stream_finish_audio flushes both stages.
 *
 * sr_stream_set_projection  only while no id is open; M == NULL detaches.  SR_ELIMIT for E > 512; SR_EINVAL for in_dim == 0, for an attached
 *                           front end whose model's dimension is not in_dim, and for detaching with an attached front end that does not
 *                           belong to the stream set's model.  With a projection attached sr_stream_set_frontend accepts a front end of
 *                           any model of dimension in_dim on the stream set's device (such a front end and its model are destroyed after
 *                           the stream set); without one it behaves as before.  Device memory: M, max_streams x 2c x in_dim floats of
 *                           history (the last 2c input rows of every slot) and one more per-push buffer, of input rows.
 * sr_stream_set_transform   between sr_stream_begin and the id's first push of either kind, else SR_EINVAL.  W == NULL clears it; a fresh
 *                           id has none.  SR_ELIMIT for a model dimension above 63 (sr_corpus_transform's limit).  Device memory:
 *                           max_streams x p x (p + 1) doubles, allocated by the first call.
 * sr_stream_push_rows       the general row push.  feats has in_dim columns with a projection attached, else p; ids, frame_off as
 *                           sr_stream_push.  finish != 0: every named id is finished after its rows and its last c rows are emitted; a
 *                           finish without new rows is allowed (frame_off, feats may then be NULL).  A finished id takes no more rows
 *                           (SR_EINVAL).  out_feats, cap_rows, out_frame_off as in sr_stream_push_audio: the rows this call searched,
 *                           in the model's space; too small a cap_rows is SR_EINVAL with the count in out_frame_off[n], and nothing
 *                           changes.  A push that readies no row launches no scoring and no search.
 *                           sr_stream_push(s, n, ids, feats, frame_off) is sr_stream_push_rows(.., 0, NULL, 0, NULL).
 * sr_stream_end on a row id that has received rows not yet searched is SR_EINVAL and leaves the id open (possible only with context
 * > 0).  sr_stream_partial's *frames, sr_stream_stable and the traceback refer to the rows searched; max_frames bounds the rows
 * received (SR_ELIMIT).  Every check comes before any launch; a call refused by a check changes no utterance, its history included
 * (a call that fails after its launches -- a HIP error, SR_EINTERNAL -- may leave a slot's device history ahead of the host's count: end
 * such an utterance).  A VTLN warp per utterance is not a stage of this pipeline but a choice inside the front end: sr_stream_set_warp
 * below. */
SR_API int sr_stream_set_projection(sr_stream* s, uint32_t in_dim, uint32_t context, const double* M);
SR_API int sr_stream_set_transform(sr_stream* s, uint32_t id, const double* W);
SR_API int sr_stream_push_rows(sr_stream* s, uint32_t n, const uint32_t* ids, const float* feats, const uint64_t* frame_off, int finish,
                               float* out_feats /*optional*/, uint64_t cap_rows, uint64_t* out_frame_off /*[n+1], optional*/);
SR_API int sr_bigram_stream_set_projection(struct sr_bigram_stream* s, uint32_t in_dim, uint32_t context, const double* M);
SR_API int sr_bigram_stream_set_transform(struct sr_bigram_stream* s, uint32_t id, const double* W);
SR_API int sr_bigram_stream_push_rows(struct sr_bigram_stream* s, uint32_t n, const uint32_t* ids, const float* feats,
                                      const uint64_t* frame_off, int finish, float* out_feats /*optional*/, uint64_t cap_rows,
                                      uint64_t* out_frame_off /*[n+1], optional*/);
/* ---- streaming from audio: a VTLN warp per utterance -------------------------------------------------------------------------------
 * With a warped front end attached (sr_frontend_create_warped, n_warps = sr_frontend_warps > 0), every audio id of a stream set may
 * carry one of the front end's warps.  stream_frontend_kernel then builds that id's statics with the filters of its warp, as
 * mfcc_kernel does for an utterance of sr_corpus_from_audio_warped; one launch still serves all the ids of a push, whatever their
 * warps.  An id without a warp uses the unwarped filters, as every id did before.
 * The rows.  With energy_max_norm == 0, row t of an id with warp w is exactly row t of sr_corpus_from_audio_warped on the whole
 * utterance with utt_warp = w, bit for bit, for every way of cutting the samples into pushes and for every mix of warps among the ids
 * of one push.  With a projection and / or a transform attached those rows are the pipeline's input, and the rows searched are the
 * batch chain's: sr_corpus_from_audio_warped, sr_corpus_splice_transform, sr_corpus_transform.  With the energy maximum on, component 0
 * is the causal maximum defined above, applied to the warped no-maximum rows.  The words and the traceback are the batch search's on
 * that corpus.
 *
 * sr_stream_set_warp   between sr_stream_begin and the id's first push of either kind, as sr_stream_set_transform; later it is SR_EINVAL.
 *                      SR_STREAM_NO_WARP clears the warp; a fresh id has none, and a slot reused by a new id does not inherit the warp of
 *                      the utterance before it.  SR_EINVAL: no front end attached, a front end without warps, warp >= n_warps other
 *                      than SR_STREAM_NO_WARP, an unknown or ended id.  Host state only: no launch, no device memory.
 * An id that carries a warp is an audio id: sr_stream_push / sr_stream_push_rows on it is SR_EINVAL and changes nothing, the warp
 * included.  Every check comes before any launch; a refused call changes nothing.  sr_stream_set_frontend is allowed only while no id
 * is open, and a warp lives from its id's begin to its end, so no warp outlives the front end it was checked against.  Not offered:
 * changing a warp after the first push, a Jacobian term for the warp, a warp search inside the stream set (INTEGRATION.md 5d composes
 * one from existing calls), warps for ids fed with rows. */
#define SR_STREAM_NO_WARP 0xFFFFFFFFu
SR_API int sr_stream_set_warp(sr_stream* s, uint32_t id, uint32_t warp);
SR_API int sr_bigram_stream_set_warp(struct sr_bigram_stream* s, uint32_t id, uint32_t warp);
/* the features of any resident corpus -- uploaded, transformed, projected or a front end's -- back to the host, out [frames x dim of the
 * corpus's model]; an asynchronous upload is waited for first */
SR_API int sr_corpus_download(sr_corpus* c, float* out);

/* ---- word posteriors and confidences: forward-backward over the recognition network --------------------------------
 * The network sr_recognize_corpus searches (Recognizer.cpp:103-232: the start hypothesis at word 0 position 0, in-word 0-1-2 jumps
 * with the penalty keyed on the DESTINATION state, every word end entering every word at position 0 or 1 with the word penalty --
 * 0 for silence -- and the emission of the word's FIRST state in both cases), with every path summed instead of only the best one
 * kept, no beam (am_threshold is ignored) and every cost multiplied by scale = kappa > 0:
 *   F_u = -(1/kappa) log sum over the paths that end in a word end at frame T_u - 1 of exp(-kappa cost);  F_u <= tb_score[T_u] of
 *   sr_recognize_corpus for any beam, nondecreasing in kappa, tending to the unpruned Viterbi cost.  T_u = 0: F_u = +inf.
 *   p_t(w | X) = the posterior mass of word w's positions at frame t (silence a word like any other; sum over w = 1).
 * p supplies word_penalty and gmm_kernel; p->flags must be 0.  Lexica of at most 8192 positions (SR_ELIMIT).  Workspace: 8 bytes per
 * (frame, position) for the utterances processed together, at most SRGPU_FB_MB MiB (default 1024); an utterance that alone needs
 * more: SR_ELIMIT.  SR_EINVAL for scale not finite or not > 0, posterior_floor negative or NaN, max_items outside 1 .. 65535 with
 * item outputs, a partial set of item outputs, a lexicon of another model.  FP64 log space without atomics: two identical calls
 * return identical bits; +inf penalties and unreachable positions stay +inf, never NaN. */

/* out_cost[n_utts] = F_u (required).  Items all or none: out_count[total_frames], out_word[total_frames * max_items],
 * out_weight[total_frames * max_items] -- per frame the words with p > 0 and p >= posterior_floor, largest first (ties: smaller
 * word id first), at most max_items, not renormalised; entries past out_count are 0. */
SR_API int sr_word_posteriors_corpus(sr_model* m, sr_corpus* c, sr_lexicon* l, const sr_search_params* p, double scale,
                                     double posterior_floor, uint32_t max_items, double* out_cost, uint16_t* out_count,
                                     uint32_t* out_word, double* out_weight);
/* Words and out_word_off exactly as sr_recognize_corpus with the same p (beam included).  For recognised word i, out_first[i] ..
 * out_last[i] are its frames within the utterance (from the traceback: bkp .. t - 1), and out_conf[i] = max over those frames of
 * p_t(word | X), computed without a beam (Wessel et al. 2001's C_max).  out_words, out_conf, out_first, out_last: capacity
 * total_frames like sr_recognize_corpus' out_words. */
SR_API int sr_recognize_confidence_corpus(sr_model* m, sr_corpus* c, sr_lexicon* l, const sr_search_params* p, double scale,
                                          uint32_t* out_words, uint64_t* out_word_off, double* out_conf, uint32_t* out_first,
                                          uint32_t* out_last);

/* ---- MMI training: mixture occupancies, numerator / denominator statistics, extended Baum-Welch ---------------------------------
 * Both networks are the one above (scale, penalties, start hypothesis, p as sr_word_posteriors_corpus).
 *   FREE network (denominator): every path, F_den = the F_u of sr_word_posteriors_corpus.
 *   TRANSCRIPT-CONSTRAINED network (numerator): transcript of utterance u = trans[trans_off[u] .. trans_off[u + 1]) (lexicon word
 *   ids, silence not listed, possibly empty); the subset of the free network's paths whose word string with silence removed -- what
 *   sr_recognize_corpus would print for the path -- is the transcript: the chain of segments sil_0 w_1 sil_1 .. w_n sil_n, a word end
 *   entering the next word segment, the silence segment after it and, from a silence segment, that segment again.  It needs the
 *   lexicon's word 0 to be its silence word.  F_num is the same formula over the subset, so F_num >= F_den up to rounding; a
 *   transcript without a path (too few frames) has F_num = +inf.
 *   occ_t(k) = the posterior probability that frame t's emission is mixture k's = dF / d e(t, k); sum over k = 1.  An entry into
 *   position 1 of a word emits the word's FIRST state (the reference's quirk) and counts for that state.
 * Limits as sr_word_posteriors_corpus; a chain of more than 8192 positions: SR_ELIMIT; its trellis takes 8 bytes per (frame, chain
 * position) of the SRGPU_FB_MB workspace.  SR_EINVAL also for trans without trans_off or the reverse, trans_off[0] != 0 or
 * decreasing, a word id >= n_words or equal to the silence word, word 0 not the silence word with a transcript.  No atomics: two
 * identical calls return identical bits. */

/* out_cost[n_utts] = F_u (required) of the free network (trans and trans_off NULL) or the constrained one (both given).  Items in
 * AlignmentItem shape like sr_state_posteriors_corpus, all or none: per frame the mixtures with occ > 0 and occ >=
 * posterior_floor, largest first (ties: smaller id first), at most max_items (1 .. 65535), not renormalised. */
SR_API int sr_net_occupancies_corpus(sr_model* m, sr_corpus* c, sr_lexicon* l, const sr_search_params* p, double scale,
                                     double posterior_floor, uint32_t max_items, const uint32_t* trans, const uint64_t* trans_off,
                                     double* out_cost, uint16_t* out_count, uint16_t* out_state, double* out_weight);

/* One MMI E-step: both passes, each side's occupancies accumulated as sr_baum_welch_corpus accumulates its posteriors (max_approx:
 * the arg-min density, else the soft memberships), ONLY over utterances with finite F_num (the others contribute to neither side).
 * out_num_cost[n_utts] = F_num, out_den_cost[n_utts] = F_den.  All outputs required, the statistics shaped as sr_accumulate_corpus'.
 * Statistics of corpus shards add up like sr_accumulate_corpus'; the var_acc seed of 1e-4 is present once per call and side. */
SR_API int sr_mmi_statistics_corpus(sr_model* m, sr_corpus* c, sr_lexicon* l, const sr_search_params* p, double scale,
                                    double posterior_floor, int max_approx, const uint32_t* trans, const uint64_t* trans_off,
                                    double* out_num_cost, double* out_den_cost, double* num_mean_acc, double* num_mean_w,
                                    double* num_var_acc, double* num_var_w, double* den_mean_acc, double* den_mean_w,
                                    double* den_var_acc, double* den_var_w);

/* Extended Baum-Welch update of the means and variances of m from one call's (or the summed shards') statistics -> new device
 * model of m's topology.  Per density, with counts gn, gd (the mean_w), sums xn, xd, second-order sums sn, sd (the 1e-4 seed
 * subtracted), old mu and var = 1 / inv_var:  if tau > 0 and gn > 0 the numerator's three are scaled by (gn + tau) / gn
 * (I-smoothing);  D = max(E gd, 2 max(gd - gn, 0) + 1e-10), doubled (at most 64 times) until every dimension's new variance is
 * >= var_floor, what still is not is set to var_floor;  mu' = (xn - xd + D mu) / (gn - gd + D),
 * var' = (sn - sd + D (var + mu^2)) / (gn - gd + D) - mu'^2.  A density with gn = gd = 0 keeps mean and variance.  The mixture
 * weights are m's (no weight update); norm is recomputed from the new variances.  m must be untied -- every density with its own
 * mean and variance row -- else SR_EINVAL; SR_EINVAL also for E <= 0, tau < 0, var_floor <= 0 or any of them not finite. */
SR_API int sr_model_create_from_mmi_statistics(sr_model* m, const double* num_mean_acc, const double* num_mean_w,
                                               const double* num_var_acc, const double* num_var_w, const double* den_mean_acc,
                                               const double* den_mean_w, const double* den_var_acc, const double* den_var_w,
                                               double E, double tau, double var_floor, sr_model** out);

/* ---- sMBR training: expected frame accuracy over the recognition network -----------------------------------------------------------
 * The FREE network above (scale kappa, penalties, start hypothesis and p as sr_word_posteriors_corpus: every path,
 * P(pi) proportional to exp(-kappa cost(pi)), no beam, p->flags == 0).
 *   ref_states[total_frames] = the reference mixture of every frame (for example the output of sr_align_corpus); a value >= the
 *   model's state count means the frame scores for no mixture.
 *   A(pi) = sum over t of [k_t(pi) == ref_states[t]], k_t(pi) = the mixture whose emission the path pays at frame t.  An entry into
 *   position 1 of a word emits the word's FIRST state (the reference's quirk) and is scored as that state.
 *   out_acc[u] = Abar_u = sum over pi of P(pi) A(pi), 0 <= Abar_u <= T_u.  T_u = 0 or F_u = +inf: Abar_u = 0 and no items.
 *   gamma_t(k) = occ_t(k) (c_t(k) - Abar_u) = -(1/kappa) d Abar_u / d e(t, k), with occ_t(k) the occupancy of
 *   sr_net_occupancies_corpus and c_t(k) the expected accuracy of the paths whose frame t emits k; sum over k of gamma_t(k) = 0.
 * Lexica of at most 5108 positions (what sr_smbr_max_positions reports) (SR_ELIMIT).  Workspace: 16 bytes per (frame, position) for the
 * utterances processed together, at most SRGPU_FB_MB MiB; an utterance that alone needs more: SR_ELIMIT.  SR_EINVAL as
 * sr_net_occupancies_corpus, and for a NULL ref_states.  Every check precedes the first launch.  No atomics: two identical calls
 * return identical bits. */
SR_API int sr_smbr_max_positions(uint32_t* out);

/* out_cost[n_utts] = F_u and out_acc[n_utts] = Abar_u (both required).  Items all or none: per frame the mixtures with gamma != 0
 * and |gamma| >= posterior_floor, largest |gamma| first (ties: smaller id first), at most max_items (1 .. 65535); out_weight is
 * signed; entries past out_count are 0. */
SR_API int sr_net_accuracies_corpus(sr_model* m, sr_corpus* c, sr_lexicon* l, const sr_search_params* p, double scale,
                                    double posterior_floor, uint32_t max_items, const uint16_t* ref_states, double* out_cost,
                                    double* out_acc, uint16_t* out_count, uint16_t* out_state, double* out_weight);

/* One sMBR E-step.  gamma is split by sign: the items (t, k, gamma) with gamma > 0 and gamma >= posterior_floor go to the numerator,
 * the items (t, k, -gamma) with -gamma > 0 and -gamma >= posterior_floor to the denominator, each spread over the mixture's
 * densities exactly as sr_mmi_statistics_corpus spreads an occupancy (max_approx: the arg-min density, else the soft memberships
 * with their < 1e-8 drop), with the accumulators, seeds and summation order of sr_baum_welch_corpus.  All outputs required; the eight
 * arrays are shaped so that sr_model_create_from_mmi_statistics takes them unchanged.  Statistics of corpus shards add up like
 * sr_mmi_statistics_corpus' (the var_acc seed of 1e-4 once per call and side). */
SR_API int sr_smbr_statistics_corpus(sr_model* m, sr_corpus* c, sr_lexicon* l, const sr_search_params* p, double scale,
                                     double posterior_floor, int max_approx, const uint16_t* ref_states, double* out_cost,
                                     double* out_acc, double* num_mean_acc, double* num_mean_w, double* num_var_acc,
                                     double* num_var_w, double* den_mean_acc, double* den_mean_w, double* den_var_acc,
                                     double* den_var_w);

/* ---- word lattices and N-best lists over the recognition network --------------------------------------------------------
 * The same network in the MIN semiring, without a beam (am_threshold is ignored) and with the decoder's order of additions, so
 * that every number below is a sum the decoder itself would form.  For an utterance of T frames:
 *   A_t(s)   the cheapest path from the start hypothesis to lexicon position s at frame t; E_t = min of A_t over the word ends
 *            (= tb_score[t + 1] of sr_recognize_corpus at an infinite beam), E_{-1} = 0;
 *   Bend_t   the cheapest continuation after a word end at frame t to a word end at frame T - 1 (Bend_{T-1} = 0).
 * An ARC per (word w, frame t) whose last position is reachable at t: word = w, last = t, first = the frame at which the cheapest
 * path to (w, t) entered w (ties resolved as the decoder resolves them), fwd = A_t(end of w), bwd = Bend_t, cost = fwd -
 * E_{first-1} (penalties and emissions of frames first .. last).  fwd + bwd is the cost of the cheapest complete path on which w
 * ends at t.  The LATTICE of an utterance holds the arcs with fwd + bwd <= E_{T-1} + lattice_beam, ordered by last, then word
 * (+inf: every arc on some complete path).  Silence is a word like any other.  A lattice path is a chain of arcs with first_0 = 0,
 * first_{k+1} = last_k + 1, last_K = T - 1, its cost the sum of the arcs' cost from left to right; the cheapest one spells
 * sr_recognize_corpus' words (infinite beam) and costs E_{T-1} up to the rounding of the arcs' cost and of their sum.  exp(-kappa (fwd + bwd - best)) is an arc's posterior-style score.
 * APPROXIMATION: there is one arc per (word, end frame), carrying the best start only.  The paths through the lattice are a subset
 * of the network's: the first entry of an N-best list is exact, the k-th is an upper bound of the network's k-th best cost.
 * Limits: lexica of at most 8176 positions (SR_ELIMIT; the forward keeps 20 bytes per position in the 160 KiB LDS), utterances
 * of at most 65535 frames.  Workspace: 10 bytes per (frame, word) + 32 per frame for the utterances processed together, at most
 * SRGPU_FB_MB MiB (default 1024); an utterance that alone needs more: SR_ELIMIT.  min and + in FP64 without atomics: two
 * identical calls return identical bits; +inf penalties and unreachable positions stay +inf, never NaN. */

/* Lattice of every utterance.  p supplies word_penalty and gmm_kernel; p->flags must be 0; am_threshold is ignored.
 * out_arc_off[n_utts + 1] and out_best[n_utts] (= E_{T-1}; +inf for T = 0, which has no arcs) are always written; utterance u owns
 * arcs out_arc_off[u] .. out_arc_off[u + 1], first and last counted within the utterance.  The arc arrays (all six or none) have
 * capacity cap arcs.  All NULL: the sizing call, SR_OK with the counts in out_arc_off.  Given but the total exceeds cap: nothing
 * is written to them, out_arc_off still holds the counts needed, SR_EINVAL.  SR_EINVAL also for lattice_beam negative or NaN,
 * p->flags != 0, a lexicon of another model, a partial set of arc arrays. */
SR_API int sr_word_lattice_corpus(sr_model* m, sr_corpus* c, sr_lexicon* l, const sr_search_params* p, double lattice_beam,
                                  uint64_t cap, uint64_t* out_arc_off, double* out_best, uint32_t* out_word, uint32_t* out_first,
                                  uint32_t* out_last, double* out_fwd, double* out_bwd, double* out_cost);
/* Host only, one utterance: the n_best cheapest DISTINCT word strings (silence removed, as sr_recognize_corpus) among the lattice
 * paths, cheapest first.  A string's cost is that of its cheapest path (the arcs' cost summed from left to right).  out_words has
 * capacity words_cap, hypothesis k owns out_words[out_off[k] .. out_off[k + 1]); out_off[n_best + 1], out_cost[n_best];
 * *out_count <= n_best of them exist (0 for n_frames = 0).  Arcs that no complete path uses are skipped.  Strings of equal cost
 * come in an order that is the same on every call.  SR_EINVAL: n_best = 0, arcs not in (last, word) order, first > last, last >=
 * n_frames, a cost that is NaN or -inf, words_cap too small (*out_count = 0). */
SR_API int sr_lattice_nbest(uint32_t n_frames, uint64_t n_arcs, const uint32_t* word, const uint32_t* first, const uint32_t* last,
                            const double* cost, uint32_t silence_word, uint32_t n_best, uint32_t* out_words, uint64_t words_cap,
                            uint64_t* out_off, double* out_cost, uint32_t* out_count);

/* ---- bigram-LM beam search over a linear lexicon ---------------------------------------------------------------
 * Replaces Teaching::LinearSearch (rwth-asr-0.5/src/Teaching/LinearSearch.cc: initialize :489-495, processFrame
 * :496-515, getResult :517-520) for a whole corpus.  Scores are float there (Teaching/Types.hh:17); the acoustic
 * score of mixture m at frame t is (float) of this library's FP64 score.
 *   word_off[W+1], mixtures[]: the linear lexicon (LinearSearch::buildLinearLexicon :477-483), mixture = emission state;
 *   lm[w*W + h] = -log p(w | h) (SearchInterface::getLanguageModelScore(w, h), SearchInterface.cc:77-81);
 *   tdp[8] = [isSilence][loop, forward, skip, exit] (SearchSpace::setTransitionScores :169-180).
 * PARITY UNPINNED: checked against the CPU restatement under oracle/ only (the toolkit cannot be built here). */
typedef struct sr_bigram sr_bigram;
typedef struct {
  float acoustic_pruning;   /* "acoustic-pruning" (:441-442); >= FLT_MAX: off */
  float lm_pruning;         /* "lm-pruning" (:444-445) */
  int gmm_kernel;
  uint32_t max_word_ends;   /* traceback book capacity per frame and utterance; 0 = W (cannot overflow) */
  int flags;                /* 0, SR_BIGRAM_DENSE_STATES or SR_BIGRAM_GLOBAL_STATES (both: SR_EINVAL) */
} sr_bigram_params;
/* Where the search keeps the state hypotheses (viterbi_bigram.hip); with flags = 0 the first that applies:
 *   1 "registers": every word has at most four states, at most 3072 words, one-state silence -- a word's states in one lane's registers;
 *   2 "lds":       the dense image of all positions (8 bytes each) beside the lists (~26 bytes per word) fits the 160 KiB LDS;
 *   3 "global":    every other lexicon -- the image in device memory, only the positions of the active words visited per frame.
 * SR_BIGRAM_DENSE_STATES forces layout 2 (SR_ELIMIT if the image does not fit), SR_BIGRAM_GLOBAL_STATES layout 3.  Same results;
 * for cross-checking the layouts. */
#define SR_BIGRAM_DENSE_STATES 1
#define SR_BIGRAM_GLOBAL_STATES 2
/* Limits: n_words <= 8192 (any lexicon within them is accepted); positions = the words' states plus n_words x the silence word's
 * states (the silence copies) < 2^31. */
SR_API int sr_bigram_create(sr_model* m, uint32_t n_words, const uint32_t* word_off, const uint16_t* mixtures,
                            uint32_t silence_word, const float* lm, const float tdp[8], sr_bigram** out);
SR_API int sr_bigram_destroy(sr_bigram* b);
/* The layout sr_recognize_bigram_corpus runs with flags = 0: "registers", "lds" or "global" (see above). */
SR_API int sr_bigram_describe(const sr_bigram* b, char* out, size_t cap);
/* The kernel sr_recognize_bigram_corpus runs with sr_bigram_params.flags = flags, as text: "registers R rows4 0bM" (R = 1..3 rows of
 * 1024 words a lane, M = the rows that carry a fourth state, in binary), "lds KW x KP" (words / positions a thread), "global KW entries
 * lds" or "global KW entries global" (the entry hypotheses in the LDS / in device memory too), "none" where SR_BIGRAM_DENSE_STATES
 * asks for an image the LDS cannot hold.  The text comes from the function the launch itself switches on. */
SR_API int sr_bigram_route(const sr_bigram* b, uint32_t flags, char* out, size_t cap);
/* out_word/out_score/out_time: capacity n_frames + n_utts (LinearSearch::getResult's traceback items, silence included);
 * out_off[n_utts+1]: items of utterance u are [out_off[u], out_off[u+1]).  SR_ELIMIT if a book overflowed.  The "global" layout
 * takes a workspace of 16 bytes per position (+ 16 per word above 4 720 words) for each of at most 2 workgroups per CU, bounded by
 * a quarter of the free device memory and independent of the corpus size (SR_EHIP if even one does not fit).  With the environment
 * variable SRGPU_BIGRAM_STATS set, that layout reports the mean positions it visited per frame on stderr. */
SR_API int sr_recognize_bigram_corpus(sr_model* m, sr_corpus* c, sr_bigram* b, const sr_bigram_params* p,
                                      uint32_t* out_word, float* out_score, uint32_t* out_time, uint64_t* out_off);

/* ---- word posteriors and confidences for the bigram search: forward-backward over ITS network ------------------------------------
 * The network sr_recognize_bigram_corpus searches, with every path summed instead of the best kept, no acoustic and no LM beam, every
 * cost multiplied by scale = kappa > 0, in FP64 (lm and tdp widened from float; emission costs are the library's FP64 scores):
 *   slots 0 .. W-1 are the words, slot h + W the silence copy entered after word h != silence (the silence word's states, the silence
 *   penalties tdp[1]).  Before frame 1 there is one word end: the silence word, cost 0.  A word end of slot x has history x (a word),
 *   h (the copy h + W) or silence (the silence word); the cost of a history is the log-sum of its word ends -- the decoder's merge
 *   WITHOUT the positional cut of mergeSilenceToBigramNodes: every history is kept.  Word w != silence is entered from every history h
 *   at hist_h + lm[w * W + h] (NaN and +inf: a forbidden transition), the copy h + W from the word end of word h alone and the silence
 *   word from its own word end, both at no LM cost.  An entry moves to the first state at no penalty or to the second at the skip
 *   penalty; a state moves to itself and the next two at tdp[isSilence][0..2]; the destination's mixture is emitted; a word end is the
 *   last state plus tdp[isSilence][3].
 *   F_u = -(1/kappa) log sum over the word ends after frame T_u of exp(-kappa cost) <= the score of the decoder's last item (up to its
 *   float rounding);  T_u = 0: F_u = 0 and no frames.
 *   p_t(w | X) = the posterior mass of word w's positions at frame t; for w = silence the silence word and all copies.  Sum over w = 1.
 * Against the decoder: its merge keeps one hypothesis per history, so besides the cut it does not enter the copy h + W from word h's
 * end at a frame where the copy's own end is the better of the two; this network does.  The decoder searches a subset of these paths.
 * The word entry is evaluated in the linear domain as an FP64 matrix product with exp(-kappa lm).  Limits of that: SR_ELIMIT for a
 * finite score with -kappa lm > 700, SR_EINVAL for a score of -inf; an LM score whose exp underflows counts as forbidden, and word w
 * is entered at a frame only if some history h has kappa lm[w * W + h] + (hist_h - the frame's best history) below about 708 -- a
 * word all of whose terms underflow is not entered at that frame, where the log-space network would enter it at that cost.
 * Memory: the table and its transpose (16 bytes per LM entry, W padded to a multiple of 64: 116 MB at 2 667 words, 1 GiB at 8 192) are
 * built on the device once per (sr_bigram, kappa), kept on the sr_bigram handle and NOT counted in SRGPU_FB_MB.  Counted in it, for
 * the utterances processed together: 8 bytes per (frame, position) plus 24 W + 16 positions bytes per utterance; beside it 8 W bytes
 * per frame of the group for the word posteriors.  An utterance that alone exceeds SRGPU_FB_MB: SR_ELIMIT.  Like the search itself,
 * the calls use workspace of the sr_bigram and the corpus handle: one call at a time per handle.  Other errors as
 * sr_word_posteriors_corpus.  No atomics and a fixed summation order: two identical calls return identical bits. */

/* Outputs exactly as sr_word_posteriors_corpus: out_cost[n_utts] = F_u (required); items all or none. */
SR_API int sr_bigram_word_posteriors_corpus(sr_model* m, sr_corpus* c, sr_bigram* b, int gmm_kernel, double scale,
                                            double posterior_floor, uint32_t max_items, double* out_cost, uint16_t* out_count,
                                            uint32_t* out_word, double* out_weight);
/* Items bit for bit as sr_recognize_bigram_corpus with the same p (beams and layout flags included), and out_conf[i] = the maximum of
 * p_t(word_i | X) over item i's 0-based frames time_{i-1} .. time_i - 1 (time_{-1} = 0), computed without a beam.  Silence items get a
 * confidence like any other.  out_conf: capacity n_frames + n_utts like the items. */
SR_API int sr_recognize_bigram_confidence_corpus(sr_model* m, sr_corpus* c, sr_bigram* b, const sr_bigram_params* p, double scale,
                                                 uint32_t* out_word, float* out_score, uint32_t* out_time, uint64_t* out_off,
                                                 double* out_conf);

/* ---- MMI training against the bigram search: occupancies and numerator / denominator statistics over ITS network -----------------
 * Both networks are the one of the block above (slots, start, every history kept, no beams, scale = kappa in FP64).
 *   FREE network (denominator): every path; F_den is bit for bit the F_u of sr_bigram_word_posteriors_corpus (the same forward pass and
 *   linear-domain word entry, so the same limits: -kappa lm > 700 SR_ELIMIT, a score of -inf SR_EINVAL, the underflow rule).
 *   TRANSCRIPT-CONSTRAINED network (numerator): transcript of utterance u = trans[trans_off[u] .. trans_off[u + 1]) (word ids, silence
 *   not listed, possibly empty); the subset of the free network's paths whose sequence of non-silence word ENTRIES is the transcript:
 *   the chain of segments S w_1 c_1 .. w_n c_n.  S, the silence word, is entered from the start's word end before frame 0 and from its
 *   own word end afterwards (the LM never enters silence: it can only lead the utterance); w_i from the word end of w_{i-1} or c_{i-1}
 *   at kappa * (double) lm[w_i * W + w_{i-1}] (w_1: from the start or the end of S, history = silence; a NaN or +inf term: no path,
 *   F_num = +inf); c_i, the silence copy after w_i, from the word end of w_i alone at no LM cost.  Paths end in the word end of w_n or
 *   c_n (n = 0: of S).  Inside a segment the rules above.  A repeated word (w w) is two segments joined by lm[w, w], distinct from
 *   staying inside w.  Evaluated in log space throughout: no product, nothing underflows to "forbidden".  F_num is the same formula
 *   over the subset, so F_num >= F_den up to rounding.  T_u = 0: F_den = 0; F_num = 0 for an empty transcript, else +inf.
 *   occ_t(k) = the posterior probability that frame t's emission is mixture k's = dF / d e(t, k) = the sum of gamma over the positions
 *   that carry k (an entry emits the mixture of the state it moves to); sum over k = 1.
 * Silence need not be word 0: the search net carries its silence word.  Errors, all found before any launch or table build: as
 * sr_bigram_word_posteriors_corpus (scale, floor, max_items, a partial item set, a net of another model, the LM limits, an utterance
 * whose free trellis alone exceeds SRGPU_FB_MB); SR_EINVAL for trans without trans_off or the reverse, trans_off[0] != 0 or decreasing,
 * a word id >= n_words or equal to the silence word; SR_ELIMIT for a chain of more than 8192 positions, a chain trellis (8 bytes per
 * frame and chain position) beyond SRGPU_FB_MB, or 2^31 (frame, mixture) pairs.
 * Memory: launch groups, workspace and the (sr_bigram, kappa) table are the block's above (no word posteriors are kept).  Added, NOT
 * counted in SRGPU_FB_MB: the item buffers, 14 bytes per (frame, distinct mixture of the net) reserved for the free network -- 9 GB at
 * 2 667 words of three states and 80 000 frames; per (frame, distinct mixture of its chain) for the constrained one --, 4 bytes per
 * net position for the position lists; the chains, 20 bytes per chain position; the host keeps slot_off, pos_info and the LM (4 W^2
 * bytes) on the sr_bigram.  One call at a time per handle.  No atomics and a fixed summation order: two identical calls return
 * identical bits.
 * The EBW update is sr_model_create_from_mmi_statistics, unchanged.  An sr_bigram belongs to its model: the next iteration's is created
 * on the NEW model with sr_bigram_create. */

/* Outputs and protocol exactly as sr_net_occupancies_corpus: trans and trans_off both NULL = the free network, both given = the
 * constrained one; out_cost required; items all or none, largest first (ties: smaller id first), at most max_items, not renormalised. */
SR_API int sr_bigram_occupancies_corpus(sr_model* m, sr_corpus* c, sr_bigram* b, int gmm_kernel, double scale,
                                        double posterior_floor, uint32_t max_items, const uint32_t* trans,
                                        const uint64_t* trans_off, double* out_cost, uint16_t* out_count,
                                        uint16_t* out_state, double* out_weight);
/* One MMI E-step exactly as sr_mmi_statistics_corpus: the numerator pass first, ONLY utterances with finite F_num contribute, to
 * either side (its cost gates the free pass on the device); all outputs required, statistics shaped and seeded as
 * sr_accumulate_corpus'; shards add up, the 1e-4 seed once per call and side. */
SR_API int sr_bigram_mmi_statistics_corpus(sr_model* m, sr_corpus* c, sr_bigram* b, int gmm_kernel, double scale,
                                           double posterior_floor, int max_approx, const uint32_t* trans,
                                           const uint64_t* trans_off, double* out_num_cost, double* out_den_cost,
                                           double* num_mean_acc, double* num_mean_w, double* num_var_acc, double* num_var_w,
                                           double* den_mean_acc, double* den_mean_w, double* den_var_acc, double* den_var_w);

/* ---- sMBR training against the bigram search: expected frame accuracy over ITS network ---------------------------------------------
 * Network: the FREE network of sr_bigram_word_posteriors_corpus / sr_bigram_occupancies_corpus, unchanged (the slots, the start's word
 * end, every history kept, no beams, scale = kappa > 0 multiplying every cost in FP64, the word entry in the linear domain with
 * exp(-kappa lm) and therefore the same limits: -kappa lm > 700 SR_ELIMIT, a score of -inf SR_EINVAL, the underflow rule).
 *   ref_states[total_frames] = the reference mixture of every frame; a value >= the model's state count means the frame scores for
 *   none.
 *   A(pi) = sum over t of [k_t(pi) == ref_states[t]], k_t(pi) = the mixture of the net position the path occupies at frame t.  An
 *   entry in this network emits the mixture of the state it moves TO, so the position-1 quirk of sr_net_accuracies_corpus does not
 *   arise: a position's accuracy at t is [state(s) == ref_t], whole.
 *   out_cost[u] = F_u, bit for bit the F_u of sr_bigram_word_posteriors_corpus (the alpha arithmetic is the same).
 *   out_acc[u] = Abar_u = sum over pi of P(pi) A(pi), 0 <= Abar_u <= T_u.  T_u = 0 or F_u = +inf: Abar_u = 0 and no items.
 *   gamma_t(k) = occ_t(k) (c_t(k) - Abar_u) = -(1/kappa) d Abar_u / d e(t, k), occ that of sr_bigram_occupancies_corpus (free);
 *   sum over k of gamma_t(k) = 0.  Per position: gamma_t(s) = occ_t(s) (abar_t(s) + bbar_t(s) - Abar_u), abar_t(s) the expected
 *   accuracy of frames 0 .. t over the paths reaching s, bbar_t(s) that of frames t + 1 .. over its continuations.
 * Items, signs, floors, max_items, "all or none" and the spreading over densities are those of sr_net_accuracies_corpus /
 * sr_smbr_statistics_corpus; seeds and shard additivity those of sr_bigram_mmi_statistics_corpus; the eight arrays go into
 * sr_model_create_from_mmi_statistics unchanged.  The next iteration's sr_bigram is created on the NEW model.
 * Errors, all found before the first launch or table build: those of sr_bigram_occupancies_corpus (free), plus SR_EINVAL for a NULL
 * ref_states.  Workspace per utterance of a launch group: 16 bytes per (frame, position) plus twice the per-utterance vectors of the
 * word-posterior pass, at most SRGPU_FB_MB MiB together; an utterance that alone needs more: SR_ELIMIT.  Item buffers as the free
 * pass of sr_bigram_mmi_statistics_corpus (the statistics call: once per sign).  No atomics and a fixed summation order: two
 * identical calls return identical bits. */
SR_API int sr_bigram_accuracies_corpus(sr_model* m, sr_corpus* c, sr_bigram* b, int gmm_kernel, double scale, double posterior_floor,
                                       uint32_t max_items, const uint16_t* ref_states, double* out_cost, double* out_acc,
                                       uint16_t* out_count, uint16_t* out_state, double* out_weight);
SR_API int sr_bigram_smbr_statistics_corpus(sr_model* m, sr_corpus* c, sr_bigram* b, int gmm_kernel, double scale,
                                            double posterior_floor, int max_approx, const uint16_t* ref_states, double* out_cost,
                                            double* out_acc, double* num_mean_acc, double* num_mean_w, double* num_var_acc,
                                            double* num_var_w, double* den_mean_acc, double* den_mean_w, double* den_var_acc,
                                            double* den_var_w);

/* ---- word lattices and N-best lists for the bigram search: ITS network in the min semiring -----------------------------------------
 * The network of the block above (slots 0 .. W-1 the words, slot h + W the silence copy after word h, the start's word end = the
 * silence word at cost 0, the merge WITHOUT the positional cut: every history is kept, no beams), evaluated in the MIN semiring, in
 * FP64 and without a scale (kappa = 1); lm and tdp widened from float, emission costs the library's FP64 scores.  The order of
 * additions is the specification: a position's cost is min(candidates) + emission; an in-word candidate is prev + penalty; a word
 * entry is hist_h + (double) lm[w * W + h]; an entry to the second state adds the skip penalty to the entry; a word end is the last
 * state + the exit penalty.  EQUAL candidates are resolved in a fixed order and the first stays: in-word from the same position, then
 * one back, then two back, then the entry; among equal entry terms the smallest h.
 * For an utterance of T frames: WE_t(x) = the cost of slot x's word end after frame t; H_t(h) = the history cost, the min over the
 * word ends with history h after frame t (H_{-1}: silence 0, everything else +inf); best = min over x of WE_{T-1}(x).
 * An ARC per (slot x, frame t) with WE_t(x) finite:
 *   word   x for a word slot, the silence word for a copy;
 *   hist   the history its end contributes to: x for a word, h for the copy h + W, silence for the silence word;
 *   last   t;  first = the frame at which the cheapest path to this word end entered the slot;
 *   pred   the history it was entered from: the arg-min h of the entry for a word, h for the copy h + W, silence for the silence word;
 *   fwd    WE_t(x);
 *   bwd    the cheapest continuation from this word end to any word end after frame T - 1 (0 at t = T - 1); unlike the zerogram
 *          lattice's it depends on the slot (the LM and the own copy);
 *   am     (fwd - c_in) - lmc, c_in = the cost the entry started from (H_{first-1}(pred) for a word, WE_{first-1}(word h) for the copy
 *          h + W, WE_{first-1}(silence) for the silence word), lmc = (double) lm[word * W + pred] for a word other than silence, else
 *          0: the acoustic cost of the arc -- transition penalties, emissions and exit of frames first .. last, independent of the
 *          LM and of the predecessor.
 * fwd + bwd is the cost of the cheapest complete path on which slot x ends at t.  The LATTICE of an utterance holds the arcs with
 * fwd + bwd <= best + lattice_beam, ordered by last, then slot (+inf: every arc on some complete path).  A lattice path is a chain of
 * arcs with first_0 = 0, first_{k+1} = last_k + 1, last_K = T - 1 that follows the network's entry rules: a copy arc with hist = h
 * directly follows an arc of word h; a silence-word arc follows the start or a silence-word arc; a word arc follows anything and
 * pays lm[word * W + hist of the arc before] (silence at the start).  Its cost is the left-to-right sum of (lm term + am).
 * APPROXIMATION as for the zerogram lattice: one arc per (slot, end frame), carrying the best start only.  The lattice's paths are a
 * subset of the network's: the first entry of an N-best list is exact (best, up to the rounding of am and of the sum), the k-th is an
 * upper bound of the network's k-th best cost.
 * LM scores: -inf is refused (SR_EINVAL); NaN and +inf mean a forbidden transition; negative finite scores are allowed (nothing is
 * exponentiated here: the -kappa lm > 700 limit above does not apply).  Limits: those of sr_bigram_create; utterances of at most
 * 65535 frames (SR_ELIMIT).  The word entry, W x W terms per frame and utterance, is a min-plus kernel over the float table; the
 * table's other orientation (4 bytes per LM entry: 28 MB at 2 667 words) is built on the device on first use, kept on the sr_bigram
 * handle and NOT counted in SRGPU_FB_MB.  Counted in it, for the utterances processed together: per (frame, slot) 8 (fwd) + 8 (bwd) +
 * 2 (first) + 4 (pred) bytes over the 2 W slots and 16 bytes per frame, i.e. 44 W + 16 bytes per frame; per utterance 28 W' (W' = W
 * rounded up to a multiple of 64: three FP64 vectors and the arg-min) + 28 positions bytes (two rows of cost, first, pred).  An
 * utterance that alone exceeds SRGPU_FB_MB: SR_ELIMIT.  One call at a time per handle.  min and + without atomics: two identical
 * calls return identical bits; +inf stays +inf, never NaN. */

/* Lattice of every utterance, by sr_word_lattice_corpus' protocol: out_arc_off[n_utts + 1] and out_best[n_utts] are always written
 * (T = 0: no arcs and best = 0 -- the empty path ends at the start's word end, as F_u = 0 above); utterance u owns arcs out_arc_off[u]
 * .. out_arc_off[u + 1], first and last counted within the utterance.  The arc arrays (all eight or none) have capacity cap arcs.
 * All NULL: the sizing call, SR_OK with the counts in out_arc_off.  Given but the total exceeds cap: nothing is written to them,
 * out_arc_off still holds the counts needed, SR_EINVAL.  SR_EINVAL also for lattice_beam negative or NaN, a partial set of arc
 * arrays, a bigram net of another model. */
SR_API int sr_bigram_word_lattice_corpus(sr_model* m, sr_corpus* c, sr_bigram* b, int gmm_kernel, double lattice_beam, uint64_t cap,
                                         uint64_t* out_arc_off, double* out_best, uint32_t* out_word, uint32_t* out_hist,
                                         uint32_t* out_pred, uint32_t* out_first, uint32_t* out_last, double* out_fwd, double* out_bwd,
                                         double* out_am);
/* Host only, one utterance: the n_best cheapest DISTINCT word strings (silence removed) among the lattice paths defined above,
 * cheapest first.  lm is any [n_words x n_words] float table in sr_bigram_create's layout; a word entry pays lm_scale * lm[w *
 * n_words + h] (NaN and +inf: forbidden).  With the search's own table and lm_scale = 1, entry 1 is the network's best path; with
 * another table the call is LM rescoring of the lattice.  A string's cost is that of its cheapest path.  Outputs as
 * sr_lattice_nbest; strings of equal cost come in an order that is the same on every call.  SR_EINVAL: as sr_lattice_nbest (n_best
 * = 0, arcs not in (last, slot) order, first > last, last >= n_frames, an am that is NaN or -inf, words_cap too small: *out_count =
 * 0), word or hist >= n_words, a word other than silence whose hist is not itself, silence_word >= n_words, lm_scale NaN or
 * negative, lm NULL. */
SR_API int sr_bigram_lattice_nbest(uint32_t n_frames, uint64_t n_arcs, const uint32_t* word, const uint32_t* hist,
                                   const uint32_t* first, const uint32_t* last, const double* am, uint32_t n_words,
                                   uint32_t silence_word, const float* lm, double lm_scale, uint32_t n_best, uint32_t* out_words,
                                   uint64_t words_cap, uint64_t* out_off, double* out_cost, uint32_t* out_count);

/* ---- streaming bigram-LM recognition: LinearSearch's own initialize / processFrame / getResult (:489-520) -------------------
 * The sr_stream_* interface for the bigram search: utterances fed as their frames arrive, many at once.  sr_bigram_stream_end
 * returns, bit for bit, the items sr_recognize_bigram_corpus returns for that utterance with the same p (any layout: they agree);
 * after t frames sr_bigram_stream_partial returns what it returns for the first t frames taken as a whole utterance.  Items are
 * LinearSearch::getResult's traceback items (word, score, time; silence included), as out_word / out_score / out_time there.
 *
 * sr_bigram_stream_open     up to max_streams concurrently open utterances of up to max_frames frames on (m, b).  p->acoustic_pruning,
 *                           p->lm_pruning and p->gmm_kernel as for sr_recognize_bigram_corpus; p->flags and p->max_word_ends must be 0
 *                           (the stream always runs the "global" layout, and its book grows with the utterance).  Device memory per
 *                           stream: the state image, 16 bytes per position (+ 16 per word above 4 720 words); the two word-end lists,
 *                           48 W bytes; the active list, 4 W bytes; the partial-result items, 12 (max_frames + 1) bytes; and the
 *                           book, 16 bytes per kept word end, grown before each push to hold W entries per frame of it (geometric
 *                           growth).  Plus staging for the largest push: 4 dim + 8 n_states bytes per frame and the scoring kernel's
 *                           own workspaces.
 * sr_bigram_stream_begin    a fresh utterance (initialize, :489-495); *id names it until sr_bigram_stream_end.  Ids as sr_stream_begin.
 * sr_bigram_stream_push     n utterances, ids[n], each at most once; their new frames back to back in feats ([frames x dim] float32),
 *                           utterance i owning rows [frame_off[i], frame_off[i+1]) (frame_off[0] == 0; an empty range is allowed).
 *                           One scoring launch, one search launch; returns when both have finished.  Everything is checked before
 *                           anything is launched: a refused push changes no utterance.
 * sr_bigram_stream_partial  the items after the frames pushed so far (*frames, may be NULL); cap = capacity of each output array (they
 *                           may be NULL if cap is 0).
 * sr_bigram_stream_end      the final items; frees the id.  An utterance ended after 0 frames returns no items.
 * sr_bigram_stream_destroy  before its bigram search net and its model.
 * Errors: SR_EINVAL for an unknown or ended id, an id repeated within one push, max_streams == 0, max_frames == 0, p->flags != 0,
 * p->max_word_ends != 0, a malformed frame_off, and a cap below the item count (*count then holds the count needed; the id stays
 * open); SR_ELIMIT for a push that would take an utterance past max_frames or its book past 2^32 - 1 entries, and for
 * sr_bigram_stream_begin with every id in use; SR_EINTERNAL if a book append found the book full (the growth rule excludes it).
 * Threading: like the model, one host thread at a time. */
typedef struct sr_bigram_stream sr_bigram_stream;  /* a set of concurrently open utterances on one (model, bigram search net) */
SR_API int sr_bigram_stream_open(sr_model* m, sr_bigram* b, const sr_bigram_params* p, uint32_t max_streams, uint64_t max_frames,
                                 sr_bigram_stream** out);
SR_API int sr_bigram_stream_begin(sr_bigram_stream* s, uint32_t* id);
SR_API int sr_bigram_stream_push(sr_bigram_stream* s, uint32_t n, const uint32_t* ids, const float* feats, const uint64_t* frame_off);
SR_API int sr_bigram_stream_partial(sr_bigram_stream* s, uint32_t id, uint32_t* out_word, float* out_score, uint32_t* out_time,
                                    uint32_t cap, uint32_t* count, uint64_t* frames);
SR_API int sr_bigram_stream_end(sr_bigram_stream* s, uint32_t id, uint32_t* out_word, float* out_score, uint32_t* out_time,
                                uint32_t cap, uint32_t* count);
SR_API int sr_bigram_stream_destroy(sr_bigram_stream* s);

/* The stable prefix of the bigram stream's result: sr_stream_stable's construction over the utterance's book.
 *   the tree    the book's entries; the parent of entry b is its back pointer book[b].z < b; the root is the start entry (time 0).
 *   B           the back pointers a later word end can start from: those of the finite state hypotheses (on the active word
 *               slots) and those of the last frame's merged word-end list, from which the next frame builds every word start.  A
 *               silence entry counts as its parent: a silence word end that follows it takes that parent instead (LinearSearch
 *               avoids chains of silence, :410-415), so both continuations run through the parent.
 *   commit      the nearest common ancestor of B; it never moves back.
 *   stable      the items (word, score, time, as sr_bigram_stream_partial reports them) from the start entry to the commit entry.
 *               They are a prefix of every later sr_bigram_stream_partial and of sr_bigram_stream_end whose count is not 0.
 * sr_bigram_stream_stable  n utterances in one launch (bigram_stream_commit_kernel), results in one pinned block: the items back to
 *                          back in out_word / out_score / out_time (cap = capacity of each; NULL allowed if cap is 0), utterance i's
 *                          at [out_off[i], out_off[i + 1]); out_commit[i] = the book time of the commit entry (0: nothing is stable).
 * Errors as sr_stream_stable; SR_EINTERNAL for an utterance whose book overflowed. */
SR_API int sr_bigram_stream_stable(sr_bigram_stream* s, uint32_t n, const uint32_t* ids, uint32_t* out_word, float* out_score,
                                   uint32_t* out_time, uint64_t cap, uint64_t* out_off, uint32_t* out_commit);

/* Diagnostic: does the fp16 matrix pipe keep subnormal inputs on this device (an assumption of SR_GMM_PREFILTER's
 * error bound; when it does not hold, models are scored by SR_GMM_EXACT's kernel instead)? */
SR_API int sr_probe_fp16_denormals(int device, int* preserved);
/* ... and does its fp32 accumulation stay inside the bound's model?  Adversarial 96-term (dimension <= 46) and 128-term
 * (dimension 47..62) fp16 dot products with known exact sums through the prefilter's own MFMA chains: within_model = 1 iff every
 * |error| <= 87 (96 terms) / 132 (128 terms) * 2^-24 * sum |a_k b_k|; worst_ratio (may be NULL) = the largest
 * |error| / (2^-24 * sum |a_k b_k|) seen, the 128-term ratios scaled by 87 / 132.  The probes run at model creation (the chain
 * length the model uses). */
SR_API int sr_probe_fp16_accumulation(int device, int* within_model, double* worst_ratio);

/* Test hook: the candidate masks the fp16 prefilter alone writes for `feats` ([n_frames x dim], host), by one of its two routes --
 * 0: frames stationary, the model staged through LDS; 1: a state group stationary in registers, the frames' operands streamed (models
 * of dimension <= 46; wider ones run the staged kernel on either route).  Both routes write the same bits; SRGPU_PREFILTER=staged|
 * stationary (read when a model is created; default stationary) picks the one the scoring calls take.  masks: [n_groups][n_frames][4]
 * 32-bit words, one per state slot; masks == NULL only reports n_groups.  SR_EINVAL for a model the prefilter does not score. */
SR_API int sr_prefilter_masks(sr_model* m, const float* feats, uint64_t n_frames, int route, uint32_t* n_groups, uint32_t* masks,
                              uint64_t cap_words);
/* The stationary route cuts a launch's frames into ranges; a launch of more than *frames frames has at least two (tests straddle one). */
SR_API int sr_prefilter_range_frames(uint32_t* frames);
/* Test hook: the FP64 refinement alone, on candidate masks the caller supplies instead of the prefilter's: uploads `feats` ([n_frames x
 * dim], host), runs the feature transpose and the refinement (the deferred-leftover route under SRGPU_DEFER_MB / SRGPU_DEFER_CAP as a
 * scoring call would) and returns the table out[n_frames x n_states]: per (frame, state) the minimum, under strict `<` from 1e10, over
 * the densities whose bits are set.  masks: sr_prefilter_masks' layout, n_words == n_groups * n_frames * 4 or SR_EINVAL; bits at or
 * beyond a pseudo-state's density count and slots beyond the last pseudo-state are ignored, so every array of that size is valid. */
SR_API int sr_refine_masks(sr_model* m, const float* feats, uint64_t n_frames, const uint32_t* masks, uint64_t n_words, double* out);
/* The refinement's launch geometry for n_frames frames of this model: out[0] threads per workgroup, out[1] pseudo-states per workgroup,
 * out[2] frames per workgroup (workgroup y of a state group takes frames [y * out[2], (y + 1) * out[2]); the thread (wave, lane) takes
 * frame y * out[2] + wave * 64 + it * out[0] + lane in iteration it), out[3] chunks of 32 densities per state.  Tests lay masks out by it. */
SR_API int sr_refine_geometry(sr_model* m, uint64_t n_frames, uint32_t out[4]);
/* Test hook: the last step of a recognition call alone, on search outputs the caller supplies (host arrays) instead of a search's:
 * utterance u has counts[u] words at words[frame_off[u] ..] and the flags flags[u] (4: its traceback did not walk).  Returns what
 * sr_recognize_corpus would: the words back to back in out_words with out_word_off[n_utts + 1], or SR_ECORRUPT naming the first
 * utterance whose flag is raised or whose count exceeds its frames.  The words are compacted on the device, or by the host with
 * SRGPU_GATHER=host (read when a model is created; a diagnostic knob, same output). */
SR_API int sr_gather_words(sr_model* m, uint32_t n_utts, const uint64_t* frame_off, const uint32_t* counts, const uint32_t* flags,
                           const uint32_t* words, uint32_t* out_words, uint64_t* out_word_off);
/* Test hook: the nearest-common-ancestor fold of the stable calls alone (commit_point.h), on forests the caller supplies (host arrays).
 * Set i: the tree parent[node_off[i] .. node_off[i + 1]) -- parent[0] = 0 is the root, parent[j] < j -- the candidate nodes
 * set[set_off[i] .. set_off[i + 1]) and floor[i], an ancestor of all of them (the previous commit point; 0 always qualifies), at which
 * a walk may stop.  out[i] = the nearest common ancestor of the candidates.  One workgroup per set: a thread folds its candidates, a
 * wave folds by shuffles, the waves through LDS.  SR_EINVAL for a parent not below its child, a node or floor out of range, an empty
 * set or an empty tree, node_off[0] or set_off[0] != 0. */
SR_API int sr_commit_points(sr_model* m, uint32_t n_sets, const uint64_t* node_off, const uint32_t* parent, const uint64_t* set_off,
                            const uint32_t* set, const uint32_t* floor, uint32_t* out);
/* Test hook: the zerogram search alone, on a score table the caller supplies instead of the GMM scores: sr_recognize_corpus' pass
 * -- the same chunks, launch order, kernel route from p->flags, replay workspace, compaction of the words and traceback copies --
 * except that a chunk's score step copies rows [f0, f1) of `scores` into the chunk's table (row stride: n_states rounded up to 8,
 * the padding columns +inf) where sr_recognize_corpus scores the chunk's frames.  scores: host, [total_frames x n_states] row-major,
 * the corpus's frames in order; any bit pattern is a valid entry (negative, +inf, NaN); n_scores == total_frames * n_states or
 * SR_EINVAL.  c is an ordinary corpus: its frame offsets are used, its features are never read, and p->gmm_kernel is ignored.
 * exact_negative (0 or 1, SR_EINVAL otherwise) is what sr_recognize_corpus derives from the model ("an emission cost of this model
 * can be negative or NaN"): 1 lets the word-per-lane kernel run its variant that replays the reference's early-out in place (where
 * its word-end arrays fit the LDS), 0 makes a fast kernel that meets such a cost hand the utterance to the replay kernel.  Outputs as
 * sr_recognize_corpus, and out_flags[n_utts] (not NULL): per utterance the search's flags as left on the device -- 1: the sequential
 * boundary replay was taken, 2: a fast kernel handed the utterance to the replay kernel, 4: the traceback did not walk (the call
 * returns SR_ECORRUPT then, out_flags filled). */
SR_API int sr_recognize_corpus_scores(sr_model* m, sr_corpus* c, sr_lexicon* l, const sr_search_params* p, const double* scores,
                                      uint64_t n_scores, int exact_negative, uint32_t* out_words, uint64_t* out_word_off,
                                      double* tb_score, uint16_t* tb_word, uint16_t* tb_bkp, uint32_t* out_flags);
/* Test hook: the bigram search alone on a score table the caller supplies: sr_recognize_bigram_corpus' pass -- the same chunks, book
 * sizing from p->max_word_ends, layout from p->flags, global-states grid, compaction of the items, SR_ELIMIT -- except that a chunk's
 * score step copies rows [f0, f1) of `scores` into the chunk's table (row stride: n_states rounded up to 8, the padding columns
 * +inf).  scores: host, [total_frames x n_states] row-major; any bit pattern is a valid entry, but the search converts an entry to
 * float with a cast, so a finite one must stay below FLT_MAX in magnitude; n_scores == total_frames * n_states or SR_EINVAL.  The
 * corpus's features are never read and p->gmm_kernel is ignored.  Outputs as sr_recognize_bigram_corpus. */
SR_API int sr_recognize_bigram_corpus_scores(sr_model* m, sr_corpus* c, sr_bigram* b, const sr_bigram_params* p, const double* scores,
                                             uint64_t n_scores, uint32_t* out_word, float* out_score, uint32_t* out_time,
                                             uint64_t* out_off);

/* Test hook: the forced aligners alone on a score table the caller supplies: sr_align_corpus' (pruned 0) or sr_align_corpus_pruned's
 * (pruned 1; SR_EINVAL for another value) pass -- the same checks and limits, chunks, utterance order and launches -- except that a
 * chunk's score step copies rows [f0, f1) of `scores` into the chunk's table (row stride: n_states rounded up to 8, the padding columns
 * +inf).  scores: host, [total_frames x n_states] row-major; n_scores == total_frames * n_states or SR_EINVAL.  Entries: any finite
 * value and +inf are valid.  NaN and -inf are no emission costs, but the aligners define what they do with them: the comparisons of the
 * reference (Alignment.cpp) in the reference's order, so the result is the oracle's on the same table, bit for bit (a NaN compares
 * false and stays where the loop transition carries it; -inf wins every comparison and -inf + inf is NaN).  pruning_threshold is
 * ignored with pruned 0.  The corpus's features are never read. */
SR_API int sr_align_corpus_scores(sr_model* m, sr_corpus* c, const uint16_t* automata, const uint64_t* aut_off, const double tdp[3],
                                  uint16_t silence_state, int pruned, double pruning_threshold, const double* scores,
                                  uint64_t n_scores, uint16_t* out_states, double* out_cost);
/* Test hook: the forward-backward pass alone on a score table the caller supplies: sr_state_posteriors_corpus' pass -- the same
 * checks, chunks, launch groups (SRGPU_FB_MB), block sizes, item path and outputs -- with the score step replaced as above.  Entries:
 * any finite value and +inf are valid.  A NaN entry counts as +inf (the cell is on no path); a -inf entry takes every path through
 * its cell to -inf.  An utterance whose F_u is not finite (+inf: no path; -inf or NaN from such entries) returns F_u as computed and
 * no items; no weight returned is NaN or exceeds 1 by more than rounding, and the other utterances of the call are unaffected.  The
 * production passes (sr_state_posteriors_corpus, sr_baum_welch_corpus and the adaptation statistics over them) run the same kernels,
 * so the same holds for a model whose scores overflow. */
SR_API int sr_state_posteriors_corpus_scores(sr_model* m, sr_corpus* c, const uint16_t* automata, const uint64_t* aut_off,
                                             const double tdp[3], uint16_t silence_state, const double* scores, uint64_t n_scores,
                                             double posterior_floor, uint32_t max_items, double* out_cost, uint16_t* out_count,
                                             uint16_t* out_state, double* out_weight);

/* Test hooks: the forward-backward passes over the recognition network alone on a score table the caller supplies:
 * sr_word_posteriors_corpus', sr_net_occupancies_corpus' (the free network, or the transcripts' chains with trans / trans_off) and
 * sr_net_accuracies_corpus' pass -- the same checks, chunks, launch groups (SRGPU_FB_MB), block sizes, item path and outputs -- except
 * that a chunk's score step copies rows [f0, f1) of `scores` into the chunk's table (row stride: n_states rounded up to 8, the padding
 * columns +inf).  scores: host, [total_frames x n_states] row-major; n_scores == total_frames * n_states or SR_EINVAL.  The corpus's
 * features are never read and p->gmm_kernel is ignored.
 * Entries (the contract of sr_state_posteriors_corpus_scores): any finite value and +inf are valid.  A NaN entry counts as +inf, as an
 * entry: every path that pays that emission is dead, and paths that pay another emission at the same slot are not (position 1 of a
 * word: a path entering there pays the word's FIRST state's emission, a path arriving inside the word the slot's own).  A -inf entry
 * takes every path through it to -inf.  An utterance whose F_u is not finite (+inf: no path; -inf from such entries) returns F_u as
 * computed and no items, and for the accuracies Abar_u = 0.  No weight returned is NaN; no posterior or occupancy exceeds 1 by more
 * than rounding, and |gamma| <= T_u.  The other utterances of the call are unaffected.  The production passes
 * (sr_word_posteriors_corpus, sr_recognize_confidence_corpus, sr_net_occupancies_corpus, sr_mmi_statistics_corpus,
 * sr_net_accuracies_corpus, sr_smbr_statistics_corpus) run the same kernels, so the same holds for a model whose scores overflow. */
SR_API int sr_word_posteriors_corpus_scores(sr_model* m, sr_corpus* c, sr_lexicon* l, const sr_search_params* p, double scale,
                                            double posterior_floor, uint32_t max_items, const double* scores, uint64_t n_scores,
                                            double* out_cost, uint16_t* out_count, uint32_t* out_word, double* out_weight);
SR_API int sr_net_occupancies_corpus_scores(sr_model* m, sr_corpus* c, sr_lexicon* l, const sr_search_params* p, double scale,
                                            double posterior_floor, uint32_t max_items, const uint32_t* trans, const uint64_t* trans_off,
                                            const double* scores, uint64_t n_scores, double* out_cost, uint16_t* out_count,
                                            uint16_t* out_state, double* out_weight);
SR_API int sr_net_accuracies_corpus_scores(sr_model* m, sr_corpus* c, sr_lexicon* l, const sr_search_params* p, double scale,
                                           double posterior_floor, uint32_t max_items, const uint16_t* ref_states, const double* scores,
                                           uint64_t n_scores, double* out_cost, double* out_acc, uint16_t* out_count, uint16_t* out_state,
                                           double* out_weight);

/* Test hooks: the forward-backward passes over the bigram search network alone on a score table the caller supplies:
 * sr_bigram_word_posteriors_corpus', sr_bigram_occupancies_corpus' (the free network, or the transcripts' chains with trans /
 * trans_off) and sr_bigram_accuracies_corpus' pass -- the same checks, chunks, launch groups (SRGPU_FB_MB), utterance order, table
 * cache, workspace, kernels, item path and outputs -- except that a chunk's score step copies rows [f0, f1) of `scores` into the chunk's
 * table (row stride: n_states rounded up to 8, the padding columns +inf); there is no gmm_kernel argument.  scores: host,
 * [total_frames x n_states] row-major; n_scores == total_frames * n_states or SR_EINVAL.  The corpus's features are never read.
 * Entries: any finite value and +inf are valid.  A NaN entry counts as +inf: every path that pays that emission is dead.  A -inf
 * entry is refused with SR_EINVAL before any launch: the word entry is a sum in the linear domain relative to the frame's best
 * history, which has no meaning at -inf (the LM's -inf is refused for the same reason).  An utterance whose F_u is +inf (no path)
 * returns no items, and for the accuracies Abar_u = 0; no weight returned is NaN; the other utterances of the call are unaffected.
 * The linear-domain rule holds here as in production: a word all of whose entry terms underflow against the frame's best history is
 * not entered at that frame. */
SR_API int sr_bigram_word_posteriors_corpus_scores(sr_model* m, sr_corpus* c, sr_bigram* b, double scale, double posterior_floor,
                                                   uint32_t max_items, const double* scores, uint64_t n_scores, double* out_cost,
                                                   uint16_t* out_count, uint32_t* out_word, double* out_weight);
SR_API int sr_bigram_occupancies_corpus_scores(sr_model* m, sr_corpus* c, sr_bigram* b, double scale, double posterior_floor,
                                               uint32_t max_items, const uint32_t* trans, const uint64_t* trans_off,
                                               const double* scores, uint64_t n_scores, double* out_cost, uint16_t* out_count,
                                               uint16_t* out_state, double* out_weight);
SR_API int sr_bigram_accuracies_corpus_scores(sr_model* m, sr_corpus* c, sr_bigram* b, double scale, double posterior_floor,
                                              uint32_t max_items, const uint16_t* ref_states, const double* scores, uint64_t n_scores,
                                              double* out_cost, double* out_acc, uint16_t* out_count, uint16_t* out_state,
                                              double* out_weight);

/* ---- measurement --------------------------------------------------------------------------------
 * When enabled, every kernel launch of this model handle is bracketed by HIP events on the
 * launch stream; sr_profile_read() synchronises and returns accumulated device times. */
typedef struct {
  double gmm_ms;        /* GMM scoring kernel(s) */
  uint64_t gmm_launches;
  double gmm_flops;     /* algorithmic: 4 * dim * densities * frames per launch, summed */
  double search_ms;     /* Viterbi decode / align kernels */
  uint64_t search_launches;
  double search_bytes;  /* algorithmic: (8*S + 4*P) * frames (decode) / (8+1)*N * frames (align) / 32*N * frames (forward-backward; N = P over a network) / (30*W + 48) * frames (word lattice) / (44*P + 120*W) * frames (bigram word lattice: rows of both walks, word-end tables out and in) / bigram MMI passes: 24*N * frames for a chain's forward-backward, 32*P * frames for the free network's, + 16*N (8*P: the count pass is in the 32) * frames for the two item passes' reads of gamma / fMLLR statistics: (32*R + 4*D) * frames + 16*R*C * segments (R = D+1 rounded up to 16 rows of the two folds out and in, C columns of a segment's partial sums out and in) / 8*D * frames (sr_corpus_transform: a row in, a row out) */
  uint64_t frames;      /* frames processed */
  uint64_t refined_pairs;      /* SR_GMM_PREFILTER: (frame, state) pairs scored ... */
  uint64_t refined_densities;  /* ... and densities the FP64 stage had to evaluate for them (>= 1 per pair) */
  double prefilter_ms;         /* SR_GMM_PREFILTER: the 16-bit MFMA pass (with the feature transpose) ... */
  double refine_ms;            /* ... and the FP64 refinement; both are inside gmm_ms */
} sr_profile;
SR_API int sr_profile_enable(sr_model* m, int on);
SR_API int sr_profile_reset(sr_model* m);
SR_API int sr_profile_read(sr_model* m, sr_profile* out);

#ifdef __cplusplus
}
#endif
#endif /* SRGPU_H */
