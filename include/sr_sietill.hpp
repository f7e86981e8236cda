// sr_sietill.hpp -- C++ host-side mirror of the reference's scorer / search interface, on top of the
// C ABI in srgpu.h.  Header-only; link with libsrgpu.so.
//
// Same names, argument meaning and error behaviour as the reference classes for this path, so code
// (and tests) written against `sietill` read the same:
//
//   sr::FeatureScorer          FeatureScorer                sietill/FeatureScorer.hpp:12-16
//   sr::Lexicon                Lexicon / MarkovAutomaton    sietill/Lexicon.hpp:16-33, MarkovAutomaton.hpp:17-67
//   sr::TdpModel               TdpModel                     sietill/TdpModel.hpp:13-29, TdpModel.cpp:19-29
//   sr::MixtureModel           MixtureModel (as scorer)     sietill/Mixtures.hpp:18-92
//   sr::Corpus                 Corpus (feature store)       sietill/Corpus.hpp:55-84
//   sr::Recognizer             Recognizer                   sietill/Recognizer.hpp:91-132
//                              (+ recognize_with_confidence: each word's frame-based confidence C_max, Wessel et al. 2001)
//                              (+ recognize_nbest: the N cheapest distinct word strings of each segment's word lattice)
//   sr::StreamingRecognizer    Recognizer fed frame by frame (sr_stream_*; the shape of RWTH ASR's OfflineRecognizer::processFeature)
//   sr::Aligner                Aligner                      sietill/Alignment.hpp:19-63
//   sr::FeaturePostProcessor   SignalAnalysis::process_features  sietill/SignalAnalysis.cpp:320-336,340-349,379-399
//   sr::read_feature_file, write_alignment, read_alignment    sietill/IO.cpp:48-69, Alignment.cpp:303-318
//   sr::Trainer (re-alignment) Trainer::train's align loop   sietill/Training.cpp:163-184, :239-253, :585-612
//                              (+ baum_welch: forward-backward E-step in place of realign + accumulate)
//                              (+ split, eliminate, train: the reference's schedule from one density per mixture upwards)
//
// Differences, all forced by the device boundary: features are passed as (pointer, frame count)
// instead of FeatureIter pairs; MixtureModel::prepare_sequence really does work (it fills the dense
// score table on the GPU, like NeuralNetwork::prepare_sequence does on the CPU,
// sietill/NeuralNetwork.cpp:184-199); errors that the reference reports with abort()
// (Mixtures.cpp:97-102) are thrown as std::runtime_error carrying the same text.
#pragma once
#include <algorithm>
#include <cstdint>
#include <fstream>
#include <limits>
#include <memory>
#include <stdexcept>
#include <time.h>
#include <string>
#include <utility>
#include <vector>

#include "srgpu.h"

namespace sr {

typedef size_t WordIdx;     // sietill/Types.hpp:14-17
typedef uint16_t StateIdx;

inline void check(int rc) {
  if (rc != SR_OK) throw std::runtime_error(sr_last_error());
}
// the loaded library must lay its parameter structs out like the header this file was compiled against (srgpu.h)
inline void check_abi() {
  static const bool ok = sr_abi_version() == SR_ABI_VERSION;
  if (!ok) throw std::runtime_error("libsrgpu.so: ABI version differs from the srgpu.h this binding was compiled against");
}

// ---- FeatureScorer.hpp:12-16 ----------------------------------------------------------------------
class FeatureScorer {
 public:
  virtual ~FeatureScorer() {}
  virtual void prepare_sequence(const float* begin, size_t n_frames) = 0;
  virtual double score(size_t frame, StateIdx state_idx) const = 0;
};

// ---- MarkovAutomaton.hpp:17-67, Lexicon.cpp:11-62 ---------------------------------------------------
struct MarkovAutomaton {
  std::vector<StateIdx> states;
  MarkovAutomaton() {}
  MarkovAutomaton(StateIdx start, uint16_t num, uint16_t repetitions) {
    for (StateIdx s = start; s < start + num; s++) states.insert(states.end(), repetitions, s);
  }
  StateIdx first_state() const { return states.front(); }
  StateIdx last_state() const { return states.back(); }
  size_t num_states() const { return states.size(); }
  StateIdx operator[](size_t i) const { return states[i]; }
  static MarkovAutomaton concat(std::vector<MarkovAutomaton const*> automata) {
    MarkovAutomaton r;
    for (auto a : automata) r.states.insert(r.states.end(), a->states.begin(), a->states.end());
    return r;
  }
};

class Lexicon {
 public:
  WordIdx add_word(std::string const& orth, uint16_t num_states, uint16_t state_repetitions, bool silence = false) {
    const WordIdx w = automata_.size();
    if (silence) silence_ = w;
    const StateIdx start = automata_.empty() ? 0 : StateIdx(automata_.back().last_state() + 1);
    orth_.push_back(orth);
    automata_.push_back(MarkovAutomaton(start, num_states, state_repetitions));
    return w;
  }
  MarkovAutomaton const& get_silence_automaton() const { return automata_[silence_]; }
  MarkovAutomaton const& get_automaton_for_word(WordIdx w) const { return automata_[w]; }
  StateIdx num_states() const { return automata_.back().last_state() + 1; }
  WordIdx num_words() const { return automata_.size(); }
  WordIdx silence_idx() const { return silence_; }
  WordIdx operator[](std::string const& orth) const {
    auto it = std::find(orth_.begin(), orth_.end(), orth);
    return it == orth_.end() ? WordIdx(-1) : WordIdx(it - orth_.begin());  // Lexicon.cpp:57-62
  }

 private:
  std::vector<std::string> orth_;
  std::vector<MarkovAutomaton> automata_;
  WordIdx silence_ = 0;
};

// ---- TdpModel.cpp:19-29 ------------------------------------------------------------------------------
struct TdpModel {
  StateIdx silence_state;
  double tdp_loop, tdp_forward, tdp_skip;
  TdpModel(StateIdx silence_state, double loop, double forward, double skip)
      : silence_state(silence_state), tdp_loop(loop), tdp_forward(forward), tdp_skip(skip) {}
  double score(StateIdx to, size_t jump) const {
    if (to == silence_state) return tdp_forward;
    switch (jump) {
      case 0: return tdp_loop;
      case 1: return tdp_forward;
      case 2: return tdp_skip;
    }
    return std::numeric_limits<double>::infinity();
  }
};

// ---- Mixtures.hpp:18-92: the GMM as a FeatureScorer, resident on one GPU ----------------------------------
class MixtureModel : public FeatureScorer {
 public:
  enum VarianceModel { GLOBAL_POOLING, MIXTURE_POOLING, NO_POOLING };  // Mixtures.hpp:20-24

  // MixtureModel(config, dimension, num_mixtures, var_model, max_approx) with action "recognize" and
  // "load-mixtures-from" = path (Mixtures.cpp:156-174)
  MixtureModel(std::string const& load_mixtures_from, size_t dimension, VarianceModel var_model, bool max_approx,
               int device = 0, int gmm_kernel = SR_GMM_DEFAULT)
      : dimension(dimension), var_model(var_model), gmm_kernel(gmm_kernel), path_(load_mixtures_from), max_approx_(max_approx),
        device_(device) {
    check_abi();
    check(sr_model_load_mixset(load_mixtures_from.c_str(), (uint32_t)dimension, (int)var_model, max_approx ? 1 : 0, device, &h_));
    uint32_t d, s;
    uint64_t c;
    check(sr_model_info(h_, &d, &s, &c));
    num_mixtures_ = s;
    num_densities_ = c;
  }
  // MixtureModel(config, dimension, num_mixtures, var_model, max_approx) with action "train" (Mixtures.cpp:156-174): one density per
  // mixture, the flat start of sr::Trainer::train.  Its table values (mean 0, variance 1, weight 1) are placeholders: the first
  // pass of training reads none of them.
  MixtureModel(size_t dimension, size_t num_mixtures, VarianceModel var_model, bool max_approx, int device = 0,
               int gmm_kernel = SR_GMM_DEFAULT)
      : dimension(dimension), var_model(var_model), gmm_kernel(gmm_kernel), num_mixtures_(num_mixtures), num_densities_(num_mixtures),
        max_approx_(max_approx), device_(device) {
    check_abi();
    std::vector<uint32_t> dens_off(num_mixtures + 1);
    for (size_t s = 0; s <= num_mixtures; s++) dens_off[s] = (uint32_t)s;
    std::vector<double> zeros(num_mixtures * dimension, 0.0), ones(num_mixtures * dimension, 1.0);
    check(sr_model_create(device, (uint32_t)dimension, (uint32_t)num_mixtures, dens_off.data(), zeros.data(), ones.data(), zeros.data(),
                          zeros.data(), max_approx ? 1 : 0, &h_));
  }
  // takes over a device model derived from `like` (sr::Trainer::mmi_iteration, split, eliminate, train); it has no file, so it cannot
  // replicate()
  MixtureModel(sr_model* adopted, MixtureModel const& like)
      : dimension(like.dimension), var_model(like.var_model), gmm_kernel(like.gmm_kernel), h_(adopted),
        num_mixtures_(like.num_mixtures_), num_densities_(like.num_densities_), max_approx_(like.max_approx_), device_(like.device_) {
    uint64_t c = 0;
    if (sr_model_info(h_, nullptr, nullptr, &c) == SR_OK) num_densities_ = c;  // split and eliminate change it
  }
  ~MixtureModel() { sr_model_destroy(h_); }
  MixtureModel(MixtureModel const&) = delete;
  MixtureModel& operator=(MixtureModel const&) = delete;

  const size_t dimension;
  const VarianceModel var_model;
  int gmm_kernel;

  size_t num_mixtures() const { return num_mixtures_; }
  size_t num_densities() const { return num_densities_; }
  sr_model* handle() const { return h_; }
  int device() const { return device_; }
  bool max_approx() const { return max_approx_; }
  // another replica of the same model file on `device` (utterance batches shard across devices, every device holds the
  // whole model: Recognizer::recognize(corpus, devices))
  std::unique_ptr<MixtureModel> replicate(int device) const {
    return std::unique_ptr<MixtureModel>(new MixtureModel(path_, dimension, var_model, max_approx_, device, gmm_kernel));
  }

  // the per-density tables in sr_model_create's shape (sr_model_tables), e.g. for a checkpoint of a model that was just split
  struct Tables {
    std::vector<uint32_t> dens_off;             // [num_mixtures + 1]
    std::vector<double> means, inv_vars;        // [num_densities x dimension]
    std::vector<double> norm, logw;             // [num_densities]
  };
  Tables tables() const {
    Tables t;
    t.dens_off.resize(num_mixtures_ + 1);
    check(sr_model_topology(h_, t.dens_off.data(), nullptr, nullptr));
    t.means.resize(num_densities_ * dimension); t.inv_vars.resize(num_densities_ * dimension);
    t.norm.resize(num_densities_); t.logw.resize(num_densities_);
    check(sr_model_tables(h_, t.means.data(), t.inv_vars.data(), t.norm.data(), t.logw.data()));
    return t;
  }

  // FeatureScorer: one dense [T x S] table per sequence
  void prepare_sequence(const float* begin, size_t n_frames) override {
    table_.resize(n_frames * num_mixtures_);
    check(sr_score_frames(h_, begin, n_frames, gmm_kernel, table_.data()));
  }
  double score(size_t frame, StateIdx mixture_idx) const override { return table_[frame * num_mixtures_ + mixture_idx]; }

 private:
  sr_model* h_ = nullptr;
  size_t num_mixtures_ = 0, num_densities_ = 0;
  std::vector<double> table_;
  std::string path_;
  bool max_approx_ = true;
  int device_ = 0;
};

// ---- Corpus.hpp:55-84: contiguous features + offsets + reference word sequences ---------------------------
class Corpus {
 public:
  explicit Corpus(size_t features_per_timeframe, double frame_duration = 0.010)
      : features_per_timeframe_(features_per_timeframe), frame_duration_(frame_duration) {
    frame_offsets_.push_back(0);
    orth_offsets_.push_back(0);
  }
  // speaker: the segment's speaker index (the corpus description's `speaker` field, numbered by the caller); sr::SpeakerAdaptation
  void add_segment(const float* feats, size_t n_frames, std::vector<WordIdx> const& orth, uint32_t speaker = 0) {
    speakers_.push_back(speaker);
    features_.insert(features_.end(), feats, feats + n_frames * features_per_timeframe_);
    frame_offsets_.push_back(frame_offsets_.back() + n_frames);
    orths_.insert(orths_.end(), orth.begin(), orth.end());
    orth_offsets_.push_back(orths_.size());
  }
  size_t get_corpus_size() const { return orth_offsets_.size() - 1; }
  size_t get_total_frame_count() const { return frame_offsets_.back(); }
  size_t get_features_per_timeframe() const { return features_per_timeframe_; }
  double get_frame_duration() const { return frame_duration_; }
  std::pair<const WordIdx*, const WordIdx*> get_word_sequence(size_t s) const {
    return {orths_.data() + orth_offsets_[s], orths_.data() + orth_offsets_[s + 1]};
  }
  std::pair<const float*, size_t> get_feature_sequence(size_t s) const {
    return {features_.data() + frame_offsets_[s] * features_per_timeframe_, (size_t)(frame_offsets_[s + 1] - frame_offsets_[s])};
  }
  const float* features() const { return features_.data(); }
  const uint64_t* frame_offsets() const { return frame_offsets_.data(); }
  std::vector<uint32_t> const& speakers() const { return speakers_; }

 private:
  std::vector<uint32_t> speakers_;
  size_t features_per_timeframe_;
  double frame_duration_;
  std::vector<uint64_t> frame_offsets_;
  std::vector<float> features_;
  std::vector<size_t> orth_offsets_;
  std::vector<WordIdx> orths_;
};

// ---- Recognizer.hpp:18-47 ---------------------------------------------------------------------------------
struct EDAccumulator {
  uint16_t total_count = 0, substitute_count = 0, insert_count = 0, delete_count = 0;
  EDAccumulator& operator+=(EDAccumulator const& o) {
    total_count += o.total_count; substitute_count += o.substitute_count;
    insert_count += o.insert_count; delete_count += o.delete_count;
    return *this;
  }
  void substitution_error() { total_count++; substitute_count++; }
  void insertion_error() { total_count++; insert_count++; }
  void deletion_error() { total_count++; delete_count++; }
};

struct RecognitionStats {  // what Recognizer::recognize prints (Recognizer.cpp:82-91)
  EDAccumulator errors;
  size_t ref_words = 0, sentence_errors = 0, corpus_size = 0;
  double wer = 0, ser = 0, seconds = 0, rtf = 0;
  std::vector<std::vector<WordIdx>> hypotheses;
  std::vector<uint64_t> frames_per_device;  // recognize(corpus, devices): how the LPT deal loaded the devices
};

class Recognizer {
 public:
  // Recognizer(config, lexicon, scorer, tdp_model): "am-threshold" (20.0), "word-penalty" (10.0),
  // "max-recognition-runs" (1000) as in Recognizer.cpp:31-34
  Recognizer(Lexicon const& lexicon, MixtureModel& scorer, TdpModel const& tdp_model, double am_threshold = 20.0,
             double word_penalty = 10.0, size_t max_recognition_runs = 1000)
      : am_threshold_(am_threshold), word_penalty_(word_penalty), max_recognition_runs_(max_recognition_runs),
        lexicon_(lexicon), scorer_(scorer) {
    word_off_.assign(1, 0);
    for (WordIdx w = 0; w < lexicon.num_words(); w++) {
      auto const& a = lexicon.get_automaton_for_word(w);
      automaton_.insert(automaton_.end(), a.states.begin(), a.states.end());
      word_off_.push_back((uint32_t)automaton_.size());
    }
    tdp_[0] = tdp_model.tdp_loop; tdp_[1] = tdp_model.tdp_forward; tdp_[2] = tdp_model.tdp_skip;
    silence_state_ = tdp_model.silence_state;
    net_ = make_net(scorer);
  }
  ~Recognizer() {
    for (auto& r : replicas_) sr_lexicon_destroy(r.net);
    sr_lexicon_destroy(net_);
  }
  Recognizer(Recognizer const&) = delete;

  sr_search_params search_params() const {
    sr_search_params p = sr_search_params();  // zeroed, then field by field: a field added to the struct cannot shift these
    p.am_threshold = am_threshold_;
    p.word_penalty = word_penalty_;
    p.gmm_kernel = scorer_.gmm_kernel;
    return p;
  }

  // Recognizer::recognizeSequence_pruned (Recognizer.cpp:103-232)
  void recognizeSequence_pruned(const float* feature_begin, size_t n_frames, std::vector<WordIdx>& output) {
    const uint64_t off[2] = {0, n_frames};
    std::vector<uint32_t> words(std::max<size_t>(n_frames, 1));
    uint64_t woff[2];
    const sr_search_params p = search_params();
    check(sr_recognize_batch(scorer_.handle(), net_, &p, feature_begin, off, 1, words.data(), woff));
    output.assign(words.begin(), words.begin() + woff[1]);
  }

  // Recognizer::recognize (Recognizer.cpp:38-92): the whole corpus in one device pass.
  // With `devices`: the reference's `#pragma omp parallel for` over segments (:46-47) at device granularity -- the
  // segments are dealt to the devices by frames (greedy LPT), every device gets a replica of the model and of the search
  // network (created on first use, kept) and one host thread that feeds and recognises its shard; hypotheses come back in
  // corpus order.  A device may be listed more than once (two replicas on it).  No collective.
  RecognitionStats recognize(Corpus const& corpus) { return recognize(corpus, std::vector<int>()); }
  RecognitionStats recognize(Corpus const& corpus, std::vector<int> const& devices) {
    RecognitionStats st;
    const size_t n = std::min(corpus.get_corpus_size(), max_recognition_runs_);
    st.corpus_size = n;
    const uint64_t total = corpus.frame_offsets()[n];
    std::vector<uint32_t> words(std::max<uint64_t>(total, 1));
    std::vector<uint64_t> woff(n + 1);
    const sr_search_params p = search_params();
    double t0;
    if (devices.size() <= 1 && (devices.empty() || devices[0] == scorer_.device())) {
      t0 = now();
      check(sr_recognize_batch(scorer_.handle(), net_, &p, corpus.features(), corpus.frame_offsets(), (uint32_t)n,
                               words.data(), woff.data()));
    } else {
      std::vector<sr_model*> models;
      std::vector<sr_lexicon*> nets;
      std::vector<size_t> used(replicas_.size(), 0);
      bool own_used = false;
      for (int dev : devices) {  // the recogniser's own model serves its device once, replicas the rest
        if (dev == scorer_.device() && !own_used) { own_used = true; models.push_back(scorer_.handle()); nets.push_back(net_); continue; }
        size_t r = 0;
        for (; r < replicas_.size(); r++)
          if (replicas_[r].model->device() == dev && !used[r]) break;
        if (r == replicas_.size()) {
          Replica rep;
          rep.model = scorer_.replicate(dev);
          rep.net = make_net(*rep.model);
          replicas_.push_back(std::move(rep));
          used.push_back(0);
        }
        used[r] = 1;
        models.push_back(replicas_[r].model->handle());
        nets.push_back(replicas_[r].net);
      }
      st.frames_per_device.assign(devices.size(), 0);
      t0 = now();
      check(sr_recognize_batch_multi(models.data(), nets.data(), (uint32_t)models.size(), &p, corpus.features(),
                                     corpus.frame_offsets(), (uint32_t)n, words.data(), woff.data(), st.frames_per_device.data()));
    }
    st.seconds = now() - t0;
    for (size_t s = 0; s < n; s++) {
      std::vector<WordIdx> hyp(words.begin() + woff[s], words.begin() + woff[s + 1]);
      auto ref = corpus.get_word_sequence(s);
      EDAccumulator ed = editDistance(ref.first, ref.second, hyp.data(), hyp.data() + hyp.size());
      st.errors += ed;
      st.ref_words += ref.second - ref.first;
      if (ed.total_count > 0) st.sentence_errors++;
      st.hypotheses.push_back(std::move(hyp));
    }
    st.wer = 100.0 * st.errors.total_count / (double)st.ref_words;
    st.ser = 100.0 * st.sentence_errors / (double)n;
    st.rtf = st.seconds / (corpus.get_frame_duration() * (double)total);  // Recognizer.cpp:85
    return st;
  }

  // A recognised word with its frames within the segment and its confidence: the largest posterior p_t(word | X) over those
  // frames, from a forward-backward over the whole recognition network without a beam (sr_recognize_confidence_corpus).
  struct ScoredWord {
    WordIdx word;
    double confidence;
    uint32_t first_frame, last_frame;
  };
  // The words recognize() returns for each segment (same beam and word penalty), each with its confidence.  scale (kappa > 0)
  // multiplies every path cost before the sum: below 1 it flattens the posteriors (usual for confidences), at 1 they are peaked.
  std::vector<std::vector<ScoredWord>> recognize_with_confidence(Corpus const& corpus, double scale = 1.0) {
    const size_t n = std::min(corpus.get_corpus_size(), max_recognition_runs_);
    const uint64_t total = corpus.frame_offsets()[n];
    std::vector<uint32_t> words(std::max<uint64_t>(total, 1)), first(words.size()), last(words.size());
    std::vector<double> conf(words.size());
    std::vector<uint64_t> woff(n + 1);
    const sr_search_params p = search_params();
    sr_corpus* c = nullptr;
    check(sr_corpus_upload(scorer_.handle(), corpus.features(), corpus.frame_offsets(), (uint32_t)n, &c));
    const int rc = sr_recognize_confidence_corpus(scorer_.handle(), c, net_, &p, scale, words.data(), woff.data(), conf.data(),
                                                  first.data(), last.data());
    sr_corpus_destroy(c);
    check(rc);
    std::vector<std::vector<ScoredWord>> out(n);
    for (size_t s = 0; s < n; s++)
      for (uint64_t i = woff[s]; i < woff[s + 1]; i++) out[s].push_back(ScoredWord{(WordIdx)words[i], conf[i], first[i], last[i]});
    return out;
  }

  // One entry of an N-best list: a word string (silence removed) and the cost of its cheapest path through the utterance's lattice.
  struct Hypothesis {
    std::vector<WordIdx> words;
    double cost;
  };
  // Per segment the n_best cheapest distinct word strings among the paths of its word lattice (sr_word_lattice_corpus with this
  // recogniser's word penalty and no search beam, arcs within lattice_beam of the best path; sr_lattice_nbest), cheapest first.
  // Entry 0 is the unpruned decoder's result; the lattice keeps one arc per (word, end frame), so later entries are upper bounds
  // of the true k-th best cost.
  std::vector<std::vector<Hypothesis>> recognize_nbest(Corpus const& corpus, uint32_t n_best,
                                                       double lattice_beam = std::numeric_limits<double>::infinity()) {
    const size_t n = std::min(corpus.get_corpus_size(), max_recognition_runs_);
    const sr_search_params p = search_params();
    sr_corpus* c = nullptr;
    check(sr_corpus_upload(scorer_.handle(), corpus.features(), corpus.frame_offsets(), (uint32_t)n, &c));
    std::vector<uint64_t> off(n + 1);
    std::vector<double> best(std::max<size_t>(n, 1));
    int rc = sr_word_lattice_corpus(scorer_.handle(), c, net_, &p, lattice_beam, 0, off.data(), best.data(), nullptr, nullptr,
                                    nullptr, nullptr, nullptr, nullptr);
    const uint64_t cap = rc == SR_OK ? std::max<uint64_t>(off[n], 1) : 1;
    std::vector<uint32_t> word(cap), first(cap), last(cap);
    std::vector<double> fwd(cap), bwd(cap), cost(cap);
    if (rc == SR_OK)
      rc = sr_word_lattice_corpus(scorer_.handle(), c, net_, &p, lattice_beam, cap, off.data(), best.data(), word.data(),
                                  first.data(), last.data(), fwd.data(), bwd.data(), cost.data());
    sr_corpus_destroy(c);
    check(rc);
    std::vector<std::vector<Hypothesis>> out(n);
    for (size_t s = 0; s < n; s++) {
      const uint32_t T = (uint32_t)(corpus.frame_offsets()[s + 1] - corpus.frame_offsets()[s]);
      const uint64_t a = off[s], na = off[s + 1] - off[s];
      std::vector<uint32_t> words((size_t)n_best * std::max<uint32_t>(T, 1));  // (a path has at most one word per frame)
      std::vector<uint64_t> woff((size_t)n_best + 1);
      std::vector<double> costs(std::max<uint32_t>(n_best, 1));
      uint32_t count = 0;
      check(sr_lattice_nbest(T, na, word.data() + a, first.data() + a, last.data() + a, cost.data() + a,
                             (uint32_t)lexicon_.silence_idx(), n_best, words.data(), words.size(), woff.data(), costs.data(), &count));
      for (uint32_t k = 0; k < count; k++) {
        Hypothesis h;
        for (uint64_t i = woff[k]; i < woff[k + 1]; i++) h.words.push_back((WordIdx)words[i]);
        h.cost = costs[k];
        out[s].push_back(std::move(h));
      }
    }
    return out;
  }

  // Recognizer::editDistance (Recognizer.cpp:332-389), including its 16-bit counters and the stale row-0
  // insertion counter (`current_rates[0].insertion_error()` after the swap, :349-352)
  static EDAccumulator editDistance(const WordIdx* ref_begin, const WordIdx* ref_end, const WordIdx* rec_begin,
                                    const WordIdx* rec_end) {
    const size_t ref_size = ref_end - ref_begin, hyp_size = rec_end - rec_begin;
    std::vector<EDAccumulator> current(1 + ref_size), previous(1 + ref_size);
    for (size_t r = 1; r <= ref_size; r++) { current[r] = current[r - 1]; current[r].deletion_error(); }
    for (size_t h = 1; h <= hyp_size; h++) {
      current.swap(previous);
      current[0].insertion_error();
      for (size_t r = 1; r <= ref_size; r++) {
        uint16_t best = 0xFFFF;
        if (previous[r - 1].total_count < best && ref_begin[r - 1] == rec_begin[h - 1]) {
          current[r] = previous[r - 1]; best = current[r].total_count;
        }
        if (previous[r - 1].total_count + 1 < best) {
          current[r] = previous[r - 1]; current[r].substitution_error(); best = current[r].total_count;
        }
        if (previous[r].total_count + 1 < best) {
          current[r] = previous[r]; current[r].insertion_error(); best = current[r].total_count;
        }
        if (current[r - 1].total_count + 1 < best) {
          current[r] = current[r - 1]; current[r].deletion_error(); best = current[r].total_count;
        }
      }
    }
    return current[ref_size];
  }

 private:
  static double now() {
    timespec ts;
    clock_gettime(CLOCK_MONOTONIC, &ts);  // Timer.hpp:11-40
    return ts.tv_sec + 1e-9 * ts.tv_nsec;
  }
  sr_lexicon* make_net(MixtureModel& scorer) const {
    sr_lexicon* net = nullptr;
    check(sr_lexicon_create(scorer.handle(), (uint32_t)lexicon_.num_words(), word_off_.data(), automaton_.data(),
                            (uint32_t)lexicon_.silence_idx(), tdp_, silence_state_, &net));
    return net;
  }
  struct Replica {
    std::unique_ptr<MixtureModel> model;
    sr_lexicon* net = nullptr;
  };
  const double am_threshold_, word_penalty_;
  const size_t max_recognition_runs_;
  Lexicon const& lexicon_;
  MixtureModel& scorer_;
  std::vector<uint32_t> word_off_;
  std::vector<uint16_t> automaton_;
  double tdp_[3] = {0, 0, 0};
  StateIdx silence_state_ = 0;
  sr_lexicon* net_ = nullptr;
  std::vector<Replica> replicas_;
};

// ---- streaming: recognizeSequence_pruned while the frames of several utterances are still arriving (sr_stream_*, srgpu.h) --------
// begin() opens an utterance; push() hands over new frames of one or several open utterances (one scoring and one search launch
// per call); partial() is what recognizeSequence_pruned returns for the frames pushed so far; end() returns its result on the
// whole utterance and frees the id.  Errors are thrown as std::runtime_error with sr_last_error()'s text.
class FrontEnd;
class StreamingRecognizer {
 public:
  StreamingRecognizer(Lexicon const& lexicon, MixtureModel& scorer, TdpModel const& tdp_model, double am_threshold = 20.0,
                      double word_penalty = 10.0, uint32_t max_streams = 64, uint64_t max_frames = 65535)
      : max_frames_(max_frames) {
    std::vector<uint32_t> word_off(1, 0);
    std::vector<uint16_t> automaton;
    for (WordIdx w = 0; w < lexicon.num_words(); w++) {
      auto const& a = lexicon.get_automaton_for_word(w);
      automaton.insert(automaton.end(), a.states.begin(), a.states.end());
      word_off.push_back((uint32_t)automaton.size());
    }
    const double tdp[3] = {tdp_model.tdp_loop, tdp_model.tdp_forward, tdp_model.tdp_skip};
    check(sr_lexicon_create(scorer.handle(), (uint32_t)lexicon.num_words(), word_off.data(), automaton.data(),
                            (uint32_t)lexicon.silence_idx(), tdp, tdp_model.silence_state, &net_));
    sr_search_params p = sr_search_params();  // zeroed, then field by field
    p.am_threshold = am_threshold;
    p.word_penalty = word_penalty;
    p.gmm_kernel = scorer.gmm_kernel;
    const int rc = sr_stream_open(scorer.handle(), net_, &p, max_streams, max_frames, &s_);
    if (rc != SR_OK) {
      const std::string msg = sr_last_error();
      sr_lexicon_destroy(net_);
      throw std::runtime_error(msg);
    }
  }
  ~StreamingRecognizer() {
    sr_stream_destroy(s_);  // before its lexicon
    sr_lexicon_destroy(net_);
  }
  StreamingRecognizer(StreamingRecognizer const&) = delete;
  StreamingRecognizer& operator=(StreamingRecognizer const&) = delete;

  uint32_t begin() {
    uint32_t id = 0;
    check(sr_stream_begin(s_, &id));
    return id;
  }
  // n_frames new frames ([n_frames x dimension] float32) of one utterance
  void push(uint32_t id, const float* frames, size_t n_frames) {
    const uint64_t off[2] = {0, n_frames};
    check(sr_stream_push(s_, 1, &id, frames, off));
  }
  // Audio in (srgpu.h: sr_stream_push_audio): with a front end attached -- while no utterance is open; it outlives this object's
  // use of it -- an utterance takes its samples as they arrive, in pieces of any size; the rows that became ready are searched.
  // finish_audio() before end().  An utterance takes samples or frames, not both.
  void set_frontend(FrontEnd& fe);
  void push_audio(uint32_t id, const int16_t* samples, size_t n_samples) {
    const uint64_t off[2] = {0, n_samples};
    check(sr_stream_push_audio(s_, 1, &id, samples, off, nullptr, 0, nullptr));
  }
  void finish_audio(uint32_t id) { check(sr_stream_finish_audio(s_, 1, &id, nullptr, 0, nullptr)); }
  // the utterance's VTLN warp (srgpu.h: sr_stream_set_warp): an index into the attached warped front end's warps, SR_STREAM_NO_WARP
  // clears it; between begin() and the utterance's first push.  Its rows are then FrontEnd::from_audio_warped's under that warp.
  void set_warp(uint32_t id, uint32_t warp) { check(sr_stream_set_warp(s_, id, warp)); }
  // The pipeline (srgpu.h: sr_stream_set_projection): rows of in_dim columns are spliced with `context` neighbours on either side and
  // projected by M [dimension x ((2 context + 1) in_dim + 1)] (nullptr detaches; while no utterance is open), then the utterance's
  // W [dimension x (dimension + 1)] (nullptr clears it; between begin() and its first push) is applied, on the device.  push_rows:
  // n_frames rows of one utterance, in_dim columns with a projection; finish: no more follow, its last `context` rows are searched.
  void set_projection(uint32_t in_dim, uint32_t context, const double* M) { check(sr_stream_set_projection(s_, in_dim, context, M)); }
  void set_transform(uint32_t id, const double* W) { check(sr_stream_set_transform(s_, id, W)); }
  void push_rows(uint32_t id, const float* frames, size_t n_frames, bool finish = false) {
    const uint64_t off[2] = {0, n_frames};
    check(sr_stream_push_rows(s_, 1, &id, frames, off, finish ? 1 : 0, nullptr, 0, nullptr));
  }
  // new frames of several utterances back to back: ids[i] owns rows [frame_off[i], frame_off[i+1])
  void push(std::vector<uint32_t> const& ids, const float* frames, std::vector<uint64_t> const& frame_off) {
    if (frame_off.size() != ids.size() + 1) throw std::runtime_error("StreamingRecognizer::push: frame_off needs ids.size() + 1 entries");
    check(sr_stream_push(s_, (uint32_t)ids.size(), ids.data(), frames, frame_off.data()));
  }
  // (a trimmed utterance can hold more words than max_frames: a call that reports too small a buffer says how many it needs)
  std::vector<WordIdx> partial(uint32_t id) {
    std::vector<uint32_t> w(max_frames_);
    uint32_t n = 0;
    int rc = sr_stream_partial(s_, id, w.data(), (uint32_t)w.size(), &n, nullptr);
    if (rc == SR_EINVAL && n > w.size()) {
      w.resize(n);
      rc = sr_stream_partial(s_, id, w.data(), (uint32_t)w.size(), &n, nullptr);
    }
    check(rc);
    return std::vector<WordIdx>(w.begin(), w.begin() + n);
  }
  // the leading words of partial(id) that no later frame can change (sr_stream_stable): a prefix of every later partial() and of
  // end() whose traceback entry is finite.  *commit (may be null): the frame they end at; *trailing_silence (may be null): the frames
  // the best hypothesis has spent in silence at the end -- an endpointer calls end() once it passes its threshold
  std::vector<WordIdx> stable(uint32_t id, uint32_t* commit = nullptr, uint32_t* trailing_silence = nullptr) {
    std::vector<uint32_t> w(max_frames_);
    uint64_t off[2] = {0, 0};
    uint32_t c = 0, sil = 0;
    int rc = sr_stream_stable(s_, 1, &id, w.data(), w.size(), off, &c, &sil);
    if (rc == SR_EINVAL && off[1] > w.size()) {
      w.resize(off[1]);
      rc = sr_stream_stable(s_, 1, &id, w.data(), w.size(), off, &c, &sil);
    }
    check(rc);
    if (commit) *commit = c;
    if (trailing_silence) *trailing_silence = sil;
    return std::vector<WordIdx>(w.begin(), w.begin() + off[1]);
  }
  // Drops the frames of the utterance up to its commit point on the device and keeps their words on the host (sr_stream_trim):
  // max_frames then bounds the frames since, not the utterance, which can go on without limit when it is trimmed every few pushes.
  // partial(), stable() and end() still report the whole utterance.  -> the frames dropped (0: the commit point has not moved)
  uint32_t trim(uint32_t id) {
    uint32_t dropped = 0;
    check(sr_stream_trim(s_, 1, &id, &dropped));
    return dropped;
  }
  std::vector<uint32_t> trim(std::vector<uint32_t> const& ids) {
    std::vector<uint32_t> dropped(ids.size(), 0);
    check(sr_stream_trim(s_, (uint32_t)ids.size(), ids.data(), dropped.data()));
    return dropped;
  }
  std::vector<WordIdx> end(uint32_t id) {
    std::vector<uint32_t> w(max_frames_);
    uint32_t n = 0;
    int rc = sr_stream_end(s_, id, w.data(), (uint32_t)w.size(), &n, nullptr, nullptr, nullptr);
    if (rc == SR_EINVAL && n > w.size()) {  // (the id is still open)
      w.resize(n);
      rc = sr_stream_end(s_, id, w.data(), (uint32_t)w.size(), &n, nullptr, nullptr, nullptr);
    }
    check(rc);
    return std::vector<WordIdx>(w.begin(), w.begin() + n);
  }

 private:
  const uint64_t max_frames_;
  sr_lexicon* net_ = nullptr;
  sr_stream* s_ = nullptr;
};

// ---- Alignment.hpp:19-63 -------------------------------------------------------------------------------------
struct AlignmentItem {  // sietill/Types.hpp:29-38
  uint16_t count = 0;
  StateIdx state = 0;
  float weight = 0.0f;
};

class Aligner {
 public:
  Aligner(MixtureModel& mixtures, TdpModel const& tdp_model) : mixtures_(mixtures), tdp_(tdp_model) {}

  // Aligner::align_sequence_full (Alignment.cpp:50-144); alignment receives one item per frame
  double align_sequence_full(const float* feature_begin, size_t n_frames, MarkovAutomaton const& reference,
                             std::vector<AlignmentItem>& alignment) {
    return run(feature_begin, n_frames, reference, alignment, false, 0.0);
  }
  // Aligner::align_sequence_pruned (Alignment.cpp:149-288)
  double align_sequence_pruned(const float* feature_begin, size_t n_frames, MarkovAutomaton const& reference,
                               std::vector<AlignmentItem>& alignment, double pruning_threshold) {
    return run(feature_begin, n_frames, reference, alignment, true, pruning_threshold);
  }

 private:
  double run(const float* feats, size_t T, MarkovAutomaton const& ref, std::vector<AlignmentItem>& alignment, bool pruned,
             double thr) {
    const uint64_t foff[2] = {0, T}, aoff[2] = {0, ref.num_states()};
    const double tdp[3] = {tdp_.tdp_loop, tdp_.tdp_forward, tdp_.tdp_skip};
    sr_corpus* c = nullptr;
    check(sr_corpus_upload(mixtures_.handle(), feats, foff, 1, &c));
    std::vector<uint16_t> states(std::max<size_t>(T, 1));
    double cost = 0.0;
    const int rc = pruned ? sr_align_corpus_pruned(mixtures_.handle(), c, ref.states.data(), aoff, tdp, tdp_.silence_state, thr,
                                                   mixtures_.gmm_kernel, states.data(), &cost)
                          : sr_align_corpus(mixtures_.handle(), c, ref.states.data(), aoff, tdp, tdp_.silence_state,
                                            mixtures_.gmm_kernel, states.data(), &cost);
    sr_corpus_destroy(c);
    check(rc);
    alignment.assign(T, AlignmentItem());
    for (size_t t = 0; t < T; t++) { alignment[t].state = states[t]; alignment[t].weight = 1; alignment[t].count = 1; }
    return cost;
  }
  MixtureModel& mixtures_;
  TdpModel tdp_;
};

// ---- on-disk formats either side of the path ------------------------------------------
// `<feature-path><name>.mm2`: raw little-endian float32, n-features-file values per frame (IO.cpp:48-69)
inline std::vector<float> read_feature_file(std::string const& path) {
  std::vector<float> features;
  std::ifstream in(path.c_str(), std::ios_base::in | std::ios_base::binary);
  if (!in.good()) return features;  // the reference prints an error and returns an empty vector (IO.cpp:52-55)
  in.seekg(0, std::ios_base::end);
  const std::streamoff bytes = in.tellg();
  in.seekg(0);
  features.resize((size_t)bytes / sizeof(float));
  in.read(reinterpret_cast<char*>(features.data()), features.size() * sizeof(float));
  return features;
}

// What Corpus::read applies to every utterance (Corpus.cpp:101-102): static features -> static | delta | delta-delta,
// optional mean/variance normalisation (computed in double, stored as float) and per-utterance maximum
// normalisation of component 0 (SignalAnalysis.cpp:379-399, :320-336, :340-349).
struct FeaturePostProcessor {
  size_t n_features_in_file = 12, n_features_first = 12, n_features_second = 1, deriv_step = 3;  // SignalAnalysis.cpp:53-56
  bool energy_max_norm = true;                                                                   // :46
  std::vector<double> mean, stddev;  // empty: no mean/variance normalisation
  size_t n_features_total() const { return n_features_in_file + n_features_first + n_features_second; }

  // normalisation file: n_features_total f64 means then as many f64 standard deviations (SignalAnalysis.cpp:364-375)
  bool read_normalization_file(std::string const& path) {
    std::ifstream in(path.c_str(), std::ios_base::in | std::ios_base::binary);
    if (!in.good()) return false;
    mean.resize(n_features_total());
    stddev.resize(n_features_total());
    in.read(reinterpret_cast<char*>(mean.data()), sizeof(double) * mean.size());
    in.read(reinterpret_cast<char*>(stddev.data()), sizeof(double) * stddev.size());
    return (bool)in;
  }

  void process_features(std::vector<float>& features) const {
    const size_t nf = n_features_in_file, nt = n_features_total(), T = features.size() / nf;
    std::vector<float> seq(T * nt, 0.0f);
    for (size_t f = 0; f < T; f++) std::copy(features.begin() + f * nf, features.begin() + (f + 1) * nf, seq.begin() + f * nt);
    // An utterance of at most deriv_step frames: the reference indexes frame max(t, deriv_step) >= T and frame
    // T - 1 - deriv_step (size_t underflow) -- reads past its buffer, results undefined (found by tools/sanitize_host.py; the
    // corpus has no such utterance).  Here both windows are clamped into [0, T - 1] instead; for T > deriv_step the indices
    // below are exactly the reference's.
    for (size_t t = 0; t < T; t++) {  // first derivative, window clamped at the start (:322-328)
      const size_t a = std::min(std::max(t, deriv_step), T - 1), b = a >= deriv_step ? a - deriv_step : 0;
      for (size_t k = 0; k < n_features_first; k++) seq[t * nt + nf + k] = seq[a * nt + k] - seq[b * nt + k];
    }
    for (size_t t = 0; t < T; t++) {  // second derivative from the first, window clamped at the end (:329-335)
      const size_t a = T > deriv_step ? std::min(t, T - 1 - deriv_step) + deriv_step : T - 1;
      for (size_t k = 0; k < n_features_second; k++) seq[t * nt + nf + n_features_first + k] = seq[a * nt + nf + k] - seq[t * nt + nf + k];
    }
    if (!mean.empty()) {
      for (size_t t = 0; t < T; t++) {
        for (size_t k = 0; k < nt; k++) seq[t * nt + k] = (float)((double)seq[t * nt + k] - mean[k]);
        for (size_t k = 0; k < nt; k++) seq[t * nt + k] = (float)((double)seq[t * nt + k] / stddev[k]);
      }
    }
    if (energy_max_norm) {
      float mx = -std::numeric_limits<float>::infinity();
      for (size_t t = 0; t < T; t++) mx = std::max(mx, seq[t * nt]);
      for (size_t t = 0; t < T; t++) seq[t * nt] -= mx;
    }
    features.swap(seq);
  }

  // srgpu.h's view of this configuration (mean / stddev point into this object)
  sr_feature_post_params params() const {
    sr_feature_post_params q{};
    q.n_static = (uint32_t)n_features_in_file; q.n_first = (uint32_t)n_features_first; q.n_second = (uint32_t)n_features_second;
    q.deriv_step = (uint32_t)deriv_step;
    q.energy_max_norm = energy_max_norm ? 1 : 0;
    q.mean = mean.empty() ? nullptr : mean.data();
    q.stddev = mean.empty() ? nullptr : stddev.data();
    return q;
  }

  // The corpus that process_features on every utterance and sr_corpus_upload would give, bit for bit, made on the device from the
  // static features [frames x n_features_in_file] (sr_corpus_from_cepstra).  Destroyed before `model`.
  std::shared_ptr<sr_corpus> device_corpus(sr_model* model, const float* cepstra, const uint64_t* frame_off, uint32_t n_utts) const {
    const sr_feature_post_params q = params();
    sr_frontend* fe = nullptr;
    check(sr_frontend_create(model, nullptr, &q, &fe));
    std::shared_ptr<sr_frontend> own(fe, sr_frontend_destroy);
    sr_corpus* c = nullptr;
    check(sr_corpus_from_cepstra(fe, cepstra, frame_off, n_utts, &c));
    return std::shared_ptr<sr_corpus>(c, sr_corpus_destroy);
  }
};

// ---- the audio front end on the device (srgpu.h: sr_frontend_*): SignalAnalysis' MFCC stage as srgpu.h defines it, then
// FeaturePostProcessor's stage bit for bit.  Samples or static features in, a resident corpus of `model` out; every corpus is
// destroyed before the model, and so is this object.
class FrontEnd {
 public:
  FrontEnd(sr_model* model, sr_mfcc_params const& mfcc, FeaturePostProcessor const& post) {
    const sr_feature_post_params q = post.params();
    sr_frontend* fe = nullptr;
    check(sr_frontend_create(model, &mfcc, &q, &fe));
    fe_.reset(fe, sr_frontend_destroy);
    n_static_ = q.n_static;
  }
  // a warped front end (srgpu.h: sr_frontend_create_warped): a filterbank per warp factor beside the unwarped one
  FrontEnd(sr_model* model, sr_mfcc_params const& mfcc, std::vector<double> const& alpha, double break_frac, FeaturePostProcessor const& post) {
    const sr_feature_post_params q = post.params();
    sr_vtln_params v{};
    v.n_warps = (uint32_t)alpha.size(); v.alpha = alpha.data(); v.break_frac = break_frac;
    sr_frontend* fe = nullptr;
    check(sr_frontend_create_warped(model, &mfcc, &v, &q, &fe));
    fe_.reset(fe, sr_frontend_destroy);
    n_static_ = q.n_static;
    n_warps_ = v.n_warps;
  }
  uint32_t n_warps() const { return n_warps_; }
  // the chunks of warps vtln_costs takes for that many frames and utterances (sr_vtln_chunks)
  uint32_t vtln_chunks(uint64_t n_frames, uint32_t n_utts) const {
    uint32_t n = 0;
    check(sr_vtln_chunks(fe_.get(), n_frames, n_utts, &n));
    return n;
  }
  // both stages, utterance u through the filters of warp utt_warp[u]
  std::shared_ptr<sr_corpus> from_audio_warped(std::vector<int16_t> const& samples, std::vector<uint64_t> const& sample_off,
                                               std::vector<uint32_t> const& utt_warp, std::vector<uint64_t>& frame_off) {
    frame_off.assign(sample_off.size(), 0);
    sr_corpus* c = nullptr;
    check(sr_corpus_from_audio_warped(fe_.get(), samples.data(), sample_off.data(), (uint32_t)sample_off.size() - 1, utt_warp.data(), &c,
                                      frame_off.data()));
    return std::shared_ptr<sr_corpus>(c, sr_corpus_destroy);
  }
  // the warp search: cost [n_speakers x n_warps] of the speakers' utterances along `states`, an alignment of the unwarped corpus;
  // frames [n_speakers].  Smaller is better; no Jacobian term.
  void vtln_costs(std::vector<int16_t> const& samples, std::vector<uint64_t> const& sample_off, std::vector<uint16_t> const& states,
                  std::vector<uint32_t> const& utt_speaker, uint32_t n_speakers, std::vector<double>& cost, std::vector<uint64_t>& frames) {
    cost.assign((size_t)n_speakers * n_warps_, 0.0);
    frames.assign(n_speakers, 0);
    check(sr_vtln_costs_corpus(fe_.get(), samples.data(), sample_off.data(), (uint32_t)sample_off.size() - 1, states.data(), utt_speaker.data(),
                               n_speakers, cost.data(), frames.data()));
  }
  uint64_t frames(uint64_t n_samples) const {
    uint64_t T = 0;
    check(sr_frontend_frames(fe_.get(), n_samples, &T));
    return T;
  }
  // both stages; frame_off [n_utts + 1] receives the corpus's frame offsets
  std::shared_ptr<sr_corpus> from_audio(std::vector<int16_t> const& samples, std::vector<uint64_t> const& sample_off,
                                        std::vector<uint64_t>& frame_off) {
    frame_off.assign(sample_off.size(), 0);
    sr_corpus* c = nullptr;
    check(sr_corpus_from_audio(fe_.get(), samples.data(), sample_off.data(), (uint32_t)sample_off.size() - 1, &c, frame_off.data()));
    return std::shared_ptr<sr_corpus>(c, sr_corpus_destroy);
  }
  std::shared_ptr<sr_corpus> from_cepstra(std::vector<float> const& cepstra, std::vector<uint64_t> const& frame_off) {
    sr_corpus* c = nullptr;
    check(sr_corpus_from_cepstra(fe_.get(), cepstra.data(), frame_off.data(), (uint32_t)frame_off.size() - 1, &c));
    return std::shared_ptr<sr_corpus>(c, sr_corpus_destroy);
  }
  // the MFCC stage alone: the static features [frames x n_cepstra], what read_feature_file reads from an .mm2 file
  std::vector<float> mfcc(std::vector<int16_t> const& samples, std::vector<uint64_t> const& sample_off, std::vector<uint64_t>& frame_off) {
    uint64_t total = 0;
    for (size_t u = 0; u + 1 < sample_off.size(); u++) total += frames(sample_off[u + 1] - sample_off[u]);
    std::vector<float> out((size_t)total * n_static_);
    frame_off.assign(sample_off.size(), 0);
    check(sr_mfcc_corpus(fe_.get(), samples.data(), sample_off.data(), (uint32_t)sample_off.size() - 1, out.data(), frame_off.data()));
    return out;
  }
  // a resident corpus's features [frames x dim] (sr_corpus_download)
  static std::vector<float> download(sr_corpus* c, uint64_t n_frames, uint32_t dim) {
    std::vector<float> out((size_t)n_frames * dim);
    check(sr_corpus_download(c, out.data()));
    return out;
  }
  sr_frontend* handle() const { return fe_.get(); }

 private:
  std::shared_ptr<sr_frontend> fe_;
  uint32_t n_static_ = 0, n_warps_ = 0;
};

// per speaker the first warp of smallest cost; `fallback` for fewer than min_frames frames or costs that are not finite (sr_vtln_choose)
inline std::vector<uint32_t> vtln_choose(std::vector<double> const& cost, std::vector<uint64_t> const& frames, uint32_t n_warps,
                                         uint64_t min_frames, uint32_t fallback) {
  std::vector<uint32_t> out(frames.size(), fallback);
  check(sr_vtln_choose((uint32_t)frames.size(), n_warps, cost.data(), frames.data(), min_frames, fallback, out.data()));
  return out;
}

inline void StreamingRecognizer::set_frontend(FrontEnd& fe) { check(sr_stream_set_frontend(s_, fe.handle())); }

// alignment dump: size_t max_aligns; size_t num_frames; AlignmentItem[num_frames * max_aligns] (Alignment.cpp:303-318)
inline void write_alignment(std::ostream& out, std::vector<AlignmentItem> const& alignment, size_t max_aligns) {
  const size_t num_frames = alignment.size() / max_aligns;
  out.write(reinterpret_cast<const char*>(&max_aligns), sizeof max_aligns);
  out.write(reinterpret_cast<const char*>(&num_frames), sizeof num_frames);
  out.write(reinterpret_cast<const char*>(alignment.data()), max_aligns * num_frames * sizeof(AlignmentItem));
}
inline void read_alignment(std::istream& in, std::vector<AlignmentItem>& alignment, size_t& max_aligns) {
  size_t num_frames = 0;
  in.read(reinterpret_cast<char*>(&max_aligns), sizeof max_aligns);
  in.read(reinterpret_cast<char*>(&num_frames), sizeof num_frames);
  alignment.resize(num_frames * max_aligns);
  in.read(reinterpret_cast<char*>(alignment.data()), max_aligns * num_frames * sizeof(AlignmentItem));
}

// ---- the training-side callers of the path (Training.hpp:18-107): NOT the EM trainer, only the two loops of
// Trainer::train that run the scorer and the aligner over the whole corpus -- re-alignment (Training.cpp:163-184)
// and the average acoustic score along the alignment (calc_am_score, :585-612) -- each as one device pass; and the
// Baum-Welch E-step that can take re-alignment's and accumulation's place (baum_welch).
class Trainer {
 public:
  Trainer(Lexicon const& lexicon, MixtureModel& mixtures, TdpModel const& tdp_model, double pruning_threshold = 50.0,
          bool alignment_pruning = true)
      : pruning_threshold_(pruning_threshold), alignment_pruning_(alignment_pruning), lexicon_(lexicon),
        mixtures_(mixtures), tdp_(tdp_model) {}

  // Trainer::build_segment_automaton (Training.cpp:238-253): sil w1 sil w2 ... sil
  MarkovAutomaton build_segment_automaton(const WordIdx* segment_begin, const WordIdx* segment_end) const {
    std::vector<MarkovAutomaton const*> automata;
    for (const WordIdx* it = segment_begin; it != segment_end; ++it) {
      automata.push_back(&lexicon_.get_silence_automaton());
      automata.push_back(&lexicon_.get_automaton_for_word(*it));
    }
    automata.push_back(&lexicon_.get_silence_automaton());
    return MarkovAutomaton::concat(automata);
  }

  // the re-alignment loop of Trainer::train (Training.cpp:163-184) over every segment of the corpus;
  // alignment gets one item per corpus frame, costs (optional) the per-segment path costs
  void realign(Corpus const& corpus, std::vector<AlignmentItem>& alignment, std::vector<double>* costs = nullptr) {
    const size_t n = corpus.get_corpus_size();
    std::vector<uint16_t> automata;
    std::vector<uint64_t> aut_off;
    segment_automata(corpus, automata, aut_off);
    const uint64_t F = corpus.get_total_frame_count();
    std::vector<uint16_t> states;
    std::vector<double> cost;
    align_states(mixtures_.handle(), corpus, automata, aut_off, states, cost);
    alignment.assign(F, AlignmentItem());
    for (uint64_t t = 0; t < F; t++) { alignment[t].state = states[t]; alignment[t].weight = 1; alignment[t].count = 1; }
    if (costs) costs->assign(cost.begin(), cost.begin() + n);
  }

  // MixtureModel's accumulators (Mixtures.hpp:80-86) as sr_accumulate_corpus / sr_baum_welch_corpus return them
  struct Statistics {
    std::vector<double> mean_acc, mean_w, var_acc, var_w;
  };

  // Baum-Welch in place of Viterbi training: one device pass does the forward-backward over every segment's automaton and the
  // posterior-weighted accumulation (sr_baum_welch_corpus) -- what realign + MixtureModel::accumulate do in Trainer::train, with
  // every frame shared among the states by its posterior instead of one hard decision.  costs (optional): the per-segment
  // -log P(X | transcript), the quantity EM lowers.  Memberships within a state follow the model (arg-min with max-approx
  // scoring, soft otherwise); posteriors below posterior_floor are dropped.
  void baum_welch(Corpus const& corpus, Statistics& stats, std::vector<double>* costs = nullptr, double posterior_floor = 0.0,
                  bool first_pass = false) {
    const size_t n = corpus.get_corpus_size();
    std::vector<uint16_t> automata;
    std::vector<uint64_t> aut_off;
    segment_automata(corpus, automata, aut_off);
    uint32_t n_mean = 0, n_var = 0;
    check(sr_model_tying_info(mixtures_.handle(), &n_mean, &n_var));
    const size_t D = mixtures_.dimension;
    stats.mean_acc.assign(n_mean * D, 0.0); stats.mean_w.assign(n_mean, 0.0);
    stats.var_acc.assign(n_var * D, 0.0); stats.var_w.assign(n_var, 0.0);
    const double tdp[3] = {tdp_.tdp_loop, tdp_.tdp_forward, tdp_.tdp_skip};
    sr_corpus* c = nullptr;
    check(sr_corpus_upload(mixtures_.handle(), corpus.features(), corpus.frame_offsets(), (uint32_t)n, &c));
    std::vector<double> cost(std::max<size_t>(n, 1));
    const int rc = sr_baum_welch_corpus(mixtures_.handle(), c, automata.data(), aut_off.data(), tdp, tdp_.silence_state,
                                        mixtures_.gmm_kernel, posterior_floor, first_pass ? 1 : 0, mixtures_.max_approx() ? 1 : 0,
                                        cost.data(), stats.mean_acc.data(), stats.mean_w.data(), stats.var_acc.data(),
                                        stats.var_w.data());
    sr_corpus_destroy(c);
    check(rc);
    if (costs) costs->assign(cost.begin(), cost.begin() + n);
  }

  // One iteration of MMI training (sr_mmi_statistics_corpus + sr_model_create_from_mmi_statistics): the numerator over the recognition
  // network restricted to each segment's transcript (lexicon word ids, silence not listed; silence must be word 0), the denominator
  // over the free network, every cost multiplied by scale (kappa); then the extended Baum-Welch update of means and variances with
  // smoothing constant E per density (D = E x denominator count, at least what keeps the variances above var_floor) and I-smoothing
  // tau.  Returns the next model -- mixture weights unchanged -- and sets *objective (optional) to sum(F_num - F_den) >= 0 under the
  // CURRENT model over the segments with a path through their transcript: the quantity the iteration lowers.
  std::unique_ptr<MixtureModel> mmi_iteration(Corpus const& corpus, std::vector<std::vector<WordIdx>> const& transcripts, double scale,
                                              double E, double tau, double* objective = nullptr, double word_penalty = 0.0,
                                              double posterior_floor = 0.0, double var_floor = 1e-6) {
    const size_t n = corpus.get_corpus_size();
    if (transcripts.size() != n) throw std::invalid_argument("mmi_iteration: one transcript per segment");
    std::vector<uint32_t> word_off(1, 0), trans(1, 0);
    std::vector<uint16_t> automaton;
    for (WordIdx w = 0; w < lexicon_.num_words(); w++) {
      auto const& a = lexicon_.get_automaton_for_word(w);
      automaton.insert(automaton.end(), a.states.begin(), a.states.end());
      word_off.push_back((uint32_t)automaton.size());
    }
    std::vector<uint64_t> trans_off(1, 0);
    trans.clear();
    for (auto const& t : transcripts) {
      trans.insert(trans.end(), t.begin(), t.end());
      trans_off.push_back(trans.size());
    }
    trans.push_back(0);  // (never empty: the ABI tells "no transcripts" by a null pointer)
    uint32_t n_mean = 0, n_var = 0;
    check(sr_model_tying_info(mixtures_.handle(), &n_mean, &n_var));
    const size_t D = mixtures_.dimension;
    Statistics num, den;
    for (Statistics* st : {&num, &den}) {
      st->mean_acc.assign(n_mean * D, 0.0); st->mean_w.assign(n_mean, 0.0);
      st->var_acc.assign(n_var * D, 0.0); st->var_w.assign(n_var, 0.0);
    }
    const double tdp[3] = {tdp_.tdp_loop, tdp_.tdp_forward, tdp_.tdp_skip};
    sr_lexicon* net = nullptr;
    check(sr_lexicon_create(mixtures_.handle(), (uint32_t)lexicon_.num_words(), word_off.data(), automaton.data(),
                            (uint32_t)lexicon_.silence_idx(), tdp, tdp_.silence_state, &net));
    sr_corpus* c = nullptr;
    int rc = sr_corpus_upload(mixtures_.handle(), corpus.features(), corpus.frame_offsets(), (uint32_t)n, &c);
    std::vector<double> f_num(std::max<size_t>(n, 1)), f_den(std::max<size_t>(n, 1));
    if (rc == SR_OK) {
      sr_search_params p = sr_search_params();  // zeroed, then field by field: a field added to the struct cannot shift these
      p.word_penalty = word_penalty;
      p.gmm_kernel = mixtures_.gmm_kernel;
      rc = sr_mmi_statistics_corpus(mixtures_.handle(), c, net, &p, scale, posterior_floor, mixtures_.max_approx() ? 1 : 0, trans.data(),
                                    trans_off.data(), f_num.data(), f_den.data(), num.mean_acc.data(), num.mean_w.data(),
                                    num.var_acc.data(), num.var_w.data(), den.mean_acc.data(), den.mean_w.data(), den.var_acc.data(),
                                    den.var_w.data());
      sr_corpus_destroy(c);
    }
    sr_lexicon_destroy(net);
    check(rc);
    if (objective) {
      *objective = 0.0;
      for (size_t u = 0; u < n; u++)
        if (f_num[u] < std::numeric_limits<double>::infinity()) *objective += f_num[u] - f_den[u];
    }
    sr_model* next = nullptr;
    check(sr_model_create_from_mmi_statistics(mixtures_.handle(), num.mean_acc.data(), num.mean_w.data(), num.var_acc.data(),
                                              num.var_w.data(), den.mean_acc.data(), den.mean_w.data(), den.var_acc.data(),
                                              den.var_w.data(), E, tau, var_floor, &next));
    return std::unique_ptr<MixtureModel>(new MixtureModel(next, mixtures_));
  }

  // One iteration of sMBR training (sr_smbr_statistics_corpus + sr_model_create_from_mmi_statistics): the expected frame accuracy of
  // the free recognition network against the alignment's mixtures (one AlignmentItem per frame of the corpus, as align() leaves
  // them), every cost multiplied by scale (kappa); the positive weights are the numerator's statistics, the negative ones the
  // denominator's, then the extended Baum-Welch update as in mmi_iteration.  Returns the next model and sets *expected_correct
  // (optional) to the sum of the expected accuracies under the CURRENT model -- the quantity the iteration raises -- and *n_frames
  // (optional) to the frame count it is out of.
  std::unique_ptr<MixtureModel> smbr_iteration(Corpus const& corpus, std::vector<AlignmentItem> const& alignment, double scale, double E,
                                               double tau, double* expected_correct = nullptr, uint64_t* n_frames = nullptr,
                                               double word_penalty = 0.0, double posterior_floor = 0.0, double var_floor = 1e-6) {
    const size_t n = corpus.get_corpus_size();
    const uint64_t F = corpus.get_total_frame_count();
    if (alignment.size() < F) throw std::invalid_argument("smbr_iteration: one alignment item per frame");
    std::vector<uint16_t> ref(std::max<uint64_t>(F, 1));
    for (uint64_t t = 0; t < F; t++) ref[t] = alignment[t].state;
    std::vector<uint32_t> word_off(1, 0);
    std::vector<uint16_t> automaton;
    for (WordIdx w = 0; w < lexicon_.num_words(); w++) {
      auto const& a = lexicon_.get_automaton_for_word(w);
      automaton.insert(automaton.end(), a.states.begin(), a.states.end());
      word_off.push_back((uint32_t)automaton.size());
    }
    uint32_t n_mean = 0, n_var = 0;
    check(sr_model_tying_info(mixtures_.handle(), &n_mean, &n_var));
    const size_t D = mixtures_.dimension;
    Statistics num, den;
    for (Statistics* st : {&num, &den}) {
      st->mean_acc.assign(n_mean * D, 0.0); st->mean_w.assign(n_mean, 0.0);
      st->var_acc.assign(n_var * D, 0.0); st->var_w.assign(n_var, 0.0);
    }
    const double tdp[3] = {tdp_.tdp_loop, tdp_.tdp_forward, tdp_.tdp_skip};
    sr_lexicon* net = nullptr;
    check(sr_lexicon_create(mixtures_.handle(), (uint32_t)lexicon_.num_words(), word_off.data(), automaton.data(),
                            (uint32_t)lexicon_.silence_idx(), tdp, tdp_.silence_state, &net));
    sr_corpus* c = nullptr;
    int rc = sr_corpus_upload(mixtures_.handle(), corpus.features(), corpus.frame_offsets(), (uint32_t)n, &c);
    std::vector<double> cost(std::max<size_t>(n, 1)), acc(std::max<size_t>(n, 1));
    if (rc == SR_OK) {
      sr_search_params p = sr_search_params();  // zeroed, then field by field: a field added to the struct cannot shift these
      p.word_penalty = word_penalty;
      p.gmm_kernel = mixtures_.gmm_kernel;
      rc = sr_smbr_statistics_corpus(mixtures_.handle(), c, net, &p, scale, posterior_floor, mixtures_.max_approx() ? 1 : 0, ref.data(),
                                     cost.data(), acc.data(), num.mean_acc.data(), num.mean_w.data(), num.var_acc.data(),
                                     num.var_w.data(), den.mean_acc.data(), den.mean_w.data(), den.var_acc.data(), den.var_w.data());
      sr_corpus_destroy(c);
    }
    sr_lexicon_destroy(net);
    check(rc);
    if (expected_correct) {
      *expected_correct = 0.0;
      for (size_t u = 0; u < n; u++) *expected_correct += acc[u];
    }
    if (n_frames) *n_frames = F;
    sr_model* next = nullptr;
    check(sr_model_create_from_mmi_statistics(mixtures_.handle(), num.mean_acc.data(), num.mean_w.data(), num.var_acc.data(),
                                              num.var_w.data(), den.mean_acc.data(), den.mean_w.data(), den.var_acc.data(),
                                              den.var_w.data(), E, tau, var_floor, &next));
    return std::unique_ptr<MixtureModel>(new MixtureModel(next, mixtures_));
  }

  // MixtureModel::split / eliminate in the schedule of Trainer::train (sr_model_split, sr_model_eliminate: the operations srgpu.h
  // specifies, not the reference's bits).  The weights are the per mean row observation counts of the last E-step: Statistics::mean_w,
  // or a corpus handle of this model in which sr_accumulate_corpus / sr_baum_welch_corpus left its statistics.  Variance rows follow
  // the model's var_model.  The result is a model of a new shape; this trainer keeps pointing at the old one.
  std::unique_ptr<MixtureModel> split(std::vector<double> const& mean_w, double min_obs, double epsilon) {
    return split_of(mixtures_.handle(), nullptr, checked_weights(mixtures_.handle(), mean_w), min_obs, epsilon);
  }
  std::unique_ptr<MixtureModel> split(sr_corpus* resident, double min_obs, double epsilon) {
    return split_of(mixtures_.handle(), resident, nullptr, min_obs, epsilon);
  }
  std::unique_ptr<MixtureModel> eliminate(std::vector<double> const& mean_w, double min_obs) {
    return eliminate_of(mixtures_.handle(), nullptr, checked_weights(mixtures_.handle(), mean_w), min_obs);
  }
  std::unique_ptr<MixtureModel> eliminate(sr_corpus* resident, double min_obs) {
    return eliminate_of(mixtures_.handle(), resident, nullptr, min_obs);
  }

  // Trainer::train's schedule (Training.cpp:44-235): from the trainer's model -- normally the flat start MixtureModel(dimension,
  // num_mixtures, ...) -- to a model of up to 2^num_splits densities per mixture.
  //   1. linear segmentation: every segment's `sil w1 sil ... sil` automaton, frame t of T at position t * N / T of its N positions
  //      (equal shares; our own variant of the reference's first alignment)
  //   2. accumulate(first_pass) / finalize
  //   3. per split: split / accumulate / finalize / eliminate / accumulate / finalize
  //   4. per alignment round: re-alignment (realign's aligner), then num_estimates x accumulate / finalize
  // After every finalize the average AM score along the current alignment (calc_am_score) is recorded.  The statistics of every pass
  // come to the host (sr_accumulate_corpus with its four arrays): the split and the eliminate that follow a finalize need the mean
  // weights of the pass before it, and a corpus handle belongs to the model it was uploaded for, so every new model gets its own upload.
  struct TrainSchedule {
    uint32_t num_splits = 0, num_aligns = 0, num_estimates = 1;
    double min_obs = 0.0;    // a density splits / survives with at least this many observations
    double epsilon = 0.2;    // children sit epsilon standard deviations either side of the parent
    MixtureModel::VarianceModel pooling = MixtureModel::NO_POOLING;
    bool max_approx = true;
  };
  struct TrainResult {
    std::unique_ptr<MixtureModel> model;
    std::vector<double> am_scores;            // after every finalize, in order
    std::vector<AlignmentItem> alignment;     // the last alignment
  };
  TrainResult train(Corpus const& corpus, TrainSchedule const& sch) {
    const size_t n = corpus.get_corpus_size();
    const uint64_t F = corpus.get_total_frame_count();
    std::vector<uint16_t> automata, states(std::max<uint64_t>(F, 1));
    std::vector<uint64_t> aut_off;
    segment_automata(corpus, automata, aut_off);
    for (size_t u = 0; u < n; u++) {  // 1. linear segmentation
      const uint64_t f0 = corpus.frame_offsets()[u], T = corpus.frame_offsets()[u + 1] - f0, N = aut_off[u + 1] - aut_off[u];
      for (uint64_t t = 0; t < T; t++) states[f0 + t] = automata[aut_off[u] + t * N / T];
    }
    TrainResult r;
    typedef std::unique_ptr<sr_model, int (*)(sr_model*)> Owned;
    Owned cur(nullptr, sr_model_destroy);
    sr_model* h = mixtures_.handle();
    Statistics st;
    // accumulate on h / finalize -> cur (and h), the AM score of the new model recorded
    auto estimate = [&](bool first_pass) {
      accumulate_on(h, corpus, states, first_pass, sch.max_approx, st);
      uint32_t d = 0, S = 0, n_mean = 0, n_var = 0;
      uint64_t C = 0;
      check(sr_model_info(h, &d, &S, &C));
      check(sr_model_tying_info(h, &n_mean, &n_var));
      std::vector<uint32_t> off(S + 1), dm(std::max<uint64_t>(C, 1)), dv(std::max<uint64_t>(C, 1));
      check(sr_model_topology(h, off.data(), dm.data(), dv.data()));
      sr_model* next = nullptr;
      check(sr_model_create_from_statistics(mixtures_.device(), d, S, off.data(), n_mean, n_var, dm.data(), dv.data(), st.mean_acc.data(),
                                            st.mean_w.data(), st.var_acc.data(), st.var_w.data(), (int)sch.pooling,
                                            sch.max_approx ? 1 : 0, &next));
      cur.reset(next);
      h = next;
      r.am_scores.push_back(am_score_of(h, corpus, states));
    };
    auto reshape = [&](bool do_split) {
      sr_model* next = nullptr;
      check(do_split ? sr_model_split(h, nullptr, st.mean_w.data(), sch.min_obs, sch.epsilon, (int)sch.pooling, &next, nullptr)
                     : sr_model_eliminate(h, nullptr, st.mean_w.data(), sch.min_obs, &next, nullptr));
      cur.reset(next);
      h = next;
    };
    estimate(true);                                    // 2.
    for (uint32_t s = 0; s < sch.num_splits; s++) {    // 3.
      reshape(true);
      estimate(false);
      reshape(false);
      estimate(false);
    }
    for (uint32_t a = 0; a < sch.num_aligns; a++) {    // 4.
      std::vector<double> cost;
      align_states(h, corpus, automata, aut_off, states, cost);
      for (uint32_t e = 0; e < sch.num_estimates; e++) estimate(false);
    }
    r.alignment.assign(F, AlignmentItem());
    for (uint64_t t = 0; t < F; t++) { r.alignment[t].state = states[t]; r.alignment[t].weight = 1; r.alignment[t].count = 1; }
    r.model.reset(new MixtureModel(cur.release(), mixtures_));
    return r;
  }

  // Trainer::calc_am_score (Training.cpp:585-612): sequential sum of score(frame, aligned state) / frames
  double calc_am_score(Corpus const& corpus, std::vector<AlignmentItem> const& alignment) {
    const uint64_t F = corpus.get_total_frame_count();
    std::vector<uint16_t> states(std::max<uint64_t>(F, 1));
    for (uint64_t t = 0; t < F; t++) states[t] = alignment[t].state;
    return am_score_of(mixtures_.handle(), corpus, states);
  }

 private:
  double am_score_of(sr_model* h, Corpus const& corpus, std::vector<uint16_t> const& states) {
    const uint64_t F = corpus.get_total_frame_count();
    std::vector<double> per_frame(std::max<uint64_t>(F, 1));
    sr_corpus* c = nullptr;
    check(sr_corpus_upload(h, corpus.features(), corpus.frame_offsets(), (uint32_t)corpus.get_corpus_size(), &c));
    const int rc = sr_path_scores_corpus(h, c, states.data(), mixtures_.gmm_kernel, per_frame.data());
    sr_corpus_destroy(c);
    check(rc);
    double total_score = 0.0;
    for (uint64_t t = 0; t < F; t++) total_score += per_frame[t];
    return total_score / F;
  }
  // the aligner of realign() over every segment, on model h
  void align_states(sr_model* h, Corpus const& corpus, std::vector<uint16_t> const& automata, std::vector<uint64_t> const& aut_off,
                    std::vector<uint16_t>& states, std::vector<double>& cost) {
    const size_t n = corpus.get_corpus_size();
    const double tdp[3] = {tdp_.tdp_loop, tdp_.tdp_forward, tdp_.tdp_skip};
    sr_corpus* c = nullptr;
    check(sr_corpus_upload(h, corpus.features(), corpus.frame_offsets(), (uint32_t)n, &c));
    states.assign(std::max<uint64_t>(corpus.get_total_frame_count(), 1), 0);
    cost.assign(std::max<size_t>(n, 1), 0.0);
    const int rc = alignment_pruning_
                       ? sr_align_corpus_pruned(h, c, automata.data(), aut_off.data(), tdp, tdp_.silence_state, pruning_threshold_,
                                                mixtures_.gmm_kernel, states.data(), cost.data())
                       : sr_align_corpus(h, c, automata.data(), aut_off.data(), tdp, tdp_.silence_state, mixtures_.gmm_kernel,
                                         states.data(), cost.data());
    sr_corpus_destroy(c);
    check(rc);
  }
  // sr_accumulate_corpus of an alignment on model h, the statistics brought to the host
  void accumulate_on(sr_model* h, Corpus const& corpus, std::vector<uint16_t> const& states, bool first_pass, bool max_approx,
                     Statistics& st) {
    uint32_t n_mean = 0, n_var = 0;
    check(sr_model_tying_info(h, &n_mean, &n_var));
    const size_t D = mixtures_.dimension;
    st.mean_acc.assign(std::max<size_t>(n_mean * D, 1), 0.0); st.mean_w.assign(std::max<size_t>(n_mean, 1), 0.0);
    st.var_acc.assign(std::max<size_t>(n_var * D, 1), 0.0); st.var_w.assign(std::max<size_t>(n_var, 1), 0.0);
    sr_corpus* c = nullptr;
    check(sr_corpus_upload(h, corpus.features(), corpus.frame_offsets(), (uint32_t)corpus.get_corpus_size(), &c));
    const int rc = sr_accumulate_corpus(h, c, states.data(), first_pass ? 1 : 0, max_approx ? 1 : 0, st.mean_acc.data(), st.mean_w.data(),
                                        st.var_acc.data(), st.var_w.data());
    sr_corpus_destroy(c);
    check(rc);
  }
  static const double* checked_weights(sr_model* h, std::vector<double> const& mean_w) {
    uint32_t n_mean = 0, n_var = 0;
    check(sr_model_tying_info(h, &n_mean, &n_var));
    if (mean_w.size() < n_mean) throw std::invalid_argument("split / eliminate: one weight per mean row");
    return mean_w.data();
  }
  std::unique_ptr<MixtureModel> split_of(sr_model* h, sr_corpus* c, const double* w, double min_obs, double epsilon) {
    sr_model* next = nullptr;
    check(sr_model_split(h, c, w, min_obs, epsilon, (int)mixtures_.var_model, &next, nullptr));
    return std::unique_ptr<MixtureModel>(new MixtureModel(next, mixtures_));
  }
  std::unique_ptr<MixtureModel> eliminate_of(sr_model* h, sr_corpus* c, const double* w, double min_obs) {
    sr_model* next = nullptr;
    check(sr_model_eliminate(h, c, w, min_obs, &next, nullptr));
    return std::unique_ptr<MixtureModel>(new MixtureModel(next, mixtures_));
  }
  // every segment's automaton (build_segment_automaton), concatenated, with offsets
  void segment_automata(Corpus const& corpus, std::vector<uint16_t>& automata, std::vector<uint64_t>& aut_off) const {
    automata.clear();
    aut_off.assign(1, 0);
    for (size_t s = 0; s < corpus.get_corpus_size(); s++) {
      auto w = corpus.get_word_sequence(s);
      MarkovAutomaton a = build_segment_automaton(w.first, w.second);
      automata.insert(automata.end(), a.states.begin(), a.states.end());
      aut_off.push_back(automata.size());
    }
  }

  const double pruning_threshold_;
  const bool alignment_pruning_;
  Lexicon const& lexicon_;
  MixtureModel& mixtures_;
  TdpModel tdp_;
};

// ---- fMLLR speaker adaptation (srgpu.h: sr_fmllr_*, sr_corpus_transform) -------------------------------------------------------
// One affine feature transform per speaker of the corpus (Corpus::speakers()), estimated by maximum likelihood from the trainer's
// re-alignment; the model is untouched.  In the reference's flow the adapted features take the place of the corpus' features after
// FeaturePostProcessor::process_features and before any prepare_sequence.
class SpeakerAdaptation {
 public:
  struct Result {
    uint32_t n_speakers = 0;
    std::vector<double> transforms;   // [n_speakers x D x (D+1)] W_s = [A_s b_s], row-major
    std::vector<double> logdet;       // [n_speakers] log|det A_s|
    std::vector<double> beta;         // [n_speakers] frames (occupancy) behind each estimate
    std::vector<int32_t> status;      // [n_speakers] sr_fmllr_estimate's: 0 estimated, 1 too little data (identity), 2 failed (identity)
    std::vector<double> aux;          // [n_speakers x (n_sweeps + 1)] the auxiliary function after 0 .. n_sweeps sweeps
    std::vector<float> features;      // the adapted corpus features, the corpus' layout (for a FeatureScorer's prepare_sequence)
    // the adapted corpus, resident (sr_corpus_transform): what sr_recognize_corpus, sr_align_corpus, ... take in place of an upload
    // of `features`.  Destroyed with the last copy of the Result, which must not outlive the model.
    std::shared_ptr<sr_corpus> adapted;
  };

  SpeakerAdaptation(Trainer& trainer, MixtureModel& mixtures, uint32_t n_sweeps = 10, double min_count = 100.0)
      : trainer_(trainer), mixtures_(mixtures), n_sweeps_(n_sweeps), min_count_(min_count) {}

  static std::vector<double> identity(size_t dim, uint32_t n_speakers) {
    std::vector<double> W((size_t)n_speakers * dim * (dim + 1), 0.0);
    for (uint32_t s = 0; s < n_speakers; s++)
      for (size_t i = 0; i < dim; i++) W[((size_t)s * dim + i) * (dim + 1) + i] = 1.0;
    return W;
  }

  // the estimate alone, from statistics, starting at the identity (host code, no device)
  static void estimate(size_t dim, std::vector<double> const& beta, std::vector<double> const& k, std::vector<double> const& G,
                       uint32_t n_sweeps, double min_count, Result& r) {
    r.n_speakers = (uint32_t)beta.size();
    r.beta = beta;
    r.transforms = identity(dim, r.n_speakers);
    r.logdet.assign(r.n_speakers, 0.0);
    r.status.assign(r.n_speakers, 0);
    r.aux.assign((size_t)r.n_speakers * (n_sweeps + 1), 0.0);
    check(sr_fmllr_estimate((uint32_t)dim, r.n_speakers, beta.data(), k.data(), G.data(), n_sweeps, min_count, r.transforms.data(),
                            r.aux.data(), r.logdet.data(), r.status.data()));
  }

  // sr_corpus_transform's loop on the host: acc = b_i, then acc = acc + A_ij * (double) x_j for j ascending, every product rounded
  // before it is added (the volatile keeps a compiler from fusing the two), (float) acc -- the device's bits
  static void transform_row(const double* W, size_t D, const float* x, float* y) {
    for (size_t i = 0; i < D; i++) {
      double acc = W[i * (D + 1) + D];
      for (size_t j = 0; j < D; j++) {
        volatile double p = W[i * (D + 1) + j] * (double)x[j];
        acc = acc + p;
      }
      y[i] = (float)acc;
    }
  }

  // re-align, take the statistics of the alignment, estimate, transform
  Result adapt(Corpus const& corpus) {
    const size_t n = corpus.get_corpus_size(), D = mixtures_.dimension;
    const uint64_t F = corpus.get_total_frame_count();
    std::vector<uint32_t> const& spk = corpus.speakers();
    uint32_t S = 0;
    for (uint32_t s : spk) S = std::max(S, s + 1);
    if (S == 0) throw std::runtime_error("SpeakerAdaptation: empty corpus");
    std::vector<AlignmentItem> alignment;
    trainer_.realign(corpus, alignment);
    std::vector<uint16_t> states(std::max<uint64_t>(F, 1));
    for (uint64_t t = 0; t < F; t++) states[t] = (uint16_t)alignment[t].state;
    std::vector<double> beta(S), k((size_t)S * D * (D + 1)), G((size_t)S * D * (D + 1) * (D + 1));
    sr_corpus* c = nullptr;
    check(sr_corpus_upload(mixtures_.handle(), corpus.features(), corpus.frame_offsets(), (uint32_t)n, &c));
    std::shared_ptr<sr_corpus> original(c, sr_corpus_destroy);
    check(sr_fmllr_statistics_corpus(mixtures_.handle(), c, states.data(), spk.data(), S, mixtures_.max_approx() ? 1 : 0, beta.data(),
                                     k.data(), G.data()));
    Result r;
    estimate(D, beta, k, G, n_sweeps_, min_count_, r);
    sr_corpus* adapted = nullptr;
    check(sr_corpus_transform(mixtures_.handle(), c, spk.data(), S, r.transforms.data(), &adapted));
    r.adapted.reset(adapted, sr_corpus_destroy);
    r.features.resize((size_t)F * D);
    for (size_t u = 0; u < n; u++)
      for (uint64_t t = corpus.frame_offsets()[u]; t < corpus.frame_offsets()[u + 1]; t++)
        transform_row(r.transforms.data() + (size_t)spk[u] * D * (D + 1), D, corpus.features() + t * D, r.features.data() + t * D);
    return r;
  }

 private:
  Trainer& trainer_;
  MixtureModel& mixtures_;
  uint32_t n_sweeps_;
  double min_count_;
};

// ---- MLLR of the means with regression classes (srgpu.h: sr_mllr_*, sr_model_transform_means) ----------------------------------
// One affine transform of the means per speaker and regression class, estimated by maximum likelihood from the trainer's
// re-alignment over a regression-class tree; the features are untouched.  A speaker is then recognised or aligned with its own adapted
// model: upload that speaker's utterances to adapted_model(...).
class MeanAdaptation {
 public:
  struct Result {
    uint32_t n_speakers = 0, n_classes = 0;
    std::vector<double> transforms;   // [n_speakers x n_classes x D x (D+1)] W_{s,r} = [A b], row-major
    std::vector<double> beta;         // [n_speakers x n_classes] occupancy of each base class
    std::vector<int32_t> node;        // [n_speakers x n_classes] the tree node whose statistics gave the transform, -1: identity kept
    std::vector<double> aux;          // [n_speakers x n_classes x 2] Q of that node at the identity and at the result
  };

  // dens_class[n_densities] in mixture order, < n_classes; parent[n_nodes]: the tree over the classes (sr_mllr_estimate), empty: none
  MeanAdaptation(Trainer& trainer, MixtureModel& mixtures, std::vector<uint32_t> dens_class, uint32_t n_classes,
                 std::vector<int32_t> parent = std::vector<int32_t>(), double min_count = 100.0)
      : trainer_(trainer), mixtures_(mixtures), dens_class_(std::move(dens_class)), n_classes_(n_classes), parent_(std::move(parent)),
        min_count_(min_count) {
    if (parent_.empty()) parent_.assign(n_classes_, -1);
  }

  // the estimate alone, from statistics, starting at the identity (host code, no device)
  static void estimate(size_t dim, uint32_t n_speakers, uint32_t n_classes, std::vector<int32_t> const& parent,
                       std::vector<double> const& beta, std::vector<double> const& k, std::vector<double> const& G, double min_count,
                       Result& r) {
    r.n_speakers = n_speakers;
    r.n_classes = n_classes;
    r.beta = beta;
    r.transforms = SpeakerAdaptation::identity(dim, n_speakers * n_classes);
    r.node.assign((size_t)n_speakers * n_classes, -1);
    r.aux.assign((size_t)n_speakers * n_classes * 2, 0.0);
    check(sr_mllr_estimate((uint32_t)dim, n_speakers, n_classes, (uint32_t)parent.size(), parent.data(), beta.data(), k.data(), G.data(),
                           min_count, r.transforms.data(), r.node.data(), r.aux.data()));
  }

  // re-align, take the statistics of the alignment per (speaker, class), estimate
  Result adapt(Corpus const& corpus) {
    const size_t n = corpus.get_corpus_size(), D = mixtures_.dimension;
    const uint64_t F = corpus.get_total_frame_count();
    std::vector<uint32_t> const& spk = corpus.speakers();
    uint32_t S = 0;
    for (uint32_t s : spk) S = std::max(S, s + 1);
    if (S == 0) throw std::runtime_error("MeanAdaptation: empty corpus");
    std::vector<AlignmentItem> alignment;
    trainer_.realign(corpus, alignment);
    std::vector<uint16_t> states(std::max<uint64_t>(F, 1));
    for (uint64_t t = 0; t < F; t++) states[t] = (uint16_t)alignment[t].state;
    const size_t groups = (size_t)S * n_classes_;
    std::vector<double> beta(groups), k(groups * D * (D + 1)), G(groups * D * (D + 1) * (D + 1));
    sr_corpus* c = nullptr;
    check(sr_corpus_upload(mixtures_.handle(), corpus.features(), corpus.frame_offsets(), (uint32_t)n, &c));
    std::shared_ptr<sr_corpus> original(c, sr_corpus_destroy);
    check(sr_mllr_statistics_corpus(mixtures_.handle(), c, states.data(), spk.data(), S, dens_class_.data(), n_classes_,
                                    mixtures_.max_approx() ? 1 : 0, beta.data(), k.data(), G.data()));
    Result r;
    estimate(D, S, n_classes_, parent_, beta, k, G, min_count_, r);
    return r;
  }

  // the model of one speaker (sr_model_transform_means): a model of its own, the base model's tables are copied
  std::shared_ptr<sr_model> adapted_model(Result const& r, uint32_t speaker) const {
    const size_t D = mixtures_.dimension;
    if (speaker >= r.n_speakers) throw std::runtime_error("MeanAdaptation: no such speaker");
    sr_model* out = nullptr;
    check(sr_model_transform_means(mixtures_.handle(), dens_class_.data(), n_classes_,
                                   r.transforms.data() + (size_t)speaker * n_classes_ * D * (D + 1), &out));
    return std::shared_ptr<sr_model>(out, sr_model_destroy);
  }

 private:
  Trainer& trainer_;
  MixtureModel& mixtures_;
  std::vector<uint32_t> dens_class_;
  uint32_t n_classes_;
  std::vector<int32_t> parent_;
  double min_count_;
};

// ---- MAP adaptation of the means and weights (srgpu.h: sr_map_statistics_*, sr_model_map_adapt) ---------------------------------
// Every density a speaker's data reached moves towards that data, (tau mu + X) / (tau + O); every other density stays.  The statistics
// come from the trainer's re-alignment; a speaker is then recognised or aligned with its own adapted model: upload that speaker's
// utterances to adapted_model(...).  To iterate, re-align under the adapted model and adapt the speaker-independent model again.
class MapAdaptation {
 public:
  struct Result {
    uint32_t n_speakers = 0;
    std::vector<uint64_t> ent_off;    // [n_speakers + 1] speaker s owns entries ent_off[s] .. ent_off[s + 1]
    std::vector<uint32_t> dens;       // [n_entries] density id in mixture order, ascending within a speaker
    std::vector<double> occ;          // [n_entries] sum gamma
    std::vector<double> x;            // [n_entries x D] sum gamma x
  };

  MapAdaptation(Trainer& trainer, MixtureModel& mixtures) : trainer_(trainer), mixtures_(mixtures) {}

  // re-align, take the statistics of the alignment per (speaker, density): the sizing call, then the filled call
  Result adapt(Corpus const& corpus) {
    const size_t n = corpus.get_corpus_size(), D = mixtures_.dimension;
    const uint64_t F = corpus.get_total_frame_count();
    std::vector<uint32_t> const& spk = corpus.speakers();
    uint32_t S = 0;
    for (uint32_t s : spk) S = std::max(S, s + 1);
    if (S == 0) throw std::runtime_error("MapAdaptation: empty corpus");
    std::vector<AlignmentItem> alignment;
    trainer_.realign(corpus, alignment);
    std::vector<uint16_t> states(std::max<uint64_t>(F, 1));
    for (uint64_t t = 0; t < F; t++) states[t] = (uint16_t)alignment[t].state;
    sr_corpus* c = nullptr;
    check(sr_corpus_upload(mixtures_.handle(), corpus.features(), corpus.frame_offsets(), (uint32_t)n, &c));
    std::shared_ptr<sr_corpus> original(c, sr_corpus_destroy);
    const int max_approx = mixtures_.max_approx() ? 1 : 0;
    Result r;
    r.n_speakers = S;
    r.ent_off.assign((size_t)S + 1, 0);
    check(sr_map_statistics_corpus(mixtures_.handle(), c, states.data(), spk.data(), S, max_approx, 0, r.ent_off.data(), nullptr, nullptr,
                                   nullptr));
    const uint64_t cap = r.ent_off[S];
    r.dens.assign(std::max<uint64_t>(cap, 1), 0); r.occ.assign(std::max<uint64_t>(cap, 1), 0.0); r.x.assign(std::max<uint64_t>(cap, 1) * D, 0.0);
    check(sr_map_statistics_corpus(mixtures_.handle(), c, states.data(), spk.data(), S, max_approx, cap, r.ent_off.data(), r.dens.data(),
                                   r.occ.data(), r.x.data()));
    r.dens.resize(cap); r.occ.resize(cap); r.x.resize(cap * D);
    return r;
  }

  // the model of one speaker (sr_model_map_adapt) with mixtures as the prior -- or `prior`, e.g. MeanAdaptation::adapted_model's
  // result for MAP on top of MLLR; tau_w > 0: the mixture weights are updated too
  std::shared_ptr<sr_model> adapted_model(Result const& r, uint32_t speaker, double tau, double tau_w = 0.0, sr_model* prior = nullptr) const {
    const size_t D = mixtures_.dimension;
    if (speaker >= r.n_speakers) throw std::runtime_error("MapAdaptation: no such speaker");
    const uint64_t e0 = r.ent_off[speaker], ne = r.ent_off[speaker + 1] - e0;
    sr_model* out = nullptr;
    check(sr_model_map_adapt(prior ? prior : mixtures_.handle(), ne, r.dens.data() + e0, r.occ.data() + e0, r.x.data() + e0 * D, tau,
                             tau_w > 0.0 ? 1 : 0, tau_w, &out));
    return std::shared_ptr<sr_model>(out, sr_model_destroy);
  }

 private:
  Trainer& trainer_;
  MixtureModel& mixtures_;
};

// ---- MLLT, the global semi-tied covariance transform (srgpu.h: sr_mllt_*) --------------------------------------------------------
// One square matrix A for the whole feature space, estimated by maximum likelihood from the trainer's re-alignment so that the model's
// diagonal covariances fit as well as they can; features and means both move (y = A x, mu' = A mu).  The variances are re-estimated
// by the next training pass over the adapted corpus with the adapted model.
class Mllt {
 public:
  struct Result {
    std::vector<double> A;            // [D x D] row-major
    std::vector<double> affine;       // [D x (D+1)] = [A 0]: the W of sr_corpus_transform and sr_model_transform_means
    double logdet = 0.0;              // log|det A|
    double beta = 0.0;                // frames (occupancy) behind the estimate
    int32_t status = 0;               // sr_mllt_estimate's: 0 estimated, 1 too little data (identity), 2 failed (identity)
    std::vector<double> aux;          // [n_sweeps + 1] the auxiliary function after 0 .. n_sweeps sweeps
    std::vector<float> features;      // the adapted corpus features, the corpus' layout: what is uploaded to `model`
    // the adapted corpus, resident (sr_corpus_transform), and the adapted model (sr_model_transform_means).  Destroyed with the last
    // copy of the Result; `adapted` belongs to the base model and must not outlive it.
    std::shared_ptr<sr_corpus> adapted;
    std::shared_ptr<sr_model> model;
  };

  Mllt(Trainer& trainer, MixtureModel& mixtures, uint32_t n_sweeps = 10, double min_count = 100.0)
      : trainer_(trainer), mixtures_(mixtures), n_sweeps_(n_sweeps), min_count_(min_count) {}

  // the estimate alone, from statistics, starting at the identity (host code, no device)
  static void estimate(size_t dim, double beta, std::vector<double> const& G, uint32_t n_sweeps, double min_count, Result& r) {
    r.beta = beta;
    r.A.assign(dim * dim, 0.0);
    for (size_t i = 0; i < dim; i++) r.A[i * dim + i] = 1.0;
    r.aux.assign((size_t)n_sweeps + 1, 0.0);
    check(sr_mllt_estimate((uint32_t)dim, beta, G.data(), n_sweeps, min_count, r.A.data(), r.aux.data(), &r.logdet, &r.status));
    r.affine.assign(dim * (dim + 1), 0.0);
    for (size_t i = 0; i < dim; i++) std::copy(r.A.begin() + i * dim, r.A.begin() + (i + 1) * dim, r.affine.begin() + i * (dim + 1));
  }

  // re-align, take the statistics of the alignment, estimate, transform the corpus and the means
  Result adapt(Corpus const& corpus) {
    const size_t n = corpus.get_corpus_size(), D = mixtures_.dimension;
    const uint64_t F = corpus.get_total_frame_count();
    std::vector<AlignmentItem> alignment;
    trainer_.realign(corpus, alignment);
    std::vector<uint16_t> states(std::max<uint64_t>(F, 1));
    for (uint64_t t = 0; t < F; t++) states[t] = (uint16_t)alignment[t].state;
    double beta = 0.0;
    std::vector<double> G(D * D * D);
    sr_corpus* c = nullptr;
    check(sr_corpus_upload(mixtures_.handle(), corpus.features(), corpus.frame_offsets(), (uint32_t)n, &c));
    std::shared_ptr<sr_corpus> original(c, sr_corpus_destroy);
    check(sr_mllt_statistics_corpus(mixtures_.handle(), c, states.data(), mixtures_.max_approx() ? 1 : 0, &beta, G.data()));
    Result r;
    estimate(D, beta, G, n_sweeps_, min_count_, r);
    const std::vector<uint32_t> one_speaker(std::max<size_t>(n, 1), 0);
    sr_corpus* adapted = nullptr;
    check(sr_corpus_transform(mixtures_.handle(), c, one_speaker.data(), 1, r.affine.data(), &adapted));
    r.adapted.reset(adapted, sr_corpus_destroy);
    r.features.resize((size_t)F * D);
    for (uint64_t t = 0; t < F; t++)
      SpeakerAdaptation::transform_row(r.affine.data(), D, corpus.features() + t * D, r.features.data() + t * D);
    uint32_t dim = 0, n_states = 0;
    uint64_t n_dens = 0;
    check(sr_model_info(mixtures_.handle(), &dim, &n_states, &n_dens));
    const std::vector<uint32_t> one_class(std::max<uint64_t>(n_dens, 1), 0);
    sr_model* model = nullptr;
    check(sr_model_transform_means(mixtures_.handle(), one_class.data(), 1, r.affine.data(), &model));
    r.model.reset(model, sr_model_destroy);
    return r;
  }

 private:
  Trainer& trainer_;
  MixtureModel& mixtures_;
  uint32_t n_sweeps_;
  double min_count_;
};

// ---- LDA with frame splicing (srgpu.h: sr_lda_*, sr_corpus_splice_transform) ------------------------------------------------------
// Every frame is stacked with `context` neighbours on either side and projected to p dimensions so that the classes -- the aligned
// states through class_of_state, SR_LDA_SKIP for the ones to leave out (silence) -- are separated as well as a linear map can.  The
// projected corpus lives with a placeholder model of p dimensions; one first-pass accumulate over it gives the first model of the
// new space (one density per state), from which EM and then sr::Mllt go on.
class Lda {
 public:
  struct Result {
    uint32_t E = 0, p = 0;
    std::vector<double> M;            // [p x (E+1)] = [A b], row-major
    std::vector<double> eig;          // [E] descending (status 0 only)
    std::vector<double> count;        // [n_classes] kept frames per class
    int32_t status = 0;               // sr_lda_estimate's: 0 estimated, 1 too little data, 2 failed (then no corpus and no model)
    // the placeholder that owns the projected corpus, the projected corpus (sr_corpus_splice_transform) and the model of one first-pass
    // accumulate over it.  Declared in this order: the corpus goes before its model.
    std::shared_ptr<sr_model> placeholder;
    std::shared_ptr<sr_corpus> projected;
    std::shared_ptr<sr_model> model;
  };

  struct Config {
    uint32_t context = 4, p = 40;
    std::vector<uint32_t> class_of_state;  // [n_states]; empty: the state is the class
    uint32_t n_classes = 0;                // 0: the number of states
    bool remove_mean = true;
    double min_count = 100.0;
    int device = 0;
  };

  Lda(Trainer& trainer, MixtureModel& mixtures, Config const& config) : trainer_(trainer), mixtures_(mixtures), config_(config) {}

  // the estimate alone, from statistics (host code, no device)
  static void estimate(uint32_t E, uint32_t n_classes, std::vector<double> const& count, std::vector<double> const& sum,
                       std::vector<double> const& scatter, uint32_t p, bool remove_mean, double min_count, Result& r) {
    if (count.size() < n_classes || sum.size() < (size_t)n_classes * E || scatter.size() < (size_t)E * E)
      throw std::runtime_error("Lda: statistics too short");
    r.E = E; r.p = p; r.count = count;
    r.M.assign((size_t)p * (E + 1), 0.0);
    r.eig.assign(E, 0.0);
    check(sr_lda_estimate(E, n_classes, count.data(), sum.data(), scatter.data(), p, remove_mean ? 1 : 0, min_count, r.M.data(), r.eig.data(),
                          &r.status));
  }

  // statistics of an alignment given by the caller, estimate, projected corpus, first-pass model
  static Result from_alignment(sr_model* base, Corpus const& corpus, std::vector<uint16_t> const& states, Config const& cfg) {
    const size_t n = corpus.get_corpus_size();
    uint32_t D = 0, n_states = 0;
    uint64_t n_dens = 0;
    check(sr_model_info(base, &D, &n_states, &n_dens));
    if (!cfg.class_of_state.empty() && cfg.class_of_state.size() != n_states) throw std::runtime_error("Lda: one class per state");
    if (states.size() < corpus.get_total_frame_count()) throw std::runtime_error("Lda: one state per frame");
    const uint32_t K = cfg.n_classes ? cfg.n_classes : n_states, E = (2 * cfg.context + 1) * D;
    sr_corpus* c = nullptr;
    check(sr_corpus_upload(base, corpus.features(), corpus.frame_offsets(), (uint32_t)n, &c));
    std::shared_ptr<sr_corpus> original(c, sr_corpus_destroy);
    std::vector<double> count(K), sum((size_t)K * E), scatter((size_t)E * E);
    check(sr_lda_statistics_corpus(base, c, states.data(), cfg.context, cfg.class_of_state.empty() ? nullptr : cfg.class_of_state.data(), K,
                                   count.data(), sum.data(), scatter.data()));
    Result r;
    estimate(E, K, count, sum, scatter, cfg.p, cfg.remove_mean, cfg.min_count, r);
    if (r.status != 0) return r;
    // the placeholder: p dimensions, the alignment's states with one density each
    std::vector<uint32_t> dens_off(n_states + 1);
    for (uint32_t s = 0; s <= n_states; s++) dens_off[s] = s;
    const std::vector<double> zeros((size_t)n_states * cfg.p, 0.0), ones((size_t)n_states * cfg.p, 1.0);
    sr_model* target = nullptr;
    check(sr_model_create(cfg.device, cfg.p, n_states, dens_off.data(), zeros.data(), ones.data(), zeros.data(), zeros.data(), 1, &target));
    r.placeholder.reset(target, sr_model_destroy);
    sr_corpus* projected = nullptr;
    check(sr_corpus_splice_transform(base, c, target, cfg.context, r.M.data(), &projected));
    r.projected.reset(projected, sr_corpus_destroy);
    check(sr_accumulate_corpus(target, projected, states.data(), 1, 1, nullptr, nullptr, nullptr, nullptr));
    sr_model* model = nullptr;
    check(sr_model_create_from_accumulated(target, projected, MixtureModel::NO_POOLING, 1, &model));
    r.model.reset(model, sr_model_destroy);
    return r;
  }

  // re-align with the trainer, then from_alignment
  Result adapt(Corpus const& corpus) {
    const uint64_t F = corpus.get_total_frame_count();
    std::vector<AlignmentItem> alignment;
    trainer_.realign(corpus, alignment);
    std::vector<uint16_t> states(std::max<uint64_t>(F, 1));
    for (uint64_t t = 0; t < F; t++) states[t] = (uint16_t)alignment[t].state;
    return from_alignment(mixtures_.handle(), corpus, states, config_);
  }

 private:
  Trainer& trainer_;
  MixtureModel& mixtures_;
  Config config_;
};

// ---- Teaching::LinearSearch (rwth-asr-0.5/src/Teaching/LinearSearch.hh:9-62, SearchInterface.hh:20-30) -------------
// Bigram-LM beam search over a linear lexicon, one device pass per corpus.  The toolkit wires lexicon, language model
// and transition model through Speech::ModelCombination (LinearSearch.cc:462-475); here they are plain arrays:
//   linear_lexicon[w] = mixture (emission state) sequence of word w (LinearSearch::buildLinearLexicon :477-483),
//   lm[w * W + h]     = getLanguageModelScore(w, h) = -log p(w | h) (SearchInterface.cc:77-81),
//   tdp[isSilence][loop, forward, skip, exit] (SearchSpace::setTransitionScores :169-180).
// Parameters keep the reference's names: "acoustic-pruning", "lm-pruning" (:438-446), infinity = no beam.
class LinearSearch {
 public:
  struct TracebackItem {  // SearchInterface::TracebackItem
    uint32_t word;
    float score;
    uint32_t time;
  };
  typedef std::vector<TracebackItem> Traceback;

  LinearSearch(MixtureModel& scorer, std::vector<std::vector<uint16_t> > const& linear_lexicon, uint32_t silence,
               std::vector<float> const& lm, const float tdp[2][4], float acoustic_pruning = std::numeric_limits<float>::max(),
               float lm_pruning = std::numeric_limits<float>::max())
      : scorer_(scorer), acoustic_pruning_(acoustic_pruning), lm_pruning_(lm_pruning), n_words_((uint32_t)linear_lexicon.size()),
        silence_(silence), lm_(lm) {
    std::vector<uint32_t> word_off(1, 0);
    std::vector<uint16_t> mixtures;
    for (size_t w = 0; w < linear_lexicon.size(); w++) {
      mixtures.insert(mixtures.end(), linear_lexicon[w].begin(), linear_lexicon[w].end());
      word_off.push_back((uint32_t)mixtures.size());
    }
    if (lm.size() != linear_lexicon.size() * linear_lexicon.size()) throw std::runtime_error("LinearSearch: lm must be W x W");
    check(sr_bigram_create(scorer.handle(), (uint32_t)linear_lexicon.size(), word_off.data(), mixtures.data(), silence, lm.data(),
                           &tdp[0][0], &net_));
  }
  ~LinearSearch() { sr_bigram_destroy(net_); }
  LinearSearch(LinearSearch const&) = delete;
  LinearSearch& operator=(LinearSearch const&) = delete;

  // initialize() + processFrame(1..T) + getResult() (LinearSearch.cc:489-520) for every segment of the corpus
  void recognize(Corpus const& corpus, std::vector<Traceback>& results) {
    const size_t n = corpus.get_corpus_size();
    const uint64_t F = corpus.get_total_frame_count();
    std::vector<uint32_t> words(F + n + 1), times(F + n + 1);
    std::vector<float> scores(F + n + 1);
    std::vector<uint64_t> off(n + 1);
    sr_corpus* c = nullptr;
    check(sr_corpus_upload(scorer_.handle(), corpus.features(), corpus.frame_offsets(), (uint32_t)n, &c));
    sr_bigram_params p = sr_bigram_params();  // zeroed, then field by field: a field added to the struct cannot shift these
    p.acoustic_pruning = acoustic_pruning_;
    p.lm_pruning = lm_pruning_;
    p.gmm_kernel = scorer_.gmm_kernel;
    const int rc = sr_recognize_bigram_corpus(scorer_.handle(), c, net_, &p, words.data(), scores.data(), times.data(), off.data());
    sr_corpus_destroy(c);
    check(rc);
    results.assign(n, Traceback());
    for (size_t s = 0; s < n; s++)
      for (uint64_t i = off[s]; i < off[s + 1]; i++) results[s].push_back(TracebackItem{words[i], scores[i], times[i]});
  }

  // recognize()'s items, bit for bit, and for each the maximum over its frames of the word's posterior in the search network
  // summed without beams, every cost times `scale` (sr_recognize_bigram_confidence_corpus): confidences[s][i] belongs to results[s][i]
  void recognize_with_confidence(Corpus const& corpus, double scale, std::vector<Traceback>& results,
                                 std::vector<std::vector<double> >& confidences) {
    const size_t n = corpus.get_corpus_size();
    const uint64_t F = corpus.get_total_frame_count();
    std::vector<uint32_t> words(F + n + 1), times(F + n + 1);
    std::vector<float> scores(F + n + 1);
    std::vector<double> conf(F + n + 1);
    std::vector<uint64_t> off(n + 1);
    sr_corpus* c = nullptr;
    check(sr_corpus_upload(scorer_.handle(), corpus.features(), corpus.frame_offsets(), (uint32_t)n, &c));
    sr_bigram_params p = sr_bigram_params();
    p.acoustic_pruning = acoustic_pruning_;
    p.lm_pruning = lm_pruning_;
    p.gmm_kernel = scorer_.gmm_kernel;
    const int rc = sr_recognize_bigram_confidence_corpus(scorer_.handle(), c, net_, &p, scale, words.data(), scores.data(), times.data(),
                                                         off.data(), conf.data());
    sr_corpus_destroy(c);
    check(rc);
    results.assign(n, Traceback());
    confidences.assign(n, std::vector<double>());
    for (size_t s = 0; s < n; s++)
      for (uint64_t i = off[s]; i < off[s + 1]; i++) {
        results[s].push_back(TracebackItem{words[i], scores[i], times[i]});
        confidences[s].push_back(conf[i]);
      }
  }

  // One MMI E-step against THIS search's network (sr_bigram_mmi_statistics_corpus): the numerator over the network restricted to each
  // segment's transcript (word ids, silence not listed), the denominator over the free network with the bigram LM, every cost times
  // scale (kappa).  f_num / f_den per segment (+inf: no path through the transcript; such a segment contributes to neither side) and
  // both statistics sets, ready for sr_model_create_from_mmi_statistics.  The next iteration needs a LinearSearch on the NEW model: an
  // sr_bigram belongs to the model it was created on.
  struct MmiStatistics {
    std::vector<double> f_num, f_den;
    Trainer::Statistics num, den;
  };
  MmiStatistics mmi_statistics(Corpus const& corpus, std::vector<std::vector<uint32_t> > const& transcripts, double scale,
                               double posterior_floor = 0.0) {
    const size_t n = corpus.get_corpus_size();
    if (transcripts.size() != n) throw std::invalid_argument("mmi_statistics: one transcript per segment");
    std::vector<uint32_t> trans;
    std::vector<uint64_t> trans_off(1, 0);
    for (auto const& t : transcripts) {
      trans.insert(trans.end(), t.begin(), t.end());
      trans_off.push_back(trans.size());
    }
    trans.push_back(0);  // (never empty: the ABI tells "no transcripts" by a null pointer)
    uint32_t n_mean = 0, n_var = 0;
    check(sr_model_tying_info(scorer_.handle(), &n_mean, &n_var));
    const size_t D = scorer_.dimension;
    MmiStatistics r;
    r.f_num.assign(std::max<size_t>(n, 1), 0.0);
    r.f_den.assign(std::max<size_t>(n, 1), 0.0);
    for (Trainer::Statistics* st : {&r.num, &r.den}) {
      st->mean_acc.assign(n_mean * D, 0.0); st->mean_w.assign(n_mean, 0.0);
      st->var_acc.assign(n_var * D, 0.0); st->var_w.assign(n_var, 0.0);
    }
    sr_corpus* c = nullptr;
    check(sr_corpus_upload(scorer_.handle(), corpus.features(), corpus.frame_offsets(), (uint32_t)n, &c));
    const int rc = sr_bigram_mmi_statistics_corpus(scorer_.handle(), c, net_, scorer_.gmm_kernel, scale, posterior_floor,
                                                   scorer_.max_approx() ? 1 : 0, trans.data(), trans_off.data(), r.f_num.data(),
                                                   r.f_den.data(), r.num.mean_acc.data(), r.num.mean_w.data(), r.num.var_acc.data(),
                                                   r.num.var_w.data(), r.den.mean_acc.data(), r.den.mean_w.data(), r.den.var_acc.data(),
                                                   r.den.var_w.data());
    sr_corpus_destroy(c);
    check(rc);
    r.f_num.resize(n);
    r.f_den.resize(n);
    return r;
  }

  // One sMBR E-step against THIS search's network (sr_bigram_smbr_statistics_corpus): the expected frame accuracy of the free network
  // with the bigram LM against ref_states (one reference mixture per frame of the corpus, for example an alignment; a value >= the
  // state count scores for none), every cost times scale (kappa).  f and accuracy per segment; num from the positive gamma, den from
  // the negative, ready for sr_model_create_from_mmi_statistics.  The training loop: align -> ref_states -> smbr_statistics ->
  // sr_model_create_from_mmi_statistics -> a LinearSearch on the NEW model.
  struct SmbrStatistics {
    std::vector<double> f, accuracy;
    Trainer::Statistics num, den;
  };
  SmbrStatistics smbr_statistics(Corpus const& corpus, std::vector<uint16_t> const& ref_states, double scale,
                                 double posterior_floor = 0.0) {
    const size_t n = corpus.get_corpus_size();
    const uint64_t frames = corpus.get_total_frame_count();
    if (ref_states.size() != frames) throw std::invalid_argument("smbr_statistics: one reference mixture per frame");
    std::vector<uint16_t> ref(ref_states);
    ref.push_back(0);  // (never empty: a null pointer is an error of the ABI)
    uint32_t n_mean = 0, n_var = 0;
    check(sr_model_tying_info(scorer_.handle(), &n_mean, &n_var));
    const size_t D = scorer_.dimension;
    SmbrStatistics r;
    r.f.assign(std::max<size_t>(n, 1), 0.0);
    r.accuracy.assign(std::max<size_t>(n, 1), 0.0);
    for (Trainer::Statistics* st : {&r.num, &r.den}) {
      st->mean_acc.assign(n_mean * D, 0.0); st->mean_w.assign(n_mean, 0.0);
      st->var_acc.assign(n_var * D, 0.0); st->var_w.assign(n_var, 0.0);
    }
    sr_corpus* c = nullptr;
    check(sr_corpus_upload(scorer_.handle(), corpus.features(), corpus.frame_offsets(), (uint32_t)n, &c));
    const int rc = sr_bigram_smbr_statistics_corpus(scorer_.handle(), c, net_, scorer_.gmm_kernel, scale, posterior_floor,
                                                    scorer_.max_approx() ? 1 : 0, ref.data(), r.f.data(), r.accuracy.data(),
                                                    r.num.mean_acc.data(), r.num.mean_w.data(), r.num.var_acc.data(),
                                                    r.num.var_w.data(), r.den.mean_acc.data(), r.den.mean_w.data(),
                                                    r.den.var_acc.data(), r.den.var_w.data());
    sr_corpus_destroy(c);
    check(rc);
    r.f.resize(n);
    r.accuracy.resize(n);
    return r;
  }

  // Per frame of the corpus the (at most max_items) mixtures with the largest |gamma| of the sMBR criterion (sr_bigram_accuracies_corpus),
  // gamma signed, beside f and accuracy per segment.
  struct Accuracies {
    std::vector<double> f, accuracy;
    std::vector<uint16_t> count, state;  // [frames], [frames x max_items]
    std::vector<double> weight;          // [frames x max_items]
  };
  Accuracies accuracies(Corpus const& corpus, std::vector<uint16_t> const& ref_states, double scale, uint32_t max_items,
                        double posterior_floor = 0.0) {
    const size_t n = corpus.get_corpus_size();
    const uint64_t frames = corpus.get_total_frame_count();
    if (ref_states.size() != frames) throw std::invalid_argument("accuracies: one reference mixture per frame");
    std::vector<uint16_t> ref(ref_states);
    ref.push_back(0);
    Accuracies r;
    r.f.assign(std::max<size_t>(n, 1), 0.0);
    r.accuracy.assign(std::max<size_t>(n, 1), 0.0);
    r.count.assign(std::max<uint64_t>(frames, 1), 0);
    r.state.assign(std::max<uint64_t>(frames, 1) * std::max<uint32_t>(max_items, 1), 0);
    r.weight.assign(r.state.size(), 0.0);
    sr_corpus* c = nullptr;
    check(sr_corpus_upload(scorer_.handle(), corpus.features(), corpus.frame_offsets(), (uint32_t)n, &c));
    const int rc = sr_bigram_accuracies_corpus(scorer_.handle(), c, net_, scorer_.gmm_kernel, scale, posterior_floor, max_items, ref.data(),
                                               r.f.data(), r.accuracy.data(), r.count.data(), r.state.data(), r.weight.data());
    sr_corpus_destroy(c);
    check(rc);
    r.f.resize(n);
    r.accuracy.resize(n);
    r.count.resize(frames);
    r.state.resize(frames * std::max<uint32_t>(max_items, 1));
    r.weight.resize(r.state.size());
    return r;
  }

  struct Hypothesis {
    std::vector<uint32_t> words;  // silence removed
    double cost;                  // of the string's cheapest lattice path
  };
  // Per segment the n_best cheapest distinct word strings among the paths of its word lattice over the search network without beams
  // (sr_bigram_word_lattice_corpus with this lattice_beam, then sr_bigram_lattice_nbest), cheapest first.  rescoring_lm (W x W, the
  // constructor's layout; null: the search's own table) and lm_scale price the word entries: another table is second-pass LM
  // rescoring of the lattice.  With the own table and lm_scale = 1 the first entry is the network's best path.
  std::vector<std::vector<Hypothesis> > recognize_nbest(Corpus const& corpus, uint32_t n_best,
                                                        double lattice_beam = std::numeric_limits<double>::infinity(),
                                                        std::vector<float> const* rescoring_lm = nullptr, double lm_scale = 1.0) {
    const size_t n = corpus.get_corpus_size();
    if (rescoring_lm && rescoring_lm->size() != lm_.size()) throw std::runtime_error("LinearSearch: rescoring lm must be W x W");
    std::vector<float> const& lm = rescoring_lm ? *rescoring_lm : lm_;
    sr_corpus* c = nullptr;
    check(sr_corpus_upload(scorer_.handle(), corpus.features(), corpus.frame_offsets(), (uint32_t)n, &c));
    std::vector<uint64_t> off(n + 1);
    std::vector<double> best(n + 1), fwd, bwd, am;
    std::vector<uint32_t> word, hist, pred, first, last;
    int rc = sr_bigram_word_lattice_corpus(scorer_.handle(), c, net_, scorer_.gmm_kernel, lattice_beam, 0, off.data(), best.data(), nullptr,
                                           nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr);
    if (rc == SR_OK) {
      const uint64_t cap = off[n] + 1;
      word.resize(cap); hist.resize(cap); pred.resize(cap); first.resize(cap); last.resize(cap);
      fwd.resize(cap); bwd.resize(cap); am.resize(cap);
      rc = sr_bigram_word_lattice_corpus(scorer_.handle(), c, net_, scorer_.gmm_kernel, lattice_beam, cap, off.data(), best.data(),
                                         word.data(), hist.data(), pred.data(), first.data(), last.data(), fwd.data(), bwd.data(),
                                         am.data());
    }
    sr_corpus_destroy(c);
    check(rc);
    std::vector<std::vector<Hypothesis> > out(n);
    for (size_t s = 0; s < n; s++) {
      const uint32_t T = (uint32_t)(corpus.frame_offsets()[s + 1] - corpus.frame_offsets()[s]);
      const uint64_t a = off[s], na = off[s + 1] - off[s];
      std::vector<uint32_t> words((size_t)n_best * (T ? T : 1));
      std::vector<uint64_t> hoff(n_best + 1);
      std::vector<double> cost(n_best);
      uint32_t count = 0;
      check(sr_bigram_lattice_nbest(T, na, word.data() + a, hist.data() + a, first.data() + a, last.data() + a, am.data() + a, n_words_,
                                    silence_, lm.data(), lm_scale, n_best, words.data(), words.size(), hoff.data(), cost.data(), &count));
      for (uint32_t k = 0; k < count; k++)
        out[s].push_back(Hypothesis{std::vector<uint32_t>(words.begin() + hoff[k], words.begin() + hoff[k + 1]), cost[k]});
    }
    return out;
  }

 private:
  MixtureModel& scorer_;
  float acoustic_pruning_, lm_pruning_;
  uint32_t n_words_, silence_;
  std::vector<float> lm_;
  sr_bigram* net_ = nullptr;
};

// ---- streaming LinearSearch: initialize / processFrame / getResult (LinearSearch.cc:489-520) over many concurrent utterances ------
// (sr_bigram_stream_*, srgpu.h).  begin() is initialize(); push() hands over new frames of one or several open utterances (one
// scoring and one search launch per call: processFrame for each of their frames); getResult() is the traceback after the frames
// pushed so far; end() returns it for the whole utterance -- what LinearSearch::recognize returns for it -- and frees the id.
// Errors are thrown as std::runtime_error with sr_last_error()'s text.
class StreamingLinearSearch {
 public:
  typedef LinearSearch::TracebackItem TracebackItem;
  typedef LinearSearch::Traceback Traceback;

  StreamingLinearSearch(MixtureModel& scorer, std::vector<std::vector<uint16_t> > const& linear_lexicon, uint32_t silence,
                        std::vector<float> const& lm, const float tdp[2][4], float acoustic_pruning = std::numeric_limits<float>::max(),
                        float lm_pruning = std::numeric_limits<float>::max(), uint32_t max_streams = 64, uint64_t max_frames = 65535)
      : max_frames_(max_frames) {
    std::vector<uint32_t> word_off(1, 0);
    std::vector<uint16_t> mixtures;
    for (size_t w = 0; w < linear_lexicon.size(); w++) {
      mixtures.insert(mixtures.end(), linear_lexicon[w].begin(), linear_lexicon[w].end());
      word_off.push_back((uint32_t)mixtures.size());
    }
    if (lm.size() != linear_lexicon.size() * linear_lexicon.size()) throw std::runtime_error("StreamingLinearSearch: lm must be W x W");
    check(sr_bigram_create(scorer.handle(), (uint32_t)linear_lexicon.size(), word_off.data(), mixtures.data(), silence, lm.data(),
                           &tdp[0][0], &net_));
    sr_bigram_params p = sr_bigram_params();  // zeroed, then field by field
    p.acoustic_pruning = acoustic_pruning;
    p.lm_pruning = lm_pruning;
    p.gmm_kernel = scorer.gmm_kernel;
    const int rc = sr_bigram_stream_open(scorer.handle(), net_, &p, max_streams, max_frames, &s_);
    if (rc != SR_OK) {
      const std::string msg = sr_last_error();
      sr_bigram_destroy(net_);
      throw std::runtime_error(msg);
    }
  }
  ~StreamingLinearSearch() {
    sr_bigram_stream_destroy(s_);  // before its search net
    sr_bigram_destroy(net_);
  }
  StreamingLinearSearch(StreamingLinearSearch const&) = delete;
  StreamingLinearSearch& operator=(StreamingLinearSearch const&) = delete;

  uint32_t begin() {
    uint32_t id = 0;
    check(sr_bigram_stream_begin(s_, &id));
    return id;
  }
  // n_frames new frames ([n_frames x dimension] float32) of one utterance
  void push(uint32_t id, const float* frames, size_t n_frames) {
    const uint64_t off[2] = {0, n_frames};
    check(sr_bigram_stream_push(s_, 1, &id, frames, off));
  }
  // new frames of several utterances back to back: ids[i] owns rows [frame_off[i], frame_off[i+1])
  // audio in, as StreamingRecognizer's (srgpu.h: sr_bigram_stream_push_audio)
  void set_frontend(FrontEnd& fe) { check(sr_bigram_stream_set_frontend(s_, fe.handle())); }
  void push_audio(uint32_t id, const int16_t* samples, size_t n_samples) {
    const uint64_t off[2] = {0, n_samples};
    check(sr_bigram_stream_push_audio(s_, 1, &id, samples, off, nullptr, 0, nullptr));
  }
  void finish_audio(uint32_t id) { check(sr_bigram_stream_finish_audio(s_, 1, &id, nullptr, 0, nullptr)); }
  // the utterance's VTLN warp, as StreamingRecognizer's (srgpu.h: sr_bigram_stream_set_warp)
  void set_warp(uint32_t id, uint32_t warp) { check(sr_bigram_stream_set_warp(s_, id, warp)); }
  // The pipeline (srgpu.h: sr_bigram_stream_set_projection): rows of in_dim columns are spliced with `context` neighbours on either side and
  // projected by M [dimension x ((2 context + 1) in_dim + 1)] (nullptr detaches; while no utterance is open), then the utterance's
  // W [dimension x (dimension + 1)] (nullptr clears it; between begin() and its first push) is applied, on the device.  push_rows:
  // n_frames rows of one utterance, in_dim columns with a projection; finish: no more follow, its last `context` rows are searched.
  void set_projection(uint32_t in_dim, uint32_t context, const double* M) { check(sr_bigram_stream_set_projection(s_, in_dim, context, M)); }
  void set_transform(uint32_t id, const double* W) { check(sr_bigram_stream_set_transform(s_, id, W)); }
  void push_rows(uint32_t id, const float* frames, size_t n_frames, bool finish = false) {
    const uint64_t off[2] = {0, n_frames};
    check(sr_bigram_stream_push_rows(s_, 1, &id, frames, off, finish ? 1 : 0, nullptr, 0, nullptr));
  }
  void push(std::vector<uint32_t> const& ids, const float* frames, std::vector<uint64_t> const& frame_off) {
    if (frame_off.size() != ids.size() + 1) throw std::runtime_error("StreamingLinearSearch::push: frame_off needs ids.size() + 1 entries");
    check(sr_bigram_stream_push(s_, (uint32_t)ids.size(), ids.data(), frames, frame_off.data()));
  }
  void getResult(uint32_t id, Traceback& result) { items(id, result, false); }
  void end(uint32_t id, Traceback& result) { items(id, result, true); }
  // the leading items of getResult(id) that no later frame can change (sr_bigram_stream_stable): a prefix of every later
  // getResult() and of end() that is not empty.  *commit (may be null): the time of the last of them, 0 if there is none
  void stable(uint32_t id, Traceback& result, uint32_t* commit = nullptr) {
    std::vector<uint32_t> words(max_frames_), times(max_frames_);
    std::vector<float> scores(max_frames_);
    uint64_t off[2] = {0, 0};
    uint32_t c = 0;
    check(sr_bigram_stream_stable(s_, 1, &id, words.data(), scores.data(), times.data(), words.size(), off, &c));
    if (commit) *commit = c;
    result.clear();
    for (uint64_t i = 0; i < off[1]; i++) result.push_back(TracebackItem{words[i], scores[i], times[i]});
  }

 private:
  void items(uint32_t id, Traceback& result, bool final_) {
    std::vector<uint32_t> words(max_frames_ + 1), times(max_frames_ + 1);
    std::vector<float> scores(max_frames_ + 1);
    uint32_t n = 0;
    if (final_)
      check(sr_bigram_stream_end(s_, id, words.data(), scores.data(), times.data(), (uint32_t)words.size(), &n));
    else
      check(sr_bigram_stream_partial(s_, id, words.data(), scores.data(), times.data(), (uint32_t)words.size(), &n, nullptr));
    result.clear();
    for (uint32_t i = 0; i < n; i++) result.push_back(TracebackItem{words[i], scores[i], times[i]});
  }
  const uint64_t max_frames_;
  sr_bigram* net_ = nullptr;
  sr_bigram_stream* s_ = nullptr;
};

}  // namespace sr
