// stream_trim_driver.cpp -- include/sr_sietill.hpp's StreamingRecognizer::trim against the C calls of srgpu.h on one utterance, as
// INTEGRATION.md 5d uses it (tests/test_stream_trim_cpu.py compiles it for syntax and types, tests/test_gpu_stream_trim.py runs it).
//   run <mixset> <dim> <case.bin>   the utterance in pieces through a StreamingRecognizer and through sr_stream_* with the same
//                                   max_frames, a trim after every push; per push "push <frames> <dropped> <words...>" of the
//                                   mirror, "final <words...>", and "same" when every figure of the C calls agreed (else "DIFF ...")
//   case.bin: u32 n_words, (u16 states, u16 reps) per word, u32 silence word, f64 tdp[3], f64 beam, f64 word penalty, u32 gmm kernel,
//             u32 max_frames, u32 piece, u32 T, f32 feats[T x dim]
#include <cstdio>
#include <cstring>
#include <fstream>
#include <string>
#include <vector>

#include "sr_sietill.hpp"

template <typename T>
static T rd(std::istream& in) {
  T v;
  in.read(reinterpret_cast<char*>(&v), sizeof v);
  return v;
}

// the recipe of INTEGRATION.md 5d: push; trim every `every` pushes; endpoint on the silence count
static std::vector<sr::WordIdx> feed_endless(sr::StreamingRecognizer& rec, const float* frames, size_t n_frames, size_t dim, size_t piece,
                                             size_t every, uint32_t hangover) {
  const uint32_t id = rec.begin();
  size_t pushes = 0;
  for (size_t t = 0; t < n_frames; t += piece) {
    rec.push(id, frames + t * dim, t + piece <= n_frames ? piece : n_frames - t);
    if (++pushes % every == 0) rec.trim(id);
    uint32_t silence = 0;
    rec.stable(id, nullptr, &silence);
    if (silence >= hangover) break;
  }
  return rec.end(id);
}

static int fail_c(const char* what) {
  printf("error %s: %s\n", what, sr_last_error());
  return 2;
}

int main(int argc, char** argv) {
  (void)&feed_endless;
  if (argc < 5 || strcmp(argv[1], "run")) return 0;
  try {
    const size_t dim = std::stoul(argv[3]);
    std::ifstream in(argv[4], std::ios::binary);
    sr::Lexicon lex;
    const uint32_t n_words = rd<uint32_t>(in);
    std::vector<std::pair<uint16_t, uint16_t>> ws(n_words);
    for (auto& w : ws) { w.first = rd<uint16_t>(in); w.second = rd<uint16_t>(in); }
    const uint32_t sil = rd<uint32_t>(in);
    for (uint32_t w = 0; w < n_words; w++) lex.add_word("w" + std::to_string(w), ws[w].first, ws[w].second, w == sil);
    const double tl = rd<double>(in), tf = rd<double>(in), ts = rd<double>(in), beam = rd<double>(in), wp = rd<double>(in);
    const int kernel = (int)rd<uint32_t>(in);
    const uint32_t max_frames = rd<uint32_t>(in), piece = rd<uint32_t>(in), T = rd<uint32_t>(in);
    std::vector<float> feats((size_t)T * dim);
    in.read(reinterpret_cast<char*>(feats.data()), sizeof(float) * feats.size());
    if (!in || piece == 0) { printf("error case file\n"); return 2; }
    sr::MixtureModel mm(argv[2], dim, sr::MixtureModel::NO_POOLING, true, 0, kernel);
    sr::TdpModel tdp(lex.get_silence_automaton().first_state(), tl, tf, ts);
    sr::StreamingRecognizer rec(lex, mm, tdp, beam, wp, 1, max_frames);

    // the same set through the C calls
    std::vector<uint32_t> word_off(1, 0);
    std::vector<uint16_t> automaton;
    for (size_t w = 0; w < lex.num_words(); w++) {
      auto const& a = lex.get_automaton_for_word(w);
      automaton.insert(automaton.end(), a.states.begin(), a.states.end());
      word_off.push_back((uint32_t)automaton.size());
    }
    const double tdp3[3] = {tl, tf, ts};
    sr_lexicon* net = nullptr;
    if (sr_lexicon_create(mm.handle(), n_words, word_off.data(), automaton.data(), sil, tdp3, tdp.silence_state, &net)) return fail_c("lexicon");
    sr_search_params p = sr_search_params();
    p.am_threshold = beam; p.word_penalty = wp; p.gmm_kernel = kernel;
    sr_stream* cs = nullptr;
    if (sr_stream_open(mm.handle(), net, &p, 1, max_frames, &cs)) return fail_c("open");
    uint32_t cid = 0;
    if (sr_stream_begin(cs, &cid)) return fail_c("begin");

    const uint32_t id = rec.begin();
    std::string diff;
    std::vector<uint32_t> cw(T + 1);
    uint64_t total_dropped = 0;
    for (uint32_t t = 0; t < T; t += piece) {
      const uint32_t k = t + piece <= T ? piece : T - t;
      rec.push(id, feats.data() + (size_t)t * dim, k);
      const uint32_t dropped = rec.trim(id);
      const std::vector<sr::WordIdx> words = rec.partial(id);
      total_dropped += dropped;
      printf("push %u %u", t + k, dropped);
      for (auto w : words) printf(" %zu", (size_t)w);
      printf("\n");
      const uint64_t off[2] = {0, k};
      uint32_t cdropped = 0xFFFFFFFFu, cn = 0;
      uint64_t cframes = 0;
      if (sr_stream_push(cs, 1, &cid, feats.data() + (size_t)t * dim, off)) return fail_c("push");
      if (sr_stream_trim(cs, 1, &cid, &cdropped)) return fail_c("trim");
      if (sr_stream_partial(cs, cid, cw.data(), (uint32_t)cw.size(), &cn, &cframes)) return fail_c("partial");
      bool same = cdropped == dropped && cn == words.size() && cframes == t + k;
      for (uint32_t i = 0; same && i < cn; i++) same = cw[i] == words[i];
      if (!same && diff.empty()) diff = "at frame " + std::to_string(t + k);
    }
    const std::vector<sr::WordIdx> fin = rec.end(id);
    uint32_t cn = 0;
    if (sr_stream_end(cs, cid, cw.data(), (uint32_t)cw.size(), &cn, nullptr, nullptr, nullptr)) return fail_c("end");
    bool same = cn == fin.size();
    for (uint32_t i = 0; same && i < cn; i++) same = cw[i] == fin[i];
    if (!same && diff.empty()) diff = "at the end";
    printf("final");
    for (auto w : fin) printf(" %zu", (size_t)w);
    printf("\ndropped %llu\n", (unsigned long long)total_dropped);
    printf(diff.empty() ? "same\n" : "DIFF %s\n", diff.c_str());
    sr_stream_destroy(cs);
    sr_lexicon_destroy(net);
  } catch (std::exception const& e) {
    printf("error %s\n", e.what());
    return 2;
  }
  return 0;
}
