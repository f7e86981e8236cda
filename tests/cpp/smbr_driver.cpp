// smbr_driver.cpp -- drives include/sr_sietill.hpp's sr::Trainer::smbr_iteration for tests/test_gpu_smbr.py.
//   smbr <mixset> <dim> <case.bin>   case.bin: u32 n_words, per word (u16 states, u16 repetitions), u32 silence word, f64 loop,
//                                    forward, skip, f64 word penalty, scale, E, tau, u32 n_utts, per utterance u32 T,
//                                    f32 feats[T * dim], u16 reference mixtures[T].  Runs two iterations and prints
//                                    "accuracy <k> <hex bits> <frames>": sum Abar under the model iteration k starts from.
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

static unsigned long long bits(double d) {
  unsigned long long b;
  memcpy(&b, &d, sizeof b);
  return b;
}

int main(int argc, char** argv) {
  if (argc < 5 || strcmp(argv[1], "smbr")) {
    fprintf(stderr, "usage: %s smbr <mixset> <dim> <case.bin>\n", argv[0]);
    return 2;
  }
  try {
    const size_t dim = std::stoul(argv[3]);
    std::ifstream in(argv[4], std::ios::binary);
    sr::Lexicon lex;
    const uint32_t n_words = rd<uint32_t>(in);
    std::vector<std::pair<uint16_t, uint16_t>> ws(n_words);
    for (auto& w : ws) { w.first = rd<uint16_t>(in); w.second = rd<uint16_t>(in); }
    const uint32_t sil = rd<uint32_t>(in);
    for (uint32_t w = 0; w < n_words; w++) lex.add_word("w" + std::to_string(w), ws[w].first, ws[w].second, w == sil);
    const double tl = rd<double>(in), tf = rd<double>(in), ts = rd<double>(in);
    const double wp = rd<double>(in), scale = rd<double>(in), E = rd<double>(in), tau = rd<double>(in);
    sr::MixtureModel mm(argv[2], dim, sr::MixtureModel::NO_POOLING, true);
    sr::TdpModel tdp(lex.get_silence_automaton().first_state(), tl, tf, ts);
    sr::Corpus corpus(dim);
    std::vector<sr::AlignmentItem> alignment;
    const uint32_t n_utts = rd<uint32_t>(in);
    for (uint32_t u = 0; u < n_utts; u++) {
      const uint32_t T = rd<uint32_t>(in);
      std::vector<float> f((size_t)T * dim);
      in.read(reinterpret_cast<char*>(f.data()), sizeof(float) * f.size());
      corpus.add_segment(f.data(), T, std::vector<sr::WordIdx>());
      for (uint32_t t = 0; t < T; t++) {
        sr::AlignmentItem it;
        it.count = 1; it.state = rd<uint16_t>(in); it.weight = 1.0f;
        alignment.push_back(it);
      }
    }
    double acc = 0.0;
    uint64_t frames = 0;
    sr::Trainer first(lex, mm, tdp);
    std::unique_ptr<sr::MixtureModel> next = first.smbr_iteration(corpus, alignment, scale, E, tau, &acc, &frames, wp, 0.0, 1e-3);
    printf("accuracy 0 %llx %llu\n", bits(acc), (unsigned long long)frames);
    sr::Trainer second(lex, *next, tdp);
    second.smbr_iteration(corpus, alignment, scale, E, tau, &acc, &frames, wp, 0.0, 1e-3);
    printf("accuracy 1 %llx %llu\n", bits(acc), (unsigned long long)frames);
  } catch (std::exception const& e) {
    printf("error %s\n", e.what());
    return 1;
  }
  return 0;
}
