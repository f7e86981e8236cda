// nbest_driver.cpp -- drives include/sr_sietill.hpp's sr::Recognizer::recognize_nbest for tests/test_gpu_word_lattice.py.
//   nbest <mixset> <dim> <case.bin>   case.bin: u32 n_words, per word (u16 states, u16 repetitions), u32 silence word, f64 loop,
//                                     forward, skip, f64 word_penalty, lattice_beam, u32 n_best, u32 n_utts, per utterance u32 T,
//                                     f32 feats[T * dim].  Prints "hyp <u> <k> <cost hex bits> <word> ..." per hypothesis.
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
  if (argc < 5 || strcmp(argv[1], "nbest")) {
    fprintf(stderr, "usage: %s nbest <mixset> <dim> <case.bin>\n", argv[0]);
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
    const double word_penalty = rd<double>(in), lattice_beam = rd<double>(in);
    const uint32_t n_best = rd<uint32_t>(in);
    sr::MixtureModel mm(argv[2], dim, sr::MixtureModel::NO_POOLING, true);
    sr::TdpModel tdp(lex.get_silence_automaton().first_state(), tl, tf, ts);
    sr::Corpus corpus(dim);
    const uint32_t n_utts = rd<uint32_t>(in);
    for (uint32_t u = 0; u < n_utts; u++) {
      const uint32_t T = rd<uint32_t>(in);
      std::vector<float> f((size_t)T * dim);
      in.read(reinterpret_cast<char*>(f.data()), sizeof(float) * f.size());
      corpus.add_segment(f.data(), T, std::vector<sr::WordIdx>());
    }
    sr::Recognizer rec(lex, mm, tdp, 20.0, word_penalty);
    const auto out = rec.recognize_nbest(corpus, n_best, lattice_beam);
    for (size_t u = 0; u < out.size(); u++)
      for (size_t k = 0; k < out[u].size(); k++) {
        printf("hyp %zu %zu %llx", u, k, bits(out[u][k].cost));
        for (auto w : out[u][k].words) printf(" %u", (unsigned)w);
        printf("\n");
      }
  } catch (std::exception const& e) {
    printf("error %s\n", e.what());
    return 1;
  }
  return 0;
}
