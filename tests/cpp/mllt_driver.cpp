// mllt_driver.cpp -- drives include/sr_sietill.hpp's sr::Mllt for tests/test_mllt_cpu.py (compilation) and tests/test_gpu_mllt.py.
//   estimate <stats.bin>            host only.  stats.bin: u32 dim, u32 n_sweeps, f64 min_count, f64 beta, f64 G[D * D * D].  Prints
//                                   "status <st> logdet <hex bits> aux <hex bits of the last Q>" and "A <hex bits> ...".
//   adapt <mixset> <dim> <case.bin> device.  case.bin as fmllr_driver's (the speaker of an utterance is read and ignored).  Prints the
//                                   same lines, "checksum <rotating xor of the adapted features' bits>", "resident equal" when the
//                                   adapted handle scores like an upload of those features, and "scores <rotating xor of the bits of
//                                   the adapted model's exact scores of the adapted features>".
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

static void print(sr::Mllt::Result const& r) {
  printf("status %d logdet %llx aux %llx\nA", r.status, bits(r.logdet), bits(r.aux.back()));
  for (double v : r.A) printf(" %llx", bits(v));
  printf("\n");
}

int main(int argc, char** argv) {
  try {
    if (argc == 3 && !strcmp(argv[1], "estimate")) {
      std::ifstream in(argv[2], std::ios::binary);
      const uint32_t dim = rd<uint32_t>(in), sweeps = rd<uint32_t>(in);
      const double min_count = rd<double>(in), beta = rd<double>(in);
      std::vector<double> G((size_t)dim * dim * dim);
      in.read(reinterpret_cast<char*>(G.data()), sizeof(double) * G.size());
      if (!in) throw std::runtime_error("short statistics file");
      sr::Mllt::Result r;
      sr::Mllt::estimate(dim, beta, G, sweeps, min_count, r);
      print(r);
      return 0;
    }
    if (argc == 5 && !strcmp(argv[1], "adapt")) {
      const size_t dim = std::stoul(argv[3]);
      std::ifstream in(argv[4], std::ios::binary);
      sr::Lexicon lex;
      const uint32_t n_words = rd<uint32_t>(in);
      std::vector<std::pair<uint16_t, uint16_t>> ws(n_words);
      for (auto& w : ws) { w.first = rd<uint16_t>(in); w.second = rd<uint16_t>(in); }
      const uint32_t sil = rd<uint32_t>(in);
      for (uint32_t w = 0; w < n_words; w++) lex.add_word("w" + std::to_string(w), ws[w].first, ws[w].second, w == sil);
      const double tl = rd<double>(in), tf = rd<double>(in), ts = rd<double>(in), min_count = rd<double>(in);
      sr::MixtureModel mm(argv[2], dim, sr::MixtureModel::NO_POOLING, true);
      sr::TdpModel tdp(lex.get_silence_automaton().first_state(), tl, tf, ts);
      sr::Corpus corpus(dim);
      const uint32_t n_utts = rd<uint32_t>(in);
      for (uint32_t u = 0; u < n_utts; u++) {
        const uint32_t speaker = rd<uint32_t>(in);
        std::vector<sr::WordIdx> orth(rd<uint32_t>(in));
        for (auto& w : orth) w = rd<uint32_t>(in);
        const uint32_t T = rd<uint32_t>(in);
        std::vector<float> f((size_t)T * dim);
        in.read(reinterpret_cast<char*>(f.data()), sizeof(float) * f.size());
        corpus.add_segment(f.data(), T, orth, speaker);
      }
      sr::Trainer trainer(lex, mm, tdp, 50.0, false);
      sr::Mllt mllt(trainer, mm, 10, min_count);
      sr::Mllt::Result r = mllt.adapt(corpus);
      print(r);
      unsigned long long x = 0;
      for (float v : r.features) { unsigned int b; memcpy(&b, &v, sizeof b); x ^= b; x = (x << 1) | (x >> 63); }
      printf("checksum %llx\n", x);
      // the resident adapted corpus against an upload of the returned features: the base model's exact scores of both, bit for bit
      const uint64_t F = corpus.get_total_frame_count();
      std::vector<double> a(F * mm.num_mixtures()), b(a.size());
      sr_corpus* up = nullptr;
      sr::check(sr_corpus_upload(mm.handle(), r.features.data(), corpus.frame_offsets(), n_utts, &up));
      int rc = sr_score_corpus(mm.handle(), up, SR_GMM_EXACT, b.data());
      sr_corpus_destroy(up);
      sr::check(rc);
      sr::check(sr_score_corpus(mm.handle(), r.adapted.get(), SR_GMM_EXACT, a.data()));
      printf("resident %s\n", memcmp(a.data(), b.data(), sizeof(double) * a.size()) ? "differs" : "equal");
      // the adapted pair: the adapted features under the adapted model
      sr::check(sr_corpus_upload(r.model.get(), r.features.data(), corpus.frame_offsets(), n_utts, &up));
      rc = sr_score_corpus(r.model.get(), up, SR_GMM_EXACT, a.data());
      sr_corpus_destroy(up);
      sr::check(rc);
      x = 0;
      for (double v : a) { x ^= bits(v); x = (x << 1) | (x >> 63); }
      printf("scores %llx\n", x);
      return 0;
    }
    fprintf(stderr, "usage: %s estimate <stats.bin> | adapt <mixset> <dim> <case.bin>\n", argv[0]);
    return 2;
  } catch (std::exception const& e) {
    printf("error %s\n", e.what());
    return 1;
  }
}
