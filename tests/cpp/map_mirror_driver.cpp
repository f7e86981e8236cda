// map_mirror_driver.cpp -- drives include/sr_sietill.hpp's sr::MapAdaptation for tests/test_gpu_map.py; links against libsrgpu.so.
//   map_mirror_driver <mixset> <dim> <case.bin>   case.bin as fmllr_driver's "adapt" case, with f64 tau in min_count's place and f64
//                                                 tau_w after it.  Prints "off <ent_off ...>", "dens <...>", "occ <hex bits ...>",
//                                                 "x <hex bits ...>", then per speaker "means <s> <hex bits ...>" and "logw <s> <hex bits
//                                                 ...>" of adapted_model(s, tau, tau_w).
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

static void hex_line(const char* name, const std::vector<double>& v) {
  printf("%s", name);
  for (double d : v) {
    unsigned long long b;
    memcpy(&b, &d, sizeof b);
    printf(" %llx", b);
  }
  printf("\n");
}

int main(int argc, char** argv) {
  try {
    if (argc != 4) { fprintf(stderr, "usage: %s <mixset> <dim> <case.bin>\n", argv[0]); return 2; }
    const size_t dim = std::stoul(argv[2]);
    std::ifstream in(argv[3], std::ios::binary);
    sr::Lexicon lex;
    const uint32_t n_words = rd<uint32_t>(in);
    std::vector<std::pair<uint16_t, uint16_t>> ws(n_words);
    for (auto& w : ws) { w.first = rd<uint16_t>(in); w.second = rd<uint16_t>(in); }
    const uint32_t sil = rd<uint32_t>(in);
    for (uint32_t w = 0; w < n_words; w++) lex.add_word("w" + std::to_string(w), ws[w].first, ws[w].second, w == sil);
    const double tl = rd<double>(in), tf = rd<double>(in), ts = rd<double>(in), tau = rd<double>(in), tau_w = rd<double>(in);
    sr::MixtureModel mm(argv[1], dim, sr::MixtureModel::NO_POOLING, true);
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
    if (!in) throw std::runtime_error("short case file");
    sr::Trainer trainer(lex, mm, tdp, 50.0, false);
    sr::MapAdaptation ad(trainer, mm);
    sr::MapAdaptation::Result r = ad.adapt(corpus);
    printf("off");
    for (uint64_t e : r.ent_off) printf(" %llu", (unsigned long long)e);
    printf("\ndens");
    for (uint32_t d : r.dens) printf(" %u", d);
    printf("\n");
    hex_line("occ", r.occ);
    hex_line("x", r.x);
    uint32_t d_ = 0, s_ = 0;
    uint64_t C = 0;
    sr::check(sr_model_info(mm.handle(), &d_, &s_, &C));
    std::vector<double> means(C * dim), iv(C * dim), norm(C), logw(C);
    for (uint32_t s = 0; s < r.n_speakers; s++) {
      std::shared_ptr<sr_model> a = ad.adapted_model(r, s, tau, tau_w);
      sr::check(sr_model_tables(a.get(), means.data(), iv.data(), norm.data(), logw.data()));
      hex_line(("means " + std::to_string(s)).c_str(), means);
      hex_line(("logw " + std::to_string(s)).c_str(), logw);
    }
    return 0;
  } catch (std::exception const& e) {
    printf("error %s\n", e.what());
    return 1;
  }
}
