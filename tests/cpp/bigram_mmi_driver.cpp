// bigram_mmi_driver.cpp -- drives include/sr_sietill.hpp's sr::LinearSearch::mmi_statistics for tests/test_gpu_bigram_mmi.py.
//   mmi <mixset> <dim> <case.bin>   case.bin: W, word_off[W+1] (u32), mixtures (u16), silence (u32), lm[W x W] (f32), tdp[8] (f32),
//                                   gmm kernel (u32), scale and posterior floor (f64), then the utterance count and per utterance the
//                                   transcript length (u32), its word ids (u32), T (u32) and the [T x dim] float32 frames.  Prints
//                                   "cost <utterance> <F_num bits> <F_den bits>" per utterance and "stat <side> <array> <index> <bits>"
//                                   for every element of both statistics sets, the bits in hexadecimal.
#include <cstdio>
#include <cstring>
#include <fstream>
#include <iostream>
#include <string>

#include "sr_sietill.hpp"

template <typename T>
static T rd(std::istream& in) {
  T v;
  in.read(reinterpret_cast<char*>(&v), sizeof v);
  return v;
}

static unsigned long long bits(double x) {
  uint64_t b;
  memcpy(&b, &x, sizeof b);
  return (unsigned long long)b;
}

int main(int argc, char** argv) {
  if (argc < 5 || strcmp(argv[1], "mmi")) {
    fprintf(stderr, "usage: %s mmi <mixset> <dim> <case.bin>\n", argv[0]);
    return 2;
  }
  try {
    const size_t dim = std::stoul(argv[3]);
    std::ifstream in(argv[4], std::ios::binary);
    const uint32_t W = rd<uint32_t>(in);
    std::vector<uint32_t> word_off(W + 1);
    for (auto& x : word_off) x = rd<uint32_t>(in);
    std::vector<std::vector<uint16_t>> lexicon(W);
    for (uint32_t w = 0; w < W; w++) lexicon[w].resize(word_off[w + 1] - word_off[w]);
    for (uint32_t w = 0; w < W; w++)
      for (auto& m : lexicon[w]) m = rd<uint16_t>(in);
    const uint32_t sil = rd<uint32_t>(in);
    std::vector<float> lm((size_t)W * W);
    for (auto& x : lm) x = rd<float>(in);
    float tdp[2][4];
    for (auto& row : tdp)
      for (auto& x : row) x = rd<float>(in);
    const int kernel = (int)rd<uint32_t>(in);
    const double scale = rd<double>(in), floor = rd<double>(in);
    const uint32_t n_utts = rd<uint32_t>(in);
    sr::Corpus corpus(dim);
    std::vector<std::vector<uint32_t>> transcripts(n_utts);
    for (uint32_t u = 0; u < n_utts; u++) {
      transcripts[u].resize(rd<uint32_t>(in));
      for (auto& w : transcripts[u]) w = rd<uint32_t>(in);
      const uint32_t T = rd<uint32_t>(in);
      std::vector<float> f((size_t)T * dim);
      in.read(reinterpret_cast<char*>(f.data()), sizeof(float) * f.size());
      corpus.add_segment(f.data(), T, {});
    }
    sr::MixtureModel mm(argv[2], dim, sr::MixtureModel::NO_POOLING, true, 0, kernel);
    sr::LinearSearch search(mm, lexicon, sil, lm, tdp);
    const sr::LinearSearch::MmiStatistics r = search.mmi_statistics(corpus, transcripts, scale, floor);
    for (size_t u = 0; u < r.f_num.size(); u++) printf("cost %zu %llx %llx\n", u, bits(r.f_num[u]), bits(r.f_den[u]));
    const sr::Trainer::Statistics* sides[2] = {&r.num, &r.den};
    for (int s = 0; s < 2; s++) {
      const std::vector<double>* arrays[4] = {&sides[s]->mean_acc, &sides[s]->mean_w, &sides[s]->var_acc, &sides[s]->var_w};
      for (int a = 0; a < 4; a++)
        for (size_t i = 0; i < arrays[a]->size(); i++) printf("stat %d %d %zu %llx\n", s, a, i, bits((*arrays[a])[i]));
    }
  } catch (std::exception const& e) {
    printf("error %s\n", e.what());
    return 1;
  }
  return 0;
}
