// bigram_smbr_driver.cpp -- drives include/sr_sietill.hpp's sr::LinearSearch::smbr_statistics and ::accuracies for
// tests/test_gpu_bigram_smbr.py.
//   smbr <mixset> <dim> <case.bin>  case.bin: W, word_off[W+1] (u32), mixtures (u16), silence (u32), lm[W x W] (f32), tdp[8] (f32),
//                                   gmm kernel (u32), scale and posterior floor (f64), max_items (u32), then the utterance count and
//                                   per utterance T (u32), the [T x dim] float32 frames and the T reference mixtures (u16).  Prints
//                                   "cost <utterance> <F bits> <Abar bits>" per utterance, "stat <side> <array> <index> <bits>" for
//                                   every element of both statistics sets and "item <frame> <count> (<state> <weight bits>)*" per
//                                   frame, the bits in hexadecimal.
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
  if (argc < 5 || strcmp(argv[1], "smbr")) {
    fprintf(stderr, "usage: %s smbr <mixset> <dim> <case.bin>\n", argv[0]);
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
    const uint32_t max_items = rd<uint32_t>(in);
    const uint32_t n_utts = rd<uint32_t>(in);
    sr::Corpus corpus(dim);
    std::vector<uint16_t> ref;
    for (uint32_t u = 0; u < n_utts; u++) {
      const uint32_t T = rd<uint32_t>(in);
      std::vector<float> f((size_t)T * dim);
      in.read(reinterpret_cast<char*>(f.data()), sizeof(float) * f.size());
      corpus.add_segment(f.data(), T, {});
      for (uint32_t t = 0; t < T; t++) ref.push_back(rd<uint16_t>(in));
    }
    sr::MixtureModel mm(argv[2], dim, sr::MixtureModel::NO_POOLING, true, 0, kernel);
    sr::LinearSearch search(mm, lexicon, sil, lm, tdp);
    const sr::LinearSearch::SmbrStatistics r = search.smbr_statistics(corpus, ref, scale, floor);
    for (size_t u = 0; u < r.f.size(); u++) printf("cost %zu %llx %llx\n", u, bits(r.f[u]), bits(r.accuracy[u]));
    const sr::Trainer::Statistics* sides[2] = {&r.num, &r.den};
    for (int s = 0; s < 2; s++) {
      const std::vector<double>* arrays[4] = {&sides[s]->mean_acc, &sides[s]->mean_w, &sides[s]->var_acc, &sides[s]->var_w};
      for (int a = 0; a < 4; a++)
        for (size_t i = 0; i < arrays[a]->size(); i++) printf("stat %d %d %zu %llx\n", s, a, i, bits((*arrays[a])[i]));
    }
    const sr::LinearSearch::Accuracies a = search.accuracies(corpus, ref, scale, max_items, floor);
    for (size_t t = 0; t < a.count.size(); t++) {
      printf("item %zu %u", t, (unsigned)a.count[t]);
      for (uint32_t i = 0; i < a.count[t]; i++) printf(" %u %llx", (unsigned)a.state[t * max_items + i], bits(a.weight[t * max_items + i]));
      printf("\n");
    }
  } catch (std::exception const& e) {
    printf("error %s\n", e.what());
    return 1;
  }
  return 0;
}
