// bigram_nbest_driver.cpp -- drives include/sr_sietill.hpp's sr::LinearSearch::recognize_nbest for tests/test_gpu_bigram_lattice.py.
//   <mixset> <dim> <case.bin>   case.bin: W, silence (u32), word_off[W+1] (u32), mixtures (u16), lm[W x W] (f32), tdp[8] (f32), the
//                               lattice beam (f64), n_best (u32), then the utterance count and per utterance T (u32) and its
//                               [T x dim] float32 frames.  Prints per hypothesis "hyp <utterance> <rank> <cost bits> <words ...>", the
//                               bits in hexadecimal.
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

int main(int argc, char** argv) {
  if (argc < 4) {
    fprintf(stderr, "usage: %s <mixset> <dim> <case.bin>\n", argv[0]);
    return 2;
  }
  try {
    const size_t dim = std::stoul(argv[2]);
    std::ifstream in(argv[3], std::ios::binary);
    const uint32_t W = rd<uint32_t>(in), sil = rd<uint32_t>(in);
    std::vector<uint32_t> word_off(W + 1);
    for (auto& x : word_off) x = rd<uint32_t>(in);
    std::vector<std::vector<uint16_t>> lexicon(W);
    for (uint32_t w = 0; w < W; w++) lexicon[w].resize(word_off[w + 1] - word_off[w]);
    for (uint32_t w = 0; w < W; w++)
      for (auto& m : lexicon[w]) m = rd<uint16_t>(in);
    std::vector<float> lm((size_t)W * W);
    for (auto& x : lm) x = rd<float>(in);
    float tdp[2][4];
    for (auto& row : tdp)
      for (auto& x : row) x = rd<float>(in);
    const double beam = rd<double>(in);
    const uint32_t n_best = rd<uint32_t>(in), n_utts = rd<uint32_t>(in);
    sr::Corpus corpus(dim);
    for (uint32_t u = 0; u < n_utts; u++) {
      const uint32_t T = rd<uint32_t>(in);
      std::vector<float> f((size_t)T * dim);
      in.read(reinterpret_cast<char*>(f.data()), sizeof(float) * f.size());
      corpus.add_segment(f.data(), T, {});
    }
    sr::MixtureModel mm(argv[1], dim, sr::MixtureModel::NO_POOLING, true, 0, SR_GMM_DEFAULT);
    sr::LinearSearch search(mm, lexicon, sil, lm, tdp);
    const auto hyps = search.recognize_nbest(corpus, n_best, beam);
    for (size_t u = 0; u < hyps.size(); u++)
      for (size_t k = 0; k < hyps[u].size(); k++) {
        uint64_t cb;
        memcpy(&cb, &hyps[u][k].cost, sizeof cb);
        printf("hyp %zu %zu %llx", u, k, (unsigned long long)cb);
        for (uint32_t w : hyps[u][k].words) printf(" %u", w);
        printf("\n");
      }
  } catch (std::exception const& e) {
    printf("error %s\n", e.what());
    return 1;
  }
  return 0;
}
