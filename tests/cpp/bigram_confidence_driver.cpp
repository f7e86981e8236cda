// bigram_confidence_driver.cpp -- drives include/sr_sietill.hpp's sr::LinearSearch::recognize_with_confidence for
// tests/test_gpu_bigram_posteriors.py.
//   conf <mixset> <dim> <case.bin>   case.bin: W, word_off[W+1] (u32), mixtures (u16), silence (u32), lm[W x W] (f32), tdp[8] (f32),
//                                    acoustic and LM beams (f32), gmm kernel (u32), scale (f64), then the utterance count and per
//                                    utterance T (u32) and its [T x dim] float32 frames.  Prints per item
//                                    "item <utterance> <word> <score bits> <time> <confidence bits>", the bits in hexadecimal.
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
  if (argc < 5 || strcmp(argv[1], "conf")) {
    fprintf(stderr, "usage: %s conf <mixset> <dim> <case.bin>\n", argv[0]);
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
    const float acp = rd<float>(in), lmp = rd<float>(in);
    const int kernel = (int)rd<uint32_t>(in);
    const double scale = rd<double>(in);
    const uint32_t n_utts = rd<uint32_t>(in);
    sr::Corpus corpus(dim);
    for (uint32_t u = 0; u < n_utts; u++) {
      const uint32_t T = rd<uint32_t>(in);
      std::vector<float> f((size_t)T * dim);
      in.read(reinterpret_cast<char*>(f.data()), sizeof(float) * f.size());
      corpus.add_segment(f.data(), T, {});
    }
    sr::MixtureModel mm(argv[2], dim, sr::MixtureModel::NO_POOLING, true, 0, kernel);
    sr::LinearSearch search(mm, lexicon, sil, lm, tdp, acp, lmp);
    std::vector<sr::LinearSearch::Traceback> results;
    std::vector<std::vector<double>> conf;
    search.recognize_with_confidence(corpus, scale, results, conf);
    for (size_t u = 0; u < results.size(); u++)
      for (size_t i = 0; i < results[u].size(); i++) {
        uint32_t sb;
        uint64_t cb;
        memcpy(&sb, &results[u][i].score, sizeof sb);
        memcpy(&cb, &conf[u][i], sizeof cb);
        printf("item %zu %u %x %u %llx\n", u, results[u][i].word, sb, results[u][i].time, (unsigned long long)cb);
      }
  } catch (std::exception const& e) {
    printf("error %s\n", e.what());
    return 1;
  }
  return 0;
}
