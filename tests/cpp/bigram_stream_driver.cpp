// bigram_stream_driver.cpp -- drives include/sr_sietill.hpp's sr::StreamingLinearSearch for tests/test_gpu_bigram_stream.py.
//   stream <mixset> <dim> <case.bin>   case.bin: W, word_off[W+1] (u32), mixtures (u16), silence (u32), lm[W x W] (f32), tdp[8] (f32),
//                                      acoustic and LM beams (f32), gmm kernel, piece (u32), then per utterance T (u32) and its
//                                      [T x dim] float32 frames.  Feeds all utterances at once, `piece` frames of each per push, and
//                                      prints per utterance "partial <u> <items after the first push>" and "final <u> <items>", every
//                                      item as three hexadecimal numbers: word, score bits, time.
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

static void print(const char* tag, size_t u, sr::StreamingLinearSearch::Traceback const& tb) {
  printf("%s %zu", tag, u);
  for (auto const& it : tb) {
    uint32_t bits;
    memcpy(&bits, &it.score, sizeof bits);
    printf(" %x %x %x", it.word, bits, it.time);
  }
  printf("\n");
}

int main(int argc, char** argv) {
  if (argc < 5 || strcmp(argv[1], "stream")) {
    fprintf(stderr, "usage: %s stream <mixset> <dim> <case.bin>\n", argv[0]);
    return 2;
  }
  try {
    const size_t dim = std::stoul(argv[3]);
    std::ifstream in(argv[4], std::ios::binary);
    const uint32_t W = rd<uint32_t>(in);
    std::vector<uint32_t> word_off(W + 1);
    for (auto& x : word_off) x = rd<uint32_t>(in);
    std::vector<std::vector<uint16_t>> lexicon(W);
    for (uint32_t w = 0; w < W; w++)
      for (uint32_t i = word_off[w]; i < word_off[w + 1]; i++) lexicon[w].push_back(0);
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
    const uint32_t piece = rd<uint32_t>(in);
    const uint32_t n_utts = rd<uint32_t>(in);
    std::vector<std::vector<float>> feats(n_utts);
    for (uint32_t u = 0; u < n_utts; u++) {
      const uint32_t T = rd<uint32_t>(in);
      feats[u].resize((size_t)T * dim);
      in.read(reinterpret_cast<char*>(feats[u].data()), sizeof(float) * feats[u].size());
    }
    sr::MixtureModel mm(argv[2], dim, sr::MixtureModel::NO_POOLING, true, 0, kernel);
    sr::StreamingLinearSearch search(mm, lexicon, sil, lm, tdp, acp, lmp, n_utts, 4096);
    std::vector<uint32_t> ids;
    for (uint32_t u = 0; u < n_utts; u++) ids.push_back(search.begin());  // initialize()
    sr::StreamingLinearSearch::Traceback tb;
    for (size_t t0 = 0, round = 0;; t0 += piece, round++) {
      std::vector<uint32_t> who;
      std::vector<uint64_t> off(1, 0);
      std::vector<float> buf;
      for (uint32_t u = 0; u < n_utts; u++) {
        const size_t T = feats[u].size() / dim;
        if (t0 >= T) continue;
        const size_t k = std::min<size_t>(piece, T - t0);
        who.push_back(ids[u]);
        buf.insert(buf.end(), feats[u].begin() + t0 * dim, feats[u].begin() + (t0 + k) * dim);
        off.push_back(off.back() + k);
      }
      if (who.empty()) break;
      search.push(who, buf.data(), off);  // processFrame() for each of the pushed frames
      if (round == 0)
        for (uint32_t u = 0; u < n_utts; u++) {
          search.getResult(ids[u], tb);
          print("partial", u, tb);
        }
    }
    for (uint32_t u = 0; u < n_utts; u++) {
      search.end(ids[u], tb);
      print("final", u, tb);
    }
    try {
      search.end(ids[0], tb);
      printf("ended_again accepted\n");
    } catch (std::runtime_error const& e) {
      printf("ended_again refused\n");
    }
  } catch (std::exception const& e) {
    printf("error %s\n", e.what());
    return 1;
  }
  return 0;
}
