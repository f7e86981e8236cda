// stream_driver.cpp -- drives include/sr_sietill.hpp's sr::StreamingRecognizer for tests/test_gpu_stream.py.
//   stream <mixset> <dim> <case.bin>   case.bin as host_mirror_driver's "run" reads it, without the alignment part.  Feeds all
//                                      utterances at once, `piece` frames of each per push, and prints per utterance
//                                      "partial <u> <words after the first push>" and "final <u> <words>".
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

static void print(const char* tag, size_t u, std::vector<sr::WordIdx> const& w) {
  printf("%s %zu", tag, u);
  for (sr::WordIdx x : w) printf(" %zu", x);
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
    sr::Lexicon lex;
    const uint32_t n_words = rd<uint32_t>(in);
    std::vector<std::pair<uint16_t, uint16_t>> ws(n_words);
    for (auto& w : ws) { w.first = rd<uint16_t>(in); w.second = rd<uint16_t>(in); }
    const uint32_t sil = rd<uint32_t>(in);
    for (uint32_t w = 0; w < n_words; w++) lex.add_word("w" + std::to_string(w), ws[w].first, ws[w].second, w == sil);
    const double tl = rd<double>(in), tf = rd<double>(in), ts = rd<double>(in), beam = rd<double>(in), wp = rd<double>(in);
    const int kernel = (int)rd<uint32_t>(in);
    const uint32_t piece = rd<uint32_t>(in);
    sr::MixtureModel mm(argv[2], dim, sr::MixtureModel::NO_POOLING, true, 0, kernel);
    sr::TdpModel tdp(lex.get_silence_automaton().first_state(), tl, tf, ts);
    const uint32_t n_utts = rd<uint32_t>(in);
    std::vector<std::vector<float>> feats(n_utts);
    for (uint32_t u = 0; u < n_utts; u++) {
      const uint32_t T = rd<uint32_t>(in);
      feats[u].resize((size_t)T * dim);
      in.read(reinterpret_cast<char*>(feats[u].data()), sizeof(float) * feats[u].size());
    }
    sr::StreamingRecognizer rec(lex, mm, tdp, beam, wp, n_utts, 4096);
    std::vector<uint32_t> ids;
    for (uint32_t u = 0; u < n_utts; u++) ids.push_back(rec.begin());
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
      rec.push(who, buf.data(), off);
      if (round == 0)
        for (uint32_t u = 0; u < n_utts; u++) print("partial", u, rec.partial(ids[u]));
    }
    for (uint32_t u = 0; u < n_utts; u++) print("final", u, rec.end(ids[u]));
    try {
      rec.end(ids[0]);
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
