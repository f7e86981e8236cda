// stream_audio_driver.cpp -- drives the audio side of include/sr_sietill.hpp's sr::StreamingRecognizer and sr::StreamingLinearSearch
// for tests/test_gpu_stream_audio.py: utterances fed as PCM samples through a sr::FrontEnd (12 + 12 + 1 features, step 3, no energy
// maximum).
//   <mixset> <dim> <case.bin>   case.bin: the MFCC parameters (window, shift, n_fft, n_mel, n_cepstra u32; sample rate, f_low, f_high
//                               f64; pre-emphasis, energy floor f32); the lexicon as W, word_off[W+1] (u32), mixtures (u16), silence
//                               (u32); the zerogram search's tdp[3], beam, word penalty (f64); the bigram search's lm[W x W], tdp[8],
//                               beams (f32); gmm kernel, piece (u32); then per utterance its sample count (u32) and int16 samples.
// Feeds all utterances at once, `piece` samples of each per push, finishes and ends them, and prints per utterance
// "words <u> <words>" (StreamingRecognizer) and "items <u> <word, score bits, time in hexadecimal> ..." (StreamingLinearSearch).
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

// every utterance through `rec` as audio, `piece` samples of each per push
template <class Rec, class End>
static void feed(Rec& rec, std::vector<std::vector<int16_t>> const& utts, size_t piece, End end) {
  std::vector<uint32_t> ids;
  for (size_t u = 0; u < utts.size(); u++) ids.push_back(rec.begin());
  for (size_t at = 0;; at += piece) {
    bool any = false;
    for (size_t u = 0; u < utts.size(); u++) {
      if (at >= utts[u].size()) continue;
      rec.push_audio(ids[u], utts[u].data() + at, std::min(piece, utts[u].size() - at));
      any = true;
    }
    if (!any) break;
  }
  for (size_t u = 0; u < utts.size(); u++) {
    rec.finish_audio(ids[u]);
    end(u, ids[u]);
  }
}

int main(int argc, char** argv) {
  if (argc < 4) {
    fprintf(stderr, "usage: %s <mixset> <dim> <case.bin>\n", argv[0]);
    return 2;
  }
  try {
    const size_t dim = std::stoul(argv[2]);
    std::ifstream in(argv[3], std::ios::binary);
    sr_mfcc_params mp = sr_mfcc_params();
    mp.window = rd<uint32_t>(in); mp.shift = rd<uint32_t>(in); mp.n_fft = rd<uint32_t>(in); mp.n_mel = rd<uint32_t>(in);
    mp.n_cepstra = rd<uint32_t>(in);
    mp.sample_rate = rd<double>(in); mp.f_low = rd<double>(in); mp.f_high = rd<double>(in);
    mp.preemphasis = rd<float>(in); mp.energy_floor = rd<float>(in);
    const uint32_t W = rd<uint32_t>(in);
    std::vector<uint32_t> word_off(W + 1);
    for (auto& x : word_off) x = rd<uint32_t>(in);
    std::vector<std::vector<uint16_t>> lexicon(W);
    for (uint32_t w = 0; w < W; w++)
      for (uint32_t i = word_off[w]; i < word_off[w + 1]; i++) lexicon[w].push_back(rd<uint16_t>(in));
    const uint32_t sil = rd<uint32_t>(in);
    const double tl = rd<double>(in), tf = rd<double>(in), ts = rd<double>(in), beam = rd<double>(in), wp = rd<double>(in);
    std::vector<float> lm((size_t)W * W);
    for (auto& x : lm) x = rd<float>(in);
    float tdp8[2][4];
    for (auto& row : tdp8)
      for (auto& x : row) x = rd<float>(in);
    const float acp = rd<float>(in), lmp = rd<float>(in);
    const int kernel = (int)rd<uint32_t>(in);
    const uint32_t piece = rd<uint32_t>(in);
    const uint32_t n_utts = rd<uint32_t>(in);
    std::vector<std::vector<int16_t>> utts(n_utts);
    for (auto& x : utts) {
      x.resize(rd<uint32_t>(in));
      in.read(reinterpret_cast<char*>(x.data()), sizeof(int16_t) * x.size());
    }
    if (!in) throw std::runtime_error("short case file");
    // the lexicon's words as runs of consecutive states, once each (what the test writes)
    sr::Lexicon lex;
    for (uint32_t w = 0; w < W; w++) lex.add_word("w" + std::to_string(w), (uint16_t)lexicon[w].size(), 1, w == sil);
    sr::MixtureModel mm(argv[1], dim, sr::MixtureModel::NO_POOLING, true, 0, kernel);
    sr::FeaturePostProcessor post;
    post.energy_max_norm = false;
    sr::FrontEnd fe(mm.handle(), mp, post);
    {
      sr::TdpModel tdp(lex.get_silence_automaton().first_state(), tl, tf, ts);
      sr::StreamingRecognizer rec(lex, mm, tdp, beam, wp, n_utts, 4096);
      rec.set_frontend(fe);
      feed(rec, utts, piece, [&](size_t u, uint32_t id) {
        printf("words %zu", u);
        for (sr::WordIdx x : rec.end(id)) printf(" %zu", (size_t)x);
        printf("\n");
      });
    }
    {
      sr::StreamingLinearSearch search(mm, lexicon, sil, lm, tdp8, acp, lmp, n_utts, 4096);
      search.set_frontend(fe);
      sr::StreamingLinearSearch::Traceback tb;
      feed(search, utts, piece, [&](size_t u, uint32_t id) {
        search.end(id, tb);
        printf("items %zu", u);
        for (auto const& it : tb) {
          uint32_t bits;
          memcpy(&bits, &it.score, sizeof bits);
          printf(" %x %x %x", it.word, bits, it.time);
        }
        printf("\n");
      });
    }
  } catch (std::exception const& e) {
    printf("error %s\n", e.what());
    return 1;
  }
  return 0;
}
