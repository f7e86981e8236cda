// stream_vtln_driver.cpp -- drives sr::StreamingRecognizer::set_warp of include/sr_sietill.hpp for tests/test_gpu_stream_vtln.py (and,
// compiled only, for tests/test_stream_vtln_cpu.py): one utterance fed as PCM samples under one VTLN warp of a warped sr::FrontEnd
// (12 + 12 + 1 features, step 3, no energy maximum), beside the mirror's batch call on the same samples under the same warp.
//   <mixset> <dim> <case.bin>   case.bin: the MFCC parameters (window, shift, n_fft, n_mel, n_cepstra u32; sample rate, f_low, f_high
//                               f64; pre-emphasis, energy floor f32); the warps as n (u32), alpha[n], break_frac (f64); the lexicon as
//                               W, word_off[W+1] (u32), mixtures (u16), silence (u32); the search's tdp[3], beam, word penalty (f64);
//                               gmm kernel, piece, warp (u32); the utterance's sample count (u32) and int16 samples.
// Streams the utterance `piece` samples per push under `warp`, then once more in the same slot without a warp, and prints
//   "words <words>"   StreamingRecognizer under the warp
//   "batch <words>"   Recognizer::recognizeSequence_pruned on FrontEnd::from_audio_warped's rows under the warp
//   "plain <words>"   StreamingRecognizer on the slot's next utterance, which sets no warp
// Exit status 0 when the first two agree, 1 otherwise or on an error.
#include <cstdio>
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

static void print(const char* what, std::vector<sr::WordIdx> const& words) {
  printf("%s", what);
  for (sr::WordIdx x : words) printf(" %zu", (size_t)x);
  printf("\n");
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
    std::vector<double> alpha(rd<uint32_t>(in));
    for (auto& x : alpha) x = rd<double>(in);
    const double break_frac = rd<double>(in);
    const uint32_t W = rd<uint32_t>(in);
    std::vector<uint32_t> word_off(W + 1);
    for (auto& x : word_off) x = rd<uint32_t>(in);
    for (uint32_t i = 0; i < word_off[W]; i++) rd<uint16_t>(in);  // (the words are runs of consecutive states: only their lengths matter)
    const uint32_t sil = rd<uint32_t>(in);
    const double tl = rd<double>(in), tf = rd<double>(in), ts = rd<double>(in), beam = rd<double>(in), wp = rd<double>(in);
    const int kernel = (int)rd<uint32_t>(in);
    const uint32_t piece = rd<uint32_t>(in);
    const uint32_t warp = rd<uint32_t>(in);
    std::vector<int16_t> utt(rd<uint32_t>(in));
    in.read(reinterpret_cast<char*>(utt.data()), sizeof(int16_t) * utt.size());
    if (!in || piece == 0) throw std::runtime_error("short case file");
    sr::Lexicon lex;
    for (uint32_t w = 0; w < W; w++) lex.add_word("w" + std::to_string(w), (uint16_t)(word_off[w + 1] - word_off[w]), 1, w == sil);
    sr::MixtureModel mm(argv[1], dim, sr::MixtureModel::NO_POOLING, true, 0, kernel);
    sr::FeaturePostProcessor post;
    post.energy_max_norm = false;
    sr::FrontEnd fe(mm.handle(), mp, alpha, break_frac, post);
    sr::TdpModel tdp(lex.get_silence_automaton().first_state(), tl, tf, ts);
    std::vector<sr::WordIdx> streamed, plain, batch;
    {
      sr::StreamingRecognizer rec(lex, mm, tdp, beam, wp, 1, 4096);
      rec.set_frontend(fe);
      for (int pass = 0; pass < 2; pass++) {
        const uint32_t id = rec.begin();
        if (pass == 0) rec.set_warp(id, warp);
        for (size_t at = 0; at < utt.size(); at += piece) rec.push_audio(id, utt.data() + at, std::min<size_t>(piece, utt.size() - at));
        rec.finish_audio(id);
        (pass == 0 ? streamed : plain) = rec.end(id);
      }
    }
    {
      std::vector<uint64_t> frame_off;
      std::shared_ptr<sr_corpus> c = fe.from_audio_warped(utt, {0, utt.size()}, {warp}, frame_off);
      const std::vector<float> rows = sr::FrontEnd::download(c.get(), frame_off[1], (uint32_t)dim);
      c.reset();
      sr::Recognizer rec(lex, mm, tdp, beam, wp);
      rec.recognizeSequence_pruned(rows.data(), frame_off[1], batch);
    }
    print("words", streamed);
    print("batch", batch);
    print("plain", plain);
    return streamed == batch ? 0 : 1;
  } catch (std::exception const& e) {
    printf("error %s\n", e.what());
    return 1;
  }
}
