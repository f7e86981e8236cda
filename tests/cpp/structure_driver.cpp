// structure_driver.cpp -- drives include/sr_sietill.hpp's sr::Trainer::train (flat start, splits, eliminations, re-alignment) for
// tests/test_gpu_structure.py.
//   structure_driver <case.bin>
// case.bin: u32 n_words, (u16 states, u16 repetitions) per word, u32 silence word, f64 tdp loop / forward / skip, u32 num_splits,
// u32 num_aligns, u32 num_estimates, f64 min_obs, f64 epsilon, u32 dim, u32 n_utts, then per utterance u32 word count, u32 words[],
// u32 frames, f32 features[frames x dim].  Max-approx, no pooling, the unpruned aligner.
// Prints "score <hex bits>" for the average AM score after every finalize, "densities <per mixture ...>" of the final model and
// "checksum <xor of the final means' bits>".
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

int main(int argc, char** argv) {
  if (argc != 2) { fprintf(stderr, "usage: %s <case.bin>\n", argv[0]); return 2; }
  try {
    std::ifstream in(argv[1], std::ios::binary);
    sr::Lexicon lex;
    const uint32_t n_words = rd<uint32_t>(in);
    std::vector<std::pair<uint16_t, uint16_t>> ws(n_words);
    for (auto& w : ws) { w.first = rd<uint16_t>(in); w.second = rd<uint16_t>(in); }
    const uint32_t sil = rd<uint32_t>(in);
    for (uint32_t w = 0; w < n_words; w++) lex.add_word("w" + std::to_string(w), ws[w].first, ws[w].second, w == sil);
    const double tl = rd<double>(in), tf = rd<double>(in), ts = rd<double>(in);
    sr::Trainer::TrainSchedule sch;
    sch.num_splits = rd<uint32_t>(in); sch.num_aligns = rd<uint32_t>(in); sch.num_estimates = rd<uint32_t>(in);
    sch.min_obs = rd<double>(in); sch.epsilon = rd<double>(in);
    const size_t dim = rd<uint32_t>(in);
    sr::Corpus corpus(dim);
    const uint32_t n_utts = rd<uint32_t>(in);
    for (uint32_t u = 0; u < n_utts; u++) {
      std::vector<sr::WordIdx> orth(rd<uint32_t>(in));
      for (auto& w : orth) w = rd<uint32_t>(in);
      const uint32_t T = rd<uint32_t>(in);
      std::vector<float> f((size_t)T * dim);
      in.read(reinterpret_cast<char*>(f.data()), sizeof(float) * f.size());
      corpus.add_segment(f.data(), T, orth);
    }
    if (!in) throw std::runtime_error("short case file");
    sr::MixtureModel flat(dim, lex.num_states(), sr::MixtureModel::NO_POOLING, true);
    sr::TdpModel tdp(lex.get_silence_automaton().first_state(), tl, tf, ts);
    sr::Trainer trainer(lex, flat, tdp, 50.0, false);
    sr::Trainer::TrainResult r = trainer.train(corpus, sch);
    for (double s : r.am_scores) printf("score %llx\n", bits(s));
    sr::MixtureModel::Tables t = r.model->tables();
    printf("densities");
    for (size_t s = 0; s + 1 < t.dens_off.size(); s++) printf(" %u", t.dens_off[s + 1] - t.dens_off[s]);
    printf("\n");
    unsigned long long x = 0;
    for (double v : t.means) { x ^= bits(v); x = (x << 1) | (x >> 63); }
    printf("checksum %llx\n", x);
    return 0;
  } catch (std::exception const& e) {
    printf("error %s\n", e.what());
    return 1;
  }
}
