// lda_driver.cpp -- drives include/sr_sietill.hpp's sr::Lda for tests/test_lda_cpu.py (compilation, the host estimate) and
// tests/test_gpu_lda.py.
//   estimate <stats.bin>   host only.  stats.bin: u32 E, u32 n_classes, u32 p, u32 remove_mean, f64 min_count, f64 count[K],
//                          f64 sum[K * E], f64 scatter[E * E].  Prints "status <st> dim <p>", "M <hex bits> ..." and "eig <hex bits> ...".
//   device <corpus.bin>    corpus.bin: u32 dim, u32 n_states, u32 n_utts, u32 context, u32 p, u64 frame_off[n_utts + 1],
//                          u16 states[F], u32 class_of_state[n_states], f32 feats[F * dim].  Statistics of the alignment given, the
//                          estimate with remove_mean, the projected corpus in a placeholder model, one first-pass accumulate.  Prints
//                          "status <st> dim <p>", "M <hex bits> ..." and "means <hex bits of the first-pass model's means> ...".
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

template <typename T>
static std::vector<T> rdv(std::istream& in, size_t n) {
  std::vector<T> v(n);
  in.read(reinterpret_cast<char*>(v.data()), sizeof(T) * n);
  if (!in) throw std::runtime_error("short input file");
  return v;
}

static unsigned long long bits(double d) {
  unsigned long long b;
  memcpy(&b, &d, sizeof b);
  return b;
}

static void print(const char* name, std::vector<double> const& v) {
  printf("%s", name);
  for (double x : v) printf(" %llx", bits(x));
  printf("\n");
}

int main(int argc, char** argv) {
  try {
    if (argc == 3 && !strcmp(argv[1], "estimate")) {
      std::ifstream in(argv[2], std::ios::binary);
      const uint32_t E = rd<uint32_t>(in), K = rd<uint32_t>(in), p = rd<uint32_t>(in), remove_mean = rd<uint32_t>(in);
      const double min_count = rd<double>(in);
      const std::vector<double> count = rdv<double>(in, K), sum = rdv<double>(in, (size_t)K * E), scatter = rdv<double>(in, (size_t)E * E);
      sr::Lda::Result r;
      sr::Lda::estimate(E, K, count, sum, scatter, p, remove_mean != 0, min_count, r);
      printf("status %d dim %u\n", r.status, r.p);
      print("M", r.M);
      print("eig", r.eig);
      return 0;
    }
    if (argc == 3 && !strcmp(argv[1], "device")) {
      std::ifstream in(argv[2], std::ios::binary);
      const uint32_t dim = rd<uint32_t>(in), n_states = rd<uint32_t>(in), n_utts = rd<uint32_t>(in);
      sr::Lda::Config cfg;
      cfg.context = rd<uint32_t>(in);
      cfg.p = rd<uint32_t>(in);
      cfg.min_count = 0.0;
      const std::vector<uint64_t> off = rdv<uint64_t>(in, (size_t)n_utts + 1);
      const std::vector<uint16_t> states = rdv<uint16_t>(in, off.back());
      cfg.class_of_state = rdv<uint32_t>(in, n_states);
      const std::vector<float> feats = rdv<float>(in, (size_t)off.back() * dim);
      sr::Corpus corpus(dim);
      for (uint32_t u = 0; u < n_utts; u++) corpus.add_segment(feats.data() + off[u] * dim, off[u + 1] - off[u], std::vector<sr::WordIdx>());
      // the base model only holds the corpus: one density per state
      std::vector<uint32_t> dens_off(n_states + 1);
      for (uint32_t s = 0; s <= n_states; s++) dens_off[s] = s;
      const std::vector<double> zeros((size_t)n_states * dim, 0.0), ones((size_t)n_states * dim, 1.0);
      sr_model* base = nullptr;
      sr::check(sr_model_create(0, dim, n_states, dens_off.data(), zeros.data(), ones.data(), zeros.data(), zeros.data(), 1, &base));
      std::shared_ptr<sr_model> own(base, sr_model_destroy);
      sr::Lda::Result r = sr::Lda::from_alignment(base, corpus, states, cfg);
      printf("status %d dim %u\n", r.status, r.p);
      print("M", r.M);
      if (r.model) {
        std::vector<double> means((size_t)n_states * cfg.p);
        sr::check(sr_model_tables(r.model.get(), means.data(), nullptr, nullptr, nullptr));
        print("means", means);
      }
      return 0;
    }
    fprintf(stderr, "usage: %s estimate <stats.bin> | device <corpus.bin>\n", argv[0]);
    return 2;
  } catch (std::exception const& e) {
    printf("error %s\n", e.what());
    return 1;
  }
}
