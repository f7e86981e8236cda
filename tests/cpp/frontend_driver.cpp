// frontend_driver.cpp -- drives include/sr_sietill.hpp's sr::FeaturePostProcessor and sr::FrontEnd for tests/test_frontend_cpu.py
// (compilation, the host loop) and tests/test_gpu_frontend.py.
//   host <post.bin>      host only: process_features on every utterance.
//   time <post.bin>      host only: the same loop timed; prints "host_ms <ms> checksum <x>" (tools/frontend_time.py).
//   cepstra <post.bin>   FeaturePostProcessor::device_corpus on a placeholder model, downloaded.
//                        post.bin: u32 n_static, n_first, n_second, deriv_step, energy_max_norm, has_norm, n_utts, u64 frame_off[n_utts + 1],
//                        has_norm ? f64 mean[nt], f64 stddev[nt], f32 cepstra[F * n_static].  Both print "feats <hex bits> ...".
//   audio <audio.bin>    sr::FrontEnd: from_audio downloaded, and mfcc.  audio.bin: u32 window, shift, n_fft, n_mel, n_cepstra, n_first,
//                        n_second, deriv_step, energy_max_norm, n_utts, f64 sample_rate, f_low, f_high, f32 preemphasis, energy_floor,
//                        u64 sample_off[n_utts + 1], i16 samples[].  Prints "frame_off <decimal> ...", "feats <hex bits> ..." and
//                        "cepstra <hex bits> ...".
#include <chrono>
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

static void print(const char* name, std::vector<float> const& v) {
  printf("%s", name);
  for (float x : v) {
    unsigned b;
    memcpy(&b, &x, sizeof b);
    printf(" %x", b);
  }
  printf("\n");
}

// a model that only holds a corpus: one state, one density
static std::shared_ptr<sr_model> placeholder(uint32_t dim) {
  const uint32_t dens_off[2] = {0, 1};
  const std::vector<double> zeros(dim, 0.0), ones(dim, 1.0);
  sr_model* m = nullptr;
  sr::check(sr_model_create(0, dim, 1, dens_off, zeros.data(), ones.data(), zeros.data(), zeros.data(), 1, &m));
  return std::shared_ptr<sr_model>(m, sr_model_destroy);
}

int main(int argc, char** argv) {
  try {
    if (argc == 3 && (!strcmp(argv[1], "host") || !strcmp(argv[1], "cepstra") || !strcmp(argv[1], "time"))) {
      std::ifstream in(argv[2], std::ios::binary);
      sr::FeaturePostProcessor post;
      post.n_features_in_file = rd<uint32_t>(in);
      post.n_features_first = rd<uint32_t>(in);
      post.n_features_second = rd<uint32_t>(in);
      post.deriv_step = rd<uint32_t>(in);
      post.energy_max_norm = rd<uint32_t>(in) != 0;
      const uint32_t has_norm = rd<uint32_t>(in), n_utts = rd<uint32_t>(in);
      const std::vector<uint64_t> off = rdv<uint64_t>(in, (size_t)n_utts + 1);
      if (has_norm) {
        post.mean = rdv<double>(in, post.n_features_total());
        post.stddev = rdv<double>(in, post.n_features_total());
      }
      const size_t nf = post.n_features_in_file;
      const std::vector<float> cep = rdv<float>(in, (size_t)off.back() * nf);
      std::vector<float> feats;
      if (!strcmp(argv[1], "time")) {  // the host loop alone, one thread: its time and a checksum instead of the rows
        const auto t0 = std::chrono::steady_clock::now();
        double sum = 0.0;
        for (uint32_t u = 0; u < n_utts; u++) {
          std::vector<float> seq(cep.begin() + off[u] * nf, cep.begin() + off[u + 1] * nf);
          post.process_features(seq);
          sum += seq.empty() ? 0.0 : seq.back();
        }
        const double ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
        printf("host_ms %.3f checksum %.6g\n", ms, sum);
        return 0;
      }
      if (!strcmp(argv[1], "host")) {
        for (uint32_t u = 0; u < n_utts; u++) {
          std::vector<float> seq(cep.begin() + off[u] * nf, cep.begin() + off[u + 1] * nf);
          post.process_features(seq);
          feats.insert(feats.end(), seq.begin(), seq.end());
        }
      } else {
        std::shared_ptr<sr_model> model = placeholder((uint32_t)post.n_features_total());
        std::shared_ptr<sr_corpus> corpus = post.device_corpus(model.get(), cep.data(), off.data(), n_utts);
        feats = sr::FrontEnd::download(corpus.get(), off.back(), (uint32_t)post.n_features_total());
      }
      print("feats", feats);
      return 0;
    }
    if (argc == 3 && !strcmp(argv[1], "audio")) {
      std::ifstream in(argv[2], std::ios::binary);
      sr_mfcc_params p{};
      p.window = rd<uint32_t>(in); p.shift = rd<uint32_t>(in); p.n_fft = rd<uint32_t>(in); p.n_mel = rd<uint32_t>(in);
      p.n_cepstra = rd<uint32_t>(in);
      sr::FeaturePostProcessor post;
      post.n_features_in_file = p.n_cepstra;
      post.n_features_first = rd<uint32_t>(in);
      post.n_features_second = rd<uint32_t>(in);
      post.deriv_step = rd<uint32_t>(in);
      post.energy_max_norm = rd<uint32_t>(in) != 0;
      const uint32_t n_utts = rd<uint32_t>(in);
      p.sample_rate = rd<double>(in); p.f_low = rd<double>(in); p.f_high = rd<double>(in);
      p.preemphasis = rd<float>(in); p.energy_floor = rd<float>(in);
      const std::vector<uint64_t> sample_off = rdv<uint64_t>(in, (size_t)n_utts + 1);
      const std::vector<int16_t> samples = rdv<int16_t>(in, sample_off.back());
      std::shared_ptr<sr_model> model = placeholder((uint32_t)post.n_features_total());
      sr::FrontEnd fe(model.get(), p, post);
      std::vector<uint64_t> frame_off, frame_off2;
      std::shared_ptr<sr_corpus> corpus = fe.from_audio(samples, sample_off, frame_off);
      const std::vector<float> feats = sr::FrontEnd::download(corpus.get(), frame_off.back(), (uint32_t)post.n_features_total());
      const std::vector<float> cep = fe.mfcc(samples, sample_off, frame_off2);
      if (frame_off != frame_off2) throw std::runtime_error("from_audio and mfcc disagree about the frames");
      printf("frame_off");
      for (uint64_t f : frame_off) printf(" %llu", (unsigned long long)f);
      printf("\n");
      print("feats", feats);
      print("cepstra", cep);
      return 0;
    }
    fprintf(stderr, "usage: %s host <post.bin> | time <post.bin> | cepstra <post.bin> | audio <audio.bin>\n", argv[0]);
    return 2;
  } catch (std::exception const& e) {
    printf("error %s\n", e.what());
    return 1;
  }
}
