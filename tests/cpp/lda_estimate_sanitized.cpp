// lda_estimate_sanitized.cpp -- a stand-alone program around the host estimate (speechrecognition_amd/csrc/lda.cpp, included as
// source) for tests/test_lda_cpu.py, which compiles it with -fsanitize=address,undefined and runs it directly.
//   <stats.bin> ...   each file as lda_driver's estimate mode: u32 E, u32 n_classes, u32 p, u32 remove_mean, f64 min_count,
//                     f64 count[K], f64 sum[K * E], f64 scatter[E * E].  Prints "status <st> E <E> p <p>" and "M <hex bits> ..." per file.
#include <cstdio>
#include <cstring>
#include <fstream>
#include <stdexcept>
#include <vector>

#include "../../speechrecognition_amd/csrc/lda.cpp"

namespace srhost {
int set_error(int code, const char* msg) {
  fprintf(stderr, "%s\n", msg);
  return code;
}
}  // namespace srhost

template <typename T>
static std::vector<T> rdv(std::istream& in, size_t n) {
  std::vector<T> v(n);
  in.read(reinterpret_cast<char*>(v.data()), sizeof(T) * n);
  if (!in) throw std::runtime_error("short input file");
  return v;
}

int main(int argc, char** argv) {
  for (int f = 1; f < argc; f++) {
    std::ifstream in(argv[f], std::ios::binary);
    const std::vector<uint32_t> head = rdv<uint32_t>(in, 4);
    const uint32_t E = head[0], K = head[1], p = head[2];
    const double min_count = rdv<double>(in, 1)[0];
    const std::vector<double> count = rdv<double>(in, K), sum = rdv<double>(in, (size_t)K * E), scatter = rdv<double>(in, (size_t)E * E);
    // exactly sized buffers: an access past either end is the sanitizer's to find
    std::vector<double> M((size_t)p * (E + 1), 0.0), eig(E, 0.0);
    int32_t status = -1;
    const int rc = sr_lda_estimate(E, K, count.data(), sum.data(), scatter.data(), p, (int)head[3], min_count, M.data(), eig.data(), &status);
    if (rc != 0) return 3;
    printf("status %d E %u p %u\nM", status, E, p);
    for (double v : M) {
      unsigned long long b;
      memcpy(&b, &v, sizeof b);
      printf(" %llx", b);
    }
    printf("\n");
  }
  return 0;
}
