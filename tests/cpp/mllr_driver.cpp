// mllr_driver.cpp -- a stand-alone program around sr_mllr_estimate (speechrecognition_amd/csrc/mllr.cpp) for tests/test_mllr_cpu.py:
// compiled together with mllr.cpp by g++ -fsanitize=address,undefined, no library, no device.
//   mllr_driver <case.bin>   case.bin: u32 dim, u32 n_speakers, u32 n_classes, u32 n_nodes, f64 min_count, i32 parent[n_nodes],
//                            f64 beta[S * R], f64 k[S * R * D * (D+1)], f64 G[S * R * D * (D+1)^2], f64 W[S * R * D * (D+1)].
//                            Prints "leaf <s> <r> node <v> aux <hex bits> <hex bits>" and "W <hex bits> ..." per (speaker, class).
#include <cstdio>
#include <cstring>
#include <fstream>
#include <string>
#include <vector>

#include "../../speechrecognition_amd/csrc/host_util.h"

static std::string last_error;
int srhost::set_error(int code, const char* msg) {
  last_error = msg;
  return code;
}

template <typename T>
static T rd(std::istream& in) {
  T v;
  in.read(reinterpret_cast<char*>(&v), sizeof v);
  return v;
}

template <typename T>
static std::vector<T> rd_n(std::istream& in, size_t n) {
  std::vector<T> v(n);
  in.read(reinterpret_cast<char*>(v.data()), sizeof(T) * n);
  return v;
}

static unsigned long long bits(double d) {
  unsigned long long b;
  memcpy(&b, &d, sizeof b);
  return b;
}

int main(int argc, char** argv) {
  if (argc != 2) { fprintf(stderr, "usage: %s <case.bin>\n", argv[0]); return 2; }
  std::ifstream in(argv[1], std::ios::binary);
  const uint32_t D = rd<uint32_t>(in), S = rd<uint32_t>(in), R = rd<uint32_t>(in), N = rd<uint32_t>(in);
  const double min_count = rd<double>(in);
  const size_t nW = (size_t)D * (D + 1);
  std::vector<int32_t> parent = rd_n<int32_t>(in, N);
  std::vector<double> beta = rd_n<double>(in, (size_t)S * R), k = rd_n<double>(in, (size_t)S * R * nW);
  std::vector<double> G = rd_n<double>(in, (size_t)S * R * nW * (D + 1)), W = rd_n<double>(in, (size_t)S * R * nW);
  if (!in) { printf("error short case file\n"); return 1; }
  std::vector<int32_t> node((size_t)S * R);
  std::vector<double> aux((size_t)S * R * 2);
  const int rc = sr_mllr_estimate(D, S, R, N, parent.data(), beta.data(), k.data(), G.data(), min_count, W.data(), node.data(), aux.data());
  if (rc) { printf("error %d %s\n", rc, last_error.c_str()); return 1; }
  // a malformed tree is refused without touching anything
  if (N > R) {
    std::vector<int32_t> bad(parent);
    bad[N - 1] = 0;
    if (sr_mllr_estimate(D, S, R, N, bad.data(), beta.data(), k.data(), G.data(), min_count, W.data(), node.data(), aux.data()) != SR_EINVAL) {
      printf("error a malformed tree was accepted\n");
      return 1;
    }
  }
  for (uint32_t s = 0; s < S; s++)
    for (uint32_t r = 0; r < R; r++) {
      const size_t g = (size_t)s * R + r;
      printf("leaf %u %u node %d aux %llx %llx\nW", s, r, node[g], bits(aux[2 * g]), bits(aux[2 * g + 1]));
      for (size_t e = 0; e < nW; e++) printf(" %llx", bits(W[g * nW + e]));
      printf("\n");
    }
  return 0;
}
