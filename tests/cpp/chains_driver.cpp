// chains_driver.cpp -- a stand-alone program around the transcript-chain builders (speechrecognition_amd/csrc/chains.cpp) for
// tests/test_chains_cpu.py: compiled together with chains.cpp by g++ -fsanitize=address,undefined, no library, no device.
//   chains_driver <case.bin>   case.bin: u32 kind (0: build_chains, 1: build_bgchains), u32 W, u32 sil, f64 scale, u32 n_off,
//                              u32 off[n_off] (word_off [W + 1] / slot_off [2 W + 1]), u32 n_info, u32 info[n_info] (slot_info / pos_info),
//                              f32 lmT[W * W] (kind 1), u32 U, u64 trans_off[U + 1], u32 trans[trans_off[U]].
//                              Prints the lines "sil_len", "off", "info", "src", "dst" and "lmc" (64-bit patterns, hex).
#include <cstdio>
#include <cstring>
#include <fstream>
#include <vector>

#include "../../speechrecognition_amd/csrc/host_util.h"

int srhost::set_error(int code, const char*) { return code; }

template <typename T>
static T rd(std::istream& in) {
  T v{};
  in.read(reinterpret_cast<char*>(&v), sizeof v);
  return v;
}

template <typename T>
static std::vector<T> rd_n(std::istream& in, size_t n) {
  std::vector<T> v(n);
  in.read(reinterpret_cast<char*>(v.data()), sizeof(T) * n);
  return v;
}

template <typename T>
static void line(const char* name, const std::vector<T>& v) {
  printf("%s", name);
  for (T e : v) printf(" %llu", (unsigned long long)e);
  printf("\n");
}

int main(int argc, char** argv) {
  if (argc != 2) { fprintf(stderr, "usage: %s <case.bin>\n", argv[0]); return 2; }
  std::ifstream in(argv[1], std::ios::binary);
  const uint32_t kind = rd<uint32_t>(in), W = rd<uint32_t>(in), sil = rd<uint32_t>(in);
  const double scale = rd<double>(in);
  const std::vector<uint32_t> off = rd_n<uint32_t>(in, rd<uint32_t>(in)), info = rd_n<uint32_t>(in, rd<uint32_t>(in));
  const std::vector<float> lmT = rd_n<float>(in, kind ? (size_t)W * W : 0);
  const uint32_t U = rd<uint32_t>(in);
  const std::vector<uint64_t> trans_off = rd_n<uint64_t>(in, (size_t)U + 1);
  const std::vector<uint32_t> trans = rd_n<uint32_t>(in, trans_off[U]);
  if (!in) { printf("error short case file\n"); return 1; }
  chain_host::Chains ch;
  ch.info.assign(3, 99);  // what an earlier call left is not kept
  if (kind == 0) chain_host::build_chains(off.data(), info.data(), U, trans.data(), trans_off.data(), &ch);
  else chain_host::build_bgchains(off.data(), info.data(), W, sil, lmT.data(), scale, U, trans.data(), trans_off.data(), &ch);
  printf("sil_len %u\n", ch.sil_len);
  line("off", ch.off); line("info", ch.info); line("src", ch.src); line("dst", ch.dst);
  std::vector<uint64_t> bits(ch.lmc.size());
  if (!bits.empty()) memcpy(bits.data(), ch.lmc.data(), sizeof(uint64_t) * bits.size());
  printf("lmc");
  for (uint64_t b : bits) printf(" %llx", (unsigned long long)b);
  printf("\n");
  return 0;
}
