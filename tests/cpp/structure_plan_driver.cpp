// structure_plan_driver.cpp -- runs speechrecognition_amd/csrc/structure_plan.h (host code, no HIP) for tests/test_structure_cpu.py.
//   structure_plan_driver <case.txt>
// case.txt, whitespace separated: "split" or "eliminate", n_states, n_mean, n_var, pooling, min_obs (hex bits of the double),
// dens_off[n_states + 1], dens_mean[C], dens_var[C], mean_w[n_mean] (hex bits).  Prints one line per array:
// "n <C'> <n_mean'> <n_var'>", "dens_off ...", "parent ...", "sign ...", "dens_mean ...", "dens_var ..." and, for eliminate,
// "mean_map ..." and "var_map ..." (-1: dropped); "too_many <C'>" alone when the split model would not fit.
#include <cstdio>
#include <cstring>
#include <fstream>
#include <string>
#include <vector>

#include "structure_plan.h"

static double from_bits(std::string const& hex) {
  const unsigned long long b = std::stoull(hex, nullptr, 16);
  double d;
  memcpy(&d, &b, sizeof d);
  return d;
}

template <typename V>
static void line(const char* name, V const& v, bool map = false) {
  printf("%s", name);
  for (auto x : v) {
    if (map && (uint32_t)x == srplan::kDropped) printf(" -1");
    else printf(" %lld", (long long)x);
  }
  printf("\n");
}

int main(int argc, char** argv) {
  if (argc != 2) { fprintf(stderr, "usage: %s <case.txt>\n", argv[0]); return 2; }
  std::ifstream in(argv[1]);
  std::string op, tok;
  uint32_t n_states = 0, n_mean = 0, n_var = 0;
  int pooling = 0;
  in >> op >> n_states >> n_mean >> n_var >> pooling >> tok;
  const double min_obs = from_bits(tok);
  std::vector<uint32_t> dens_off(n_states + 1);
  for (auto& v : dens_off) in >> v;
  const uint32_t C = dens_off[n_states];
  std::vector<uint32_t> dens_mean(C), dens_var(C);
  for (auto& v : dens_mean) in >> v;
  for (auto& v : dens_var) in >> v;
  std::vector<double> mean_w(n_mean);
  for (auto& v : mean_w) { in >> tok; v = from_bits(tok); }
  if (!in) { fprintf(stderr, "short case file\n"); return 2; }
  srplan::Plan p;
  if (op == "split") {
    if (!srplan::split_plan(n_states, dens_off.data(), n_mean, n_var, dens_mean.data(), dens_var.data(), mean_w.data(), min_obs, pooling, &p)) {
      printf("too_many %llu\n", (unsigned long long)p.n_dens);
      return 0;
    }
  } else {
    srplan::eliminate_plan(n_states, dens_off.data(), n_mean, n_var, dens_mean.data(), dens_var.data(), mean_w.data(), min_obs, &p);
  }
  printf("n %llu %u %u\n", (unsigned long long)p.n_dens, p.n_mean, p.n_var);
  line("dens_off", p.dens_off);
  line("parent", p.parent);
  line("sign", p.sign);
  line("dens_mean", p.dens_mean);
  line("dens_var", p.dens_var);
  if (op != "split") {
    line("mean_map", p.mean_map, true);
    line("var_map", p.var_map, true);
  }
  return 0;
}
