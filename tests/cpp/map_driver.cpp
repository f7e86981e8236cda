// map_driver.cpp -- a stand-alone program around the host part of sr_model_map_adapt (speechrecognition_amd/csrc/map.cpp) for
// tests/test_map_cpu.py: compiled together with map.cpp by g++ -fsanitize=address,undefined, no library, no device.
//   map_driver <case.bin>   case.bin: u32 n_states, u32 D, u32 C, u32 n_mean, u32 n_entries, f64 tau, f64 tau_w, u32 dens_off[n_states+1],
//                           u32 dens_mean[C], f64 logw[C], u32 dens[n], f64 occ[n], f64 x[n * D].
//                           Prints the plan ("slot", "off", "ent", "rep" lines), "logw <hex bits> ..." after the weight update, then
//                           "empty ok" (n_entries = 0 changes nothing) and "invalid ok" (every malformed input is refused).
#include <cmath>
#include <cstdio>
#include <cstring>
#include <fstream>
#include <limits>
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

static void line(const char* name, const std::vector<uint32_t>& v) {
  printf("%s", name);
  for (uint32_t e : v) printf(" %u", e);
  printf("\n");
}

int main(int argc, char** argv) {
  if (argc != 2) { fprintf(stderr, "usage: %s <case.bin>\n", argv[0]); return 2; }
  std::ifstream in(argv[1], std::ios::binary);
  const uint32_t S = rd<uint32_t>(in), D = rd<uint32_t>(in), C = rd<uint32_t>(in), n_mean = rd<uint32_t>(in), n = rd<uint32_t>(in);
  const double tau = rd<double>(in), tau_w = rd<double>(in);
  const std::vector<uint32_t> dens_off = rd_n<uint32_t>(in, S + 1), dens_mean = rd_n<uint32_t>(in, C);
  const std::vector<double> logw = rd_n<double>(in, C);
  const std::vector<uint32_t> dens = rd_n<uint32_t>(in, n);
  const std::vector<double> occ = rd_n<double>(in, n), x = rd_n<double>(in, (size_t)n * D);
  if (!in) { printf("error short case file\n"); return 1; }
  auto valid = [&](uint64_t ne, const uint32_t* d, const double* o, const double* xx, double t, int uw, double tw) {
    return map_host::validate(C, D, ne, d, o, xx, t, uw, tw);
  };
  if (int rc = valid(n, dens.data(), occ.data(), x.data(), tau, 1, tau_w)) { printf("error %d %s\n", rc, last_error.c_str()); return 1; }
  map_host::Plan plan;
  map_host::plan(C, n_mean, dens_mean.data(), n, dens.data(), &plan);
  line("slot", plan.row_slot); line("off", plan.row_off); line("ent", plan.row_ent); line("rep", plan.row_rep);
  std::vector<double> w(logw);
  map_host::update_weights(S, dens_off.data(), n, dens.data(), occ.data(), tau_w, w.data());
  printf("logw");
  for (double v : w) printf(" %llx", bits(v));
  printf("\n");
  // no entry: valid, an empty plan, every weight as it was
  if (valid(0, nullptr, nullptr, nullptr, tau, 1, tau_w) != SR_OK) { printf("error no entries were refused\n"); return 1; }
  map_host::plan(C, n_mean, dens_mean.data(), 0, nullptr, &plan);
  w = logw;
  map_host::update_weights(S, dens_off.data(), 0, nullptr, nullptr, tau_w, w.data());
  bool same = plan.row_off.size() == 1 && plan.row_ent.empty() && plan.row_rep.empty();
  for (uint32_t s : plan.row_slot) same = same && s == 0xFFFFFFFFu;
  for (uint32_t d = 0; d < C; d++) same = same && bits(w[d]) == bits(logw[d]);
  if (!same) { printf("error no entries changed something\n"); return 1; }
  printf("empty ok\n");
  // every malformed input
  const double nan = std::numeric_limits<double>::quiet_NaN(), inf = std::numeric_limits<double>::infinity();
  int refused = 0, cases = 0;
  auto expect = [&](int rc) { cases++; if (rc == SR_EINVAL) refused++; };
  if (n >= 2) {
    expect(valid(n, nullptr, occ.data(), x.data(), tau, 0, 0.0));
    expect(valid(n, dens.data(), nullptr, x.data(), tau, 0, 0.0));
    expect(valid(n, dens.data(), occ.data(), nullptr, tau, 0, 0.0));
    std::vector<uint32_t> d2(dens);
    d2[1] = d2[0];  // not strictly ascending
    expect(valid(n, d2.data(), occ.data(), x.data(), tau, 0, 0.0));
    d2 = dens; std::swap(d2[0], d2[1]);
    expect(valid(n, d2.data(), occ.data(), x.data(), tau, 0, 0.0));
    d2 = dens; d2[n - 1] = C;  // beyond the model's densities
    expect(valid(n, d2.data(), occ.data(), x.data(), tau, 0, 0.0));
    for (double v : {0.0, -1.0, nan, inf}) {
      std::vector<double> o2(occ);
      o2[n / 2] = v;
      expect(valid(n, dens.data(), o2.data(), x.data(), tau, 0, 0.0));
    }
    for (double v : {nan, inf, -inf}) {
      std::vector<double> x2(x);
      x2[x2.size() - 1] = v;
      expect(valid(n, dens.data(), occ.data(), x2.data(), tau, 0, 0.0));
    }
    for (double v : {-1.0, nan, inf}) expect(valid(n, dens.data(), occ.data(), x.data(), v, 0, 0.0));
    for (double v : {0.0, -1.0, nan, inf}) expect(valid(n, dens.data(), occ.data(), x.data(), tau, 1, v));
    // tau_w is not looked at without update_weights; tau = 0 is allowed
    if (valid(n, dens.data(), occ.data(), x.data(), 0.0, 0, nan) != SR_OK) { printf("error tau = 0 was refused\n"); return 1; }
  }
  if (refused != cases) { printf("error %d of %d malformed inputs were refused\n", refused, cases); return 1; }
  printf("invalid ok %d\n", cases);
  return 0;
}
