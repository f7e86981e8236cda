// fb_plan_driver.cpp -- runs speechrecognition_amd/csrc/fb_plan.h (host code, no HIP) for tests/test_fb_plan_cpu.py.
//   fb_plan_driver <cases.txt>
// cases.txt, whitespace separated, any number of cases; every answer ends with a line "end".
//   groups <n_chunks> <U> <budget>  u0 u1 (per chunk)  frame_off[U + 1]  cost[U + 1]
//     -> "chunk u0 u1 u0 u1 ..." per chunk (its groups), "max <frames> <utterances> <cost>" (the accessors), "order ...",
//        and per group in corpus order "steps <t_max> alive(0) ... alive(t_max)"
//   mix <16|32> <masked 0|1> <n_sets>  N ids[N] (per set)
//     -> "mix_off ...", "mix ...", "slot_beg ...", "slot_pos ..."; masked: 32-bit ids under the mask 0xFFFF, else 16-bit ids
//   occ <16|32> <chain 0|1> <lists 0|1> <U> <P>  frame_off[U + 1]  chain: chain_off[U + 1] info[chain_off[U]]; else: info[P]
//     -> "tr_off ...", "bound <item_bound>", the four lines of mix, and "maxpos ..." (max_positions of every single utterance, then of
//        all of them as one group; over chain_off, or over frame_off for the free network)
//   seg <n_ranges> <L>  bounds[n_ranges + 1]
//     -> "begin ...", "len ...", "off ..."
//   block <n>  max_positions[n]
//     -> "threads ..." (fb_block_threads of each), "chain_threads ..." (chain_block_threads of each)
#include <cstdio>
#include <fstream>
#include <string>
#include <vector>

#include "fb_plan.h"

template <typename V>
static void line(const char* name, V const& v) {
  printf("%s", name);
  for (auto x : v) printf(" %llu", (unsigned long long)x);
  printf("\n");
}

static bool groups_case(std::ifstream& in) {
  size_t n_chunks = 0;
  uint32_t U = 0;
  uint64_t budget = 0;
  in >> n_chunks >> U >> budget;
  std::vector<srplan::Chunk> chunks(n_chunks);
  for (auto& c : chunks) in >> c.u0 >> c.u1;
  std::vector<uint64_t> frame_off(U + 1), cost(U + 1);
  for (auto& v : frame_off) in >> v;
  for (auto& v : cost) in >> v;
  if (!in) return false;
  for (auto& c : chunks) { c.f0 = frame_off[c.u0]; c.f1 = frame_off[c.u1]; }
  const srplan::Groups g = srplan::launch_groups(chunks, cost.data(), budget);
  for (const auto& gs : g.of_chunk) {
    printf("chunk");
    for (const srplan::Group& x : gs) printf(" %u %u", x.u0, x.u1);
    printf("\n");
  }
  printf("max %llu %u %llu\n", (unsigned long long)g.max_span(frame_off.data()), g.max_utts(), (unsigned long long)g.max_span(cost.data()));
  const srplan::StepOrder so(g, frame_off.data(), U);
  line("order", so.order);
  for (const auto& gs : g.of_chunk)
    for (const srplan::Group& x : gs) {
      const uint32_t t_max = so.t_max(x);
      printf("steps %u", t_max);
      for (uint32_t t = 0; t <= t_max; t++) printf(" %u", so.alive(x, t));
      printf("\n");
    }
  return true;
}

template <class Pos>
static bool mix_case(std::ifstream& in, bool masked, uint32_t n_sets) {
  srplan::MixLists<Pos> ml;
  for (uint32_t s = 0; s < n_sets; s++) {
    uint64_t N = 0;
    in >> N;
    std::vector<uint32_t> ids(N);
    for (auto& v : ids) in >> v;
    if (!in) return false;
    if (masked) {
      ml.add(ids.data(), N, 0xFFFFu);
    } else {
      const std::vector<uint16_t> narrow(ids.begin(), ids.end());
      ml.add(narrow.data(), N);
    }
  }
  line("mix_off", ml.mix_off);
  line("mix", ml.mix);
  line("slot_beg", ml.slot_beg);
  line("slot_pos", ml.slot_pos);
  return true;
}

template <class Pos>
static bool occ_case(std::ifstream& in, bool chain, bool lists, uint32_t U, uint64_t P) {
  std::vector<uint64_t> frame_off(U + 1), chain_off(chain ? U + 1 : 0);
  for (auto& v : frame_off) in >> v;
  for (auto& v : chain_off) in >> v;
  if (!in) return false;
  std::vector<uint32_t> info(chain ? chain_off[U] : P);
  for (auto& v : info) in >> v;
  if (!in) return false;
  const srplan::OccPlan<Pos> pl(frame_off.data(), U, chain ? chain_off.data() : nullptr, info.data(), P, lists);
  line("tr_off", pl.tr_off);
  printf("bound %llu\n", (unsigned long long)pl.item_bound);
  line("mix_off", pl.ml.mix_off);
  line("mix", pl.ml.mix);
  line("slot_beg", pl.ml.slot_beg);
  line("slot_pos", pl.ml.slot_pos);
  const uint64_t* off = chain ? chain_off.data() : frame_off.data();
  std::vector<uint32_t> maxpos;
  for (uint32_t u = 0; u < U; u++) maxpos.push_back(srplan::max_positions({u, u + 1}, off));
  maxpos.push_back(srplan::max_positions({0, U}, off));
  line("maxpos", maxpos);
  return true;
}

static bool seg_case(std::ifstream& in) {
  uint32_t n = 0, L = 0;
  in >> n >> L;
  std::vector<uint32_t> bounds((size_t)n + 1);
  for (auto& v : bounds) in >> v;
  if (!in || L == 0) return false;
  const srplan::Segments seg(bounds.data(), n, L);
  line("begin", seg.begin);
  line("len", seg.len);
  line("off", seg.off);
  return true;
}

int main(int argc, char** argv) {
  if (argc != 2) { fprintf(stderr, "usage: %s <cases.txt>\n", argv[0]); return 2; }
  std::ifstream in(argv[1]);
  std::string op;
  while (in >> op) {
    bool ok = false;
    if (op == "groups") {
      ok = groups_case(in);
    } else if (op == "mix") {
      uint32_t width = 0, masked = 0, n_sets = 0;
      in >> width >> masked >> n_sets;
      ok = width == 16 ? mix_case<uint16_t>(in, masked != 0, n_sets) : mix_case<uint32_t>(in, masked != 0, n_sets);
    } else if (op == "occ") {
      uint32_t width = 0, chain = 0, lists = 0, U = 0;
      uint64_t P = 0;
      in >> width >> chain >> lists >> U >> P;
      ok = width == 16 ? occ_case<uint16_t>(in, chain != 0, lists != 0, U, P) : occ_case<uint32_t>(in, chain != 0, lists != 0, U, P);
    } else if (op == "seg") {
      ok = seg_case(in);
    } else if (op == "block") {
      size_t n = 0;
      in >> n;
      std::vector<uint32_t> v(n);
      for (auto& x : v) in >> x;
      ok = (bool)in;
      std::vector<uint32_t> c(v);
      for (auto& x : v) x = srplan::fb_block_threads(x);
      for (auto& x : c) x = srplan::chain_block_threads(x);
      line("threads", v);
      line("chain_threads", c);
    }
    if (!ok) { fprintf(stderr, "bad case file\n"); return 2; }
    printf("end\n");
  }
  return 0;
}
