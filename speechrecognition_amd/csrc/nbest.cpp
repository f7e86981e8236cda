// nbest.cpp -- N-best word strings from a word lattice: sr_lattice_nbest (the recognition network's lattices, sr_word_lattice_corpus)
// and sr_bigram_lattice_nbest (the bigram search network's, sr_bigram_word_lattice_corpus; the LM may be another than the lattice's).
// Host code on the caller's arrays: no handle, no device.
//
// Both are one best-first search (A*) over (search state, word string so far) with an exact heuristic h = the cheapest completion
// from the state: the first time a (state, string) leaves the queue its cost is that of the string's cheapest path to the state, so
// the complete strings leave in order of their cheapest paths.  best_first() owns the search.  An entry point checks its arguments,
// sorts the arcs by first frame, computes h in one backward pass and supplies its states:
//   sr_lattice_nbest         a frame: the arcs that start there follow; final at frame T
//   sr_bigram_lattice_nbest  the last arc taken (kStart: none yet): it fixes the frame, the slot it left (what may follow: its own copy after
//                            a word, the silence word after the silence word or the start) and the history the next word pays the LM for
//
// Compiled as part of srgpu_api.cpp's translation unit (which includes this file where the lattice entry points end).  The file is
// complete by itself -- host_util.h, srgpu.h and the standard library -- which is how tests/cpp/nbest_host_driver.cpp builds it.
#include <cmath>
#include <cstdarg>
#include <cstdio>
#include <limits>
#include <map>
#include <queue>
#include <set>
#include <utility>
#include <vector>

#include "../../include/srgpu.h"
#include "host_util.h"

namespace nbest_host {

static int bad(int code, const char* fmt, ...) {
  char msg[256];
  va_list ap;
  va_start(ap, fmt);
  vsnprintf(msg, sizeof msg, fmt, ap);
  va_end(ap);
  return srhost::set_error(code, msg);
}

static constexpr double kInf = std::numeric_limits<double>::infinity();

// where the strings go: sr_lattice_nbest's output arguments (*count is 0 and off[0] is 0 already)
struct Output { uint32_t* words; uint64_t words_cap; uint64_t* off; double* cost; uint32_t* count; };

// The best-first search from `start` (nothing to search where h_start is +inf: no complete path).  is_final(state); expand(state,
// visit) calls visit(next state, word, step cost, h of the next state) for every successor, in the order the entries are to be pushed
// (equal f leave the queue in push order).  A successor whose step or h is +inf is on no complete path; `silence_word` adds nothing
// to the string.  The strings live in a trie (node = parent node + word).  unique: a string that has left through one final state is
// not given out again through another (the bigram search's several final arcs; the search with one final state keeps no such set).
template <class IsFinal, class Expand>
static int best_first(uint32_t start, double h_start, uint32_t silence_word, bool unique, uint32_t n_best, IsFinal is_final, Expand expand,
                      const Output& o) {
  struct Node { uint32_t parent, word; };
  std::vector<Node> trie{{0xFFFFFFFFu, 0}};  // node 0: the empty string
  std::map<std::pair<uint32_t, uint32_t>, uint32_t> child;
  std::map<std::pair<uint32_t, uint32_t>, double> best_g;  // (state, node) -> the cheapest cost pushed
  struct Item { double f, g; uint32_t state, node; uint64_t seq; };
  auto later = [](const Item& x, const Item& y) { return x.f > y.f || (x.f == y.f && x.seq > y.seq); };
  std::priority_queue<Item, std::vector<Item>, decltype(later)> queue(later);
  uint64_t seq = 0, n_words_out = 0;
  if (h_start < kInf) {
    best_g[{start, 0u}] = 0.0;
    queue.push(Item{h_start, 0.0, start, 0, seq++});
  }
  uint32_t n_out = 0;
  std::vector<uint32_t> rev;
  std::set<uint32_t> done;  // unique: the strings (trie nodes) given out
  while (!queue.empty() && n_out < n_best) {
    const Item it = queue.top();
    queue.pop();
    if (it.g > best_g[{it.state, it.node}]) continue;  // a cheaper path reached this state later
    if (is_final(it.state)) {
      if (unique && !done.insert(it.node).second) continue;  // the string has left already, at its cheapest, through another final state
      rev.clear();
      for (uint32_t n = it.node; n != 0; n = trie[n].parent) rev.push_back(trie[n].word);
      if (n_words_out + rev.size() > o.words_cap) {
        *o.count = 0;
        return bad(SR_EINVAL, "words_cap %llu is too small", (unsigned long long)o.words_cap);
      }
      for (size_t k = rev.size(); k-- > 0;) o.words[n_words_out++] = rev[k];
      o.cost[n_out] = it.g;
      o.off[++n_out] = n_words_out;
      continue;
    }
    expand(it.state, [&](uint32_t next, uint32_t word, double step, double h_next) {
      if (!(h_next < kInf) || !(step < kInf)) return;  // no complete path goes this way
      uint32_t node = it.node;
      if (word != silence_word) {
        auto ins = child.emplace(std::make_pair(it.node, word), (uint32_t)trie.size());
        if (ins.second) trie.push_back(Node{it.node, word});
        node = ins.first->second;
      }
      const double g = it.g + step;
      auto bg = best_g.find({next, node});
      if (bg != best_g.end() && !(g < bg->second)) return;
      best_g[{next, node}] = g;
      queue.push(Item{g + h_next, g, next, node, seq++});
    });
  }
  *o.count = n_out;
  return SR_OK;
}

}  // namespace nbest_host

extern "C" SR_API int sr_lattice_nbest(uint32_t n_frames, uint64_t n_arcs, const uint32_t* word, const uint32_t* first, const uint32_t* last,
                                       const double* cost, uint32_t silence_word, uint32_t n_best, uint32_t* out_words, uint64_t words_cap,
                                       uint64_t* out_off, double* out_cost, uint32_t* out_count) {
  using namespace nbest_host;
  return srhost::guarded(__func__, [&]() -> int {
  if (!out_off || !out_cost || !out_count || (n_arcs && (!word || !first || !last || !cost)) || (words_cap && !out_words))
    return bad(SR_EINVAL, "null argument");
  *out_count = 0;
  out_off[0] = 0;
  if (n_best == 0) return bad(SR_EINVAL, "n_best must be >= 1");
  for (uint64_t i = 0; i < n_arcs; i++) {
    if (first[i] > last[i] || last[i] >= n_frames) return bad(SR_EINVAL, "arc %llu: frames %u .. %u of %u", (unsigned long long)i, first[i], last[i], n_frames);
    if (i && (last[i] < last[i - 1] || (last[i] == last[i - 1] && word[i] < word[i - 1])))
      return bad(SR_EINVAL, "arc %llu: the arcs are not in (last, word) order", (unsigned long long)i);
    if (std::isnan(cost[i]) || cost[i] == -kInf) return bad(SR_EINVAL, "arc %llu: cost %g", (unsigned long long)i, cost[i]);
  }
  if (n_frames == 0) return SR_OK;
  const uint32_t T = n_frames;
  // the arcs by first frame (a counting sort: arcs of one frame keep their order)
  std::vector<uint64_t> beg((size_t)T + 2, 0);
  for (uint64_t i = 0; i < n_arcs; i++) beg[first[i] + 1]++;
  for (uint32_t f = 0; f <= T; f++) beg[f + 1] += beg[f];
  std::vector<uint64_t> by_first(n_arcs), fill(beg.begin(), beg.end() - 1);
  for (uint64_t i = 0; i < n_arcs; i++) by_first[fill[first[i]]++] = i;
  // what follows frame f: the arcs that start there.  h[f] = the cheapest completion from frame f, from the last frame backwards
  std::vector<double> h((size_t)T + 1, kInf);
  h[T] = 0.0;
  auto expand = [&](uint32_t f, auto&& visit) {
    for (uint64_t k = beg[f]; k < beg[f + 1]; k++) {
      const uint64_t i = by_first[k];
      visit(last[i] + 1, word[i], cost[i], h[last[i] + 1]);
    }
  };
  for (uint32_t f = T; f-- > 0;)
    expand(f, [&](uint32_t, uint32_t, double c, double h_next) { if (c + h_next < h[f]) h[f] = c + h_next; });
  // (one final state, frame T: a string leaves once)
  return best_first(0, h[0], silence_word, false, n_best, [&](uint32_t f) { return f == T; }, expand,
                    Output{out_words, words_cap, out_off, out_cost, out_count});
  });
}

extern "C" SR_API int sr_bigram_lattice_nbest(uint32_t n_frames, uint64_t n_arcs, const uint32_t* word, const uint32_t* hist,
                                              const uint32_t* first, const uint32_t* last, const double* am, uint32_t n_words,
                                              uint32_t silence_word, const float* lm, double lm_scale, uint32_t n_best, uint32_t* out_words,
                                              uint64_t words_cap, uint64_t* out_off, double* out_cost, uint32_t* out_count) {
  using namespace nbest_host;
  return srhost::guarded(__func__, [&]() -> int {
  if (!out_off || !out_cost || !out_count || (n_arcs && (!word || !hist || !first || !last || !am)) || (words_cap && !out_words))
    return bad(SR_EINVAL, "null argument");
  *out_count = 0;
  out_off[0] = 0;
  if (!lm) return bad(SR_EINVAL, "lm is null");
  if (n_best == 0) return bad(SR_EINVAL, "n_best must be >= 1");
  if (!(lm_scale >= 0.0)) return bad(SR_EINVAL, "lm_scale must be >= 0 (got %g)", lm_scale);
  if (n_words == 0 || silence_word >= n_words) return bad(SR_EINVAL, "silence word %u out of range (%u words)", silence_word, n_words);
  if (n_arcs >= 0xFFFFFFFFull) return bad(SR_ELIMIT, "too many arcs");
  const uint32_t W = n_words, sil = silence_word;
  // the slot an arc ends: the word itself, the silence word, or the copy hist + W
  auto slot_of = [&](uint64_t i) { return word[i] != sil ? word[i] : (hist[i] == sil ? sil : hist[i] + W); };
  for (uint64_t i = 0; i < n_arcs; i++) {
    if (word[i] >= W || hist[i] >= W) return bad(SR_EINVAL, "arc %llu: word %u, history %u of %u words", (unsigned long long)i, word[i], hist[i], W);
    if (word[i] != sil && hist[i] != word[i]) return bad(SR_EINVAL, "arc %llu: word %u ends with history %u", (unsigned long long)i, word[i], hist[i]);
    if (first[i] > last[i] || last[i] >= n_frames) return bad(SR_EINVAL, "arc %llu: frames %u .. %u of %u", (unsigned long long)i, first[i], last[i], n_frames);
    if (i && (last[i] < last[i - 1] || (last[i] == last[i - 1] && slot_of(i) <= slot_of(i - 1))))
      return bad(SR_EINVAL, "arc %llu: the arcs are not in (last, slot) order", (unsigned long long)i);
    if (std::isnan(am[i]) || am[i] == -kInf) return bad(SR_EINVAL, "arc %llu: cost %g", (unsigned long long)i, am[i]);
  }
  if (n_frames == 0) return SR_OK;
  const uint32_t T = n_frames, kStart = 0xFFFFFFFFu;
  // the arcs by first frame (a counting sort: arcs of one frame keep their order)
  std::vector<uint64_t> beg((size_t)T + 2, 0);
  for (uint64_t i = 0; i < n_arcs; i++) beg[first[i] + 1]++;
  for (uint32_t f = 0; f <= T; f++) beg[f + 1] += beg[f];
  std::vector<uint32_t> by_first(n_arcs);
  {
    std::vector<uint64_t> fill(beg.begin(), beg.end() - 1);
    for (uint64_t i = 0; i < n_arcs; i++) by_first[fill[first[i]]++] = (uint32_t)i;
  }
  // the cost of arc j right after arc i (kStart: the start, a word end of the silence word): +inf where the network has no such entry
  auto step = [&](uint32_t i, uint32_t j) -> double {
    const uint32_t pw = i == kStart ? sil : word[i], ph = i == kStart ? sil : hist[i];
    double c = 0.0;
    if (word[j] != sil) {
      const float l = lm[(size_t)word[j] * W + ph];
      if (!(l < std::numeric_limits<float>::infinity())) return kInf;  // NaN and +inf: forbidden
      c = lm_scale * (double)l;
    } else if (hist[j] == sil) {
      if (!(pw == sil && ph == sil)) return kInf;  // the silence word follows the start or itself
    } else if (pw != hist[j] || pw == sil) {
      return kInf;  // the copy h + W follows word h alone
    }
    return c + am[j];
  };
  // what follows arc i: the arcs that start where it ended.  h[i] = the cheapest completion after arc i
  std::vector<double> h(n_arcs, kInf);
  auto frame_after = [&](uint32_t i) { return i == kStart ? 0u : last[i] + 1; };
  auto expand = [&](uint32_t i, auto&& visit) {
    for (uint64_t q = beg[frame_after(i)]; q < beg[frame_after(i) + 1]; q++) {
      const uint32_t j = by_first[q];
      visit(j, word[j], step(i, j), h[j]);
    }
  };
  auto cheapest = [&](uint32_t i) {
    double best = kInf;
    expand(i, [&](uint32_t, uint32_t, double st, double h_next) { if (st + h_next < best) best = st + h_next; });
    return best;
  };
  // (last ascends with the index, and an arc's successors start after its last: they are done)
  for (uint64_t k = n_arcs; k-- > 0;) h[k] = last[k] + 1 == T ? 0.0 : cheapest((uint32_t)k);
  // (several arcs end at frame T - 1: a string can arrive through more than one of them)
  return best_first(kStart, cheapest(kStart), sil, true, n_best, [&](uint32_t i) { return frame_after(i) == T; }, expand,
                    Output{out_words, words_cap, out_off, out_cost, out_count});
  });
}
