// chains.cpp -- the transcripts' chains of the MMI passes: the recognition network (build_chains: ChainArgs of kernels.h,
// viterbi_mmi.hip) and the bigram search network (build_bgchains: BgChainArgs, viterbi_bigram_mmi.hip) restricted to each utterance's
// transcript w_1 .. w_n.  Host code on plain arrays: no handle, no device.
//
// Either chain is 2 n + 1 segments, each the positions of one slot of its network with that slot's info words; a segment's first two
// positions carry `src` = the (up to two) word ends that enter it, its last position `dst` = the first positions of the (up to two)
// segments its word end enters: chain positions within the utterance, low | high << 16, 0xFFFF = none.  lay_out() places an utterance's
// segments, link() writes one segment's links; the two builders say which slot a segment is and who enters whom.
//
// Compiled as part of srgpu_api.cpp's translation unit (which includes this file ahead of the network passes).  The file is complete by
// itself -- host_util.h and the standard library -- which is how tests/cpp/chains_driver.cpp builds it.
#include <algorithm>
#include <limits>
#include <vector>

#include "host_util.h"

namespace chain_host {

static constexpr uint32_t kNone = 0xFFFFu;

// an utterance's segments while its links are written: first and last chain position of each, from the utterance's first (`base`)
struct Segments {
  uint32_t base = 0;
  std::vector<uint32_t> slot, beg, end;
};

// appends the info of sg->slot's segments (slot x: info[slot_off[x] .. slot_off[x + 1])) to the chains, with no link yet
static void lay_out(Chains* ch, const uint32_t* slot_off, const uint32_t* info, bool with_lmc, Segments* sg) {
  const size_t G = sg->slot.size();
  sg->base = (uint32_t)ch->info.size();
  sg->beg.assign(G, 0); sg->end.assign(G, 0);
  for (size_t g = 0; g < G; g++) {
    const uint32_t x = sg->slot[g];
    sg->beg[g] = (uint32_t)ch->info.size() - sg->base;
    ch->info.insert(ch->info.end(), info + slot_off[x], info + slot_off[x + 1]);
    sg->end[g] = (uint32_t)ch->info.size() - sg->base - 1;
  }
  ch->src.resize(ch->info.size(), 0xFFFFFFFFu);
  ch->dst.resize(ch->info.size(), 0xFFFFFFFFu);
  if (with_lmc) ch->lmc.resize(ch->info.size(), 0.0);
}

// segment g is entered by the word ends s0 and s1 (at the LM cost *lmc: the bigram chains) and enters d0 and d1
static void link(Chains* ch, const Segments& sg, uint32_t g, uint32_t s0, uint32_t s1, uint32_t d0, uint32_t d1, const double* lmc = nullptr) {
  for (uint32_t k = sg.beg[g]; k <= std::min(sg.beg[g] + 1, sg.end[g]); k++) {
    ch->src[sg.base + k] = s0 | s1 << 16;
    if (lmc) ch->lmc[sg.base + k] = *lmc;
  }
  ch->dst[sg.base + sg.end[g]] = d0 | d1 << 16;
}

void build_chains(const uint32_t* word_off, const uint32_t* slot_info, uint32_t U, const uint32_t* trans, const uint64_t* trans_off,
                  Chains* ch) {
  *ch = Chains();
  ch->sil_len = word_off[1];
  ch->off.assign((size_t)U + 1, 0);
  Segments sg;
  for (uint32_t u = 0; u < U; u++) {
    const uint32_t n = (uint32_t)(trans_off[u + 1] - trans_off[u]), G = 2 * n + 1;
    sg.slot.resize(G);
    for (uint32_t g = 0; g < G; g++) sg.slot[g] = (g & 1) ? trans[trans_off[u] + g / 2] : 0u;  // sil_0 w_1 sil_1 .. w_n sil_n
    lay_out(ch, word_off, slot_info, false, &sg);
    const std::vector<uint32_t>&beg = sg.beg, &end = sg.end;
    for (uint32_t g = 0; g < G; g++) {
      // a word is entered by the silence before it and the word before that; a silence by the word before it and by itself
      const uint32_t s0 = g ? end[g - 1] : kNone, s1 = (g & 1) ? (g >= 2 ? end[g - 2] : kNone) : end[g];
      // a word end enters the next word and the silence after it; a silence's the next word and itself
      const uint32_t d0 = g + 1 < G ? beg[g + 1] : kNone, d1 = (g & 1) ? (g + 2 < G ? beg[g + 2] : kNone) : beg[g];
      link(ch, sg, g, s0, s1, d0, d1);
    }
    ch->off[u + 1] = ch->info.size();
  }
}

void build_bgchains(const uint32_t* slot_off, const uint32_t* pos_info, uint32_t W, uint32_t sil, const float* lmT, double scale, uint32_t U,
                    const uint32_t* trans, const uint64_t* trans_off, Chains* ch) {
  *ch = Chains();
  ch->sil_len = slot_off[sil + 1] - slot_off[sil];
  ch->off.assign((size_t)U + 1, 0);
  Segments sg;
  for (uint32_t u = 0; u < U; u++) {
    const uint32_t n = (uint32_t)(trans_off[u + 1] - trans_off[u]), G = 2 * n + 1;
    const uint32_t* tr = trans + trans_off[u];
    sg.slot.resize(G);
    for (uint32_t g = 0; g < G; g++) sg.slot[g] = g == 0 ? sil : ((g & 1) ? tr[g / 2] : tr[g / 2 - 1] + W);  // S w_1 c_1 .. w_n c_n
    lay_out(ch, slot_off, pos_info, true, &sg);
    const std::vector<uint32_t>&beg = sg.beg, &end = sg.end;
    for (uint32_t g = 0; g < G; g++) {
      double lmc = 0.0;
      if (g == 0) {  // S: from the start and itself; into itself and w_1
        link(ch, sg, g, end[0], kNone, beg[0], G > 1 ? beg[1] : kNone, &lmc);
      } else if (g & 1) {  // w_i: from w_{i-1} and c_{i-1} (w_1: the start and S); into c_i and w_{i+1}
        const float x = lmT[(size_t)(g == 1 ? sil : tr[g / 2 - 1]) * W + tr[g / 2]];
        lmc = x < std::numeric_limits<float>::infinity() ? scale * (double)x : std::numeric_limits<double>::infinity();  // (NaN: forbidden)
        link(ch, sg, g, g == 1 ? end[0] : end[g - 2], g == 1 ? kNone : end[g - 1], beg[g + 1], g + 2 < G ? beg[g + 2] : kNone, &lmc);
      } else {  // c_i: from w_i; into w_{i+1}
        link(ch, sg, g, end[g - 1], kNone, g + 1 < G ? beg[g + 1] : kNone, kNone, &lmc);
      }
    }
    ch->off[u + 1] = ch->info.size();
  }
}

}  // namespace chain_host
