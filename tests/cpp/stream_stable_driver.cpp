// stream_stable_driver.cpp -- include/sr_sietill.hpp's stable() members against srgpu.h, as INTEGRATION.md 5d / 5e use them
// (tests/test_stream_stable_cpu.py compiles it for syntax and types; the entry points themselves are tested through the C ABI).
//   feed_zerogram   prints the stable words as they grow and ends the utterance after `hangover` frames of trailing silence
//   feed_bigram     prints the stable items as they grow
#include <cstdio>
#include <vector>

#include "sr_sietill.hpp"

static std::vector<sr::WordIdx> feed_zerogram(sr::StreamingRecognizer& rec, const float* frames, size_t n_frames, size_t dim,
                                              size_t piece, uint32_t hangover) {
  const uint32_t id = rec.begin();
  size_t shown = 0;
  for (size_t t = 0; t < n_frames; t += piece) {
    rec.push(id, frames + t * dim, t + piece <= n_frames ? piece : n_frames - t);
    uint32_t commit = 0, silence = 0;
    const std::vector<sr::WordIdx> words = rec.stable(id, &commit, &silence);
    for (; shown < words.size(); shown++) printf("stable %zu (frame %u)\n", words[shown], commit);
    if (shown > 0 && silence >= hangover) break;  // the speaker has stopped
  }
  return rec.end(id);
}

static void feed_bigram(sr::StreamingLinearSearch& rec, const float* frames, size_t n_frames, size_t dim, size_t piece,
                        sr::StreamingLinearSearch::Traceback& result) {
  const uint32_t id = rec.begin();
  size_t shown = 0;
  for (size_t t = 0; t < n_frames; t += piece) {
    rec.push(id, frames + t * dim, t + piece <= n_frames ? piece : n_frames - t);
    sr::StreamingLinearSearch::Traceback items;
    uint32_t commit = 0;
    rec.stable(id, items, &commit);
    for (; shown < items.size(); shown++) printf("stable %u at %u (commit %u)\n", (unsigned)items[shown].word, (unsigned)items[shown].time, commit);
  }
  rec.end(id, result);
}

int main() {
  (void)&feed_zerogram;
  (void)&feed_bigram;
  return 0;
}
