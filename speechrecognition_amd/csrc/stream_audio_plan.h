// stream_audio_plan.h -- the bookkeeping of one utterance fed as audio to a stream set (sr_stream_push_audio, sr_stream_finish_audio and
// their bigram twins; the definition is in include/srgpu.h).  Host code over plain arrays, no HIP include:
// tests/cpp/stream_audio_plan_driver.cpp compiles it with the host compiler alone.
//
// An utterance has received N samples and has S = frames(N) statics; frame t covers samples [t shift, t shift + window).  What the
// host keeps between pushes (the carry) is what the next frame, S, still needs of the samples received:
//   tail   samples [S shift, N), fewer than `window` of them -- or, where shift > window left N short of S shift, nothing and
//   skip   = S shift - N, the samples still to pass over before frame S begins;
//   prev   the sample before the tail's first (the pre-emphasis reads it), 0 before sample 0; while skipping, the last sample received.
// A push uploads  prev | tail | the new samples after the skipped ones  for stream_frontend_kernel: frame S + j of the utterance starts
// 1 + j shift samples into that piece.
//
// Rows.  Row t needs the statics t - step .. t + step (the header's definition), so before the finish the rows 0 .. S - 1 - step are
// out, and the finish emits the rest with the clamps of T = S.  A step emits rows [row0, row0 + rows).
#pragma once
#include <cstdint>
#include <vector>

namespace srplan {

struct AudioCarry {
  uint64_t n_samples = 0;     // N
  uint64_t statics = 0;       // S
  uint64_t skip = 0;
  int16_t prev = 0;
  std::vector<int16_t> tail;
  bool finished = false;
};

struct AudioStep {
  uint64_t drop = 0;          // new samples passed over
  uint64_t n_buf = 0;         // samples behind prev in the upload: the tail and the new samples from `drop` on (0 while still skipping)
  uint64_t new_statics = 0;   // frames S .. S + new_statics - 1 become complete
  uint64_t row0 = 0, rows = 0;
  AudioCarry next;            // the carry after the step
};

inline uint64_t audio_frames(uint32_t window, uint32_t shift, uint64_t n) { return n < window ? 0 : 1 + (n - window) / shift; }
inline uint64_t audio_rows_out(uint64_t statics, uint32_t step, bool finished) { return finished ? statics : statics > step ? statics - step : 0; }

// the step that takes n new samples x (finishing: no more follow; then usually n == 0)
inline AudioStep plan_audio_step(uint32_t window, uint32_t shift, uint32_t step, const AudioCarry& c, const int16_t* x, uint64_t n,
                                 bool finishing) {
  AudioStep s;
  s.drop = c.skip < n ? c.skip : n;
  const uint64_t skip_left = c.skip - s.drop, n_tail = c.tail.size();
  int16_t prev = s.drop ? x[s.drop - 1] : c.prev;
  const uint64_t L = skip_left ? 0 : n_tail + (n - s.drop);
  auto at = [&](uint64_t i) { return i < n_tail ? c.tail[i] : x[s.drop + (i - n_tail)]; };
  s.n_buf = L;
  s.new_statics = audio_frames(window, shift, L);
  s.next.n_samples = c.n_samples + n;
  s.next.statics = c.statics + s.new_statics;
  s.next.finished = finishing;
  const uint64_t consumed = s.new_statics * shift;  // where frame S + new_statics begins in the piece
  if (consumed <= L) {
    s.next.skip = skip_left;
    s.next.prev = consumed ? at(consumed - 1) : prev;
    s.next.tail.reserve(L - consumed);
    for (uint64_t i = consumed; i < L; i++) s.next.tail.push_back(at(i));
  } else {
    s.next.skip = consumed - L;
    s.next.prev = at(L - 1);  // (new_statics > 0, so L >= window >= 2)
  }
  s.row0 = audio_rows_out(c.statics, step, false);
  s.rows = audio_rows_out(s.next.statics, step, finishing) - s.row0;
  return s;
}

// the step's upload, dst[1 + n_buf]: prev, the tail, the new samples after the skipped ones
inline void audio_fill(const AudioCarry& c, const AudioStep& s, const int16_t* x, uint64_t n, int16_t* dst) {
  dst[0] = s.drop ? x[s.drop - 1] : c.prev;
  if (s.n_buf == 0) return;
  uint64_t o = 1;
  for (int16_t v : c.tail) dst[o++] = v;
  for (uint64_t i = s.drop; i < n; i++) dst[o++] = x[i];
}

}  // namespace srplan
