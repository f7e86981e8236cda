// splice_clamp.h -- the edge rule of frame splicing (sr_corpus_splice_transform, sr_stream_set_projection): block o of the spliced
// vector of frame t, context c, of an utterance whose frames are [lo, hi), is frame min(max(t + o - c, lo), hi - 1).  One copy for
// lda_stats.hip, stream_pipeline.hip and the host plan (stream_pipeline_plan.h); no HIP include of its own.
#pragma once
#include <cstdint>

#if defined(__HIPCC__)
#define SR_SPLICE_HD __host__ __device__
#else
#define SR_SPLICE_HD
#endif

namespace srplan {

SR_SPLICE_HD inline int64_t splice_frame(int64_t t, int64_t o, int64_t c, int64_t lo, int64_t hi) {
  int64_t s = t + o - c;
  s = s < lo ? lo : s;
  s = s > hi - 1 ? hi - 1 : s;
  return s;
}

}  // namespace srplan
