// stream_pipeline_plan.h -- the bookkeeping of one utterance that passes through a stream set's pipeline (sr_stream_set_projection,
// sr_stream_set_transform, sr_stream_push_rows and their bigram twins; the definition is in include/srgpu.h).  Host code over plain
// integers, no HIP include: tests/cpp/stream_pipeline_plan_driver.cpp compiles it with the host compiler alone.  The two rules of
// the history ring -- where input row g is found (pipeline_source) and which new rows are stored (pipeline_keep0) -- are the
// functions stream_pipeline_kernel itself calls, so the driver exercises the code the device runs; a step's hist_rows, need0 and
// need1 are not handed to the kernel: they state what the step may read, for the driver to hold every read against.
//
// An utterance has received R input rows (pushed rows, or the rows its front end has readied) and the projection's context is c.
// Output row t splices the input rows t - c .. t + c, clamped to [0, T): before the finish the rows 0 .. R - 1 - c are out (the right
// clamp is inactive while input row t + c exists), the finish emits the rest with T = R.  A step emits rows [row0, row0 + rows).
//
// What the device keeps between pushes is the slot's history: the last min(R, 2c) input rows, input row g at ring position g mod 2c
// (the first row a later step can need is (R - c) - c).  A step's kernel finds input row g < R there and input row g >= R at
// position g - R of the push's new rows; afterwards it stores the new rows max(R, R + k - 2c) .. R + k - 1 at their positions.
#pragma once
#include <cstdint>

#include "splice_clamp.h"

namespace srplan {

struct PipelineCarry {
  uint64_t received = 0;  // R
  uint64_t searched = 0;  // rows out so far
  bool finished = false;
};

struct PipelineStep {
  uint64_t rows_in = 0;           // k new input rows
  uint64_t row0 = 0, rows = 0;    // the output rows of the step
  uint64_t hist_rows = 0;         // input rows in the history before the step: R - hist_rows .. R - 1
  uint64_t need0 = 0, need1 = 0;  // the input rows [need0, need1) the step's output rows read (empty without output rows)
  uint64_t keep0 = 0;             // the new input rows [keep0, R + k) go into the history
  PipelineCarry next;             // the carry after the step
};

struct PipelineSource { bool history; uint64_t index; };  // ring position in the slot's history, or row among the step's new rows

inline uint64_t pipeline_rows_out(uint64_t received, uint32_t c, bool finished) { return finished ? received : received > c ? received - c : 0; }
SR_SPLICE_HD inline uint64_t pipeline_hist_rows(uint64_t received, uint32_t c) { return received < 2ull * c ? received : 2ull * c; }
// where a step's kernel finds input row g of an utterance that had `received` rows before the step (g within the step's need)
SR_SPLICE_HD inline PipelineSource pipeline_source(uint32_t c, uint64_t received, uint64_t g) {
  if (g >= received) return {false, g - received};
  return {true, (uint32_t)g % (2u * c)};  // (rows are counted in 32 bits: max_frames < 2^32; a 32-bit division on the device)
}
// the new input rows [keep0, received + k) of a step go into the history, row g at position g mod 2c
SR_SPLICE_HD inline uint64_t pipeline_keep0(uint32_t c, uint64_t received, uint64_t k) {
  const uint64_t after = received + k, first = after - pipeline_hist_rows(after, c);
  return first > received ? first : received;
}

// the step that takes k new input rows (finishing: no more follow)
inline PipelineStep plan_pipeline_step(uint32_t c, const PipelineCarry& s, uint64_t k, bool finishing) {
  PipelineStep p;
  p.rows_in = k;
  p.next.received = s.received + k;
  p.next.finished = finishing;
  p.row0 = s.searched;
  p.rows = pipeline_rows_out(p.next.received, c, finishing) - p.row0;
  p.next.searched = p.row0 + p.rows;
  p.hist_rows = pipeline_hist_rows(s.received, c);
  if (p.rows) {
    p.need0 = (uint64_t)splice_frame((int64_t)p.row0, 0, c, 0, (int64_t)p.next.received);
    p.need1 = (uint64_t)splice_frame((int64_t)(p.row0 + p.rows - 1), 2ll * c, c, 0, (int64_t)p.next.received) + 1;
  }
  p.keep0 = pipeline_keep0(c, s.received, k);
  return p;
}

}  // namespace srplan
