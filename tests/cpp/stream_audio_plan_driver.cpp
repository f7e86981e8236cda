// stream_audio_plan_driver -- runs speechrecognition_amd/csrc/stream_audio_plan.h (host code, no HIP) for tests/test_stream_audio_cpu.py.
// Input file, a case per line:  window shift step n_cuts cut_1 .. cut_n   -- the utterance's samples arrive in pieces of cut_i samples,
// then the finish.  Sample i of the utterance has the value i - 20000, so a piece's contents tell where they come from.
// Output per case: a line per step (the pushes, then the finish)
//   step <row0> <rows> <statics before> <new statics> <carried samples after> <skip after> <piece ok>
//        <start of every new frame, read from the piece> ... | <the sample before each, read from the piece (0 before sample 0)> ...
// and "end".  "piece ok": every new frame's `window` samples in the piece are the utterance's.
#include <cstdio>
#include <cstdlib>
#include <fstream>
#include <sstream>
#include <string>
#include <vector>

#include "stream_audio_plan.h"

int main(int argc, char** argv) {
  if (argc != 2) { fprintf(stderr, "usage: %s cases.txt\n", argv[0]); return 2; }
  std::ifstream in(argv[1]);
  std::string line;
  while (std::getline(in, line)) {
    if (line.empty()) continue;
    std::istringstream ls(line);
    uint32_t window, shift, step;
    size_t n_cuts;
    ls >> window >> shift >> step >> n_cuts;
    std::vector<uint64_t> cuts(n_cuts);
    uint64_t N = 0;
    for (auto& c : cuts) { ls >> c; N += c; }
    if (!ls || N > 50000) { fprintf(stderr, "bad case: %s\n", line.c_str()); return 2; }
    std::vector<int16_t> x(N);
    for (uint64_t i = 0; i < N; i++) x[i] = (int16_t)((int64_t)i - 20000);
    srplan::AudioCarry carry;
    uint64_t at = 0;
    for (size_t i = 0; i <= n_cuts; i++) {
      const bool finishing = i == n_cuts;
      const uint64_t n = finishing ? 0 : cuts[i];
      // exactly n samples of their own, so that a read past them is a read past an allocation
      std::vector<int16_t> piece_in(x.begin() + at, x.begin() + at + n);
      const srplan::AudioStep s = srplan::plan_audio_step(window, shift, step, carry, n ? piece_in.data() : nullptr, n, finishing);
      std::vector<int16_t> piece(1 + s.n_buf);
      srplan::audio_fill(carry, s, n ? piece_in.data() : nullptr, n, piece.data());
      bool ok = true;
      std::string starts, prevs;
      for (uint64_t j = 0; j < s.new_statics; j++) {
        const uint64_t o = 1 + j * shift, first = (carry.statics + j) * shift;
        for (uint32_t k = 0; k < window; k++) ok = ok && o + k < piece.size() && piece[o + k] == (int16_t)((int64_t)(first + k) - 20000);
        starts += " " + std::to_string((int64_t)piece[o] + 20000);
        prevs += " " + std::to_string((int)piece[o - 1]);
      }
      printf("step %llu %llu %llu %llu %zu %llu %d%s |%s\n", (unsigned long long)s.row0, (unsigned long long)s.rows,
             (unsigned long long)carry.statics, (unsigned long long)s.new_statics, s.next.tail.size(), (unsigned long long)s.next.skip, ok ? 1 : 0,
             starts.c_str(), prevs.c_str());
      carry = s.next;
      at += n;
    }
    printf("end\n");
  }
  return 0;
}
