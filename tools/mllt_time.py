"""HIP-event time of the MLLT statistics (sr_mllt_statistics_corpus) at the benchmark model's shape, that of profiles/fmllr.txt:
4000 states x 32 densities, dimension 39, 1000 utterances of 200..400 frames, a seeded alignment; once with arg-min memberships (one
pair per frame) and once with soft memberships (32 pairs per frame, the dropped ones keeping their place).  Beside them, in the same
run on the same corpus and alignment, sr_fmllr_statistics_corpus with one speaker and sr_accumulate_corpus, each in the same mode.
The kernels' times are the library's own event pairs (sr_profile_*: the contraction and the reduction of every round count under
search_ms, like sr_accumulate_corpus' kernels); the wall times are the whole calls (pairs, launches, the copy of G).  The contraction's
FP64 rate is 2 * pairs * R * cols / the kernels' time (R = 48 rows, cols = 784 at D = 39; padding counted, as the instruction runs
it), quoted as a share of the 78.6 TFLOP/s FP64 matrix peak DESIGN.md uses.  One process, one warm-up call before each mean.
Writes profiles/mllt.txt (or --out).

  python tools/mllt_time.py [--out PATH] [--reps N] [--no-write]"""
import argparse
import os
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
sys.path.insert(0, ROOT)

PEAK_TFLOPS = 78.6


def profiled(m, f, reps):
    """-> (result, search_ms per call, wall ms per call) after one warm-up"""
    f()
    m.profile(True)
    t0 = time.perf_counter()
    for _ in range(reps):
        r = f()
    wall = (time.perf_counter() - t0) / reps
    p = m.profile_read()
    m.profile(False)
    return r, p["search_ms"] / reps, wall * 1e3


def measure(reps):
    from speechrecognition_amd import build, capi, synth
    D, M = 39, 32
    rows, cols = (D + 1 + 15) // 16 * 16, (D * (D + 1) // 2 + 1 + 15) // 16 * 16
    spec = synth.make_mixset(4000, M, D, seed=23)
    mp = os.path.join(tempfile.mkdtemp(), "m.mix")
    synth.write_mixset(mp, spec)
    feats, off = synth.make_batch(1000, 200, 400, D, seed=7)
    F = int(off[-1])
    rng = np.random.default_rng(5)
    states = rng.integers(0, 4000, size=F).astype(np.uint16)
    spk = np.zeros(1000, np.uint32)
    info = build.build_info()
    head = info.get("git_head", "unknown")
    where = f"the tree of the change that adds MLLT, over parent commit {head}" if info.get("dirty") else f"commit {head}"
    lines = [f"{where}; 1000 utterances, {F} frames, 4000 states x {M} densities (dim {D}); mean of {reps} calls after one warm-up; "
             f"workspace {os.environ.get('SRGPU_MLLT_MB', '256')} MiB"]
    with capi.Model.from_mixset(mp, D) as m:
        c = m.upload(feats, off)
        for name, max_approx, pairs in (("arg-min", True, F), ("soft", False, F * M)):
            _, acc_ms, acc_wall = profiled(m, lambda: c.accumulate(states, False, max_approx), reps)
            (fb, _, _), fm_ms, fm_wall = profiled(m, lambda: c.fmllr_statistics(states, spk, 1, max_approx), reps)
            (beta, G), ms, wall = profiled(m, lambda: c.mllt_statistics(states, max_approx), reps)
            assert abs(beta - F) <= 1e-6 * F and abs(fb[0] - F) <= 1e-6 * F
            tf = 2.0 * pairs * rows * cols / (ms * 1e-3) / 1e12
            lines.append(f"  {name} memberships: {pairs} pairs, {(pairs + 1023) // 1024} segments")
            lines.append(f"    sr_accumulate_corpus (yardstick)        kernels {acc_ms:9.3f} ms   call {acc_wall:9.2f} ms")
            lines.append(f"    sr_fmllr_statistics_corpus, 1 speaker   kernels {fm_ms:9.3f} ms   call {fm_wall:9.2f} ms")
            lines.append(f"    sr_mllt_statistics_corpus               kernels {ms:9.3f} ms   call {wall:9.2f} ms   "
                         f"{ms / acc_ms:6.2f} x the yardstick's kernels, {ms / fm_ms:6.2f} x the fMLLR statistics'")
            lines.append(f"    contraction {tf:6.2f} TFLOP/s FP64 = {tf / PEAK_TFLOPS:5.3f} of the {PEAK_TFLOPS} TF matrix peak "
                         f"(2 x {pairs} x {rows} x {cols} flop; the reduction's time included)")
        c.close()
    return lines


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "mllt.txt"))
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--no-write", action="store_true")
    a = ap.parse_args()
    lines = measure(a.reps)
    print("\n".join(lines))
    if not a.no_write:
        with open(a.out, "w") as f:
            f.write("MLLT statistics (tools/mllt_time.py)\n" + "\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
