"""HIP-event time of the fMLLR statistics (sr_fmllr_statistics_corpus) and of the adapted corpus (sr_corpus_transform) at the
benchmark model's shape: 4000 states x 32 densities, dimension 39, 1000 utterances of 200..400 frames, 16 and 1000 speakers, a
seeded alignment, arg-min memberships.  Beside them, in the same run, sr_accumulate_corpus on the same corpus and alignment: the
yardstick.  The times are the library's own event pairs (sr_profile_*: the fold, the contraction and the reduction count under
search_ms, like sr_accumulate_corpus' kernels); the rate is the algorithmic 2 D (D+1)^2 flops per frame of G over that time against
the 78.6 TF FP64 matrix peak DESIGN.md uses; the transform's kernel is timed the same way.  Wall times of the whole calls (pairs,
copies of the results, the new corpus' allocation and release) are printed too.
Writes profiles/fmllr.txt (or --out).

  python tools/fmllr_time.py [--out PATH] [--reps N] [--no-write]"""
import argparse
import os
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
sys.path.insert(0, ROOT)

PEAK = 78.6e12


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
    D = 39
    spec = synth.make_mixset(4000, 32, D, seed=23)
    mp = os.path.join(tempfile.mkdtemp(), "m.mix")
    synth.write_mixset(mp, spec)
    feats, off = synth.make_batch(1000, 200, 400, D, seed=7)
    F = int(off[-1])
    rng = np.random.default_rng(5)
    states = rng.integers(0, 4000, size=F).astype(np.uint16)
    flops = 2.0 * D * (D + 1) ** 2 * F
    info = build.build_info()
    where = f"commit {info.get('git_head', 'unknown')}" + (" with uncommitted changes" if info.get("dirty") else "")
    lines = [f"{where}; 1000 utterances, {F} frames, 4000 states x 32 "
             f"densities (dim {D}), arg-min memberships; mean of {reps} calls after one warm-up; G: {flops:.3e} flops"]
    with capi.Model.from_mixset(mp, D) as m:
        c = m.upload(feats, off)
        _, acc_ms, acc_wall = profiled(m, lambda: c.accumulate(states, False, True), reps)
        lines.append(f"  sr_accumulate_corpus (yardstick)      kernels {acc_ms:8.3f} ms   call {acc_wall:8.2f} ms")
        for S in (16, 1000):
            spk = (np.arange(1000) % S).astype(np.uint32)
            (beta, k, G), ms, wall = profiled(m, lambda: c.fmllr_statistics(states, spk, S, True), reps)
            assert beta.sum() == F
            lines.append(f"  sr_fmllr_statistics_corpus S = {S:4d}    kernels {ms:8.3f} ms   call {wall:8.2f} ms   "
                         f"{flops / (ms * 1e-3) / 1e12:6.2f} TFLOP/s FP64 = {flops / (ms * 1e-3) / PEAK:.3f} of the matrix peak   "
                         f"{ms / acc_ms:5.2f} x the yardstick's kernels")
            W = np.tile(np.hstack([np.eye(D), np.zeros((D, 1))]), (S, 1, 1)) + 0.01 * rng.normal(size=(S, D, D + 1))

            def tr():
                t = c.transform(spk, W)
                t.close()
            _, tr_ms, tr_wall = profiled(m, tr, reps)
            lines.append(f"  sr_corpus_transform S = {S:4d}           kernel  {tr_ms:8.3f} ms   call + destroy {tr_wall:8.2f} ms   "
                         f"{8.0 * F * D / (tr_ms * 1e-3) / 1e12:6.3f} TB/s of rows in and out")
        c.close()
    return lines


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "fmllr.txt"))
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--no-write", action="store_true")
    a = ap.parse_args()
    lines = measure(a.reps)
    print("\n".join(lines))
    if not a.no_write:
        with open(a.out, "w") as f:
            f.write("fMLLR statistics and adapted corpus (tools/fmllr_time.py)\n" + "\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
