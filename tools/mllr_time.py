"""HIP-event time of the MLLR statistics (sr_mllr_statistics_corpus) at the benchmark model's shape: 4000 states x 32 densities,
dimension 39, 1000 utterances of 200..400 frames, 16 and 1000 speakers, 1 and 8 regression classes (density d in class d mod 8), a
seeded alignment, arg-min memberships.  Beside them, in the same run, sr_fmllr_statistics_corpus and sr_accumulate_corpus on the same
corpus and alignment, and sr_model_transform_means of one speaker's transforms.  The statistics' times are the library's own event pairs
(sr_profile_*: keys, sorts and runs, entry sums, contraction and reduction count under search_ms, like sr_accumulate_corpus' kernels;
the two host reads between them are outside the pairs); the wall times are the whole calls (pairs, host reads, the copies of the
results).  The transform has no event pair: its time is the wall time of the call and of the new model's release.
Writes profiles/mllr.txt (or --out).

  python tools/mllr_time.py [--out PATH] [--reps N] [--no-write]"""
import argparse
import os
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
sys.path.insert(0, ROOT)


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
    info = build.build_info()
    head = info.get("git_head", "unknown")
    where = f"the tree of the change that adds MLLR, over parent commit {head}" if info.get("dirty") else f"commit {head}"
    lines = [f"{where}; 1000 utterances, {F} frames, 4000 states x 32 densities (dim {D}), arg-min memberships; "
             f"mean of {reps} calls after one warm-up"]
    with capi.Model.from_mixset(mp, D) as m:
        c = m.upload(feats, off)
        _, acc_ms, acc_wall = profiled(m, lambda: c.accumulate(states, False, True), reps)
        lines.append(f"  sr_accumulate_corpus (yardstick)             kernels {acc_ms:8.3f} ms   call {acc_wall:9.2f} ms")
        for S in (16, 1000):
            spk = (np.arange(1000) % S).astype(np.uint32)
            (beta, _, _), ms, wall = profiled(m, lambda: c.fmllr_statistics(states, spk, S, True), reps)
            assert beta.sum() == F
            lines.append(f"  sr_fmllr_statistics_corpus S = {S:4d}           kernels {ms:8.3f} ms   call {wall:9.2f} ms")
            for R in (1, 8):
                cls = (np.arange(m.n_densities) % R).astype(np.uint32)
                (beta, k, G), ms, wall = profiled(m, lambda: c.mllr_statistics(states, spk, S, cls, R, True), reps)
                assert beta.sum() == F
                lines.append(f"  sr_mllr_statistics_corpus  S = {S:4d} R = {R}     kernels {ms:8.3f} ms   call {wall:9.2f} ms   "
                             f"{ms / acc_ms:5.2f} x the yardstick's kernels")
                del k, G
        for R in (1, 8):
            cls = (np.arange(m.n_densities) % R).astype(np.uint32)
            W = np.tile(np.hstack([np.eye(D), np.zeros((D, 1))]), (R, 1, 1)) + 0.01 * rng.normal(size=(R, D, D + 1))
            m.transform_means(cls, W).close()
            t0 = time.perf_counter()
            for _ in range(reps):
                m.transform_means(cls, W).close()
            lines.append(f"  sr_model_transform_means R = {R}                 call + destroy {(time.perf_counter() - t0) * 1e3 / reps:8.2f} ms "
                         f"wall ({m.n_densities} densities)")
        c.close()
    return lines


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "mllr.txt"))
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--no-write", action="store_true")
    a = ap.parse_args()
    lines = measure(a.reps)
    print("\n".join(lines))
    if not a.no_write:
        with open(a.out, "w") as f:
            f.write("MLLR statistics and adapted model (tools/mllr_time.py)\n" + "\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
