"""HIP-event time of the MAP statistics (sr_map_statistics_corpus, the filled call with cap = total frames) beside
sr_mllr_statistics_corpus with one class and sr_accumulate_corpus, in one process on one tree:
  (a) the shape of profiles/mllr.txt: 4000 states x 32 densities, dimension 39, 1000 utterances of 200..400 frames, 16 and 1000
      speakers, a seeded uniform alignment, arg-min memberships;
  (b) the case the segments exist for: one speaker, 106 states x 8 densities at dimension 25 (the real-speech model's shape) over as
      many frames, a seeded alignment that gives state 0 ("silence") 30 % of the frames: entries of thousands of pairs, which
      mllr_entry_kernel walks with one wave each;
  (c) sr_model_map_adapt of one speaker's entries at 128 000 densities beside sr_model_transform_means with one class: the wall time of
      the call and of the new model's release.
The statistics' times are the library's own event pairs (sr_profile_*: keys, sort, runs, plan and sums count under search_ms, like
sr_accumulate_corpus' kernels; the host read between plan and sums is outside the pairs); the wall times are the whole calls (pairs,
host reads, the copies of the results).  Writes profiles/map.txt (or --out).

  python tools/map_time.py [--out PATH] [--reps N] [--no-write]"""
import argparse
import os
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
sys.path.insert(0, ROOT)

from tools.mllr_time import profiled  # noqa: E402


def map_call(capi, c, states, spk, S):
    """the filled call alone: with arg-min memberships of an alignment, cap = total frames always suffices"""
    D, F = c.model.dim, c.n_frames
    off, dens, occ, x = np.zeros(S + 1, np.uint64), np.zeros(F, np.uint32), np.zeros(F), np.zeros((F, D))
    P = lambda a: a.ctypes.data  # noqa: E731

    def call():
        capi._check(capi.lib().sr_map_statistics_corpus(c.model.h, c.h, P(states), P(spk), S, 1, F, P(off), P(dens), P(occ), P(x)))
        n = int(off[-1])
        return off, dens[:n], occ[:n], x[:n]
    return call


def shape(capi, synth, n_states, n_mix, D, speakers, states_of, reps, lines, seed):
    spec = synth.make_mixset(n_states, n_mix, D, seed=seed)
    mp = os.path.join(tempfile.mkdtemp(), "m.mix")
    synth.write_mixset(mp, spec)
    feats, off = synth.make_batch(1000, 200, 400, D, seed=7)
    F = int(off[-1])
    states = states_of(F)
    out = None
    with capi.Model.from_mixset(mp, D) as m:
        c = m.upload(feats, off)
        lines.append(f"{n_states} states x {n_mix} densities (dim {D}), 1000 utterances, {F} frames, arg-min memberships")
        _, acc_ms, acc_wall = profiled(m, lambda: c.accumulate(states, False, True), reps)
        lines.append(f"  sr_accumulate_corpus (yardstick)             kernels {acc_ms:8.3f} ms   call {acc_wall:9.2f} ms")
        cls = np.zeros(m.n_densities, np.uint32)
        for S in speakers:
            spk = (np.arange(1000) % S).astype(np.uint32)
            (beta, _, _), ml_ms, ml_wall = profiled(m, lambda: c.mllr_statistics(states, spk, S, cls, 1, True), reps)
            assert beta.sum() == F
            lines.append(f"  sr_mllr_statistics_corpus S = {S:4d} R = 1      kernels {ml_ms:8.3f} ms   call {ml_wall:9.2f} ms   "
                         f"{ml_ms / acc_ms:5.2f} x the yardstick's kernels")
            (eo, dens, occ, x), ms, wall = profiled(m, map_call(capi, c, states, spk, S), reps)
            assert occ.sum() == F
            lines.append(f"  sr_map_statistics_corpus  S = {S:4d}            kernels {ms:8.3f} ms   call {wall:9.2f} ms   "
                         f"{ms / acc_ms:5.2f} x the yardstick's, {ms / ml_ms:5.2f} x MLLR's kernels   "
                         f"({len(dens)} entries, the longest {int(occ.max())} pairs)")
            if out is None:
                e = eo.astype(np.int64)
                out = (dens[e[0]:e[1]].copy(), occ[e[0]:e[1]].copy(), x[e[0]:e[1]].copy())
        if n_states * n_mix == 128000:   # (c)
            W = np.hstack([np.eye(D), np.zeros((D, 1))])[None] + 0.01 * np.random.default_rng(5).normal(size=(1, D, D + 1))
            for name, f in (("sr_model_transform_means R = 1", lambda: m.transform_means(cls, W).close()),
                            ("sr_model_map_adapt, means     ", lambda: m.map_adapt(*out, 10.0).close()),
                            ("sr_model_map_adapt, + weights ", lambda: m.map_adapt(*out, 10.0, 10.0).close())):
                f()
                t0 = time.perf_counter()
                for _ in range(reps):
                    f()
                lines.append(f"  {name}               call + destroy {(time.perf_counter() - t0) * 1e3 / reps:8.2f} ms wall "
                             f"({m.n_densities} densities, {len(out[0])} entries)")
        c.close()


def measure(reps):
    from speechrecognition_amd import build, capi, synth
    info = build.build_info()
    head = info.get("git_head", "unknown")
    where = f"the tree of the change that adds MAP adaptation, over parent commit {head}" if info.get("dirty") else f"commit {head}"
    lines = [f"{where}; one process, one GPU run; mean of {reps} calls after one warm-up.  Expectation, stated before the run: the MAP "
             "kernels cost no more than MLLR's with one class (the same sort, the entry sums, no contraction)."]
    rng = np.random.default_rng(5)
    lines.append("(a) the shape of profiles/mllr.txt, a uniform seeded alignment")
    shape(capi, synth, 4000, 32, 39, (16, 1000), lambda F: rng.integers(0, 4000, size=F).astype(np.uint16), reps, lines, 23)

    def skewed(F):   # state 0 takes 30 % of the frames
        st = rng.integers(1, 106, size=F)
        st[rng.uniform(size=F) < 0.3] = 0
        return st.astype(np.uint16)
    lines.append("(b) one speaker, the real-speech model's shape, state 0 on 30 % of the frames")
    shape(capi, synth, 106, 8, 25, (1,), skewed, reps, lines, 29)
    return lines


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "map.txt"))
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--no-write", action="store_true")
    a = ap.parse_args()
    lines = measure(a.reps)
    print("\n".join(lines))
    if not a.no_write:
        with open(a.out, "w") as f:
            f.write("MAP statistics and adapted model (tools/map_time.py)\n" + "\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
