"""HIP-event time of the LDA calls (sr_lda_statistics_corpus, sr_corpus_splice_transform) at the benchmark's corpus shape: 1000
utterances of 200..400 frames, dimension 25 and 39, context 4 (E = 225 and 351), the 4000 states of a seeded alignment as the classes,
p = 40.  Beside them, in the same run on the same corpus and alignment, sr_accumulate_corpus and sr_mllt_statistics_corpus (arg-min
memberships) of a 4000 x 32 model.  The kernels' times are the library's own event pairs (sr_profile_*: search_ms); the wall times
are the whole calls (lists, launches, copies).  Rates:
  scatter   the flop the statistic needs, 2 F E^2 / 2, and the flop the matrix instruction runs (every live 16 x 16 tile of the upper
            triangle's 64 x 64 blocks, padding and the diagonal blocks' upper tiles included), both over the statistics' kernel time --
            class sums and reductions included, so the scatter kernel's own rate is a little higher -- as shares of the 78.6 TFLOP/s
            FP64 matrix peak DESIGN.md uses
  project   the bytes that must move, 4 F (D + p), and the flop, 2 F p E, over its kernel time
One process, one warm-up call before each mean.  Writes profiles/lda.txt (or --out); the estimate's worst residual ratios printed by
tests/test_lda_cpu.py are appended by hand.

  python tools/lda_time.py [--out PATH] [--reps N] [--no-write]"""
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


def executed_tiles(E):
    """live 16 x 16 tiles the scatter kernel runs per 4 items"""
    nP, n = (E + 63) // 64, 0
    for I in range(nP):
        for J in range(I, nP):
            for r in range(4):
                for q in range(4):
                    n += I * 64 + r * 16 < E and J * 64 + q * 16 < E and not (I == J and r > q)
    return n


def measure(reps):
    from speechrecognition_amd import build, capi, synth
    S, M, context, p = 4000, 32, 4, 40
    info = build.build_info()
    head = info.get("git_head", "unknown")
    where = f"the tree of the change that adds LDA, over parent commit {head}" if info.get("dirty") else f"commit {head}"
    lines = []
    for D in (25, 39):
        E = (2 * context + 1) * D
        spec = synth.make_mixset(S, M, D, seed=23)
        mp = os.path.join(tempfile.mkdtemp(), "m.mix")
        synth.write_mixset(mp, spec)
        feats, off = synth.make_batch(1000, 200, 400, D, seed=7)
        F = int(off[-1])
        states = np.random.default_rng(5).integers(0, S, size=F).astype(np.uint16)
        if not lines:
            lines.append(f"{where}; 1000 utterances, {F} frames, {S} states x {M} densities; context {context}, p = {p}; mean of {reps} calls "
                         f"after one warm-up; workspace {os.environ.get('SRGPU_LDA_MB', '256')} MiB")
        Mx = np.random.default_rng(6).normal(size=(p, E + 1)) / np.sqrt(E)
        with capi.Model.from_mixset(mp, D) as m, capi.Model.from_tables(np.arange(S + 1, dtype=np.uint32), np.zeros((S, p)), np.ones((S, p)),
                                                                        np.zeros(S), np.zeros(S)) as target:
            c = m.upload(feats, off)
            _, acc_ms, acc_wall = profiled(m, lambda: c.accumulate(states, False, True), reps)
            (beta, _), ml_ms, ml_wall = profiled(m, lambda: c.mllt_statistics(states, True), reps)
            (count, _, _), ms, wall = profiled(m, lambda: c.lda_statistics(states, context, None, S), reps)
            assert count.sum() == F and abs(beta - F) <= 1e-6 * F

            def project():
                c.splice_transform(target, context, Mx).close()

            _, pr_ms, pr_wall = profiled(m, project, reps)
            c.close()
        need = float(F) * E * E
        run = 2.0 * F / 4 * executed_tiles(E) * 16 * 16 * 4
        lines.append(f"  dimension {D}, E = {E}: {(F + 1023) // 1024} segments of {(E + 63) // 64 * ((E + 63) // 64 + 1) // 2} blocks")
        lines.append(f"    sr_accumulate_corpus, arg-min (yardstick)   kernels {acc_ms:9.3f} ms   call {acc_wall:9.2f} ms")
        lines.append(f"    sr_mllt_statistics_corpus, arg-min          kernels {ml_ms:9.3f} ms   call {ml_wall:9.2f} ms")
        lines.append(f"    sr_lda_statistics_corpus                    kernels {ms:9.3f} ms   call {wall:9.2f} ms   "
                     f"{ms / acc_ms:6.2f} x the yardstick's kernels, {ms / ml_ms:6.2f} x the MLLT statistics'")
        lines.append(f"      scatter, needed   {need / 1e9:7.2f} GFLOP -> {need / (ms * 1e-3) / 1e12:6.2f} TFLOP/s FP64 = "
                     f"{need / (ms * 1e-3) / 1e12 / PEAK_TFLOPS:5.3f} of the {PEAK_TFLOPS} TF matrix peak")
        lines.append(f"      scatter, executed {run / 1e9:7.2f} GFLOP -> {run / (ms * 1e-3) / 1e12:6.2f} TFLOP/s FP64 = "
                     f"{run / (ms * 1e-3) / 1e12 / PEAK_TFLOPS:5.3f} of the peak (class sums' and reductions' time included)")
        by, fl = 4.0 * F * (D + p), 2.0 * F * p * E
        lines.append(f"    sr_corpus_splice_transform, p = {p}          kernels {pr_ms:9.3f} ms   call {pr_wall:9.2f} ms   "
                     f"{by / (pr_ms * 1e-3) / 1e9:7.1f} GB/s of the {by / 1e6:.1f} MB that must move, "
                     f"{fl / (pr_ms * 1e-3) / 1e12:5.2f} TFLOP/s FP64 (vector, unfused)")
    return lines


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "lda.txt"))
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--no-write", action="store_true")
    a = ap.parse_args()
    lines = measure(a.reps)
    print("\n".join(lines))
    if not a.no_write:
        with open(a.out, "w") as f:
            f.write("LDA statistics and projection (tools/lda_time.py)\n" + "\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
