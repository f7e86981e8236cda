"""Time of sr_model_split (4000 states x 32 densities -> 4000 x 64, dimension 39) and of sr_model_eliminate back to 4000 x 32, with
sr_model_create_from_accumulated at the 4000 x 32 shape in the same run as the yardstick: the model update every EM iteration
already pays.  Per call the wall time (host plan, model shell, uploads, kernel, log weights) and the HIP-event time of the expansion
kernel alone (the library's own event pair, SRGPU_STRUCT_TIMING); what is left of the wall time is host work, allocations and the
small uploads (plan, tying, log weights).  Mean of --reps calls after one warm-up.
Writes profiles/model_structure.txt (or --out).

  python tools/structure_time.py [--out PATH] [--reps N] [--no-write]"""
import argparse
import os
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
sys.path.insert(0, ROOT)


def timed(f, reps):
    """-> (wall ms, expansion kernel's HIP-event ms or None) per call after one warm-up; f returns a Model, closed outside the timed part.
    The kernel time is the library's own event pair (SRGPU_STRUCT_TIMING: one line on stderr per call), read back through a file."""
    f().close()
    sys.stderr.flush()
    keep = os.dup(2)
    with tempfile.TemporaryFile() as tmp:
        os.dup2(tmp.fileno(), 2)
        try:
            wall = 0.0
            for _ in range(reps):
                t0 = time.perf_counter()
                m = f()
                wall += time.perf_counter() - t0
                m.close()
        finally:
            os.dup2(keep, 2)
            os.close(keep)
        tmp.seek(0)
        ms = [float(ln.split()[3]) for ln in tmp.read().decode().splitlines() if ln.startswith("[structure] expand kernel")]
    return wall * 1e3 / reps, (sum(ms) / len(ms) if ms else None)


def measure(reps):
    os.environ["SRGPU_STRUCT_TIMING"] = "1"     # read once, at the library's first split or eliminate
    from speechrecognition_amd import build, capi
    D, S, M = 39, 4000, 32
    rng = np.random.default_rng(3)
    off = (np.arange(S + 1) * M).astype(np.uint32)
    C = S * M
    var = rng.uniform(0.5, 2.0, size=(C, D))
    tables = (rng.normal(size=(C, D)), 1 / var, (D * np.log(2 * np.pi) + np.log(var).sum(axis=1)) / 2, np.full(C, -np.log(M)))
    feats = rng.normal(size=(20000, D)).astype(np.float32)
    foff = np.arange(0, 20001, 200).astype(np.uint64)
    states = rng.integers(0, S, size=len(feats)).astype(np.uint16)
    info = build.build_info()
    where = f"commit {info.get('git_head', 'unknown')}" + (" with uncommitted changes" if info.get("dirty") else "")
    lines = [f"{where}; {S} states, dimension {D}; mean of {reps} calls after one warm-up; wall = the whole call, kernel = HIP events "
             f"around the expansion kernel, rest = wall - kernel (host plan, shell, allocations, uploads, log weights)"]

    def row(name, wall, dev):
        k = f"kernel {dev:8.3f} ms   rest {wall - dev:8.2f} ms" if dev is not None else "(no kernel of this change)"
        lines.append(f"  {name:58s} wall {wall:8.2f} ms   {k}")

    with capi.Model.from_tables(off, *tables) as m:
        w = np.ones(C)
        row(f"sr_model_split {S} x {M} -> {S} x {2 * M} (host weights)", *timed(lambda: m.split(w, 0.0, 0.2), reps))
        c = m.upload(feats, foff)
        c.accumulate_on_device(states, False, True)
        row(f"sr_model_split {S} x {M} -> {S} x {2 * M} (resident weights)", *timed(lambda: m.split(c, 0.0, 0.2), reps))
        row(f"sr_model_create_from_accumulated {S} x {M} (yardstick)", *timed(lambda: c.next_model(), reps))
        c.close()
        big = m.split(w, 0.0, 0.2)
        w2 = np.concatenate([np.ones(C), np.zeros(C)])       # the upper children starve
        row(f"sr_model_eliminate {S} x {2 * M} -> {S} x {M}", *timed(lambda: big.eliminate(w2, 0.5), reps))
        back = big.eliminate(w2, 0.5)
        assert back.n_densities == C and big.n_densities == 2 * C
        back.close()
        big.close()
    return lines


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "model_structure.txt"))
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--no-write", action="store_true")
    a = ap.parse_args()
    lines = measure(a.reps)
    print("\n".join(lines))
    if not a.no_write:
        with open(a.out, "w") as f:
            f.write("sr_model_split / sr_model_eliminate (tools/structure_time.py)\n" + "\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
