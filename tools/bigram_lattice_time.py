"""Wall time of the bigram search's word lattices (sr_bigram_word_lattice_corpus) beside its posterior call
(sr_bigram_word_posteriors_corpus) and the bigram search itself, in one run, on BASELINE configs[4]'s shape as
tools/bigram_posteriors_time.py draws it: 2667 words, 1000 utterances of 200..400 frames (302 685 frames), features resident.
Timed: the sizing call at beam +inf, the sizing call and the filling call at a finite beam, both arg-min routes of the min-plus
entry (SRGPU_BGLAT_ARGMIN), the posterior call (kappa = 0.1) and the search (beam 200).  The kernel split comes from one run of this
tool's --child under rocprofv3 --kernel-trace --stats, started by the tool itself.  Writes profiles/bigram_lattice.txt (or --out).

  python tools/bigram_lattice_time.py [--out PATH] [--reps N] [--utts N] [--beam B] [--no-profile]"""
import argparse
import csv
import ctypes as C
import glob
import os
import shutil
import subprocess
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from bigram_posteriors_time import BG_TDP, KAPPA, setup, timed  # noqa: E402


def sizing(capi, m, c, bg, beam):
    off = np.zeros(c.n_utts + 1, np.uint64)
    best = np.zeros(max(c.n_utts, 1))
    capi._check(capi.lib().sr_bigram_word_lattice_corpus(m.h, c.h, bg.h, capi.GMM_PREFILTER, float(beam), 0, capi._ptr(off), capi._ptr(best),
                                                         *([None] * 8)))
    return int(off[-1]), best


def measure(reps, n_utts, beam, child):
    from speechrecognition_amd import capi
    lex, mp, feats, off, lm = setup(n_utts)
    word_off, aut, sil_state = lex.flatten()
    F, W = int(off[-1]), lex.n_words
    lines = []
    with capi.Model.from_mixset(mp, 39) as m:
        bg = m.bigram(word_off, aut, lex.silence_idx, lm, BG_TDP)
        c = m.upload(feats, off)
        if child:  # under the profiler: the sizing call twice (warm-up and one more)
            sizing(capi, m, c, bg, np.inf)
            sizing(capi, m, c, bg, np.inf)
            c.close()
            bg.close()
            return []
        (n_inf, best), t_inf = timed(lambda: sizing(capi, m, c, bg, np.inf), reps)
        (n_b, _), t_size = timed(lambda: sizing(capi, m, c, bg, beam), reps)
        r, t_both = timed(lambda: c.bigram_word_lattice(bg, beam), 1)
        os.environ["SRGPU_BGLAT_ARGMIN"] = "rescan"
        (n_inf2, best2), t_rescan = timed(lambda: sizing(capi, m, c, bg, np.inf), reps)
        del os.environ["SRGPU_BGLAT_ARGMIN"]
        assert n_inf2 == n_inf and best2.tobytes() == best.tobytes()
        (cost, *_), t_post = timed(lambda: c.bigram_word_posteriors(bg, KAPPA, capi.GMM_PREFILTER, 1e-4, 4), reps)
        _, t_rec = timed(lambda: c.recognize_bigram(bg, 200.0, capi.FLT_MAX), reps)
        c.close()
        bg.close()
    P = int(word_off[-1]) + W * int(word_off[lex.silence_idx + 1] - word_off[lex.silence_idx])
    lines = [
        f"configs[4] shape: {n_utts} utterances, {F} frames, {lex.n_states} states x 64 densities (dim 39), {W} words, {P} positions "
        f"(words and silence copies); mean of {reps} calls after one warm-up, features resident, SRGPU_FB_MB default",
        f"  min-plus entry: W^2 (add, min) pairs per (frame, utterance) and direction = {2.0 * W * W * F:.4g} pairs per call",
        f"  sizing call, beam +inf, arg-min by compare-and-select      {t_inf * 1e3:10.1f} ms   arcs {n_inf} ({n_inf / F:.1f} per frame), finite best: {int(np.isfinite(best).sum())} of {len(best)}",
        f"  sizing call, beam +inf, arg-min by equality rescan         {t_rescan * 1e3:10.1f} ms   (same counts and best, bit for bit)",
        f"  sizing call, beam {beam:g}                                  {t_size * 1e3:10.1f} ms   arcs {n_b} ({n_b / F:.2f} per frame)",
        f"  sizing + filling call, beam {beam:g} (one call each)        {t_both * 1e3:10.1f} ms   filling alone about {(t_both - t_size) * 1e3:.1f} ms",
        f"  sr_bigram_word_posteriors_corpus (kappa {KAPPA}, 4 items)      {t_post * 1e3:10.1f} ms   finite F: {int(np.isfinite(cost).sum())} of {len(cost)}",
        f"  sr_recognize_bigram_corpus (beam 200)                      {t_rec * 1e3:10.1f} ms",
        f"  lattice sizing call / posterior call = {t_inf / t_post:.2f}",
    ]
    return lines


def kernel_table(path):
    rows = [(r["Name"], int(r["Calls"]), float(r["TotalDurationNs"])) for r in csv.DictReader(open(path))]
    total = sum(r[2] for r in rows)
    short = lambda n: n.replace("void ", "").replace("srgpu::", "").split("(")[0]  # noqa: E731
    out = ["", "rocprofv3 --kernel-trace --stats, one run of this tool's --child (the sizing call at beam +inf twice: warm-up and one more); "
           "the lattice's own kernels first, then the rest by time:",
           f"  {'kernel':60s} {'calls':>7s} {'total ms':>10s} {'avg us':>10s} {'share':>7s}"]
    rows.sort(key=lambda r: (not short(r[0]).startswith("bglat_"), -r[2]))
    for name, calls, ns in rows[:14]:
        name = short(name)
        name = name if len(name) <= 60 else name[:57] + "..."
        out.append(f"  {name:60s} {calls:7d} {ns / 1e6:10.3f} {ns / calls / 1e3:10.1f} {100 * ns / total:6.1f}%")
    return out


def profile(n_utts):
    """the kernel split: this tool's --child in a fresh process under the profiler"""
    if not shutil.which("rocprofv3"):
        return ["", "kernel split: not measured (no rocprofv3)"]
    d = tempfile.mkdtemp()
    cmd = ["rocprofv3", "--kernel-trace", "--stats", "-d", d, "-o", "bglat", "--output-format", "csv", "--", sys.executable,
           os.path.abspath(__file__), "--child", "--utts", str(n_utts)]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=900)
    found = glob.glob(os.path.join(d, "**", "*kernel_stats.csv"), recursive=True)
    if r.returncode != 0 or not found:
        return ["", f"kernel split: not measured (rocprofv3 exit {r.returncode})"]
    return kernel_table(found[0])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "bigram_lattice.txt"))
    ap.add_argument("--reps", type=int, default=2)
    ap.add_argument("--utts", type=int, default=1000)
    ap.add_argument("--beam", type=float, default=20.0)
    ap.add_argument("--no-profile", action="store_true")
    ap.add_argument("--child", action="store_true")
    a = ap.parse_args()
    if a.child:
        measure(1, a.utts, a.beam, True)
        return
    lines = measure(a.reps, a.utts, a.beam, False)
    print("\n".join(lines), flush=True)
    if not a.no_profile:
        lines += profile(a.utts)
    with open(a.out, "w") as f:
        f.write("Word lattices for the bigram search (tools/bigram_lattice_time.py), MI355X\n" + "\n".join(lines) + "\n")
    print("\n".join(lines[-16:]), flush=True)


if __name__ == "__main__":
    main()
