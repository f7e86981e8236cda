"""Wall time of one Baum-Welch E-step (sr_baum_welch_corpus) against the Viterbi-training pair it replaces (sr_align_corpus +
sr_accumulate_corpus) on BASELINE configs[2]'s shape: 4000 states x 32 densities, 1000 utterances of 200..400 frames, automata
`sil w1 sil w2 sil w3 sil` from seeded transcripts, features resident, arg-min memberships on both sides.  Writes
profiles/baum_welch.txt (or --out).

  python tools/baum_welch_time.py [--out PATH] [--reps N]
  rocprofv3 --kernel-trace --stats -d DIR -o bw -- python tools/baum_welch_time.py --reps 1 --no-write
  python tools/baum_welch_time.py --append-stats DIR/.../bw_results.db (or bw_kernel_stats.csv) [--out PATH]
                                                                                      (no GPU: adds the kernel table)"""
import argparse
import csv
import os
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
sys.path.insert(0, ROOT)

TDP = (3.0, 0.0, 30.0)
FB_KERNELS = ("fb_", "items_", "em_item_pairs", "em_assign_weighted", "em_iota")


def setup():
    from speechrecognition_amd import synth
    lex = synth.make_lexicon(1333, 3, 1)
    spec = synth.make_mixset(lex.n_states, 32, 39, seed=23)
    mp = os.path.join(tempfile.mkdtemp(), "m.mix")
    synth.write_mixset(mp, spec)
    feats, off = synth.make_batch(1000, 200, 400, 39, seed=7)
    word_off, automaton, sil = lex.flatten()
    rng = np.random.default_rng(5)
    auts = []
    for _ in range(1000):
        a = [sil]
        for w in rng.integers(1, lex.n_words, size=3):
            a += list(automaton[word_off[w]:word_off[w + 1]]) + [sil]
        auts.append(np.asarray(a, np.uint16))
    return mp, feats, off, auts, sil


def timed(f, reps):
    f()
    t0 = time.perf_counter()
    for _ in range(reps):
        r = f()
    return r, (time.perf_counter() - t0) / reps


def measure(reps):
    from speechrecognition_amd import capi
    mp, feats, off, auts, sil = setup()
    F = int(off[-1])
    positions = sum(len(a) * int(off[u + 1] - off[u]) for u, a in enumerate(auts))
    lines = []
    with capi.Model.from_mixset(mp, 39) as m:
        c = m.upload(feats, off)
        (states, _), t_align = timed(lambda: c.align(auts, TDP, sil, capi.GMM_DEFAULT), reps)
        _, t_acc = timed(lambda: c.accumulate(states, False, True), reps)
        for floor in (0.0, 1e-4):
            (cost, stats), t_bw = timed(lambda: c.baum_welch(auts, TDP, sil, capi.GMM_DEFAULT, floor, False, True), reps)
            _, t_post = timed(lambda: c.state_posteriors(auts, TDP, sil, capi.GMM_DEFAULT, floor, 8), reps)
            lines.append(f"  floor {floor:g}: sr_baum_welch_corpus {t_bw * 1e3:8.2f} ms   sr_state_posteriors_corpus (8 items) {t_post * 1e3:8.2f} ms"
                         f"   sum mean_w {stats[1].sum():.6f}")
        c.close()
    head = [f"configs[2] shape: 1000 utterances, {F} frames, 4000 states x 32 densities (dim 39), automata of 13 positions, "
            f"{positions} (frame, position) cells = {8 * positions / 2**20:.1f} MiB of trellis; mean of {reps} calls after one warm-up, "
            "features resident, listed exact scoring (SR_GMM_DEFAULT), arg-min memberships",
            f"  Viterbi training: sr_align_corpus {t_align * 1e3:8.2f} ms + sr_accumulate_corpus {t_acc * 1e3:8.2f} ms = "
            f"{(t_align + t_acc) * 1e3:8.2f} ms"]
    return head + lines


def _stats_rows(path):
    """(name, calls, total ns) per kernel from rocprofv3's SQLite output (top_kernels, microseconds) or its --stats CSV"""
    if path.endswith(".db"):
        import sqlite3
        db = sqlite3.connect(path)
        return [(n, int(c), 1e3 * float(t)) for n, c, t in db.execute("select name, total_calls, total_duration from top_kernels")]
    return [(r["Name"], int(r["Calls"]), float(r["TotalDurationNs"])) for r in csv.DictReader(open(path))]


def kernel_table(path):
    rows = _stats_rows(path)
    total = sum(r[2] for r in rows)
    short = lambda n: n.replace("void ", "").replace("srgpu::", "").split("(")[0]  # noqa: E731
    out = ["", f"rocprofv3 --kernel-trace --stats ({os.path.basename(path)}), one run of this tool with --reps 1 (every entry point called "
           "twice per floor); the forward-backward's own kernels first, then the rest by time:",
           f"  {'kernel':60s} {'calls':>6s} {'total ms':>10s} {'avg us':>10s} {'share':>7s}"]
    rows.sort(key=lambda r: (not short(r[0]).startswith(FB_KERNELS), -r[2]))
    for name, calls, ns in rows[:24]:
        name = short(name)
        name = name if len(name) <= 60 else name[:57] + "..."
        out.append(f"  {name:60s} {calls:6d} {ns / 1e6:10.3f} {ns / calls / 1e3:10.1f} {100 * ns / total:6.1f}%")
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "baum_welch.txt"))
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--no-write", action="store_true")
    ap.add_argument("--append-stats")
    a = ap.parse_args()
    if a.append_stats:
        with open(a.out, "a") as f:
            f.write("\n".join(kernel_table(a.append_stats)) + "\n")
        return
    lines = measure(a.reps)
    print("\n".join(lines))
    if not a.no_write:
        with open(a.out, "w") as f:
            f.write("Baum-Welch E-step against Viterbi training (tools/baum_welch_time.py)\n" + "\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
