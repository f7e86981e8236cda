"""Wall time of the bigram search's posterior call (sr_bigram_word_posteriors_corpus) beside the zerogram one
(sr_word_posteriors_corpus) and the bigram search itself on BASELINE configs[4]'s shape: 8000 states x 64 densities, 2666 words +
silence, a Dirichlet bigram as bench.py draws it, 1000 utterances of 200..400 frames (302 685 frames), kappa = 0.1, features
resident.  Writes profiles/bigram_posteriors.txt (or --out); the kernel split comes from a second run under the profiler.

  python tools/bigram_posteriors_time.py [--out PATH] [--reps N] [--utts N]
  rocprofv3 --kernel-trace --stats -d DIR -o bg --output-format csv -- python tools/bigram_posteriors_time.py --reps 1 --no-write --only-bigram
  python tools/bigram_posteriors_time.py --append-stats DIR/.../bg_kernel_stats.csv [--out PATH]     (no GPU: adds the kernel table)"""
import argparse
import csv
import os
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
sys.path.insert(0, ROOT)

KAPPA = 0.1
BG_TDP = np.array([[3.0, 0.0, 3.0, 150.0], [0.0001, 3.0, np.inf, 15.0]], np.float32)  # bench.py's


def setup(n_utts):
    from speechrecognition_amd import synth
    lex = synth.make_lexicon(2666, 3, 1, extra_states_last=2)
    spec = synth.make_mixset(lex.n_states, 64, 39, seed=23)
    mp = os.path.join(tempfile.mkdtemp(), "m.mix")
    synth.write_mixset(mp, spec)
    feats, off = synth.make_batch(n_utts, 200, 400, 39, seed=7)
    rng = np.random.default_rng(99)
    nW = lex.n_words
    lm = np.empty((nW, nW), np.float32)
    for h0 in range(0, nW, 256):
        p = rng.dirichlet(np.ones(nW), size=min(256, nW - h0))
        lm[:, h0:h0 + p.shape[0]] = (-np.log(np.maximum(p, 1e-30))).T
    return lex, mp, feats, off, lm


def timed(f, reps):
    f()
    t0 = time.perf_counter()
    for _ in range(reps):
        r = f()
    return r, (time.perf_counter() - t0) / reps


def measure(reps, n_utts, only_bigram):
    from speechrecognition_amd import capi
    lex, mp, feats, off, lm = setup(n_utts)
    word_off, aut, sil_state = lex.flatten()
    F, W = int(off[-1]), lex.n_words
    lines = []
    with capi.Model.from_mixset(mp, 39) as m:
        bg = m.bigram(word_off, aut, lex.silence_idx, lm, BG_TDP)
        c = m.upload(feats, off)
        (cost, *_), t_bg = timed(lambda: c.bigram_word_posteriors(bg, KAPPA, capi.GMM_PREFILTER, 1e-4, 4), reps)
        lines.append(f"  sr_bigram_word_posteriors_corpus (4 items, floor 1e-4)   {t_bg * 1e3:10.1f} ms   finite F: {int(np.isfinite(cost).sum())} of {len(cost)}")
        if not only_bigram:
            _, t_rec = timed(lambda: c.recognize_bigram(bg, 200.0, capi.FLT_MAX), reps)
            _, t_conf = timed(lambda: c.recognize_bigram_confidence(bg, KAPPA, 200.0, capi.FLT_MAX), reps)
            L = m.lexicon(word_off, aut, lex.silence_idx, (3.0, 0.0, 30.0), sil_state)
            _, t_zero = timed(lambda: c.word_posteriors(L, 10.0, KAPPA, capi.GMM_PREFILTER, 1e-4, 4), reps)
            L.close()
            lines += [f"  sr_recognize_bigram_corpus (beam 200)                    {t_rec * 1e3:10.1f} ms",
                      f"  sr_recognize_bigram_confidence_corpus (beam 200)         {t_conf * 1e3:10.1f} ms",
                      f"  sr_word_posteriors_corpus (zerogram network, same run)   {t_zero * 1e3:10.1f} ms"]
        c.close()
        bg.close()
    flops = 2.0 * W * W * F * 2
    head = [f"configs[4] shape: {n_utts} utterances, {F} frames, {lex.n_states} states x 64 densities (dim 39), {W} words, "
            f"{int(word_off[-1]) + W} positions (words and silence copies), kappa = {KAPPA}; mean of {reps} calls after one warm-up "
            "(the warm-up builds exp(-kappa lm)), features resident, SRGPU_FB_MB default",
            f"  entry product: 2 W^2 flop per (frame, utterance) and direction = {flops:.4g} flop per call"]
    return head + lines


def kernel_table(path):
    rows = [(r["Name"], int(r["Calls"]), float(r["TotalDurationNs"])) for r in csv.DictReader(open(path))]
    total = sum(r[2] for r in rows)
    short = lambda n: n.replace("void ", "").replace("srgpu::", "").split("(")[0]  # noqa: E731
    out = ["", f"rocprofv3 --kernel-trace --stats ({os.path.basename(path)}), one run of this tool with --reps 1 --only-bigram (the call twice: "
           "warm-up and timed); the forward-backward's own kernels first, then the rest by time:",
           f"  {'kernel':60s} {'calls':>7s} {'total ms':>10s} {'avg us':>10s} {'share':>7s}"]
    rows.sort(key=lambda r: (not short(r[0]).startswith(("bgfb_", "netfb_top")), -r[2]))
    for name, calls, ns in rows[:14]:
        name = short(name)
        name = name if len(name) <= 60 else name[:57] + "..."
        out.append(f"  {name:60s} {calls:7d} {ns / 1e6:10.3f} {ns / calls / 1e3:10.1f} {100 * ns / total:6.1f}%")
    prod = [r for r in rows if "bgfb_product" in r[0]]
    if prod:  # (the default corpus: 2667 words, 302 685 frames, both directions, two calls)
        flop = 2.0 * 2667 ** 2 * 302685 * 2 * 2
        out.append(f"  product: {flop:.4g} flop in {prod[0][2] / 1e6:.1f} ms = {flop / prod[0][2] / 1e3:.2f} TFLOP/s FP64 (matrix peak 78.6)")
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "bigram_posteriors.txt"))
    ap.add_argument("--reps", type=int, default=2)
    ap.add_argument("--utts", type=int, default=1000)
    ap.add_argument("--no-write", action="store_true")
    ap.add_argument("--only-bigram", action="store_true")
    ap.add_argument("--append-stats")
    a = ap.parse_args()
    if a.append_stats:
        with open(a.out, "a") as f:
            f.write("\n".join(kernel_table(a.append_stats)) + "\n")
        return
    lines = measure(a.reps, a.utts, a.only_bigram)
    print("\n".join(lines), flush=True)
    if not a.no_write:
        with open(a.out, "w") as f:
            f.write("Posteriors for the bigram search (tools/bigram_posteriors_time.py), MI355X\n" + "\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
