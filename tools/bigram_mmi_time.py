"""Wall time of one MMI E-step against the bigram search network (sr_bigram_mmi_statistics_corpus) split into its passes, beside the
bigram posterior call (sr_bigram_word_posteriors_corpus) in the same run, on BASELINE configs[4]'s bigram shape: 8000 states x 64
densities (dim 39), 2666 words + silence, a Dirichlet bigram as bench.py draws it, 1000 utterances, kappa = 0.1, posterior floor
1e-4, arg-min memberships, features resident.  The utterances are 40..120 frames long, not bench.py's 200..400: the item buffers are
reserved for every (frame, distinct mixture) pair and the call refuses 2^31 of them (302 685 frames x 8001 mixtures = 2.4e9).  The
constrained and the free pass are sr_bigram_occupancies_corpus with one item per frame; the accumulation is the remainder of
sr_bigram_mmi_statistics_corpus.  The denominator's items are counted through a free call with 512 items per frame.  Writes
profiles/bigram_mmi.txt (or --out).

  python tools/bigram_mmi_time.py [--out PATH] [--reps N] [--utts N]"""
import argparse
import os
import sys
import time

import numpy as np

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

FLOOR = 1e-4
COUNT_K = 512


def timed(f, reps):
    f()
    t0 = time.perf_counter()
    for _ in range(reps):
        r = f()
    return r, (time.perf_counter() - t0) / reps


def setup(n_utts):
    import tempfile

    from bigram_posteriors_time import BG_TDP, KAPPA
    from speechrecognition_amd import synth
    lex = synth.make_lexicon(2666, 3, 1, extra_states_last=2)
    spec = synth.make_mixset(lex.n_states, 64, 39, seed=23)
    mp = os.path.join(tempfile.mkdtemp(), "m.mix")
    synth.write_mixset(mp, spec)
    feats, off = synth.make_batch(n_utts, 40, 120, 39, seed=7)
    rng = np.random.default_rng(99)
    nW = lex.n_words
    lm = np.empty((nW, nW), np.float32)
    for h0 in range(0, nW, 256):
        p = rng.dirichlet(np.ones(nW), size=min(256, nW - h0))
        lm[:, h0:h0 + p.shape[0]] = (-np.log(np.maximum(p, 1e-30))).T
    trans = [[int(w) for w in rng.integers(1, nW, size=int(rng.integers(3, 9)))] for _ in range(n_utts)]
    return lex, mp, feats, np.asarray(off, np.uint64), lm, trans, BG_TDP, KAPPA


def measure(reps, n_utts):
    from speechrecognition_amd import capi
    lex, mp, feats, off, lm, trans, tdp, kappa = setup(n_utts)
    word_off, aut, _ = lex.flatten()
    F, W = int(off[-1]), lex.n_words
    with capi.Model.from_mixset(mp, 39) as m:
        bg = m.bigram(word_off, aut, lex.silence_idx, lm, tdp)
        c = m.upload(feats, off)
        _, t_post = timed(lambda: c.bigram_word_posteriors(bg, kappa, capi.GMM_PREFILTER, FLOOR, 4), reps)
        _, t_free = timed(lambda: c.bigram_occupancies(bg, kappa, None, capi.GMM_PREFILTER, FLOOR, 1), reps)
        _, t_chain = timed(lambda: c.bigram_occupancies(bg, kappa, trans, capi.GMM_PREFILTER, FLOOR, 1), reps)
        (fn, fd, num, den), t_mmi = timed(lambda: c.bigram_mmi_statistics(bg, trans, kappa, capi.GMM_PREFILTER, FLOOR, True), reps)
        count = c.bigram_occupancies(bg, kappa, None, capi.GMM_PREFILTER, FLOOR, COUNT_K)[1]
        ncount = c.bigram_occupancies(bg, kappa, trans, capi.GMM_PREFILTER, FLOOR, COUNT_K)[1]
        c.close()
        bg.close()
    ok = np.isfinite(fn)
    live = np.repeat(ok, np.diff(off).astype(np.int64))  # frames of the utterances that contribute
    acc = t_mmi - t_free - t_chain
    capped = " (at least: some frame holds 512 or more)" if count.max() >= COUNT_K else ""
    return [f"configs[4] bigram shape: {n_utts} utterances of 40..120 frames, {F} frames, {lex.n_states} states x 64 densities (dim 39), {W} words, "
            f"{int(word_off[-1]) + W} positions (words and silence copies), transcripts of 3..8 words, kappa = {kappa}, floor {FLOOR}; "
            f"mean of {reps} call(s) after one warm-up, features resident, SRGPU_FB_MB default",
            f"  sr_bigram_word_posteriors_corpus (4 items / frame)   {t_post * 1e3:10.1f} ms",
            f"  sr_bigram_mmi_statistics_corpus                      {t_mmi * 1e3:10.1f} ms",
            f"    free pass (sr_bigram_occupancies_corpus, 1 item)   {t_free * 1e3:10.1f} ms   = {t_free / t_post:.2f} x the posterior call",
            f"    constrained pass (the same, transcripts)           {t_chain * 1e3:10.1f} ms",
            f"    accumulation, both sides (the remainder)           {acc * 1e3:10.1f} ms   = {100 * acc / t_mmi:.0f} % of the call",
            f"  utterances with a path through their transcript: {int(ok.sum())} of {n_utts} ({int(live.sum())} frames)",
            f"  denominator items: {int(count[live].sum())}{capped} = {count[live].mean():.1f} per frame; numerator items: {int(ncount[live].sum())} = "
            f"{ncount[live].mean():.2f} per frame",
            f"  occupancy mass kept: numerator {num[1].sum():.0f}, denominator {den[1].sum():.0f} of {int(live.sum())} frames; "
            f"sum(F_num - F_den) = {(fn - fd)[ok].sum():.1f}"]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "bigram_mmi.txt"))
    ap.add_argument("--reps", type=int, default=1)
    ap.add_argument("--utts", type=int, default=1000)
    ap.add_argument("--no-write", action="store_true")
    a = ap.parse_args()
    lines = measure(a.reps, a.utts)
    print("\n".join(lines), flush=True)
    if not a.no_write:
        with open(a.out, "w") as f:
            f.write("One MMI E-step against the bigram search network beside its posterior call (tools/bigram_mmi_time.py), MI355X\n" + "\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
