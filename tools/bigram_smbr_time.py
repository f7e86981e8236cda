"""Wall time of the sMBR accuracy pass over the bigram search network (sr_bigram_accuracies_corpus, one item per frame) and of one
sMBR E-step (sr_bigram_smbr_statistics_corpus), beside the free occupancy pass (sr_bigram_occupancies_corpus) and one MMI E-step
(sr_bigram_mmi_statistics_corpus) in the same run, on tools/bigram_mmi_time.py's shape: BASELINE configs[4]'s bigram lexicon, 1000
utterances of 40..120 frames, kappa = 0.1, posterior floor 1e-4, arg-min memberships, features resident.  The reference mixtures
are random states (an alignment would do as well: the pass' work does not depend on them).  Writes profiles/bigram_smbr.txt (or
--out).

  python tools/bigram_smbr_time.py [--out PATH] [--reps N] [--utts N]"""
import argparse
import os
import sys

import numpy as np

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from bigram_mmi_time import FLOOR, setup, timed  # noqa: E402


def measure(reps, n_utts):
    from speechrecognition_amd import capi
    lex, mp, feats, off, lm, trans, tdp, kappa = setup(n_utts)
    word_off, aut, _ = lex.flatten()
    F, W = int(off[-1]), lex.n_words
    ref = np.random.default_rng(5).integers(0, lex.n_states, size=F).astype(np.uint16)
    with capi.Model.from_mixset(mp, 39) as m:
        bg = m.bigram(word_off, aut, lex.silence_idx, lm, tdp)
        c = m.upload(feats, off)
        _, t_free = timed(lambda: c.bigram_occupancies(bg, kappa, None, capi.GMM_PREFILTER, FLOOR, 1), reps)
        (cost, acc, count, _, _), t_acc = timed(lambda: c.bigram_accuracies(bg, ref, kappa, capi.GMM_PREFILTER, FLOOR, 1), reps)
        (_, _, num, den), t_smbr = timed(lambda: c.bigram_smbr_statistics(bg, ref, kappa, capi.GMM_PREFILTER, FLOOR, True), reps)
        _, t_mmi = timed(lambda: c.bigram_mmi_statistics(bg, trans, kappa, capi.GMM_PREFILTER, FLOOR, True), reps)
        c.close()
        bg.close()
    rest = t_smbr - t_acc
    return [f"configs[4] bigram shape: {n_utts} utterances of 40..120 frames, {F} frames, {lex.n_states} states x 64 densities (dim 39), {W} words, "
            f"{int(word_off[-1]) + W} positions (words and silence copies), random reference mixtures, kappa = {kappa}, floor {FLOOR}; "
            f"mean of {reps} call(s) after one warm-up, features resident, SRGPU_FB_MB default",
            f"  sr_bigram_occupancies_corpus (free, 1 item / frame)       {t_free * 1e3:10.1f} ms",
            f"  sr_bigram_accuracies_corpus (1 item / frame)              {t_acc * 1e3:10.1f} ms   = {t_acc / t_free:.2f} x the free occupancy pass",
            f"  sr_bigram_smbr_statistics_corpus                          {t_smbr * 1e3:10.1f} ms",
            f"    items of both signs and accumulation (the remainder)    {rest * 1e3:10.1f} ms   = {100 * rest / t_smbr:.0f} % of the call",
            f"  sr_bigram_mmi_statistics_corpus (transcripts of 3..8)     {t_mmi * 1e3:10.1f} ms",
            f"  utterances with a complete path: {int(np.isfinite(cost).sum())} of {n_utts}; sum Abar = {acc.sum():.1f} of {F} frames; "
            f"frames with an item: {int((count > 0).sum())}",
            f"  |gamma| mass kept: numerator {num[1].sum():.1f}, denominator {den[1].sum():.1f}"]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "bigram_smbr.txt"))
    ap.add_argument("--reps", type=int, default=1)
    ap.add_argument("--utts", type=int, default=1000)
    ap.add_argument("--no-write", action="store_true")
    a = ap.parse_args()
    lines = measure(a.reps, a.utts)
    print("\n".join(lines), flush=True)
    if not a.no_write:
        with open(a.out, "w") as f:
            f.write("The sMBR accuracy pass over the bigram search network beside the free occupancy pass and one MMI E-step "
                    "(tools/bigram_smbr_time.py), MI355X\n" + "\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
