"""Wall time of one MMI E-step (sr_mmi_statistics_corpus) split into its passes, beside the word-posterior pass
(sr_word_posteriors_corpus) and the Baum-Welch E-step (sr_baum_welch_corpus) on the same inputs: BASELINE configs[2]'s shape -- 4000
states x 32 densities (dim 39), silence + 1333 three-state words -- and the reference's own lexicon shape -- silence + 11 words of 9
or 12 states, each repeated twice, 3 densities (dim 25); 1000 utterances of 200..400 frames sampled along 3..8 random words, features
resident, SR_GMM_PREFILTER, word penalty 10, kappa 0.1, posterior floor 1e-4, arg-min memberships.  The free and the constrained pass
are sr_net_occupancies_corpus with one item per frame; the accumulation is the remainder of sr_mmi_statistics_corpus.  Writes
profiles/mmi.txt (or --out).

  python tools/mmi_time.py [--out PATH] [--reps N] [--shapes configs2,sietill]"""
import argparse
import os
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
sys.path.insert(0, ROOT)

TDP = (3.0, 0.0, 30.0)
FLOOR = 1e-4


def timed(f, reps):
    f()
    t0 = time.perf_counter()
    for _ in range(reps):
        r = f()
    return r, (time.perf_counter() - t0) / reps


def make_case(shape):
    from speechrecognition_amd import synth
    if shape == "configs2":
        lex, mix, dim = synth.make_lexicon(1333, 3, 1), 32, 39
    else:
        lex = synth.LexiconSpec(np.array([1, 9, 9, 9, 9, 12, 9, 12, 9, 9, 9, 9], np.uint16), np.array([1] + [2] * 11, np.uint16), 0)
        mix, dim = 3, 25
    spec = synth.make_mixset(lex.n_states, mix, dim, seed=23)
    rng = np.random.default_rng(29)
    feats, off = synth.make_batch(1000, 200, 400, dim, seed=7)
    trans = [[int(w) for w in rng.integers(1, lex.n_words, size=int(rng.integers(3, 9)))] for _ in range(1000)]
    return lex, spec, mix, dim, feats, off, trans


def measure(shape, reps):
    from speechrecognition_amd import capi, synth
    lex, spec, mix, dim, feats, off, trans = make_case(shape)
    mp = os.path.join(tempfile.mkdtemp(), "m.mix")
    synth.write_mixset(mp, spec)
    word_off, automaton, sil_state = lex.flatten()
    auts = []
    for tr in trans:
        a = [sil_state]
        for w in tr:
            a += list(automaton[word_off[w]:word_off[w + 1]]) + [sil_state]
        auts.append(np.asarray(a, np.uint16))
    with capi.Model.from_mixset(mp, dim) as m:
        L = capi.Lexicon(m, word_off, automaton, lex.silence_idx, TDP, sil_state)
        c = m.upload(feats, off)
        _, t_post = timed(lambda: c.word_posteriors(L, 10.0, 0.1, capi.GMM_PREFILTER, FLOOR, 1), reps)
        _, t_bw = timed(lambda: c.baum_welch(auts, TDP, sil_state, capi.GMM_PREFILTER, FLOOR, False, True), reps)
        _, t_free = timed(lambda: c.net_occupancies(L, 10.0, 0.1, None, capi.GMM_PREFILTER, FLOOR, 1), reps)
        _, t_chain = timed(lambda: c.net_occupancies(L, 10.0, 0.1, trans, capi.GMM_PREFILTER, FLOOR, 1), reps)
        (fn, fd, num, den), t_mmi = timed(lambda: c.mmi_statistics(L, 10.0, trans, 0.1, capi.GMM_PREFILTER, FLOOR, True), reps)
        c.close()
        L.close()
    chain = sum(len(a) for a in auts) / len(auts)
    return [f"{shape}: {len(automaton)} positions, {lex.n_words} words, {lex.n_states} states x {mix} densities, 1000 utterances, "
            f"{int(off[-1])} frames, chains of {chain:.0f} positions on average; mean of {reps} calls after one warm-up",
            f"  sr_word_posteriors_corpus (1 item / frame)   {t_post * 1e3:9.2f} ms",
            f"  sr_baum_welch_corpus (aligner's automata)    {t_bw * 1e3:9.2f} ms",
            f"  sr_mmi_statistics_corpus                     {t_mmi * 1e3:9.2f} ms",
            f"    free pass (sr_net_occupancies_corpus)      {t_free * 1e3:9.2f} ms",
            f"    constrained pass (the same, transcripts)   {t_chain * 1e3:9.2f} ms",
            f"    accumulation, both sides (the remainder)   {(t_mmi - t_free - t_chain) * 1e3:9.2f} ms",
            f"  occupancy mass kept: numerator {num[1].sum():.0f}, denominator {den[1].sum():.0f} of {int(off[-1])} frames; "
            f"sum(F_num - F_den) = {(fn - fd)[np.isfinite(fn)].sum():.1f}"]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "mmi.txt"))
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--shapes", default="configs2,sietill")
    ap.add_argument("--no-write", action="store_true")
    a = ap.parse_args()
    lines = []
    for s in a.shapes.split(","):
        lines += measure(s, a.reps)
        print("\n".join(lines[-8:]), flush=True)
    if not a.no_write:
        with open(a.out, "w") as f:
            f.write("One MMI E-step against the word-posterior pass and the Baum-Welch E-step (tools/mmi_time.py)\n" + "\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
