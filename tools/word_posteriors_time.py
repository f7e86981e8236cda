"""Wall time of word posteriors and confidences (sr_word_posteriors_corpus, sr_recognize_confidence_corpus) against plain
recognition (sr_recognize_corpus) at BASELINE configs[2]'s shape -- 4000 states x 32 densities (dim 39), silence + 1333 three-state
words -- and configs[4]'s lexicon shape -- 8000 states x 64 densities, silence + 2666 three-state words (the last with two more):
1000 utterances of 200..400 frames each, features resident, SR_GMM_PREFILTER, beam 200, word penalty 10, kappa 0.1.  The
forward-backward alone is the search window of the profiler (sr_profile_read's search_ms) during sr_word_posteriors_corpus with
one item per frame.  Writes profiles/word_posteriors.txt (or --out).

  python tools/word_posteriors_time.py [--out PATH] [--reps N] [--shapes configs2,configs4]"""
import argparse
import os
import sys
import tempfile
import time

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
sys.path.insert(0, ROOT)

TDP = (3.0, 0.0, 30.0)
SHAPES = {"configs2": (1333, 0, 32), "configs4": (2666, 2, 64)}


def timed(f, reps):
    f()
    t0 = time.perf_counter()
    for _ in range(reps):
        r = f()
    return r, (time.perf_counter() - t0) / reps


def measure(shape, reps):
    from speechrecognition_amd import capi, synth
    n_words, extra, mix = SHAPES[shape]
    lex = synth.make_lexicon(n_words, 3, 1, extra_states_last=extra)
    spec = synth.make_mixset(lex.n_states, mix, 39, seed=23)
    mp = os.path.join(tempfile.mkdtemp(), "m.mix")
    synth.write_mixset(mp, spec)
    feats, off = synth.make_batch(1000, 200, 400, 39, seed=7)
    word_off, automaton, sil_state = lex.flatten()
    with capi.Model.from_mixset(mp, 39) as m:
        L = capi.Lexicon(m, word_off, automaton, lex.silence_idx, TDP, sil_state)
        c = m.upload(feats, off)
        _, t_rec = timed(lambda: c.recognize(L, 200.0, 10.0, capi.GMM_PREFILTER), reps)
        _, t_conf = timed(lambda: c.recognize_confidence(L, 200.0, 10.0, 0.1, capi.GMM_PREFILTER), reps)
        _, t_post = timed(lambda: c.word_posteriors(L, 10.0, 0.1, capi.GMM_PREFILTER, 0.0, 1), reps)
        fb = []
        for _ in range(reps):
            m.profile(True)
            c.word_posteriors(L, 10.0, 0.1, capi.GMM_PREFILTER, 0.0, 1)
            fb.append(m.profile_read()["search_ms"])
            m.profile(False)
        c.close()
        L.close()
    F = int(off[-1])
    return [f"{shape}: {len(automaton)} positions, {lex.n_words} words, {lex.n_states} states x {mix} densities, 1000 utterances, "
            f"{F} frames; mean of {reps} calls after one warm-up",
            f"  sr_recognize_corpus                        {t_rec * 1e3:9.2f} ms",
            f"  sr_recognize_confidence_corpus             {t_conf * 1e3:9.2f} ms",
            f"  sr_word_posteriors_corpus (1 item / frame) {t_post * 1e3:9.2f} ms",
            f"    of which forward-backward kernels        {sum(fb) / len(fb):9.2f} ms (profiler search window)"]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "word_posteriors.txt"))
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--shapes", default="configs2,configs4")
    ap.add_argument("--no-write", action="store_true")
    a = ap.parse_args()
    lines = []
    for s in a.shapes.split(","):
        lines += measure(s, a.reps)
        print("\n".join(lines[-5:]), flush=True)
    if not a.no_write:
        with open(a.out, "w") as f:
            f.write("Word posteriors and confidences against plain recognition (tools/word_posteriors_time.py)\n" + "\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
