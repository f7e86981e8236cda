"""Wall time of word lattices (sr_word_lattice_corpus) against plain recognition (sr_recognize_corpus) and the word posteriors
(sr_word_posteriors_corpus) in the same run, at BASELINE configs[2]'s shape -- 4000 states x 32 densities (dim 39), silence + 1333
three-state words -- and configs[4]'s lexicon shape -- 8000 states x 64 densities, silence + 2666 three-state words (the last with
two more): 1000 utterances of 200..400 frames each, features resident, SR_GMM_PREFILTER, word penalty 10.

At beam +inf nearly every (word, frame) is an arc (40 bytes each: 12 and 32 GB at these shapes), so that beam is timed as the
sizing call, which runs every kernel but writes no arc; the finite beam is timed as Corpus.word_lattice does it (the sizing call,
then the filling call, arcs copied to the host).  The lattice kernels alone are the profiler's search window (sr_profile_read's
search_ms) during one sizing call.  Writes profiles/word_lattice.txt (or --out).

  python tools/word_lattice_time.py [--out PATH] [--reps N] [--shapes configs2,configs4] [--beam B]"""
import argparse
import ctypes as C
import os
import sys
import tempfile
import time

import numpy as np

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


def measure(shape, reps, beam):
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
        sp = capi.SearchParams(np.inf, 10.0, capi.GMM_PREFILTER, 0)
        aoff, best = np.zeros(c.n_utts + 1, np.uint64), np.zeros(c.n_utts)

        def sizing(b):
            capi._check(capi.lib().sr_word_lattice_corpus(m.h, c.h, L.h, C.byref(sp), float(b), 0, capi._ptr(aoff), capi._ptr(best),
                                                          None, None, None, None, None, None))
            return int(aoff[-1])

        _, t_rec = timed(lambda: c.recognize(L, 200.0, 10.0, capi.GMM_PREFILTER), reps)
        _, t_post = timed(lambda: c.word_posteriors(L, 10.0, 0.1, capi.GMM_PREFILTER, 0.0, 1), reps)
        n_inf, t_inf = timed(lambda: sizing(np.inf), reps)
        n_beam, t_size = timed(lambda: sizing(beam), reps)
        r, t_full = timed(lambda: c.word_lattice(L, 10.0, beam, capi.GMM_PREFILTER), reps)
        assert len(r[2]) == n_beam
        win = {}
        for name, f in (("post", lambda: c.word_posteriors(L, 10.0, 0.1, capi.GMM_PREFILTER, 0.0, 1)), ("lat", lambda: sizing(np.inf))):
            ms = []
            for _ in range(reps):
                m.profile(True)
                f()
                ms.append(m.profile_read()["search_ms"])
                m.profile(False)
            win[name] = sum(ms) / len(ms)
        c.close()
        L.close()
    F = int(off[-1])
    return [f"{shape}: {len(automaton)} positions, {lex.n_words} words, {lex.n_states} states x {mix} densities, 1000 utterances, "
            f"{F} frames; mean of {reps} calls after one warm-up",
            f"  sr_recognize_corpus                               {t_rec * 1e3:9.2f} ms",
            f"  sr_word_posteriors_corpus (1 item / frame)        {t_post * 1e3:9.2f} ms",
            f"    of which forward-backward kernels               {win['post']:9.2f} ms (profiler search window)",
            f"  sr_word_lattice_corpus, beam +inf, sizing call    {t_inf * 1e3:9.2f} ms ({n_inf} arcs counted, none written)",
            f"    of which lattice kernels                        {win['lat']:9.2f} ms (profiler search window)",
            f"  sr_word_lattice_corpus, beam {beam:g}, sizing call     {t_size * 1e3:9.2f} ms ({n_beam} arcs)",
            f"  sizing + filling call, beam {beam:g}, arcs on the host {t_full * 1e3:9.2f} ms"]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "word_lattice.txt"))
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--shapes", default="configs2,configs4")
    ap.add_argument("--beam", type=float, default=50.0)
    ap.add_argument("--no-write", action="store_true")
    a = ap.parse_args()
    lines = []
    for s in a.shapes.split(","):
        lines += measure(s, a.reps, a.beam)
        print("\n".join(lines[-8:]), flush=True)
    if not a.no_write:
        with open(a.out, "w") as f:
            f.write("Word lattices against plain recognition and the word posteriors (tools/word_lattice_time.py)\n" + "\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
