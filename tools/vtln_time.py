"""Time of the VTLN warp search (sr_vtln_costs_corpus) at the benchmark's frame count, beside the only way to do the same work without
it.  The shape is tools/frontend_time.py's: 1000 utterances of 200..400 frames (302 685 frames) of 16 kHz noise, window 400, shift 160,
FFT 512, 24 filters, 12 + 12 + 1 features with mean / deviation and energy normalisation; a model of 4000 states x 32 densities in 25
dimensions; 13 warps (0.88 .. 1.12, break 0.875), 50 speakers (utterance u belongs to speaker u mod 50), an alignment of the unwarped
corpus from sr_align_corpus_pruned against transcripts of ten random words.

  (default)    one sr_vtln_costs_corpus call: wall time, the device time of all its kernels (sr_profile_*), and the split into
               mfcc_warps_kernel, post-processing, scoring and reduction (the library's own HIP events, SRGPU_VTLN_TIMING, which this
               tool sets: a handful of event records per call ride along in the other two numbers)
  --baseline   only calls that exist without VTLN: 13 x (sr_corpus_from_audio + sr_path_scores_corpus + the sums on the host) on one
               unwarped front end -- the same amount of work, every pass repeating the transform.  Wall time of the whole and of its
               three parts, and the device time of the front end's kernels (sr_path_scores_corpus records none)
Run the two in one session, interleaved; one process each, one warm-up before each mean.

  python tools/vtln_time.py [--baseline] [--reps N] [--out PATH]"""
import argparse
import os
import re
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
sys.path.insert(0, ROOT)

ALPHAS = [round(0.88 + 0.02 * i, 2) for i in range(13)]
N_SPEAKERS = 50


def setup():
    from speechrecognition_amd import synth
    from tests import frontend_reference as R
    p = R.params()
    D, M = 25, 32
    _, off = synth.make_batch(1000, 200, 400, 1, seed=7)
    T = np.diff(off.astype(np.int64))
    rng = np.random.default_rng(11)
    lens = p["window"] + (T - 1) * p["shift"]
    soff = np.concatenate([[0], np.cumsum(lens)]).astype(np.uint64)
    samples = np.clip(np.rint(rng.normal(0.0, 1000.0, int(soff[-1]))), -32768, 32767).astype(np.int16)
    lex = synth.make_lexicon(1333, 3, 1)
    mp = os.path.join(tempfile.mkdtemp(), "m.mix")
    synth.write_mixset(mp, synth.make_mixset(lex.n_states, M, D, seed=23))
    word_off, automaton, sil = lex.flatten()
    auts = []
    for u in range(len(T)):
        aut = [sil]
        for w in rng.integers(1, 1333, size=10):
            aut += list(automaton[word_off[w]:word_off[w + 1]]) + [sil]
        auts.append(np.asarray(aut, dtype=np.uint16))
    return p, D, off, soff, samples, mp, auts, sil


def normalisation(m, p, post, samples, soff):
    with m.frontend(p, post) as plain:
        c = plain.from_audio(samples, soff)
        rows = c.download().astype(np.float64)
        c.close()
    return rows.mean(axis=0), rows.std(axis=0)


def alignment(fe, samples, soff, auts, sil):
    c = fe.from_audio(samples, soff)
    states, _ = c.align(auts, (3.0, 0.0, 30.0), sil, pruning_threshold=200.0)
    foff = c.frame_off.copy()
    c.close()
    return states, foff


def head(what, reps):
    from speechrecognition_amd import build
    info = build.build_info()
    return (f"{what}: commit {info.get('git_head', 'unknown')}{' + uncommitted changes' if info.get('dirty') else ''}; 1000 utterances, "
            f"302685 frames, 13 warps, {N_SPEAKERS} speakers; mean of {reps} calls after one warm-up")


def measure_new(reps):
    os.environ["SRGPU_VTLN_TIMING"] = "1"
    from speechrecognition_amd import capi
    p, D, off, soff, samples, mp, auts, sil = setup()
    post = dict(n_static=12, n_first=12, n_second=1, deriv_step=3, energy_max_norm=1)
    speaker = (np.arange(len(soff) - 1) % N_SPEAKERS).astype(np.uint32)
    with capi.Model.from_mixset(mp, D) as m:
        mean, stddev = normalisation(m, p, post, samples, soff)
        with m.frontend(p, dict(post, mean=mean, stddev=stddev), vtln=dict(alpha=ALPHAS, break_frac=0.875)) as fe:
            states, foff = alignment(fe, samples, soff, auts, sil)
            assert np.array_equal(foff, off.astype(np.uint64))
            cost, frames = fe.vtln_costs(samples, soff, states, speaker, N_SPEAKERS)   # warm-up
            # the library's stage times go to stderr: into a file while the timed calls run
            log = tempfile.TemporaryFile(mode="w+")
            sys.stderr.flush()
            keep = os.dup(2)
            os.dup2(log.fileno(), 2)
            try:
                m.profile(True)
                t0 = time.perf_counter()
                for _ in range(reps):
                    again, _ = fe.vtln_costs(samples, soff, states, speaker, N_SPEAKERS)
                wall = (time.perf_counter() - t0) / reps * 1e3
                dev = m.profile_read()["search_ms"] / reps
                m.profile(False)
            finally:
                os.dup2(keep, 2)
                os.close(keep)
            assert np.array_equal(again.view(np.uint64), cost.view(np.uint64))
            log.seek(0)
            rows = [[float(x) for x in re.findall(r"_ms ([0-9.]+)", ln)] + [int(re.search(r"chunks (\d+)", ln).group(1))]
                    for ln in log.read().splitlines() if ln.startswith("vtln_timing")]
            assert len(rows) == reps
            mfcc, postp, score, red, chunks = np.mean(np.array(rows), axis=0)
            chosen = capi.vtln_choose(cost, frames, 0, 6)
    return [head("sr_vtln_costs_corpus", reps),
            f"  one call, samples and alignment on the host   call {wall:8.2f} ms   kernels {dev:8.3f} ms   ({int(chunks)} chunk(s) of warps)",
            f"    mfcc_warps_kernel {mfcc:8.3f} ms   post-processing {postp:8.3f} ms   scoring {score:8.3f} ms   reduction {red:8.3f} ms",
            f"    MFCC stage per warp {mfcc / 13:6.3f} ms; costs {cost.min():.1f} .. {cost.max():.1f}; warps chosen (noise: no true warp): "
            f"{np.bincount(chosen, minlength=13).tolist()}"]


def measure_baseline(reps):
    from speechrecognition_amd import capi
    p, D, off, soff, samples, mp, auts, sil = setup()
    post = dict(n_static=12, n_first=12, n_second=1, deriv_step=3, energy_max_norm=1)
    speaker = (np.arange(len(soff) - 1) % N_SPEAKERS).astype(np.uint32)
    o = off.astype(np.int64)
    with capi.Model.from_mixset(mp, D) as m:
        mean, stddev = normalisation(m, p, post, samples, soff)
        with m.frontend(p, dict(post, mean=mean, stddev=stddev)) as fe:
            states, _ = alignment(fe, samples, soff, auts, sil)

            def one_pass(t):
                cost = np.zeros((N_SPEAKERS, 13))
                for a in range(13):
                    t0 = time.perf_counter()
                    c = fe.from_audio(samples, soff)
                    t1 = time.perf_counter()
                    sc = c.path_scores(states)
                    t2 = time.perf_counter()
                    utt = np.add.reduceat(sc, o[:-1])
                    for s in range(N_SPEAKERS):
                        cost[s, a] = utt[speaker == s].sum()
                    t3 = time.perf_counter()
                    c.close()
                    t[0] += t1 - t0
                    t[1] += t2 - t1
                    t[2] += t3 - t2
                return cost

            one_pass([0.0, 0.0, 0.0])   # warm-up
            t = [0.0, 0.0, 0.0]
            m.profile(True)
            t0 = time.perf_counter()
            for _ in range(reps):
                one_pass(t)
            wall = (time.perf_counter() - t0) / reps * 1e3
            dev = m.profile_read()["search_ms"] / reps
            m.profile(False)
    fa, ps, hs = (x / reps * 1e3 for x in t)
    return [head("baseline, 13 x (sr_corpus_from_audio + sr_path_scores_corpus + host sums)", reps),
            f"  13 passes                                      call {wall:8.2f} ms   front-end kernels {dev:8.3f} ms ({dev / 13:.3f} ms a pass)",
            f"    sr_corpus_from_audio {fa:8.2f} ms   sr_path_scores_corpus {ps:8.2f} ms (wall: states in, kernel, scores out)   host sums {hs:8.2f} ms"]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--baseline", action="store_true")
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    lines = measure_baseline(a.reps) if a.baseline else measure_new(a.reps)
    print("\n".join(lines))
    if a.out:
        with open(a.out, "a") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
