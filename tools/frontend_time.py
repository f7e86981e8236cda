"""Time and accuracy of the audio front end (sr_corpus_from_audio, sr_corpus_from_cepstra) at the benchmark's frame count: the 1000
utterances of 200..400 frames of bench.py (302 685 frames) as 16 kHz noise of exactly that many frames -- window 400, shift 160, FFT
512, 24 filters, 12 + 12 + 1 features with mean / deviation and energy normalisation -- beside what it replaces and what it feeds:
  from_audio      the whole call with the samples on the host (copy in, span list, both kernels, allocation of the corpus), and the
                  kernels alone (the library's event pairs, sr_profile_*: the same without the copy)
  from_cepstra    the same two numbers for the post-processing stage alone, cepstra on the host
  host            sr::FeaturePostProcessor::process_features over the same cepstra on one thread (tests/cpp/frontend_driver.cpp, mode
                  `time`) plus sr_corpus_upload of its rows: what from_cepstra replaces
  numpy           the rate of the float64 restatement tests/frontend_reference.py on a few utterances
  recognize       one sr_recognize_corpus step on the corpus from_audio returned: the benchmark's lexicon (1333 words, 4000 states) and
                  32 densities a state in 25 dimensions, beam 200, prefilter kernel
The expectation it checks: audio -> corpus costs less than the recognition step it feeds.  Also the device's largest
|cepstrum - float64 reference| on the test signals of tests/test_gpu_frontend.py (bound there: 2e-4).
One process, one warm-up call before each mean.  Writes profiles/frontend.txt (or --out).

  python tools/frontend_time.py [--out PATH] [--reps N] [--no-write]"""
import argparse
import os
import subprocess
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
sys.path.insert(0, ROOT)


def timed(m, f, reps):
    """-> (result of the last call, kernels' ms per call, wall ms per call) after one warm-up; the caller closes the results"""
    f().close()
    m.profile(True)
    t0 = time.perf_counter()
    for i in range(reps):
        r = f()
        if i + 1 < reps:
            r.close()
    wall = (time.perf_counter() - t0) / reps
    p = m.profile_read()
    m.profile(False)
    return r, p["search_ms"] / reps, wall * 1e3


def accuracy(capi, R):
    from tests.test_gpu_frontend import MFCC8, MFCC16, MFCC64, batch, placeholder, post_of
    out = []
    for name, p in (("16 kHz, 400 / 160 / 512, 24 filters", MFCC16), ("8 kHz, 200 / 80 / 256, 20 filters", MFCC8), ("16 kHz, 64 / 32 / 64, 6 filters", MFCC64)):
        sig = R.signals(p["sample_rate"])
        samples, soff = batch(sig)
        refs = [R.mfcc(s, p, with_energies=True) for s in sig]
        with placeholder(2 * p["n_cepstra"] + 1) as m, m.frontend(p, post_of(p)) as fe:
            got, _ = fe.mfcc(samples, soff)
        want = np.concatenate([c for c, _ in refs])
        out.append(f"    {name}: max |device - reference| {np.abs(got - want).max():.3e}, max |c| {np.abs(want).max():.1f}, "
                   f"smallest filter energy {min(float(E.min()) for _, E in refs):.2f} (floor 1.0)")
    return out


def measure(reps):
    from speechrecognition_amd import build, capi, synth
    from tests import frontend_reference as R
    from tests.test_frontend_cpu import build_driver, post_blob
    info = build.build_info()
    head = info.get("git_head", "unknown")
    where = f"the tree of the change that adds the front end, over parent commit {head}" if info.get("dirty") else f"commit {head}"
    p = R.params()
    D, M = 25, 32
    _, off = synth.make_batch(1000, 200, 400, 1, seed=7)
    T = np.diff(off.astype(np.int64))
    F = int(T.sum())
    rng = np.random.default_rng(11)
    lens = p["window"] + (T - 1) * p["shift"]
    soff = np.concatenate([[0], np.cumsum(lens)]).astype(np.uint64)
    samples = np.clip(np.rint(rng.normal(0.0, 1000.0, int(soff[-1]))), -32768, 32767).astype(np.int16)
    lex = synth.make_lexicon(1333, 3, 1)
    spec = synth.make_mixset(lex.n_states, M, D, seed=23)
    tmp = tempfile.mkdtemp()
    mp = os.path.join(tmp, "m.mix")
    synth.write_mixset(mp, spec)
    word_off, automaton, sil = lex.flatten()
    lines = [f"{where}; 1000 utterances, {F} frames, {len(samples)} samples of 16 kHz audio ({len(samples) / 16000.0:.0f} s); window 400, "
             f"shift 160, FFT 512, 24 filters, 12 + 12 + 1 features, mean / deviation and energy normalisation; mean of {reps} calls after one warm-up"]
    with capi.Model.from_mixset(mp, D) as m:
        post = dict(n_static=12, n_first=12, n_second=1, deriv_step=3, energy_max_norm=1)
        with m.frontend(p, post) as plain:
            cep, foff = plain.mfcc(samples, soff)
            assert np.array_equal(foff, off.astype(np.uint64))
            unnorm = plain.from_cepstra(cep, foff)
            rows = unnorm.download()
            unnorm.close()
        mean, stddev = rows.astype(np.float64).mean(axis=0), rows.astype(np.float64).std(axis=0)
        with m.frontend(p, dict(post, mean=mean, stddev=stddev)) as fe:
            corpus, a_ms, a_wall = timed(m, lambda: fe.from_audio(samples, soff), reps)
            c2, c_ms, c_wall = timed(m, lambda: fe.from_cepstra(cep, foff), reps)
            feats = corpus.download()
            assert np.array_equal(feats.view(np.uint32), c2.download().view(np.uint32))
            c2.close()
            _, _, up_wall = timed(m, lambda: m.upload(feats, foff), reps)
            lexh = m.lexicon(word_off, automaton, lex.silence_idx, (3.0, 0.0, 30.0), sil)
            corpus.recognize(lexh, 200.0, 10.0)
            t0 = time.perf_counter()
            for _ in range(reps):
                corpus.recognize(lexh, 200.0, 10.0)
            rec = (time.perf_counter() - t0) / reps * 1e3
            lexh.close()
            corpus.close()
    drv = build_driver(tmp)
    blob = os.path.join(tmp, "post.bin")
    with open(blob, "wb") as f:
        f.write(post_blob(cep, foff, 12, 1, 3, True, mean, stddev))
    host = min(float(subprocess.check_output([drv, "time", blob], text=True).split()[1]) for _ in range(3))
    t0 = time.perf_counter()
    n_ref = 0
    for u in range(4):
        n_ref += len(R.mfcc(samples[int(soff[u]):int(soff[u + 1])], p))
    ref_rate = n_ref / (time.perf_counter() - t0)
    audio_s = len(samples) / 16000.0
    lines += [
        f"  sr_corpus_from_audio, samples on the host    call {a_wall:8.2f} ms   kernels {a_ms:7.3f} ms   "
        f"({audio_s / (a_wall * 1e-3):,.0f} x real time the call, {audio_s / (a_ms * 1e-3):,.0f} x the kernels; {len(samples) * 2 / 1e6:.0f} MB in)",
        f"  sr_corpus_from_cepstra, cepstra on the host   call {c_wall:8.2f} ms   kernels {c_ms:7.3f} ms",
        f"  host: FeaturePostProcessor on one thread     {host:8.2f} ms + sr_corpus_upload {up_wall:6.2f} ms = {host + up_wall:8.2f} ms   "
        f"({(host + up_wall) / c_wall:.1f} x sr_corpus_from_cepstra's call)",
        f"  numpy float64 restatement of the MFCC stage  {ref_rate:8.0f} frames/s ({F / ref_rate * 1e3:,.0f} ms for this corpus)",
        f"  sr_recognize_corpus on the resulting corpus  call {rec:8.2f} ms   (1333 words, {lex.n_states} states x {M} densities, dimension {D}, beam 200)",
        f"  audio -> corpus / recognition step: {a_wall / rec:.2f} (call), {a_ms / rec:.3f} (kernels)   -- expected below 1: "
        f"{'holds' if a_wall < rec else 'DOES NOT HOLD for the call' if a_ms < rec else 'DOES NOT HOLD'}",
        "  accuracy of the MFCC stage on the four test signals (white noise, tone + noise, chirp + noise, faint noise), pre-emphasis 0.9:"]
    lines += accuracy(capi, R)
    return lines


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "frontend.txt"))
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--no-write", action="store_true")
    a = ap.parse_args()
    lines = measure(a.reps)
    print("\n".join(lines))
    if not a.no_write:
        with open(a.out, "w") as f:
            f.write("The audio front end (tools/frontend_time.py)\n" + "\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
