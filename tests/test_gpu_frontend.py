"""The audio front end on the device (sr_frontend_*, sr_corpus_from_audio, sr_corpus_from_cepstra, sr_mfcc_corpus,
sr_corpus_download) against tests/frontend_reference.py.

Post-processing: bit for bit -- every operation of it is one correctly rounded IEEE operation, and a maximum has no order.

MFCC bound.  The device works in FP32 on the float tables the float64 reference widens, so its arithmetic alone separates them.  On
the four test signals a float32 numpy restatement of the same stages differs from the float64 one by at most 2.6e-5 (|c| up to 121);
the bound on |device - reference| is 2e-4 absolute, eight times that, which allows for another sound transform order and the device's
logarithm.  The bound speaks about the logarithm's argument only where the clamp is not in play, so every case first asserts, on the
reference alone, that the smallest filter energy lies above twice the floor (1.0).  The pre-emphasis of these cases is 0.9: with
0.97 the lowest filter of the sigma-3 noise sits at 0.8, below the floor -- (1 - 0.97)^2 of a variance of 9 over a 400-sample
window -- and with 0.9 at 2.9."""
import ctypes as C
import os
import struct
import subprocess

import numpy as np
import pytest

from speechrecognition_amd import capi, synth
from tests import frontend_reference as R

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
REAL = os.path.join(ROOT, "tests", "golden_real", "sietill_real.npz")
BOUND = 2e-4
TDP = (3.0, 0.0, 30.0)
POST = dict(n_static=12, n_first=12, n_second=1, deriv_step=3, energy_max_norm=1)
MFCC16 = R.params(preemphasis=0.9)
MFCC8 = R.params(preemphasis=0.9, sample_rate=8000.0, window=200, shift=80, n_fft=256, n_mel=20, n_cepstra=13, f_low=100.0, f_high=4000.0)
MFCC64 = R.params(preemphasis=0.9, window=64, shift=32, n_fft=64, n_mel=6, n_cepstra=6, f_low=1000.0, f_high=8000.0)


def u32(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def placeholder(D, n_states=3):
    """a model that only holds a corpus"""
    return capi.Model.from_tables(np.arange(n_states + 1, dtype=np.uint32), np.zeros((n_states, D)), np.ones((n_states, D)),
                                  np.zeros(n_states), np.zeros(n_states))


def batch(parts):
    off = np.concatenate([[0], np.cumsum([len(x) for x in parts])]).astype(np.uint64)
    return (np.concatenate(parts) if len(parts) else np.zeros(0, dtype=np.int16)).astype(np.int16), off


def post_of(p, **kw):
    q = dict(n_static=p["n_cepstra"], n_first=p["n_cepstra"], n_second=1, deriv_step=3, energy_max_norm=1)
    q.update(kw)
    return q


# ---- 1. post-processing bits -----------------------------------------------------------------------------------------------------
def test_golden_cepstra_give_the_golden_features_and_words(tmp_path):
    z = np.load(REAL)
    off = z["frame_off"].astype(np.int64)
    norm = z["normalization"].astype(np.float64)
    raw = [z[f"raw_mm2_{i}"].astype(np.float32).reshape(-1, 12) for i in (0, 1)]
    assert [len(r) for r in raw] == [off[1] - off[0], off[2] - off[1]]
    foff = off[:3].astype(np.uint64)
    lex = synth.sietill_lexicon()
    word_off, automaton, sil = lex.flatten()
    mp = tmp_path / "real.mix"
    mp.write_bytes(z["model_mixture"].tobytes())
    tdp = tuple(float(x) for x in z["tdp"])
    with capi.Model.from_mixset(str(mp), 25, capi.POOL_MIXTURE, True) as m:
        with m.frontend(None, dict(POST, mean=norm[:25], stddev=norm[25:])) as fe:
            corpus = fe.from_cepstra(np.concatenate(raw), foff)
            got = corpus.download()
            want = z["feats"][:off[2]]
            assert got.shape == want.shape and np.array_equal(u32(got), u32(want))
            for i in (0, 1):
                ref = R.post_process(raw[i], 12, 1, 3, norm[:25], norm[25:], True)
                assert np.array_equal(u32(got[off[i]:off[i + 1]]), u32(ref))
            lexh = m.lexicon(word_off, automaton, lex.silence_idx, tdp, sil)
            words, woff = corpus.recognize(lexh, float(z["mixture_wide_beam"]), float(z["mixture_wide_wp"]), capi.GMM_EXACT)
            gw = z["mixture_wide_word_off"].astype(np.int64)
            assert np.array_equal(woff.astype(np.int64), gw[:3]) and np.array_equal(words, z["mixture_wide_words"][:gw[2]])
            lexh.close()
            corpus.close()


def random_cepstra(rng, lengths, n_static):
    off = np.concatenate([[0], np.cumsum(lengths)]).astype(np.uint64)
    cep = (rng.normal(size=(int(off[-1]), n_static)) * np.linspace(20.0, 1.0, n_static)[None]).astype(np.float32)
    return cep, off


@pytest.mark.parametrize("normalise", [False, True])
@pytest.mark.parametrize("energy", [False, True])
@pytest.mark.parametrize("shape", [(12, 12, 1, 3), (13, 13, 13, 2)])
def test_random_cepstra_carry_the_host_loop_s_bits(shape, energy, normalise):
    ns, n1, n2, step = shape
    nt = ns + n1 + n2
    rng = np.random.default_rng(nt + 2 * energy + normalise)
    lengths = [0, 1, 2, 3, 4, 7, 50, 0, 700]   # 700: more frames than the maximum's workgroup has threads
    cep, off = random_cepstra(rng, lengths, ns)
    o = off.astype(np.int64)
    cep[o[5] + 2, 0] = cep[o[5]:o[6], 0].max()          # the maximum twice in one utterance
    cep[o[4]:o[5], 0] = [-0.0, 0.0, -1.0, 0.0]           # a maximum of zero, -0 first
    cep[o[8] + 300, 0] = cep[o[8] + 650, 0] = 99.0       # ... and twice far apart
    mean = rng.normal(size=nt) if normalise else None
    stddev = rng.uniform(0.5, 3.0, size=nt) if normalise else None
    want = R.post_process_corpus(cep, off, n1, n2, step, mean, stddev, energy)
    with placeholder(nt) as m:
        post = dict(n_static=ns, n_first=n1, n_second=n2, deriv_step=step, energy_max_norm=int(energy))
        if normalise:
            post.update(mean=mean, stddev=stddev)
        with m.frontend(None, post) as fe:
            corpus = fe.from_cepstra(cep, off)
            got = corpus.download()
            assert got.shape == want.shape and np.array_equal(u32(got), u32(want))
            corpus.close()


# ---- 2. download -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("asynchronous", [False, True])
def test_download_returns_the_uploaded_bits(asynchronous):
    feats, off = synth.make_batch(5, 30, 60, 25, seed=3)
    feats = feats.astype(np.float32)
    feats[7, 3] = -0.0
    feats[8, 4] = np.float32(1e-42)   # a denormal survives too
    with placeholder(25) as m:
        corpus = m.upload(feats, off, asynchronous=asynchronous)
        got = corpus.download()
        assert got.shape == feats.shape and np.array_equal(u32(got), u32(feats))
        # still a corpus like any other
        assert corpus.score(capi.GMM_EXACT).shape == (len(feats), 3)
        corpus.close()
        empty = m.upload(np.zeros((0, 25), dtype=np.float32), np.zeros(3, dtype=np.uint64))
        assert empty.download().shape == (0, 25)
        empty.close()


# ---- 3. framing ------------------------------------------------------------------------------------------------------------------
def test_framing():
    p = MFCC16
    rng = np.random.default_rng(1)
    lens = [p["window"] - 1, p["window"], p["window"] + p["shift"] - 1, p["window"] + p["shift"], 16000]
    samples, soff = batch([rng.normal(0, 300, n).astype(np.int16) for n in lens])
    with placeholder(25) as m, m.frontend(p, post_of(p)) as fe:
        assert [fe.frames(n) for n in lens] == [0, 1, 1, 2, 98]
        corpus = fe.from_audio(samples, soff)
        assert np.array_equal(np.diff(corpus.frame_off.astype(np.int64)), [0, 1, 1, 2, 98])
        assert corpus.download().shape == (102, 25)
        cep, foff = fe.mfcc(samples, soff)
        assert np.array_equal(foff, corpus.frame_off) and cep.shape == (102, 12)
        corpus.close()
        # an all-empty batch, and a batch of no utterances
        samples, soff = batch([np.zeros(n, dtype=np.int16) for n in (0, 10, 399)])
        corpus = fe.from_audio(samples, soff)
        assert corpus.n_frames == 0 and not corpus.frame_off.any() and corpus.download().shape == (0, 25)
        assert corpus.score(capi.GMM_EXACT).shape == (0, 3)
        corpus.close()
        corpus = fe.from_audio(np.zeros(0, dtype=np.int16), np.zeros(1, dtype=np.uint64))
        assert corpus.n_utts == 0 and corpus.n_frames == 0
        corpus.close()
        cep, foff = fe.mfcc(np.zeros(0, dtype=np.int16), np.zeros(1, dtype=np.uint64))
        assert cep.shape == (0, 12) and foff.tolist() == [0]


# ---- 4. MFCC against the float64 reference ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("p", [MFCC16, MFCC8, MFCC64], ids=["16k-400-512", "8k-200-256", "16k-64-64"])
def test_mfcc_matches_the_float64_reference(p):
    sig = R.signals(p["sample_rate"])
    samples, soff = batch(sig)
    refs = [R.mfcc(s, p, with_energies=True) for s in sig]
    smallest = min(float(E.min()) for _, E in refs)
    print(f"smallest reference filter energy {smallest:.3f} (floor {p['energy_floor']})")
    assert smallest > 2.0 * p["energy_floor"]
    want = np.concatenate([c for c, _ in refs])
    with placeholder(2 * p["n_cepstra"] + 1) as m, m.frontend(p, post_of(p)) as fe:
        got, foff = fe.mfcc(samples, soff)
    assert got.shape == want.shape and np.array_equal(np.diff(foff.astype(np.int64)), [len(c) for c, _ in refs])
    err = np.abs(got.astype(np.float64) - want)
    o = foff.astype(np.int64)
    print("max |device - reference| per signal:", [f"{err[o[i]:o[i + 1]].max():.3e}" for i in range(4)], f"max |c| {np.abs(want).max():.1f}")
    assert err.max() <= BOUND


# ---- 5. the clamp ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("floor", [1.0, 2.5])
def test_silence_gives_the_floor(floor):
    p = R.params(preemphasis=0.9, energy_floor=floor)
    samples, soff = batch([np.zeros(2000, dtype=np.int16)])
    want = R.mfcc(samples, p)
    assert np.allclose(want[:, 0], np.sqrt(2.0 / 24) * 24 * np.log(floor), atol=1e-6) and np.abs(want[:, 1:]).max() < 1e-6
    with placeholder(25) as m, m.frontend(p, post_of(p)) as fe:
        got, _ = fe.mfcc(samples, soff)
    assert got.shape == want.shape and np.abs(got - want).max() <= BOUND


# ---- 6. independence and determinism ---------------------------------------------------------------------------------------------
def test_an_utterance_has_the_same_bits_alone_and_twice():
    p = MFCC16
    sig = R.signals(p["sample_rate"], seed=4)
    # lengths that put utterance and workgroup-span boundaries at odd places: 17 frames (one more than a span), an odd sample count
    parts = [sig[0][:3001], sig[1][:400 + 16 * 160], sig[2], sig[3][:399], sig[1][5000:9000]]
    samples, soff = batch(parts)
    norm = np.random.default_rng(2)
    mean, stddev = norm.normal(size=25), norm.uniform(0.5, 2.0, size=25)
    with placeholder(25) as m, m.frontend(p, post_of(p, mean=mean, stddev=stddev)) as fe:
        corpus = fe.from_audio(samples, soff)
        whole = corpus.download()
        again = fe.from_audio(samples, soff)
        assert np.array_equal(u32(again.download()), u32(whole))
        again.close()
        o = corpus.frame_off.astype(np.int64)
        cep, coff = fe.mfcc(samples, soff)
        assert np.array_equal(coff, corpus.frame_off)
        for u, part in enumerate(parts):
            alone = fe.from_audio(part, np.array([0, len(part)], dtype=np.uint64))
            assert alone.n_frames == o[u + 1] - o[u]
            assert np.array_equal(u32(alone.download()), u32(whole[o[u]:o[u + 1]])), u
            alone.close()
            c1, _ = fe.mfcc(part, np.array([0, len(part)], dtype=np.uint64))
            assert np.array_equal(u32(c1), u32(cep[o[u]:o[u + 1]])), u
        # both stages in one call, or one after the other
        two = fe.from_cepstra(cep, coff)
        assert np.array_equal(u32(two.download()), u32(whole))
        two.close()
        corpus.close()


# ---- 7. end to end ---------------------------------------------------------------------------------------------------------------
def test_the_audio_corpus_is_a_corpus_like_any_other(tmp_path):
    p = MFCC16
    lex = synth.make_lexicon(6, 3, 1)
    spec = synth.make_mixset(lex.n_states, 3, 25, seed=41)
    mp = os.path.join(str(tmp_path), "e.mix")
    synth.write_mixset(mp, spec)
    word_off, automaton, sil = lex.flatten()
    samples, soff = batch(R.signals(p["sample_rate"]))
    auts = []
    for w in (1, 2, 3, 4):
        auts.append(np.asarray([sil] + list(automaton[word_off[w]:word_off[w + 1]]) + [sil], dtype=np.uint16))
    with capi.Model.from_mixset(mp, 25) as m, m.frontend(p, post_of(p)) as fe:
        lexh = m.lexicon(word_off, automaton, lex.silence_idx, TDP, sil)
        corpus = fe.from_audio(samples, soff)
        feats = corpus.download()
        assert np.isfinite(feats).all() and feats[:, 0].max() == 0.0
        host = m.upload(feats, corpus.frame_off)
        a, b = corpus.score(capi.GMM_EXACT), host.score(capi.GMM_EXACT)
        assert np.array_equal(a.view(np.uint64), b.view(np.uint64)) and len(np.unique(a.view(np.uint64))) > a.size // 2
        ra = corpus.recognize(lexh, 500.0, 10.0, traceback=True)
        rb = host.recognize(lexh, 500.0, 10.0, traceback=True)
        assert np.array_equal(ra[0], rb[0]) and np.array_equal(ra[1], rb[1])
        for x, y in zip(ra[2], rb[2]):
            assert np.array_equal(x.view(np.uint8), y.view(np.uint8))
        sa, ca = corpus.align(auts, TDP, sil, capi.GMM_EXACT)
        sb, cb = host.align(auts, TDP, sil, capi.GMM_EXACT)
        assert np.array_equal(sa, sb) and np.array_equal(ca.view(np.uint64), cb.view(np.uint64))
        for c in (host, corpus):
            c.close()
        lexh.close()


# ---- 8. errors -------------------------------------------------------------------------------------------------------------------
def test_errors_come_before_any_launch():
    L = capi.lib()
    P = lambda a: None if a is None else a.ctypes.data  # noqa: E731
    with placeholder(25) as m, placeholder(26) as other:
        def create(mfcc=MFCC16, post=POST, model=m, out=True, **kw):
            q = None
            if mfcc is not None:
                d = dict(mfcc, **{k: v for k, v in kw.items() if k in MFCC16 or k == "flags"})
                ints = ("window", "shift", "n_fft", "n_mel", "n_cepstra", "flags")
                q = capi.MfccParams(**{k: (int(v) if k in ints else float(v)) for k, v in d.items()})
            pp = dict(post, **{k: v for k, v in kw.items() if k in POST})
            mean, stddev = kw.get("mean"), kw.get("stddev")
            fp = capi.FeaturePostParams(mean=P(mean), stddev=P(stddev), **pp)
            h = C.c_void_p(0xDEAD)
            rc = L.sr_frontend_create(model.h if model is not None else None, None if q is None else C.byref(q), C.byref(fp),
                                      C.byref(h) if out else None)
            if rc == 0:
                L.sr_frontend_destroy(h)
            else:
                assert not out or not h.value, kw
            return rc

        assert create() == 0
        assert create(mfcc=None) == 0
        nan, inf = float("nan"), float("inf")
        for kw in (dict(shift=0), dict(window=1), dict(n_cepstra=0, n_static=0), dict(n_cepstra=25, n_static=25, n_first=0, n_second=0),
                   dict(f_low=-1.0), dict(f_low=nan), dict(f_high=8000.5), dict(f_high=nan), dict(f_low=5000.0, f_high=4000.0),
                   dict(sample_rate=0.0), dict(sample_rate=inf),
                   dict(f_low=0.0, f_high=200.0),                   # 24 filters within 200 Hz: bins are 31.25 Hz apart
                   dict(energy_floor=0.0), dict(energy_floor=-1.0), dict(energy_floor=inf), dict(energy_floor=nan),
                   dict(preemphasis=nan), dict(flags=1),
                   dict(n_cepstra=11),                              # != n_static
                   dict(n_second=2),                                # the model has 25 dimensions
                   dict(model=other),
                   dict(n_static=12, n_first=13, n_second=0),                           # 25 in all, n_first > n_static
                   dict(n_cepstra=13, n_static=13, n_first=5, n_second=7),              # 25 in all, n_second > n_first
                   dict(deriv_step=0), dict(mean=np.zeros(25)), dict(stddev=np.ones(25)), dict(model=None)):
            assert create(**kw) == -1, kw
        assert create(out=False) == -1
        for kw in (dict(n_fft=500), dict(n_fft=32, window=32), dict(n_fft=4096), dict(window=513), dict(n_mel=65), dict(n_fft=0)):
            assert create(**kw) == -4, kw
        h = C.c_void_p(0xDEAD)
        assert L.sr_frontend_create(m.h, None, None, C.byref(h)) == -1 and not h.value

        samples, soff = batch([np.full(1000, 7, dtype=np.int16), np.full(500, 9, dtype=np.int16)])
        with m.frontend(MFCC16, POST) as fe, m.frontend(None, POST) as cep_only:
            def refused(code, call):
                out = C.c_void_p(0xDEAD)
                foff = np.full(3, 77, dtype=np.uint64)
                cep = np.full((6, 12), 7.5, dtype=np.float32)
                assert call(out, foff, cep) == code
                assert not out.value or out.value == 0xDEAD
                assert (foff == 77).all() and (cep == 7.5).all()
                return out

            bad_first = np.array([1, 1000, 1500], dtype=np.uint64)
            falling = np.array([0, 1000, 900], dtype=np.uint64)
            for fh, so, sp in ((fe.h, bad_first, samples), (fe.h, falling, samples), (fe.h, None, samples), (fe.h, soff, None),
                               (None, soff, samples), (cep_only.h, soff, samples)):
                o = refused(-1, lambda out, foff, cep: L.sr_corpus_from_audio(fh, P(sp), P(so), 2, C.byref(out), P(foff)))
                assert not o.value
                refused(-1, lambda out, foff, cep: L.sr_mfcc_corpus(fh, P(sp), P(so), 2, P(cep), P(foff)))
            o = refused(-1, lambda out, foff, cep: L.sr_corpus_from_audio(fe.h, P(samples), P(soff), 2, C.byref(out), None))
            assert not o.value
            refused(-1, lambda out, foff, cep: L.sr_corpus_from_audio(fe.h, P(samples), P(soff), 2, None, P(foff)))
            refused(-1, lambda out, foff, cep: L.sr_mfcc_corpus(fe.h, P(samples), P(soff), 2, None, P(foff)))
            refused(-1, lambda out, foff, cep: L.sr_mfcc_corpus(fe.h, P(samples), P(soff), 2, P(cep), None))
            # more frames than a corpus takes in one utterance: 65536 frames of window 400, shift 160
            long_off = np.array([0, 400 + 65535 * 160, 400 + 65535 * 160 + 500], dtype=np.uint64)
            long_samples = np.zeros(int(long_off[-1]), dtype=np.int16)
            o = refused(-4, lambda out, foff, cep: L.sr_corpus_from_audio(fe.h, P(long_samples), P(long_off), 2, C.byref(out), P(foff)))
            assert not o.value and b"65535" in L.sr_last_error()
            # cepstra in
            rows = np.zeros((6, 12), dtype=np.float32)
            good = np.array([0, 2, 6], dtype=np.uint64)
            for fh, fo, rw in ((cep_only.h, np.array([1, 2, 6], dtype=np.uint64), rows), (cep_only.h, np.array([0, 4, 2], dtype=np.uint64), rows),
                               (cep_only.h, None, rows), (cep_only.h, good, None), (None, good, rows)):
                o = refused(-1, lambda out, foff, cep: L.sr_corpus_from_cepstra(fh, P(rw), P(fo), 2, C.byref(out)))
                assert not o.value
            assert L.sr_corpus_from_cepstra(cep_only.h, P(rows), P(good), 2, None) == -1
            n = C.c_uint64(77)
            assert L.sr_frontend_frames(cep_only.h, 1000, C.byref(n)) == -1 and n.value == 77
            assert L.sr_frontend_frames(None, 1000, C.byref(n)) == -1 and L.sr_frontend_frames(fe.h, 1000, None) == -1
            # the same arguments without a fault go through
            out = C.c_void_p()
            foff = np.zeros(3, dtype=np.uint64)
            assert L.sr_corpus_from_audio(fe.h, P(samples), P(soff), 2, C.byref(out), P(foff)) == 0 and foff.tolist() == [0, 4, 5]
            assert L.sr_corpus_download(out, None) == -1
            assert L.sr_corpus_download(None, P(np.zeros((5, 25), dtype=np.float32))) == -1
            L.sr_corpus_destroy(out)
            assert L.sr_corpus_from_cepstra(fe.h, P(rows), P(good), 2, C.byref(out)) == 0   # a front end with an MFCC stage takes cepstra too
            L.sr_corpus_destroy(out)


# ---- 9. the C++ mirror -----------------------------------------------------------------------------------------------------------
def test_cpp_front_end_returns_the_same_bits(tmp_path):
    from tests.test_frontend_cpu import build_driver, post_blob, run_driver
    drv = build_driver(tmp_path)
    # FeaturePostProcessor::device_corpus on the golden cepstra
    z = np.load(REAL)
    off = z["frame_off"].astype(np.int64)
    norm = z["normalization"].astype(np.float64)
    raw = np.concatenate([z[f"raw_mm2_{i}"].astype(np.float32).reshape(-1, 12) for i in (0, 1)])
    blob = tmp_path / "post.bin"
    blob.write_bytes(post_blob(raw, off[:3].astype(np.uint64), 12, 1, 3, True, norm[:25], norm[25:]))
    got = run_driver(drv, "cepstra", blob)["feats"].reshape(-1, 25)
    assert np.array_equal(got, u32(z["feats"][:off[2]]))
    # sr::FrontEnd on the test signals
    p = MFCC16
    samples, soff = batch([s[:4000] for s in R.signals(p["sample_rate"])] + [np.zeros(100, dtype=np.int16)])
    blob = tmp_path / "audio.bin"
    blob.write_bytes(struct.pack("<10I", p["window"], p["shift"], p["n_fft"], p["n_mel"], p["n_cepstra"], 12, 1, 3, 1, len(soff) - 1) +
                     struct.pack("<3d2f", p["sample_rate"], p["f_low"], p["f_high"], p["preemphasis"], p["energy_floor"]) +
                     soff.tobytes() + samples.tobytes())
    out = run_driver(drv, "audio", blob)
    with placeholder(25) as m, m.frontend(p, POST) as fe:
        corpus = fe.from_audio(samples, soff)
        feats = corpus.download()
        cep, _ = fe.mfcc(samples, soff)
        assert np.array_equal(out["frame_off"], corpus.frame_off)
        corpus.close()
    assert np.array_equal(out["feats"], u32(feats).reshape(-1)) and np.array_equal(out["cepstra"], u32(cep).reshape(-1))
    want = np.concatenate([R.mfcc(samples[int(soff[u]):int(soff[u + 1])], p) for u in range(4)])
    assert np.abs(cep - want).max() <= BOUND
