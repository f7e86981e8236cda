"""VTLN on the device (sr_frontend_create_warped, sr_corpus_from_audio_warped, sr_vtln_costs_corpus, sr_vtln_choose) against
tests/vtln_reference.py.

Bits.  A warped front end behaves as an unwarped one through every older entry point; the filters of alpha == 1.0 are the unwarped
ones; an utterance's rows depend on its samples and its warp alone; the warp search's costs are the sequential sums, in the header's
order, of the path scores of the corpus made with every utterance on that warp -- however the warps are cut into chunks.

Accuracy.  |device - reference| <= 2e-4 on the cepstra of every warp, the unwarped front end's bound (tests/test_gpu_frontend.py gives
its derivation), where the clamp is not in play: every case first asserts, on the reference alone, that the smallest filter energy
over all warps lies above twice the floor.  The sigma-3 noise of frontend_reference.signals() sits at 2.011 under alpha = 1.12, too
close to 2, so the faint signal of these cases is noise of sigma 6 generated here.

The search finds the warp.  A model whose states are the reference's own rows of a signal under alpha* must be matched best by the
device's rows under alpha*; the condition, on the reference alone with costs 0.5 |x - mu|^2, is a gap of at least 1.0 to the second
best warp, where a 2e-4 error per feature moves a cost by about 0.1 at most."""
import ctypes as C
import os

import numpy as np
import pytest

from speechrecognition_amd import capi, synth
from tests import frontend_reference as R
from tests import vtln_reference as V

pytestmark = pytest.mark.gpu

BOUND = 2e-4
# the parameter sets of tests/test_gpu_frontend.py
MFCC16 = R.params(preemphasis=0.9)
MFCC8 = R.params(preemphasis=0.9, sample_rate=8000.0, window=200, shift=80, n_fft=256, n_mel=20, n_cepstra=13, f_low=100.0, f_high=4000.0)
MFCC64 = R.params(preemphasis=0.9, window=64, shift=32, n_fft=64, n_mel=6, n_cepstra=6, f_low=1000.0, f_high=8000.0)
SETS = {"16k-400-512": MFCC16, "8k-200-256": MFCC8, "16k-64-64": MFCC64}
FRAMES = [0, 1, 2, 15, 16, 17, 33]   # 16 is the span length: 17 crosses a span, 33 crosses two
VTLN = dict(alpha=V.ALPHAS, break_frac=V.BREAK)
IDENTITY = V.ALPHAS.index(1.0)
# 14 filters on 33 bins: the unwarped bank is fine, alpha = 1.12 leaves filter 0 without a bin
EMPTIED = R.params(preemphasis=0.9, window=64, shift=32, n_fft=64, n_mel=14, n_cepstra=6, f_low=0.0, f_high=8000.0)


def u32(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def u64(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def placeholder(D, n_states=3):
    return capi.Model.from_tables(np.arange(n_states + 1, dtype=np.uint32), np.zeros((n_states, D)), np.ones((n_states, D)),
                                  np.zeros(n_states), np.zeros(n_states))


def batch(parts):
    off = np.concatenate([[0], np.cumsum([len(x) for x in parts])]).astype(np.uint64)
    return (np.concatenate(parts) if len(parts) else np.zeros(0, dtype=np.int16)).astype(np.int16), off


def post_of(p, **kw):
    q = dict(n_static=p["n_cepstra"], n_first=p["n_cepstra"], n_second=1, deriv_step=3, energy_max_norm=1)
    q.update(kw)
    return q


def utterances(p, faint=False):
    """the seven utterances of FRAMES frames (and a few samples more, short of another frame), cut from the four test signals; faint:
    noise of sigma 6 in place of the sigma-3 signal"""
    sig = R.signals(p["sample_rate"])
    if faint:
        sig[3] = np.clip(np.rint(np.random.default_rng(5).normal(0.0, 6.0, len(sig[3]))), -32768, 32767).astype(np.int16)
    parts = []
    for i, T in enumerate(FRAMES):
        n = p["window"] - 1 if T == 0 else p["window"] + (T - 1) * p["shift"] + (7 * i) % p["shift"]
        parts.append(sig[i % 4][:n])
        assert R.n_frames(n, p) == T
    return parts


@pytest.fixture(scope="module", params=list(SETS), ids=list(SETS))
def warped(request):
    """per parameter set: the utterances (faint noise for the fourth signal), the float64 reference's cepstra and smallest filter
    energy under every warp, and the device's rows with every utterance on warp a -- no normalisation and no energy maximum, so the
    first n_cepstra columns are the cepstra themselves"""
    p = SETS[request.param]
    parts = utterances(p, faint=True)
    samples, soff = batch(parts)
    ref, smallest = [], np.inf
    for alpha in V.ALPHAS:
        got = [V.mfcc(x, p, alpha, V.BREAK, with_energies=True) for x in parts]
        ref.append(np.concatenate([c for c, _ in got]))
        smallest = min([smallest] + [float(E.min()) for _, E in got if E.size])
    D = 2 * p["n_cepstra"] + 1
    with placeholder(D) as m, m.frontend(p, post_of(p, energy_max_norm=0), vtln=VTLN) as fe:
        assert fe.n_warps == 13
        rows = []
        for a in range(13):
            c = fe.from_audio_warped(samples, soff, np.full(len(parts), a))
            assert np.array_equal(np.diff(c.frame_off.astype(np.int64)), FRAMES)
            rows.append(c.download())
            c.close()
    return dict(p=p, parts=parts, samples=samples, soff=soff, ref=ref, smallest=smallest, rows=rows)


# ---- 1. a warped front end is an unwarped one through the old entry points; alpha == 1.0 is the unwarped bank ------------------------
@pytest.mark.parametrize("name", list(SETS))
def test_a_warped_front_end_gives_the_unwarped_bits(name):
    p = SETS[name]
    parts = utterances(p)
    samples, soff = batch(parts)
    D = 2 * p["n_cepstra"] + 1
    rng = np.random.default_rng(3)
    post = post_of(p, mean=rng.normal(size=D), stddev=rng.uniform(0.5, 2.0, size=D))
    no_one = dict(alpha=[0.9, 1.1], break_frac=V.BREAK)   # the unwarped filters are built whether or not 1.0 is among the alphas
    with placeholder(D) as m, m.frontend(p, post) as plain, m.frontend(p, post, vtln=VTLN) as fe, m.frontend(p, post, vtln=no_one) as fe2:
        assert plain.n_warps == 0 and fe.n_warps == 13 and fe2.n_warps == 2
        want = plain.from_audio(samples, soff)
        rows = want.download()
        cep, coff = plain.mfcc(samples, soff)
        assert rows.shape == (sum(FRAMES), D)
        for f in (fe, fe2):
            got = f.from_audio(samples, soff)
            assert np.array_equal(got.frame_off, want.frame_off) and np.array_equal(u32(got.download()), u32(rows))
            got.close()
            c2, o2 = f.mfcc(samples, soff)
            assert np.array_equal(o2, coff) and np.array_equal(u32(c2), u32(cep))
            got = f.from_cepstra(cep, coff)
            assert np.array_equal(u32(got.download()), u32(rows))
            got.close()
            assert [f.frames(len(x)) for x in parts] == FRAMES
        got = fe.from_audio_warped(samples, soff, np.full(len(parts), IDENTITY))
        assert np.array_equal(got.frame_off, want.frame_off) and np.array_equal(u32(got.download()), u32(rows))
        got.close()
        other = fe.from_audio_warped(samples, soff, np.full(len(parts), 0))
        assert not np.array_equal(u32(other.download()), u32(rows))     # (a warp does something)
        other.close()
        want.close()


def test_a_stream_takes_a_warped_front_end_as_an_unwarped_one(tmp_path):
    p = MFCC16
    lex = synth.make_lexicon(6, 3, 1)
    mp = os.path.join(str(tmp_path), "e.mix")
    synth.write_mixset(mp, synth.make_mixset(lex.n_states, 3, 25, seed=41))
    word_off, automaton, sil = lex.flatten()
    x = R.signals(p["sample_rate"])[1][:p["window"] + 16 * p["shift"] + 5]
    out = []
    with capi.Model.from_mixset(mp, 25) as m, m.frontend(p, post_of(p, energy_max_norm=0)) as plain, \
            m.frontend(p, post_of(p, energy_max_norm=0), vtln=VTLN) as fe:
        lexh = m.lexicon(word_off, automaton, lex.silence_idx, (3.0, 0.0, 30.0), sil)
        for f in (plain, fe):
            with m.stream(lexh, 500.0, 10.0, capi.GMM_EXACT, 1, 100) as s:
                s.set_frontend(f)
                i = s.begin()
                a = s.push_audio({i: x[:3000]}, feats=True)[i]
                b = s.push_audio({i: x[3000:]}, feats=True)[i]
                c = s.finish_audio([i], feats=True)[i]
                out.append((np.concatenate([a, b, c]), s.end(i)))
        lexh.close()
    assert out[0][0].shape == (17, 25) and np.array_equal(u32(out[0][0]), u32(out[1][0])) and np.array_equal(out[0][1], out[1][1])


def test_a_bigram_stream_takes_a_warped_front_end_as_an_unwarped_one(tmp_path):
    from tests.test_bigram import _setup
    from tests.test_gpu_bigram_stream import _same
    p = MFCC16
    lex, spec, mp, word_off, mixtures, lm, tdp, _ = _setup(tmp_path, 51, 9, 2, D=25)
    x = R.signals(p["sample_rate"])[2][:p["window"] + 16 * p["shift"] + 5]
    out = []
    with capi.Model.from_mixset(mp, 25) as m, m.frontend(p, post_of(p, energy_max_norm=0)) as plain, \
            m.frontend(p, post_of(p, energy_max_norm=0), vtln=VTLN) as fe:
        bg = m.bigram(word_off, mixtures, lex.silence_idx, lm, tdp)
        for f in (plain, fe):
            with m.bigram_stream(bg, 60.0, 30.0, capi.GMM_PREFILTER, max_streams=1, max_frames=100) as s:
                s.set_frontend(f)
                i = s.begin()
                a = s.push_audio({i: x[:2000]}, feats=True)[i]
                b = s.push_audio({i: x[2000:]}, feats=True)[i]
                c = s.finish_audio([i], feats=True)[i]
                out.append((np.concatenate([a, b, c]), s.end(i)))
        bg.close()
    assert out[0][0].shape == (17, 25) and np.array_equal(u32(out[0][0]), u32(out[1][0])) and _same(out[0][1], out[1][1])


# ---- 2. an utterance's rows depend on its samples and its warp alone ------------------------------------------------------------------
@pytest.mark.parametrize("name", list(SETS))
def test_mixed_warps_equal_each_utterance_alone_on_its_warp(name):
    p = SETS[name]
    parts = utterances(p)
    samples, soff = batch(parts)
    D = 2 * p["n_cepstra"] + 1
    rng = np.random.default_rng(4)
    post = post_of(p, mean=rng.normal(size=D), stddev=rng.uniform(0.5, 2.0, size=D))
    warps = np.array([(5 * i + 1) % 13 for i in range(len(parts))], dtype=np.uint32)   # 1 6 11 3 8 0 5: the identity among them
    with placeholder(D) as m, m.frontend(p, post, vtln=VTLN) as fe:
        c = fe.from_audio_warped(samples, soff, warps)
        mixed, o = c.download(), c.frame_off.astype(np.int64)
        c.close()
        rs, ro = batch(parts[::-1])
        c = fe.from_audio_warped(rs, ro, warps[::-1])
        back, bo = c.download(), c.frame_off.astype(np.int64)
        c.close()
        n = len(parts)
        for u, x in enumerate(parts):
            with m.frontend(p, post, vtln=dict(alpha=[V.ALPHAS[warps[u]]], break_frac=V.BREAK)) as single:
                c = single.from_audio_warped(x, np.array([0, len(x)], dtype=np.uint64), [0])
                alone = c.download()
                c.close()
            assert alone.shape == (FRAMES[u], D)
            assert np.array_equal(u32(alone), u32(mixed[o[u]:o[u + 1]])), u
            assert np.array_equal(u32(alone), u32(back[bo[n - 1 - u]:bo[n - u]])), u


# ---- 3. accuracy ----------------------------------------------------------------------------------------------------------------------
def test_every_warp_s_cepstra_match_the_float64_reference(warped):
    p, nc = warped["p"], warped["p"]["n_cepstra"]
    print(f"smallest reference filter energy over 13 warps {warped['smallest']:.3f} (floor {p['energy_floor']})")
    assert warped["smallest"] > 2.0 * p["energy_floor"]
    worst = []
    for a in range(13):
        got, want = warped["rows"][a][:, :nc].astype(np.float64), warped["ref"][a]
        assert got.shape == want.shape
        worst.append(float(np.abs(got - want).max()))
    print("max |device - reference| per warp:", " ".join(f"{w:.2e}" for w in worst))
    assert max(worst) <= BOUND
    # the warps differ by far more than the bound (the test would notice one warp's table used for another)
    assert min(np.abs(warped["ref"][a] - warped["ref"][a + 1]).max() for a in range(12)) > 100 * BOUND


# ---- 4. the costs are the path scores' sums in the header's order ---------------------------------------------------------------------
SPEAKER = np.array([3, 0, 1, 0, 1, 0, 1], dtype=np.uint32)   # two interleaved speakers; 2 has no utterance; 3 only the one without frames


def mixture_model(D, rng):
    """3 states with 2 densities each"""
    return capi.Model.from_tables(np.array([0, 2, 4, 6], dtype=np.uint32), rng.normal(size=(6, D)) * 3.0, rng.uniform(0.2, 2.0, size=(6, D)),
                                  rng.normal(size=6), np.full(6, np.log(0.5)), max_approx=False)


def with_budget(kb, f):
    """f() under SRGPU_VTLN_KB = kb (None: the default budget), which is read when a model is made"""
    keep = os.environ.get("SRGPU_VTLN_KB")
    if kb is not None:
        os.environ["SRGPU_VTLN_KB"] = str(kb)
    try:
        return f()
    finally:
        if kb is not None:
            os.environ.pop("SRGPU_VTLN_KB")
            if keep is not None:
                os.environ["SRGPU_VTLN_KB"] = keep


def check_composition(m, fe, samples, soff, states, speaker, n_speakers, want_chunks=None):
    """want_chunks: the chunks of warps the library says the call takes (sr_vtln_chunks; the call sizes its chunks with the same
    function); None: not looked at"""
    scores = []
    for a in range(fe.n_warps):
        c = fe.from_audio_warped(samples, soff, np.full(len(soff) - 1, a))
        foff = c.frame_off
        scores.append(c.path_scores(states))
        c.close()
    want, want_frames = V.costs(np.array(scores), foff, speaker, n_speakers)
    assert want_chunks is None or fe.vtln_chunks(int(foff[-1]), len(soff) - 1) == want_chunks
    cost, frames = fe.vtln_costs(samples, soff, states, speaker, n_speakers)
    again, _ = fe.vtln_costs(samples, soff, states, speaker, n_speakers)
    assert cost.shape == (n_speakers, fe.n_warps) and np.array_equal(frames, want_frames)
    assert np.array_equal(u64(cost), u64(want)) and np.array_equal(u64(cost), u64(again))
    return cost, frames


# one warp of the 84 frames takes 84 x (12 x 4 + 25 x 4 + 2 + 8) = 13 272 bytes: 30 KiB are chunks of two warps (seven for 13 warps, the
# last of one), 1 KiB chunks of one; sr_vtln_chunks tells how many chunks a call takes
@pytest.mark.parametrize("n_warps,kb,chunks", [(1, None, 1), (2, None, 1), (3, None, 1), (13, None, 1), (13, 30, 7), (3, 1, 3), (13, 1, 13)])
def test_the_costs_are_the_path_scores_sums(n_warps, kb, chunks):
    p = MFCC16
    parts = utterances(p)
    samples, soff = batch(parts)
    rng = np.random.default_rng(6)
    post = post_of(p, mean=rng.normal(size=25) * 3.0, stddev=rng.uniform(0.5, 2.0, size=25) * 10.0)
    states = rng.integers(0, 3, size=sum(FRAMES)).astype(np.uint16)
    alphas = V.ALPHAS if n_warps == 13 else [0.9, 1.0, 1.1][:n_warps]   # 3 warps x 24 filters: 72 pairs, more than one round of 64 lanes

    def run():
        with mixture_model(25, rng) as m, m.frontend(p, post, vtln=dict(alpha=alphas, break_frac=V.BREAK)) as fe:
            return check_composition(m, fe, samples, soff, states, SPEAKER, 4, want_chunks=chunks)
    cost, frames = with_budget(kb, run)
    assert frames.tolist() == [1 + 15 + 17, 2 + 16 + 33, 0, 0]
    assert not cost[2:].any() and not np.signbit(cost[2:]).any()   # no utterance, and one without frames: +0
    assert np.isfinite(cost).all() and (n_warps == 1 or len(np.unique(u64(cost[0]))) == n_warps)


def test_the_chunks_do_not_change_the_bits():
    p = MFCC16
    samples, soff = batch(utterances(p))
    rng = np.random.default_rng(6)
    states = rng.integers(0, 3, size=sum(FRAMES)).astype(np.uint16)
    got = []
    for kb, chunks in ((None, 1), (30, 7), (1, 13)):
        def run():
            r = np.random.default_rng(8)
            with mixture_model(25, r) as m, m.frontend(p, post_of(p), vtln=VTLN) as fe:
                return fe.vtln_costs(samples, soff, states, SPEAKER, 4)[0], fe.vtln_chunks(sum(FRAMES), len(soff) - 1)
        cost, used = with_budget(kb, run)
        assert used == chunks
        got.append(cost)
    assert np.array_equal(u64(got[0]), u64(got[1])) and np.array_equal(u64(got[0]), u64(got[2]))


# ---- 5. the search finds the warp -----------------------------------------------------------------------------------------------------
STARS = [0.88, 0.94, 1.0, 1.06, 1.12]


@pytest.fixture(scope="module")
def star_rows():
    """the reference's rows (12 + 12 + 1, no normalisation, no energy maximum) of a 30-frame cut of each signal under every warp"""
    p = MFCC16
    parts = [s[:p["window"] + 29 * p["shift"]] for s in R.signals(p["sample_rate"])]
    rows = [[R.post_process(V.mfcc(x, p, alpha, V.BREAK).astype(np.float32), 12, 1, 3, None, None, False).astype(np.float64) for alpha in V.ALPHAS]
            for x in parts]
    return parts, rows


@pytest.mark.parametrize("stars", [STARS[:4], [STARS[4], STARS[0], STARS[3], STARS[2]]], ids=["0.88-1.06", "1.12-1.0"])
def test_the_search_finds_the_warp(star_rows, stars):
    p = MFCC16
    parts, rows = star_rows
    want = [V.ALPHAS.index(a) for a in stars]
    # the condition, on the reference alone: the best cost at alpha*, the second best at least 1.0 above
    for s in range(4):
        c = np.array([0.5 * ((rows[s][a] - rows[s][want[s]]) ** 2).sum() for a in range(13)])
        order = np.argsort(c)
        print(f"signal {s}, alpha* {stars[s]}: gap to the second best warp {c[order[1]] - c[order[0]]:.2f}")
        assert order[0] == want[s] and c[order[1]] - c[order[0]] >= 1.0
    means = np.concatenate([rows[s][want[s]] for s in range(4)])          # 120 states: speaker s has states 30 s .. 30 s + 29
    samples, soff = batch(parts)
    states = np.arange(120, dtype=np.uint16)                                # state t at frame t
    with capi.Model.from_tables(np.arange(121, dtype=np.uint32), means, np.ones((120, 25)), np.zeros(120), np.zeros(120)) as m, \
            m.frontend(p, post_of(p, energy_max_norm=0), vtln=VTLN) as fe:
        cost, frames = check_composition(m, fe, samples, soff, states, np.arange(4, dtype=np.uint32), 4)
    assert frames.tolist() == [30] * 4
    assert capi.vtln_choose(cost, frames, 0, 0).tolist() == want
    assert capi.vtln_choose(cost, frames, 31, 5).tolist() == [5] * 4


# ---- 6. refusals ----------------------------------------------------------------------------------------------------------------------
def test_refusals_come_before_any_launch():
    L = capi.lib()
    P = lambda a: None if a is None else a.ctypes.data  # noqa: E731
    nan, inf = float("nan"), float("inf")
    ints = ("window", "shift", "n_fft", "n_mel", "n_cepstra", "flags")
    with placeholder(25) as m, placeholder(13) as m13:
        def create(alpha=V.ALPHAS, brk=V.BREAK, mfcc=MFCC16, model=m, vtln=True, n_warps=None, out=True):
            q = None if mfcc is None else capi.MfccParams(**{k: (int(v) if k in ints else float(v)) for k, v in mfcc.items()})
            D = 25 if mfcc is None else 2 * mfcc["n_cepstra"] + 1
            fp = capi.FeaturePostParams(n_static=D // 2, n_first=D // 2, n_second=1, deriv_step=3, energy_max_norm=1, mean=None, stddev=None)
            al = None if alpha is None else np.ascontiguousarray(alpha, dtype=np.float64)
            vp = capi.VtlnParams(n_warps=(0 if al is None else len(al)) if n_warps is None else n_warps, alpha=P(al), break_frac=brk)
            h = C.c_void_p(0xDEAD)
            rc = L.sr_frontend_create_warped(model.h, None if q is None else C.byref(q), C.byref(vp) if vtln else None, C.byref(fp),
                                             C.byref(h) if out else None)
            if rc == 0:
                L.sr_frontend_destroy(h)
            else:
                assert not out or not h.value
            return rc

        assert create() == 0 and create(alpha=[1.0] * 32) == 0
        assert create(mfcc=dict(MFCC16, n_mel=40)) == 0                      # 13 x 40 fits
        for kw in (dict(alpha=[]), dict(alpha=None, n_warps=3), dict(alpha=[1.0, 0.0]), dict(alpha=[-1.0]), dict(alpha=[nan]), dict(alpha=[inf]),
                   dict(brk=0.0), dict(brk=1.0), dict(brk=nan), dict(mfcc=None), dict(vtln=False), dict(out=False),
                   dict(mfcc=dict(MFCC16, shift=0)), dict(model=m13)):
            assert create(**kw) == -1, kw
        for kw in (dict(alpha=[1.0] * 33), dict(alpha=[1.0] * 26, mfcc=dict(MFCC16, n_mel=40)), dict(mfcc=dict(MFCC16, n_fft=500))):
            assert create(**kw) == -4, kw
        assert create(alpha=[1.0], mfcc=EMPTIED, model=m13) == 0
        assert create(alpha=[1.0, 1.12], mfcc=EMPTIED, model=m13) == -1
        assert b"warp 1" in L.sr_last_error() and b"filter 0" in L.sr_last_error()
        n = C.c_uint32(77)
        assert L.sr_frontend_warps(None, C.byref(n)) == -1 and n.value == 77

        samples, soff = batch([np.full(1000, 7, dtype=np.int16), np.full(500, 9, dtype=np.int16)])   # 4 frames and 1
        with m.frontend(MFCC16, post_of(MFCC16), vtln=VTLN) as fe, m.frontend(MFCC16, post_of(MFCC16)) as plain:
            assert L.sr_frontend_warps(fe.h, None) == -1
            k = C.c_uint32(77)
            assert L.sr_vtln_chunks(plain.h, 5, 2, C.byref(k)) == -1 and L.sr_vtln_chunks(None, 5, 2, C.byref(k)) == -1
            assert L.sr_vtln_chunks(fe.h, 5, 2, None) == -1 and k.value == 77
            assert L.sr_vtln_chunks(fe.h, 5, 2, C.byref(k)) == 0 and k.value == 1
            warps = np.array([0, 12], dtype=np.uint32)
            falling = np.array([0, 1000, 900], dtype=np.uint64)
            for fh, so, sp, uw in ((fe.h, soff, samples, np.array([0, 13], dtype=np.uint32)), (fe.h, soff, samples, None), (plain.h, soff, samples, warps),
                                   (None, soff, samples, warps), (fe.h, falling, samples, warps), (fe.h, soff, None, warps)):
                out = C.c_void_p(0xDEAD)
                foff = np.full(3, 77, dtype=np.uint64)
                assert L.sr_corpus_from_audio_warped(fh, P(sp), P(so), 2, P(uw), C.byref(out), P(foff)) == -1
                assert not out.value and (foff == 77).all()
            out = C.c_void_p(0xDEAD)
            assert L.sr_corpus_from_audio_warped(fe.h, P(samples), P(soff), 2, P(warps), C.byref(out), None) == -1 and not out.value
            assert L.sr_corpus_from_audio_warped(fe.h, P(samples), P(soff), 2, P(warps), None, P(np.zeros(3, dtype=np.uint64))) == -1

            states = np.zeros(5, dtype=np.uint16)
            spk = np.array([0, 1], dtype=np.uint32)
            bad_state = np.array([0, 0, 3, 0, 0], dtype=np.uint16)
            for fh, so, sp, st, sk, ns in ((fe.h, soff, samples, bad_state, spk, 2), (fe.h, soff, samples, states, np.array([0, 2], dtype=np.uint32), 2),
                                           (plain.h, soff, samples, states, spk, 2), (None, soff, samples, states, spk, 2),
                                           (fe.h, falling, samples, states, spk, 2), (fe.h, soff, samples, None, spk, 2),
                                           (fe.h, soff, samples, states, None, 2), (fe.h, soff, None, states, spk, 2)):
                cost = np.full((ns, 13), 7.5)
                frames = np.full(ns, 77, dtype=np.uint64)
                assert L.sr_vtln_costs_corpus(fh, P(sp), P(so), 2, P(st), P(sk), ns, P(cost), P(frames)) == -1
                assert (cost == 7.5).all() and (frames == 77).all()
            frames = np.full(2, 77, dtype=np.uint64)
            assert L.sr_vtln_costs_corpus(fe.h, P(samples), P(soff), 2, P(states), P(spk), 2, None, P(frames)) == -1 and (frames == 77).all()
            cost = np.full((2, 13), 7.5)
            assert L.sr_vtln_costs_corpus(fe.h, P(samples), P(soff), 2, P(states), P(spk), 2, P(cost), None) == -1 and (cost == 7.5).all()
            # the same arguments without a fault go through
            assert L.sr_vtln_costs_corpus(fe.h, P(samples), P(soff), 2, P(states), P(spk), 2, P(cost), P(frames)) == 0
            assert frames.tolist() == [4, 1] and np.isfinite(cost).all()

        w = np.full(2, 77, dtype=np.uint32)
        c2 = np.zeros((2, 3))
        f2 = np.ones(2, dtype=np.uint64)
        assert L.sr_vtln_choose(2, 0, P(c2), P(f2), 0, 0, P(w)) == -1 and L.sr_vtln_choose(2, 3, P(c2), P(f2), 0, 3, P(w)) == -1
        assert L.sr_vtln_choose(2, 3, None, P(f2), 0, 0, P(w)) == -1 and L.sr_vtln_choose(2, 3, P(c2), None, 0, 0, P(w)) == -1
        assert L.sr_vtln_choose(2, 3, P(c2), P(f2), 0, 0, None) == -1 and (w == 77).all()
        assert L.sr_vtln_choose(2, 3, P(c2), P(f2), 0, 2, P(w)) == 0 and w.tolist() == [0, 0]
