"""fMLLR on the device (sr_fmllr_statistics_corpus, sr_fmllr_statistics_bw_corpus, sr_corpus_transform) against the numpy
restatement (tests/fmllr_reference.py), and end to end with sr_fmllr_estimate.

The statistics bound.  u = 2^-53.  A sum of n terms added in any order errs by at most (n - 1) u times the sum of the terms' absolute
values (to first order); the device and the reference each add a speaker's n_s terms in an order of their own, so they differ by at most
2 (n_s - 1) u = (n_s - 1) 2^-52 of that sum.  Forming a term costs a few roundings on either side: gamma iv, (gamma iv) mu, the fold of a
frame's pairs, the fused multiply-add (xi_j xi_k is exact: two 24-bit significands); in soft mode the membership itself -- the device's
exp within 2 ulp, the sum of at most 8 of them, one division, the product with the posterior -- about a dozen u.  C_TERM = 32 halves of
2^-52 cover both sides with room; the bound is (n_s + 32) 2^-52 sum |terms|, derived, not tuned."""
import ctypes as C
import os
import struct
import subprocess

import numpy as np
import pytest

from speechrecognition_amd import capi, synth
from tests import fmllr_reference as R

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EPS = 2.0 ** -52
C_TERM = 32
TDP = (3.0, 0.0, 30.0)


def make_case(D, seed, n_utts=60, speakers=(0, 1, 0, 3, 0, 1), n_speakers=4, tied=False, S=10, M=4, lens=(30, 90)):
    """random model and corpus; utterance u belongs to speakers[u % len]; the last utterance has one frame"""
    rng = np.random.default_rng(seed)
    model = R.random_model(rng, S, M, D)
    T = rng.integers(lens[0], lens[1], size=n_utts)
    T[-1] = 1
    off = np.concatenate([[0], np.cumsum(T)]).astype(np.uint64)
    feats, auts = [], []
    for u in range(n_utts):
        N = 1 if T[u] == 1 else int(rng.integers(2, min(8, T[u]) + 1))
        a = rng.integers(0, S, size=N).astype(np.uint16)
        auts.append(a)
        st = a[np.minimum(np.arange(T[u]) * N // T[u], N - 1)]
        d = np.array([rng.integers(model[0][k], model[0][k + 1]) for k in st])
        feats.append((model[1][d] + 1.3 * rng.normal(size=(T[u], D)) / np.sqrt(model[2][d])).astype(np.float32))
    spk = np.array([speakers[u % len(speakers)] for u in range(n_utts)], dtype=np.uint32)
    return model, np.concatenate(feats), off, auts, spk, n_speakers, tied


def open_model(model, max_approx, tied):
    m = capi.Model.from_tables(*model, max_approx=max_approx)
    if tied:   # one variance row per mixture, one mean row per density
        dens_off = model[0]
        n = int(dens_off[-1])
        dm = np.arange(n, dtype=np.uint32)
        dv = np.repeat(np.arange(len(dens_off) - 1, dtype=np.uint32), np.diff(dens_off.astype(np.int64)))
        capi._check(capi.lib().sr_model_set_tying(m.h, n, len(dens_off) - 1, dm.ctypes.data, dv.ctypes.data))
    return m


def check_stats(got, ref, label):
    beta, k, G = got
    rbeta, rk, rG, kabs, Gabs, n = ref
    worst = 0.0
    for s in range(len(beta)):
        f = (n[s] + C_TERM) * EPS
        for name, a, b, mag in (("G", G[s], rG[s], Gabs[s]), ("k", k[s], rk[s], kabs[s])):
            err, lim = np.abs(a - b), f * mag
            ratio = float((err / np.where(lim > 0, lim, 1.0)).max()) if err.size else 0.0
            worst = max(worst, ratio)
            assert (err <= lim).all(), (label, s, name, ratio)
        assert abs(beta[s] - rbeta[s]) <= f * abs(rbeta[s]), (label, s, beta[s], rbeta[s])
        assert np.array_equal(G[s], np.swapaxes(G[s], 1, 2)), (label, s, "G not exactly symmetric")
        if n[s] == 0:
            assert beta[s] == 0 and not k[s].any() and not G[s].any()
    print(f"{label}: worst |gpu - ref| / bound = {worst:.3f}, pairs per speaker {n.tolist()}")


def aligned_states(corpus, auts, off):
    states, cost = corpus.align(auts, TDP, 0, capi.GMM_DEFAULT)
    states = states.copy()
    for u, a in enumerate(auts):   # a one-frame utterance has no aligner path: its frame takes the automaton's only state
        if int(off[u + 1] - off[u]) == 1:
            states[int(off[u])] = a[0]
    return states


@pytest.mark.parametrize("max_approx", [True, False])
@pytest.mark.parametrize("D,tied", [(2, False), (13, True), (25, False), (39, True), (39, False), (63, False)])
def test_alignment_statistics_against_the_reference(D, tied, max_approx):
    model, feats, off, auts, spk, S, tied = make_case(D, 100 + D, tied=tied)
    with open_model(model, max_approx, tied) as m:
        corpus = m.upload(feats, off)
        states = aligned_states(corpus, auts, off)
        got = corpus.fmllr_statistics(states, spk, S, max_approx)
        again = corpus.fmllr_statistics(states, spk, S, max_approx)
        corpus.close()
    pairs = R.alignment_pairs(feats, model, states, max_approx)
    ref = R.statistics(feats, model, pairs, off, spk, S)
    check_stats(got, ref, f"align D={D} tied={tied} max_approx={max_approx}")
    for a, b in zip(got, again):
        assert np.array_equal(a.view(np.uint64), b.view(np.uint64)), "two identical calls differ"
    if max_approx:   # one pair of weight 1 per frame: beta is the frame count, exactly
        frames = np.zeros(S)
        for u in range(len(spk)):
            frames[spk[u]] += int(off[u + 1] - off[u])
        assert np.array_equal(got[0], frames)
    assert max(ref[5]) > 1024   # some speaker spans more than one segment


@pytest.mark.parametrize("max_approx", [True, False])
@pytest.mark.parametrize("D,tied", [(2, False), (13, True), (25, False), (39, True), (39, False), (63, False)])
def test_posterior_statistics_against_the_reference(D, tied, max_approx):
    # D = 39 untied: a corpus on which speaker 0 spans more than one segment of 1024 frames; the others stay small (the reference
    # walks every posterior item in Python)
    big = D == 39 and not tied
    model, feats, off, auts, spk, S, tied = make_case(D, 200 + D, n_utts=60 if big else 24, tied=tied, lens=(30, 60) if big else (20, 50))
    with open_model(model, max_approx, tied) as m:
        corpus = m.upload(feats, off)
        cost, count, state, weight = corpus.state_posteriors(auts, TDP, 0, capi.GMM_DEFAULT, 0.0, 64)
        bw_cost, got = corpus.fmllr_statistics_bw(auts, TDP, 0, spk, S, capi.GMM_DEFAULT, 0.0, max_approx)
        bw_cost2, again = corpus.fmllr_statistics_bw(auts, TDP, 0, spk, S, capi.GMM_DEFAULT, 0.0, max_approx)
        corpus.close()
    assert int(count.max()) < 64   # no item lost
    assert np.array_equal(cost.view(np.uint64), bw_cost.view(np.uint64))
    pairs = R.posterior_pairs(feats, model, count, state, weight, max_approx)
    ref = R.statistics(feats, model, pairs, off, spk, S)
    check_stats(got, ref, f"posterior D={D} tied={tied} max_approx={max_approx}")
    for a, b in zip(got, again):
        assert np.array_equal(a.view(np.uint64), b.view(np.uint64)), "two identical calls differ"
    if big:   # frames, not pairs: the segments cut a speaker's frames
        frames = np.zeros(S)
        for u in range(len(spk)):
            frames[spk[u]] += int(off[u + 1] - off[u])
        assert frames.max() > 1024


def test_one_speaker_and_shards_add_up():
    D = 13
    model, feats, off, auts, spk, S, _ = make_case(D, 7, speakers=(0,), n_speakers=1)
    o = off.astype(np.int64)
    with open_model(model, True, False) as m:
        corpus = m.upload(feats, off)
        states = aligned_states(corpus, auts, off)
        whole = corpus.fmllr_statistics(states, spk, S, True)
        corpus.close()
        pairs = R.alignment_pairs(feats, model, states, True)
        ref = R.statistics(feats, model, pairs, off, spk, S)
        check_stats(whole, ref, "one speaker")
        rng = np.random.default_rng(3)
        for split in (np.arange(len(spk)) % 2 == 0, rng.random(len(spk)) < 0.3):
            total = [np.zeros_like(a) for a in whole]
            for part in (split, ~split):
                us = np.flatnonzero(part)
                f = np.concatenate([feats[o[u]:o[u + 1]] for u in us])
                st = np.concatenate([states[o[u]:o[u + 1]] for u in us])
                po = np.concatenate([[0], np.cumsum([o[u + 1] - o[u] for u in us])]).astype(np.uint64)
                c = m.upload(f, po)
                for acc, a in zip(total, c.fmllr_statistics(st, spk[us], S, True)):
                    acc += a
                c.close()
            check_stats(total, ref, "two shards")
            assert total[0][0] == whole[0][0]


def _search_case(tmp_path, D=39):
    lex = synth.make_lexicon(20, 3, 1)
    spec = synth.make_mixset(lex.n_states, 4, D, seed=21)
    mp = os.path.join(str(tmp_path), "t.mix")
    synth.write_mixset(mp, spec)
    feats, off = synth.make_batch(8, 40, 80, D, seed=22)
    return lex, mp, feats, off


def test_transform_is_the_documented_loop(tmp_path):
    D = 39
    lex, mp, feats, off = _search_case(tmp_path, D)
    rng = np.random.default_rng(5)
    spk = np.array([0, 2, 1, 0, 2, 2, 1, 0], dtype=np.uint32)
    W = np.tile(np.hstack([np.eye(D), np.zeros((D, 1))]), (3, 1, 1)) + 0.05 * rng.normal(size=(3, D, D + 1))
    want = R.transform(feats, off, spk, W)
    word_off, automaton, sil_state = lex.flatten()
    with capi.Model.from_mixset(mp, D) as m:
        lexh = m.lexicon(word_off, automaton, lex.silence_idx, TDP, sil_state)
        corpus = m.upload(feats, off)
        adapted = corpus.transform(spk, W)
        host = m.upload(want, off)
        a, b = adapted.score(capi.GMM_EXACT), host.score(capi.GMM_EXACT)
        assert np.array_equal(a.view(np.uint64), b.view(np.uint64))
        ra = adapted.recognize(lexh, 200.0, 10.0, traceback=True)
        rb = host.recognize(lexh, 200.0, 10.0, traceback=True)
        assert np.array_equal(ra[0], rb[0]) and np.array_equal(ra[1], rb[1])
        for x, y in zip(ra[2], rb[2]):
            assert np.array_equal(x, y)
        # identity: the original rows (0 + 1 x + zeros), seen through the exact scores; the original corpus is still valid
        ident = corpus.transform(spk, np.tile(np.hstack([np.eye(D), np.zeros((D, 1))]), (3, 1, 1)))
        assert np.array_equal(ident.score(capi.GMM_EXACT).view(np.uint64), corpus.score(capi.GMM_EXACT).view(np.uint64))
        for c in (ident, host, adapted, corpus):
            c.close()
        lexh.close()


def test_adaptation_lowers_the_cost_of_the_alignment():
    """Synthetic corpus drawn from a max-approx model along known alignments, every speaker's features bent by its own affine map.
    With the alignment and the arg-min densities fixed, cost(adapted) - sum_s beta_s logdet_s = cost(original) - (Q(W) - Q(I)); the
    device's path scores re-pick the arg-min, which can only lower the left side."""
    D, S = 13, 3
    rng = np.random.default_rng(77)
    model = R.random_model(rng, 10, 3, D)
    n_utts = 18
    T = rng.integers(40, 80, size=n_utts)
    off = np.concatenate([[0], np.cumsum(T)]).astype(np.uint64)
    spk = (np.arange(n_utts) % S).astype(np.uint32)
    bend = [(np.eye(D) + 0.3 * rng.normal(size=(D, D)) / np.sqrt(D), 0.5 * rng.normal(size=D)) for _ in range(S)]
    feats, auts = [], []
    for u in range(n_utts):
        N = int(rng.integers(3, 8))
        a = rng.integers(0, 10, size=N).astype(np.uint16)
        auts.append(a)
        st = a[np.minimum(np.arange(T[u]) * N // T[u], N - 1)]
        d = np.array([rng.integers(model[0][k], model[0][k + 1]) for k in st])
        y = model[1][d] + rng.normal(size=(T[u], D)) / np.sqrt(model[2][d])
        A, b = bend[spk[u]]
        feats.append((y @ A.T + b).astype(np.float32))
    feats = np.concatenate(feats)
    with capi.Model.from_tables(*model, max_approx=True) as m:
        corpus = m.upload(feats, off)
        states, cost0 = corpus.align(auts, TDP, 0, capi.GMM_DEFAULT)
        # the reference's own gain and the float32 rounding of the adapted features, before any device statistic is looked at
        pairs = R.alignment_pairs(feats, model, states, True)
        rbeta, rk, rG, _, _, _ = R.statistics(feats, model, pairs, off, spk, S)
        I = np.hstack([np.eye(D), np.zeros((D, 1))])
        Wref = np.stack([R.estimate(rbeta[s], rk[s], rG[s], 10) for s in range(S)])
        gain = sum(R.aux(rbeta[s], rk[s], rG[s], Wref[s])[0] - R.aux(rbeta[s], rk[s], rG[s], I)[0] for s in range(S))
        y = R.transform(feats, off, spk, Wref).astype(np.float64)
        dens = np.array([d for _, d, _ in pairs])
        rounding = float((np.abs(y - model[1][dens]) * model[2][dens] * np.abs(y)).sum()) * 2.0 ** -24
        print(f"reference gain {gain:.3f}, float32 rounding of the adapted features at most {rounding:.3e}")
        assert gain > 100 * rounding and gain > 0
        beta, k, G = corpus.fmllr_statistics(states, spk, S, True)
        W, aux, logdet, status = capi.fmllr_estimate(beta, k, G, n_sweeps=10)
        assert status.tolist() == [0] * S
        adapted = corpus.transform(spk, W)
        before = corpus.path_scores(states).sum()
        after = adapted.path_scores(states).sum()
        jac = float((beta * logdet).sum())
        print(f"cost {before:.3f} -> {after:.3f} - {jac:.3f} = {after - jac:.3f}; Q gain {float((aux[:, -1] - aux[:, 0]).sum()):.3f}")
        assert after - jac < before
        # re-aligning the adapted corpus: the new best path costs no more than the old path does on the adapted features
        states2, cost2 = adapted.align(auts, TDP, 0, capi.GMM_DEFAULT)
        old_path = cost0.sum() - before + after
        assert cost2.sum() <= old_path + 1e-9 * abs(old_path)
        adapted.close()
        corpus.close()


def test_errors_are_refused_before_any_launch():
    D = 5
    model, feats, off, auts, spk, S, _ = make_case(D, 9, n_utts=6, lens=(10, 20))
    L = capi.lib()
    with capi.Model.from_tables(*model, max_approx=True) as m:
        corpus = m.upload(feats, off)
        states = aligned_states(corpus, auts, off)
        beta, k, G = corpus._fmllr_out(S)
        P = lambda a: a.ctypes.data  # noqa: E731
        call = lambda sp, n, b, kk, g: L.sr_fmllr_statistics_corpus(m.h, corpus.h, P(states), P(sp), n, 1, b, kk, g)  # noqa: E731
        bad = spk.copy()
        bad[2] = S
        assert call(bad, S, P(beta), P(k), P(G)) == -1
        assert call(spk, 0, P(beta), P(k), P(G)) == -1
        assert call(spk, S, None, P(k), P(G)) == -1
        assert call(spk, S, P(beta), None, P(G)) == -1
        assert call(spk, S, P(beta), P(k), None) == -1
        assert call(spk, 2_000_000_000, P(beta), P(k), P(G)) == -4     # G alone would take 2.9 TB
        assert not beta.any() and not k.any() and not G.any()
        t3 = (C.c_double * 3)(*TDP)
        flat, aoff = corpus._aut(auts)
        cost = np.zeros(len(auts))
        bw = lambda sp, n, b: L.sr_fmllr_statistics_bw_corpus(m.h, corpus.h, P(flat), P(aoff), C.byref(t3), 0, capi.GMM_DEFAULT, 0.0,  # noqa: E731
                                                               P(sp), n, 1, P(cost), b, P(k), P(G))
        assert bw(bad, S, P(beta)) == -1 and bw(spk, 0, P(beta)) == -1 and bw(spk, S, None) == -1
        assert bw(spk, 2_000_000_000, P(beta)) == -4
        assert L.sr_fmllr_statistics_bw_corpus(m.h, corpus.h, P(flat), P(aoff), C.byref(t3), 0, capi.GMM_DEFAULT, -1.0, P(spk), S, 1, P(cost),
                                               P(beta), P(k), P(G)) == -1
        out = C.c_void_p()
        W = np.tile(np.hstack([np.eye(D), np.zeros((D, 1))]), (S, 1, 1))
        assert L.sr_corpus_transform(m.h, corpus.h, P(bad), S, P(W), C.byref(out)) == -1 and not out.value
        assert L.sr_corpus_transform(m.h, corpus.h, P(spk), 0, P(W), C.byref(out)) == -1
        assert L.sr_corpus_transform(m.h, corpus.h, P(spk), S, None, C.byref(out)) == -1
        assert L.sr_corpus_transform(m.h, corpus.h, P(spk), S, P(W), None) == -1
        bad_states = states.copy()
        bad_states[0] = 60000
        assert L.sr_fmllr_statistics_corpus(m.h, corpus.h, P(bad_states), P(spk), S, 1, P(beta), P(k), P(G)) == -1
        corpus.close()
    wide = R.random_model(np.random.default_rng(1), 3, 2, 64)
    with capi.Model.from_tables(*wide, max_approx=True) as m:
        f = np.zeros((4, 64), np.float32)
        corpus = m.upload(f, np.array([0, 4], np.uint64))
        sp = np.zeros(1, np.uint32)
        b, kk, g = np.zeros(1), np.zeros((1, 64, 65)), np.zeros((1, 64, 65, 65))
        st = np.zeros(4, np.uint16)
        assert L.sr_fmllr_statistics_corpus(m.h, corpus.h, st.ctypes.data, sp.ctypes.data, 1, 1, b.ctypes.data, kk.ctypes.data,
                                            g.ctypes.data) == -4
        corpus.close()


def test_cpp_helper_adapts_a_corpus(tmp_path):
    """sr::SpeakerAdaptation through tests/cpp/fmllr_driver: the same transforms, bit for bit, as the calls made from here"""
    D = 13
    lex = synth.make_lexicon(6, 3, 1)
    spec = synth.make_mixset(lex.n_states, 3, D, seed=31)
    mp = os.path.join(str(tmp_path), "a.mix")
    synth.write_mixset(mp, spec)
    feats, off = synth.make_batch(6, 60, 90, D, seed=32)
    spk = np.array([0, 1, 0, 1, 1, 0], dtype=np.uint32)
    word_off, automaton, sil = lex.flatten()
    rng = np.random.default_rng(4)
    orths = [rng.integers(1, 6, size=3).astype(np.uint32) for _ in range(6)]
    orths = [np.where(o == lex.silence_idx, (lex.silence_idx + 1) % 6, o).astype(np.uint32) for o in orths]
    blob = struct.pack("<I", len(lex.word_states))
    for n, r in zip(lex.word_states, lex.word_reps):
        blob += struct.pack("<HH", int(n), int(r))
    blob += struct.pack("<Idddd", lex.silence_idx, *TDP, 10.0) + struct.pack("<I", 6)
    o = off.astype(np.int64)
    for u in range(6):
        blob += struct.pack("<II", int(spk[u]), len(orths[u])) + orths[u].tobytes()
        blob += struct.pack("<I", int(o[u + 1] - o[u])) + feats[o[u]:o[u + 1]].tobytes()
    case = tmp_path / "case.bin"
    case.write_bytes(blob)
    drv = str(tmp_path / "fmllr_driver")
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-Wall", "-I" + os.path.join(ROOT, "include"),
                           os.path.join(ROOT, "tests", "cpp", "fmllr_driver.cpp"), "-o", drv,
                           "-L" + os.path.join(ROOT, "speechrecognition_amd"), "-lsrgpu",
                           "-Wl,-rpath," + os.path.join(ROOT, "speechrecognition_amd"), "-Wl,-rpath,/opt/rocm/lib"])
    out = subprocess.check_output([drv, "adapt", mp, str(D), str(case)], text=True).splitlines()
    assert not out[0].startswith("error"), out[0]
    auts = []
    for u in range(6):
        a = [sil]
        for w in orths[u]:
            a += list(automaton[word_off[w]:word_off[w + 1]]) + [sil]
        auts.append(np.asarray(a, dtype=np.uint16))
    with capi.Model.from_mixset(mp, D) as m:
        corpus = m.upload(feats, off)
        states, _ = corpus.align(auts, TDP, sil, capi.GMM_DEFAULT)
        beta, k, G = corpus.fmllr_statistics(states, spk, 2, True)
        corpus.close()
    W, aux, logdet, status = capi.fmllr_estimate(beta, k, G, n_sweeps=10, min_count=10.0)
    for s in range(2):
        assert out[2 * s].split()[:4] == ["speaker", str(s), "status", str(int(status[s]))]
        got = np.array([int(x, 16) for x in out[2 * s + 1].split()[2:]], dtype=np.uint64)
        assert np.array_equal(got, W[s].reshape(-1).view(np.uint64))
    want = R.transform(feats, off, spk, W)
    x = 0
    for b in want.reshape(-1).view(np.uint32).tolist():
        x ^= b
        x = ((x << 1) | (x >> 63)) & 0xFFFFFFFFFFFFFFFF
    assert out[4].split() == ["checksum", format(x, "x")]
    assert out[5] == "resident equal"
