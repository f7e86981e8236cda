"""MLLR mean adaptation on the device (sr_mllr_statistics_corpus, sr_mllr_statistics_bw_corpus, sr_model_transform_means) against the
numpy restatement (tests/mllr_reference.py, sums in longdouble), and end to end with sr_mllr_estimate.

The statistics bound, per (speaker, class) group and element: (n + C_TERM) 2^-52 sum |terms|, n = the group's pairs + its entries
(occupied densities).  u = 2^-53.  Counting the device's roundings of one element:
  - x_acc of an entry: a product gamma x and an addition per pair, occ an addition per pair: at most 2 u per pair, 2 n_pairs u in all,
    relative to the sum of |gamma x| (what the reference's absolute sums carry);
  - the contraction: a product and an addition per entry (whether or not the matrix core fuses them): 2 n_entries u;
  so far 2 (n_pairs + n_entries) u = n 2^-52;
  - forming a term: occ iv or iv x_acc (1 u), xi_j xi_k (1 u; xi_j 1 is exact): 2 u;
  - the segments' partial sums: one addition per segment, at most 2 here: 2 u;
  - the weights themselves in soft mode: the scores are bit-equal on both sides (the reference replays the kernel's order), the device's
    exp is within 2 ulp and numpy's within 1 (3 u), the normalising sum adds the same values in the same order and inherits those 3 u,
    one division (1 u), the product with the posterior (1 u): 8 u;
  - the reference's longdouble sums: below 2^-11 u per term.
That is 12 u = 6 x 2^-52 besides n; C_TERM = 16 covers it with room and was fixed before the first run."""
import ctypes as C

import numpy as np
import pytest

from speechrecognition_amd import capi
from tests import fmllr_reference as F
from tests import mllr_reference as R

pytestmark = pytest.mark.gpu

EPS = 2.0 ** -52
C_TERM = 16
SEG = 1024   # entries per segment (include/srgpu.h)
TDP = (3.0, 0.0, 30.0)
N_CLASSES = 3


def make_case(D, seed, n_utts=60, speakers=(0, 1, 0, 3, 0, 1), n_speakers=4, tied=False, S=10, M=4, lens=(30, 90)):
    """random model and corpus; utterance u belongs to speakers[u % len] (speaker 2 has none); the last utterance has one frame;
    the densities of the first third of the mixtures are class 0, the rest class 2: class 1 has none"""
    rng = np.random.default_rng(seed)
    model = F.random_model(rng, S, M, D)
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
    return model, np.concatenate(feats), off, auts, spk, n_speakers, tied, state_classes(model[0], S // 3)


def state_classes(dens_off, first):
    n = np.diff(dens_off.astype(np.int64))
    return np.repeat(np.where(np.arange(len(n)) < first, 0, 2), n).astype(np.uint32)


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
    rbeta, rk, rG, kabs, Gabs, n, n_ent = ref
    worst = 0.0
    for s in range(beta.shape[0]):
        for r in range(beta.shape[1]):
            f = (n[s, r] + C_TERM) * EPS
            for name, a, b, mag in (("G", G[s, r], rG[s, r], Gabs[s, r]), ("k", k[s, r], rk[s, r], kabs[s, r])):
                err, lim = np.abs(a - b), f * mag
                ratio = float((err / np.where(lim > 0, lim, 1.0)).max())
                worst = max(worst, ratio)
                assert (err <= lim).all(), (label, s, r, name, ratio)
            assert abs(beta[s, r] - rbeta[s, r]) <= f * abs(rbeta[s, r]), (label, s, r, beta[s, r], rbeta[s, r])
            assert np.array_equal(G[s, r], np.swapaxes(G[s, r], 1, 2)), (label, s, r, "G not exactly symmetric")
            if n[s, r] == 0:
                assert beta[s, r] == 0 and not k[s, r].any() and not G[s, r].any()
    print(f"{label}: worst |gpu - ref| / bound = {worst:.3f}, pairs + entries per group {n.tolist()}")


def aligned_states(corpus, auts, off):
    states, cost = corpus.align(auts, TDP, 0, capi.GMM_DEFAULT)
    states = states.copy()
    for u, a in enumerate(auts):   # a one-frame utterance has no aligner path: its frame takes the automaton's only state
        if int(off[u + 1] - off[u]) == 1:
            states[int(off[u])] = a[0]
    return states


def bits(a):
    return np.ascontiguousarray(a).view(np.uint64)


SHAPES = [(2, False), (13, True), (39, False), (63, False)]   # one per row-tile count of the contraction


@pytest.mark.parametrize("max_approx", [True, False])
@pytest.mark.parametrize("D,tied", SHAPES)
def test_alignment_statistics_against_the_reference(D, tied, max_approx):
    model, feats, off, auts, spk, S, tied, cls = make_case(D, 300 + D, tied=tied)
    with open_model(model, max_approx, tied) as m:
        corpus = m.upload(feats, off)
        states = aligned_states(corpus, auts, off)
        got = corpus.mllr_statistics(states, spk, S, cls, N_CLASSES, max_approx)
        again = corpus.mllr_statistics(states, spk, S, cls, N_CLASSES, max_approx)
        corpus.close()
    pairs = F.alignment_pairs(feats, model, states, max_approx)
    ref = R.statistics(feats, model, pairs, off, spk, S, cls, N_CLASSES)
    check_stats(got, ref, f"align D={D} tied={tied} max_approx={max_approx}")
    for a, b in zip(got, again):
        assert np.array_equal(bits(a), bits(b)), "two identical calls differ"
    assert not ref[5][2].any() and not ref[5][:, 1].any()   # a speaker and a class without pairs ...
    assert (ref[5][[0, 1, 3]][:, [0, 2]] > 0).all()                                  # ... every other group has some
    if max_approx:   # one pair of weight 1 per frame: a speaker's betas add up to its frame count, exactly
        frames = np.zeros(S)
        for u in range(len(spk)):
            frames[spk[u]] += int(off[u + 1] - off[u])
        assert np.array_equal(got[0].sum(axis=1), frames)


@pytest.mark.parametrize("max_approx", [True, False])
@pytest.mark.parametrize("D,tied", SHAPES)
def test_posterior_statistics_against_the_reference(D, tied, max_approx):
    model, feats, off, auts, spk, S, tied, cls = make_case(D, 400 + D, n_utts=24, tied=tied, lens=(20, 50))
    with open_model(model, max_approx, tied) as m:
        corpus = m.upload(feats, off)
        cost, count, state, weight = corpus.state_posteriors(auts, TDP, 0, capi.GMM_DEFAULT, 0.0, 64)
        bw_cost, got = corpus.mllr_statistics_bw(auts, TDP, 0, spk, S, cls, N_CLASSES, capi.GMM_DEFAULT, 0.0, max_approx)
        bw_cost2, again = corpus.mllr_statistics_bw(auts, TDP, 0, spk, S, cls, N_CLASSES, capi.GMM_DEFAULT, 0.0, max_approx)
        corpus.close()
    assert int(count.max()) < 64   # no item lost
    assert np.array_equal(bits(cost), bits(bw_cost))
    pairs = F.posterior_pairs(feats, model, count, state, weight, max_approx)
    ref = R.statistics(feats, model, pairs, off, spk, S, cls, N_CLASSES)
    check_stats(got, ref, f"posterior D={D} tied={tied} max_approx={max_approx}")
    for a, b in zip(got, again):
        assert np.array_equal(bits(a), bits(b)), "two identical calls differ"


def two_segment_case():
    """48 mixtures x 32 densities, means close together under wide variances, so that every soft membership stays above the 1e-8 drop;
    one speaker visits every mixture; the last mixture's densities are class 1, all others class 0: more than SEG entries there"""
    D, S, M = 3, 48, 32
    rng = np.random.default_rng(11)
    dens_off = (np.arange(S + 1) * M).astype(np.uint32)
    means = rng.normal(0.0, 0.5, size=(S * M, D))
    var = rng.uniform(4.0, 8.0, size=(S * M, D))
    norm = 0.5 * (D * np.log(2 * np.pi) + np.log(var).sum(axis=1))
    logw = np.full(S * M, -np.log(M))
    model = (dens_off, means, 1.0 / var, norm, logw)
    n_utts, T = 12, 10
    states = (np.arange(n_utts * T) * 7 % S).astype(np.uint16)   # 7 and 48 are coprime: all 48 mixtures within 48 frames
    feats = (means[states.astype(np.int64) * M] + rng.normal(size=(n_utts * T, D))).astype(np.float32)
    off = (np.arange(n_utts + 1) * T).astype(np.uint64)
    spk = np.array([0] * 9 + [1] * 3, dtype=np.uint32)
    cls = state_classes(dens_off, S - 1) // 2
    return model, feats, off, states, spk, cls


def test_a_group_of_more_than_one_segment():
    model, feats, off, states, spk, cls = two_segment_case()
    pairs = F.alignment_pairs(feats, model, states, False)
    ref = R.statistics(feats, model, pairs, off, spk, 2, cls, 2)
    assert ref[6][0, 0] > SEG, ref[6].tolist()   # (speaker 0, class 0) spans two segments; checked on the CPU before any device run
    assert 0 < ref[6][1, 0] <= SEG and ref[6][0, 1] > 0
    with capi.Model.from_tables(*model, max_approx=False) as m:
        corpus = m.upload(feats, off)
        got = corpus.mllr_statistics(states, spk, 2, cls, 2, False)
        again = corpus.mllr_statistics(states, spk, 2, cls, 2, False)
        corpus.close()
    check_stats(got, ref, f"two segments ({ref[6].tolist()} entries)")
    for a, b in zip(got, again):
        assert np.array_equal(bits(a), bits(b))


def test_shards_add_up():
    D = 13
    model, feats, off, auts, spk, S, _, cls = make_case(D, 17)
    o = off.astype(np.int64)
    with open_model(model, True, False) as m:
        corpus = m.upload(feats, off)
        states = aligned_states(corpus, auts, off)
        whole = corpus.mllr_statistics(states, spk, S, cls, N_CLASSES, True)
        corpus.close()
        ref = R.statistics(feats, model, F.alignment_pairs(feats, model, states, True), off, spk, S, cls, N_CLASSES)
        split = np.arange(len(spk)) % 2 == 0
        total = [np.zeros_like(a) for a in whole]
        for part in (split, ~split):
            us = np.flatnonzero(part)
            f = np.concatenate([feats[o[u]:o[u + 1]] for u in us])
            st = np.concatenate([states[o[u]:o[u + 1]] for u in us])
            po = np.concatenate([[0], np.cumsum([o[u + 1] - o[u] for u in us])]).astype(np.uint64)
            c = m.upload(f, po)
            for acc, a in zip(total, c.mllr_statistics(st, spk[us], S, cls, N_CLASSES, True)):
                acc += a
            c.close()
        n2 = ref[5] + ref[6]   # an entry may be occupied in both shards
        check_stats(total, ref[:5] + (n2, ref[6]), "two shards")
        assert np.array_equal(total[0], whole[0])


def test_identity_transform_keeps_every_table_and_score():
    D = 39
    model, feats, off, auts, spk, S, _, cls = make_case(D, 21, n_utts=6, tied=True)
    with open_model(model, True, True) as m:
        with m.transform_means(cls, R.identity(D, N_CLASSES)) as a:
            for x, y in zip(m.tables(), a.tables()):
                assert np.array_equal(bits(x), bits(y))
            for x, y in zip(m.topology(), a.topology()):
                assert np.array_equal(x, y)
            assert m.tying_info() == a.tying_info()
            c0, c1 = m.upload(feats, off), a.upload(feats, off)
            for kernel in (capi.GMM_EXACT, capi.GMM_PREFILTER, capi.GMM_MFMA):
                assert np.array_equal(bits(c0.score(kernel)), bits(c1.score(kernel))), kernel
            c0.close()
            c1.close()


@pytest.mark.parametrize("D", [2, 39, 63])
def test_random_transform_is_the_documented_loop(D):
    model, feats, off, auts, spk, S, _, cls = make_case(D, 23 + D, n_utts=4, S=40, M=8)   # 40 mixtures: a class of several blocks
    rng = np.random.default_rng(D)
    W = R.identity(D, N_CLASSES) + 0.2 * rng.normal(size=(N_CLASSES, D, D + 1))
    want = R.transform_means(model[1], cls, W)
    assert int((cls == 2).sum()) > 64
    with open_model(model, True, True) as m:
        with m.transform_means(cls, W) as a:
            t0, t1 = m.tables(), a.tables()
            assert np.array_equal(bits(t1[0]), bits(want))
            assert not np.array_equal(t1[0], t0[0])
            for x, y in zip(t0[1:], t1[1:]):
                assert np.array_equal(bits(x), bits(y))
            for x, y in zip(m.topology(), a.topology()):
                assert np.array_equal(x, y)
            assert m.tying_info() == a.tying_info()
            # the adapted model scores like a model created from its tables
            with capi.Model.from_tables(model[0], want, *model[2:], max_approx=True) as b:
                ca, cb = a.upload(feats, off), b.upload(feats, off)
                assert np.array_equal(bits(ca.score(capi.GMM_EXACT)), bits(cb.score(capi.GMM_EXACT)))
                ca.close()
                cb.close()


def test_transform_errors():
    D = 5
    model, feats, off, auts, spk, S, _, cls = make_case(D, 29, n_utts=4)
    L = capi.lib()
    P = lambda a: a.ctypes.data  # noqa: E731
    W = R.identity(D, N_CLASSES)
    with capi.Model.from_tables(*model, max_approx=True) as m:
        out = C.c_void_p()
        call = lambda c, n, w, o: L.sr_model_transform_means(m.h, c, n, w, o)  # noqa: E731
        bad = cls.copy()
        bad[1] = N_CLASSES
        assert call(P(bad), N_CLASSES, P(W), C.byref(out)) == -1 and not out.value
        assert call(P(cls), 0, P(W), C.byref(out)) == -1
        assert call(None, N_CLASSES, P(W), C.byref(out)) == -1
        assert call(P(cls), N_CLASSES, None, C.byref(out)) == -1
        assert call(P(cls), N_CLASSES, P(W), None) == -1
        # densities 0 and n - 1 share a mean row but not a class
        n = m.n_densities
        dm = np.arange(n, dtype=np.uint32)
        dm[n - 1] = 0
        dv = np.arange(n, dtype=np.uint32)
        capi._check(L.sr_model_set_tying(m.h, n, n, P(dm), P(dv)))
        assert cls[0] != cls[n - 1]
        assert call(P(cls), N_CLASSES, P(W), C.byref(out)) == -1 and not out.value
        assert b"mean row" in L.sr_last_error()
        same = cls.copy()
        same[n - 1] = cls[0]
        assert call(P(same), N_CLASSES, P(W), C.byref(out)) == 0
        L.sr_model_destroy(out)


def test_statistics_errors_are_refused_before_any_launch():
    D = 5
    model, feats, off, auts, spk, S, _, cls = make_case(D, 9, n_utts=6, lens=(10, 20))
    L = capi.lib()
    P = lambda a: a.ctypes.data  # noqa: E731
    with capi.Model.from_tables(*model, max_approx=True) as m:
        corpus = m.upload(feats, off)
        states = aligned_states(corpus, auts, off)
        _, _, (beta, k, G) = corpus._mllr_args(spk, S, cls, N_CLASSES)
        call = lambda sp, n, c, r, b, kk, g: L.sr_mllr_statistics_corpus(m.h, corpus.h, P(states), P(sp), n, c, r, 1, b, kk, g)  # noqa: E731
        bad_spk, bad_cls = spk.copy(), cls.copy()
        bad_spk[2] = S
        bad_cls[0] = N_CLASSES
        assert call(bad_spk, S, P(cls), N_CLASSES, P(beta), P(k), P(G)) == -1
        assert call(spk, 0, P(cls), N_CLASSES, P(beta), P(k), P(G)) == -1
        assert call(spk, S, P(bad_cls), N_CLASSES, P(beta), P(k), P(G)) == -1
        assert call(spk, S, P(cls), 0, P(beta), P(k), P(G)) == -1
        assert call(spk, S, None, N_CLASSES, P(beta), P(k), P(G)) == -1
        assert call(spk, S, P(cls), N_CLASSES, None, P(k), P(G)) == -1
        assert call(spk, S, P(cls), N_CLASSES, P(beta), None, P(G)) == -1
        assert call(spk, S, P(cls), N_CLASSES, P(beta), P(k), None) == -1
        assert call(spk, 2_000_000_000, P(cls), N_CLASSES, P(beta), P(k), P(G)) == -4       # the outputs alone would take terabytes
        one = np.zeros_like(cls)   # a single class: what is refused is the (speaker, density) key range alone
        assert call(spk, 2 ** 32 // m.n_densities + 1, P(one), 1, P(beta), P(k), P(G)) == -4
        assert b"keys" in L.sr_last_error()
        assert not beta.any() and not k.any() and not G.any()
        t3 = (C.c_double * 3)(*TDP)
        flat, aoff = corpus._aut(auts)
        cost = np.zeros(len(auts))
        bw = lambda sp, n, c, r, b, floor=0.0: L.sr_mllr_statistics_bw_corpus(  # noqa: E731
            m.h, corpus.h, P(flat), P(aoff), C.byref(t3), 0, capi.GMM_DEFAULT, floor, P(sp), n, c, r, 1, P(cost), b, P(k), P(G))
        assert bw(bad_spk, S, P(cls), N_CLASSES, P(beta)) == -1 and bw(spk, 0, P(cls), N_CLASSES, P(beta)) == -1
        assert bw(spk, S, P(bad_cls), N_CLASSES, P(beta)) == -1 and bw(spk, S, P(cls), 0, P(beta)) == -1
        assert bw(spk, S, P(cls), N_CLASSES, None) == -1 and bw(spk, S, P(cls), N_CLASSES, P(beta), -1.0) == -1
        assert bw(spk, 2_000_000_000, P(cls), N_CLASSES, P(beta)) == -4
        bad_states = states.copy()
        bad_states[0] = 60000
        assert L.sr_mllr_statistics_corpus(m.h, corpus.h, P(bad_states), P(spk), S, P(cls), N_CLASSES, 1, P(beta), P(k), P(G)) == -1
        corpus.close()
    wide = F.random_model(np.random.default_rng(1), 3, 2, 64)
    with capi.Model.from_tables(*wide, max_approx=True) as m:
        corpus = m.upload(np.zeros((4, 64), np.float32), np.array([0, 4], np.uint64))
        sp, c1 = np.zeros(1, np.uint32), np.zeros(m.n_densities, np.uint32)
        b, kk, g = np.zeros((1, 1)), np.zeros((1, 1, 64, 65)), np.zeros((1, 1, 64, 65, 65))
        st = np.zeros(4, np.uint16)
        assert L.sr_mllr_statistics_corpus(m.h, corpus.h, P(st), P(sp), 1, P(c1), 1, 1, P(b), P(kk), P(g)) == -4
        out, W = C.c_void_p(), R.identity(64, 1)
        assert L.sr_model_transform_means(m.h, P(c1), 1, P(W), C.byref(out)) == -4 and not out.value
        corpus.close()


def shifted_case():
    """12 mixtures x 4 densities, D = 5; two classes, the first four mixtures (16 densities) and the rest: every class holds more than
    D + 1 densities, which a positive definite G_i needs; a mean shift planted per speaker and class"""
    D, S, n_states = 5, 3, 12
    rng = np.random.default_rng(91)
    model = F.random_model(rng, n_states, 4, D, ragged=False)
    cls = (state_classes(model[0], 4) // 2).astype(np.uint32)
    shift = rng.normal(0.0, 0.8, size=(S, 2, D))
    n_utts = 18
    T = rng.integers(40, 80, size=n_utts)
    off = np.concatenate([[0], np.cumsum(T)]).astype(np.uint64)
    spk = (np.arange(n_utts) % S).astype(np.uint32)
    feats, auts, planted = [], [], []
    for u in range(n_utts):
        N = int(rng.integers(3, 8))
        a = rng.integers(0, n_states, size=N).astype(np.uint16)
        auts.append(a)
        st = a[np.minimum(np.arange(T[u]) * N // T[u], N - 1)]
        d = np.array([rng.integers(model[0][k], model[0][k + 1]) for k in st])
        y = model[1][d] + shift[spk[u]][cls[d]] + rng.normal(size=(T[u], D)) / np.sqrt(model[2][d])
        feats.append(y.astype(np.float32))
        planted.append(st)
    return model, np.concatenate(feats), off, auts, spk, S, cls, np.concatenate(planted)


def test_adapted_models_lower_the_cost_of_the_alignment():
    """With the alignment and the arg-min densities fixed, the summed cost under the adapted model is the cost under m minus
    Q(W) - Q(I) >= 0 (W maximises Q); the adapted model's path scores re-pick the arg-min, which can only lower it further.  The margin
    is the rounding of the two sums: n_frames 2^-52 sum |scores|."""
    model, feats, off, auts, spk, S, cls, _ = shifted_case()
    o = off.astype(np.int64)
    with capi.Model.from_tables(*model, max_approx=True) as m:
        corpus = m.upload(feats, off)
        states, _ = corpus.align(auts, TDP, 0, capi.GMM_DEFAULT)
        beta, k, G = corpus.mllr_statistics(states, spk, S, cls, 2, True)
        corpus.close()
        W, node, aux = capi.mllr_estimate(beta, k, G)
        assert (node == np.arange(2)[None, :]).all() and (aux[:, :, 1] >= aux[:, :, 0]).all()
        for s in range(S):
            us = np.flatnonzero(spk == s)
            f = np.concatenate([feats[o[u]:o[u + 1]] for u in us])
            st = np.concatenate([states[o[u]:o[u + 1]] for u in us])
            po = np.concatenate([[0], np.cumsum([o[u + 1] - o[u] for u in us])]).astype(np.uint64)
            with m.transform_means(cls, W[s]) as adapted:
                c0, c1 = m.upload(f, po), adapted.upload(f, po)
                before, after = c0.path_scores(st), c1.path_scores(st)
                c0.close()
                c1.close()
            margin = len(st) * EPS * float(np.abs(before).sum() + np.abs(after).sum())
            gain = float((aux[s, :, 1] - aux[s, :, 0]).sum())
            print(f"speaker {s}: cost {before.sum():.3f} -> {after.sum():.3f}, Q gain {gain:.3f}, margin {margin:.3e}")
            assert after.sum() <= before.sum() + margin
