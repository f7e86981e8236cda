"""LDA with frame splicing on the device (sr_lda_statistics_corpus, sr_corpus_splice_transform; sr_lda_estimate between them)
against the numpy restatement tests/lda_reference.py.

Statistics bound.  u = 2^-53.  Every term of a sum is exact in FP64: a float widened to double (class sums) or the product of two
such (24 + 24 significant bits; the scatter).  The device and the reference add the same n terms, each in its own order, so each errs
by at most (n - 1) u sum|terms| (1 + O(n u)) and they differ by at most (n - 1) 2^-52 sum|terms|.  As in tests/test_gpu_mllt.py the
tests take (n + 32) 2^-52 times the reference's sum of absolute values, n the items of the class for a class sum and all items for
the scatter.  The projection is compared bit for bit: the order of its operations is specified."""
import ctypes as C
import os
import struct
import subprocess

import numpy as np
import pytest

from speechrecognition_amd import capi
from tests import fmllr_reference as RF
from tests import lda_reference as R

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EPS = 2.0 ** -52
C_TERM = 32
S = 10
SEG = 1024
CASES = [(5, 1), (13, 4), (25, 4), (39, 2), (25, 0), (64, 3), (39, 6), (160, 1)]
# states 0 and 1 merged into class 0 (class 1 stays empty), state 2 skipped
MERGED = np.array([0, 0, R.SKIP, 3, 4, 5, 6, 7, 8, 9], dtype=np.uint32)


def u64(a):
    return np.ascontiguousarray(a).view(np.uint64)


def make_corpus(D, seed, n_utts=72):
    """about 60 frames an utterance, about 4000 in all; the last one has one frame, the third two; states in runs of about 10 frames, every state
    with its own mean"""
    rng = np.random.default_rng(seed)
    T = rng.integers(30, 90, size=n_utts)
    T[-1] = 1
    T[2] = 2
    off = np.concatenate([[0], np.cumsum(T)]).astype(np.uint64)
    means = 2 * rng.normal(size=(S, D))
    states = np.concatenate([np.repeat(rng.integers(0, S, size=(t + 9) // 10), 10)[:t] for t in T]).astype(np.uint16)
    states[: S] = np.arange(S)   # every state has a frame
    feats = (means[states] + rng.normal(size=(len(states), D))).astype(np.float32)
    return feats, off, states


def placeholder(D, n_states=S):
    """a model that only holds a corpus: one density per state, any finite tables"""
    return capi.Model.from_tables(np.arange(n_states + 1, dtype=np.uint32), np.zeros((n_states, D)), np.ones((n_states, D)),
                                  np.zeros(n_states), np.zeros(n_states))


def check_stats(got, ref, label):
    count, total, scatter = got
    rcount, rtotal, rscatter, tabs, sabs = ref
    assert np.array_equal(count, rcount), label
    n = rcount.sum()
    worst = 0.0
    for name, a, b, lim in (("sum", total, rtotal, (rcount[:, None] + C_TERM) * EPS * tabs), ("scatter", scatter, rscatter, (n + C_TERM) * EPS * sabs)):
        err = np.abs(a - b)
        ratio = float((err / np.where(lim > 0, lim, 1.0)).max())
        worst = max(worst, ratio)
        assert (err <= lim).all(), (label, name, ratio)
    assert np.array_equal(u64(scatter), u64(scatter.T)), (label, "scatter not exactly symmetric")
    for k in np.flatnonzero(rcount == 0):
        assert not total[k].any(), (label, "empty class", k)
    print(f"{label}: worst |gpu - ref| / bound = {worst:.3f}, items {int(n)}")


@pytest.mark.parametrize("D,context", CASES)
def test_statistics_match_the_reference(D, context):
    feats, off, states = make_corpus(D, 100 + D + context)
    with placeholder(D) as m:
        corpus = m.upload(feats, off)
        for label, cls in (("identity", None), ("merged", MERGED)):
            ref = R.statistics(feats, off, states, context, cls, S)
            assert ref[0].sum() > 3 * SEG   # more than three segments
            got = corpus.lda_statistics(states, context, cls, S)
            check_stats(got, ref, f"D={D} c={context} {label}")
            again = corpus.lda_statistics(states, context, cls, S)
            for a, b in zip(got, again):
                assert np.array_equal(u64(a), u64(b)), (label, "two identical calls differ")
            if cls is not None:
                assert got[0][1] == 0 and got[0][2] == 0 and got[0][0] == ref[0][0] > 0
        corpus.close()


def test_workspace_rounds_keep_the_bits(monkeypatch):
    """E = 225: a segment's partials are 10 blocks of 32 KiB, so 1 MiB holds three of the eight segments"""
    D, context = 25, 4
    feats, off, states = make_corpus(D, 7, n_utts=120)
    assert len(states) > 6 * SEG
    with placeholder(D) as m:
        corpus = m.upload(feats, off)
        whole = corpus.lda_statistics(states, context, None, S)
        corpus.close()
    monkeypatch.setenv("SRGPU_LDA_MB", "1")
    with placeholder(D) as m:
        corpus = m.upload(feats, off)
        rounds = corpus.lda_statistics(states, context, None, S)
        corpus.close()
    for a, b in zip(whole, rounds):
        assert np.array_equal(u64(a), u64(b))
    check_stats(rounds, R.statistics(feats, off, states, context, None, S), "rounds")


def test_workspace_below_one_segment_runs_segment_by_segment(monkeypatch):
    """E = 507: a segment's partials are 36 blocks of 32 KiB, more than the 1 MiB asked for; a round then holds one segment"""
    D, context = 39, 6
    feats, off, states = make_corpus(D, 100 + D + context)
    with placeholder(D) as m:
        corpus = m.upload(feats, off)
        whole = corpus.lda_statistics(states, context, None, S)
        corpus.close()
    monkeypatch.setenv("SRGPU_LDA_MB", "1")
    with placeholder(D) as m:
        corpus = m.upload(feats, off)
        rounds = corpus.lda_statistics(states, context, None, S)
        corpus.close()
    for a, b in zip(whole, rounds):
        assert np.array_equal(u64(a), u64(b))


def test_more_classes_than_a_grid_dimension():
    """70 000 classes, all but ten empty: the same sums in the first ten rows, zeros below"""
    D, context, K = 13, 1, 70000
    feats, off, states = make_corpus(D, 14)
    with placeholder(D) as m:
        corpus = m.upload(feats, off)
        few = corpus.lda_statistics(states, context, None, S)
        many = corpus.lda_statistics(states, context, None, K)
        corpus.close()
    assert many[1].shape == (K, 3 * D)
    assert np.array_equal(u64(many[0][:S]), u64(few[0])) and np.array_equal(u64(many[1][:S]), u64(few[1]))
    assert np.array_equal(u64(many[2]), u64(few[2]))
    assert not many[0][S:].any() and not many[1][S:].any()


def test_shards_add_up():
    D, context = 13, 4
    feats, off, states = make_corpus(D, 8)
    ref = R.statistics(feats, off, states, context, MERGED, S)
    h = 37
    cut = int(off[h])
    with placeholder(D) as m:
        a = m.upload(feats[:cut], off[: h + 1])
        b = m.upload(feats[cut:], off[h:] - off[h])
        sa = a.lda_statistics(states[:cut], context, MERGED, S)
        sb = b.lda_statistics(states[cut:], context, MERGED, S)
        a.close()
        b.close()
    check_stats(tuple(x + y for x, y in zip(sa, sb)), ref, "two shards")


def test_all_frames_skipped_gives_zeros():
    D, context = 13, 2
    feats, off, states = make_corpus(D, 9)
    with placeholder(D) as m:
        corpus = m.upload(feats, off)
        got = corpus.lda_statistics(states, context, np.full(S, R.SKIP, dtype=np.uint32), 3)
        corpus.close()
    assert all(not x.any() for x in got) and got[1].shape == (3, 5 * D)


def test_errors_come_before_any_launch():
    D, context = 13, 1
    E = 3 * D
    feats, off, states = make_corpus(D, 10)
    L = capi.lib()
    P = lambda a: None if a is None else a.ctypes.data  # noqa: E731
    with placeholder(D) as m, placeholder(D) as other:
        corpus = m.upload(feats, off)
        count, total, scatter = np.full(S, 7.5), np.full((S, E), 7.5), np.full((E, E), 7.5)

        def call(model=m, st=states, ctx=context, cls=None, K=S, c=count, t=total, s=scatter):
            return L.sr_lda_statistics_corpus(model.h, corpus.h, P(st), ctx, P(cls), K, P(c), P(t), P(s))

        def refused(code, **kw):
            """the call fails with `code` and leaves all three outputs as they were"""
            assert call(**kw) == code, kw
            assert (count == 7.5).all() and (total == 7.5).all() and (scatter == 7.5).all(), kw

        refused(-1, c=None)
        refused(-1, t=None)
        refused(-1, s=None)
        refused(-1, K=0)
        bad = states.copy()
        bad[len(bad) // 2] = S
        refused(-1, st=bad)                             # a state >= n_states, half-way through the corpus
        refused(-1, K=S - 1)                            # identity map: state 9 is class 9
        cls = MERGED.copy()
        cls[4] = S
        refused(-1, cls=cls)                            # a class that is neither < n_classes nor SR_LDA_SKIP
        refused(-4, ctx=20)                             # E = 41 x 13 = 533
        assert b"512" in L.sr_last_error()
        refused(-4, K=2 ** 31, cls=MERGED)              # 8 x 2^31 x 39 bytes of class sums: beyond a quarter of any device
        assert b"quarter" in L.sr_last_error()
        refused(-1, model=other)                        # a corpus of another model
        # the same arguments without a fault go through (on arrays of their own)
        assert call(cls=MERGED, c=np.zeros(S), t=np.zeros((S, E)), s=np.zeros((E, E))) == 0
        # the projection's
        M = np.zeros((D, E + 1))
        out = C.c_void_p()
        assert L.sr_corpus_splice_transform(m.h, corpus.h, other.h, context, None, C.byref(out)) == -1 and not out.value
        assert L.sr_corpus_splice_transform(m.h, corpus.h, None, context, P(M), C.byref(out)) == -1 and not out.value
        assert L.sr_corpus_splice_transform(m.h, corpus.h, other.h, context, P(M), None) == -1
        assert L.sr_corpus_splice_transform(m.h, corpus.h, other.h, 20, P(M), C.byref(out)) == -4 and not out.value
        assert L.sr_corpus_splice_transform(other.h, corpus.h, other.h, context, P(M), C.byref(out)) == -1 and not out.value
        if capi.device_count() > 1:
            with capi.Model.from_tables(np.arange(S + 1, dtype=np.uint32), np.zeros((S, D)), np.ones((S, D)), np.zeros(S), np.zeros(S),
                                        device=1) as far:
                assert L.sr_corpus_splice_transform(m.h, corpus.h, far.h, context, P(M), C.byref(out)) == -1 and not out.value
        corpus.close()


@pytest.mark.parametrize("D,context,p,kind", [(13, 4, 40, "lda"), (25, 4, 40, "lda"), (5, 1, 7, "lda"), (64, 3, 63, "lda"),
                                              (25, 4, 160, "random"), (25, 0, 25, "identity")])
def test_projection_is_the_documented_loop(D, context, p, kind):
    """the projected corpus, seen through the exact scores of a random model of dimension p, against the reference's rows uploaded to
    the same model (how tests/test_gpu_fmllr.py reads sr_corpus_transform's result): the same bits in, the same bits out"""
    feats, off, states = make_corpus(D, 200 + D + p)
    E = (2 * context + 1) * D
    rng = np.random.default_rng(p)
    if kind == "lda":
        count, total, scatter, _, _ = R.statistics(feats, off, states, context, None, S)
        M, _, status = capi.lda_estimate(count, total, scatter, p, remove_mean=True)
        assert status == 0
    elif kind == "random":
        M = rng.normal(size=(p, E + 1)) / np.sqrt(E)
    else:
        M = np.hstack([np.eye(D), np.zeros((D, 1))])
    want = R.project(feats, off, context, M)
    with placeholder(D) as m, capi.Model.from_tables(*RF.random_model(rng, 6, 3, p)) as target:
        corpus = m.upload(feats, off)
        proj = corpus.splice_transform(target, context, M)
        host = target.upload(want, off)
        a, b = proj.score(capi.GMM_EXACT), host.score(capi.GMM_EXACT)
        assert np.array_equal(u64(a), u64(b))
        assert len(np.unique(u64(a))) > a.size // 2      # the scores do tell rows apart
        if kind == "identity":                           # 0 + 1 x + zeros: the input itself
            assert np.array_equal(want.view(np.uint32), feats.view(np.uint32))
        # the original corpus is still valid
        assert np.array_equal(corpus.lda_statistics(states, 0, None, S)[0], np.bincount(states, minlength=S))
        for c in (host, proj, corpus):
            c.close()


def test_closed_loop_statistics_of_the_projected_corpus():
    """statistics -> estimate -> projected corpus -> its statistics with context 0, against the reference's statistics of the
    reference's projection with the same M: the corpora are bit-equal (test above), so only the summation differs.

    Separately, on the reference alone (a guard of the test's inputs, not of the device): the within-class covariance of the
    projected float features is I and the between-class one diag(eig), up to the features' rounding to float.  A feature y carries a
    relative error of at most 2^-24, so an entry of either covariance moves by at most 2 x 2^-24 x mean|y_i||y_j| <= 2^-23 x
    sqrt(T_ii T_jj) with T = W + B the total covariance, at most 1 + eig[0]; measured on the CPU for this case: 8e-9 (within),
    4e-8 (between), 2e-9 (mean) -- the roundings average out over the frames; the bound taken is the worst case's, with a factor 4:
    4 x 2^-23 x (1 + eig[0]) = 1e-5."""
    D, context, p = 13, 4, 40
    feats, off, states = make_corpus(D, 11)
    with placeholder(D) as m, placeholder(p) as target:
        corpus = m.upload(feats, off)
        count, total, scatter = corpus.lda_statistics(states, context, MERGED, S)
        M, eig, status = capi.lda_estimate(count, total, scatter, p, remove_mean=True)
        assert status == 0
        proj = corpus.splice_transform(target, context, M)
        got = proj.lda_statistics(states, 0, MERGED, S)
        proj.close()
        corpus.close()
    y = R.project(feats, off, context, M)
    ref = R.statistics(y, off, states, 0, MERGED, S)
    check_stats(got, ref, "closed loop")
    W, B, mu = R.covariances(*ref[:3])
    tol = 4 * 2.0 ** -23 * (1 + eig[0])
    print(f"projected features: |W - I| {np.abs(W - np.eye(p)).max():.3e}, |B - diag| {np.abs(B - np.diag(eig[:p])).max():.3e}, "
          f"|mean| {np.abs(mu).max():.3e}, tol {tol:.3e}")
    assert np.abs(W - np.eye(p)).max() <= tol and np.abs(B - np.diag(eig[:p])).max() <= tol
    assert np.abs(mu).max() <= tol


def test_first_pass_model_of_the_projected_corpus():
    """a placeholder target holds the projected corpus; a first-pass accumulate and sr_model_create_from_accumulated give a model of
    dimension p whose means are the class means of the projected features: the first pass adds a state's rows in frame order
    (tests/test_gpu_structure.py holds its statistics to the bits), so bit for bit"""
    D, context, p = 13, 2, 20
    feats, off, states = make_corpus(D, 12)
    count, total, scatter, _, _ = R.statistics(feats, off, states, context, None, S)
    M, _, status = capi.lda_estimate(count, total, scatter, p, remove_mean=True)
    assert status == 0
    y = R.project(feats, off, context, M).astype(np.float64)
    with placeholder(D) as m, placeholder(p) as target:
        corpus = m.upload(feats, off)
        proj = corpus.splice_transform(target, context, M)
        proj.accumulate_on_device(states, first_pass=True)
        first = proj.next_model()
        assert first.dim == p and first.n_states == S
        means = first.tables()[0]
        first.close()
        proj.close()
        corpus.close()
    want = np.stack([np.add.accumulate(y[states == s], axis=0)[-1] / (states == s).sum() for s in range(S)])
    assert np.array_equal(u64(means), u64(want))


def test_cpp_helper_projects_and_trains(tmp_path):
    """tests/cpp/lda_driver.cpp (sr::Lda of include/sr_sietill.hpp) on a small blob corpus: M's bits are the Python path's"""
    D, context, p = 5, 1, 7
    feats, off, states = make_corpus(D, 13)
    drv = str(tmp_path / "lda_driver")
    r = subprocess.run(["g++", "-O2", "-std=c++17", "-Wall", "-Werror", "-I" + os.path.join(ROOT, "include"),
                        os.path.join(ROOT, "tests", "cpp", "lda_driver.cpp"), "-o", drv, "-L" + os.path.join(ROOT, "speechrecognition_amd"),
                        "-lsrgpu", "-Wl,-rpath," + os.path.join(ROOT, "speechrecognition_amd"), "-Wl,-rpath,/opt/rocm/lib"],
                       text=True, stdout=subprocess.PIPE, stderr=subprocess.STDOUT)
    assert r.returncode == 0, r.stdout[-3000:]
    blob = tmp_path / "corpus.bin"
    blob.write_bytes(struct.pack("<IIIII", D, S, len(off) - 1, context, p) + off.tobytes() + states.tobytes() + MERGED.tobytes() + feats.tobytes())
    out = subprocess.run([drv, "device", str(blob)], text=True, stdout=subprocess.PIPE, stderr=subprocess.STDOUT)
    assert out.returncode == 0, out.stdout[-3000:]
    lines = out.stdout.splitlines()
    with placeholder(D) as m:
        corpus = m.upload(feats, off)
        count, total, scatter = corpus.lda_statistics(states, context, MERGED, S)
        corpus.close()
    M, eig, status = capi.lda_estimate(count, total, scatter, p, remove_mean=True)
    head = lines[0].split()
    assert head[:2] == ["status", "0"] and head[2:4] == ["dim", str(p)]
    got = np.array([int(x, 16) for x in lines[1].split()[1:]], dtype=np.uint64)
    assert np.array_equal(got, u64(M).reshape(-1))
    # the target model's means, from one first-pass accumulate of the projected corpus: the skipped state and all
    y = R.project(feats, off, context, M).astype(np.float64)
    want = np.stack([np.add.accumulate(y[states == s], axis=0)[-1] / (states == s).sum() for s in range(S)])
    means = np.array([int(x, 16) for x in lines[2].split()[1:]], dtype=np.uint64)
    assert np.array_equal(means, u64(want).reshape(-1))
