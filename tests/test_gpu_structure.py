"""sr_model_split, sr_model_eliminate and sr_model_tables on the device against the numpy restatement (tests/structure_reference.py),
and Trainer::train's schedule from one density per mixture to four.

Means of split children.  The kernel computes mean -+ epsilon * sqrt(1.0 / inv_var) in FP64 without contraction; the device's FP64
division and square root are correctly rounded (OpenCL's requirement for doubles, which the ROCm device library meets), as numpy's
are, so the means are asserted BIT-EQUAL rather than within the 2^-50 (|mean| + |delta|) the specification would allow.

Log weights of an eliminated model.  The library takes the host C library's log; the reference takes the same one (math.log) and the
two are compared bit for bit.  numpy's own vectorised log is within 1 ulp of the correctly rounded value like the C library's, so it
is compared too, within 2 ulp.

SR_ELIMIT (a split model of 2^31 densities or more) is not exercised: the parent alone would take 2^30 densities."""
import ctypes as C
import math
import os
import struct
import subprocess

import numpy as np
import pytest

from speechrecognition_amd import capi
from tests import structure_reference as R

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
COUNTS = [1, 2, 5, 31, 33, 0]      # 31 -> 62 and 33 -> 66 cross the 32-density route; the last mixture is empty
TDP = (3.0, 0.0, 30.0)


def u64(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def make_model(D, pooling, seed):
    """-> (dens_off, tables, (n_mean, n_var, dens_mean, dens_var), mean_w): random tables whose variances follow the pooling"""
    rng = np.random.default_rng(seed)
    off = np.concatenate([[0], np.cumsum(COUNTS)]).astype(np.uint32)
    Cn = int(off[-1])
    mix_of = np.repeat(np.arange(len(COUNTS)), COUNTS)
    dm = np.arange(Cn, dtype=np.uint32)
    dv = {R.POOL_NONE: dm.copy(), R.POOL_MIXTURE: mix_of.astype(np.uint32), R.POOL_GLOBAL: np.zeros(Cn, np.uint32)}[pooling]
    n_var = int(dv.max()) + 1
    var_rows = rng.uniform(0.3, 3.0, size=(n_var, D))
    means = 3.0 * rng.normal(size=(Cn, D))
    ivars = (1 / var_rows)[dv]
    norm = ((D * np.log(2 * np.pi) + np.log(var_rows).sum(axis=1)) / 2)[dv]
    w = rng.uniform(0.5, 30.0, size=Cn)
    logw = np.concatenate([np.log(w[a:b] / w[a:b].sum()) for a, b in zip(off[:-1], off[1:])])
    return off, (means, ivars, norm, logw), (Cn, n_var, dm, dv), w


def open_model(off, tables, tying, max_approx):
    m = capi.Model.from_tables(off, *tables, max_approx=max_approx)
    n_mean, n_var, dm, dv = tying
    capi._check(capi.lib().sr_model_set_tying(m.h, n_mean, n_var, dm.ctypes.data, dv.ctypes.data))
    return m


def features(D, seed, n=64):
    return (3.0 * np.random.default_rng(seed).normal(size=(n, D))).astype(np.float32), np.array([0, 40, n], dtype=np.uint64)


def check_against_plan(model, parents, plan, want_tables, label):
    off, dm, dv = model.topology()
    assert off.tolist() == plan["dens_off"].tolist(), label
    assert dm.tolist() == plan["dens_mean"].tolist() and dv.tolist() == plan["dens_var"].tolist(), label
    assert model.tying_info() == (plan["n_mean"], plan["n_var"]), label
    assert model.n_densities == len(plan["parent"]) and parents.tolist() == plan["parent"].tolist(), label
    got = model.tables()
    for name, g, w in zip(("means", "inv_vars", "norm", "logw"), got, want_tables):
        diff = int((u64(g) != u64(w)).sum())
        print(f"{label}: {name} differing elements {diff} of {g.size}")
        assert diff == 0, (label, name)
    return got


def rebuilt_scores_equal(model, feats, foff, max_approx):
    """a model made by sr_model_create + sr_model_set_tying from sr_model_tables scores bit-identically on every route"""
    off, dm, dv = model.topology()
    with open_model(off, model.tables(), model.tying_info() + (dm, dv), max_approx) as twin:
        a, b = model.upload(feats, foff), twin.upload(feats, foff)
        for kernel in (capi.GMM_DEFAULT, capi.GMM_MFMA, capi.GMM_EXACT):
            assert np.array_equal(u64(a.score(kernel)), u64(b.score(kernel))), kernel
        a.close()
        b.close()


@pytest.mark.parametrize("max_approx", [True, False])
@pytest.mark.parametrize("pooling", [R.POOL_NONE, R.POOL_MIXTURE, R.POOL_GLOBAL])
@pytest.mark.parametrize("D", [3, 39])
def test_split_and_eliminate_against_the_reference(D, pooling, max_approx):
    off, tables, tying, w = make_model(D, pooling, 10 * D + pooling)
    w[7] = np.nan                       # a density of the 5-mixture that neither splits nor survives
    n_mean, n_var, dm, dv = tying
    feats, foff = features(D, 5)
    min_obs, eps = 8.0, 0.2
    with open_model(off, tables, tying, max_approx) as m:
        child, par = m.split(w, min_obs, eps, pooling, parents=True)
        plan = R.split_plan(off, n_mean, n_var, dm, dv, w, min_obs, pooling)
        assert 0 < (plan["sign"] > 0).sum() < len(dm)          # some split, some do not
        want = R.split_tables(tables, plan, eps)
        got = check_against_plan(child, par, plan, want[:4], f"split D={D} pooling={pooling}")
        bound = 2.0 ** -50 * (np.abs(want[0]) + want[4])
        assert (np.abs(got[0] - want[0]) <= bound).all()
        again = m.split(w, min_obs, eps, pooling)
        for a, b in zip(got, again.tables()):
            assert np.array_equal(u64(a), u64(b)), "two identical calls differ"
        again.close()
        rebuilt_scores_equal(child, feats, foff, max_approx)
        child.close()

        gone, par = m.eliminate(w, min_obs, parents=True)
        plan = R.eliminate_plan(off, n_mean, n_var, dm, dv, w, min_obs)
        assert len(plan["parent"]) < len(dm) and plan["n_mean"] < n_mean
        want = R.eliminate_tables(tables, plan, dm, w)
        got = check_against_plan(gone, par, plan, want, f"eliminate D={D} pooling={pooling}")
        np_logw = R.eliminate_tables(tables, plan, dm, w, log=lambda q: float(np.log(np.float64(q))))[3]
        assert (np.abs(got[3] - np_logw) <= 2 * np.spacing(np.abs(np_logw))).all()
        rebuilt_scores_equal(gone, feats, foff, max_approx)
        gone.close()


@pytest.mark.parametrize("D", [3, 39])
def test_children_at_the_parents_place_cost_ln2_more(D):
    """epsilon = 0, min_obs = 0, max-approx: both children are the parent at half the weight"""
    off, tables, tying, w = make_model(D, R.POOL_NONE, 77 + D)
    feats, foff = features(D, 6)
    with open_model(off, tables, tying, True) as m:
        child = m.split(w, 0.0, 0.0)
        assert child.n_densities == 2 * m.n_densities
        a, b = m.upload(feats, foff), child.upload(feats, foff)
        filled = np.array(COUNTS) > 0        # an empty mixture has no children: its constant score stays
        for kernel in (capi.GMM_DEFAULT, capi.GMM_EXACT):
            p, c = a.score(kernel), b.score(kernel)
            assert np.array_equal(u64(p[:, ~filled]), u64(c[:, ~filled]))
            p, c = p[:, filled], c[:, filled]
            err = np.abs(c - (p + np.log(2.0)))
            lim = 4 * 2.0 ** -52 * (np.abs(c) + 1)
            print(f"D={D} kernel={kernel}: worst |child - (parent + ln 2)| / bound = {float((err / lim).max()):.3f}")
            assert (err <= lim).all()
        a.close()
        b.close()
        child.close()


def test_resident_statistics_give_the_same_bits_as_the_host_array():
    D = 39
    off, tables, tying, _ = make_model(D, R.POOL_MIXTURE, 21)
    feats, foff = features(D, 8)
    states = np.random.default_rng(2).choice(np.flatnonzero(np.array(COUNTS) > 0), size=len(feats)).astype(np.uint16)
    with open_model(off, tables, tying, True) as m:
        c = m.upload(feats, foff)
        mw = c.accumulate(states)[1]
        assert (mw >= 2.0).any() and (mw < 2.0).any()
        c.accumulate_on_device(states)
        pairs = [(m.split(mw, 2.0, 0.1, R.POOL_MIXTURE, parents=True), m.split(c, 2.0, 0.1, R.POOL_MIXTURE, parents=True)),
                 (m.eliminate(mw, 2.0, parents=True), m.eliminate(c, 2.0, parents=True))]
        for (a, pa), (b, pb) in pairs:
            assert pa.tolist() == pb.tolist()
            for x, y in zip(a.topology() + a.tables(), b.topology() + b.tables()):
                assert np.array_equal(x.view(np.uint8), y.view(np.uint8))
            a.close()
            b.close()
        c.close()


def test_a_starved_mixture_keeps_its_heaviest_density():
    D = 3
    off = np.array([0, 3, 5], dtype=np.uint32)
    rng = np.random.default_rng(4)
    tables = (rng.normal(size=(5, D)), rng.uniform(0.5, 2.0, size=(5, D)), rng.normal(size=5), np.log(np.full(5, 0.25)))
    w = np.array([0.5, 0.75, 0.75, 6.0, 2.0])          # mixture 0: three starved densities, a tie between 1 and 2
    with capi.Model.from_tables(off, *tables) as m:
        e, par = m.eliminate(w, 1.0, parents=True)
        assert par.tolist() == [1, 3, 4] and e.topology()[0].tolist() == [0, 1, 3]
        means, ivars, norm, logw = e.tables()
        for g, t in zip((means, ivars, norm), tables):
            assert np.array_equal(u64(g), u64(t[[1, 3, 4]]))           # gathered bit for bit
        assert logw.tolist() == [math.log(0.75 / 0.75), math.log(6.0 / 8.0), math.log(2.0 / 8.0)]
        assert e.tying_info() == (3, 3) and e.topology()[1].tolist() == [0, 1, 2]
        e.close()


def test_errors_are_refused_before_any_launch():
    D = 3
    off, tables, tying, w = make_model(D, R.POOL_NONE, 1)
    feats, foff = features(D, 3)
    L = capi.lib()
    P = lambda a: a.ctypes.data  # noqa: E731
    with open_model(off, tables, tying, True) as m, open_model(off, tables, tying, True) as other:
        c, foreign = m.upload(feats, foff), other.upload(feats, foff)
        out = C.c_void_p()

        def refused(rc, code=-1):
            assert rc == code and not out.value and L.sr_last_error()
            return True

        split = lambda cc, ww, mo, ep, po, o=C.byref(out): L.sr_model_split(m.h, cc, ww, mo, ep, po, o, None)  # noqa: E731
        elim = lambda cc, ww, mo, o=C.byref(out): L.sr_model_eliminate(m.h, cc, ww, mo, o, None)  # noqa: E731
        for bad in (-1.0, float("nan"), float("inf"), -float("inf")):
            assert refused(split(None, P(w), bad, 0.2, 2)) and refused(split(None, P(w), 1.0, bad, 2)) and refused(elim(None, P(w), bad))
        for po in (-1, 3):
            assert refused(split(None, P(w), 1.0, 0.2, po))
        assert refused(split(c.h, P(w), 1.0, 0.2, 2)) and refused(split(None, None, 1.0, 0.2, 2))         # both / neither
        assert refused(elim(c.h, P(w), 1.0)) and refused(elim(None, None, 1.0))
        assert refused(split(c.h, None, 1.0, 0.2, 2)) and refused(elim(c.h, None, 1.0))                   # no statistics in c yet
        assert refused(split(foreign.h, None, 1.0, 0.2, 2)) and refused(elim(foreign.h, None, 1.0))       # another model's corpus
        assert L.sr_model_split(None, None, P(w), 1.0, 0.2, 2, C.byref(out), None) == -1 and not out.value
        assert L.sr_model_eliminate(None, None, P(w), 1.0, C.byref(out), None) == -1 and not out.value
        assert L.sr_model_split(m.h, None, P(w), 1.0, 0.2, 2, None, None) == -1
        assert L.sr_model_eliminate(m.h, None, P(w), 1.0, None, None) == -1
        assert L.sr_model_tables(None, None, None, None, None) == -1
        assert L.sr_model_tables(m.h, None, None, None, None) == 0
        c.close()
        foreign.close()


# ---- training from scratch -------------------------------------------------------------------------------------------------------

SEED, MIN_OBS, EPSILON, NUM_SPLITS = 3, 40.0, 0.2, 2   # on the CPU alone (R.train_splits_cpu) this case goes 13.76 -> 12.16 per frame


def accumulate_and_finalize(m, feats, foff, states, first_pass, traj):
    """one accumulate / finalize on the device, both checked against the CPU pipeline started from m's own tables"""
    off, dm, dv = m.topology()
    n_mean, n_var = m.tying_info()
    c = m.upload(feats, foff)
    acc = c.accumulate(states, first_pass=first_pass, max_approx=True)
    c.close()
    want = R.accumulate(feats, states, off, dm, dv, n_mean, n_var, m.tables(), first_pass)
    for name, g, w in zip(("mean_acc", "mean_w", "var_acc", "var_w"), acc, want):
        assert np.array_equal(u64(g), u64(w)), name            # max-approx statistics: bit-equal
    nxt = capi.Model.from_statistics(m.dim, off, dm, dv, acc, R.POOL_NONE, True)
    for name, g, w in zip(("means", "inv_vars", "norm", "logw"), nxt.tables(), R.finalize(off, dm, dv, acc)):
        assert np.array_equal(u64(g), u64(w)), name
    c = nxt.upload(feats, foff)
    traj.append(float(np.add.accumulate(c.path_scores(states, capi.GMM_DEFAULT))[-1]) / len(feats))
    c.close()
    return nxt, acc[1]


def test_training_from_scratch_follows_the_cpu_pipeline(tmp_path):
    feats, foff, auts, orths, S = R.training_case(SEED)
    D = feats.shape[1]
    states = R.linear_segmentation(foff, auts)
    traj = []
    flat = capi.Model.from_tables(np.arange(S + 1, dtype=np.uint32), np.zeros((S, D)), np.ones((S, D)), np.zeros(S), np.zeros(S))
    m, mw = accumulate_and_finalize(flat, feats, foff, states, True, traj)
    flat.close()
    per_mixture = [np.diff(m.topology()[0].astype(np.int64))]
    for _ in range(NUM_SPLITS):
        for op in ("split", "eliminate"):
            off, dm, dv = m.topology()
            n_mean, n_var = m.tying_info()
            if op == "split":
                nxt, par = m.split(mw, MIN_OBS, EPSILON, R.POOL_NONE, parents=True)
                plan = R.split_plan(off, n_mean, n_var, dm, dv, mw, MIN_OBS, R.POOL_NONE)
                want = R.split_tables(m.tables(), plan, EPSILON)[:4]
            else:
                nxt, par = m.eliminate(mw, MIN_OBS, parents=True)
                plan = R.eliminate_plan(off, n_mean, n_var, dm, dv, mw, MIN_OBS)
                want = R.eliminate_tables(m.tables(), plan, dm, mw)
            check_against_plan(nxt, par, plan, want, op)
            m.close()
            m, mw = accumulate_and_finalize(nxt, feats, foff, states, False, traj)
            nxt.close()
            per_mixture.append(np.diff(m.topology()[0].astype(np.int64)))
    # 1 -> 2 -> 4 densities per mixture, minus what did not split or was eliminated
    assert per_mixture[0].tolist() == [1] * S
    assert per_mixture[1].max() == 2 and per_mixture[3].max() == 4
    assert (per_mixture[2] <= per_mixture[1]).all() and (per_mixture[4] <= per_mixture[3]).all() and (per_mixture[4] >= 1).all()
    after_splits = traj[-1]
    # one re-alignment round with one estimate
    c = m.upload(feats, foff)
    states2, _ = c.align(auts, TDP, 0, capi.GMM_DEFAULT)
    c.close()
    last, _ = accumulate_and_finalize(m, feats, foff, states2.copy(), False, traj)
    final_means = last.tables()[0]
    final_counts = np.diff(last.topology()[0].astype(np.int64))
    m.close()
    last.close()
    print("average AM score after every finalize:", [round(x, 4) for x in traj], "densities", final_counts.tolist())
    assert after_splits < traj[0] and traj[-1] < traj[0]

    # sr::Trainer::train through the C++ driver: the same trajectory, bit for bit
    blob = struct.pack("<I", 4) + struct.pack("<HH", 1, 1) + struct.pack("<HH", 3, 1) * 3
    blob += struct.pack("<Iddd", 0, *TDP) + struct.pack("<IIIdd", NUM_SPLITS, 1, 1, MIN_OBS, EPSILON) + struct.pack("<II", D, len(auts))
    o = foff.astype(np.int64)
    for u in range(len(auts)):
        blob += struct.pack("<I", len(orths[u])) + orths[u].astype(np.uint32).tobytes()
        blob += struct.pack("<I", int(o[u + 1] - o[u])) + feats[o[u]:o[u + 1]].tobytes()
    case = tmp_path / "case.bin"
    case.write_bytes(blob)
    drv = str(tmp_path / "structure_driver")
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-Wall", "-I" + os.path.join(ROOT, "include"),
                           os.path.join(ROOT, "tests", "cpp", "structure_driver.cpp"), "-o", drv,
                           "-L" + os.path.join(ROOT, "speechrecognition_amd"), "-lsrgpu",
                           "-Wl,-rpath," + os.path.join(ROOT, "speechrecognition_amd"), "-Wl,-rpath,/opt/rocm/lib"])
    out = subprocess.check_output([drv, str(case)], text=True).splitlines()
    assert not out[0].startswith("error"), out[0]
    scores = [int(ln.split()[1], 16) for ln in out if ln.startswith("score")]
    assert scores == u64(np.array(traj)).tolist()
    assert out[len(scores)].split()[1:] == [str(v) for v in final_counts]
    x = 0
    for b in u64(final_means).reshape(-1).tolist():
        x ^= b
        x = ((x << 1) | (x >> 63)) & 0xFFFFFFFFFFFFFFFF
    assert out[len(scores) + 1].split() == ["checksum", format(x, "x")]
