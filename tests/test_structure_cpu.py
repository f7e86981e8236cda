"""The plan of sr_model_split / sr_model_eliminate without a GPU: tests/structure_reference.py pinned by hand-written cases, and
speechrecognition_amd/csrc/structure_plan.h -- compiled with the host compiler alone into tests/cpp/structure_plan_driver -- against
it, integer for integer."""
import math
import os
import struct
import subprocess

import numpy as np
import pytest

from tests import structure_reference as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAN = float("nan")

# four mixtures of 2, 1, 0 and 3 densities; mean row 1 is shared by density 1 of mixture 0 and the density of mixture 1
OFF = [0, 2, 3, 3, 6]
DM = [0, 1, 1, 2, 3, 4]
DV_NONE = [0, 1, 2, 3, 4, 5]          # one variance row per density
DV_MIX = [0, 0, 1, 2, 2, 2]           # one per mixture
W = [10.0, 5.0, 0.5, 3.0, NAN]


def eq(plan, **want):
    for k, v in want.items():
        got = plan[k]
        if isinstance(got, np.ndarray):
            assert got.tolist() == list(v), (k, got.tolist(), v)
        else:
            assert got == v, (k, got, v)


def test_split_by_hand_tied_row_nan_and_empty_mixture():
    p = R.split_plan(OFF, 5, 6, DM, DV_NONE, W, 4.0, R.POOL_NONE)
    eq(p, dens_off=[0, 4, 6, 6, 9], parent=[0, 1, 0, 1, 2, 2, 3, 4, 5], sign=[-1, -1, 1, 1, -1, 1, 0, 0, 0],
       dens_mean=[0, 1, 5, 6, 1, 7, 2, 3, 4], dens_var=[0, 1, 6, 7, 2, 8, 3, 4, 5], n_mean=8, n_var=9)


@pytest.mark.parametrize("pooling", [R.POOL_MIXTURE, R.POOL_GLOBAL])
def test_split_pooled_children_share_the_parents_variance_row(pooling):
    p = R.split_plan(OFF, 5, 3, DM, DV_MIX, W, 4.0, pooling)
    eq(p, dens_off=[0, 4, 6, 6, 9], parent=[0, 1, 0, 1, 2, 2, 3, 4, 5], dens_mean=[0, 1, 5, 6, 1, 7, 2, 3, 4],
       dens_var=[0, 0, 0, 0, 1, 1, 2, 2, 2], n_mean=8, n_var=3)


def test_nobody_splits_is_the_identity_plan():
    for min_obs in (1e300, 10.0 + 1e-9):   # the second: just above the largest weight
        p = R.split_plan(OFF, 5, 6, DM, DV_NONE, W, min_obs, R.POOL_NONE)
        eq(p, dens_off=OFF, parent=range(6), sign=[0] * 6, dens_mean=DM, dens_var=DV_NONE, n_mean=5, n_var=6)


def test_everybody_splits():
    p = R.split_plan(OFF, 5, 6, DM, DV_NONE, [10.0, 5.0, 0.5, 3.0, 0.0], 0.0, R.POOL_NONE)
    eq(p, dens_off=[0, 4, 6, 6, 12], parent=[0, 1, 0, 1, 2, 2, 3, 4, 5, 3, 4, 5], sign=[-1, -1, 1, 1, -1, 1, -1, -1, -1, 1, 1, 1],
       dens_mean=[0, 1, 5, 6, 1, 7, 2, 3, 4, 8, 9, 10], dens_var=[0, 1, 6, 7, 2, 8, 3, 4, 5, 9, 10, 11], n_mean=11, n_var=12)
    # a NaN weight does not split, not even at min_obs = 0
    p = R.split_plan(OFF, 5, 6, DM, DV_NONE, W, 0.0, R.POOL_NONE)
    assert p["sign"].tolist() == [-1, -1, 1, 1, -1, 1, -1, -1, 0, 1, 1]


def test_eliminate_by_hand_starved_mixture_and_renumbering():
    p = R.eliminate_plan(OFF, 5, 6, DM, DV_NONE, W, 4.0)
    # mixture 3 (0.5, 3, NaN) would lose everything: its heaviest, density 4, stays
    eq(p, dens_off=[0, 2, 3, 3, 4], parent=[0, 1, 2, 4], dens_mean=[0, 1, 1, 2], dens_var=[0, 1, 2, 3], n_mean=3, n_var=4,
       mean_map=[0, 1, -1, 2, -1], var_map=[0, 1, 2, -1, 3, -1])
    p = R.eliminate_plan(OFF, 5, 3, DM, DV_MIX, W, 4.0)
    eq(p, dens_var=[0, 0, 1, 2], n_var=3, var_map=[0, 1, 2])
    # the shared row 1 goes with both densities that reference it; mixture 1 keeps its only density anyway
    p = R.eliminate_plan(OFF, 5, 6, DM, DV_NONE, W, 6.0)
    eq(p, dens_off=[0, 1, 2, 2, 3], parent=[0, 2, 4], dens_mean=[0, 1, 2], mean_map=[0, 1, -1, 2, -1])


def test_eliminate_tie_on_the_heaviest_and_nan_weights():
    eq(R.eliminate_plan(OFF, 5, 6, DM, DV_NONE, [10.0, 5.0, 3.0, 3.0, 1.0], 4.0), parent=[0, 1, 2, 3])      # tie: the lowest index
    eq(R.eliminate_plan(OFF, 5, 6, DM, DV_NONE, [10.0, 5.0, NAN, 1.0, 1.0], 4.0), parent=[0, 1, 2, 4])      # NaN below everything
    eq(R.eliminate_plan(OFF, 5, 6, DM, DV_NONE, [10.0, 5.0, NAN, NAN, NAN], 4.0), parent=[0, 1, 2, 3])      # all NaN: the first
    eq(R.eliminate_plan(OFF, 5, 6, DM, DV_NONE, [NAN, NAN, NAN, NAN, 7.0], 4.0), parent=[0, 2, 5])          # NaN does not survive


def test_round_trip_identities():
    w = [10.0, 5.0, 0.5, 3.0, 0.0]
    p = R.eliminate_plan(OFF, 5, 6, DM, DV_NONE, w, 0.0)
    eq(p, dens_off=OFF, parent=range(6), dens_mean=DM, dens_var=DV_NONE, n_mean=5, n_var=6, mean_map=range(5), var_map=range(6))
    p = R.split_plan(OFF, 5, 6, DM, DV_NONE, w, math.nextafter(10.0, math.inf), R.POOL_NONE)
    eq(p, dens_off=OFF, parent=range(6), sign=[0] * 6, dens_mean=DM, dens_var=DV_NONE, n_mean=5, n_var=6)


def test_tables_by_hand():
    tables = (np.array([[2.0, -1.0], [7.0, 0.5]]), np.array([[4.0, 0.25], [1.0, 16.0]]), np.array([1.5, 2.5]), np.array([-0.5, -1.0]))
    plan = R.split_plan([0, 2], 2, 2, [0, 1], [0, 1], [9.0, 1.0], 2.0, R.POOL_NONE)
    means, ivars, norm, logw, delta = R.split_tables(tables, plan, 0.5)
    # density 0: sd = (0.5, 2), delta = (0.25, 1)
    assert means.tolist() == [[1.75, -2.0], [7.0, 0.5], [2.25, 0.0]]
    assert ivars.tolist() == [[4.0, 0.25], [1.0, 16.0], [4.0, 0.25]] and norm.tolist() == [1.5, 2.5, 1.5]
    assert logw.tolist() == [-0.5 - math.log(2.0), -1.0, -0.5 - math.log(2.0)]
    assert delta.tolist() == [[0.25, 1.0], [0.0, 0.0], [0.25, 1.0]]
    plan = R.eliminate_plan([0, 3], 3, 3, [0, 1, 2], [0, 1, 2], [3.0, 0.5, 1.0], 1.0)
    t3 = (np.array([[1.0], [2.0], [3.0]]), np.array([[1.0], [2.0], [4.0]]), np.array([0.1, 0.2, 0.3]), np.zeros(3))
    means, ivars, norm, logw = R.eliminate_tables(t3, plan, [0, 1, 2], [3.0, 0.5, 1.0])
    assert means.tolist() == [[1.0], [3.0]] and ivars.tolist() == [[1.0], [4.0]] and norm.tolist() == [0.1, 0.3]
    assert logw.tolist() == [math.log(0.75), math.log(0.25)]


# ---- the header against the reference --------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("plan") / "structure_plan_driver")
    subprocess.check_call(["g++", "-O1", "-std=c++17", "-Wall", "-Werror", "-I" + os.path.join(ROOT, "speechrecognition_amd", "csrc"),
                           os.path.join(ROOT, "tests", "cpp", "structure_plan_driver.cpp"), "-o", exe])
    return exe


def bits(x):
    return format(struct.unpack("<Q", struct.pack("<d", float(x)))[0], "x")


def run_driver(exe, tmp_path, op, off, n_mean, n_var, dm, dv, w, min_obs, pooling=R.POOL_NONE):
    toks = [op, len(off) - 1, n_mean, n_var, pooling, bits(min_obs)] + list(off) + list(dm) + list(dv) + [bits(v) for v in w]
    case = tmp_path / "case.txt"
    case.write_text(" ".join(str(t) for t in toks) + "\n")
    out = {}
    for ln in subprocess.check_output([exe, str(case)], text=True).splitlines():
        name, *vals = ln.split()
        out[name] = [int(v) for v in vals]
    return out


def same(got, plan, eliminate):
    assert got["n"] == [len(plan["parent"]), plan["n_mean"], plan["n_var"]]
    for k in ("dens_off", "parent", "sign", "dens_mean", "dens_var") + (("mean_map", "var_map") if eliminate else ()):
        assert got[k] == plan[k].tolist(), k


def hand_cases():
    ws = [W, [10.0, 5.0, 0.5, 3.0, 0.0], [10.0, 5.0, 3.0, 3.0, 1.0], [10.0, 5.0, NAN, NAN, NAN], [NAN, NAN, NAN, NAN, 7.0],
          [-math.inf, NAN, 0.0, NAN, -math.inf]]
    for w in ws:
        for min_obs in (0.0, 4.0, 6.0, math.nextafter(10.0, math.inf), 1e300):
            yield OFF, 5, 6, DM, DV_NONE, w, min_obs
            yield OFF, 5, 3, DM, DV_MIX, w, min_obs


def random_cases():
    rng = np.random.default_rng(5)
    for _ in range(40):
        S = int(rng.integers(1, 7))
        counts = rng.choice([0, 1, 2, 5, 33], size=S)
        off = np.concatenate([[0], np.cumsum(counts)])
        C = int(off[-1])
        n_mean, n_var = int(rng.integers(1, C + 2)), int(rng.integers(1, C + 2))
        dm, dv = rng.integers(0, n_mean, size=C), rng.integers(0, n_var, size=C)
        w = rng.choice([0.0, 1.0, 2.0, 2.0, 7.5, NAN], size=n_mean)
        yield off.tolist(), n_mean, n_var, dm.tolist(), dv.tolist(), w.tolist(), float(rng.choice([0.0, 1.0, 2.0, 3.0, 100.0]))


def test_header_plans_equal_the_reference(driver, tmp_path):
    n = 0
    for off, n_mean, n_var, dm, dv, w, min_obs in list(hand_cases()) + list(random_cases()):
        for pooling in (R.POOL_GLOBAL, R.POOL_MIXTURE, R.POOL_NONE):
            got = run_driver(driver, tmp_path, "split", off, n_mean, n_var, dm, dv, w, min_obs, pooling)
            same(got, R.split_plan(off, n_mean, n_var, dm, dv, w, min_obs, pooling), False)
        got = run_driver(driver, tmp_path, "eliminate", off, n_mean, n_var, dm, dv, w, min_obs)
        same(got, R.eliminate_plan(off, n_mean, n_var, dm, dv, w, min_obs), True)
        n += 1
    assert n == 100


def test_header_has_no_device_include():
    src = open(os.path.join(ROOT, "speechrecognition_amd", "csrc", "structure_plan.h")).read()
    assert "#include <hip" not in src and "handles.h" not in src
