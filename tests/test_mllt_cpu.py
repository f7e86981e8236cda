"""MLLT without a GPU: the binding, sr_mllt_estimate (host code) on statistics made by the numpy restatement
(tests/mllt_reference.py) from random models and features, the code objects of mllt_stats.hip and the C++ mirror's compilation.

Rounding bounds.  u = 2^-53; every bound on Q is a multiple of 2^-52 = 2u times a sum of absolute values the reference computes.
This is test_fmllr_cpu.py's derivation with D in the place of E = D + 1 and without the linear term: Q(A) is a sum of D^3 + 1
products; an evaluation adds them in chains of at most D (a row of G_i times a_i) + D (that vector times a_i) + D (over the rows) + 3
operations, so it errs by at most (3D + 3) u times the sum of the terms' absolute values; log|det A| comes from D pivots of an
elimination whose entries carry up to D u relative error each, D^2 u absolute in the logarithm, times beta -- and beta D is the
quadratic terms' sum at any A the update leaves (a_i G_i a_i^T = beta exactly at a row's optimum), so at most D u of the same sum.
One evaluation: (4D + 3) u < 5 (D + 1) u; a comparison of two evaluations (the library's and the reference's, or two sweeps'):
10 (D + 1) u = 5 (D + 1) 2^-52.  The tests use test_fmllr_cpu.py's multiple, Q_MULT = 8 (D + 1)."""
import os
import re
import subprocess
import sys

import numpy as np
import pytest

from tests import fmllr_reference as RF
from tests import mllt_reference as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EPS = 2.0 ** -52
NEW = ["sr_mllt_statistics_corpus", "sr_mllt_statistics_bw_corpus", "sr_mllt_estimate"]
DIMS = [1, 2, 13, 39, 63]
# The stationarity test.  The row updates are a coordinate ascent that converges linearly; with 200 D frames behind the statistics
# the reference's own relative gradient falls by about a factor of 10 every 20 sweeps from 3e-2 after the first few, and is below
# GRAD_TOL = 1e-5 after SWEEPS = 100 for every D of the test -- which the test asserts on the reference before it looks at the library.
SWEEPS = 100
GRAD_TOL = 1e-5


def q_mult(D):
    return 8 * (D + 1)


@pytest.fixture(scope="module")
def capi():
    from speechrecognition_amd import build, capi
    build.build()
    return capi


def make_statistics(D, seed=0, frames=None):
    """random model; features drawn around its densities in the model's own basis, then features and means mixed by one random
    well-conditioned matrix while the model keeps its diagonal variances; hard pairs -> (beta, G) of the reference, added up
    over blocks of 2000 frames (the reference holds every z_j z_k of a block at once)"""
    rng = np.random.default_rng(1000 * D + seed)
    dens_off, means, inv_vars, norm, logw = RF.random_model(rng, 12, 3, D)
    frames = frames or max(60, 12 * (D + 1))
    M = np.eye(D) + 0.3 * rng.normal(size=(D, D)) / np.sqrt(D)
    model = (dens_off, means @ M.T, inv_vars, norm, logw)
    beta, G = 0.0, np.zeros((D, D, D))
    for f0 in range(0, frames, 2000):
        n = min(2000, frames - f0)
        d = rng.integers(0, len(means), size=n)
        y = means[d] + rng.normal(size=(n, D)) / np.sqrt(inv_vars[d])
        feats = (y @ M.T).astype(np.float32)
        b, g, _, _ = R.statistics(feats, model, [(t, int(d[t]), 1.0) for t in range(n)])
        beta, G = beta + b, G + g
    return beta, G


def bits(a):
    return np.ascontiguousarray(a).view(np.uint64)


def test_symbols_declared_exported_and_listed(capi):
    hdr = open(os.path.join(ROOT, "include", "srgpu.h")).read()
    declared = set(re.findall(r"SR_API\s+[\w\s\*]+?\b(sr_\w+)\s*\(", hdr))
    for name in NEW:
        assert name in declared, name
        assert name in capi.SYMBOLS, name
        assert hasattr(capi.lib(), name), name
    assert capi.lib().sr_abi_version() == 4 and capi.SR_ABI_VERSION == 4
    assert "#define SR_ABI_VERSION 4" in hdr


@pytest.mark.parametrize("D", DIMS)
def test_auxiliary_is_monotone_and_matches_the_reference(capi, D):
    beta, G = make_statistics(D)
    q0, mag0 = R.aux(beta, G, np.eye(D))
    for sweeps in (1, 2, 5):
        A, aux, logdet, status = capi.mllt_estimate(beta, G, n_sweeps=sweeps)
        assert status == 0
        q, mag = R.aux(beta, G, A)
        tol = q_mult(D) * EPS * mag
        print(f"D={D} sweeps={sweeps}: Q={q:.6f} lib-ref={aux[-1] - q:.3e} tol={tol:.3e} smallest step={np.diff(aux).min():.3e}")
        assert abs(aux[-1] - q) <= tol
        assert abs(aux[0] - q0) <= q_mult(D) * EPS * mag0
        for j in range(sweeps):
            assert aux[j + 1] >= aux[j] - q_mult(D) * EPS * max(mag, mag0)
        assert aux[-1] > aux[0]   # the fixture is mixed: there is something to gain
        sign, ld = np.linalg.slogdet(A)
        assert sign > 0           # the positive root at every row update
        # D pivots, each with up to D u relative error on either side
        assert abs(logdet - ld) <= 2 * D * D * EPS + EPS * abs(ld)
    # every sweep of one call against the sweeps of shorter calls: the same rows in the same order, the same bits
    A5, aux5, _, _ = capi.mllt_estimate(beta, G, n_sweeps=5)
    A2, aux2, _, _ = capi.mllt_estimate(beta, G, n_sweeps=2)
    assert np.array_equal(bits(aux5[:3]), bits(aux2))


@pytest.mark.parametrize("D", DIMS)
def test_rows_are_stationary_after_enough_sweeps(capi, D):
    """dQ/da_i = beta (A^-T)_i - a_i G_i.  At a fixed point of the sweep every row's gradient vanishes; a_i G_i a_i^T = beta there, so
    beta ||(A^-T)_i|| is the size of either term and the gradient is measured against it."""
    beta, G = make_statistics(D, seed=1, frames=200 * D)

    def worst(A):
        inv = np.linalg.inv(A)
        return max(np.linalg.norm(R.row_gradient(beta, G, A, i)) / (beta * np.linalg.norm(inv[:, i])) for i in range(D))

    Ar, _ = R.estimate(beta, G, SWEEPS)
    ref = worst(Ar)
    assert ref <= GRAD_TOL, f"the reference itself has not converged: {ref:.3e}"
    A, aux, _, status = capi.mllt_estimate(beta, G, n_sweeps=SWEEPS)
    assert status == 0
    got = worst(A)
    print(f"D={D}: relative gradient after {SWEEPS} sweeps: reference {ref:.3e}, library {got:.3e}")
    assert got <= GRAD_TOL
    assert np.linalg.det(A) > 0


def test_one_dimension_has_a_closed_form(capi):
    """D = 1: Q = beta log|a| - a^2 G / 2, maximal at a = +sqrt(beta / G); one sweep reaches it from any start, of either sign"""
    beta, G = make_statistics(1, seed=2)
    want = np.sqrt(beta / G[0, 0, 0])
    for start in (1.0, 0.3, -2.0):
        A, aux, logdet, status = capi.mllt_estimate(beta, G, n_sweeps=1, A=np.array([[start]]))
        assert status == 0
        assert abs(A[0, 0] - want) <= 4 * EPS * want   # a division, a square root, a product and the solve's two divisions
        assert abs(logdet - np.log(want)) <= 4 * EPS * max(1.0, abs(np.log(want)))
    A3, _, _, _ = capi.mllt_estimate(beta, G, n_sweeps=3)
    assert abs(A3[0, 0] - want) <= 4 * EPS * want


@pytest.mark.parametrize("D", [2, 13, 39])
def test_a_decorrelated_model_keeps_the_identity(capi, D):
    """G_i e_i = beta e_i for every i -- dimension i uncorrelated with the others under density weights 1/var_i, and of weighted
    variance 1, which is what the variance update of EM leaves on decorrelated data -- makes I a fixed point: p_i = e_i,
    G_i^-1 e_i = e_i / beta, alpha = beta.  The solve is a Cholesky solve with G_i: relative error at most D u cond(G_i) per entry."""
    rng = np.random.default_rng(50 + D)
    beta = 500.0
    G = np.empty((D, D, D))
    for i in range(D):
        B = rng.normal(size=(D, 3 * D))
        Gi = beta * (B @ B.T) / (3 * D)
        Gi[i, :] = 0.0
        Gi[:, i] = 0.0
        Gi[i, i] = beta
        G[i] = Gi
    A, aux, logdet, status = capi.mllt_estimate(beta, G, n_sweeps=3)
    assert status == 0
    kappa = max(np.linalg.cond(G[i]) for i in range(D))
    assert np.abs(A - np.eye(D)).max() <= 4 * D * EPS * kappa
    q0, mag0 = R.aux(beta, G, np.eye(D))
    assert np.abs(aux - q0).max() <= q_mult(D) * EPS * mag0
    assert abs(logdet) <= 2 * D * D * EPS


def test_status_cases_leave_the_matrix_as_given(capi):
    D = 5
    beta, G = make_statistics(D, seed=3)
    rng = np.random.default_rng(9)
    A0 = np.eye(D) + 0.01 * rng.normal(size=(D, D))
    q0, mag0 = R.aux(beta, G, A0)
    # too little data: left as given, bit for bit; out_aux holds Q of the A given at every sweep
    A, aux, logdet, status = capi.mllt_estimate(beta, G, n_sweeps=2, min_count=beta + 0.5, A=A0)
    assert status == 1 and np.array_equal(bits(A), bits(A0))
    assert np.abs(aux - q0).max() <= q_mult(D) * EPS * mag0 and len(set(bits(aux).tolist())) == 1
    assert abs(logdet - np.linalg.slogdet(A0)[1]) <= 2 * D * D * EPS
    A, _, _, status = capi.mllt_estimate(beta, G, n_sweeps=2, min_count=beta, A=A0)
    assert status == 0 and not np.array_equal(A, A0)
    # a G_i with a negative eigenvalue: restored
    Gs = G.copy()
    w, V = np.linalg.eigh(Gs[3])
    w[0] = -w[0]
    Gs[3] = (V * w) @ V.T
    Gs[3] = 0.5 * (Gs[3] + Gs[3].T)
    assert np.linalg.eigvalsh(Gs[3])[0] < 0
    A, aux, logdet, status = capi.mllt_estimate(beta, Gs, n_sweeps=2, A=A0)
    assert status == 2 and np.array_equal(bits(A), bits(A0))
    assert np.isfinite(aux).all() and len(set(bits(aux).tolist())) == 1   # Q of A0 exists even though no update does
    # a singular start: restored, and it has no Q
    As = A0.copy()
    As[2] = As[1]
    A, aux, logdet, status = capi.mllt_estimate(beta, G, n_sweeps=2, A=As)
    assert status == 2 and np.array_equal(bits(A), bits(As))
    assert np.isnan(aux).all() and np.isnan(logdet)


def test_argument_errors(capi):
    D = 4
    beta, G = make_statistics(D, seed=4)
    A0 = np.eye(D)
    A = A0.copy()
    st = np.zeros(1, np.int32)
    L = capi.lib()
    P = lambda a: None if a is None else a.ctypes.data  # noqa: E731

    def call(dim=D, g=G, sweeps=1, mc=0.0, a=A, status=st):
        return L.sr_mllt_estimate(dim, beta, P(g), sweeps, mc, P(a), None, None, P(status))

    assert call(dim=0) == -1
    assert call(g=None) == -1 and call(a=None) == -1 and call(status=None) == -1
    assert call(sweeps=0) == -1
    assert call(mc=-1.0) == -1 and call(mc=float("nan")) == -1
    assert np.array_equal(A, A0)
    assert b"sr_mllt_estimate" in L.sr_last_error()
    assert call() == 0 and st[0] == 0   # optional outputs may be NULL


def test_reference_row_update_agrees_with_the_library(capi):
    """the restatement's own update (numpy's inverse and solve) lands on the same matrix: a check of the reference, at the
    conditioning's level"""
    D = 6
    beta, G = make_statistics(D, seed=5)
    A, _, _, _ = capi.mllt_estimate(beta, G, n_sweeps=3)
    Ar, _ = R.estimate(beta, G, 3)
    kappa = max(np.linalg.cond(G[i]) for i in range(D))
    assert np.abs(A - Ar).max() <= 1e3 * D * EPS * kappa * np.abs(Ar).max()


def test_fmllr_estimate_keeps_its_bits(capi):
    """the Gauss-Jordan inverse moved to host_util.h unchanged: sr_fmllr_estimate on fixed integer-valued statistics gives the bits
    it gave before the move (recorded from the parent commit's library)"""
    D = 3
    beta = np.array([40.0])
    k = np.arange(D * (D + 1), dtype=np.float64).reshape(1, D, D + 1) - 4.0
    base = np.array([[9.0, 1.0, 2.0, 0.0], [1.0, 8.0, 1.0, 1.0], [2.0, 1.0, 7.0, 2.0], [0.0, 1.0, 2.0, 6.0]])
    G = np.stack([base * (10.0 + i) for i in range(D)])[None]
    W, aux, logdet, status = capi.fmllr_estimate(beta, k, G, n_sweeps=3)
    assert status.tolist() == [0]
    assert [format(int(b), "x") for b in bits(W).reshape(-1)] == FMLLR_BITS


FMLLR_BITS = ["bfe6b47e7eb31059", "bfa01136e20e2e9d", "3fcc007c5c6367fe", "bfb5987d445ab05e", "bfb87a2a6aa45866", "3fe608f1649d995f",
              "bfb379ff107707ec", "bfa680b2e24d271b", "3f8e7b77f0509fed", "3faff3b80f88051a", "3fe798e3f68b1fe0", "bfc459908242b8ee"]


def _isa():
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import isa_info
    return isa_info


def test_contraction_code_objects(capi, tmp_path):
    """mllt_contract_kernel<1..4> in the gfx950 code object of mllt_stats.hip: the FP64 matrix instruction, no scratch, no spills"""
    isa_info = _isa()
    if not os.path.exists(os.path.join(isa_info.LLVM, "llvm-objdump")):
        pytest.skip("no ROCm LLVM tools")
    co = isa_info.code_object("mllt_stats", str(tmp_path))
    meta, dis = isa_info.kernel_metadata(co), isa_info.disassembly(co)
    for rt in (1, 2, 3, 4):
        name = f"mllt_contract_kernel<{rt}>"
        assert name in meta, sorted(meta)
        k = meta[name]
        assert k["private_segment_fixed_size"] == 0 and k["vgpr_spill_count"] == 0 and k["sgpr_spill_count"] == 0, (name, k)
        n = sum("v_mfma_f64_16x16x4" in line for line in dis[name])
        assert n >= 2 * rt, (name, n)   # two column tiles per wave, rt row tiles each
    assert meta["mllt_reduce_kernel"]["private_segment_fixed_size"] == 0


def test_cpp_driver_compiles_and_estimates(capi, tmp_path):
    """tests/cpp/mllt_driver.cpp against the headers with -Wall; its host-only mode gives the binding's bits (its device mode runs in
    tests/test_gpu_mllt.py)"""
    import struct
    drv = str(tmp_path / "mllt_driver")
    p = subprocess.run(["g++", "-O2", "-std=c++17", "-Wall", "-Werror", "-I" + os.path.join(ROOT, "include"),
                        os.path.join(ROOT, "tests", "cpp", "mllt_driver.cpp"), "-o", drv,
                        "-L" + os.path.join(ROOT, "speechrecognition_amd"), "-lsrgpu",
                        "-Wl,-rpath," + os.path.join(ROOT, "speechrecognition_amd"), "-Wl,-rpath,/opt/rocm/lib"],
                       text=True, stdout=subprocess.PIPE, stderr=subprocess.STDOUT)
    assert p.returncode == 0, p.stdout[-3000:]
    D, sweeps = 4, 3
    beta, G = make_statistics(D, seed=6)
    f = tmp_path / "stats.bin"
    f.write_bytes(struct.pack("<IIdd", D, sweeps, 0.0, beta) + G.tobytes())
    out = subprocess.check_output([drv, "estimate", str(f)], text=True).splitlines()
    A, aux, logdet, status = capi.mllt_estimate(beta, G, n_sweeps=sweeps)
    head = out[0].split()
    assert head[:2] == ["status", "0"]
    assert int(head[3], 16) == int(bits(np.array([logdet]))[0]) and int(head[5], 16) == int(bits(aux[-1:])[0])
    got = np.array([int(x, 16) for x in out[1].split()[1:]], dtype=np.uint64)
    assert np.array_equal(got, bits(A).reshape(-1))
