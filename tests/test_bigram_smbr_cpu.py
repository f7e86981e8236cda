"""The bigram sMBR restatement (tests/bigram_smbr_reference.py) pinned by itself: path enumeration with every path's accuracy, finite
differences, identities against the bigram MMI restatement's free occupancies, the criterion on test_bigram_mmi_cpu's small sampled
task, and the header's declarations.  The GPU tests (tests/test_gpu_bigram_smbr.py) hold the library against the restatement."""
import os
import re

import numpy as np
import pytest

from tests import bigram_fb_reference as R
from tests import bigram_mmi_reference as BM
from tests import bigram_smbr_reference as BS
from tests import fb_reference as FB
from tests import mmi_reference as M
from tests import smbr_reference as SM
from tests.test_bigram_mmi_cpu import CRITERION_E, DIM, TDP, TINY, _tiny, criterion_task
from tests.test_mmi_cpu import _scores
from tests.test_smbr_cpu import criterion_refs

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
# test_one_ebw_step_raises_the_expected_accuracy: the smallest E of (1, 2, 4, 8) x CRITERION_E for which one EBW step raises
# sum_u Abar_u on criterion_task, found with the restatement alone; the GPU test takes its step at this E
BIGRAM_SMBR_E = 4 * CRITERION_E


def enumerate_accuracies(e, net, lm, tdp, ref, scale=1.0):
    """Every path of the free network with the mixtures it emits (bigram_mmi_reference.enumerate_paths' walk, path by path) ->
    (total mass, sum of mass * accuracy, per (t, k) the mass and the mass * accuracy of the paths whose frame t emits k [T, S] each)"""
    E = np.asarray(e, dtype=np.float64)
    T, S = E.shape
    W = net.W
    klm, td = R._klm(net, lm, scale), R._tdp(tdp, scale)
    tot = [0.0, 0.0]
    mass, macc = np.zeros((T, S)), np.zeros((T, S))

    def enter(x, c, t, emitted):
        p0 = int(net.first[x])
        step(p0, c, t, emitted)
        if net.slot_off[x + 1] - p0 >= 2:
            step(p0 + 1, c + td[int(net.slot_sil[x]), 2], t, emitted)

    def step(p, c, t, emitted):
        if not np.isfinite(c):
            return
        c = c + scale * E[t, net.state[p]]
        emitted = emitted + [int(net.state[p])]
        x, s = int(net.slot[p]), int(net.is_sil[p])
        if p == net.last[x]:
            end(x, c + td[s, 3], t + 1, emitted)
        if t + 1 == T:
            return
        for j in range(3):
            if net.k[p] + j < net.n[p]:
                step(p + j, c + td[s, j], t + 1, emitted)

    def end(x, c, t, emitted):
        if t == T:
            if np.isfinite(c):
                m = np.exp(-c)
                acc = sum(1 for tt, k in enumerate(emitted) if k == ref[tt])
                tot[0] += m
                tot[1] += m * acc
                for tt, k in enumerate(emitted):
                    mass[tt, k] += m
                    macc[tt, k] += m * acc
            return
        h = int(net.hist[x])
        for w in range(W):
            if w != net.sil and np.isfinite(klm[w, h]):
                enter(w, c + klm[w, h], t, emitted)
        if x == net.sil:
            enter(x, c, t, emitted)
        elif x < W:
            enter(x + W, c, t, emitted)

    end(net.sil, 0.0, 0, [])
    return tot[0], tot[1], mass, macc


@pytest.mark.parametrize("li", range(len(TINY)))
def test_restatement_is_path_enumeration(li):
    """Abar = sum P(pi) A(pi) and gamma_t(k) = sum over the paths emitting k at t of P(pi) (A(pi) - Abar), path by path; the walk's
    mass and emission counts are bigram_mmi_reference.enumerate_paths'.  One-state silence, a multi-state silence that is not word 0
    with ragged words, a shared mixture; NaN and +inf LM entries; references out of range"""
    net, lm, S, _ = _tiny(li)
    rng = np.random.default_rng(410 + li)
    for T in (1, 2, 4, 5):
        e = rng.uniform(0.0, 4.0, size=(T, S))
        ref = rng.integers(0, S + 1, size=T)  # S = out of range
        ref[0] = 65535 if T > 2 else ref[0]
        for scale in (0.4, 1.0, 2.5):
            total, tacc, mass, macc = enumerate_accuracies(e, net, lm, TDP, ref, scale)
            paths = BM.enumerate_paths(e, net, lm, TDP, scale)
            assert abs(total - sum(m for m, _ in paths.values())) <= 1e-12 * total
            assert np.abs(mass - sum(c for _, c in paths.values())).max() <= 1e-12 * total
            F, A, g = BS.smbr(e, net, lm, TDP, ref, scale)
            tol = 1e-12 * max(1, T)
            assert abs(F + np.log(total) / scale) <= 1e-12 * max(1.0, abs(F))
            assert abs(A - tacc / total) <= tol
            assert np.abs(g - (macc - mass * (tacc / total)) / total).max() <= tol
            assert 0.0 <= A <= T


@pytest.mark.parametrize("li", range(len(TINY)))
def test_gamma_is_the_gradient(li):
    """-kappa gamma_t(k) = d Abar / d e(t, k) by central differences; step and tolerance of test_bigram_mmi_cpu's occupancy check"""
    net, lm, S, _ = _tiny(li)
    rng = np.random.default_rng(420 + li)
    T, h = 7, 1e-5
    e = rng.uniform(0.0, 4.0, size=(T, S))
    ref = rng.integers(0, S, size=T)
    ref[3] = S + 2
    for scale in (0.4, 1.0):
        _, _, g = BS.smbr(e, net, lm, TDP, ref, scale)
        for t in range(T):
            for k in range(S):
                d = np.zeros_like(e)
                d[t, k] = h
                fd = (BS.smbr(e + d, net, lm, TDP, ref, scale)[1] - BS.smbr(e - d, net, lm, TDP, ref, scale)[1]) / (2 * h)
                assert abs(fd + scale * g[t, k]) <= 1e-8, (t, k, fd, g[t, k])


@pytest.mark.parametrize("li", range(len(TINY)))
def test_identities(li):
    """sum_k gamma_t(k) = 0; Abar = sum_t occ_t(ref_t) with the bigram MMI restatement's free occupancies; F is its F; references
    out of range everywhere give Abar = 0 and gamma = 0; constant references k = 0 .. S - 1 give accuracies that sum to T; no
    frames: F = 0, Abar = 0; no path: F = +inf, Abar = 0"""
    net, lm, S, _ = _tiny(li)
    rng = np.random.default_rng(430 + li)
    for T in (1, 3, 12):
        e = rng.uniform(0.0, 4.0, size=(T, S))
        ref = rng.integers(0, S, size=T)
        ref[T // 2] = S + 3
        for scale in (1.0, 0.3):
            F, A, g = BS.smbr(e, net, lm, TDP, ref, scale)
            Fo, occ = BM.free_occupancies(e, net, lm, TDP, scale)
            assert abs(F - Fo) <= 1e-12 * max(1.0, abs(Fo))
            assert np.abs(g.sum(axis=1)).max() <= 1e-12 * T
            assert abs(A - sum(occ[t, ref[t]] for t in range(T) if ref[t] < S)) <= 1e-12 * T
            F0, A0, g0 = BS.smbr(e, net, lm, TDP, np.full(T, S), scale)
            assert A0 == 0.0 and not g0.any() and F0 == F
            assert abs(sum(BS.smbr(e, net, lm, TDP, np.full(T, k), scale)[1] for k in range(S)) - T) <= 1e-12 * T
    F, A, g = BS.smbr(np.zeros((0, S)), net, lm, TDP, [], 1.0)
    assert (F, A) == (0.0, 0.0) and g.shape == (0, S)
    e = np.full((3, S), np.inf)
    F, A, g = BS.smbr(e, net, lm, TDP, [0, 0, 0], 1.0)
    assert F == np.inf and A == 0.0 and not g.any()


def _accuracy_and_statistics(net, lm, tdp, feats, off, refs, scale, tb, means, inv_vars, norm):
    items, total = [[], []], 0.0
    e_all = _scores(feats, means, inv_vars, norm, tb["logw"], tb["mix_off"])
    for u in range(len(off) - 1):
        a, b = int(off[u]), int(off[u + 1])
        _, A, g = BS.smbr(e_all[a:b], net, lm, tdp, refs[a:b], scale)
        total += A
        items[0] += SM.signed_items(g, +1)
        items[1] += SM.signed_items(g, -1)
    tables = dict(tb, means=means, vars_inv=inv_vars, norm=norm)
    C_ = len(means)
    return total, [FB.accumulate(feats, it, tables, C_, C_, False, True) for it in items]


def test_one_ebw_step_raises_the_expected_accuracy(tmp_path, oracle_lib):
    """test_bigram_mmi_cpu.criterion_task under the restatement alone, references = the oracle's alignment to the transcripts:
    sum_u Abar_u = 83.36 of 152 frames before the step; after one EBW step from the sMBR statistics (tau = 0, var_floor = 1e-3)
    64.33 at E = 8 = CRITERION_E, 67.51 at E = 16, 84.22 at E = 32, 95.31 at E = 64.  The smallest E of the doubling sequence
    from CRITERION_E that raises it, 32, is BIGRAM_SMBR_E: the GPU test takes its step there."""
    lex, mp, word_off, mixtures, lm, tdp, feats, off, trans, scale = criterion_task(tmp_path)
    o = oracle_lib.Oracle(mp, DIM, lex)
    tb = o.tables()
    refs = criterion_refs(o, lex, feats, off, trans)
    o.close()
    net = R.Net(word_off, mixtures, lex.silence_idx)
    acc0, (num, den) = _accuracy_and_statistics(net, lm, tdp, feats, off, refs, scale, tb, tb["means"], tb["vars_inv"], tb["norm"])
    assert abs(num[1].sum() - den[1].sum()) <= 1e-9 * num[1].sum()
    raised = {}
    for E in (CRITERION_E, 2 * CRITERION_E, 4 * CRITERION_E, 8 * CRITERION_E):
        means, var = M.ebw_update(tb["means"], tb["vars_inv"], (num[0], num[1], num[2]), (den[0], den[1], den[2]), E, 0.0, 1e-3)
        norm = (DIM * np.log(2 * np.pi) + np.log(var).sum(axis=1)) / 2
        raised[E] = _accuracy_and_statistics(net, lm, tdp, feats, off, refs, scale, tb, means, 1.0 / var, norm)[0]
        print("E", E, len(feats), acc0, raised[E])
    assert min(E for E, a in raised.items() if a > acc0) == BIGRAM_SMBR_E


def test_header_declares_the_entry_points():
    """include/srgpu.h declares the two entry points with the issue's signatures and SR_ABI_VERSION stays 4; the binding lists them"""
    with open(os.path.join(ROOT, "include", "srgpu.h")) as f:
        h = f.read()
    flat = re.sub(r"\s+", " ", h)
    assert re.search(r"#define SR_ABI_VERSION 4\b", h)
    assert ("SR_API int sr_bigram_accuracies_corpus(sr_model* m, sr_corpus* c, sr_bigram* b, int gmm_kernel, double scale, "
            "double posterior_floor, uint32_t max_items, const uint16_t* ref_states, double* out_cost, double* out_acc, "
            "uint16_t* out_count, uint16_t* out_state, double* out_weight);") in flat
    assert ("SR_API int sr_bigram_smbr_statistics_corpus(sr_model* m, sr_corpus* c, sr_bigram* b, int gmm_kernel, double scale, "
            "double posterior_floor, int max_approx, const uint16_t* ref_states, double* out_cost, double* out_acc, "
            "double* num_mean_acc, double* num_mean_w, double* num_var_acc, double* num_var_w, double* den_mean_acc, "
            "double* den_mean_w, double* den_var_acc, double* den_var_w);") in flat
    from speechrecognition_amd import capi
    assert capi.SR_ABI_VERSION == 4
    assert {"sr_bigram_accuracies_corpus", "sr_bigram_smbr_statistics_corpus"} <= set(capi.SYMBOLS)


def test_kernels_have_no_scratch():
    """the gfx950 code objects of viterbi_bigram_smbr.hip: no private segment and no vector spills in its two step kernels (scalar
    spills go to VGPR lanes), within the 128 VGPRs their 512 threads assume; the kernels of the item path
    (posterior_items.hip) likewise"""
    import sys
    import tempfile
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import isa_info
    if not os.path.exists(os.path.join(isa_info.LLVM, "llvm-objdump")):
        pytest.skip("no ROCm LLVM tools")
    from speechrecognition_amd import build
    build.build()
    with tempfile.TemporaryDirectory() as tmp:
        md = isa_info.kernel_metadata(isa_info.code_object("viterbi_bigram_smbr", tmp))
        items = isa_info.kernel_metadata(isa_info.code_object("posterior_items", tmp))
    mine = {k: v for k, v in md.items() if k.startswith("bgsmbr_")}
    assert set(mine) == {"bgsmbr_forward_kernel", "bgsmbr_backward_kernel"}
    mine.update({k: v for k, v in items.items() if k.startswith("items_")})
    assert {"items_kernel<false, unsigned short>", "items_kernel<true, unsigned short>", "items_kernel<false, unsigned int>",
            "items_kernel<true, unsigned int>", "items_advance_kernel", "items_top_kernel"} <= set(mine)
    for k, v in mine.items():
        print(k, v)
        assert v["private_segment_fixed_size"] == 0 and v["vgpr_spill_count"] == 0 and v["vgpr_count"] <= 128, (k, v)
