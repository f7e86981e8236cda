"""The sMBR restatement (tests/smbr_reference.py) pinned by itself: path enumeration with every path's accuracy, finite
differences, identities against the MMI restatement's occupancies, and the criterion on test_mmi_cpu's small synthetic task.  The
GPU tests (tests/test_gpu_smbr.py) hold the library against the restatement."""
import numpy as np
import pytest

from tests import fb_reference as FB
from tests import mmi_reference as M
from tests import net_fb_reference as R
from tests import smbr_reference as SM
from tests.test_mmi_cpu import CRITERION_E, DIM, PEN, _scores, criterion_task
from tests.test_word_posteriors_cpu import _lex

# silence is word 0 (one position)
TINY = [[1, 2], [1, 3, 3, 2]]
# test_one_ebw_step_raises_the_expected_accuracy: the smallest E of (1, 2, 4, 8) x CRITERION_E for which one EBW step raises
# sum_u Abar_u on criterion_task, found with the restatement alone; the GPU test takes its step at this E
SMBR_E = 4 * CRITERION_E


def _net(lex):
    word_off, aut, sil_state = lex.flatten()
    return R.Net(word_off, aut, lex.silence_idx, sil_state)


def enumerate_accuracies(e, net, tdp, wp, ref, scale=1.0):
    """Every path of the free network with the states it emits -> (total mass, sum of mass * accuracy, per (t, k) the mass and the
    mass * accuracy of the paths whose frame t emits k [T, S] each)"""
    e = np.asarray(e, dtype=np.float64)
    T, S = e.shape
    gr = M.free_graph(net)
    into, ent = M._penalties(gr, tdp, wp, scale)
    tot = [0.0, 0.0]
    mass, macc = np.zeros((T, S)), np.zeros((T, S))

    def succ(s, t):
        em = scale * e[t]
        if gr.end[s]:  # a word end enters every word at position 0 or 1, emitting its first state
            for v in range(net.W):
                b = int(net.word_off[v])
                yield b, ent[b] + em[gr.state[b]], int(gr.state[b])
                if not gr.end[b]:
                    yield b + 1, ent[b + 1] + em[gr.state[b]], int(gr.state[b])
            return
        for j in range(3):
            if gr.pos[s] + j < net.n_pos[s]:
                yield s + j, into[j, s + j] + em[gr.state[s + j]], int(gr.state[s + j])

    def walk(s, t, c, emitted):
        if t == T:
            if gr.end[s]:
                m = np.exp(-c)
                acc = sum(1 for tt, k in enumerate(emitted) if k == ref[tt])
                tot[0] += m
                tot[1] += m * acc
                for tt, k in enumerate(emitted):
                    mass[tt, k] += m
                    macc[tt, k] += m * acc
            return
        for d, x, k in succ(s, t):
            walk(d, t + 1, c + x, emitted + [k])

    walk(0, 0, 0.0, [])  # the start hypothesis: position 0 of word 0
    return tot[0], tot[1], mass, macc


@pytest.mark.parametrize("li", range(len(TINY)))
def test_restatement_is_path_enumeration(li):
    """Abar = sum P(pi) A(pi) and gamma_t(k) = sum over the paths emitting k at t of P(pi) (A(pi) - Abar), path by path"""
    net = _net(_lex(TINY[li], 0))
    S = int(net.state.max()) + 1
    rng = np.random.default_rng(160 + li)
    tdp, wp = PEN
    for T in (1, 2, 4, 5):
        e = rng.uniform(0.0, 4.0, size=(T, S))
        ref = rng.integers(0, S + 1, size=T)  # S = out of range
        for scale in (0.3, 1.0, 2.5):
            total, tacc, mass, macc = enumerate_accuracies(e, net, tdp, wp, ref, scale)
            F, A, g = SM.smbr(e, M.free_graph(net), tdp, wp, ref, scale)
            tol = 1e-12 * max(1, T)
            assert abs(F + np.log(total) / scale) <= 1e-12 * max(1.0, abs(F))
            assert abs(A - tacc / total) <= tol
            assert np.abs(g - (macc - mass * (tacc / total)) / total).max() <= tol
            assert 0.0 <= A <= T


@pytest.mark.parametrize("li", range(len(TINY)))
def test_gamma_is_the_gradient(li):
    """-kappa gamma_t(k) = d Abar / d e(t, k) by central differences; step and tolerance of test_mmi_cpu's occupancy check"""
    lex = _lex(TINY[li], 0)
    word_off, aut, sil_state = lex.flatten()
    aut = aut.copy()
    aut[-1] = aut[-2]  # the last word repeats a state
    net = R.Net(word_off, aut, 0, sil_state)
    gr = M.free_graph(net)
    rng = np.random.default_rng(180 + li)
    T, S, h = 9, lex.n_states, 1e-5
    e = rng.uniform(0.0, 4.0, size=(T, S))
    ref = rng.integers(0, S, size=T)
    for scale in (0.4, 1.0):
        _, _, g = SM.smbr(e, gr, PEN[0], PEN[1], ref, scale)
        for t in range(T):
            for k in range(S):
                d = np.zeros_like(e)
                d[t, k] = h
                fd = (SM.smbr(e + d, gr, *PEN, ref, scale)[1] - SM.smbr(e - d, gr, *PEN, ref, scale)[1]) / (2 * h)
                assert abs(fd + scale * g[t, k]) <= 1e-8, (t, k, fd, g[t, k])


@pytest.mark.parametrize("li", range(len(TINY)))
def test_identities(li):
    """sum_k gamma_t(k) = 0; Abar = sum_t occ_t(ref_t) with the MMI restatement's occupancies; F is its F; references out of range
    everywhere give Abar = 0 and gamma = 0; constant references k = 0 .. S - 1 give accuracies that sum to T"""
    net = _net(_lex(TINY[li], 0))
    gr = M.free_graph(net)
    S = int(net.state.max()) + 1
    rng = np.random.default_rng(190 + li)
    for T in (1, 3, 12):
        e = rng.uniform(0.0, 4.0, size=(T, S))
        ref = rng.integers(0, S, size=T)
        ref[T // 2] = S + 3
        for tdp, wp, scale in ((PEN[0], PEN[1], 1.0), ((3.0, 0.0, np.inf), 4.0, 0.3)):
            F, A, g = SM.smbr(e, gr, tdp, wp, ref, scale)
            Fo, occ = M.occupancies(e, gr, tdp, wp, scale)
            assert abs(F - Fo) <= 1e-12 * max(1.0, abs(Fo))
            assert np.abs(g.sum(axis=1)).max() <= 1e-12 * T
            assert abs(A - sum(occ[t, ref[t]] for t in range(T) if ref[t] < S)) <= 1e-12 * T
            F0, A0, g0 = SM.smbr(e, gr, tdp, wp, np.full(T, S), scale)
            assert A0 == 0.0 and not g0.any() and F0 == F
            assert abs(sum(SM.smbr(e, gr, tdp, wp, np.full(T, k), scale)[1] for k in range(S)) - T) <= 1e-12 * T
    assert SM.smbr(np.zeros((0, S)), gr, PEN[0], PEN[1], [], 1.0)[:2] == (np.inf, 0.0)


def criterion_refs(o, lex, feats, off, trans):
    """the reference mixtures of criterion_task: the oracle's alignment of every utterance to sil w_1 sil .. w_n sil"""
    word_off, aut, sil = lex.flatten()
    out = []
    for u, tr in enumerate(trans):
        seq = [sil]
        for w in tr:
            seq += list(aut[word_off[w]:word_off[w + 1]]) + [sil]
        out.append(o.align_full(feats[int(off[u]):int(off[u + 1])], np.asarray(seq, np.uint16))[0])
    return np.concatenate(out).astype(np.uint16)


def _accuracy_and_statistics(net, feats, off, refs, wp, scale, tb, means, inv_vars, norm):
    items, total = [[], []], 0.0
    e_all = _scores(feats, means, inv_vars, norm, tb["logw"], tb["mix_off"])
    gr = M.free_graph(net)
    for u in range(len(off) - 1):
        a, b = int(off[u]), int(off[u + 1])
        _, A, g = SM.smbr(e_all[a:b], gr, (3.0, 0.0, 30.0), wp, refs[a:b], scale)
        total += A
        items[0] += SM.signed_items(g, +1)
        items[1] += SM.signed_items(g, -1)
    tables = dict(tb, means=means, vars_inv=inv_vars, norm=norm)
    C_ = len(means)
    return total, [FB.accumulate(feats, it, tables, C_, C_, False, True) for it in items]


def test_one_ebw_step_raises_the_expected_accuracy(tmp_path, oracle_lib):
    """criterion_task under the restatement alone, references = the oracle's alignment to the transcripts: sum_u Abar_u = 76.63 of
    161 frames before the step; after one EBW step from the sMBR statistics (tau = 0, var_floor = 1e-3) 69.79 at E = 4 =
    CRITERION_E, 75.54 at E = 8, 94.91 at E = 16, 101.55 at E = 32.  The smallest E of the doubling sequence from CRITERION_E that
    raises it, 16, is SMBR_E: the GPU test takes its step there."""
    lex, spec, mp, feats, off, trans, wp, scale = criterion_task(tmp_path)
    o = oracle_lib.Oracle(mp, DIM, lex)
    tb = o.tables()
    refs = criterion_refs(o, lex, feats, off, trans)
    o.close()
    net = _net(lex)
    acc0, (num, den) = _accuracy_and_statistics(net, feats, off, refs, wp, scale, tb, tb["means"], tb["vars_inv"], tb["norm"])
    assert abs(num[1].sum() - den[1].sum()) <= 1e-9 * num[1].sum()
    raised = {}
    for E in (CRITERION_E, 2 * CRITERION_E, 4 * CRITERION_E, 8 * CRITERION_E):
        means, var = M.ebw_update(tb["means"], tb["vars_inv"], (num[0], num[1], num[2]), (den[0], den[1], den[2]), E, 0.0, 1e-3)
        norm = (DIM * np.log(2 * np.pi) + np.log(var).sum(axis=1)) / 2
        raised[E] = _accuracy_and_statistics(net, feats, off, refs, wp, scale, tb, means, 1.0 / var, norm)[0]
        print("E", E, len(feats), acc0, raised[E])
    assert min(E for E, a in raised.items() if a > acc0) == SMBR_E


def test_kernels_have_no_scratch():
    """the gfx950 code objects of viterbi_smbr.hip and of the item path (posterior_items.hip): no private segment and no vector spills
    in any of their kernels (the scalar spills of the two recursions go to VGPR lanes), and the recursions stay within the
    128 VGPRs their 512 threads assume"""
    import os
    import sys
    import tempfile
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    sys.path.insert(0, os.path.join(root, "tools"))
    import isa_info
    if not os.path.exists(os.path.join(isa_info.LLVM, "llvm-objdump")):
        pytest.skip("no ROCm LLVM tools")
    from speechrecognition_amd import build
    build.build()
    with tempfile.TemporaryDirectory() as tmp:
        md = isa_info.kernel_metadata(isa_info.code_object("viterbi_smbr", tmp))
        md.update(isa_info.kernel_metadata(isa_info.code_object("posterior_items", tmp)))
    mine = {k: v for k, v in md.items() if k.startswith(("smbr_", "items_"))}
    assert {"smbr_forward_kernel", "smbr_backward_kernel", "items_kernel<false, unsigned short>", "items_kernel<true, unsigned short>",
            "items_advance_kernel", "items_top_kernel"} <= set(mine)
    for k, v in mine.items():
        assert v.get("private_segment_fixed_size", 0) == 0 and v.get("vgpr_spill_count", 0) == 0, (k, v)
        assert v.get("vgpr_count", 0) <= 128, (k, v)
