"""The conditions of tests/netfb_cases.py, from the references alone: every case triggers the edge it is named for, the three
references agree with path enumeration and with each other, and their float64 runs lie a finite distance from the longdouble ones."""
import math

import numpy as np
import pytest

from tests import mmi_reference as M
from tests import net_fb_reference as R
from tests import netfb_cases as nc

SMALL = [c for c in nc.CASES if c.lex in ("a", "b", "c", "d", "e", "s", "twins")]


def test_longdouble_has_64_bits_of_mantissa():
    assert np.finfo(np.longdouble).nmant == 63


def test_lexica_have_their_edges():
    P = {k: nc.net(k).P for k in nc.LEXICA}
    assert (P["p511"], P["p512"], P["p513"], P["p1025"], P["w600"]) == (nc.BLOCK - 1, nc.BLOCK, nc.BLOCK + 1, 2 * nc.BLOCK + 1, 601)
    for k, lx in nc.LEXICA.items():
        off, aut, sil, sil_state = nc.lexicon(k)
        assert int(aut.max()) < lx.S and max(lx.lens) >= 2, k
        assert [int(s) for s in np.flatnonzero(aut == sil_state)] == sorted((int(off[sil]),) + lx.sil_at), k
    n = nc.net("s")  # the silence state inside words, behind another state: a move into it costs `forward` whatever the jump
    assert all(n.pos[s] >= 1 and n.state[s - 1] != 0 for s in nc.LEXICA["s"].sil_at)
    # the silence word is first, or not: both
    assert {nc.LEXICA[c.lex].sil == 0 for c in nc.CASES} == {True, False}
    assert {nc.LEXICA[c.lex].lens[0] == 1 for c in nc.CASES} == {True, False}
    # p1025: thread 0 owns three slots, 512 distinct states, the 65-position word covers a whole wave (slots 1 .. 65: lanes 1 .. 63 of
    # wave 0 and 0 .. 1 of wave 1 hold no word end but its own)
    n = nc.net("p1025")
    assert len(range(0, n.P, nc.BLOCK)) == 3 and len(np.unique(n.state)) == 512
    assert n.word[1] == 1 and n.word[65] == 1 and n.word[66] == 2 and not n.end[1:65].any()
    assert set(int(x) for x in np.diff(n.word_off)[2:]) == {1, 2, 3, 4, 5, 6}
    # w600: the word ends lie in waves 0 and 1 only
    assert sorted({int(s % nc.BLOCK) // 64 for s in np.flatnonzero(nc.net("w600").end)}) == [0, 1]
    # ones: slots 60 .. 70 are position 0 and word end at once, on both sides of slot 64
    n = nc.net("ones")
    assert np.all(n.end[60:71] & (n.pos[60:71] == 0)) and n.pos[59] > 0 and n.pos[71] == 0 and not n.end[71]
    # the word lanes and the top-K passes: one under, at and over 64 words, and more than two passes
    assert [nc.net(k).W for k in ("w64", "w65", "w130")] == [64, 65, 130]
    assert all(set(nc.LEXICA[k].lens) == {1, 2} for k in ("w64", "w65", "w130"))
    # twins: every word but the silence twice, the same states
    off, aut, _, _ = nc.lexicon("twins")
    for w in range(1, 9, 2):
        assert np.array_equal(aut[off[w]:off[w + 1]], aut[off[w + 1]:off[w + 2]])


def test_lengths_and_launch_groups():
    assert {1, 2, 3} <= {t for c in nc.CASES for t in c.lens}
    assert min(nc.RAGGED) == 1 and max(nc.RAGGED) == 70
    long = {c.name: max(c.lens) for c in nc.CASES if max(c.lens) > 70}
    assert set(long) == {"chain-n256_257", "chain-n514", "chain-mixed"}  # (netfb_cases' docstring: a path needs the frames)
    # every residue of a launch group's frame count mod 4 (netfb_words_kernel and netfb_top_kernel take four frames a block): the
    # default budgets make one group of a call
    assert {sum(c.lens) % 4 for c in nc.CASES if "post" in c.passes} == {0, 1, 2, 3}
    c = nc.by_name("chunks")
    assert nc.LEXICA[c.lex].S * 8 == 4096 and (1 << 20) // 4096 == 256
    for cell in (8, 16):  # the posteriors' and occupancies' trellis, the accuracies'
        plan = nc.plan(c, cell)
        groups = [g for ch in plan for g in ch]
        assert len(plan) >= 2 and len(groups) >= 3 and any(v - u > 1 for u, v in groups), plan
        assert any(u > 0 for ch in plan[1:] for u, _ in ch[1:])  # a group that starts at neither a chunk's nor the call's first frame
        assert groups[0][0] == 0 and groups[-1][1] == len(c.lens) and all(a[1] == b[0] for a, b in zip(groups, groups[1:]))
        assert all(nc.net(c.lex).P * cell * sum(c.lens[u:v]) <= 1 << 20 for u, v in groups)
    assert len({f % 4 for f in nc.group_frames(c)}) >= 3
    assert all(u < len(c.lens) for u in c.sample) and len(c.sample) == 4


def test_chains_have_their_lengths():
    n = nc.net("two")
    for k, (trans, frames) in nc.CHAINS.items():
        assert tuple(M.chain_graph(n, t).P for t in trans) == nc.CHAIN_LENGTHS[k], k
        assert len(trans) == len(frames)
    got = {x for v in nc.CHAIN_LENGTHS.values() for x in v}
    assert {64, 65, 256, 257} <= got and max(got) > 512
    # chain_block's three sizes, and the group that mixes two of them
    assert nc.CHAIN_LENGTHS["mixed"] == (10, 300)
    # which have a path: all but the three-position word in one frame
    for k in nc.CHAINS:
        c = nc.by_name(f"chain-{k}")
        F = [float(nc.occ_reference(c, "float64", True)[u][0]) for u in range(len(c.lens))]
        want = [True, True, False] if k == "empty_one" else [True] * len(F)
        assert [math.isfinite(f) for f in F] == want, (k, F)


@pytest.mark.parametrize("case", [c for c in nc.CASES if c.table.startswith("nan_")], ids=nc.case_id)
def test_nan_placements(case):
    n = nc.net(case.lex)
    t, k, slot = nc.nan_cells(case)
    tab = nc.rows(case, nc.HOSTILE, clean=False)
    assert np.argwhere(np.isnan(nc.table(case))).tolist() == [[int(nc.frame_off(case)[nc.HOSTILE]) + t, k]]
    assert np.isnan(tab[t, k]) and n.state[slot] == k
    want_pos = {"nan_pos0": 0, "nan_own1": 1, "nan_first1": 0, "nan_pos2": 2}[case.table]
    assert n.pos[slot] == want_pos and list(np.flatnonzero(n.state == k)) == [slot]
    if case.table == "nan_first1":  # ... and the word has a position 1 whose entry pays this state
        assert n.n_pos[slot] >= 2 and n.first[slot + 1] == k and n.state[slot + 1] != k
    if case.table == "nan_pos0" and case.lex == "d":
        assert n.n_pos[slot] == 1
    # the cell lies on paths (a cheap value there moves F), and as +inf it leaves the utterance others
    F = nc.post_reference(case, "float64")[nc.HOSTILE][0]
    other = np.array(tab)
    other[t, k] = -100.0
    tdp, wp = case.penalties
    F0 = R.posteriors(other, n, tdp, wp, case.kappa)[0]
    assert math.isfinite(F) and math.isfinite(F0) and F0 < F


def test_hostile_tables():
    for c in nc.CASES:
        if c.table == "inf_frame":
            F = [float(nc.post_reference(c, "float64")[u][0]) for u in range(3)]
            assert math.isfinite(F[0]) and F[1] == math.inf and math.isfinite(F[2]), (c.name, F)
        if c.table == "neginf":
            t = nc.table(c)
            assert np.sum(np.isneginf(t)) == 1 and not np.isneginf(np.delete(t, slice(*nc.frame_off(c)[1:3].astype(int)), axis=0)).any()
        if c.table == "inf_band":  # one way through the band: the silence word's loop
            p = nc.post_reference(c, "float64")[3][1]
            sil = nc.LEXICA[c.lex].sil
            T = c.lens[3]
            assert np.all(np.abs(p[T // 3:2 * T // 3 + 1, sil] - 1.0) <= 1e-12)
        if c.table == "dyadic" and c.lex == "twins":
            p = nc.post_reference(c, "float64")[2][1]
            assert np.array_equal(p[:, 1::2], p[:, 2::2]) and (p[:, 1:] > 0).any()


def test_labels():
    for c in nc.CASES:
        S, lab = nc.LEXICA[c.lex].S, nc.labels(c)
        if c.labels == "none":
            assert np.all(lab >= S)
            assert all(a == 0.0 and not g.any() for _, a, g in nc.smbr_reference(c, "float64").values())
        else:
            assert np.all(lab < S)
    # the best path carries most of the mass, so its labels are mostly right (a random walk hits one frame in some twenty)
    c = nc.by_name("labels_best-c")
    acc = [a / T for (F, a, _), T in zip(nc.smbr_reference(c, "float64").values(), c.lens) if math.isfinite(F) and T > 10]
    assert acc and min(acc) > 0.5, acc
    # `first`: some of the expected accuracy comes through entries into position 1 (which pay, and score as, the first state)
    c = nc.by_name("labels_first-d")
    n = nc.net(c.lex)
    k = int(nc.labels(c)[0])
    assert list(n.pos[n.state == k]) == [0] and n.n_pos[n.state == k][0] >= 3


@pytest.mark.parametrize("name", ["t123-a", "ragged-e"])
def test_recursions_are_path_enumeration(name):
    c = nc.by_name(name)
    n = nc.net(c.lex)
    tdp, wp = c.penalties
    for u, T in enumerate(c.lens):
        if T > 5:
            continue
        e = nc.rows(c, u)
        F, p = nc.post_reference(c, "float64")[u]
        Fb = R.brute_force(e, n, tdp, wp, c.kappa)
        assert abs(F - Fb) <= 1e-12 * max(1.0, abs(Fb))
        paths = M.enumerate_paths(e, n, tdp, wp, c.kappa)
        mass = sum(m for m, _ in paths.values())
        occ = sum(cnt for _, cnt in paths.values()) / mass
        Fo, o = nc.occ_reference(c, "float64", False)[u]
        assert abs(Fo - F) <= 1e-12 * max(1.0, abs(F)) and np.abs(o - occ).max() <= 1e-12


@pytest.mark.parametrize("case", [c for c in SMALL if c.lex != "twins" and "occ" in c.passes and "post" in c.passes], ids=nc.case_id)
def test_references_agree_and_lie_close_to_longdouble(case):
    n = nc.net(case.lex)
    p64, p80 = nc.post_reference(case, "float64"), nc.post_reference(case, "longdouble")
    o64, o80 = nc.occ_reference(case, "float64", False), nc.occ_reference(case, "longdouble", False)
    s64, s80 = nc.smbr_reference(case, "float64"), nc.smbr_reference(case, "longdouble")
    for u in o64:
        if case.table == "neginf" and u == nc.HOSTILE:  # (no reference for a -inf entry: the contract's conditions hold it)
            continue
        F, p = p64[u]
        Fo, occ = o64[u]
        if not math.isfinite(F):
            assert F == Fo == s64[u][0] == math.inf and not p.any() and not occ.any()
            continue
        tol = 64 * nc.ulp(F) + 8 * nc.dist(F, p80[u][0])
        assert abs(F - Fo) <= tol and abs(F - s64[u][0]) <= tol, (u, F, Fo)
        if len(np.unique(n.state)) < n.P:
            continue
        # (the states of these lexica are distinct: a word's posterior is the occupancy of its states)
        by_word = np.stack([occ[:, n.state[n.word_off[w]:n.word_off[w + 1]]].sum(axis=1) for w in range(n.W)], axis=1)
        assert np.abs(by_word - p).max() <= 1e-12 + 8 * (nc.dist(p, p80[u][1]) + nc.dist(occ, o80[u][1]))
        for a, b in ((F, p80[u][0]), (p, p80[u][1]), (Fo, o80[u][0]), (occ, o80[u][1]), (s64[u][1], s80[u][1]), (s64[u][2], s80[u][2])):
            assert math.isfinite(nc.dist(a, b))
