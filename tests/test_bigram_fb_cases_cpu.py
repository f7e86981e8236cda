"""The conditions of tests/bigram_fb_cases.py, from the references alone: every case triggers the edge it is named for, no entry term
lies where a double's exp gives out, the references agree with path enumeration in both precisions, and a reference that is wrong in one
of four ways gives an answer further from the right one than the tolerance reaches.  Each test prints what it found holding."""
import math

import numpy as np
import pytest

from tests import bigram_fb_cases as bc
from tests import bigram_fb_reference as R
from tests import bigram_mmi_reference as BM

OWN = [c for c in bc.CASES if not c.base]
FREE = [c for c in OWN if c.passes != ("occ",) or c.trans is None]

needs_x87 = pytest.mark.skipif(np.finfo(np.longdouble).nmant != 63,
                               reason="np.longdouble has no 64-bit mantissa on this host: it is no yardstick for a float64 run")


def finite(x):
    return math.isfinite(float(x))


@needs_x87
def test_longdouble_has_64_bits_of_mantissa():
    assert np.finfo(np.longdouble).nmant == 63
    c = bc.by_name("dyadic-r6")
    assert bc.free_reference(c, "longdouble", "cut")[0][1].dtype == np.longdouble
    assert bc.smbr_reference(c, "longdouble", "cut")[0][2].dtype == np.longdouble and bc.chain_reference(c, "longdouble")[0][1].dtype == np.longdouble
    print(f"{len(bc.CASES)} cases, {len(OWN)} with a table of their own; longdouble carries 64 bits of mantissa")


def test_lexica_have_their_edges():
    W = {k: bc.net(k).W for k in bc.LEXICA}
    assert [W[k] for k in ("w63", "w64", "w65", "w511", "w512", "w513")] == [63, 64, 65, 511, 512, 513]
    assert all(set(bc.LEXICA[k].lens) == {1, 2} for k in ("w63", "w64", "w65", "w511", "w512", "w513"))
    assert bc.net("p513").P == bc.BLOCK + 1 and bc.net("chunks").P == 1000
    assert max(bc.LEXICA["long"].lens) > 64
    assert {bc.LEXICA[c.lex].sil == 0 for c in bc.CASES} == {True, False}
    assert {bc.LEXICA[c.lex].lens[bc.LEXICA[c.lex].sil] for c in bc.CASES} == {1, 2}
    assert {n for c in bc.CASES for n in bc.LEXICA[c.lex].lens} >= {1, 2, 3}
    for k, lx in bc.LEXICA.items():
        off, mix, sil = bc.lexicon(k)
        assert int(mix.max()) < lx.S and len(mix) == int(off[-1])
        assert sorted(set(mix[off[sil]:off[sil + 1]].tolist())) == list(range(lx.lens[sil]))
    off, mix, _ = bc.lexicon("twins")
    for w in range(1, 7, 2):
        assert np.array_equal(mix[off[w]:off[w + 1]], mix[off[w + 1]:off[w + 2]])
    t = bc.lm(bc.by_name("twins"))
    assert np.array_equal(t[1::2][:3], t[2::2]) and np.array_equal(t[:, 1::2][:, :3], t[:, 2::2])
    print("word counts 63 64 65 511 512 513; P = 513; a word of 70 states; silence first and not, of one and of two states: hold")


def test_lengths_cover_every_alive_count():
    assert sorted(bc.RAGGED70) == list(range(1, 71)) and bc.RAGGED70 != tuple(sorted(bc.RAGGED70, reverse=True))
    c = bc.by_name("ragged70")
    assert {sum(1 for T in c.lens if T > t) for t in range(70)} == set(range(1, 71))
    for n in bc.HEADS:
        h = bc.by_name(f"ragged{n}")
        assert len(h.lens) == n and h.lens == c.lens[:n] and bc.table(h).shape[0] == sum(h.lens)
        assert np.array_equal(bc.table(h), bc.table(c)[:sum(h.lens)]) and bc.labels(h).shape[0] == sum(h.lens)
    t0 = bc.by_name("t0_between")
    assert t0.lens[1] == 0 and t0.lens[0] > 0 and t0.lens[2] > 0 and 1 in t0.lens
    assert all(max(c.lens) <= 70 for c in bc.CASES)
    assert all(max(c.lens) <= 12 and len(c.lens) <= 4 for c in bc.CASES if c.lex in ("w511", "w512", "w513"))
    print("70 utterances of the lengths 1 .. 70 (n_alive 70 .. 1), heads of 16 17 48 49 64 65, a T = 0 utterance between others: hold")


@pytest.mark.parametrize("case", FREE, ids=bc.case_id)
def test_no_entry_term_where_exp_gives_out(case):
    """no term of any entry sum between -790 and -650: the references cut at 650 and at 790 agree exactly (asserted on the cases small
    enough to run a third and a fourth time)"""
    seen = bc.exponents(case)
    assert seen["band"] == 0, seen
    if bc.net(case.lex).W <= 70 and sum(case.lens) <= 400:
        a, b = bc.free_reference(case, "float64", "cut650"), bc.free_reference(case, "float64", "cut790")
        for u in a:
            assert bc.same_bytes(a[u][1:], b[u][1:]) and (a[u][0] == b[u][0] or not finite(a[u][0])), u
    print(f"{case.name}: no term inside {bc.BAND}, {seen['dropped']} below")


@pytest.mark.parametrize("case", OWN, ids=bc.case_id)
def test_utterances_have_paths_and_are_compared(case):
    U = len(case.lens)
    assert len(bc.sampled(case)) >= 0.9 * U
    if case.sample is not None:
        assert case.name in sorted(bc.CASES, key=lambda c: -sum(c.lens) * bc.net(c.lex).P)[:2]
    clean = [u for u in bc.sampled(case) if u not in case.hostile]
    if case in FREE:
        F = {u: bc.free_reference(case, "float64", bc.yardstick(case))[u][0] for u in bc.sampled(case)}
        assert all(finite(F[u]) for u in clean), F
        assert all((F[u] == 0.0) == (case.lens[u] == 0) for u in clean)
    if case.trans is not None:
        Fc = {u: bc.chain_reference(case, "float64")[u][0] for u in bc.sampled(case)}
        assert all(finite(Fc[u]) for u in clean), Fc
    print(f"{case.name}: {len(bc.sampled(case))} of {U} utterances against the references, {len(clean)} of them with a finite F")


def _F(case, u, kind="post", tab=None, lm=None, variant=None):
    e = bc.rows(case, u) if tab is None else tab
    with np.errstate(all="ignore"):
        return R.posteriors(e, bc.net(case.lex), bc.lm(case) if lm is None else lm, bc.tdp32(case), case.kappa,
                            bc._entry(case, variant or bc.yardstick(case), False))


def _moves(case, u, other):
    """the yardstick's (F, posteriors) of utterance u and `other`: do they differ by more than the rule's bound on F or on a posterior"""
    F80, p80 = bc.reference(case, "post", u)
    dF = max(bc.dist(F, F80) for F, _ in bc.restatements(case, "post", u)) if finite(F80) else 0.0
    dw = max(bc.dist(p, p80) for _, p in bc.restatements(case, "post", u))
    F2, p2 = other
    if finite(F80) != finite(F2):
        return True
    return (finite(F80) and abs(float(F2) - float(F80)) > bc.bound(dF, float(F80))) or bool(np.any(np.abs(p2 - p80.astype(np.float64)) > bc.bound(dw, p80.astype(np.float64))))


@needs_x87
def test_edges_change_the_answer():
    """each edge case's answer differs from the answer with the edge removed"""
    said = []
    for c in bc.CASES:
        u = bc.HOSTILE
        if c.table.startswith("nan_"):  # the NaN one state on: another answer; the cell lies on paths, and as +inf it leaves others
            t, k = bc.nan_cell(c)
            raw = bc.rows(c, u, clean=False)
            assert np.argwhere(np.isnan(bc.table(c))).tolist() == [[int(bc.frame_off(c)[u]) + t, k]]
            moved = np.array(raw)
            moved[t, k], moved[t, (k + 1) % raw.shape[1]] = 7.0, np.nan
            assert finite(_F(c, u)[0]) and _moves(c, u, _F(c, u, tab=bc.nc.sanitised(moved))), c.name
            cheap = np.array(bc.rows(c, u))
            cheap[t, k] = -100.0
            assert _F(c, u, tab=cheap)[0] < _F(c, u)[0]
            said.append(c.name)
        if c.table == "inf_frame":
            F = [bc.free_reference(c, "float64", "cut")[v][0] for v in range(3)]
            assert finite(F[0]) and F[1] == math.inf and finite(F[2])
            said.append(c.name)
        if c.table == "inf_band":  # one way through the band: the silence
            p = bc.free_reference(c, "float64", "cut")[3][1]
            T, sil = c.lens[3], bc.LEXICA[c.lex].sil
            assert np.all(np.abs(p[T // 3:2 * T // 3 + 1, sil] - 1.0) <= 1e-12)
            said.append(c.name)
        if c.lm == "holes" and "post" in c.passes:  # the word with one permitted history: permit no history, and its mass is gone
            W, sil = bc.net(c.lex).W, bc.LEXICA[c.lex].sil
            words = [w for w in range(W) if w != sil]
            t = bc.lm(c)
            assert np.isfinite(t[words[1]]).sum() == 1 and not np.isfinite(np.delete(t[:, words[-1]], sil)).any()
            assert np.isnan(t).any() and np.isposinf(t).any()
            shut = np.array(t)
            shut[words[1], :] = np.inf
            assert any(_moves(c, v, _F(c, v, lm=shut)) for v in range(len(c.lens))), c.name
            said.append(c.name)
        if c.lm == "negative":
            assert (bc.lm(c) < 0).any() and (bc.table(c) < 0).any()
        if c.name == "twins":  # equal bits in the reference already; another LM row for a twin: no longer
            p = bc.free_reference(c, "float64", "cut")[2][1]
            assert np.array_equal(p[:, 1::2], p[:, 2::2]) and (p[:, 1:] > 0).all(axis=0).any()
            t = np.array(bc.lm(c))
            t[2, :] += 0.25
            p2 = _F(c, 2, lm=t)[1]
            assert not np.array_equal(p2[:, 1], p2[:, 2]) and _moves(c, 2, _F(c, 2, lm=t))
            said.append(c.name)
        if c.table == "gap":
            far = c.name.startswith("gap_far")
            Fcut, Fplain = _F(c, u, variant="cut")[0], _F(c, u, variant="plain")[0]
            assert finite(Fplain) and finite(Fcut) != far, (c.name, Fcut, Fplain)
            assert _moves(c, u, _F(c, u, variant="plain")) == far
            said.append(c.name)
    assert len(said) >= 14
    print("with the edge removed the answer moves by more than the bound: " + " ".join(said))


def test_kappas_and_transcripts():
    assert {0.3, 1.0, 2.5} <= {c.kappa for c in bc.CASES}
    tr, lens = bc.CHAINS["shapes"][1:]
    assert tr[0] == () and len(tr[1]) == 1 and tr[2][0] == tr[2][1]
    F = [bc.chain_reference(bc.by_name("chain-shapes"), "float64")[u][0] for u in range(len(lens))]
    assert [finite(f) for f in F] == [True, True, True, False, True], F  # (the chain of three words in two frames: no path)
    c = bc.by_name("chain-forbidden")
    t, tr = bc.lm(c), bc.transcripts(c)
    assert np.isposinf(t[tr[1][1], tr[1][0]]) and np.isnan(t[tr[2][1], tr[2][0]])
    F = [bc.chain_reference(c, "float64")[u][0] for u in range(4)]
    assert [finite(f) for f in F] == [True, False, False, True], F
    for name in ("ragged70", "t0_between", "twins"):  # the chain's paths are paths of the free network
        c = bc.by_name(name)
        for u in bc.sampled(c):
            assert bc.chain_reference(c, "float64")[u][0] >= bc.free_reference(c, "float64", "cut")[u][0] - 1e-9
    print("kappa 0.3 1 2.5; transcripts empty, of one word, w w, forbidden by +inf and by NaN, longer than T allows: hold")


def test_labels():
    for c in OWN:
        if "smbr" not in c.passes:
            continue
        S, lab = bc.LEXICA[c.lex].S, bc.labels(c)
        if c.labels == "none":
            assert np.all(lab >= S)
            assert all(a == 0.0 and not g.any() for _, a, g in bc.smbr_reference(c, "float64", "cut").values())
        else:
            assert np.all(lab < S)
    assert {"none", "first", "best", "random"} <= {c.labels for c in bc.CASES}
    c = bc.by_name("ragged70")  # the best path carries most of the mass, so its labels are mostly right
    acc = [float(a) / T for (F, a, _), T in zip(bc.smbr_reference(c, "float64", "cut").values(), c.lens) if T > 10]
    assert min(acc) > 0.5, acc
    print(f"labels none, first, best (expected accuracy at least {min(acc):.2f} of the frames) and random: hold")


@needs_x87
@pytest.mark.parametrize("name", ["chain-shapes", "t0_between", "holes-b5"])
def test_recursions_are_path_enumeration(name):
    """the brute force agrees with the float64 and the longdouble run, on the utterances short enough to enumerate"""
    c = bc.by_name(name)
    nt = bc.net(c.lex)
    done = 0
    for u, T in enumerate(c.lens):
        if not 0 < T <= 4:
            continue
        e = bc.rows(c, u)
        Fb, pb = R.brute_force(e, nt, bc.lm(c), bc.tdp32(c), c.kappa)
        paths = BM.enumerate_paths(e, nt, bc.lm(c), bc.tdp32(c), c.kappa)
        mass = sum(m for m, _ in paths.values())
        occ = sum(cnt for _, cnt in paths.values()) / mass
        for dt in ("float64", "longdouble"):
            F, p, o = bc.free_reference(c, dt, "plain")[u] if "post" in c.passes else (None, None, None)
            if F is not None:
                assert abs(float(F) - Fb) <= 1e-12 * max(1.0, abs(Fb)) and bc.dist(p, pb) <= 1e-12 and bc.dist(o, occ) <= 1e-12
            if c.trans is not None:
                key = tuple(bc.transcripts(c)[u])
                Fc, oc = bc.chain_reference(c, dt)[u]
                if key in paths:
                    assert abs(float(Fc) + math.log(paths[key][0]) / c.kappa) <= 1e-12 * max(1.0, abs(float(Fc)))
                    assert bc.dist(oc, paths[key][1] / paths[key][0]) <= 1e-12
                else:
                    assert Fc == math.inf
        done += 1
    assert done
    print(f"{name}: {done} utterances enumerated, both precisions agree")


def test_chunks_are_cut_small():
    c = bc.by_name("chunks")
    assert 20 <= len(c.lens) <= 28 and min(c.lens) >= 10 and max(c.lens) <= 40
    for mult in (1, 2):
        plan = bc.plan(c, mult)
        groups = [g for ch in plan for g in ch]
        assert len(plan) >= 3 and len(groups) >= 5 and any(v - u > 1 for u, v in groups), plan
        assert any(u > 0 for ch in plan[1:] for u, _ in ch[1:])  # a group that starts at neither a chunk's nor the call's first frame
        assert groups[0][0] == 0 and groups[-1][1] == len(c.lens) and all(a[1] == b[0] for a, b in zip(groups, groups[1:]))
        print(f"chunks at multiplicity {mult}: {len(plan)} score chunks, {len(groups)} launch groups")


# ---- references that are wrong on purpose ---------------------------------------------------------------------------------------------------
def _wrong_F(case, u, copy_through_lm=False, no_skip_penalty=False):
    """kappa F of bigram_fb_reference.forward's recursion with one of two mistakes: the silence copies entered through the LM (as
    the silence row of the LM, which the network never reads), or the entry into a second state at no skip penalty"""
    nt, e, scale = bc.net(case.lex), bc.rows(case, u), case.kappa
    klm, td = R._klm(nt, bc.lm(case), scale), R._tdp(bc.tdp32(case), scale)
    raw = scale * np.where(np.isnan(bc.lm(case)), np.inf, bc.lm(case).astype(np.float64))
    pt = td[nt.is_sil]
    we = R.start_ends(nt)
    prev = np.full(nt.P, np.inf)
    with np.errstate(all="ignore"):
        for t in range(e.shape[0]):
            ent = R.entries(nt, we, klm)
            if copy_through_lm:
                ent[nt.W:] = R._lsum(R.histories(nt, we)[None, :] + raw[nt.sil][None, :], axis=1)
                ent[nt.sil + nt.W] = np.inf
            ent = ent[nt.slot]
            c = [prev + pt[:, 0], np.where(nt.k >= 1, R._shift(prev, 1) + pt[:, 1], np.inf), np.where(nt.k >= 2, R._shift(prev, 2) + pt[:, 2], np.inf),
                 np.where(nt.k == 0, ent, np.inf), np.where(nt.k == 1, ent + (0.0 if no_skip_penalty else pt[:, 2]), np.inf)]
            prev = R._comb(c, "log") + scale * e[t, nt.state]
            prev = np.where(np.isnan(prev), np.inf, prev)
            we = prev[nt.last] + td[nt.slot_sil, 3]
        return R._lsum(we) / scale


@needs_x87
def test_wrong_references_lie_outside_the_bound():
    """the silence copy entered through the LM; the skip penalty dropped from a second-state entry; the underflow cut removed on the
    far side; a NaN treated as 0: each moves some case's F by more than that case's bound"""
    def outside(case, u, F_wrong):
        F80 = bc.reference(case, "post", u)[0]
        dF = max(bc.dist(F, F80) for F, _ in bc.restatements(case, "post", u)) if finite(F80) else 0.0
        return finite(F80) != finite(F_wrong) or (finite(F80) and abs(float(F_wrong) - float(F80)) > bc.bound(dF, float(F80)))

    c = bc.by_name("t0_between")
    assert not outside(c, 0, _wrong_F(c, 0)) and not outside(c, 2, _wrong_F(c, 2))  # (without a mistake it restates the reference)
    assert outside(c, 0, _wrong_F(c, 0, copy_through_lm=True)) and outside(c, 2, _wrong_F(c, 2, no_skip_penalty=True))
    n = 0
    for case in FREE:
        if "post" in case.passes and bc.net(case.lex).W <= 70 and sum(case.lens) <= 400 and not case.plain:
            us = [u for u in range(len(case.lens)) if case.lens[u] > 1 and u not in case.hostile]
            n += any(outside(case, u, _wrong_F(case, u, copy_through_lm=True)) for u in us)
            n += any(outside(case, u, _wrong_F(case, u, no_skip_penalty=True)) for u in us)
    assert n >= 20
    far = bc.by_name("gap_far")
    assert outside(far, bc.HOSTILE, _F(far, bc.HOSTILE, variant="plain")[0])
    for name in ("nan_first-r6", "nan_sil-b5"):
        case = bc.by_name(name)
        zero = np.nan_to_num(bc.rows(case, bc.HOSTILE, clean=False), nan=0.0, posinf=np.inf)
        assert outside(case, bc.HOSTILE, _F(case, bc.HOSTILE, tab=zero)[0])
    print(f"wrong references outside the bound: the copy through the LM and the missing skip penalty on {n} case sides, the missing cut on "
          "gap_far, NaN as 0 on nan_first-r6 and nan_sil-b5")
