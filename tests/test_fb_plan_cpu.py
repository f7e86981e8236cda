"""The host planning of the forward-backward passes without a GPU: speechrecognition_amd/csrc/fb_plan.h -- compiled with the host
compiler alone, under AddressSanitizer and UBSan, into tests/cpp/fb_plan_driver -- against the rules restated here: the launch groups
of a chunk, the longest-first order with its alive counts, the mixture lists, an occupancy pass' trellis offsets and lists, and the
segments of the adaptation statistics."""
import os
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("fbplan") / "fb_plan_driver")
    subprocess.check_call(["g++", "-O1", "-std=c++17", "-Wall", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           "-I" + os.path.join(ROOT, "speechrecognition_amd", "csrc"),
                           os.path.join(ROOT, "tests", "cpp", "fb_plan_driver.cpp"), "-o", exe])
    return exe


def run_cases(exe, tmp_path, cases):
    """cases: token lists, one per case -> per case the answer's lines as (name, [ints])"""
    path = tmp_path / "cases.txt"
    path.write_text("\n".join(" ".join(str(t) for t in c) for c in cases) + "\n")
    out, cur = [], []
    for ln in subprocess.check_output([exe, str(path)], text=True).splitlines():
        name, *vals = ln.split()
        if name == "end":
            out.append(cur)
            cur = []
        else:
            cur.append((name, [int(v) for v in vals]))
    assert not cur and len(out) == len(cases)
    return out


# ---- launch groups, order, alive -------------------------------------------------------------------------------------------------

def greedy(chunks, cost, budget):
    """The rule: a group takes its first utterance whatever it costs, then the next ones of its chunk while it stays in the budget."""
    out = []
    for u0, u1 in chunks:
        gs, u = [], u0
        while u < u1:
            v = u + 1
            while v < u1 and cost[v + 1] - cost[u] <= budget:
                v += 1
            gs.append((u, v))
            u = v
        out.append(gs)
    return out


def group_case(chunks, lens, budget, per_frame=8, per_utt=0):
    frame_off = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64).tolist()
    cost = [per_frame * frame_off[u] + u * per_utt for u in range(len(lens) + 1)]
    return dict(chunks=chunks, lens=list(lens), frame_off=frame_off, cost=cost, budget=budget)


def tokens(c):
    return ["groups", len(c["chunks"]), len(c["lens"]), c["budget"]] + [x for ch in c["chunks"] for x in ch] + c["frame_off"] + c["cost"]


def check_groups(c, answer):
    chunks, lens, cost, budget, frame_off = c["chunks"], c["lens"], c["cost"], c["budget"], c["frame_off"]
    U = len(lens)
    rows = [v for n, v in answer if n == "chunk"]
    got = [list(zip(r[0::2], r[1::2])) for r in rows]
    assert got == greedy(chunks, cost, budget)
    assert len(got) == len(chunks)
    flat = []
    for (u0, u1), gs in zip(chunks, got):
        # a partition of the chunk's range, in order; nothing empty, nothing across a chunk
        assert [g[0] for g in gs] == [u0] + [g[1] for g in gs[:-1]] if gs else u0 == u1
        assert all(a < b for a, b in gs) and (not gs or gs[-1][1] == u1)
        for a, b in gs:
            if b - a > 1:
                assert cost[b] - cost[a] <= budget
            if b < u1:
                assert cost[b + 1] - cost[a] > budget      # it could not have taken the next one
            if cost[a + 1] - cost[a] > budget:
                assert b == a + 1                          # alone over the budget: a group of one
        flat += gs
    (mx,) = [v for n, v in answer if n == "max"]
    assert mx == [max([frame_off[b] - frame_off[a] for a, b in flat], default=0), max([b - a for a, b in flat], default=0),
                  max([cost[b] - cost[a] for a, b in flat], default=0)]
    (order,) = [v for n, v in answer if n == "order"]
    assert sorted(order) == list(range(U))
    covered = np.zeros(U, bool)
    steps = [v for n, v in answer if n == "steps"]
    assert len(steps) == len(flat)
    for (a, b), st in zip(flat, steps):
        covered[a:b] = True
        assert order[a:b] == sorted(range(a, b), key=lambda u: -lens[u])     # (sorted is stable) longest first inside the group
        t_max, alive = st[0], st[1:]
        assert t_max == max(lens[a:b]) and len(alive) == t_max + 1
        assert alive == [sum(1 for u in range(a, b) if lens[u] > t) for t in range(t_max + 1)]
    for u in np.flatnonzero(~covered):
        assert order[u] == u                                                 # the identity outside the groups


def hand_group_cases():
    L = [3, 5, 2, 7, 1]                                   # 8 bytes a frame: 24, 40, 16, 56, 8
    yield group_case([(0, 5)], L, 64)                     # (0 1) (2) (3 4): 64 fits exactly, 80 and 72 do not
    yield group_case([(0, 5)], L, 63)
    yield group_case([(0, 2), (2, 5)], L, 10 ** 9)        # a budget above everything still stops at the chunk's end
    yield group_case([(0, 5)], L, 0)                      # below every utterance: groups of one, no empty group, no endless loop
    yield group_case([(0, 5)], L, 55)                     # utterance 3 alone exceeds the budget
    yield group_case([(0, 5)], [0, 0, 4, 0, 0], 32)       # zero-length utterances
    yield group_case([(0, 3)], [0, 0, 0], 0)
    yield group_case([], [], 100)                         # U = 0, no chunk
    yield group_case([(0, 0)], [], 100)                   # U = 0, an empty chunk
    yield group_case([(0, 4)], [4, 4, 4, 4], 100, per_frame=8, per_utt=20)   # 52 each: (0) (1) (2) (3); 104 > 100
    yield group_case([(0, 4)], [4, 4, 4, 4], 104, per_frame=8, per_utt=20)   # (0 1) (2 3)
    yield group_case([(1, 3)], [9, 2, 2, 9], 1000)        # a chunk list that leaves utterances out: their order is the identity
    yield group_case([(0, 6)], [5, 5, 9, 5, 9, 1], 10 ** 6)                  # ties keep corpus order: 2 4 0 1 3 5


def random_group_cases():
    rng = np.random.default_rng(11)
    for _ in range(300):
        U = int(rng.integers(0, 41))
        lens = rng.choice([0, 1, 2, 3, 7, 20, 50], size=U).tolist() if rng.random() < 0.3 else rng.integers(1, 60, size=U).tolist()
        n_chunks = int(rng.integers(1, 5))
        cuts = sorted(rng.integers(0, U + 1, size=n_chunks - 1).tolist())
        chunks = list(zip([0] + cuts, cuts + [U]))
        per_frame, per_utt = int(rng.choice([8, 16, 42])), int(rng.choice([0, 0, 100]))
        alone = [per_frame * t + per_utt for t in lens] or [0]
        total = per_frame * sum(lens) + U * per_utt
        budget = int(rng.choice([max(min(alone) - 1, 0), min(alone), max(alone), max(alone) + 1, 2 * max(alone), total // 2, total,
                                 total + 1, int(rng.integers(0, total + 2))]))
        yield group_case(chunks, lens, budget, per_frame, per_utt)


def test_hand_cases_of_the_reference_rule():
    c = group_case([(0, 5)], [3, 5, 2, 7, 1], 64)
    assert greedy(c["chunks"], c["cost"], 64) == [[(0, 2), (2, 3), (3, 5)]]
    assert greedy(c["chunks"], c["cost"], 63) == [[(0, 1), (1, 3), (3, 4), (4, 5)]]
    assert greedy(c["chunks"], c["cost"], 0) == [[(0, 1), (1, 2), (2, 3), (3, 4), (4, 5)]]
    assert greedy([(0, 2), (2, 5)], c["cost"], 10 ** 9) == [[(0, 2)], [(2, 5)]]


def test_header_groups_order_and_alive(driver, tmp_path):
    cases = list(hand_group_cases()) + list(random_group_cases())
    assert len(cases) > 300
    answers = run_cases(driver, tmp_path, [tokens(c) for c in cases])
    multi = 0
    for c, a in zip(cases, answers):
        check_groups(c, a)
        multi += any(b - a_ > 1 for n, v in a if n == "chunk" for a_, b in zip(v[0::2], v[1::2]))
    assert multi > 100     # the random budgets do produce groups of several utterances


# ---- mixture lists ---------------------------------------------------------------------------------------------------------------

def check_mix(sets, masked, answer):
    d = dict(answer)
    mix_off, mix, slot_beg, slot_pos = d["mix_off"], d["mix"], d["slot_beg"], d["slot_pos"]
    assert len(mix_off) == len(sets) + 1 and mix_off[0] == 0
    assert len(slot_beg) == len(mix) + 1 and slot_beg[-1] == len(slot_pos) == sum(len(s) for s in sets)
    pos0 = 0
    for s, ids in enumerate(sets):
        want = [i & 0xFFFF for i in ids] if masked else list(ids)
        mine = mix[mix_off[s]:mix_off[s + 1]]
        assert mine == sorted(set(want))                    # ascending and distinct
        back = {}
        for k in range(mix_off[s], mix_off[s + 1]):
            ps = slot_pos[slot_beg[k]:slot_beg[k + 1]]
            assert ps == sorted(ps) and ps
            for p in ps:
                assert p not in back
                back[p] = mix[k]
        assert [back[p] for p in range(len(ids))] == want    # the position -> mixture map, exactly
        assert slot_beg[mix_off[s]] == pos0
        pos0 += len(ids)


def mix_cases():
    rng = np.random.default_rng(3)
    shapes = [[[]], [[], [5, 5, 5], []], [[7, 3, 7, 3, 9]], [[0, 65535, 0]], []]
    for _ in range(30):
        shapes.append([rng.choice([0, 1, 2, 40, 41, 3000, 65535], size=int(rng.integers(0, 30))).tolist() for _ in range(int(rng.integers(1, 6)))])
    for sets in shapes:
        for width in (16, 32):
            yield sets, width, False
            # masked: the upper half of an entry is something else (slot_info / pos_info keep flags there)
            yield [[i | int(rng.integers(0, 1 << 15)) << 16 for i in s] for s in sets], width, True


def test_header_mixture_lists(driver, tmp_path):
    cases = list(mix_cases())
    toks = [["mix", w, int(m), len(sets)] + [x for s in sets for x in [len(s)] + s] for sets, w, m in cases]
    for (sets, _, masked), a in zip(cases, run_cases(driver, tmp_path, toks)):
        check_mix(sets, masked, a)


# ---- an occupancy pass' plan, a group's longest utterance -------------------------------------------------------------------------

def occ_cases():
    rng = np.random.default_rng(5)
    ids = [0, 1, 2, 40, 41, 3000, 65535]
    for k in range(60):
        U = int(rng.integers(0, 7))
        lens = rng.choice([0, 1, 4, 7, 20], size=U).tolist()
        chain, lists, width = bool(k & 1), bool(k & 2) or k % 5 == 0, (16, 32)[(k >> 2) & 1]
        P = int(rng.integers(0, 12))
        chains = [rng.choice(ids, size=int(rng.integers(0, 9))).tolist() for _ in range(U)] if chain else None
        info = [int(i) | int(rng.integers(0, 1 << 15)) << 16 for i in (sum(chains, []) if chain else rng.choice(ids, size=P).tolist())]
        yield dict(U=U, P=P, lens=lens, chains=chains, info=info, lists=lists, width=width)


def test_header_occupancy_plan(driver, tmp_path):
    cases = list(occ_cases())
    toks = []
    for c in cases:
        frame_off = np.concatenate([[0], np.cumsum(c["lens"])]).astype(np.int64).tolist()
        chain_off = np.concatenate([[0], np.cumsum([len(x) for x in c["chains"]])]).astype(np.int64).tolist() if c["chains"] is not None else []
        toks.append(["occ", c["width"], int(c["chains"] is not None), int(c["lists"]), c["U"], c["P"]] + frame_off + chain_off + c["info"])
    assert any(c["chains"] is not None and c["lists"] and c["U"] > 2 for c in cases) and any(c["chains"] is None and not c["lists"] for c in cases)
    for c, a in zip(cases, run_cases(driver, tmp_path, toks)):
        d = dict(a)
        U, lens, chains = c["U"], c["lens"], c["chains"]
        n_pos = [len(x) for x in chains] if chains is not None else [c["P"]] * U
        assert d["tr_off"] == np.concatenate([[0], np.cumsum([n * t for n, t in zip(n_pos, lens)])]).astype(np.int64).tolist()
        sets = ([[i & 0xFFFF for i in c["info"][sum(n_pos[:u]):sum(n_pos[:u + 1])]] for u in range(U)] if chains is not None
                else [[i & 0xFFFF for i in c["info"]]]) if c["lists"] else []
        check_mix(sets, False, a)
        distinct = [len(set(s)) for s in sets]
        assert d["bound"] == [sum(t * (distinct[u] if chains is not None else distinct[0]) for u, t in enumerate(lens)) if c["lists"] else 0]
        per = n_pos if chains is not None else lens          # the driver scans chain_off, or frame_off for the free network
        assert d["maxpos"] == [max(1, n) for n in per] + [max([1] + per)]


# ---- segments ----------------------------------------------------------------------------------------------------------------------

def test_header_segments(driver, tmp_path):
    rng = np.random.default_rng(9)
    cases = [([], 4), ([0], 4), ([0, 0, 0], 1), ([4], 4), ([5], 4), ([3, 0, 8, 1], 4), ([128, 129, 127], 128)]
    cases += [(rng.integers(0, 40, size=int(rng.integers(0, 8))).tolist(), int(rng.choice([1, 3, 16]))) for _ in range(40)]
    toks = [["seg", len(sizes), L] + np.concatenate([[0], np.cumsum(sizes)]).astype(np.int64).tolist() for sizes, L in cases]
    for (sizes, L), a in zip(cases, run_cases(driver, tmp_path, toks)):
        d = dict(a)
        begin, ln, off = d["begin"], d["len"], d["off"]
        assert len(off) == len(sizes) + 1 and off[0] == 0 and off[-1] == len(begin) == len(ln)
        b0 = 0
        for r, n in enumerate(sizes):
            mine = list(zip(begin[off[r]:off[r + 1]], ln[off[r]:off[r + 1]]))
            assert len(mine) == -(-n // L)                                     # no segment for an empty range
            assert [b for b, _ in mine] == [b0 + k * L for k in range(len(mine))]
            assert all(x == L for _, x in mine[:-1]) and sum(x for _, x in mine) == n and all(1 <= x <= L for _, x in mine)
            b0 += n


def test_header_forward_backward_block(driver, tmp_path):
    """one wave up to 64 positions, 256 threads from 65 on (tests/test_gpu_fb_scores.py runs 64 and 65 positions, alone and together)"""
    ns = [1, 2, 63, 64, 65, 66, 127, 128, 129, 255, 256, 257, 600, 8192]
    (a, c), = run_cases(driver, tmp_path, [["block", len(ns)] + ns])
    assert a == ("threads", [64 if n <= 64 else 256 for n in ns])
    # the transcripts' chains (tests/test_gpu_netocc_scores.py runs 64, 65, 256, 257 and 514 positions, and 10 with 300 in one group)
    assert c == ("chain_threads", [64 if n <= 64 else 256 if n <= 256 else 512 for n in ns])


def test_header_has_no_device_include():
    src = open(os.path.join(ROOT, "speechrecognition_amd", "csrc", "fb_plan.h")).read()
    assert "#include <hip" not in src and "handles.h" not in src
