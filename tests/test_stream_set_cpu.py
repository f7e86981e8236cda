"""The bookkeeping of a stream set without a GPU: speechrecognition_amd/csrc/stream_set_plan.h -- the slots and their ids, the
resolution of a call's id list, the window checks of a push, the layout of the stable and trim calls' pinned block -- compiled with
the host compiler alone into tests/cpp/stream_set_plan_driver, once plainly and once more under AddressSanitizer and UBSan, as a
stand-alone program.  Every answer is held against the plain-Python restatement below, which follows the definition of
include/srgpu.h: an id is slot + max_streams * generation, a fresh utterance takes the first free slot, the generation wraps before
the id leaves 32 bits; max_frames bounds the window (what an utterance has received since the last frame sr_stream_trim dropped),
2^32 - 1 the utterance."""
import os
import re
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "speechrecognition_amd", "csrc", "stream_set_plan.h")
U32 = 0xFFFFFFFF
GOOD, NOT_OPEN, TWICE = 0, 1, 2              # resolve_ids
OVER_MAX_FRAMES, OVER_UTTERANCE = 1, 2       # check_window
JOB_BYTES, RESULT_BYTES = (24, 32), 16       # StableJob, BigramStableJob; StableResult (kernels.h)
FRAME_BYTES = {24: 4, 32: 12}                # a word; a word, a score and a time


class Slots:
    """the restatement: the slots of a set"""

    def __init__(self, n):
        self.n, self.open, self.id, self.gen = n, [False] * n, [0] * n, [0] * n

    def begin(self):
        free = [s for s in range(self.n) if not self.open[s]]
        if not free:
            return None
        s = free[0]
        if s + self.n * self.gen[s] > U32:
            self.gen[s] = 0
        self.id[s] = s + self.n * self.gen[s]
        self.gen[s] += 1
        self.open[s] = True
        return s, self.id[s]

    def find(self, i):
        s = i % self.n
        return s if self.open[s] and self.id[s] == i else -1

    def resolve(self, ids):
        """-> (entry, fault, the slots of the entries before it)"""
        slots = []
        for k, i in enumerate(ids):
            s = self.find(i)
            if s < 0:
                return k, NOT_OPEN, slots
            if s in slots:
                return k, TWICE, slots
            slots.append(s)
        return len(ids), GOOD, slots


def window(max_frames, base, have, add):
    if have - base + add > max_frames:
        return OVER_MAX_FRAMES
    return OVER_UTTERANCE if have + add > U32 else GOOD


class Script:
    """commands for the driver, each with the answer the restatement gives"""

    def __init__(self):
        self.lines, self.want, self.sl = [], [], None

    def add(self, cmd, want):
        self.lines.append(cmd)
        self.want.append(want)

    def set(self, n, max_frames=10):
        self.sl = Slots(n)
        self.add(f"set {n} {max_frames}", "set")

    def begin(self):
        got = self.sl.begin()
        self.add("begin", "begin -1" if got is None else f"begin {got[0]} {got[1]}")
        return got

    def end(self, slot):
        self.sl.open[slot] = False
        self.add(f"end {slot}", "end")

    def gen(self, slot, g):
        self.sl.gen[slot] = g
        self.add(f"gen {slot} {g}", "gen")

    def find(self, i):
        got = self.sl.find(i)
        self.add(f"find {i}", f"find {got}")
        return got

    def resolve(self, ids):
        entry, fault, slots = self.sl.resolve(ids)
        for cmd in ("resolve", "resolve24"):  # into a plain array, and into the first field of records (as the job blocks' calls do)
            self.add(" ".join(str(v) for v in [cmd, len(ids)] + list(ids)), " ".join(str(v) for v in ["resolve", entry, fault] + slots))
        return entry, fault, slots

    def window(self, max_frames, base, have, add):
        got = window(max_frames, base, have, add)
        self.add(f"window {max_frames} {base} {have} {add}", f"window {got}")
        return got


def build(tmp, sanitized):
    exe = str(tmp / ("stream_set_plan_driver" + ("_san" if sanitized else "")))
    flags = ["-fsanitize=address,undefined", "-fno-sanitize-recover=all"] if sanitized else []
    subprocess.check_call(["g++", "-O1", "-std=c++17", "-Wall", "-Werror"] + flags +
                          ["-I" + os.path.join(ROOT, "speechrecognition_amd", "csrc"),
                           os.path.join(ROOT, "tests", "cpp", "stream_set_plan_driver.cpp"), "-o", exe])
    return exe


@pytest.fixture(scope="module")
def drivers(tmp_path_factory):
    tmp = tmp_path_factory.mktemp("streamset")
    exes = [build(tmp, san) for san in (False, True)]
    count = [0]

    def run(script):
        """the driver's answers to the script, which the plain and the sanitized build give alike and without a report"""
        count[0] += 1
        path = tmp / f"commands{count[0]}.txt"
        path.write_text("\n".join(script.lines) + "\n")
        outs = [subprocess.run([exe, str(path)], text=True, stdout=subprocess.PIPE, stderr=subprocess.STDOUT) for exe in exes]
        for o in outs:
            assert o.returncode == 0, o.stdout[-3000:]
        assert outs[0].stdout == outs[1].stdout and not re.search(r"runtime error|AddressSanitizer", outs[1].stdout)
        return outs[0].stdout.splitlines()

    return run


def test_ids_round_trip_and_slots_are_reused(drivers):
    sc = Script()
    sc.set(3)
    assert [sc.begin() for _ in range(4)] == [(0, 0), (1, 1), (2, 2), None]
    assert [sc.find(i) for i in (0, 1, 2, 3, 4)] == [0, 1, 2, -1, -1]
    sc.end(1)
    assert sc.find(1) == -1
    assert sc.begin() == (1, 4) and sc.find(4) == 1 and sc.find(1) == -1  # the slot's next generation; its last id is gone
    sc.end(0)
    sc.end(2)
    assert sc.begin() == (0, 3) and sc.begin() == (2, 5) and sc.begin() is None  # the first free slot first
    # ... and at random: begins, ends and finds of current, past and never-given ids
    rng = np.random.default_rng(5)
    for n in (1, 3, 5):
        sc.set(n)
        given = [0]
        for _ in range(300):
            op = rng.integers(0, 3)
            if op == 0:
                full = all(sc.sl.open)
                got = sc.begin()
                assert (got is None) == full
                if got:
                    assert got[1] % n == got[0] and got[1] not in given[1:]
                    given.append(got[1])
            elif op == 1:
                sc.end(int(rng.integers(0, n)))
            else:
                i = int(rng.choice(given)) if rng.random() < 0.8 else int(rng.integers(0, 40 * n))
                s = sc.find(i)
                assert s == -1 or (s == i % n and sc.sl.open[s] and sc.sl.id[s] == i)
        assert len(given) > 40
    assert drivers(sc) == sc.want


def test_the_generation_wraps_before_the_id_leaves_32_bits(drivers):
    sc = Script()
    sc.set(3)
    sc.gen(0, 1431655765)
    assert sc.begin() == (0, 4294967295)      # 0 + 3 * 1431655765: the last id of slot 0 that fits
    assert sc.begin() == (1, 1)
    sc.gen(2, 1431655764)
    assert sc.begin() == (2, 4294967294)      # 2 + 3 * 1431655764 likewise of slot 2
    assert sc.find(4294967295) == 0 and sc.find(4294967294) == 2
    sc.end(0)
    assert sc.begin() == (0, 0)               # 0 + 3 * 1431655766 = 2^32 + 2: generation 0 again
    assert sc.find(4294967295) == -1 and sc.find(0) == 0
    sc.end(2)
    assert sc.begin() == (2, 2)               # 2 + 3 * 1431655765 = 2^32 + 1
    assert sc.find(4294967294) == -1 and sc.find(2) == 2
    sc.end(0)
    assert sc.begin() == (0, 3)               # ... and on from there
    # one slot: every id up to 2^32 - 1 is given before the wrap
    sc.set(1)
    sc.gen(0, U32)
    assert sc.begin() == (0, U32)
    sc.end(0)
    assert sc.begin() == (0, 0) and sc.find(U32) == -1
    assert drivers(sc) == sc.want


def test_a_call_s_ids_resolve_up_to_the_first_offender(drivers):
    sc = Script()
    sc.set(4)
    ids = [sc.begin()[1] for _ in range(4)]
    sc.end(2)                                  # 2 was open once; 9 and 4000000000 never were
    a, b, c = ids[0], ids[1], ids[3]
    assert sc.resolve([]) == (0, GOOD, [])
    assert sc.resolve([c, a, b]) == (3, GOOD, [3, 0, 1])
    assert sc.resolve([a, 9, b]) == (1, NOT_OPEN, [0])
    assert sc.resolve([2]) == (0, NOT_OPEN, [])
    assert sc.resolve([b, c, 4000000000]) == (2, NOT_OPEN, [1, 3])
    assert sc.resolve([a, a]) == (1, TWICE, [0])
    assert sc.resolve([b, c, a, c]) == (3, TWICE, [1, 3, 0])
    # both in one list: whichever stands first
    assert sc.resolve([a, a, 9]) == (1, TWICE, [0])
    assert sc.resolve([a, 9, a]) == (1, NOT_OPEN, [0])
    assert sc.resolve([9, 9]) == (0, NOT_OPEN, [])
    sc.begin()                                 # slot 2's next utterance: id 6, and 2 stays gone
    assert sc.resolve([6, 2]) == (1, NOT_OPEN, [2])
    assert sc.resolve([6, a, 6]) == (2, TWICE, [2, 0])
    assert drivers(sc) == sc.want


def test_the_window_is_held_against_max_frames_and_the_utterance_against_32_bits(drivers):
    sc = Script()
    for base in (0, 7):
        # an utterance with 5 rows in its window (have = base + 5) and max_frames 9: 3, 4 and 5 rows more
        assert [sc.window(9, base, base + 5, add) for add in (3, 4, 5)] == [GOOD, GOOD, OVER_MAX_FRAMES]
        # ... an empty window, and a full one
        assert [sc.window(9, base, base, add) for add in (8, 9, 10)] == [GOOD, GOOD, OVER_MAX_FRAMES]
        assert [sc.window(9, base, base + 9, add) for add in (0, 1)] == [GOOD, OVER_MAX_FRAMES]
        # a window with room to spare: the utterance ends one below, at and one above 2^32 - 1 rows
        have = U32 - 100
        wide = base + (1 << 33)
        assert [sc.window(wide, base, have, add) for add in (99, 100, 101)] == [GOOD, GOOD, OVER_UTTERANCE]
        # over both: the window answers
        assert sc.window(U32 - 50, base, have, 101) == OVER_MAX_FRAMES
        # a count no 64-bit sum holds
        assert sc.window(9, base, base + 5, (1 << 64) - 1) == OVER_MAX_FRAMES
        # the audio push's form: `made` frames of which `base` are dropped, as have = base, add = made - base
        for made, want in ((base + 8, GOOD), (base + 9, GOOD), (base + 10, OVER_MAX_FRAMES)):
            assert sc.window(9, base, base, made - base) == want == (OVER_MAX_FRAMES if made - base > 9 else GOOD)
        for made, want in ((U32 - 1, GOOD), (U32, GOOD), (U32 + 1, OVER_UTTERANCE)):
            assert sc.window(wide, base, base, made - base) == want
    assert drivers(sc) == sc.want


def test_the_block_s_areas_follow_each_other_and_grow_geometrically(drivers):
    sc = Script()
    cases = [(job, n, F) for job in JOB_BYTES for n in (0, 1, 3) for F in ((0,) if n == 0 else (0, 1, 77, 1 << 33))]
    for job, n, F in cases:
        sc.add(f"layout {job} {RESULT_BYTES} {FRAME_BYTES[job]} {n} {F}", None)
    grows = [(0, 0), (1, 0), (100, 100), (101, 100), (200, 100), (201, 100), (5000, 100)]
    for need, have in grows:
        sc.add(f"grown {need} {have}", None)
    got = drivers(sc)
    assert len(got) == len(cases) + len(grows)
    for (job, n, F), line in zip(cases, got):
        f = line.split()
        assert f[0] == "layout"
        res_at, items_at, need = (int(v) for v in f[1:])
        # the jobs from 0, the results behind them, the items behind those, nothing between and nothing after
        assert res_at == job * n and items_at - res_at == RESULT_BYTES * n and need - items_at == FRAME_BYTES[job] * F, (job, n, F)
        assert 0 <= res_at <= items_at <= need == job * n + RESULT_BYTES * n + FRAME_BYTES[job] * F
        assert res_at % 8 == 0 and items_at % 8 == 0  # the results and the items stay aligned for their 4-byte fields
    for (need, have), line in zip(grows, got[len(cases):]):
        size = int(line.split()[1])
        assert size >= max(need, have) and size == (have if need <= have else max(need, 2 * have)), (need, have)


def test_the_header_is_free_of_hip_and_handles():
    src = open(HEADER).read()
    assert "#include <hip" not in src and "handles.h" not in src and "kernels.h" not in src and "__device__" not in src
    handles = open(os.path.join(ROOT, "speechrecognition_amd", "csrc", "handles.h")).read()
    assert '#include "stream_set_plan.h"' in handles and "struct StreamSlots" not in handles
