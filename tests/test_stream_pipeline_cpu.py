"""The streaming pipeline without a GPU: the bookkeeping of one utterance, speechrecognition_amd/csrc/stream_pipeline_plan.h, compiled
with the host compiler alone into tests/cpp/stream_pipeline_plan_driver -- once plainly and once more under AddressSanitizer and UBSan,
as a stand-alone program -- against the definition of include/srgpu.h: whatever the cut, the rows come out once each and in order,
none before input row t + context exists, every part of a spliced row is the clamped input row the definition names, and the history
never exceeds 2 context rows.  Then the numpy restatement of both stages (tests/stream_pipeline_reference.py) against the batch
references of the projection and the transform, and streaming by any cut against the whole utterance."""
import os
import re
import subprocess

import numpy as np
import pytest

from tests import fmllr_reference as FR
from tests import lda_reference as LR
from tests import stream_pipeline_reference as PR

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CONTEXTS = [0, 1, 2, 4]
FRAMES = [0, 1, 2, 3, 4, 7, 50]
MODES = ["whole", "one", "37", "random"]


def cuts_of(mode, n, rng):
    if mode == "whole":
        return [n]
    if mode == "random":
        out = []
        while sum(out) < n:
            out.append(min(int(rng.integers(0, 9)), n - sum(out)))     # (empty pushes among them)
        return out
    k = {"one": 1, "37": 37}[mode]
    return [min(k, n - a) for a in range(0, n, k)]


def all_cases():
    rng = np.random.default_rng(12)
    return [dict(c=c, T=T, mode=mode, with_rows=with_rows, cuts=cuts_of(mode, T, rng))
            for c in CONTEXTS for T in FRAMES for mode in MODES for with_rows in (0, 1)]


def build(tmp, sanitized):
    exe = str(tmp / ("stream_pipeline_plan_driver" + ("_san" if sanitized else "")))
    flags = ["-fsanitize=address,undefined", "-fno-sanitize-recover=all"] if sanitized else []
    subprocess.check_call(["g++", "-O1", "-std=c++17", "-Wall", "-Werror"] + flags +
                          ["-I" + os.path.join(ROOT, "speechrecognition_amd", "csrc"),
                           os.path.join(ROOT, "tests", "cpp", "stream_pipeline_plan_driver.cpp"), "-o", exe])
    return exe


@pytest.fixture(scope="module")
def answers(tmp_path_factory):
    """the driver's output on every case, from the plain and from the sanitized build"""
    tmp = tmp_path_factory.mktemp("streampipeline")
    cases = all_cases()
    path = tmp / "cases.txt"
    path.write_text("".join(" ".join(str(v) for v in [c["c"], c["with_rows"], len(c["cuts"])] + c["cuts"]) + "\n" for c in cases))
    outs = [subprocess.run([build(tmp, san), str(path)], text=True, stdout=subprocess.PIPE, stderr=subprocess.STDOUT) for san in (False, True)]
    for o in outs:
        assert o.returncode == 0, o.stdout[-3000:]
    return cases, outs[0].stdout, outs[1].stdout


def parse(text):
    out, cur = [], []
    for ln in text.splitlines():
        if ln == "end":
            out.append(cur)
            cur = []
            continue
        head, tail = ln.split("|")
        f = head.split()
        assert f[0] == "step"
        v = [int(x) for x in f[1:]]
        rows = [(int(r.split(":")[0]), [int(x) for x in r.split(":")[1].split(",")]) for r in tail.split()]
        cur.append(dict(row0=v[0], rows=v[1], R=v[2], k=v[3], hist=v[4], need0=v[5], need1=v[6], keep0=v[7], hist_after=v[8], out=rows))
    assert not cur
    return out


def test_the_sanitized_build_runs_clean_and_agrees(answers):
    cases, plain, san = answers
    assert plain == san and not re.search(r"runtime error|AddressSanitizer", san)
    assert len(parse(plain)) == len(cases)


def test_the_steps_do_not_depend_on_the_cut(answers):
    cases, plain, _ = answers
    seen = set()
    for case, steps in zip(cases, parse(plain)):
        c, T, cuts = case["c"], case["T"], case["cuts"]
        assert len(steps) == (len(cuts) if case["with_rows"] and cuts else len(cuts) + 1), case
        R, done = 0, 0
        for i, s in enumerate(steps):
            finish = i == len(steps) - 1
            k = cuts[i] if i < len(cuts) else 0
            assert s["R"] == R and s["k"] == k and s["hist"] == min(R, 2 * c), (case, i)
            R += k
            # rows: in order, once each; before the finish exactly those whose input row `context` ahead exists
            assert s["row0"] == done and [t for t, _ in s["out"]] == list(range(done, done + s["rows"])), (case, i)
            done += s["rows"]
            assert done == PR.rows_out(R, c, finish) == (T if finish else max(R - c, 0)), (case, i)
            if not finish:
                assert all(t + c <= R - 1 for t, _ in s["out"]), (case, i)
            # every part of a spliced row is the input row the definition names, with the clamps of the utterance's T
            for t, parts in s["out"]:
                assert parts == [min(max(t + o, 0), T - 1) for o in range(-c, c + 1)], (case, i, t)
            # the history: never more than 2 context rows, and only new rows are written into it
            assert s["hist_after"] == min(R, 2 * c) <= 2 * c and s["keep0"] == max(R - 2 * c, R - k), (case, i)
            if s["rows"]:
                assert s["need0"] == max(s["row0"] - c, 0) >= R - k - s["hist"] and s["need1"] == min(done - 1 + c, R - 1) + 1, (case, i)
        assert R == T and done == T, case
        if T:
            seen.add((c, case["mode"], case["with_rows"]))
    assert seen == {(c, m, w) for c in CONTEXTS for m in MODES for w in (0, 1)}


def random_case(rng, D, c, p, T):
    x = (rng.normal(size=(T, D)) * 3.0).astype(np.float32)
    M = rng.normal(size=(p, (2 * c + 1) * D + 1))
    W = np.hstack([np.eye(p) + 0.2 * rng.normal(size=(p, p)), rng.normal(size=(p, 1))])
    return x, M, W


@pytest.mark.parametrize("D,c,p", [(3, 0, 2), (3, 1, 3), (5, 2, 4), (7, 4, 6)])
def test_the_reference_restates_the_batch_references(D, c, p):
    rng = np.random.default_rng(100 + D)
    lens = [1, 2, 3, 9, 20]
    off = np.concatenate([[0], np.cumsum(lens)]).astype(np.uint64)
    x, M, _ = random_case(rng, D, c, p, int(off[-1]))
    Ws = np.stack([random_case(rng, D, c, p, 1)[2] for _ in lens])
    y = LR.project(x, off, c, M)
    z = FR.transform(y, off, np.arange(len(lens)), Ws)
    for u in range(len(lens)):
        a, b = int(off[u]), int(off[u + 1])
        assert np.array_equal(PR.whole(x[a:b], c, M, None).view(np.uint32), y[a:b].view(np.uint32)), u
        assert np.array_equal(PR.whole(x[a:b], c, M, Ws[u]).view(np.uint32), z[a:b].view(np.uint32)), u
        assert np.array_equal(PR.whole(y[a:b], 0, None, Ws[u]).view(np.uint32), z[a:b].view(np.uint32)), u


@pytest.mark.parametrize("c", CONTEXTS)
def test_streaming_by_any_cut_gives_the_whole_utterance_s_rows(c):
    rng = np.random.default_rng(200 + c)
    D, p = 4, 3
    for T in FRAMES:
        x, M, W = random_case(rng, D, c, p, T)
        for use_w in (None, W):
            want = PR.whole(x, c, M, use_w)
            assert want.shape == (T, p)
            for mode in MODES:
                for with_rows in (0, 1):
                    cuts = cuts_of(mode, T, rng)
                    s = PR.Streamed(c, M, use_w)
                    got, at = [], 0
                    for i, k in enumerate(cuts):
                        got.append(s.push(x[at:at + k], finish=bool(with_rows) and i == len(cuts) - 1))
                        at += k
                    if not s.finished:
                        got.append(s.push(x[:0], finish=True))
                    got = np.concatenate(got)
                    assert s.max_history <= 2 * c
                    assert got.shape == want.shape and np.array_equal(got.view(np.uint32), want.view(np.uint32)), (T, mode, with_rows)
    # without a projection there is no delay: every push gives its own rows back
    s = PR.Streamed(3, None, W)
    y = rng.normal(size=(5, p)).astype(np.float32)
    assert np.array_equal(s.push(y[:2]).view(np.uint32), PR.whole(y, 0, None, W)[:2].view(np.uint32)) and s.searched == 2


def test_the_header_declares_the_entry_points_and_the_binding_lists_them():
    from speechrecognition_amd import capi
    hdr = open(os.path.join(ROOT, "include", "srgpu.h")).read()
    assert re.search(r"#define\s+SR_ABI_VERSION\s+4\b", hdr)   # entry points more, no struct changed
    for kind in ("sr_stream", "sr_bigram_stream"):
        for fn in ("_set_projection", "_set_transform", "_push_rows"):
            assert re.search(r"SR_API int " + kind + fn + r"\(", hdr) and kind + fn in capi.SYMBOLS
    for cls in (capi.Stream, capi.BigramStream):
        assert all(hasattr(cls, f) for f in ("set_projection", "set_transform", "push_rows"))
    mirror = open(os.path.join(ROOT, "include", "sr_sietill.hpp")).read()
    for kind in ("sr_stream", "sr_bigram_stream"):
        for fn in ("_set_projection", "_set_transform", "_push_rows"):
            assert kind + fn + "(s_" in mirror
