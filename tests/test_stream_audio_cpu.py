"""Streaming from audio without a GPU: the bookkeeping of one utterance, speechrecognition_amd/csrc/stream_audio_plan.h, compiled with
the host compiler alone into tests/cpp/stream_audio_plan_driver -- once plainly and once more under AddressSanitizer and UBSan, as a
stand-alone program -- against the definition of include/srgpu.h: whatever the cut, the rows come out once each and in order, none
before the static `step` frames ahead of it exists, every new frame's samples reach the device with the sample before them, and the
host carries fewer than `window` samples.  Then the causal energy maximum of tests/stream_audio_reference.py against the batch rule."""
import os
import re
import subprocess

import numpy as np
import pytest

from tests import frontend_reference as R
from tests import stream_audio_reference as SR

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PARAMS = [(400, 160, 3), (64, 32, 2), (64, 80, 3)]          # window, shift, step; the last: shift > window
FRAMES = [0, 1, 2, 3, 4, 7, 50]
MODES = ["whole", "shift", "one", "37", "random", "16000"]


def frames_of(n, window, shift):
    return 0 if n < window else 1 + (n - window) // shift


def cuts_of(mode, n, shift, rng):
    if mode == "whole":
        return [n]
    if mode == "random":
        out = []
        while sum(out) < n:
            out.append(min(int(rng.integers(1, 1001)), n - sum(out)))
        return out
    k = {"shift": shift, "one": 1, "37": 37, "16000": 16000}[mode]
    return [min(k, n - a) for a in range(0, n, k)]


def all_cases():
    rng = np.random.default_rng(11)
    cases = []
    for window, shift, step in PARAMS:
        lengths = [window - 1 if T == 0 else window + (T - 1) * shift + (T * 13) % shift for T in FRAMES] + [16000, 0]
        for n in lengths:
            for mode in MODES:
                cases.append(dict(window=window, shift=shift, step=step, n=n, mode=mode, cuts=cuts_of(mode, n, shift, rng)))
    return cases


def build(tmp, sanitized):
    exe = str(tmp / ("stream_audio_plan_driver" + ("_san" if sanitized else "")))
    flags = ["-fsanitize=address,undefined", "-fno-sanitize-recover=all"] if sanitized else []
    subprocess.check_call(["g++", "-O1", "-std=c++17", "-Wall", "-Werror"] + flags +
                          ["-I" + os.path.join(ROOT, "speechrecognition_amd", "csrc"),
                           os.path.join(ROOT, "tests", "cpp", "stream_audio_plan_driver.cpp"), "-o", exe])
    return exe


@pytest.fixture(scope="module")
def answers(tmp_path_factory):
    """the driver's output on every case, from the plain and from the sanitized build"""
    tmp = tmp_path_factory.mktemp("streamaudio")
    cases = all_cases()
    path = tmp / "cases.txt"
    path.write_text("".join(" ".join(str(v) for v in [c["window"], c["shift"], c["step"], len(c["cuts"])] + c["cuts"]) + "\n" for c in cases))
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
        cur.append(dict(row0=v[0], rows=v[1], S=v[2], k=v[3], carry=v[4], skip=v[5], ok=v[6], starts=v[7:], prevs=[int(x) for x in tail.split()]))
    assert not cur
    return out


def test_the_sanitized_build_runs_clean_and_agrees(answers):
    cases, plain, san = answers
    assert plain == san and not re.search(r"runtime error|AddressSanitizer", san)
    assert len(parse(plain)) == len(cases)


def test_the_steps_do_not_depend_on_the_cut(answers):
    cases, plain, _ = answers
    seen_modes = set()
    for c, steps in zip(cases, parse(plain)):
        window, shift, step, n = c["window"], c["shift"], c["step"], c["n"]
        T = frames_of(n, window, shift)
        assert len(steps) == len(c["cuts"]) + 1, c
        got_n, rows_done, S = 0, 0, 0
        for i, s in enumerate(steps):
            finish = i == len(c["cuts"])
            got_n += 0 if finish else c["cuts"][i]
            # the statics follow the samples received, whatever the pieces were
            assert s["S"] == S and S + s["k"] == frames_of(got_n, window, shift), (c, i)
            # every new frame's samples, and the one before its first, are in the upload
            assert s["ok"] == 1 and s["starts"] == [(S + j) * shift for j in range(s["k"])], (c, i)
            assert s["prevs"] == [0 if (S + j) * shift == 0 else (S + j) * shift - 1 - 20000 for j in range(s["k"])], (c, i)
            S += s["k"]
            # rows: in order, once each; before the finish exactly those whose static `step` ahead exists
            assert s["row0"] == rows_done, (c, i)
            rows_done += s["rows"]
            assert rows_done == SR.rows_out(S, step, finish), (c, i)
            # the carry: fewer than `window` samples (plus the previous one, kept apart); a gap only where shift > window
            assert s["carry"] < window and (s["skip"] == 0 or (shift > window and s["carry"] == 0)), (c, i)
            assert s["carry"] == max(got_n - S * shift, 0) and s["skip"] == max(S * shift - got_n, 0), (c, i)
        assert S == T and rows_done == T, c
        if T:
            seen_modes.add(c["mode"])
    assert seen_modes == set(MODES)
    want_T = {(p, T) for p in PARAMS for T in FRAMES}
    assert want_T <= {((c["window"], c["shift"], c["step"]), frames_of(c["n"], c["window"], c["shift"])) for c in cases}


def no_max_rows(rng, T, step, mean=None, stddev=None):
    cep = (rng.normal(size=(T, 12)) * np.linspace(20.0, 1.0, 12)[None]).astype(np.float32)
    return cep, lambda c: R.post_process(c, 12, 1, step, mean, stddev, False)


@pytest.mark.parametrize("step", [2, 3])
def test_the_causal_maximum_is_the_batch_s_when_the_maximum_comes_early(step):
    rng = np.random.default_rng(step)
    mean, stddev = rng.normal(size=25), rng.uniform(0.5, 3.0, size=25)
    for T in (1, 2, 3, 4, 7, 50):
        for where in range(min(step + 1, T)):
            cep, post = no_max_rows(rng, T, step, mean, stddev)
            cep[where, 0] = np.abs(cep[:, 0]).max() + np.float32(1.0)
            if T > where + 1:
                cep[-1, 0] = cep[where, 0]            # the maximum again later: the first one still wins
            rows = post(cep)
            assert int(np.argmax(rows[:, 0])) == where
            got = SR.causal_max(rows, step)
            assert np.array_equal(got.view(np.uint32), SR.batch_max(rows).view(np.uint32))
            assert np.array_equal(got.view(np.uint32), R.post_process(cep, 12, 1, step, mean, stddev, True).view(np.uint32))
    # a maximum of zero, -0 first: the batch keeps -0, and so does the causal rule
    cep, post = no_max_rows(rng, 6, step)
    cep[:, 0] = [-0.0, 0.0, -1.0, 0.0, -2.0, -0.0]
    rows = post(cep)
    assert np.array_equal(SR.causal_max(rows, step).view(np.uint32), SR.batch_max(rows).view(np.uint32))


def test_the_causal_maximum_differs_when_the_maximum_comes_late():
    rng = np.random.default_rng(9)
    step = 3
    cep, post = no_max_rows(rng, 20, step)
    cep[:, 0] = np.arange(20, dtype=np.float32)      # rising: the maximum is the last frame
    rows = post(cep)
    got, batch = SR.causal_max(rows, step), SR.batch_max(rows)
    # row t has seen frames 0 .. t + 3: it subtracts t + 3 where the batch subtracts 19
    assert np.array_equal(got[:, 0], np.float32([-min(3, 19 - t) for t in range(20)]))
    assert np.array_equal(batch[:, 0], np.arange(20, dtype=np.float32) - 19)
    assert not np.array_equal(got[:16, 0], batch[:16, 0]) and np.array_equal(got[16:], batch[16:])
    assert np.array_equal(got[:, 1:].view(np.uint32), batch[:, 1:].view(np.uint32))


def test_the_header_declares_the_entry_points_and_the_binding_lists_them():
    from speechrecognition_amd import capi
    hdr = open(os.path.join(ROOT, "include", "srgpu.h")).read()
    assert re.search(r"#define\s+SR_ABI_VERSION\s+4\b", hdr)   # entry points more, no struct changed
    for kind in ("sr_stream", "sr_bigram_stream"):
        for fn in ("_set_frontend", "_push_audio", "_finish_audio"):
            assert re.search(r"SR_API int " + kind + fn + r"\(", hdr) and kind + fn in capi.SYMBOLS
    assert "NOT the batch's value" in hdr
    for cls in (capi.Stream, capi.BigramStream):
        assert all(hasattr(cls, f) for f in ("set_frontend", "push_audio", "finish_audio"))
