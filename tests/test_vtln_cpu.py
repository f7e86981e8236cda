"""VTLN without a GPU: the filters' table builder, the checks of sr_vtln_params and sr_vtln_choose's rule -- all host code of
speechrecognition_amd/csrc/vtln_tables.h -- compiled with the host compiler alone into tests/cpp/vtln_tables_driver, once plainly and
once under AddressSanitizer and UBSan, and run as a stand-alone program, against tests/vtln_reference.py: over the three parameter
sets of the front end's tests and 13 warps the weights lie within 1e-6 of the reference's, a filter's bins of positive weight are one
run, the table of alpha == 1.0 is byte for byte the unwarped builder's, and the warp is continuous at its break point, monotone and
fixes f_high.  Then the refusals, a warp that empties a filter among them, and the choice of a warp."""
import os
import re
import subprocess

import numpy as np
import pytest

from tests import frontend_reference as R
from tests import vtln_reference as V

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
# the parameter sets of tests/test_gpu_frontend.py
MFCC16 = R.params(preemphasis=0.9)
MFCC8 = R.params(preemphasis=0.9, sample_rate=8000.0, window=200, shift=80, n_fft=256, n_mel=20, n_cepstra=13, f_low=100.0, f_high=4000.0)
MFCC64 = R.params(preemphasis=0.9, window=64, shift=32, n_fft=64, n_mel=6, n_cepstra=6, f_low=1000.0, f_high=8000.0)
SETS = [MFCC16, MFCC8, MFCC64]
EMPTIES = R.params(n_fft=64, window=64, shift=32, n_mel=40, n_cepstra=12)   # 40 filters on 33 bins: a filter without a bin
# 14 filters on 33 bins: the unwarped bank is fine, and a warp (alpha = 1.12) leaves filter 0 without a bin
EMPTIED = R.params(n_fft=64, window=64, shift=32, n_mel=14, n_cepstra=6, f_low=0.0, f_high=8000.0)
WARP_CASES =[(a, fh, V.BREAK) for a in V.ALPHAS for fh in (8000.0, 4000.0)] + [(0.5, 8000.0, 0.3), (2.0, 8000.0, 0.99)]
CHOOSE = [
    # n_warps, min_frames, fallback, cost rows, frames -> (the reference answers)
    (3, 0, 1, [[5.0, 4.0, 4.0], [4.0, 4.0, 5.0], [7.0, 8.0, 6.0]], [10, 10, 10]),          # ties go to the first warp
    (3, 11, 2, [[5.0, 4.0, 6.0], [1.0, 2.0, 3.0]], [10, 11]),                              # min_frames
    (3, 0, 2, [[float("nan"), 4.0, 6.0], [5.0, float("nan"), 1.0], [float("nan")] * 3], [10, 10, 10]),
    (3, 0, 1, [[float("inf")] * 3, [float("inf"), 3.0, float("inf")], [float("-inf"), 3.0, 1.0]], [10, 10, 10]),
    (1, 0, 0, [[3.0], [float("inf")]], [0, 5]),
    (2, 1, 1, [[0.0, 0.0]], [0]),                                                          # a speaker without frames
]


def build(tmp, sanitized):
    exe = str(tmp / ("vtln_tables_driver" + ("_san" if sanitized else "")))
    flags = ["-fsanitize=address,undefined", "-fno-sanitize-recover=all"] if sanitized else []
    subprocess.check_call(["g++", "-O1", "-std=c++17", "-Wall", "-Werror"] + flags +
                          ["-I" + os.path.join(ROOT, "speechrecognition_amd", "csrc"),
                           os.path.join(ROOT, "tests", "cpp", "vtln_tables_driver.cpp"), "-o", exe])
    return exe


def num(x):
    return repr(float(x))


def warp_points(alpha, f_high, brk):
    f0 = brk * f_high * min(1.0, 1.0 / alpha)
    grid = np.linspace(0.0, f_high, 257)
    return np.concatenate([grid, [np.nextafter(f0, 0.0), f0, np.nextafter(f0, np.inf)]])


def commands():
    lines = []
    for p in SETS + [EMPTIES, EMPTIED]:
        lines.append(" ".join(["tables", num(p["sample_rate"]), str(p["n_fft"]), str(p["n_mel"]), num(p["f_low"]), num(p["f_high"]), num(V.BREAK),
                               str(len(V.ALPHAS))] + [num(a) for a in V.ALPHAS]))
    for alpha, fh, brk in WARP_CASES:
        pts = warp_points(alpha, fh, brk)
        lines.append(" ".join(["warp", num(alpha), num(fh), num(brk), str(len(pts))] + [num(f) for f in pts]))
    for n_mel, brk, alphas in CHECKS:
        lines.append(" ".join(["check", str(n_mel), num(brk), str(len(alphas))] + [num(a) for a in alphas]))
    for case in LDS:
        lines.append("lds " + " ".join(str(v) for v in case))
    for W, mn, fb, rows, frames in CHOOSE:
        lines.append(" ".join(["choose", str(len(rows)), str(W), str(mn), str(fb)] + [num(c) for r in rows for c in r] + [str(f) for f in frames]))
    return "\n".join(lines) + "\n"


nan, inf = float("nan"), float("inf")
CHECKS = [
    # n_mel, break_frac, alphas -> code
    (24, 0.875, V.ALPHAS), (40, 0.875, V.ALPHAS), (32, 0.5, [1.0] * 32), (64, 0.5, [1.0] * 16),
    (24, 0.875, []), (24, 0.875, [1.0, 0.0]), (24, 0.875, [-1.0]), (24, 0.875, [nan]), (24, 0.875, [inf]),
    (24, 0.0, [1.0]), (24, 1.0, [1.0]), (24, nan, [1.0]), (24, -0.5, [1.0]), (24, 1.5, [1.0]),
    (24, 0.875, [1.0] * 33), (64, 0.875, [1.0] * 17), (40, 0.875, [1.0] * 26),
]
CHECK_CODES = [0, 0, 0, 0, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 2, 2, 2]
# the warp search kernel's LDS rule (vtln_tables.h: mfcc_warps_waves, mfcc_warps_lds_bytes): y_floats -- the span's samples, at most the
# span cap of 4096 -- n_fft, n_warps, n_mel.  The first: 16 frames of 400 / 160 (2800 samples), 512 / 13 warps / 24 filters
LDS = [(2800, 512, 13, 24), (2800, 512, 13, 40)] + [(y, n_fft, w, m) for y in (64, 2800, 4096) for n_fft in (64, 256, 512, 1024, 2048)
                                                    for w, m in ((1, 1), (13, 24), (13, 40), (32, 32), (16, 64))]


@pytest.fixture(scope="module")
def answers(tmp_path_factory):
    tmp = tmp_path_factory.mktemp("vtln")
    path = tmp / "commands.txt"
    path.write_text(commands())
    outs = [subprocess.run([build(tmp, san), str(path)], text=True, stdout=subprocess.PIPE, stderr=subprocess.STDOUT) for san in (False, True)]
    for o in outs:
        assert o.returncode == 0, o.stdout[-3000:]
    return outs[0].stdout, outs[1].stdout


def parse(text):
    """-> tables: per `tables` command {warp: {filter: (first, count, off, f32 weights)}}, its empties [(warp, filter)], unwarped_equal;
    warps: the g rows; checks; chosen"""
    tables, warps, checks, chosen = [], [], [], []
    cur = dict(warps={}, empty=[], equal=None)
    a = None
    for ln in text.splitlines():
        f = ln.split()
        if f[0] == "warp":
            a = int(f[1])
            cur["warps"][a] = {}
        elif f[0] == "filter":
            w = np.array([int(x, 16) for x in f[5:]], dtype=np.uint32).view(np.float32)
            assert len(w) == int(f[3])
            cur["warps"][a][int(f[1])] = (int(f[2]), int(f[3]), int(f[4]), w)
        elif f[0] == "empty":
            cur["empty"].append((int(f[1]), int(f[2])))
        elif f[0] == "unwarped_equal":
            cur["equal"] = int(f[1])
            tables.append(cur)
            cur = dict(warps={}, empty=[], equal=None)
        elif f[0] == "g":
            warps.append(np.array([float.fromhex(x) for x in f[1:]]))
        elif f[0] == "check":
            checks.append(int(f[1]))
        elif f[0] == "chosen":
            chosen.append([int(x) for x in f[1:]])
    return tables, warps, checks, chosen


def test_the_lds_rule_keeps_two_workgroups_on_a_cu(answers):
    """the constexpr functions the launch of mfcc_warps_kernel uses, through the driver: a workgroup takes at most 64 KiB -- what a launch
    gets without opting in -- so two fit a CU's 160 KiB, and the headline shape keeps four waves in 32 704 bytes"""
    rows = [[int(x) for x in ln.split()[1:]] for ln in answers[0].splitlines() if ln.startswith("lds ")]
    assert len(rows) == len(LDS)
    for (y, n_fft, w, m), (base, waves, size, cap) in zip(LDS, rows):
        pairs = (w * m + 63) // 64 * 64
        assert cap == 4096 and base == (4 if n_fft <= 1024 else 2) and 1 <= waves <= base and (waves == base or waves * 2 == base or waves * 4 == base)
        assert size == 4 * (y + waves * (2 * n_fft + pairs)) and size <= 65536 and 2 * size <= 160 * 1024, (y, n_fft, w, m)
        # no wave given up without need: the next larger count would not have fitted
        assert waves == base or 4 * (y + 2 * waves * (2 * n_fft + pairs)) > 65536
    assert rows[0][1:3] == [4, 32704] and rows[1][1:3] == [4, 36800]
    assert rows[LDS.index((4096, 1024, 32, 32))][1:3] == [4, 65536] and rows[LDS.index((4096, 2048, 16, 64))][1:3] == [2, 57344]


def test_the_sanitized_build_runs_clean_and_agrees(answers):
    plain, san = answers
    assert plain == san and not re.search(r"runtime error|AddressSanitizer", san)


def test_the_reference_s_identity_filters_are_the_front_end_reference_s():
    for p in SETS:
        assert np.array_equal(V.filters(p, 1.0, V.BREAK).view(np.uint32), R.tables(p)[2].view(np.uint32))
        assert V.ALPHAS[6] == 1.0 and len(V.ALPHAS) == 13 and V.ALPHAS[0] == 0.88 and V.ALPHAS[-1] == 1.12


@pytest.mark.parametrize("i", range(3), ids=["16k-400-512", "8k-200-256", "16k-64-64"])
def test_the_tables_match_the_reference(answers, i):
    p = SETS[i]
    t = parse(answers[0])[0][i]
    bins = p["n_fft"] // 2 + 1
    assert t["equal"] == 1 and not t["empty"] and sorted(t["warps"]) == list(range(13))
    for a, alpha in enumerate(V.ALPHAS):
        want = V.filters(p, alpha, V.BREAK)
        off = 0
        assert sorted(t["warps"][a]) == list(range(p["n_mel"]))
        for m in range(p["n_mel"]):
            first, count, o, w = t["warps"][a][m]
            assert o == off and count >= 1 and first + count <= bins
            off += count
            dense = np.zeros(bins, dtype=np.float32)
            dense[first:first + count] = w
            assert np.abs(dense.astype(np.float64) - want[m].astype(np.float64)).max() <= 1e-6, (alpha, m)
            # the support is one run: the reference's positive bins are exactly first .. first + count - 1, up to weights below 1e-6
            pos = np.nonzero(want[m] > 1e-6)[0]
            assert len(pos) and np.array_equal(pos, np.arange(pos[0], pos[-1] + 1)) and first <= pos[0] and pos[-1] < first + count
            assert w[0] > 0.0 and w[-1] > 0.0
        if alpha == 1.0:   # the unwarped table, bit for bit
            for m in range(p["n_mel"]):
                first, count, _, w = t["warps"][a][m]
                ref = R.tables(p)[2][m]
                assert np.array_equal(w.view(np.uint32), ref[first:first + count].view(np.uint32)) and not ref[:first].any() and not ref[first + count:].any()


@pytest.mark.parametrize("i", [3, 4], ids=["40-filters", "14-filters"])
def test_a_warp_that_empties_a_filter_is_reported(answers, i):
    p = [EMPTIES, EMPTIED][i - 3]
    t = parse(answers[0])[0][i]
    want = {(a, int(np.nonzero(~(V.filters(p, alpha, V.BREAK) > 0).any(axis=1))[0][0])) for a, alpha in enumerate(V.ALPHAS)
            if not (V.filters(p, alpha, V.BREAK) > 0).any(axis=1).all()}
    assert want and set(t["empty"]) == want and t["equal"] == 1
    for a, m in t["empty"]:
        assert sorted(t["warps"][a]) == list(range(m))   # the filters before it, nothing after
    if i == 4:   # the unwarped bank and most warps are complete; only alpha = 1.12 loses a filter
        assert want == {(12, 0)} and len(t["warps"][6]) == 14


def test_the_warp_is_continuous_monotone_and_fixes_f_high(answers):
    rows = parse(answers[0])[1]
    assert len(rows) == len(WARP_CASES)
    for (alpha, fh, brk), g in zip(WARP_CASES, rows):
        pts = warp_points(alpha, fh, brk)
        want = V.warp(pts, alpha, fh, brk)
        assert np.abs(g - want).max() <= 1e-9 * fh
        grid, (below, at, above) = g[:257], g[257:]
        # g(0) = 0 and g(f_high) == f_high, exactly, for the 13 alphas at break 0.875 and both values of f_high.  The two further
        # cases are outside that set: evaluated in double as written -- a = alpha f0, x = f_high - a, y = f_high - f0, a + (x / y) y
        # -- the formula carries the roundings of x (half an ulp of f_high at most), of the quotient and the product (2^-53 of x
        # each) and of the last addition, so there the bound is 2 ulp of f_high (alpha 0.5, break 0.3 gives 8000 - 1 ulp).
        assert grid[0] == 0.0
        if alpha in V.ALPHAS and brk == V.BREAK:
            assert grid[-1] == fh, (alpha, fh)
        else:
            assert abs(grid[-1] - fh) <= 2.0 * np.spacing(fh), (alpha, fh, brk)
        assert (np.diff(grid) > 0.0).all()                           # monotone
        assert below <= at <= above and above - below <= 1e-9 * fh   # continuous at the break point
        if alpha == 1.0:
            assert np.array_equal(g, pts)                             # the identity, no arithmetic


def test_the_refusals(answers):
    assert parse(answers[0])[2] == CHECK_CODES


def test_choose(answers):
    got = parse(answers[0])[3]
    assert len(got) == len(CHOOSE)
    for (W, mn, fb, rows, frames), g in zip(CHOOSE, got):
        assert g == V.choose(np.array(rows), frames, mn, fb).tolist(), rows
    assert got[0] == [1, 0, 2] and got[1] == [2, 0] and got[2] == [2, 2, 2] and got[3] == [1, 1, 1] and got[4] == [0, 0] and got[5] == [1]


def test_the_header_declares_the_entry_points_and_the_binding_lists_them():
    from speechrecognition_amd import capi
    hdr = open(os.path.join(ROOT, "include", "srgpu.h")).read()
    for fn in ("sr_frontend_create_warped", "sr_frontend_warps", "sr_corpus_from_audio_warped", "sr_vtln_costs_corpus", "sr_vtln_chunks", "sr_vtln_choose"):
        assert re.search(r"SR_API int " + fn + r"\(", hdr) and fn in capi.SYMBOLS
    assert "NO JACOBIAN TERM" in hdr and "alpha == 1.0 is the identity by definition" in hdr
    assert all(hasattr(capi.FrontEnd, f) for f in ("from_audio_warped", "vtln_costs")) and hasattr(capi, "vtln_choose")
