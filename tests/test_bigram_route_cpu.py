"""The choice of the bigram search kernel without a GPU: speechrecognition_amd/csrc/bigram_route.h -- the one function the launchers
switch on, compiled with the host compiler alone under AddressSanitizer and UBSan into tests/cpp/bigram_route_driver -- swept over every
lexicon size and held against the rules restated in tests/bigram_cases.py: the set of routes it can return is exactly the set of
instantiations the launcher has a case for, the sizes at which the routes change are where the LDS formulas put them, and the dense
layout's <4, 4> and <8, .> instantiations are out of reach (so they are not compiled any more)."""
import os
import re
import subprocess

import numpy as np
import pytest

from tests import bigram_cases as bc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "speechrecognition_amd", "csrc")


@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("bgroute") / "bigram_route_driver")
    subprocess.check_call(["g++", "-O1", "-std=c++17", "-Wall", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           "-I" + CSRC, os.path.join(ROOT, "tests", "cpp", "bigram_route_driver.cpp"), "-o", exe])
    return exe


@pytest.fixture(scope="module")
def sweep(driver):
    """route text -> (calls, W min, W max, P2 min, P2 max, smem max)"""
    out = {}
    for ln in subprocess.check_output([driver, "sweep"], text=True).splitlines():
        text, nums = ln.split(" | ")
        out[text] = tuple(int(x) for x in nums.split())
    return out


def launcher_cases():
    """the instantiations launch_bigram / dispatch_gs have a case for, as route texts"""
    src = open(os.path.join(CSRC, "viterbi_bigram.hip")).read()
    body = src[src.index("BigramRoute bigram_route_of"):]
    regs = [(int(a), int(b)) for a, b in re.findall(r"SR_BG_REGS\((\d+), (\d+)\);", body)]
    lds = [(int(a), int(b)) for a, b in re.findall(r"SR_BG_LDS\((\d+), (\d+)\);", body)]
    gs = [(int(a), int(b)) for a, b in re.findall(r"SR_BG_GS\((\d+), (\d+)\);", body)]
    assert len(set(regs)) == len(regs) and len(set(lds)) == len(lds) and len(set(gs)) == len(gs)
    return ([f"registers {kw} rows4 {bin(m)}" for kw, m in regs] + [f"lds {kw} x {kp}" for kw, kp in lds]
            + [f"global {kw} entries {'global' if g == 2 else 'lds'}" for kw, g in gs])


def test_reachable_routes_are_the_launchers_cases(sweep):
    reachable = set(sweep) - {"none"}
    print("\n".join(f"{t:28s} W {v[1]:4d} .. {v[2]:4d}  P2 {v[3]:5d} .. {v[4]:5d}  LDS <= {v[5]}" for t, v in sorted(sweep.items())))
    cases = launcher_cases()
    assert len(cases) == 14 + 8 + 5
    assert reachable == set(cases)             # no launcher case out of reach, no reachable route without a case
    assert reachable == set(bc.ROUTES)
    assert "none" in sweep                     # dense_states with an image that does not fit
    # the removed instantiations
    assert not any(t.startswith("lds 8 x") for t in sweep) and "lds 4 x 4" not in sweep
    src = open(os.path.join(CSRC, "viterbi_bigram.hip")).read()
    assert not re.search(r"bigram_kernel<\s*8\s*,", src) and not re.search(r"bigram_kernel<\s*4\s*,\s*4\s*,\s*0", src)
    assert all(v[5] <= bc.LDS_BYTES for v in sweep.values())


def test_routes_change_where_the_formulas_say(sweep):
    W = np.arange(1, 8193)
    last_dense = int(W[[bc.lds_dense(int(w), 2 * int(w)) <= bc.LDS_BYTES for w in W]].max())       # 42 W + 3268 <= 163 840
    last_kp20 = int(W[[bc.lds_dense(int(w), 12289) <= bc.LDS_BYTES for w in W]].max())
    first_eng = int(W[[bc.gs_lds(int(w), False) > bc.LDS_BYTES for w in W]].min())
    assert (last_dense, last_kp20, first_eng) == (3823, 2394, 4723)
    rng = {t: v[1:3] for t, v in sweep.items()}
    for rows, (a, b) in {1: (1, 1024), 2: (1025, 2048), 3: (2049, 3072)}.items():
        for m in range(1 << rows):
            assert rng[f"registers {rows} rows4 {bin(m)}"] == (a, b)
    for kp in (4, 12, 20):
        assert rng[f"lds 1 x {kp}"] == (1, 1024) and rng[f"lds 2 x {kp}"] == (1025, 2048)
    assert rng["lds 4 x 12"] == (2049, last_dense) and rng["lds 4 x 20"] == (2049, last_kp20)
    assert rng["global 1 entries lds"] == (1, 1024) and rng["global 2 entries lds"] == (1025, 2048) and rng["global 4 entries lds"] == (2049, 4096)
    assert rng["global 8 entries lds"] == (4097, first_eng - 1) and rng["global 8 entries global"] == (first_eng, 8192)
    # positions: KP 4 up to 4 096, KP 12 up to 12 288, KP 20 up to what fits at the row's first size
    assert sweep["lds 1 x 4"][4] == 4096 and sweep["lds 1 x 12"][3:5] == (4097, 12288) and sweep["lds 1 x 20"][3:5] == (12289, bc.dense_fit(1))
    assert sweep["lds 2 x 4"][4] == 4096 and sweep["lds 2 x 12"][3:5] == (4097, 12288) and sweep["lds 2 x 20"][3:5] == (12289, bc.dense_fit(1025))
    assert sweep["lds 4 x 12"][3:5] == (4098, 12288) and sweep["lds 4 x 20"][3:5] == (12289, bc.dense_fit(2049))


def smem(W, P2, ld, text):
    if text.startswith("registers"):
        return bc.lds_regs(W, ld)
    if text.startswith("lds"):
        return (bc.lds_dense(W, P2) + 15) // 16 * 16
    if text.startswith("global"):
        return bc.gs_lds(W, text.endswith("global"))
    return 0


def test_function_equals_the_restated_rules(driver, tmp_path):
    rng = np.random.default_rng(7)
    cases = []
    edge_w = [1, 2, 256, 768, 769, 1023, 1024, 1025, 2047, 2048, 2049, 2394, 2395, 3071, 3072, 3073, 3823, 3824, 4095, 4096, 4097, 4722, 4723, 8191, 8192]
    for W in edge_w + [int(w) for w in rng.integers(1, 8193, size=150)]:
        fit = bc.dense_fit(W)
        for P2 in {2 * W, 2 * W + 1, 3 * W, 4096, 4097, 12288, 12289, fit, fit + 1, 5 * W + 7}:
            if P2 < 2 * W:
                continue
            for ld in {8, 16, 256, 304, 2312, bc.ld_fit(W), bc.ld_fit(W) + 8} - {0}:
                for mss, sil in ((1, 1), (3, 1), (4, 1), (5, 1), (3, 2), (4, 3)):
                    for mask in range(8) if mss == 4 and sil == 1 else (0, 6):
                        for dense, glob in ((0, 0), (1, 0), (0, 1)):
                            cases.append((W, P2, ld, mss, sil, mask, dense, glob))
    cases += [(0, 0, 8, 1, 1, 0, 0, 0), (8193, 20000, 8, 1, 1, 0, 0, 0), (100, 199, 8, 1, 1, 0, 0, 0), (100, 300, 8, 3, 1, 0, 1, 1)]  # what cannot be
    path = tmp_path / "cases.txt"
    path.write_text("\n".join(" ".join(str(x) for x in c) for c in cases) + "\n")
    lines = subprocess.check_output([driver, str(path)], text=True).splitlines()
    assert len(lines) == len(cases) > 50000
    seen = set()
    for c, ln in zip(cases, lines):
        text, size = ln.split(" | ")
        want = bc.route(*c[:6], dense=bool(c[6]), glob=bool(c[7]))
        assert text == want, (c, text, want)
        assert int(size) == smem(c[0], c[1], c[2], text), (c, ln)
        seen.add(text)
    assert seen == set(bc.ROUTES) | {"none"}


def test_header_has_no_device_include():
    src = open(os.path.join(CSRC, "bigram_route.h")).read()
    assert "#include <hip" not in src and "kernels.h" not in src and "handles.h" not in src and "__device__" not in src
