"""sr_stream_trim without a GPU: tests/stream_trim_reference.py's trim, held against the untrimmed search of
tests/stream_commit_reference.py on random non-negative score tables -- the final words, the partial result after every push, both
parities of the frames dropped, the ending without a surviving word end -- and the call's presence in the library, the header and
the binding, its kernel in the gfx950 build, and the mirror's member."""
import ctypes
import math
import os
import re
import subprocess
import sys
import tempfile

import numpy as np
import pytest

from tests import stream_commit_reference as scr
from tests import stream_trim_reference as ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import isa_info  # noqa: E402

T = 120


def _table(name, seed):
    """random costs in [0, 40): the best path changes words often, so the commit point moves"""
    lex = ref.LEXICA[name]
    return np.random.default_rng(seed).uniform(0.0, 40.0, size=(T, lex.n_states))


@pytest.mark.parametrize("beam", [60.0, math.inf])
@pytest.mark.parametrize("name", sorted(ref.LEXICA))
def test_trimmed_search_reports_what_the_untrimmed_one_does(name, beam):
    net = ref.make_net(ref.LEXICA[name])
    scores = _table(name, 7301)
    parities, dropped_any = set(), 0
    for piece in (1, 3, 7):
        per, tr, un = ref.run(net, beam, ref.WP, scores, piece)
        assert tr.frames() == un.t == T
        want_final = scr.walk(un.tb_word, un.tb_bkp, T, net.silence_word)
        assert math.isfinite(un.tb_score[T])  # (the ending without a word end has its own test)
        assert np.array_equal(tr.partial(), want_final), (name, beam, piece)
        assert len(want_final) >= 3
        for r in per:
            assert np.array_equal(r["partial"], r["want_partial"]), (name, beam, piece, r["frames"])
            assert np.array_equal(r["stable"], r["want_stable"]) and r["commit"] == r["want_commit"], (name, beam, piece, r["frames"])
            if r["dropped"]:
                parities.add(r["dropped"] & 1)
                dropped_any += 1
        # the window stays far below the utterance: max_frames bounds the uncommitted frames only
        assert ref.window_needed(per) < T // 2, (name, beam, piece, ref.window_needed(per))
        assert tr.base > T // 2 and len(tr.archive) >= 2
        # the search itself went on bit for bit: scores are absolute, back pointers differ by the base where a hypothesis is alive
        assert np.array_equal(np.array(tr.sc).view(np.uint64), np.array(un.sc).view(np.uint64))
        assert all(tr.bk[p] + tr.base == un.bk[p] for p in range(net.P) if math.isfinite(tr.sc[p]))
    assert parities == {0, 1} and dropped_any >= 10


@pytest.mark.parametrize("name", sorted(ref.LEXICA))
def test_a_trim_every_few_pushes_and_a_trim_of_nothing(name):
    net = ref.make_net(ref.LEXICA[name])
    scores = _table(name, 7302)
    per, tr, un = ref.run(net, 60.0, ref.WP, scores, 3, trim_every=4)
    for r in per:
        assert np.array_equal(r["partial"], r["want_partial"]) and np.array_equal(r["stable"], r["want_stable"])
    before = (list(tr.tb_bkp), list(tr.bk), tr.base, list(tr.archive))
    d = tr.trim()
    if d:  # right after a trim the commit point is the window's frame 0
        before = (list(tr.tb_bkp), list(tr.bk), tr.base, list(tr.archive))
        d = tr.trim()
    assert d == 0 and before == (tr.tb_bkp, tr.bk, tr.base, tr.archive)
    fresh = ref.TrimSearch(net, 60.0, ref.WP)
    assert fresh.trim() == 0 and fresh.base == 0 and len(fresh.partial()) == 0  # before any push


@pytest.mark.parametrize("how", ["inf_row", "tight_beam"])
def test_an_ending_without_a_surviving_word_end_reports_no_words(how):
    """The reference's walk starts at traceback[T]; where no word end survived frame T that entry is (inf, word 0, bkp 0) and the
    result is empty, whatever was recognised before.  The archive must not be prepended to it."""
    name = "w5x9"
    net = ref.make_net(ref.LEXICA[name])
    scores = _table(name, 7303)
    beam = 60.0
    if how == "inf_row":
        scores[-1, :] = math.inf  # nothing survives the last frame
    else:
        # the last rows put every word's last state beyond the beam: the word ends are pruned, in-word hypotheses live on
        ends = sorted({net.state[p] for p in range(net.P) if net.end[p]})
        scores[-3:, ends] += 4.0 * beam
    per, tr, un = ref.run(net, beam, ref.WP, scores, 3)
    assert not math.isfinite(un.tb_score[T]) and not math.isfinite(tr.tb_score[tr.t])  # the fixture hits the case
    assert tr.base > 0 and len(tr.archive) >= 1
    assert len(scr.walk(un.tb_word, un.tb_bkp, T, net.silence_word)) == 0
    assert len(tr.partial()) == 0
    for r in per:
        assert np.array_equal(r["partial"], r["want_partial"]), r["frames"]
    if how == "tight_beam":
        assert any(math.isfinite(v) for v in tr.sc)  # the search is alive: only the word ends are gone


# ---- the call in the library, the header, the binding and the mirror -------------------------------------------------------------
def test_library_header_and_binding_carry_the_trim_entry_point():
    from speechrecognition_amd import build, capi

    build.build()
    lib = ctypes.CDLL(build.LIB)
    with open(os.path.join(ROOT, "include", "srgpu.h")) as f:
        hdr = f.read()
    assert hasattr(lib, "sr_stream_trim")
    assert re.search(r"SR_API int sr_stream_trim\(", hdr)
    assert "sr_stream_trim" in capi.SYMBOLS
    assert re.search(r"#define\s+SR_ABI_VERSION\s+4\b", hdr) and lib.sr_abi_version() == 4  # a function only, no struct changed
    assert callable(capi.Stream.trim)
    ids = np.zeros(1, np.uint32)
    dropped = np.full(1, 77, np.uint32)
    assert capi.lib().sr_stream_trim(None, 1, ids.ctypes.data, dropped.ctypes.data) == -1  # before any device is touched
    assert dropped[0] == 77


@pytest.mark.skipif(not os.path.exists(os.path.join(isa_info.LLVM, "llvm-objdump")), reason="no ROCm LLVM tools")
def test_trim_kernel_is_built_without_scratch():
    from speechrecognition_amd import build

    build.build()
    with tempfile.TemporaryDirectory() as tmp:
        md = isa_info.kernel_metadata(isa_info.code_object("viterbi_decode", tmp))
    for kernel in ("stream_trim_kernel<256>", "stream_commit_kernel<256>"):
        assert kernel in md, (kernel, sorted(md))
        k = md[kernel]
        assert k["private_segment_fixed_size"] == 0 and k.get("vgpr_spill_count", 0) == 0 and k.get("sgpr_spill_count", 0) == 0, (kernel, k)


def test_trim_member_of_the_mirror_compiles():
    """include/sr_sietill.hpp's StreamingRecognizer::trim against srgpu.h (syntax and types)."""
    src = os.path.join(ROOT, "tests", "cpp", "stream_trim_driver.cpp")
    r = subprocess.run(["g++", "-std=c++17", "-Wall", "-fsyntax-only", "-I" + os.path.join(ROOT, "include"), src],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
