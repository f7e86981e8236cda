"""The transcripts' chains of the MMI passes without a GPU or the library: speechrecognition_amd/csrc/chains.cpp, built alone with
tests/cpp/chains_driver.cpp under -fsanitize=address,undefined, against a restatement of the ChainArgs and BgChainArgs comments of
kernels.h that names the segments and says who enters whom; the recognition network's segment graph also against
tests/mmi_reference.py::chain_graph."""
import os
import struct
import subprocess

import numpy as np
import pytest

from tests import mmi_reference as MR
from tests import net_fb_reference as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NONE = 0xFFFF


@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    drv = str(tmp_path_factory.mktemp("chains") / "chains_driver")
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                           os.path.join(ROOT, "tests", "cpp", "chains_driver.cpp"),
                           os.path.join(ROOT, "speechrecognition_amd", "csrc", "chains.cpp"), "-o", drv])
    return drv


def run(driver, tmp_path, kind, W, sil, scale, off, info, lmT, transcripts):
    """a plain program, nothing preloaded: exit status 0, nothing on stderr -> the Chains as arrays"""
    trans_off = np.concatenate([[0], np.cumsum([len(t) for t in transcripts])]).astype(np.uint64)
    trans = np.asarray([w for t in transcripts for w in t], np.uint32)
    off, info = np.asarray(off, np.uint32), np.asarray(info, np.uint32)
    blob = struct.pack("<IIIdI", kind, W, sil, scale, len(off)) + off.tobytes() + struct.pack("<I", len(info)) + info.tobytes()
    if kind:
        blob += np.ascontiguousarray(lmT, np.float32).tobytes()
    blob += struct.pack("<I", len(transcripts)) + trans_off.tobytes() + trans.tobytes()
    case = tmp_path / "case.bin"
    case.write_bytes(blob)
    p = subprocess.run([driver, str(case)], text=True, stdout=subprocess.PIPE, stderr=subprocess.PIPE)
    assert p.returncode == 0 and not p.stderr, (p.stdout[-2000:], p.stderr[-2000:])
    out = {ln.split()[0]: ln.split()[1:] for ln in p.stdout.splitlines()}
    got = {k: np.array([int(v) for v in out[k]], np.uint64) for k in ("off", "info", "src", "dst")}
    got["lmc"] = np.array([int(v, 16) for v in out["lmc"]], np.uint64)
    got["sil_len"] = int(out["sil_len"][0])
    return got


def restate(segments, enters, slot_range, info, entry_cost=None):
    """One utterance's chain from its description.  segments: names in chain order, slot_range[name] = (first, last + 1) of the
    segment's slot in `info`.  enters[a] = (the two segments whose word end enters a, the two segments a's word end enters), each
    pair as (low half, high half) with None for none.  A segment's first two positions carry src = the LAST positions of the first
    pair, its last position dst = the FIRST positions of the second; every other link is 0xFFFFFFFF.  entry_cost[name] = the lmc of
    a segment's first two positions (0 where it names none)."""
    beg, end, inf = {}, {}, []
    for s in segments:
        a, b = slot_range[s]
        beg[s] = len(inf)
        inf += list(info[a:b])
        end[s] = len(inf) - 1
    src, dst = [0xFFFFFFFF] * len(inf), [0xFFFFFFFF] * len(inf)
    lmc = [0.0] * len(inf)
    pack = lambda pair, where: (where[pair[0]] if pair[0] is not None else NONE) | (where[pair[1]] if pair[1] is not None else NONE) << 16
    for s in segments:
        into, leaves = enters[s]
        for k in range(beg[s], min(beg[s] + 2, end[s] + 1)):
            src[k] = pack(into, end)
            if entry_cost is not None:
                lmc[k] = entry_cost.get(s, 0.0)
        dst[end[s]] = pack(leaves, beg)
    return inf, src, dst, lmc


def zerogram_links(n):
    """ChainArgs: sil_0 w_1 sil_1 .. w_n sil_n.  A word is entered by the silence before it and the word before that, and its end
    enters the silence after it and the next word; a silence is entered by the word before it and by itself, and enters the next
    word and itself.  The nearer segment takes the low half."""
    sil, w = (lambda i: ("sil", i)), (lambda i: ("w", i))
    segments, enters = [sil(0)], {}
    for i in range(1, n + 1):
        segments += [w(i), sil(i)]
    for i in range(0, n + 1):
        enters[sil(i)] = ((w(i) if i else None, sil(i)), (w(i + 1) if i < n else None, sil(i)))
    for i in range(1, n + 1):
        enters[w(i)] = ((sil(i - 1), w(i - 1) if i > 1 else None), (sil(i), w(i + 1) if i < n else None))
    return segments, enters


def bigram_links(n):
    """BgChainArgs: S w_1 c_1 .. w_n c_n.  S is entered by the start -- counted as its own word end, the low half -- and by
    itself, and enters itself and w_1.  w_i is entered by w_{i-1} and the copy c_{i-1} (w_1: by the start, that is S' word end,
    alone), and enters c_i and w_{i+1}.  c_i is entered by w_i alone and enters w_{i+1}."""
    S, w, c = "S", (lambda i: ("w", i)), (lambda i: ("c", i))
    segments, enters = [S], {S: ((S, None), (S, w(1) if n else None))}
    for i in range(1, n + 1):
        segments += [w(i), c(i)]
        enters[w(i)] = ((w(i - 1) if i > 1 else S, c(i - 1) if i > 1 else None), (c(i), w(i + 1) if i < n else None))
        enters[c(i)] = ((w(i), None), (w(i + 1) if i < n else None, None))
    return segments, enters


def bits(x):
    return np.asarray(x, np.float64).view(np.uint64)


def check(got, want_utts):
    off = np.concatenate([[0], np.cumsum([len(u[0]) for u in want_utts])])
    assert got["off"].tolist() == off.tolist()
    for k, name in enumerate(("info", "src", "dst")):
        assert got[name].tolist() == [v for u in want_utts for v in u[k]], name


# (word lengths; the silence word has 1 and 2 positions; words of 1, 2 and 3 positions)
LEXICA = [[1, 2, 3, 1], [2, 1, 3, 2]]
# empty, one word, the same word twice, three words: three utterances in a call, so the per-utterance bases count
CALLS = [([], [2], [1, 1]), ([1, 2, 3], [], [3]), ([3, 3], [2, 1, 2], [])]


@pytest.mark.parametrize("lens", LEXICA)
@pytest.mark.parametrize("transcripts", CALLS)
def test_recognition_network_chains(driver, tmp_path, lens, transcripts):
    word_off = np.concatenate([[0], np.cumsum(lens)])
    slot_info = 0x10000 * np.arange(1, word_off[-1] + 1) + 7 * np.arange(word_off[-1])   # every slot its own word
    got = run(driver, tmp_path, 0, len(lens), 0, 1.0, word_off, slot_info, None, transcripts)
    assert got["sil_len"] == lens[0] and len(got["lmc"]) == 0
    want = []
    for t in transcripts:
        segments, enters = zerogram_links(len(t))
        word_of = {s: (0 if s[0] == "sil" else t[s[1] - 1]) for s in segments}
        want.append(restate(segments, enters, {s: (word_off[w], word_off[w + 1]) for s, w in word_of.items()}, slot_info))
    check(got, want)
    # the segment graph of the reference: who enters a segment (its first position's link), whom its word end enters
    net = R.Net(word_off, np.arange(word_off[-1]), 0, 0)
    for u, t in enumerate(transcripts):
        gr = MR.chain_graph(net, t)
        base = int(got["off"][u])
        assert int(got["off"][u + 1]) - base == gr.P
        halves = lambda v: {h for h in (int(v) & 0xFFFF, int(v) >> 16) if h != NONE}
        for g in range(len(gr.src)):
            assert halves(got["src"][base + gr.beg[g]]) == set(gr.src[g]), (u, g)
            assert halves(got["dst"][base + gr.last[g]]) == {gr.beg[d] for d in gr.dst[g]}, (u, g)
            if gr.last[g] > gr.beg[g]:
                assert got["src"][base + gr.beg[g] + 1] == got["src"][base + gr.beg[g]]
        linked = {base + gr.beg[g] + k for g in range(len(gr.src)) for k in range(min(2, gr.last[g] - gr.beg[g] + 1))}
        ends = {base + e for e in gr.last}
        for p in range(base, base + gr.P):
            assert (got["src"][p] == 0xFFFFFFFF) == (p not in linked) and (got["dst"][p] == 0xFFFFFFFF) == (p not in ends)


@pytest.mark.parametrize("lens,sil", [(LEXICA[0], 0), (LEXICA[1], 0), ([1, 3, 2, 2], 2)])
@pytest.mark.parametrize("transcripts", CALLS)
def test_bigram_network_chains(driver, tmp_path, lens, sil, transcripts):
    """slot x < W is word x, slot W + x the silence copy after word x (none after the silence word)"""
    W, scale = len(lens), 2.5
    if sil:   # the transcripts name words other than the silence word
        transcripts = tuple([{sil: 0}.get(w, w) for w in t] for t in transcripts)
    slot_len = list(lens) + [0 if x == sil else lens[sil] for x in range(W)]
    slot_off = np.concatenate([[0], np.cumsum(slot_len)])
    pos_info = 0x10000 * np.arange(1, slot_off[-1] + 1) + 3 * np.arange(slot_off[-1])
    rng = np.random.default_rng(5)
    lmT = rng.uniform(-0.5, 3.0, size=(W, W)).astype(np.float32)   # [history][word]
    lmT[sil, next(t[0] for t in transcripts if t)] = np.inf                           # a first word the silence history forbids
    lmT[next((h, w) for t in transcripts for h, w in zip(t, t[1:]))] = np.nan         # a pair that is not a number: forbidden too
    got = run(driver, tmp_path, 1, W, sil, scale, slot_off, pos_info, lmT, transcripts)
    assert got["sil_len"] == lens[sil]
    want = []
    for t in transcripts:
        segments, enters = bigram_links(len(t))
        slot_of = {s: (sil if s == "S" else t[s[1] - 1] + (W if s[0] == "c" else 0)) for s in segments}
        cost = {}
        for i, w in enumerate(t, 1):
            x = lmT[t[i - 2] if i > 1 else sil, w]
            cost[("w", i)] = np.float64(scale) * np.float64(x) if x < np.inf else np.inf
        want.append(restate(segments, enters, {s: (slot_off[x], slot_off[x + 1]) for s, x in slot_of.items()}, pos_info, cost))
    check(got, want)
    want_lmc = bits([v for u in want for v in u[3]])
    assert np.array_equal(got["lmc"], want_lmc)
    inf_bits = int(bits([np.inf])[0])
    forbidden = sum(1 for t in transcripts for h, w in zip([sil] + list(t), t) if not lmT[h, w] < np.inf)
    assert forbidden >= 2 and (got["lmc"] == inf_bits).sum() >= forbidden and not np.isnan(got["lmc"].view(np.float64)).any()
