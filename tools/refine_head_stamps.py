"""Diagnostic: what the waves of a SIMD do at the heads of gmm_refine_kernel's main-pass iterations (profiles/refine_iteration_head.txt).

Needs a library built from profiles/refine_iteration_head_probe.patch with -DSR_R_PROBE=3 (tools/build_variant.py; the patch's
-DSR_R_PROBE_FIXED / _MASKS_LATE / _STAGGER rebuild the kernel before the hand-out), selected with SRGPU_LIB: every wave of eight
workgroups of a launch leaves s_memtime stamps per iteration in a buffer of their own --
  T0 iteration head, T1 features and masks requested, T2 all of it back, T3 the second mask quad wanted, T4 and there,
  T5 main pass done, T6 iteration end (after the lists' batches)
-- and sr_probe_read copies them out.  A wave is "in a wait" between T1 and T2 and between T3 and T4.
usage: SRGPU_LIB=... python tools/refine_head_stamps.py [--mix 32] [--words 1333] [--utts 1000]
Recognises the headline corpus (bench.py's model and batch) twice and reads the stamps of the second launch."""
import argparse, os, sys, tempfile
import ctypes as C
import numpy as np
sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
from speechrecognition_amd import capi, synth

ap = argparse.ArgumentParser()
ap.add_argument("--mix", type=int, default=32)
ap.add_argument("--words", type=int, default=1333)
ap.add_argument("--utts", type=int, default=1000)
ap.add_argument("--dim", type=int, default=39)
args = ap.parse_args()
WGS, WAVES, ITS, ST = 8, 12, 320, 8

lex = synth.make_lexicon(args.words, 3, 1)
spec = synth.make_mixset(lex.n_states, args.mix, args.dim, seed=23)
mp = os.path.join(tempfile.mkdtemp(), "m.mix")
synth.write_mixset(mp, spec)
feats, off = synth.make_batch(args.utts, 200, 400, args.dim, seed=7)
m = capi.Model.from_mixset(mp, args.dim)
c = m.upload(feats, off)
print(f"{lex.n_states} states x {args.mix}, {c.n_frames} frames; geometry (threads, pseudo-states, frames per workgroup, chunks) {m.refine_geometry(c.n_frames)}"
      f"; library {os.path.basename(capi.LIB_PATH)}")
word_off, automaton, sil = lex.flatten()
lexh = m.lexicon(word_off, automaton, lex.silence_idx, (3.0, 0.0, 30.0), sil)
for _ in range(2):  # (a recognition step: the table stays on the device)
    c.recognize(lexh, 200.0, 10.0)
probe = C.CDLL(capi.LIB_PATH)
stamps = np.zeros((WGS, WAVES, ITS, ST), np.uint32)
hdr = np.zeros((WGS, WAVES, 8), np.uint64)
rc = probe.sr_probe_read(C.c_void_p(stamps.ctypes.data), C.c_void_p(hdr.ctypes.data))
assert rc == 0, rc


def union_len(iv):
    """total length of the union of intervals [(a, b)]"""
    tot, end = 0, None
    for a, b in sorted(iv):
        if end is None or a > end:
            tot += b - a; end = b
        elif b > end:
            tot += b - end; end = b
    return tot


def all_in(ivs):
    """length of the time in which every one of the interval lists has an interval open (sweep)"""
    ev = []
    for k, iv in enumerate(ivs):
        for a, b in iv:
            ev.append((a, 1, k)); ev.append((b, -1, k))
    ev.sort()
    open_, tot, prev = [0] * len(ivs), 0, None
    for t, d, k in ev:
        if prev is not None and all(o > 0 for o in open_):
            tot += t - prev
        open_[k] += d; prev = t
    return tot


tot = {"span": 0, "all": 0, "two": 0, "wave_wait": 0, "act": np.zeros(4)}
for g in range(WGS):
    nw = int(np.count_nonzero(hdr[g, :, 7]))
    if nw == 0:
        continue
    n_w = np.minimum(hdr[g, :nw, 7].astype(np.int64), ITS)  # iterations per wave (blocks handed out: they differ)
    n = int(n_w.min())
    hw = hdr[g, :nw, 0].astype(np.int64)
    simd, cu = (hw >> 4) & 3, (hw >> 8) & 15
    clk = (hdr[g, 0, 5] - hdr[g, 0, 3]) / max(1, int(hdr[g, 0, 6] - hdr[g, 0, 4])) * 100.0  # MHz: s_memrealtime ticks at 100 MHz
    t_start = int(hdr[g, :nw, 3].min())
    T = stamps[g, :nw, :, :7].astype(np.int64) + (t_start & ~0xFFFFFFFF)
    T[T < t_start] += 1 << 32  # (the low word wrapped after the kernel's start)
    it_len = np.median(np.concatenate([np.diff(T[w, :n_w[w], 0]) for w in range(nw)]))
    print(f"\nworkgroup ({int(hdr[g, 0, 1])}, {int(hdr[g, 0, 2])}): CU {sorted(set(cu.tolist()))} SE {int(hw[0] >> 13) & 7}, iterations per wave {n_w.tolist()}, "
          f"clock {clk:.0f} MHz, median iteration {it_len:.0f} cycles; SIMD of waves 0..{nw - 1}: {simd.tolist()}")
    seg = np.median(np.concatenate([np.diff(T[w, :n_w[w], :], axis=1) for w in range(nw)]), axis=0)
    print("  median cycles per wave: request %d | wait (features + masks) %d | convert + states 0-3 %d | second-quad wait %d | states 4-7 + stores %d | lists %d"
          % tuple(int(v) for v in seg))
    for s in range(4):
        ws = [w for w in range(nw) if simd[w] == s]
        if not ws:
            continue
        first, final = [T[w, 0, 0] for w in ws], [T[w, n_w[w] - 1, 6] for w in ws]
        lo, hi = min(first), max(final)
        waits = [[(T[w, i, 1], T[w, i, 2]) for i in range(n_w[w])] + [(T[w, i, 3], T[w, i, 4]) for i in range(n_w[w])] for w in ws]
        a_all = all_in(waits)
        two = sum(all_in([waits[i], waits[j]]) for i in range(len(ws)) for j in range(i + 1, len(ws))) - (len(ws) - 1) * a_all if len(ws) > 2 else a_all
        one = sum(union_len(w) for w in waits)
        heads = np.stack([T[w, :n, 0] for w in ws])
        spread = heads.max(0) - heads.min(0)
        q = [0, n // 4, n // 2, 3 * n // 4, n - 1]
        fin = sorted(final)
        act = [fin[0] - lo] + [fin[i] - fin[i - 1] for i in range(1, len(fin))]  # time with all, all but one, ... of the waves still at work
        print(f"  SIMD {s} waves {ws}: all in a wait {100.0 * a_all / (hi - lo):5.2f} % of {hi - lo} cycles, at least two {100.0 * two / (hi - lo):5.2f} %, "
              f"a wave's own waits {100.0 * one / len(ws) / (hi - lo):5.2f} %; heads of iteration {q} apart by {[int(spread[i]) for i in q]} cycles "
              f"(median {np.median(spread) / it_len:.2f} iterations); waves at work: " + ", ".join(f"{len(ws) - i} for {100.0 * a / (hi - lo):.1f} %" for i, a in enumerate(act)))
        tot["span"] += hi - lo; tot["all"] += a_all; tot["two"] += two; tot["wave_wait"] += one / len(ws)
        tot["act"][:len(act)] += act
if tot["span"]:
    print(f"\nall probed SIMDs: every wave in a wait {100.0 * tot['all'] / tot['span']:.2f} % of the time, at least two of them {100.0 * tot['two'] / tot['span']:.2f} %, "
          f"a wave's own waits {100.0 * tot['wave_wait'] / tot['span']:.2f} %; all waves at work {100.0 * tot['act'][0] / tot['span']:.1f} %, one gone "
          f"{100.0 * tot['act'][1] / tot['span']:.1f} %, two gone {100.0 * tot['act'][2] / tot['span']:.1f} %")
