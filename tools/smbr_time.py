"""Wall time and HIP-event kernel time of the sMBR accuracy pass (sr_net_accuracies_corpus, one item per frame) beside the free
occupancy pass (sr_net_occupancies_corpus) and one MMI E-step (sr_mmi_statistics_corpus) in the same run, on tools/mmi_time.py's two
shapes: BASELINE configs[2]'s 4000 positions and the 211-position sietill lexicon, 1000 utterances of 200..400 frames, features
resident, SR_GMM_PREFILTER, word penalty 10, kappa 0.1, posterior floor 1e-4.  The references are random mixtures of the lexicon.
Kernel time = the profile's scoring + search event time (sr_profile_read) per call.  Writes profiles/smbr.txt (or --out).

  python tools/smbr_time.py [--out PATH] [--reps N] [--shapes configs2,sietill]"""
import argparse
import os
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from mmi_time import FLOOR, TDP, make_case  # noqa: E402


def timed(m, f, reps):
    """-> (result, wall seconds per call, (scoring ms, search ms) of the device events per call): one warm-up call, then reps"""
    f()
    m.profile(True)
    t0 = time.perf_counter()
    for _ in range(reps):
        r = f()
    wall = (time.perf_counter() - t0) / reps
    p = m.profile_read()
    m.profile(False)
    return r, wall, (p["gmm_ms"] / reps, p["search_ms"] / reps)


def measure(shape, reps):
    from speechrecognition_amd import capi, synth
    lex, spec, mix, dim, feats, off, trans = make_case(shape)
    mp = os.path.join(tempfile.mkdtemp(), "m.mix")
    synth.write_mixset(mp, spec)
    word_off, automaton, sil_state = lex.flatten()
    ref = np.random.default_rng(31).choice(np.unique(automaton), size=len(feats)).astype(np.uint16)
    rows = []
    with capi.Model.from_mixset(mp, dim) as m:
        L = capi.Lexicon(m, word_off, automaton, lex.silence_idx, TDP, sil_state)
        c = m.upload(feats, off)
        for name, f in (("sr_net_occupancies_corpus (free, 1 item / frame)", lambda: c.net_occupancies(L, 10.0, 0.1, None, capi.GMM_PREFILTER, FLOOR, 1)),
                        ("sr_net_accuracies_corpus (1 item / frame)", lambda: c.net_accuracies(L, 10.0, ref, 0.1, capi.GMM_PREFILTER, FLOOR, 1)),
                        ("sr_mmi_statistics_corpus", lambda: c.mmi_statistics(L, 10.0, trans, 0.1, capi.GMM_PREFILTER, FLOOR, True))):
            r, wall, (gmm, search) = timed(m, f, reps)
            rows.append((name, wall * 1e3, gmm, search, r))
        c.close()
        L.close()
    acc = rows[1][4][1]
    out = [f"{shape}: {len(automaton)} positions, {lex.n_words} words, {lex.n_states} states x {mix} densities, 1000 utterances, "
           f"{int(off[-1])} frames; mean of {reps} calls after one warm-up",
           f"  {'':52s} {'wall ms':>10s} {'scoring ms':>11s} {'search ms':>10s}"]
    out += [f"  {n:52s} {w:10.2f} {g:11.2f} {s:10.2f}" for n, w, g, s, _ in rows]
    out.append(f"  accuracy pass / occupancy pass: wall {rows[1][1] / rows[0][1]:.2f}, search events {rows[1][3] / rows[0][3]:.2f}; "
               f"sum Abar = {acc.sum():.1f} of {int(off[-1])} frames")
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "smbr.txt"))
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--shapes", default="configs2,sietill")
    ap.add_argument("--no-write", action="store_true")
    a = ap.parse_args()
    lines = []
    for s in a.shapes.split(","):
        part = measure(s, a.reps)
        lines += part
        print("\n".join(part), flush=True)
    if not a.no_write:
        with open(a.out, "w") as f:
            f.write("The sMBR accuracy pass against the free occupancy pass and one MMI E-step (tools/smbr_time.py)\n" + "\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
