#!/usr/bin/env python3
"""Latency of streaming recognition (sr_stream_*) on bench.py's headline workload (BASELINE configs[2]: 4000 states x 32
densities, 1333 three-state words, 39-dim frames, utterances U{200..400} from bench.py's seed, beam 200, word penalty 10).

N concurrent streams (default 64); every push hands each open stream its next `--piece` frames (default 10, i.e. 100 ms of
audio); a stream that has had all its frames is ended and the next utterance begun in its place.  Prints the median and p99
wall time per push (host clock around sr_stream_push, which returns after its search has finished), the device time of the
scoring and search launches from sr_profile, and the total time to finish the corpus against one sr_recognize_corpus over the
same utterances (features resident).  The streamed words are checked against the batch's.  Needs a GPU.

--decoder bigram: the bigram-LM stream (sr_bigram_stream_*) on BASELINE configs[4]'s shape instead -- 8000 states x 64 densities,
2666 words, bench.py's seeded bigram table and transition scores, acoustic beam 200, no LM beam -- against one
sr_recognize_bigram_corpus; the streamed items (words, score bits, times) are checked against the batch's.

--stable: after every push also asks for the stable prefix of the pushed streams (sr_stream_stable / sr_bigram_stream_stable, one
call for all of them) and prints the median and p99 wall time of that call beside the push's; every answer is checked to be a
prefix of its utterance's final result (where that is not empty).

--trim (zerogram): after every push (and after the stable call, with --stable) also trims the pushed streams at their commit points
(sr_stream_trim, one call for all of them) and prints the median, p99 and maximum wall time of that call, the frames dropped, and the
largest window any stream held at a push -- the max_frames the corpus needs with a trim every push -- with sr_stream_open's device
bytes per stream at that window and at 65535.  The words are still checked against the batch's.

--audio: the same stream set fed PCM samples (sr_stream_push_audio / sr_bigram_stream_push_audio) through a front end of the model's
shape -- window 400, shift 160, 512-point transform, 13 cepstra and their deltas and delta-deltas (39 dimensions), step 3, no energy
maximum -- on noise utterances of U{200..400} frames: every push hands each open stream its next --piece x 160 samples.  In the same
run the rows the batch front end gives for the same utterances are streamed as feature pushes of --piece rows, and the two pushes'
median and p99 wall times are printed side by side.  stream_frontend_kernel's device time is the difference of the two runs' search
windows (sr_profile's HIP events: the front end's launch is counted there).  The two runs' results are checked to be equal.

--pipeline: the stream set with a projection and a transform per stream (sr_stream_set_projection, sr_stream_set_transform): rows of
39 columns, context 4 (E = 351), into the 39-dimensional model, on noise utterances of U{200..400} rows (with --audio: the front end
above on a placeholder model, its rows the pipeline's input).  In the same run the plain push of the same number of rows -- the batch
route's rows as feature pushes, or the same audio through a front end of the model itself -- is timed, and the two pushes' median and
p99 wall times are printed side by side.  stream_pipeline_kernel's device time is the difference of the two runs' search windows.  The
pipeline run's results are checked against the batch route's (splice_transform, transform, one recognition call).

--audio --vtln: the front end of --audio with 13 warps (alpha 0.88 .. 1.12, break 0.875); beside the audio run with no warp set, the same
pushes with a warp on every id (sr_stream_set_warp / sr_bigram_stream_set_warp), dealt round-robin -- the utterance begun u-th takes warp
u mod 13, so the 64 ids of a push carry all 13 -- and the two audio pushes' median and p99 wall times and stream_frontend_kernel's device
time side by side.  The warped run's results are checked against one recognition call on sr_corpus_from_audio_warped's corpus."""
from __future__ import annotations

import argparse
import os
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--streams", type=int, default=64)
    ap.add_argument("--piece", type=int, default=10, help="frames per stream per push")
    ap.add_argument("--utts", type=int, default=1000, help="utterances of bench.py's corpus to stream")
    ap.add_argument("--kernel", choices=["default", "prefilter", "exact", "mfma"], default="default")
    ap.add_argument("--decoder", choices=["zerogram", "bigram"], default="zerogram")
    ap.add_argument("--stable", action="store_true", help="after every push, time the stable-prefix call on the pushed streams")
    ap.add_argument("--trim", action="store_true", help="after every push, trim the pushed streams at their commit points and time the call")
    ap.add_argument("--audio", action="store_true", help="time audio pushes beside feature pushes of the same rows")
    ap.add_argument("--vtln", action="store_true", help="with --audio: time audio pushes whose ids carry VTLN warps beside the same pushes without")
    ap.add_argument("--pipeline", action="store_true", help="time pushes through a projection and a transform per stream beside plain pushes")
    args = ap.parse_args()
    if args.vtln and (args.pipeline or not args.audio):
        ap.error("--vtln goes with --audio (and not with --pipeline)")
    if args.trim and (args.pipeline or args.audio or args.decoder == "bigram"):
        ap.error("--trim times the zerogram feature push (the bigram stream set does not trim)")
    if args.pipeline:
        return main_pipeline(args)
    if args.audio:
        return main_audio(args)
    if args.decoder == "bigram":
        return main_bigram(args)

    from speechrecognition_amd import capi, synth

    D = 39
    lex = synth.make_lexicon(1333, 3, 1)
    tdp, beam, wp = (3.0, 0.0, 30.0), 200.0, 10.0
    kernel = {"mfma": capi.GMM_MFMA, "exact": capi.GMM_EXACT, "prefilter": capi.GMM_PREFILTER, "default": capi.GMM_DEFAULT}[args.kernel]
    tmp = tempfile.mkdtemp(prefix="srstream_")
    mp = os.path.join(tmp, "model.mix")
    synth.write_mixset(mp, synth.make_mixset(lex.n_states, 32, D, seed=23))  # bench.py's model and corpus
    feats, off = synth.make_batch(1000, 200, 400, D, seed=7)
    n = min(args.utts, len(off) - 1)
    off = off[: n + 1]
    feats = feats[: int(off[-1])]
    utts = [feats[int(off[u]):int(off[u + 1])] for u in range(n)]
    word_off, automaton, sil = lex.flatten()

    with capi.Model.from_mixset(mp, D) as m:
        lexh = m.lexicon(word_off, automaton, lex.silence_idx, tdp, sil)
        corpus = m.upload(feats, off)
        corpus.recognize(lexh, beam, wp, kernel)  # warm: packing, workspaces
        t = time.perf_counter()
        words, woff = corpus.recognize(lexh, beam, wp, kernel)
        batch_s = time.perf_counter() - t
        corpus.close()

        with m.stream(lexh, beam, wp, kernel, max_streams=args.streams, max_frames=int(np.diff(off.astype(np.int64)).max())) as st:
            warm = [st.begin() for _ in range(args.streams)]  # warm: staging at the full push size, the kernels' code objects
            st.push({sid: utts[0][:args.piece] for sid in warm})
            for sid in warm:
                st.end(sid)
            m.profile(True)
            todo = list(range(n))
            open_ = {}  # id -> (utterance, frames pushed)
            got = {}
            push_ms, stable_ms, last_stable, stable_ok = [], [], {}, True
            trim_ms, base, dropped_total, window = [], {}, 0, 0
            t_all = time.perf_counter()
            while todo or open_:
                while todo and len(open_) < args.streams:
                    u = todo.pop(0)
                    sid = st.begin()
                    open_[sid] = (u, 0)
                    base[sid] = 0
                batch = {}
                for sid, (u, t0) in open_.items():
                    batch[sid] = utts[u][t0:t0 + args.piece]
                    window = max(window, t0 + len(batch[sid]) - base[sid])  # the frames the stream holds once this push is in
                t = time.perf_counter()
                st.push(batch)
                push_ms.append(1e3 * (time.perf_counter() - t))
                if args.stable:
                    t = time.perf_counter()
                    sw, _, _ = st.stable(list(batch))
                    stable_ms.append(1e3 * (time.perf_counter() - t))
                    last_stable.update(zip(batch, sw))
                if args.trim:
                    t = time.perf_counter()
                    dropped = st.trim(list(batch))
                    trim_ms.append(1e3 * (time.perf_counter() - t))
                    for sid, d in zip(batch, dropped):
                        base[sid] += int(d)
                        dropped_total += int(d)
                for sid in list(open_):
                    u, t0 = open_[sid]
                    t0 += len(batch[sid])
                    if t0 == len(utts[u]):
                        got[u] = st.end(sid)
                        if args.stable and len(got[u]):
                            stable_ok &= np.array_equal(last_stable[sid], got[u][: len(last_stable[sid])])
                        del open_[sid]
                    else:
                        open_[sid] = (u, t0)
            stream_s = time.perf_counter() - t_all
            prof = m.profile_read()
        lexh.close()

    same = all(np.array_equal(got[u], words[int(woff[u]):int(woff[u + 1])]) for u in range(n))
    pm = np.asarray(push_ms)
    pushes = len(pm)
    print(f"workload: configs[2] model (4000 states x 32, 1333 three-state words), {n} utterances, {int(off[-1])} frames, "
          f"{args.streams} concurrent streams, {args.piece} frames per stream per push, gmm_kernel {args.kernel}")
    print(f"pushes: {pushes}; wall per push: median {np.median(pm):.3f} ms, p99 {np.percentile(pm, 99):.3f} ms, "
          f"min {pm.min():.3f} ms, max {pm.max():.3f} ms")
    print(f"device per push (sr_profile): scoring {prof['gmm_ms'] / pushes:.3f} ms ({prof['gmm_launches']} launches), "
          f"search {prof['search_ms'] / pushes:.3f} ms ({prof['search_launches']} launches); frames {prof['frames']}")
    dev = prof["gmm_ms"] + prof["search_ms"]
    print(f"device share of push wall time: {dev / pm.sum():.1%} (the rest: copies, launches, synchronisation, host)")
    print(f"corpus: streamed in {stream_s:.3f} s (of which {pm.sum() / 1e3:.3f} s in sr_stream_push) vs one "
          f"sr_recognize_corpus {batch_s:.3f} s ({stream_s / batch_s:.1f}x)")
    print(f"streamed words equal the batch's: {'yes' if same else 'NO'}")
    if args.stable:
        sm = np.asarray(stable_ms)
        print(f"sr_stream_stable on the pushed streams, after every push: median {np.median(sm):.3f} ms, p99 {np.percentile(sm, 99):.3f} ms, "
              f"min {sm.min():.3f} ms, max {sm.max():.3f} ms ({np.median(sm) / np.median(pm):.1%} of a push at the median)")
        print(f"stable words were a prefix of the final words: {'yes' if stable_ok else 'NO'}")
        same = same and stable_ok
    if args.trim:
        tm = np.asarray(trim_ms)
        print(f"sr_stream_trim on the pushed streams, after every push: median {np.median(tm):.3f} ms, p99 {np.percentile(tm, 99):.3f} ms, "
              f"min {tm.min():.3f} ms, max {tm.max():.3f} ms ({np.median(tm) / np.median(pm):.1%} of a push at the median)")
        print(f"frames dropped: {dropped_total} of {int(off[-1])}; the largest window a stream held at a push: {window} frames "
              f"(the longest utterance: {int(np.diff(off.astype(np.int64)).max())})")
        P = int(word_off[-1])

        def slot_bytes(mf):  # sr_stream_open's formula, plus the first stable or trim call's 4 + 4 max_frames
            return ((20 * P + 255) // 256) * 256 + 12 * (mf + 1) + 4 * mf + 40 + 4 + 4 * mf

        print(f"device bytes per stream (P = {P} positions): {slot_bytes(65535)} at max_frames 65535, {slot_bytes(window)} at max_frames {window}")
    return 0 if same else 1


def main_bigram(args):
    from speechrecognition_amd import capi, synth

    D = 39
    lex = synth.make_lexicon(2666, 3, 1, extra_states_last=1)  # bench.py --config cfg5
    beam = 200.0
    kernel = {"mfma": capi.GMM_MFMA, "exact": capi.GMM_EXACT, "prefilter": capi.GMM_PREFILTER, "default": capi.GMM_DEFAULT}[args.kernel]
    tmp = tempfile.mkdtemp(prefix="srstream_")
    mp = os.path.join(tmp, "model.mix")
    synth.write_mixset(mp, synth.make_mixset(lex.n_states, 64, D, seed=23))
    feats, off = synth.make_batch(1000, 200, 400, D, seed=7)
    n = min(args.utts, len(off) - 1)
    off = off[: n + 1]
    feats = feats[: int(off[-1])]
    utts = [feats[int(off[u]):int(off[u + 1])] for u in range(n)]
    word_off, automaton, _ = lex.flatten()
    lm_rng = np.random.default_rng(99)  # bench.py's bigram table and transition scores
    nW = lex.n_words
    lm = np.empty((nW, nW), np.float32)
    for h0 in range(0, nW, 256):
        p = lm_rng.dirichlet(np.ones(nW), size=min(256, nW - h0))
        lm[:, h0:h0 + p.shape[0]] = (-np.log(np.maximum(p, 1e-30))).T
    bg_tdp = np.array([[3.0, 0.0, 3.0, 150.0], [0.0001, 3.0, np.inf, 15.0]], np.float32)

    with capi.Model.from_mixset(mp, D) as m:
        bg = m.bigram(word_off, automaton, lex.silence_idx, lm, bg_tdp)
        corpus = m.upload(feats, off)
        corpus.recognize_bigram(bg, beam, capi.FLT_MAX, kernel)  # warm: packing, workspaces
        t = time.perf_counter()
        bw, bs, bt, boff = corpus.recognize_bigram(bg, beam, capi.FLT_MAX, kernel)
        batch_s = time.perf_counter() - t
        corpus.close()

        with m.bigram_stream(bg, beam, capi.FLT_MAX, kernel, max_streams=args.streams, max_frames=int(np.diff(off.astype(np.int64)).max())) as st:
            warm = [st.begin() for _ in range(args.streams)]
            st.push({sid: utts[0][:args.piece] for sid in warm})
            for sid in warm:
                st.end(sid)
            m.profile(True)
            todo = list(range(n))
            open_ = {}
            got = {}
            push_ms, stable_ms, last_stable, stable_ok = [], [], {}, True
            t_all = time.perf_counter()
            while todo or open_:
                while todo and len(open_) < args.streams:
                    u = todo.pop(0)
                    open_[st.begin()] = (u, 0)
                batch = {sid: utts[u][t0:t0 + args.piece] for sid, (u, t0) in open_.items()}
                t = time.perf_counter()
                st.push(batch)
                push_ms.append(1e3 * (time.perf_counter() - t))
                if args.stable:
                    t = time.perf_counter()
                    si, _ = st.stable(list(batch))
                    stable_ms.append(1e3 * (time.perf_counter() - t))
                    last_stable.update(zip(batch, si))
                for sid in list(open_):
                    u, t0 = open_[sid]
                    t0 += len(batch[sid])
                    if t0 == len(utts[u]):
                        got[u] = st.end(sid)
                        if args.stable and len(got[u][0]):
                            k = len(last_stable[sid][0])
                            stable_ok &= all(np.array_equal(a.view(np.uint32), b[:k].view(np.uint32)) for a, b in zip(last_stable[sid], got[u]))
                        del open_[sid]
                    else:
                        open_[sid] = (u, t0)
            stream_s = time.perf_counter() - t_all
            prof = m.profile_read()
        bg.close()

    def same(u):
        a, b = int(boff[u]), int(boff[u + 1])
        w, s, tm = got[u]
        return np.array_equal(w, bw[a:b]) and np.array_equal(tm, bt[a:b]) and np.array_equal(s.view(np.uint32), bs[a:b].view(np.uint32))

    ok = all(same(u) for u in range(n))
    pm = np.asarray(push_ms)
    pushes = len(pm)
    print(f"workload: configs[4] shape (8000 states x 64, 2666 words, bench.py's bigram table), bigram stream (global-states layout), "
          f"{n} utterances, {int(off[-1])} frames, {args.streams} concurrent streams, {args.piece} frames per stream per push, "
          f"gmm_kernel {args.kernel}")
    print(f"pushes: {pushes}; wall per push: median {np.median(pm):.3f} ms, p99 {np.percentile(pm, 99):.3f} ms, "
          f"min {pm.min():.3f} ms, max {pm.max():.3f} ms")
    print(f"device per push (sr_profile): scoring {prof['gmm_ms'] / pushes:.3f} ms ({prof['gmm_launches']} launches), "
          f"search {prof['search_ms'] / pushes:.3f} ms ({prof['search_launches']} launches); frames {prof['frames']}")
    dev = prof["gmm_ms"] + prof["search_ms"]
    print(f"device share of push wall time: {dev / pm.sum():.1%} (the rest: copies, launches, synchronisation, host)")
    print(f"corpus: streamed in {stream_s:.3f} s (of which {pm.sum() / 1e3:.3f} s in sr_bigram_stream_push) vs one "
          f"sr_recognize_bigram_corpus {batch_s:.3f} s ({stream_s / batch_s:.1f}x)")
    print(f"streamed items equal the batch's (words, times, score bits): {'yes' if ok else 'NO'}")
    if args.stable:
        sm = np.asarray(stable_ms)
        print(f"sr_bigram_stream_stable on the pushed streams, after every push: median {np.median(sm):.3f} ms, p99 {np.percentile(sm, 99):.3f} ms, "
              f"min {sm.min():.3f} ms, max {sm.max():.3f} ms ({np.median(sm) / np.median(pm):.1%} of a push at the median)")
        print(f"stable items were a prefix of the final items: {'yes' if stable_ok else 'NO'}")
        ok = ok and stable_ok
    return 0 if ok else 1


def main_audio(args):
    from speechrecognition_amd import capi, synth

    D, shift, window = 39, 160, 400
    bigram = args.decoder == "bigram"
    kernel = {"mfma": capi.GMM_MFMA, "exact": capi.GMM_EXACT, "prefilter": capi.GMM_PREFILTER, "default": capi.GMM_DEFAULT}[args.kernel]
    lex = synth.make_lexicon(2666, 3, 1, extra_states_last=1) if bigram else synth.make_lexicon(1333, 3, 1)
    tmp = tempfile.mkdtemp(prefix="srstream_")
    mp = os.path.join(tmp, "model.mix")
    synth.write_mixset(mp, synth.make_mixset(lex.n_states, 64 if bigram else 32, D, seed=23))
    word_off, automaton, sil = lex.flatten()
    rng = np.random.default_rng(7)
    n = min(args.utts, 256)
    lens = rng.integers(200, 401, size=n)
    audio = [np.clip(np.rint(rng.normal(0.0, 300.0, window + (int(T) - 1) * shift)), -32768, 32767).astype(np.int16) for T in lens]
    mfcc = dict(sample_rate=16000.0, window=window, shift=shift, n_fft=512, n_mel=24, n_cepstra=13, f_low=0.0, f_high=8000.0,
                preemphasis=0.97, energy_floor=1.0)
    post = dict(n_static=13, n_first=13, n_second=13, deriv_step=3, energy_max_norm=0)
    n_warps = 13
    vtln = dict(alpha=[round(0.88 + 0.02 * i, 2) for i in range(n_warps)], break_frac=0.875) if args.vtln else None

    with capi.Model.from_mixset(mp, D) as m, m.frontend(mfcc, post, vtln=vtln) as fe:
        if bigram:
            lm_rng = np.random.default_rng(99)
            nW = lex.n_words
            lm = np.empty((nW, nW), np.float32)
            for h0 in range(0, nW, 256):
                pr = lm_rng.dirichlet(np.ones(nW), size=min(256, nW - h0))
                lm[:, h0:h0 + pr.shape[0]] = (-np.log(np.maximum(pr, 1e-30))).T
            net = m.bigram(word_off, automaton, lex.silence_idx, lm, np.array([[3.0, 0.0, 3.0, 150.0], [0.0001, 3.0, np.inf, 15.0]], np.float32))
            open_set = lambda: m.bigram_stream(net, 200.0, capi.FLT_MAX, kernel, max_streams=args.streams, max_frames=400)  # noqa: E731
        else:
            net = m.lexicon(word_off, automaton, lex.silence_idx, (3.0, 0.0, 30.0), sil)
            open_set = lambda: m.stream(net, 200.0, 10.0, kernel, max_streams=args.streams, max_frames=400)  # noqa: E731
        soff = np.concatenate([[0], np.cumsum([len(x) for x in audio])]).astype(np.uint64)
        corpus = fe.from_audio(np.concatenate(audio), soff)
        rows_all, foff = corpus.download(), corpus.frame_off.astype(np.int64)
        corpus.close()
        rows = [rows_all[foff[u]:foff[u + 1]] for u in range(n)]
        if args.vtln:  # what the warped run must give: the batch search on the batch front end's corpus, utterance u under warp u mod 13
            corpus = fe.from_audio_warped(np.concatenate(audio), soff, np.arange(n) % n_warps)
            if bigram:
                bw, bs, bt, boff = corpus.recognize_bigram(net, 200.0, capi.FLT_MAX, kernel)
                want = [(bw[int(boff[u]):int(boff[u + 1])], bs[int(boff[u]):int(boff[u + 1])], bt[int(boff[u]):int(boff[u + 1])]) for u in range(n)]
            else:
                words, woff = corpus.recognize(net, 200.0, 10.0, kernel)
                want = [words[int(woff[u]):int(woff[u + 1])] for u in range(n)]
            corpus.close()

        def run(as_audio, warped=False):
            src, k = (audio, args.piece * shift) if as_audio else (rows, args.piece)
            with open_set() as st:
                st.set_frontend(fe)

                def begin(u):
                    sid = st.begin()
                    if warped:
                        st.set_warp(sid, u % n_warps)
                    return sid

                warm = [begin(i) for i in range(args.streams)]  # warm: staging at the full push size, the kernels' code objects
                for _ in range(2):
                    (st.push_audio if as_audio else st.push)({sid: src[0][:k] for sid in warm})
                for sid in warm:
                    if as_audio:
                        st.finish_audio([sid])
                    st.end(sid)
                m.profile(True)
                todo, open_, got, ms = list(range(n)), {}, {}, []
                while todo or open_:
                    while todo and len(open_) < args.streams:
                        u = todo.pop(0)
                        open_[begin(u)] = (u, 0)
                    push = {sid: src[u][t0:t0 + k] for sid, (u, t0) in open_.items()}
                    t = time.perf_counter()
                    (st.push_audio if as_audio else st.push)(push)
                    ms.append(1e3 * (time.perf_counter() - t))
                    for sid in list(open_):
                        u, t0 = open_[sid]
                        t0 += len(push[sid])
                        if t0 == len(src[u]):
                            if as_audio:  # (the finish's three rows stay out of the pushes' device times)
                                capi.lib().sr_profile_enable(m.h, 0)
                                st.finish_audio([sid])
                                capi.lib().sr_profile_enable(m.h, 1)
                            got[u] = st.end(sid)
                            del open_[sid]
                        else:
                            open_[sid] = (u, t0)
                return np.asarray(ms), m.profile_read(), got

        a_ms, a_prof, a_got = run(True)
        if args.vtln:
            w_ms, w_prof, w_got = run(True, warped=True)
        f_ms, f_prof, f_got = run(False)
        net.close()

    def equal(x, y):
        if bigram:
            return all(np.array_equal(np.asarray(i).view(np.uint32), np.asarray(j).view(np.uint32)) for i, j in zip(x, y))
        return np.array_equal(x, y)

    same = all(equal(a_got[u], f_got[u]) for u in range(n))
    shape = "configs[4] shape (8000 states x 64, 2666 words), bigram stream" if bigram else "configs[2] model (4000 states x 32, 1333 words)"
    print(f"workload: {shape}, {n} noise utterances, {int(foff[-1])} frames, {args.streams} concurrent streams, gmm_kernel {args.kernel}")
    print(f"front end: window {window}, shift {shift}, n_fft 512, 24 filters, 13 + 13 + 13 features, step 3, no energy maximum")
    if args.vtln:
        print(f"warps: {n_warps} (alpha 0.88 .. 1.12, break 0.875); the warped run's utterance u carries warp u mod {n_warps}, the other runs' ids none")
    lines = [("audio push  ", a_ms, a_prof, f"{args.piece * shift} samples"), ("feature push", f_ms, f_prof, f"{args.piece} rows")]
    if args.vtln:
        lines.insert(1, ("warped audio", w_ms, w_prof, f"{args.piece * shift} samples"))
    for name, ms, prof, what in lines:
        print(f"{name} ({what} per stream): {len(ms)} pushes; wall median {np.median(ms):.3f} ms, p99 {np.percentile(ms, 99):.3f} ms, "
              f"min {ms.min():.3f} ms; device per push: scoring {prof['gmm_ms'] / len(ms):.3f} ms, search window {prof['search_ms'] / len(ms):.3f} ms "
              f"({prof['search_launches']} windows)")
    fe_ms = a_prof["search_ms"] / len(a_ms) - f_prof["search_ms"] / len(f_ms)
    print(f"stream_frontend_kernel (HIP events: the audio run's search windows minus the feature run's): {fe_ms:.3f} ms per push")
    print(f"audio push / feature push at the median: {np.median(a_ms) / np.median(f_ms):.2f}x (+{np.median(a_ms) - np.median(f_ms):.3f} ms)")
    print(f"the audio run's results equal the feature run's: {'yes' if same else 'NO'}")
    if args.vtln:
        wk_ms = w_prof["search_ms"] / len(w_ms) - f_prof["search_ms"] / len(f_ms)
        print(f"stream_frontend_kernel with warps (the warped run's search windows minus the feature run's): {wk_ms:.3f} ms per push "
              f"({wk_ms - fe_ms:+.3f} ms against no warps)")
        print(f"warped audio push / audio push at the median: {np.median(w_ms) / np.median(a_ms):.3f}x ({np.median(w_ms) - np.median(a_ms):+.3f} ms)")
        w_same = all(equal(w_got[u], want[u]) for u in range(n))
        print(f"the warped run's results equal the batch's on sr_corpus_from_audio_warped's corpus: {'yes' if w_same else 'NO'}")
        same = same and w_same
    return 0 if same else 1


def main_pipeline(args):
    from speechrecognition_amd import capi, synth

    D, c, p, shift, window = 39, 4, 39, 160, 400
    E = (2 * c + 1) * D
    bigram = args.decoder == "bigram"
    kernel = {"mfma": capi.GMM_MFMA, "exact": capi.GMM_EXACT, "prefilter": capi.GMM_PREFILTER, "default": capi.GMM_DEFAULT}[args.kernel]
    lex = synth.make_lexicon(2666, 3, 1, extra_states_last=1) if bigram else synth.make_lexicon(1333, 3, 1)
    tmp = tempfile.mkdtemp(prefix="srstream_")
    mp = os.path.join(tmp, "model.mix")
    synth.write_mixset(mp, synth.make_mixset(lex.n_states, 64 if bigram else 32, p, seed=23))
    word_off, automaton, sil = lex.flatten()
    rng = np.random.default_rng(7)
    n = min(args.utts, 256)
    lens = rng.integers(200, 401, size=n)
    M = np.hstack([rng.normal(size=(p, E)) / np.sqrt(E), rng.normal(size=(p, 1))])
    Ws = np.stack([np.hstack([np.eye(p) + 0.05 * rng.normal(size=(p, p)), rng.normal(size=(p, 1))]) for _ in range(args.streams)])
    mfcc = dict(sample_rate=16000.0, window=window, shift=shift, n_fft=512, n_mel=24, n_cepstra=13, f_low=0.0, f_high=8000.0,
                preemphasis=0.97, energy_floor=1.0)
    post = dict(n_static=13, n_first=13, n_second=13, deriv_step=3, energy_max_norm=0)
    if args.audio:
        inputs = [np.clip(np.rint(rng.normal(0.0, 300.0, window + (int(T) - 1) * shift)), -32768, 32767).astype(np.int16) for T in lens]
    else:
        inputs = [(rng.normal(size=(int(T), D)) * 3.0).astype(np.float32) for T in lens]
    holder = capi.Model.from_tables(np.arange(4, dtype=np.uint32), np.zeros((3, D)), np.ones((3, D)), np.zeros(3), np.zeros(3))

    with holder as src, capi.Model.from_mixset(mp, p) as m, src.frontend(mfcc, post) as fe_in, m.frontend(mfcc, post) as fe_own:
        if bigram:
            lm_rng = np.random.default_rng(99)
            nW = lex.n_words
            lm = np.empty((nW, nW), np.float32)
            for h0 in range(0, nW, 256):
                pr = lm_rng.dirichlet(np.ones(nW), size=min(256, nW - h0))
                lm[:, h0:h0 + pr.shape[0]] = (-np.log(np.maximum(pr, 1e-30))).T
            net = m.bigram(word_off, automaton, lex.silence_idx, lm, np.array([[3.0, 0.0, 3.0, 150.0], [0.0001, 3.0, np.inf, 15.0]], np.float32))
            open_set = lambda: m.bigram_stream(net, 200.0, capi.FLT_MAX, kernel, max_streams=args.streams, max_frames=400)  # noqa: E731
        else:
            net = m.lexicon(word_off, automaton, lex.silence_idx, (3.0, 0.0, 30.0), sil)
            open_set = lambda: m.stream(net, 200.0, 10.0, kernel, max_streams=args.streams, max_frames=400)  # noqa: E731
        # the batch route: the utterance begun u-th takes the transform of slot u mod streams
        ioff = np.concatenate([[0], np.cumsum([len(x) for x in inputs])]).astype(np.uint64)
        inp = fe_in.from_audio(np.concatenate(inputs), ioff) if args.audio else src.upload(np.concatenate(inputs), ioff)
        proj = inp.splice_transform(m, c, M)
        corpus = proj.transform(np.arange(n) % args.streams, Ws)
        rows_all, foff = corpus.download(), corpus.frame_off.astype(np.int64)
        if bigram:
            bw, bs, bt, boff = corpus.recognize_bigram(net, 200.0, capi.FLT_MAX, kernel)
            want = [(bw[int(boff[u]):int(boff[u + 1])], bs[int(boff[u]):int(boff[u + 1])], bt[int(boff[u]):int(boff[u + 1])]) for u in range(n)]
        else:
            words, woff = corpus.recognize(net, 200.0, 10.0, kernel)
            want = [words[int(woff[u]):int(woff[u + 1])] for u in range(n)]
        for x in (corpus, proj, inp):
            x.close()
        rows = [rows_all[foff[u]:foff[u + 1]] for u in range(n)]

        def run(piped):
            src_, k = (inputs, args.piece * shift) if args.audio else (inputs if piped else rows, args.piece)
            with open_set() as st:
                if piped:
                    st.set_projection(D, c, M)
                if args.audio:
                    st.set_frontend(fe_in if piped else fe_own)

                def push(batch):
                    if args.audio:
                        st.push_audio(batch)
                    elif piped:
                        st.push_rows(batch)
                    else:
                        st.push(batch)

                def finish(sid):  # (outside the pushes' device times, as the audio mode's)
                    capi.lib().sr_profile_enable(m.h, 0)
                    if args.audio:
                        st.finish_audio([sid])
                    elif piped:
                        st.push_rows({}, finish=[sid])
                    capi.lib().sr_profile_enable(m.h, 1)

                def begin(u):
                    sid = st.begin()
                    if piped:
                        st.set_transform(sid, Ws[u % args.streams])
                    return sid

                warm = [begin(i) for i in range(args.streams)]  # warm: staging at the full push size, the kernels' code objects
                for i in range(3):
                    push({sid: src_[0][i * k:(i + 1) * k] for sid in warm})
                for sid in warm:
                    finish(sid)
                    st.end(sid)
                m.profile(True)
                todo, open_, got, ms = list(range(n)), {}, {}, []
                while todo or open_:
                    while todo and len(open_) < args.streams:
                        u = todo.pop(0)
                        open_[begin(u)] = (u, 0)
                    batch = {sid: src_[u][t0:t0 + k] for sid, (u, t0) in open_.items()}
                    t = time.perf_counter()
                    push(batch)
                    ms.append(1e3 * (time.perf_counter() - t))
                    for sid in list(open_):
                        u, t0 = open_[sid]
                        t0 += len(batch[sid])
                        if t0 == len(src_[u]):
                            finish(sid)
                            got[u] = st.end(sid)
                            del open_[sid]
                        else:
                            open_[sid] = (u, t0)
                return np.asarray(ms), m.profile_read(), got

        p_ms, p_prof, p_got = run(True)
        f_ms, f_prof, f_got = run(False)
        net.close()

    def equal(x, y):
        if bigram:
            return all(np.array_equal(np.asarray(i).view(np.uint32), np.asarray(j).view(np.uint32)) for i, j in zip(x, y))
        return np.array_equal(x, y)

    same = all(equal(p_got[u], want[u]) for u in range(n))
    if not args.audio:  # (the plain run was fed the batch route's rows: the same results again)
        same = same and all(equal(f_got[u], want[u]) for u in range(n))
    shape = "configs[4] shape (8000 states x 64, 2666 words), bigram stream" if bigram else "configs[2] model (4000 states x 32, 1333 words)"
    unit = f"{args.piece * shift} samples" if args.audio else f"{args.piece} rows"
    print(f"workload: {shape}, {n} noise utterances, {int(foff[-1])} frames, {args.streams} concurrent streams, gmm_kernel {args.kernel}")
    print(f"pipeline: in_dim {D}, context {c} (E = {E}), model dimension {p}, a transform per stream"
          + ("; front end: window 400, shift 160, n_fft 512, 24 filters, 13 + 13 + 13 features, step 3, no energy maximum" if args.audio else ""))
    for name, ms, prof in (("pipeline push", p_ms, p_prof), ("plain push   ", f_ms, f_prof)):
        print(f"{name} ({unit} per stream): {len(ms)} pushes; wall median {np.median(ms):.3f} ms, p99 {np.percentile(ms, 99):.3f} ms, "
              f"min {ms.min():.3f} ms; device per push: scoring {prof['gmm_ms'] / len(ms):.3f} ms, search window {prof['search_ms'] / len(ms):.3f} ms "
              f"({prof['search_launches']} windows)")
    k_ms = p_prof["search_ms"] / len(p_ms) - f_prof["search_ms"] / len(f_ms)
    print(f"stream_pipeline_kernel (HIP events: the pipeline run's search windows minus the plain run's): {k_ms:.3f} ms per push")
    print(f"pipeline push / plain push at the median: {np.median(p_ms) / np.median(f_ms):.2f}x (+{np.median(p_ms) - np.median(f_ms):.3f} ms)")
    print(f"the pipeline run's results equal the batch route's: {'yes' if same else 'NO'}")
    return 0 if same else 1


if __name__ == "__main__":
    sys.exit(main())
