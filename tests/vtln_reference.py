"""Vocal-tract-length normalisation as include/srgpu.h defines it (sr_frontend_create_warped, sr_vtln_costs_corpus, sr_vtln_choose),
restated in float64 numpy on top of tests/frontend_reference.py: the piecewise-linear warp, the warped filter weights (the unwarped
triangle evaluated at the warped bin frequency, computed in double and rounded to float), the MFCC stage under a warp, the costs'
sequential sums in their defined order, and the choice of a warp."""
import numpy as np

from tests import frontend_reference as R

ALPHAS = [round(0.88 + 0.02 * i, 2) for i in range(13)]   # 0.88 .. 1.12; ALPHAS[6] == 1.0
BREAK = 0.875


def warp(f, alpha, f_high, break_frac):
    """g_alpha(f); alpha == 1.0 is the identity by definition, with no arithmetic"""
    f = np.asarray(f, dtype=np.float64)
    if alpha == 1.0:
        return f.copy()
    f0 = break_frac * f_high * min(1.0, 1.0 / alpha)
    hi = alpha * f0 + (f_high - alpha * f0) / (f_high - f0) * (f - f0)
    return np.where(f <= f0, alpha * f, hi)


def filters(p, alpha, break_frac):
    """-> f32[n_mel, n_fft / 2 + 1]: the unwarped triangles at the warped bin frequencies"""
    N, nm = p["n_fft"], p["n_mel"]
    lo, hi = float(R.mel(p["f_low"])), float(R.mel(p["f_high"]))
    edges = R.mel_inv(lo + np.arange(nm + 2) * ((hi - lo) / (nm + 1)))
    fk = warp(np.arange(N // 2 + 1) * (p["sample_rate"] / N), alpha, p["f_high"], break_frac)
    left, centre, right = edges[:-2, None], edges[1:-1, None], edges[2:, None]
    return np.maximum(0.0, np.minimum((fk[None] - left) / (centre - left), (right - fk[None]) / (right - centre))).astype(np.float32)


def tables(p, alpha, break_frac):
    """frontend_reference.tables(p) with the filters of warp alpha: window, twiddles and DCT are shared by all warps"""
    win, tw, _, dct = R.tables(p)
    return win, tw, filters(p, alpha, break_frac), dct


def mfcc(samples, p, alpha, break_frac, with_energies=False):
    """one utterance under one warp: int16[n] -> f64[T, n_cepstra] (and the filter energies f64[T, n_mel]); frontend_reference.mfcc's
    stages with the warped filters"""
    samples = np.asarray(samples, dtype=np.int16)
    W, S, N = p["window"], p["shift"], p["n_fft"]
    T = R.n_frames(len(samples), p)
    win, tw, filt, dct = tables(p, alpha, break_frac)
    x = samples.astype(np.float64)
    pre = float(np.float32(p["preemphasis"]))
    y = x - pre * np.concatenate([[0.0], x[:-1]])
    idx = np.arange(T)[:, None] * S + np.arange(W)[None]
    fr = np.zeros((T, N))
    fr[:, :W] = y[idx] * win.astype(np.float64)[None]
    twc = tw[:, 0].astype(np.float64) + 1j * tw[:, 1].astype(np.float64)
    k = np.arange(N // 2 + 1)
    dft = twc[(np.arange(N)[:, None] * k[None]) % N]
    P = np.abs(fr @ dft) ** 2
    E = P @ filt.astype(np.float64).T
    L = np.log(np.maximum(E, float(np.float32(p["energy_floor"]))))
    c = L @ dct.astype(np.float64).T
    return (c, E) if with_energies else c


def seq_sum(values):
    """the sequential FP64 sum, the first addend taken as is; an empty sum is +0"""
    s = None
    for v in values:
        s = np.float64(v) if s is None else np.float64(s + np.float64(v))
    return np.float64(0.0) if s is None else s


def costs(scores, frame_off, utt_speaker, n_speakers):
    """scores f64[n_warps, frames] -> (cost f64[n_speakers, n_warps], frames u64[n_speakers]): per warp, an utterance's sequential sum
    over its frames in ascending order, then a speaker's sequential sum over its utterances in ascending index"""
    scores = np.asarray(scores, dtype=np.float64)
    off = np.asarray(frame_off).astype(np.int64)
    n_warps, n_utts = scores.shape[0], len(off) - 1
    cost = np.zeros((n_speakers, n_warps), dtype=np.float64)
    frames = np.zeros(n_speakers, dtype=np.uint64)
    for u in range(n_utts):
        frames[utt_speaker[u]] += np.uint64(off[u + 1] - off[u])
    for a in range(n_warps):
        utt = [seq_sum(scores[a, off[u]:off[u + 1]]) for u in range(n_utts)]
        for s in range(n_speakers):
            cost[s, a] = seq_sum(utt[u] for u in range(n_utts) if utt_speaker[u] == s)
    return cost, frames


def choose(cost, frames, min_frames, fallback):
    """the first warp of smallest cost; the fallback for fewer than min_frames frames, a NaN among the costs, a smallest cost not finite"""
    out = np.zeros(len(cost), dtype=np.uint32)
    for s, row in enumerate(np.asarray(cost, dtype=np.float64)):
        if frames[s] < min_frames or np.isnan(row).any() or not np.isfinite(row.min()):
            out[s] = fallback
        else:
            out[s] = int(np.argmin(row))   # (the first of equal minima)
    return out
