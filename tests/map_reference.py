"""numpy restatement of MAP adaptation as include/srgpu.h states it: the per-(speaker, density) sums of a set of pairs in the
documented order of summation (segments of 1024 pairs, one chain each, the partials added in ascending order), the adapted means and
the updated mixture weights.  Beside every sum the same sum in longdouble and over absolute values, which is what the tests' rounding
bounds are multiples of.  The weights go through math.exp / math.log: the process's libm, the one the library calls."""
import math

import numpy as np

from tests.fmllr_reference import alignment_pairs, posterior_pairs, random_model  # noqa: F401  (the tests take them from here)

SEG = 1024   # pairs per segment (include/srgpu.h)
LD = np.longdouble


def chain(rows, weights, seg=SEG):
    """rows f32[n, D], weights f64[n] in order -> (occ, x[D]): per segment a chain from 0.0, sum = sum + w * (double) x with the product
    rounded before the addition; the partials added in ascending order onto 0.0.  seg=None: one chain over all pairs."""
    n, D = rows.shape
    seg = n if seg is None else seg
    rows = rows.astype(np.float64)
    occ, x = 0.0, np.zeros(D)
    for s0 in range(0, n, max(seg, 1)):
        po, px = 0.0, np.zeros(D)
        for j in range(s0, min(n, s0 + seg)):
            w = float(weights[j])
            px = px + w * rows[j]
            po = po + w
        occ = occ + po
        x = x + px
    return occ, x


def entries(feats, pairs, frame_off, utt_speaker, n_speakers, seg=SEG):
    """pairs: (frame, density, weight) in the order they were formed -> dict(ent_off u64[S+1], dens u32[n], occ f64[n], x f64[n, D]:
    the documented order bit for bit; occ_ld, x_ld: the same sums in longdouble; x_abs: sum |w x|; n_pairs i64[n])"""
    F, D = feats.shape
    spk_of = np.zeros(F, dtype=np.int64)
    for u, s in enumerate(utt_speaker):
        spk_of[int(frame_off[u]):int(frame_off[u + 1])] = int(s)
    groups = {}
    for t, d, w in pairs:
        groups.setdefault((int(spk_of[t]), int(d)), []).append((t, w))
    keys = sorted(groups)
    n = len(keys)
    out = dict(ent_off=np.zeros(n_speakers + 1, np.uint64), dens=np.zeros(n, np.uint32), occ=np.zeros(n), x=np.zeros((n, D)),
               occ_ld=np.zeros(n, LD), x_ld=np.zeros((n, D), LD), x_abs=np.zeros((n, D), LD), n_pairs=np.zeros(n, np.int64))
    for e, (s, d) in enumerate(keys):
        ts = np.array([t for t, _ in groups[(s, d)]], dtype=np.int64)
        ws = np.array([w for _, w in groups[(s, d)]], dtype=np.float64)
        assert (np.diff(ts) >= 0).all()   # frames ascending
        out["ent_off"][s + 1:] += 1
        out["dens"][e] = d
        out["occ"][e], out["x"][e] = chain(feats[ts], ws, seg)
        terms = ws.astype(LD)[:, None] * feats[ts].astype(LD)
        out["occ_ld"][e] = ws.astype(LD).sum()
        out["x_ld"][e] = terms.sum(axis=0)
        out["x_abs"][e] = np.abs(terms).sum(axis=0)
        out["n_pairs"][e] = len(ts)
    return out


def map_means(means, dens_mean, dens, occ, x, tau):
    """mu'_ri = (tau * mu_ri + X_ri) / (tau + O_r), O_r and X_ri chains from 0.0 over the entries of mean row r in ascending density
    id; every density of the row gets those bits (the prior mean read is the row's lowest density's); other rows keep theirs"""
    out = means.copy()
    rows = {}
    for e, d in enumerate(dens):
        rows.setdefault(int(dens_mean[int(d)]), []).append(e)
    for r, ents in rows.items():
        O, X = 0.0, np.zeros(means.shape[1])
        for e in ents:
            O = O + float(occ[e])
            X = X + x[e]
        members = np.flatnonzero(dens_mean == r)
        out[members] = ((tau * means[members[0]] + X) / (tau + O))[None, :]
    return out


def map_weights(dens_off, logw, dens, occ, tau_w):
    """every mixture with an entry: n_d = tau_w * exp(logw_d) + occ_d, N their sum in mixture order, logw'_d = log(n_d / N)"""
    out = logw.copy()
    occ_of = {int(d): float(o) for d, o in zip(dens, occ)}
    for s in range(len(dens_off) - 1):
        c0, c1 = int(dens_off[s]), int(dens_off[s + 1])
        if not any(d in occ_of for d in range(c0, c1)):
            continue
        n = [tau_w * math.exp(float(logw[d])) + occ_of.get(d, 0.0) for d in range(c0, c1)]
        N = 0.0
        for v in n:
            N = N + v
        for d in range(c0, c1):
            out[d] = math.log(n[d - c0] / N)
    return out
