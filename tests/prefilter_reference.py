"""The fp16 prefilter and the FP64 refinement, restated once in numpy for the tests that look at each kernel alone.

Prefilter (gmm_prefilter.hip header, pack_prefilter): the host's per-state norms of the fp16 coefficients and their rounding
residuals, the kernel's per-frame |b| and |b^ - b|, the candidate limit 2 eps = limD |b^ - b| + lim1 |b| + lim0, the fp16-emulated
scores, and -- from the tables a capi.Model is created from -- the exact scores, the pseudo-state layout of the mask words and the
limit per (frame, pseudo-state) (reference_limits), with the sandwich a mask array has to lie in (check_masks).

Refinement: every density's score in density_score_sse's operation order (density_scores) and the minimum over a mask's candidates
(masked_minimum): what gmm_refine_kernel has to store for ANY mask array, not only for the prefilter's."""
from __future__ import annotations

from types import SimpleNamespace

import numpy as np

F32, F16 = np.float32, np.float16
KAPPA16, KRES16 = F32(1.05e-3), F32(4.8835e-4)
POISON = 0xA5A5A5A5  # what sr_prefilter_masks fills the mask array with before the kernel runs


def bound_consts(ks32):
    """(acc, abs, sub) of pf_bound(ks32) (kernels.h)."""
    return (F32(1.6e-5), F32(7.0e-7), F32(3.38e-7)) if ks32 == 4 else (F32(1.1e-5), F32(6.0e-7), F32(2.92e-7))


def to_f16(v):
    """double -> float -> _Float16, as the host packs (and float -> _Float16, as the kernel packs)."""
    return np.asarray(v, dtype=np.float64).astype(F32).astype(F16).astype(np.float64)


def up(v):
    """The host's rounding up of a norm to float."""
    return np.nextafter((np.asarray(v, dtype=np.float64) * (1.0 + 1e-6)).astype(F32), F32(np.inf))


def pack_model(A, konst):
    """Scaled fp16 coefficients, the 3-term konst expansion and the per-density norms the host computes (pack_prefilter)."""
    big = max(np.max(np.abs(A)), np.max(np.abs(konst)))
    sA = 2.0 ** (13 - int(np.floor(np.log2(big))))
    As, ks = A * sA, konst * sA
    Ah = to_f16(As)
    kexp, rest = [], ks.copy()
    for _ in range(3):
        c = to_f16(rest)
        kexp.append(c)
        rest = rest - c
    norms = np.stack([up(np.sqrt(np.sum(As * As, 1))), up(np.abs(ks)), up(np.sqrt(np.sum((Ah - As) ** 2, 1))),
                      up(np.sqrt(np.sum(Ah * Ah, 1)))], 1)
    return As, ks, Ah, np.stack(kexp, 1), norms


def frame_side(X):
    """b = [x^2; x] interleaved, its fp16 image, and the kernel's bnorm and dbnorm (fp32, rounded up, dbnorm capped)."""
    T, D = X.shape
    X = X.astype(F32)
    b32 = np.empty((T, 2 * D), F32)
    b32[:, 0::2], b32[:, 1::2] = X * X, X
    bh = b32.astype(F16).astype(np.float64)
    bex = np.empty((T, 2 * D))
    bex[:, 0::2], bex[:, 1::2] = X.astype(np.float64) ** 2, X
    e = (bex - bh).astype(F32)  # fmaf(x, x, -b^) rounds the exact residual once; x - b^ is exact
    n2, e2 = np.zeros(T, F32), np.zeros(T, F32)
    for k in range(2 * D):
        n2 = (n2 + b32[:, k] * b32[:, k]).astype(F32)
        e2 = (e2 + e[:, k] * e[:, k]).astype(F32)
    bnorm = (np.sqrt(n2) * F32(1.0001)).astype(F32)
    dbn = np.minimum((np.sqrt(e2) * F32(1.0001)).astype(F32), (KRES16 * bnorm).astype(F32))
    return bh, bex, bnorm, dbn


def limits(nk, bnorm, dbn, ks32):
    """2 eps per (frame, state): (residual form, norm-only form) -- the host's folding of the state's norms into
    (lim1, limD, lim0) (pack_prefilter) and the kernel's limD |b^ - b| + lim1 |b| + lim0 in fp32."""
    kacc, kabs, ksub = bound_consts(ks32)
    na, nko, nd, nh = (nk[:, i].astype(F32) for i in range(4))
    lim0 = F32(2) * (kacc * nko + kabs * na)
    lim1_norm = F32(2) * (KAPPA16 * na + kabs)
    lim1_res = up(2.0 * (nd.astype(np.float64) + float(kacc) * nh + float(kabs)))
    limd_res = up(2.0 * (1.0 + float(kacc)) * nh.astype(np.float64))
    res = ((limd_res.astype(np.float64) * float(KRES16) + lim1_res <= lim1_norm * (1.0 - 2.0**-12))
           & ((1.0 + float(kacc)) * float(ksub) * nh.astype(np.float64) <= float(kabs) * na.astype(np.float64)))
    lim1, limd = np.where(res, lim1_res, lim1_norm), np.where(res, limd_res, F32(0))
    new = (limd[None] * dbn[:, None] + (lim1[None] * bnorm[:, None] + lim0[None])).astype(F32)
    old = (lim1_norm[None] * bnorm[:, None] + lim0[None]).astype(F32)
    return new, old, res


def emulated_scores(Ah, kexp, bh):
    """The prefilter's approximate scores [T, C] in fp32: products of two fp16 values are exact in fp32; fp32 accumulation in k
    order, the three konst slots last."""
    approx = np.zeros((bh.shape[0], len(Ah)), F32)
    for k in range(bh.shape[1]):
        approx = (approx + (bh[:, k:k + 1] * Ah[None, :, k]).astype(F32)).astype(F32)
    for t in range(3):
        approx = (approx + kexp[None, :, t].astype(F32)).astype(F32)
    return approx


def midpoints(rng, shape, lo=-6, hi=3):
    """Values exactly halfway between two neighbouring fp16 numbers (fp16 rounding's worst case)."""
    m = rng.integers(1024, 2048, size=shape) + 0.5
    return m * np.exp2(rng.integers(lo, hi, size=shape) - 10.0) * rng.choice([-1.0, 1.0], size=shape)


def pseudo_states(dens_off):
    """pack_prefilter's layout -> (Cs chunks of 32 densities per state: 1 / 2 / 4 / 8 by the largest mixture, the number of
    pseudo-states ps = state * Cs + chunk, the densities of each); mask word [ps >> 2][frame][ps & 3], density i of a chunk = bit i"""
    counts = np.diff(np.asarray(dens_off, dtype=np.int64))
    mx = int(counts.max())
    Cs = 1 if mx <= 32 else 2 if mx <= 64 else 4 if mx <= 128 else 8
    PS = len(counts) * Cs
    return Cs, PS, np.array([min(32, max(0, int(counts[ps // Cs]) - 32 * (ps % Cs))) for ps in range(PS)])


# ---- the masks against the documented limit ---------------------------------------------------------------------------------------------
def reference_limits(dens_off, means, inv_vars, norm, logw, feats):
    """From the tables a capi.Model is created from and the frames [T, D] (float32): the scaled exact scores in the GEMM form
    (`exact` [T, C], float64: the limit is >= 1e-3 |a||b|, far above float64's cancellation error here), the pseudo-state layout of
    pack_prefilter (Cs = 1 / 2 / 4 / 8 chunks of 32 densities per state, ps = state * Cs + chunk, mask word [ps >> 2][frame][ps & 3],
    density i of a chunk = bit i) and the candidate limit L[t, ps] = 2 eps by the header's formula, from the STATE's largest norms."""
    dens_off = np.asarray(dens_off, dtype=np.int64)
    means, inv_vars = np.asarray(means, dtype=np.float64), np.asarray(inv_vars, dtype=np.float64)
    feats = np.ascontiguousarray(feats, dtype=F32)
    C, D = means.shape
    S = len(dens_off) - 1
    A = np.empty((C, 2 * D))
    A[:, 0::2], A[:, 1::2] = 0.5 * inv_vars, -means * inv_vars
    konst = np.asarray(norm) - np.asarray(logw) + 0.5 * np.sum(means * means * inv_vars, 1)
    As, ks, Ah, kexp, norms = pack_model(A, konst)
    ok = np.all(np.isfinite(feats) & (np.abs(feats) <= 255.0), 1)  # frames whose fp16 operands are finite
    X = np.where(ok[:, None], feats, F32(0))  # (the others keep every density: no limit is looked at)
    bh, bex, bnorm, dbn = frame_side(X)
    exact = ks[None] + bex @ As.T
    exact[~ok] = np.nan
    Cs, PS, ps_count = pseudo_states(dens_off)
    ps_first = np.array([int(dens_off[ps // Cs]) + 32 * (ps % Cs) for ps in range(PS)])
    dens_ps = np.concatenate([np.full(ps_count[ps], ps) for ps in range(PS)]).astype(np.int64)
    dens_bit = np.concatenate([np.arange(ps_count[ps]) for ps in range(PS)]).astype(np.int64)
    assert np.array_equal(np.concatenate([ps_first[ps] + np.arange(ps_count[ps]) for ps in range(PS)]), np.arange(C))
    nst = np.stack([np.max(norms[dens_off[s]:dens_off[s + 1]], 0) for s in range(S)])
    ks32 = (2 * D + 3 + 31) // 32
    new, _, res = limits(nst, bnorm, dbn, ks32)
    L = np.repeat(new.astype(np.float64), Cs, axis=1)
    unit = np.arange(PS) // min(Cs, 4)  # what the minimum is taken over: the state, or its half of four chunks (Cs = 8)
    return SimpleNamespace(exact=exact, ok=ok, L=L, Cs=Cs, PS=PS, groups=(PS + 3) // 4, ps_count=ps_count, dens_ps=dens_ps,
                           dens_bit=dens_bit, dens_state=dens_ps // Cs, unit=unit, residual_form=res, Ah=Ah, kexp=kexp, bh=bh,
                           T=feats.shape[0], C=C, S=S)


def _gaps(ref):
    """gap [T, C]: a density's exact score minus the exact minimum of its state (of its half of four chunks when Cs = 8)."""
    du = ref.unit[ref.dens_ps]
    gap = np.empty_like(ref.exact)
    for u in np.unique(du):
        sel = du == u
        gap[:, sel] = ref.exact[:, sel] - np.min(ref.exact[:, sel], 1, keepdims=True)
    return gap


def _decisions(ref, ladder_states):
    gap = _gaps(ref)
    Ld = ref.L[:, ref.dens_ps]
    okc = ref.ok[:, None]
    ladder = np.isin(ref.dens_state, np.asarray(list(ladder_states), dtype=np.int64))[None, :]
    with np.errstate(invalid="ignore"):
        must_b = gap == 0.0
        must_not = okc & (gap > 2.0 * Ld * (1.0 + 1e-3))
        must_d = okc & ladder & (gap <= 0.5 * Ld)
    return gap, Ld, must_b, must_not, must_d, ladder & okc


def decided_share(ref, ladder_states):
    """The share of the ladder states' (frame, density) entries that rule (b), (c) or (d) of check_masks decides -- from the
    reference alone.  A model on which this is low tests little: the callers require 0.85."""
    _, _, must_b, must_not, must_d, entries = _decisions(ref, ladder_states)
    return float(np.sum((must_b | must_not | must_d) & entries)) / max(1, int(np.sum(entries)))


def mask_bits(masks, ref):
    """masks [groups][T][4] -> bool [T, C] in density order"""
    masks = np.asarray(masks)
    assert masks.dtype == np.uint32 and masks.shape == (ref.groups, ref.T, 4), (masks.dtype, masks.shape)
    words = masks[ref.dens_ps >> 2, :, ref.dens_ps & 3].T  # [T, C]
    return ((words >> ref.dens_bit[None, :].astype(np.uint32)) & np.uint32(1)).astype(bool)


def check_masks(masks, ref, ladder_states):
    """The sandwich a prefilter's mask array has to lie in.  gap = a density's exact score minus the exact minimum of its state (half);
    rules (c) to (e) on the frames whose features are finite with |x| <= 255:
      (a) no word is the hook's poison 0xA5A5A5A5;
      (b) every density with gap == 0 has its bit set;
      (c) no bit is set where gap > 2 L (1 + 1e-3): with |approx - exact| <= eps nothing beyond 4 eps = 2 L passes the kernel's test
          (1e-3: the fp32 evaluation of the limit);
      (d) in a ladder state (every density a copy of one, the weights apart) every density with gap <= L / 2 has its bit set: copies
          share their fp16 coefficients, so their approximate scores differ by the konst expansion and accumulation noise only;
      (e) every bit at or beyond the pseudo-state's density count and every slot beyond the last pseudo-state is zero;
      (f) a frame with a NaN, an inf or |x| > 255 keeps every real density's bit.
    Returns decided_share(ref, ladder_states); raises AssertionError naming the first offending (group, frame, slot, bit)."""
    masks = np.asarray(masks)
    gap, Ld, must_b, must_not, must_d, _ = _decisions(ref, ladder_states)

    def fail(rule, t, c, what):
        ps = int(ref.dens_ps[c])
        raise AssertionError(f"rule ({rule}): (group, frame, slot, bit) = ({ps >> 2}, {t}, {ps & 3}, {int(ref.dens_bit[c])}) {what}: "
                             f"gap {gap[t, c]:.6g}, L {Ld[t, c]:.6g}, word {int(masks[ps >> 2, t, ps & 3]):#010x}")

    bad = np.argwhere(masks == np.uint32(POISON))
    if bad.size:
        g, t, sl = (int(v) for v in bad[0])
        raise AssertionError(f"rule (a): (group, frame, slot) = ({g}, {t}, {sl}) still holds the poison word ({len(bad)} words)")
    bits = mask_bits(masks, ref)
    for rule, wrong, what in (("b", must_b & ~bits, "the exact minimum is not a candidate"),
                              ("c", must_not & bits, "is a candidate beyond twice the limit"),
                              ("d", must_d & ~bits, "a copy within half the limit is not a candidate"),
                              ("f", ~ref.ok[:, None] & ~bits, "a frame outside fp16's range dropped a density")):
        bad = np.argwhere(wrong)
        if bad.size:
            fail(rule, int(bad[0][0]), int(bad[0][1]), f"{what} ({len(bad)} entries)")
    # (e) padding: bits at or beyond the count of a pseudo-state, slots beyond the last pseudo-state
    valid = np.zeros(4 * ref.groups, np.uint32)
    valid[:ref.PS] = [0xFFFFFFFF if n >= 32 else (1 << int(n)) - 1 for n in ref.ps_count]
    extra = masks[:, ref.ok, :] & ~valid.reshape(ref.groups, 1, 4)
    bad = np.argwhere(extra != 0)
    if bad.size:
        g, ti, sl = (int(v) for v in bad[0])
        t = int(np.flatnonzero(ref.ok)[ti])
        raise AssertionError(f"rule (e): (group, frame, slot) = ({g}, {t}, {sl}) has padding bits set: word {int(masks[g, t, sl]):#010x}, "
                             f"{int(ref.ps_count[4 * g + sl]) if 4 * g + sl < ref.PS else 0} densities ({len(bad)} words)")
    return decided_share(ref, ladder_states)


def emulated_masks(ref, limit=None):
    """The masks the kernel's rule gives on the fp16-emulated scores: a density is a candidate where its approximate score is <= the
    smallest of its state (half) + the limit, in fp32; a frame outside fp16's range keeps everything.  limit: L [T, PS] -> the limit to
    use instead (the mutations the checker has to catch)."""
    L = ref.L if limit is None else limit(ref.L)
    approx = emulated_scores(ref.Ah, ref.kexp, ref.bh)
    du = ref.unit[ref.dens_ps]
    bits = np.zeros((ref.T, ref.C), bool)
    for u in np.unique(du):
        sel = np.flatnonzero(du == u)
        amin = np.min(approx[:, sel], 1)
        for c in sel:
            bits[:, c] = approx[:, c] <= (amin + L[:, ref.dens_ps[c]].astype(F32)).astype(F32)
    bits[~ref.ok] = True
    masks = np.zeros((ref.groups, ref.T, 4), np.uint32)
    for c in range(ref.C):
        ps = ref.dens_ps[c]
        masks[ps >> 2, :, ps & 3] |= bits[:, c].astype(np.uint32) << np.uint32(ref.dens_bit[c])
    return masks


LADDER = np.array([0.0, 1e-4, 1e-3, 1e-2, 1e-1, 1.0, 1e1, 1e2])


def heterogeneous_model(rng, M, D, S=18):
    """-> (tables for capi.Model.from_tables, ladder states).  S states of M densities (18: four full groups of state slots and a
    ragged one); the variance scale of state s is (0.01, 0.1, 1, 10)[s % 4], so the four slots of a group have limits far apart and a
    limit read from the wrong slot is a wrong limit; means ~ N(0, scale).  Even states are ladder states: all M densities are copies
    of one, their logw lowered by LADDER[i % 8] times a random factor in [0.5, 2) -- near ties at every distance from 1e-4 to 1e2,
    exact ties where the ladder repeats.  Odd states are random."""
    scale = np.array([0.01, 0.1, 1.0, 10.0])[np.arange(S) % 4]
    mu = rng.standard_normal((S, M, D)) * np.sqrt(scale)[:, None, None]
    var = (0.5 + np.abs(rng.standard_normal((S, M, D)))) * scale[:, None, None]
    logw = np.full((S, M), -np.log(M))
    ladder_states = list(range(0, S, 2))
    for s in ladder_states:
        mu[s], var[s] = mu[s, 0], var[s, 0]
        logw[s] -= LADDER[np.arange(M) % 8] * rng.uniform(0.5, 2.0, M)
    mu, var = mu.reshape(S * M, D), var.reshape(S * M, D)
    norm = 0.5 * (D * np.log(2 * np.pi) + np.sum(np.log(var), 1))
    return (np.arange(S + 1, dtype=np.uint32) * M, mu, 1.0 / var, norm, logw.reshape(-1)), ladder_states


def reference_frames(rng, D, T, mean0):
    """T frames: standard normal, of which (as far as they fit into T) 45 scaled by 0.1, 50 by 3, test_prefilter_bound_cpu's
    adversarial frames -- fp16 midpoints, fp16 subnormals, |x| near 255 -- and, from 5 frames on, five special ones first: a NaN, an
    inf, one beyond fp16's range (rule (f)), all zeros, and the mean of state 0's first density."""
    X = rng.standard_normal((T, D))
    sections = [(5, 50, lambda n: rng.standard_normal((n, D)) * 0.1),
                (50, 100, lambda n: rng.standard_normal((n, D)) * 3.0),
                (100, 130, lambda n: midpoints(rng, (n, D))),
                (130, 160, lambda n: rng.standard_normal((n, D)) * 1e-6),
                (160, 175, lambda n: rng.integers(-2**13, 2**13, size=(n, D)) * 2.0**-24),
                (175, 205, lambda n: rng.uniform(250.0, 255.0, size=(n, D)) * rng.choice([-1.0, 1.0], size=(n, D)))]
    for lo, hi, gen in sections:
        block = gen(hi - lo)  # (drawn whatever T is: the frames of a shorter set are a prefix of the longer one's kinds)
        if lo < T:
            X[lo:min(hi, T)] = block[: min(hi, T) - lo]
    X = X.astype(F32)
    if T >= 5:
        X[0, D // 2] = np.nan
        X[1, 0] = np.inf
        X[2, D - 1] = 300.0
        X[3] = 0.0
        X[4] = np.asarray(mean0, dtype=F32)
    return X


# ---- the refinement against density_score_sse ------------------------------------------------------------------------------------------
def density_scores(tables, feats):
    """Every density's score [T, C] (float64) in density_score_sse's operation order (Mixtures.cpp:645-690): partial sums over the
    even and the odd dimensions, l0 + l1, an odd dimension count's tail, norm + dist / 2, then - logw; element-wise numpy, one
    rounding per operation, no FMA.  tables = (dens_off, means, inv_vars, norm, logw) as capi.Model.from_tables takes them."""
    _, means, inv_vars, norm, logw = tables
    means, inv_vars = np.asarray(means, dtype=np.float64), np.asarray(inv_vars, dtype=np.float64)
    x = np.ascontiguousarray(feats, dtype=F32).astype(np.float64)
    T, D = x.shape
    C = means.shape[0]
    l0, l1 = np.zeros((T, C)), np.zeros((T, C))
    D2 = D - D % 2
    with np.errstate(invalid="ignore", over="ignore"):
        for d in range(D2):
            a = x[:, d:d + 1] - means[None, :, d]
            a = a * a
            a = a * inv_vars[None, :, d]
            if d & 1:
                l1 = l1 + a
            else:
                l0 = l0 + a
        dist = l0 + l1
        if D % 2:
            c = x[:, D - 1:D] - means[None, :, D - 1]
            c = c * c
            c = c * inv_vars[None, :, D - 1]
            dist = dist + c
        score = np.asarray(norm, dtype=np.float64)[None, :] + dist / 2
        score = score - np.asarray(logw, dtype=np.float64)[None, :]
    return score


def state_minimum(dens_off, scores):
    """min_score (Mixtures.cpp:696-713): per state the minimum under strict `<` from the seed 1e10 -- a NaN never wins"""
    dens_off = np.asarray(dens_off, dtype=np.int64)
    out = np.full((scores.shape[0], len(dens_off) - 1), 1e10)
    clean = np.where(np.isnan(scores), np.inf, scores)
    for s in range(len(dens_off) - 1):
        if dens_off[s + 1] > dens_off[s]:
            out[:, s] = np.minimum(1e10, np.min(clean[:, dens_off[s]:dens_off[s + 1]], 1))
    return out


def state_bits(dens_off, masks, s):
    """masks [groups][T][4] -> bool [T, densities of state s]: the candidates among the state's densities (bits at or beyond a
    pseudo-state's density count are no densities)"""
    Cs, _, ps_count = pseudo_states(dens_off)
    cols = []
    for ps in range(s * Cs, (s + 1) * Cs):
        w = masks[ps >> 2, :, ps & 3]
        cols.append(((w[:, None] >> np.arange(ps_count[ps], dtype=np.uint32)[None, :]) & np.uint32(1)).astype(bool))
    return np.concatenate(cols, 1)


def masked_minimum(dens_off, scores, masks, rows=None, step=1 << 16):
    """What the refinement has to store for these masks: per (frame, state) the minimum of scores[rows[t], density] over the set bits
    below the density count, strict `<` from the seed 1e10 -- a NaN never wins, an empty mask leaves 1e10.  rows: frame t's row of
    `scores` (default t).  -> (table [T, S], the number of set bits that are densities, whether every (frame, state) -- every half of
    four chunks when Cs = 8 -- that has densities has a candidate)"""
    dens_off = np.asarray(dens_off, dtype=np.int64)
    Cs, _, ps_count = pseudo_states(dens_off)
    T, S = masks.shape[1], len(dens_off) - 1
    rows = np.arange(T) if rows is None else np.asarray(rows)
    want = np.full((T, S), 1e10)
    n_bits, complete = 0, True
    for s in range(S):
        lo, hi = int(dens_off[s]), int(dens_off[s + 1])
        if hi == lo:
            continue
        for f0 in range(0, T, step):
            f1 = min(T, f0 + step)
            bits = state_bits(dens_off, masks[:, f0:f1], s)
            sc = scores[:, lo:hi][rows[f0:f1]]
            n_bits += int(bits.sum())
            halves = [bits] if Cs < 8 else [bits[:, :128], bits[:, 128:]]
            complete = complete and all(bool(np.all(h.any(1))) for h in halves if h.shape[1])
            m = np.min(np.where(bits & ~np.isnan(sc), sc, np.inf), 1)
            want[f0:f1, s] = np.minimum(1e10, m)
    return want, n_bits, complete
