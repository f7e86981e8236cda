"""numpy restatement of sr_model_split / sr_model_eliminate (include/srgpu.h): the plan (which densities split or survive, the new
dens_off, parents, tying, row renumbering) and the per-density tables, plus the hard-assignment EM pass (accumulate / finalize
without pooling) the training-from-scratch test replays on the CPU.  numpy's float64 division and square root are IEEE correctly
rounded, so every table here is the specified value to the bit; the logarithms go through math.log (the C library's, which the
library's host code calls: numpy's own vectorised log differs from it in the last bit on some CPUs)."""
import math

import numpy as np

POOL_GLOBAL, POOL_MIXTURE, POOL_NONE = 0, 1, 2
LN2 = float.fromhex("0x1.62e42fefa39efp-1")   # M_LN2


def _i64(a):
    return np.asarray(a, dtype=np.int64)


def split_plan(dens_off, n_mean, n_var, dens_mean, dens_var, mean_w, min_obs, pooling):
    """-> dict(dens_off, parent, sign, dens_mean, dens_var, n_mean, n_var)"""
    dens_off, dens_mean, dens_var = _i64(dens_off), _i64(dens_mean), _i64(dens_var)
    w = np.asarray(mean_w, dtype=np.float64)[dens_mean] if len(dens_mean) else np.zeros(0)
    with np.errstate(invalid="ignore"):
        flag = w >= min_obs                       # NaN: False
    upper_no = np.cumsum(flag) - 1                # j of a density's upper child, in mixture order over the whole model
    off, parent, sign, dm, dv = [0], [], [], [], []
    for s in range(len(dens_off) - 1):
        ks = np.arange(dens_off[s], dens_off[s + 1])
        up = ks[flag[ks]] if len(ks) else ks
        parent += ks.tolist() + up.tolist()
        sign += np.where(flag[ks], -1, 0).tolist() + [1] * len(up)
        dm += dens_mean[ks].tolist() + (n_mean + upper_no[up]).tolist()
        dv += dens_var[ks].tolist() + ((n_var + upper_no[up]) if pooling == POOL_NONE else dens_var[up]).tolist()
        off.append(len(parent))
    J = int(flag.sum())
    return dict(dens_off=np.asarray(off, np.uint32), parent=np.asarray(parent, np.uint32), sign=np.asarray(sign, np.int8),
                dens_mean=np.asarray(dm, np.uint32), dens_var=np.asarray(dv, np.uint32), n_mean=n_mean + J,
                n_var=n_var + J if pooling == POOL_NONE else n_var)


def eliminate_plan(dens_off, n_mean, n_var, dens_mean, dens_var, mean_w, min_obs):
    """-> dict(dens_off, parent, sign, dens_mean, dens_var, n_mean, n_var, mean_map, var_map) (maps: -1 where a row is dropped)"""
    dens_off, dens_mean, dens_var = _i64(dens_off), _i64(dens_mean), _i64(dens_var)
    mean_w = np.asarray(mean_w, dtype=np.float64)
    off, parent = [0], []
    for s in range(len(dens_off) - 1):
        ks = list(range(dens_off[s], dens_off[s + 1]))
        ws = [float(mean_w[dens_mean[k]]) for k in ks]
        keep = [k for k, w in zip(ks, ws) if w >= min_obs]
        if not keep and ks:
            # heaviest; NaN below everything; ties and all-NaN: the lowest index (max returns the first maximal element)
            keep = [max(zip(ks, ws), key=lambda kw: (0, 0.0) if math.isnan(kw[1]) else (1, kw[1]))[0]]
        parent += keep
        off.append(len(parent))
    parent = _i64(parent)
    used_m, used_v = np.unique(dens_mean[parent]), np.unique(dens_var[parent])   # ascending old index
    mean_map, var_map = np.full(n_mean, -1, np.int64), np.full(n_var, -1, np.int64)
    mean_map[used_m] = np.arange(len(used_m))
    var_map[used_v] = np.arange(len(used_v))
    return dict(dens_off=np.asarray(off, np.uint32), parent=parent.astype(np.uint32), sign=np.zeros(len(parent), np.int8),
                dens_mean=mean_map[dens_mean[parent]].astype(np.uint32), dens_var=var_map[dens_var[parent]].astype(np.uint32),
                n_mean=len(used_m), n_var=len(used_v), mean_map=mean_map, var_map=var_map)


def split_tables(tables, plan, epsilon):
    """tables = (means [C, D], inv_vars [C, D], norm [C], logw [C]) of the old model -> the same of the new one, and |delta| [C', D]"""
    means, ivars, norm, logw = (np.asarray(t, dtype=np.float64) for t in tables)
    p, sg = _i64(plan["parent"]), plan["sign"].astype(np.float64)
    with np.errstate(all="ignore"):
        sd = np.sqrt(1.0 / ivars[p])
        delta = epsilon * sd
        new_means = np.where(sg[:, None] > 0, means[p] + delta, np.where(sg[:, None] < 0, means[p] - delta, means[p]))
    new_logw = np.where(sg != 0, logw[p] - LN2, logw[p])
    return new_means, ivars[p].copy(), norm[p].copy(), new_logw, np.abs(delta) * (sg != 0)[:, None]


def eliminate_tables(tables, plan, dens_mean, mean_w, log=math.log):
    means, ivars, norm, _ = (np.asarray(t, dtype=np.float64) for t in tables)
    p = _i64(plan["parent"])
    w = np.asarray(mean_w, dtype=np.float64)[_i64(dens_mean)[p]] if len(p) else np.zeros(0)
    logw = np.zeros(len(p))
    off = _i64(plan["dens_off"])
    for s in range(len(off) - 1):
        total = 0.0
        for k in range(off[s], off[s + 1]):
            total += float(w[k])
        for k in range(off[s], off[s + 1]):
            with np.errstate(all="ignore"):
                q = np.float64(w[k]) / np.float64(total)
            logw[k] = (log(q) if q > 0 else (-math.inf if q == 0 else math.nan))
    return means[p].copy(), ivars[p].copy(), norm[p].copy(), logw


# ---- the hard-assignment EM pass (max-approx or first pass, no pooling), in the library's order of operations ---------------------

def density_scores(x, means, ivars, norm, logw):
    """-log(weight N(x)) per density in the exact kernel's order (gmm_exact.hip): even / odd partial sums, their sum, the odd tail"""
    D = means.shape[1]
    l0, l1 = np.zeros(len(means)), np.zeros(len(means))
    for d in range(0, D & ~1, 2):
        p = x[d] - means[:, d]
        l0 = l0 + p * p * ivars[:, d]
        q = x[d + 1] - means[:, d + 1]
        l1 = l1 + q * q * ivars[:, d + 1]
    dist = l0 + l1
    if D & 1:
        t = x[D - 1] - means[:, D - 1]
        dist = dist + t * t * ivars[:, D - 1]
    return norm + dist / 2 - logw


def accumulate(feats, states, dens_off, dens_mean, dens_var, n_mean, n_var, tables, first_pass):
    """sr_accumulate_corpus with first_pass or max_approx: every frame to density 0 / the arg-min density of its mixture, rows summed
    in frame order -> (mean_acc, mean_w, var_acc, var_w)"""
    D = feats.shape[1]
    means, ivars, norm, logw = tables if tables is not None else (None,) * 4   # a first pass reads no table
    ma, mw, va, vw = np.zeros((n_mean, D)), np.zeros(n_mean), np.full((n_var, D), 1e-4), np.zeros(n_var)
    for t in range(len(feats)):
        x = feats[t].astype(np.float64)
        c0, c1 = int(dens_off[states[t]]), int(dens_off[states[t] + 1])
        d = c0 if first_pass else c0 + int(np.argmin(density_scores(x, means[c0:c1], ivars[c0:c1], norm[c0:c1], logw[c0:c1])))
        r, q = int(dens_mean[d]), int(dens_var[d])
        ma[r] += x
        mw[r] += 1.0
        va[q] += x * x
        vw[q] += 1.0
    return ma, mw, va, vw


def finalize(dens_off, dens_mean, dens_var, acc):
    """MixtureModel::finalize without pooling (em_finalize.hip's order) -> (means, inv_vars, norm, logw) per density"""
    ma, mw, va, vw = acc
    dens_off, dens_mean, dens_var = _i64(dens_off), _i64(dens_mean), _i64(dens_var)
    D = ma.shape[1]
    with np.errstate(all="ignore"):
        mean_rows = ma / mw[:, None]
        src = np.full(len(vw), -1, np.int64)
        src[dens_var] = dens_mean                 # the last referencing density stays
        mu = mean_rows[np.maximum(src, 0)]
        var_rows = va / vw[:, None] - mu * mu
        ivar_rows = 1 / var_rows
    norm_rows = np.zeros(len(vw))
    for j in range(len(vw)):
        if src[j] < 0:
            var_rows[j] = 0.0
            ivar_rows[j] = 0.0
            continue
        a = D * math.log(2 * math.pi)
        for d in range(D):
            v = float(var_rows[j, d])
            a = a + (math.log(v) if v > 0 else (-math.inf if v == 0 else math.nan))
        norm_rows[j] = a / 2
    logw = np.zeros(len(dens_mean))
    for s in range(len(dens_off) - 1):
        total = 0.0
        for k in range(dens_off[s], dens_off[s + 1]):
            total += float(mw[dens_mean[k]])
        for k in range(dens_off[s], dens_off[s + 1]):
            with np.errstate(all="ignore"):
                q = np.float64(mw[dens_mean[k]]) / np.float64(total)
            logw[k] = math.log(q) if q > 0 else (-math.inf if q == 0 else math.nan)
    return mean_rows[dens_mean], ivar_rows[dens_var], norm_rows[dens_var], logw


# ---- the training-from-scratch case: corpus, linear segmentation, the schedule of Trainer::train on the CPU ------------------------

def training_case(seed=3, D=8, n_words=3, n_utts=40, separation=3.0):
    """silence + n_words words of 3 states; every state emits from two components `separation` standard deviations either side of
    its centre along a direction of its own -> (feats f32[F, D], frame_off u64[n_utts + 1], automata [u16 arrays], orths, n_states)"""
    rng = np.random.default_rng(seed)
    S = 1 + 3 * n_words
    centre = 4.0 * rng.normal(size=(S, D))
    direction = rng.normal(size=(S, D))
    direction /= np.linalg.norm(direction, axis=1, keepdims=True)
    feats, auts, orths, off = [], [], [], [0]
    for _ in range(n_utts):
        words = rng.integers(1, n_words + 1, size=int(rng.integers(2, 4)))
        aut = [0]
        for w in words:
            aut += [1 + 3 * (w - 1) + k for k in range(3)] + [0]
        aut = np.asarray(aut, dtype=np.uint16)
        T = int(rng.integers(55, 66))
        st = aut[linear_positions(T, len(aut))]
        side = rng.choice([-1.0, 1.0], size=T)
        feats.append((centre[st] + separation * side[:, None] * direction[st] + rng.normal(size=(T, D))).astype(np.float32))
        auts.append(aut)
        orths.append(words.astype(np.uint32))
        off.append(off[-1] + T)
    return np.concatenate(feats), np.asarray(off, dtype=np.uint64), auts, orths, S


def linear_positions(T, N):
    """linear segmentation: frame t of T sits at position t * N // T of the N positions (equal shares)"""
    return (np.arange(T, dtype=np.int64) * N) // T


def linear_segmentation(frame_off, automata):
    o = _i64(frame_off)
    return np.concatenate([a[linear_positions(int(o[u + 1] - o[u]), len(a))] for u, a in enumerate(automata)]).astype(np.uint16)


def am_score(feats, states, dens_off, tables):
    """calc_am_score: the sequential sum of the max-approx score of every frame's state, over the frame count"""
    means, ivars, norm, logw = tables
    total = 0.0
    for t in range(len(feats)):
        c0, c1 = int(dens_off[states[t]]), int(dens_off[states[t] + 1])
        total += float(density_scores(feats[t].astype(np.float64), means[c0:c1], ivars[c0:c1], norm[c0:c1], logw[c0:c1]).min())
    return total / len(feats)


def train_splits_cpu(feats, states, n_states, num_splits, min_obs, epsilon):
    """first pass, then per split: split / accumulate / finalize / eliminate / accumulate / finalize, on a fixed alignment, without
    pooling -> the average AM score after every finalize and the densities per mixture at the end"""
    off = np.arange(n_states + 1, dtype=np.uint32)
    dm = dv = np.arange(n_states, dtype=np.uint32)
    nm = nv = n_states
    acc = accumulate(feats, states, off, dm, dv, nm, nv, None, True)
    tables = finalize(off, dm, dv, acc)
    traj = [am_score(feats, states, off, tables)]
    for _ in range(num_splits):
        for op in ("split", "eliminate"):
            if op == "split":
                plan = split_plan(off, nm, nv, dm, dv, acc[1], min_obs, POOL_NONE)
                tables = split_tables(tables, plan, epsilon)[:4]
            else:
                plan = eliminate_plan(off, nm, nv, dm, dv, acc[1], min_obs)
                tables = eliminate_tables(tables, plan, dm, acc[1])
            off, dm, dv, nm, nv = plan["dens_off"], plan["dens_mean"], plan["dens_var"], plan["n_mean"], plan["n_var"]
            acc = accumulate(feats, states, off, dm, dv, nm, nv, tables, False)
            tables = finalize(off, dm, dv, acc)
            traj.append(am_score(feats, states, off, tables))
    return traj, np.diff(off.astype(np.int64))
