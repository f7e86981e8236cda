"""The audio front end of include/srgpu.h (sr_frontend_*), restated in numpy.

MFCC stage: float64 throughout, on the tables the library uses -- window, twiddles, filter weights and DCT matrix computed in double,
rounded to float and widened again -- so that only the device's FP32 arithmetic separates the two.  The transform is a plain DFT
(a matrix product with the table's twiddles), not a fast one.

Post-processing stage: sr::FeaturePostProcessor::process_features in float32 and float64 numpy operations, one IEEE operation each,
so the result is the C++ loop's to the bit."""
import numpy as np

DEFAULT = dict(sample_rate=16000.0, window=400, shift=160, n_fft=512, n_mel=24, n_cepstra=12, f_low=0.0, f_high=8000.0,
               preemphasis=0.97, energy_floor=1.0)


def params(**kw):
    p = dict(DEFAULT)
    p.update(kw)
    return p


def signals(rate=16000.0, seed=0):
    """The four one-second test signals as int16: white noise (sigma 300), a 1 kHz tone of 8000 plus noise (sigma 100), a linear chirp
    of 6000 from 100 Hz to 90 % of the Nyquist rate plus noise (sigma 50), noise of sigma 3"""
    rng = np.random.default_rng(seed)
    n = int(rate)
    t = np.arange(n) / rate
    f0, f1 = 100.0, 0.45 * rate
    sig = [rng.normal(0.0, 300.0, n),
           8000.0 * np.sin(2.0 * np.pi * 1000.0 * t) + rng.normal(0.0, 100.0, n),
           6000.0 * np.sin(2.0 * np.pi * (f0 * t + 0.5 * (f1 - f0) * t * t)) + rng.normal(0.0, 50.0, n),
           rng.normal(0.0, 3.0, n)]
    return [np.clip(np.rint(s), -32768, 32767).astype(np.int16) for s in sig]


def n_frames(n_samples, p):
    return 0 if n_samples < p["window"] else 1 + (n_samples - p["window"]) // p["shift"]


def mel(f):
    return 2595.0 * np.log10(1.0 + np.asarray(f, dtype=np.float64) / 700.0)


def mel_inv(m):
    return 700.0 * (10.0 ** (np.asarray(m, dtype=np.float64) / 2595.0) - 1.0)


def tables(p):
    """-> window f32[window], twiddle (cos, -sin) f32[n_fft, 2], filters f32[n_mel, n_fft/2 + 1], dct f32[n_cepstra, n_mel]"""
    W, N, nm, nc = p["window"], p["n_fft"], p["n_mel"], p["n_cepstra"]
    win = (0.54 - 0.46 * np.cos(2.0 * np.pi * np.arange(W) / (W - 1))).astype(np.float32)
    ang = 2.0 * np.pi * np.arange(N) / N
    tw = np.stack([np.cos(ang), -np.sin(ang)], axis=1).astype(np.float32)
    lo, hi = float(mel(p["f_low"])), float(mel(p["f_high"]))
    edges = mel_inv(lo + np.arange(nm + 2) * ((hi - lo) / (nm + 1)))
    fk = np.arange(N // 2 + 1) * (p["sample_rate"] / N)
    left, centre, right = edges[:-2, None], edges[1:-1, None], edges[2:, None]
    filt = np.maximum(0.0, np.minimum((fk[None] - left) / (centre - left), (right - fk[None]) / (right - centre))).astype(np.float32)
    i, m = np.arange(nc)[:, None], np.arange(nm)[None]
    dct = (np.sqrt(2.0 / nm) * np.cos(np.pi * i * (m + 0.5) / nm)).astype(np.float32)
    return win, tw, filt, dct


def mfcc(samples, p, with_energies=False):
    """one utterance: int16[n] -> f64[T, n_cepstra] (and the filter energies f64[T, n_mel] before clamp and logarithm)"""
    samples = np.asarray(samples, dtype=np.int16)
    W, S, N = p["window"], p["shift"], p["n_fft"]
    T = n_frames(len(samples), p)
    win, tw, filt, dct = tables(p)
    x = samples.astype(np.float64)
    alpha = float(np.float32(p["preemphasis"]))
    y = x - alpha * np.concatenate([[0.0], x[:-1]])
    idx = np.arange(T)[:, None] * S + np.arange(W)[None]
    fr = np.zeros((T, N))
    fr[:, :W] = y[idx] * win.astype(np.float64)[None]
    twc = tw[:, 0].astype(np.float64) + 1j * tw[:, 1].astype(np.float64)
    k = np.arange(N // 2 + 1)
    dft = twc[(np.arange(N)[:, None] * k[None]) % N]   # [n, k] = exp(-2 pi i n k / N) from the table
    P = np.abs(fr @ dft) ** 2
    E = P @ filt.astype(np.float64).T
    L = np.log(np.maximum(E, float(np.float32(p["energy_floor"]))))
    c = L @ dct.astype(np.float64).T
    return (c, E) if with_energies else c


def mfcc_corpus(samples, sample_off, p):
    """-> cepstra f64[F, n_cepstra], frame_off u64[n_utts + 1]"""
    parts = [mfcc(samples[int(sample_off[u]):int(sample_off[u + 1])], p) for u in range(len(sample_off) - 1)]
    off = np.concatenate([[0], np.cumsum([len(x) for x in parts])]).astype(np.uint64)
    return (np.concatenate(parts) if parts else np.zeros((0, p["n_cepstra"]))), off


def post_process(cep, n_first, n_second, step, mean=None, stddev=None, energy_max_norm=True):
    """one utterance: f32[T, n_static] -> f32[T, n_static + n_first + n_second]"""
    cep = np.ascontiguousarray(cep, dtype=np.float32)
    T, nf = cep.shape
    out = np.zeros((T, nf + n_first + n_second), dtype=np.float32)
    if T == 0:
        return out
    out[:, :nf] = cep
    t = np.arange(T)
    a = np.minimum(np.maximum(t, step), T - 1)
    b = np.where(a >= step, a - step, 0)
    delta = cep[a, :n_first] - cep[b, :n_first]          # float32 - float32: one rounding
    out[:, nf:nf + n_first] = delta
    a2 = np.minimum(t, T - 1 - step) + step if T > step else np.full(T, T - 1)
    out[:, nf + n_first:] = delta[a2, :n_second] - delta[:, :n_second]
    if mean is not None:
        mean, stddev = np.asarray(mean, dtype=np.float64), np.asarray(stddev, dtype=np.float64)
        out = (out.astype(np.float64) - mean[None]).astype(np.float32)
        out = (out.astype(np.float64) / stddev[None]).astype(np.float32)
    if energy_max_norm:
        col = out[:, 0]
        mx = np.float32(-np.inf)
        for v in col:                                     # std::max(mx, v): replaced on `<` alone, which keeps the first of -0 / +0
            if mx < v:
                mx = v
        out[:, 0] = col - mx
    return out


def post_process_corpus(cep, frame_off, n_first, n_second, step, mean=None, stddev=None, energy_max_norm=True):
    cep = np.ascontiguousarray(cep, dtype=np.float32)
    parts = [post_process(cep[int(frame_off[u]):int(frame_off[u + 1])], n_first, n_second, step, mean, stddev, energy_max_norm)
             for u in range(len(frame_off) - 1)]
    return np.concatenate(parts) if parts else np.zeros((0, cep.shape[1] + n_first + n_second), dtype=np.float32)
