"""Streaming from audio (include/srgpu.h: sr_stream_push_audio), restated in numpy on top of tests/frontend_reference.py.

With energy_max_norm == 0 the streamed rows ARE the batch front end's, so frontend_reference.py restates them already.  What is new
is the causal energy maximum: component 0 of row t is the value without the maximum minus m(t), m(t) the maximum of that value over
frames 0 .. min(t + step, T - 1), kept by `<` alone."""
import numpy as np


def rows_out(statics, step, finished):
    """rows searched once an utterance has `statics` static frames"""
    return statics if finished else max(statics - step, 0)


def causal_max(rows, step):
    """rows: f32[T, nt] as the front end produces them WITHOUT the energy maximum -> a copy with the causal maximum applied"""
    rows = np.ascontiguousarray(rows, dtype=np.float32)
    out = rows.copy()
    T = len(rows)
    m = np.float32(-np.inf)
    seen = 0                                   # frames 0 .. seen - 1 are in m
    for t in range(T):
        upto = min(t + step, T - 1)
        while seen <= upto:
            v = rows[seen, 0]
            if m < v:                          # replaced on `<` alone: the first frame that reaches the maximum wins, -0 is told from +0
                m = v
            seen += 1
        out[t, 0] = rows[t, 0] - m             # float32 - float32: one rounding
    return out


def batch_max(rows):
    """the batch rule on the same rows: the maximum over the whole utterance (frontend_reference.post_process' loop)"""
    rows = np.ascontiguousarray(rows, dtype=np.float32)
    out = rows.copy()
    m = np.float32(-np.inf)
    for v in rows[:, 0]:
        if m < v:
            m = v
    if len(rows):
        out[:, 0] = rows[:, 0] - m
    return out
