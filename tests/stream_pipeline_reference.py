"""The pipeline of a stream set (include/srgpu.h: sr_stream_set_projection, sr_stream_set_transform, sr_stream_push_rows) restated in
numpy: both stages in float64 with the multiplication and the addition as separate, rounded operations in the documented order, the
intermediate row rounded to float32; and an utterance streamed in pieces, which keeps nothing but its last 2 context input rows."""
import numpy as np


def rows_out(received, context, finished):
    """rows searched once an utterance has received so many input rows"""
    return received if finished else max(received - context, 0)


def project_rows(window, t0, n, T, context, M):
    """rows t0 .. t0 + n - 1 of an utterance of T input rows; window(g) -> input row g as float32[D].  acc = M[i][E]; acc = acc +
    M[i][k] * z[k], k ascending"""
    M = np.asarray(M, dtype=np.float64)
    p, E = M.shape[0], M.shape[1] - 1
    out = np.empty((n, p), dtype=np.float32)
    for r in range(n):
        t = t0 + r
        z = np.concatenate([np.asarray(window(min(max(t + o, 0), T - 1)), dtype=np.float32) for o in range(-context, context + 1)]).astype(np.float64)
        assert len(z) == E
        acc = M[:, E].copy()
        for k in range(E):
            prod = M[:, k] * z[k]
            acc = acc + prod
        out[r] = acc.astype(np.float32)
    return out


def transform_rows(y, W):
    """acc = b_i; acc = acc + A_ij * (double) y_j, j ascending"""
    y = np.asarray(y, dtype=np.float32)
    if W is None:
        return y.copy()
    W = np.asarray(W, dtype=np.float64)
    p = W.shape[0]
    x = y.astype(np.float64)
    acc = np.repeat(W[None, :, p], len(y), axis=0)
    for j in range(p):
        prod = W[None, :, j] * x[:, j:j + 1]
        acc = acc + prod
    return acc.astype(np.float32)


def whole(x, context, M, W):
    """the rows of the whole utterance x float32[T, D]: the batch route's"""
    x = np.ascontiguousarray(x, dtype=np.float32)
    T = len(x)
    y = x if M is None else project_rows(lambda g: x[g], 0, T, T, context, M) if T else np.zeros((0, np.asarray(M).shape[0]), np.float32)
    return transform_rows(y, W)


class Streamed:
    """one utterance fed in pieces: push(rows, finish) -> the rows that became ready.  It keeps the last 2 context input rows."""

    def __init__(self, context, M, W):
        self.c = 0 if M is None else int(context)
        self.M, self.W = M, W
        self.received = self.searched = 0
        self.history = []          # [(g, row)], at most 2 context of them
        self.finished = False
        self.max_history = 0

    def push(self, rows, finish=False):
        assert not self.finished
        rows = np.ascontiguousarray(rows, dtype=np.float32)
        known = dict(self.history)
        known.update({self.received + i: r for i, r in enumerate(rows)})
        self.received += len(rows)
        self.finished = bool(finish)
        ready = rows_out(self.received, self.c, self.finished)
        n, t0 = ready - self.searched, self.searched
        if self.M is None:
            y = rows
            assert n == len(rows)
        elif n:
            y = project_rows(lambda g: known[g], t0, n, self.received, self.c, self.M)   # (a KeyError: a row no longer kept)
        else:
            y = np.zeros((0, np.asarray(self.M).shape[0]), np.float32)
        self.searched = ready
        keep = min(self.received, 2 * self.c)
        self.history = [(g, known[g]) for g in range(self.received - keep, self.received)]
        self.max_history = max(self.max_history, len(self.history))
        return transform_rows(y, self.W)
