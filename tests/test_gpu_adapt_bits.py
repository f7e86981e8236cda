"""The bits of the fMLLR, MLLR and MLLT statistics and of the two affine transforms, pinned to the commit before the three contraction
kernels were folded into one (csrc/sym_contract.h).

The tests beside this one compare the device with a reference inside a rounding bound, which a changed order of summation would pass.
Here every output array is hashed (SHA-256 of its raw bytes) and compared with tests/golden/adapt_stats_bits.json, recorded from the
library of the commit the file names, on an MI355X, with digests() below; nothing is asserted but equality.

The corpora are make_case's (test_gpu_mllr.py: 60 utterances of 30-90 frames, 10 mixtures x 4 densities, speakers (0, 1, 0, 3, 0, 1)
of 4, classes 0 and 2 of 3 occupied): speaker 0 has about half of some 3600 frames -- more than one segment of 1024, a last stage
that is no multiple of 32 -- speaker 2 and class 1 are empty groups, and the soft memberships give MLLT about 14 segments.
D = 2, 25, 39, 63: one, two, three and four row tiles, so every instantiation of the contraction runs.  (At D = 63 the densities lie
so far apart that every soft membership but the best falls under the 1e-8 drop: fMLLR and MLLR then equal their arg-min runs, while
MLLT, whose dropped pairs keep their place, still walks four times the pairs.)"""
import hashlib
import json
import os

import numpy as np
import pytest

from speechrecognition_amd import capi
from tests import mllr_reference as R
from tests.test_gpu_mllr import N_CLASSES, TDP, aligned_states, make_case, open_model

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "adapt_stats_bits.json")
# (D, Baum-Welch entry points instead of the alignment's); each in arg-min and soft mode
CASES = [(2, False), (25, False), (39, False), (63, False), (39, True)]


def sha(a):
    return hashlib.sha256(np.ascontiguousarray(a, dtype=np.float64).tobytes()).hexdigest()


def statistics_digests(D, bw, max_approx, mllt_only=False):
    """name -> digest of every output array of the three statistics calls on one corpus"""
    model, feats, off, auts, spk, S, _, cls = make_case(D, 500 + D)
    out = {}
    with open_model(model, max_approx, False) as m:
        corpus = m.upload(feats, off)
        if bw:
            calls = {"mllt": lambda: corpus.mllt_statistics_bw(auts, TDP, 0, capi.GMM_DEFAULT, 0.0, max_approx)}
            if not mllt_only:
                calls["fmllr"] = lambda: corpus.fmllr_statistics_bw(auts, TDP, 0, spk, S, capi.GMM_DEFAULT, 0.0, max_approx)
                calls["mllr"] = lambda: corpus.mllr_statistics_bw(auts, TDP, 0, spk, S, cls, N_CLASSES, capi.GMM_DEFAULT, 0.0, max_approx)
            got = {}
            for name, call in calls.items():
                cost, got[name] = call()
                out[f"{name}.cost"] = sha(cost)
        else:
            states = aligned_states(corpus, auts, off)
            got = {"mllt": corpus.mllt_statistics(states, max_approx)}
            if not mllt_only:
                got["fmllr"] = corpus.fmllr_statistics(states, spk, S, max_approx)
                got["mllr"] = corpus.mllr_statistics(states, spk, S, cls, N_CLASSES, max_approx)
        corpus.close()
    for name, arrays in got.items():
        for part, a in zip(("beta", "G") if name == "mllt" else ("beta", "k", "G"), arrays):
            out[f"{name}.{part}"] = sha(a)
    return out


def transform_digests():
    """sr_corpus_transform (seen through the exact scores of the adapted corpus) and sr_model_transform_means at D = 39, seeded W"""
    D = 39
    model, feats, off, auts, spk, S, _, cls = make_case(D, 600 + D, n_utts=12)
    rng = np.random.default_rng(39)
    Ws = np.tile(np.hstack([np.eye(D), np.zeros((D, 1))]), (S, 1, 1)) + 0.05 * rng.normal(size=(S, D, D + 1))
    Wr = R.identity(D, N_CLASSES) + 0.2 * rng.normal(size=(N_CLASSES, D, D + 1))
    with open_model(model, True, False) as m:
        corpus = m.upload(feats, off)
        adapted = corpus.transform(spk, Ws)
        out = {"corpus_transform.scores": sha(adapted.score(capi.GMM_EXACT))}
        adapted.close()
        corpus.close()
        with m.transform_means(cls, Wr) as a:
            out["transform_means.means"] = sha(a.tables()[0])
    return out


def case_key(D, bw, max_approx):
    return f"{'bw' if bw else 'align'}/D{D}/{'argmin' if max_approx else 'soft'}"


def digests():
    """everything the golden file holds (the MLLT rounds run has no entry of its own: it must give the one-round digests)"""
    out = {case_key(D, bw, ma): statistics_digests(D, bw, ma) for D, bw in CASES for ma in (True, False)}
    out["transforms/D39"] = transform_digests()
    return out


@pytest.fixture(scope="module")
def golden():
    with open(GOLDEN) as f:
        return json.load(f)["digests"]


@pytest.mark.parametrize("max_approx", [True, False])
@pytest.mark.parametrize("D,bw", CASES)
def test_statistics_bits(golden, D, bw, max_approx):
    assert statistics_digests(D, bw, max_approx) == golden[case_key(D, bw, max_approx)]


def test_mllt_rounds_bits(golden, monkeypatch):
    """a workspace of 1 MiB holds 3 segments of D = 39, so the soft pairs take several rounds: the same digests"""
    monkeypatch.setenv("SRGPU_MLLT_MB", "1")
    want = {k: v for k, v in golden[case_key(39, False, False)].items() if k.startswith("mllt.")}
    assert len(want) == 2 and statistics_digests(39, False, False, mllt_only=True) == want


def test_transform_bits(golden):
    assert transform_digests() == golden["transforms/D39"]
