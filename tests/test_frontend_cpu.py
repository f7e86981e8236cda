"""The audio front end's numpy restatement (tests/frontend_reference.py) against what is known without a device: the reference's
own post-processed features of two real utterances, bit for bit, and the compiled sr::FeaturePostProcessor of
include/sr_sietill.hpp through tests/cpp/frontend_driver.cpp's host mode; and a few properties of the MFCC definition."""
import os
import struct
import subprocess

import numpy as np
import pytest

from tests import frontend_reference as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
REAL = os.path.join(ROOT, "tests", "golden_real", "sietill_real.npz")


def build_driver(directory):
    """tests/cpp/frontend_driver.cpp compiled into `directory` against the built library -> the program's path"""
    drv = os.path.join(str(directory), "frontend_driver")
    r = subprocess.run(["g++", "-O2", "-std=c++17", "-Wall", "-Werror", "-I" + os.path.join(ROOT, "include"),
                        os.path.join(ROOT, "tests", "cpp", "frontend_driver.cpp"), "-o", drv, "-L" + os.path.join(ROOT, "speechrecognition_amd"),
                        "-lsrgpu", "-Wl,-rpath," + os.path.join(ROOT, "speechrecognition_amd"), "-Wl,-rpath,/opt/rocm/lib"],
                       text=True, stdout=subprocess.PIPE, stderr=subprocess.STDOUT)
    assert r.returncode == 0, r.stdout[-3000:]
    return drv


@pytest.fixture(scope="module")
def built_lib():
    from speechrecognition_amd import build
    return build.build()


def post_blob(cep, off, n_first, n_second, step, energy, mean=None, stddev=None):
    cep = np.ascontiguousarray(cep, dtype=np.float32)
    off = np.ascontiguousarray(off, dtype=np.uint64)
    head = struct.pack("<7I", cep.shape[1], n_first, n_second, step, int(energy), int(mean is not None), len(off) - 1)
    norm = b"" if mean is None else np.asarray(mean, dtype="<f8").tobytes() + np.asarray(stddev, dtype="<f8").tobytes()
    return head + off.tobytes() + norm + cep.tobytes()


def run_driver(drv, mode, blob_path):
    """the driver's output lines by their first word: hex words as u32, frame_off as u64"""
    out = subprocess.run([drv, mode, str(blob_path)], text=True, stdout=subprocess.PIPE, stderr=subprocess.STDOUT)
    assert out.returncode == 0, out.stdout[-3000:]
    lines = {ln.split(" ", 1)[0]: ln.split()[1:] for ln in out.stdout.splitlines() if ln}
    return {k: (np.array([int(x, 16) for x in v], dtype=np.uint32) if k != "frame_off" else np.array([int(x) for x in v], dtype=np.uint64))
            for k, v in lines.items()}


def random_cepstra(rng, lengths, n_static):
    """cepstrum-like rows: component 0 large and negative at times, a few exact zeros of either sign and ties of the maximum"""
    off = np.concatenate([[0], np.cumsum(lengths)]).astype(np.uint64)
    cep = (rng.normal(size=(int(off[-1]), n_static)) * np.linspace(20.0, 1.0, n_static)[None]).astype(np.float32)
    return cep, off


def test_post_processing_reproduces_the_reference_corpus_reader():
    z = np.load(REAL)
    off = z["frame_off"].astype(np.int64)
    norm = z["normalization"].astype(np.float64)
    for i in (0, 1):
        raw = z[f"raw_mm2_{i}"].astype(np.float32).reshape(-1, 12)
        got = R.post_process(raw, 12, 1, 3, norm[:25], norm[25:], True)
        want = z["feats"][off[i]:off[i + 1]]
        assert got.shape == want.shape and np.array_equal(got.view(np.uint32), want.view(np.uint32))


@pytest.mark.parametrize("normalise", [False, True])
@pytest.mark.parametrize("energy", [False, True])
def test_post_processing_equals_the_compiled_host_loop(built_lib, tmp_path, normalise, energy):
    rng = np.random.default_rng(5 + 2 * normalise + energy)
    lengths = [1, 2, 3, 4, 7, 50]
    cep, off = random_cepstra(rng, lengths, 12)
    cep[int(off[4]) + 2, 0] = cep[int(off[4]):int(off[5]), 0].max()   # the maximum twice in one utterance
    cep[int(off[3]):int(off[4]), 0] = [-0.0, 0.0, -1.0, 0.0]           # a maximum of zero, -0 first
    mean = rng.normal(size=25) if normalise else None
    stddev = rng.uniform(0.5, 3.0, size=25) if normalise else None
    drv = build_driver(tmp_path)
    blob = tmp_path / "post.bin"
    blob.write_bytes(post_blob(cep, off, 12, 1, 3, energy, mean, stddev))
    got = run_driver(drv, "host", blob)["feats"].reshape(-1, 25)
    want = R.post_process_corpus(cep, off, 12, 1, 3, mean, stddev, energy)
    assert np.array_equal(got, want.view(np.uint32))


def test_framing_and_tables():
    p = R.params()
    assert [R.n_frames(n, p) for n in (399, 400, 559, 560, 16000)] == [0, 1, 1, 2, 98]
    win, tw, filt, dct = R.tables(p)
    assert np.isclose(win[0], 0.08, atol=1e-7) and np.allclose(win, win[::-1], atol=1e-7)
    assert tw[0, 0] == 1 and tw[0, 1] == 0 and tw[128, 0] == np.float32(np.cos(np.pi / 2)) and tw[128, 1] == -1
    assert filt.shape == (24, 257) and (filt.max(axis=1) > 0).all() and (filt >= 0).all() and filt.max() <= 1
    peak = filt.argmax(axis=1)
    assert (np.diff(peak) > 0).all()
    # the DCT rows are orthogonal with norm 1 (row 0: sqrt 2)
    g = dct.astype(np.float64) @ dct.astype(np.float64).T
    assert np.allclose(g, np.diag([2.0] + [1.0] * 11), atol=1e-6)


def test_mfcc_of_silence_is_the_floor():
    p = R.params()
    c = R.mfcc(np.zeros(1000, dtype=np.int16), p)
    assert c.shape == (4, 12)
    assert np.allclose(c[:, 0], np.sqrt(2.0 / 24) * 24 * np.log(1.0), atol=1e-12) and np.allclose(c[:, 1:], 0.0, atol=1e-12)
    q = R.params(energy_floor=2.0)
    c = R.mfcc(np.zeros(1000, dtype=np.int16), q)
    assert np.allclose(c[:, 0], np.sqrt(2.0 / 24) * 24 * np.log(2.0), atol=1e-6) and np.allclose(c[:, 1:], 0.0, atol=1e-6)


def test_mfcc_matches_a_fast_transform():
    """the table-driven DFT of the restatement against numpy's FFT: the same spectrum up to the table's rounding to float"""
    p = R.params()
    s = R.signals()[1][:4000]
    c, E = R.mfcc(s, p, with_energies=True)
    win, _, filt, _ = R.tables(p)
    x = s.astype(np.float64)
    y = x - float(np.float32(0.97)) * np.concatenate([[0.0], x[:-1]])
    fr = np.stack([y[t * 160:t * 160 + 400] * win for t in range(len(c))])
    P = np.abs(np.fft.rfft(fr, 512)) ** 2
    E2 = P @ filt.astype(np.float64).T
    assert np.allclose(E, E2, rtol=1e-4)
    # a frame does not know where the utterance was cut, except at the very first sample
    c2 = R.mfcc(s[160:], p)
    assert np.allclose(c[2:], c2[1:], atol=1e-9) and not np.allclose(c[1], c2[0], atol=1e-9)
