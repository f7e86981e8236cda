"""The device fold of csrc/commit_point.h alone (sr_commit_points): on forests supplied by the test it must return exactly what
tests/commit_reference.py returns -- single and equal candidates, candidates that meet at the root, a floor equal to the answer,
set sizes around a wave (64), the workgroup and its strided loop, shallow and deep chains, many sets in one call -- and refuse
malformed input with SR_EINVAL."""
import numpy as np
import pytest

from speechrecognition_amd import capi, synth
from tests import commit_reference as ref

pytestmark = pytest.mark.gpu

SR_EINVAL = -1


@pytest.fixture(scope="module")
def model(tmp_path_factory):
    spec = synth.make_mixset(4, 1, 8, seed=7001)  # any model: the call only needs its device and stream
    mp = str(tmp_path_factory.mktemp("commit") / "tiny.mix")
    synth.write_mixset(mp, spec)
    with capi.Model.from_mixset(mp, 8) as m:
        yield m


def _chain(n):
    """node j hangs under j - 1: depth n - 1"""
    return np.concatenate([[0], np.arange(n - 1)]).astype(np.uint32)


def _check(model, parents, sets, floors=None):
    got = capi.commit_points(model, parents, sets, floors)
    want = [ref.commit_point(p, s) for p, s in zip(parents, sets)]
    assert [int(x) for x in got] == want
    return want


def test_single_equal_and_root_candidates(model):
    rng = np.random.default_rng(7002)
    tree = ref.random_forest(rng, 400, 0.9)
    star = np.zeros(50, np.uint32)  # every node hangs under the root
    want = _check(model, [tree, tree, star, star, np.zeros(1, np.uint32)],
                  [[377], [123] * 300, [7, 31], np.arange(1, 50), [0, 0, 0]])
    assert want == [377, 123, 0, 0, 0]


def test_floor_equal_to_the_answer_and_floors_above_the_root(model):
    rng = np.random.default_rng(7003)
    parents, sets, floors = [], [], []
    for _ in range(12):
        tree = ref.random_forest(rng, 600, 0.98)
        nodes = rng.integers(300, 600, size=90)
        c = ref.commit_point(tree, nodes)
        up = ref.chain(tree, c)
        for f in (c, up[len(up) // 2], 0):  # the answer itself, an ancestor of it half way up, the root
            parents.append(tree); sets.append(nodes); floors.append(f)
    want = _check(model, parents, sets, floors)
    assert sum(w != 0 for w in want) >= 6  # deep narrow trees: the candidates do meet below the root


@pytest.mark.parametrize("depth_bias", [0.0, 0.995])
def test_set_sizes_around_wave_and_workgroup(model, depth_bias):
    rng = np.random.default_rng(7004)
    tree = ref.random_forest(rng, 3000, depth_bias)
    sizes = (1, 63, 64, 65, 1024, 1025, 2500)
    sets = [rng.integers(1500, 3000, size=n) for n in sizes]
    # a second copy whose candidates all sit under one deep node, so that the answer is not the root whatever the size
    deep = _chain(400)
    hung = np.concatenate([deep, np.full(2600, 399, np.uint32)])  # nodes 400 .. 2999 hang under the chain's end
    sets2 = [rng.integers(400, 3000, size=n) for n in sizes]
    want = _check(model, [tree] * len(sizes) + [hung] * len(sizes), sets + sets2)
    assert want[len(sizes) + 1:] == [399] * (len(sizes) - 1)


def test_chains_of_depth_1_and_300(model):
    two, long = _chain(2), _chain(301)
    fork = np.concatenate([long, [150, 301, 302, 200]]).astype(np.uint32)  # two branches off the chain, at 150 and at 200
    want = _check(model, [two, two, long, long, fork, fork], [[1], [0, 1], [300], [300, 17, 250], [303, 300], [304, 303]])
    assert want == [1, 0, 300, 17, 150, 150]


def test_17_sets_of_different_sizes_in_one_call(model):
    rng = np.random.default_rng(7005)
    parents, sets = [], []
    for i in range(17):
        n = int(rng.integers(2, 900))
        parents.append(ref.random_forest(rng, n, float(rng.choice([0.0, 0.9, 0.99]))))
        sets.append(rng.integers(n // 2, n, size=1 + 37 * i))
    want = _check(model, parents, sets)
    assert len(set(want)) > 3


def test_malformed_input_is_einval(model):
    good = _chain(5)
    cases = {
        "parent not below its child": ([np.array([0, 0, 2, 1, 1], np.uint32)], [[1]], None),
        "parent[0] not 0": ([np.array([1, 0], np.uint32)], [[1]], None),
        "node out of range": ([good], [[1, 5]], None),
        "floor out of range": ([good], [[1]], [5]),
        "empty set": ([good, good], [[1], []], None),
    }
    for name, (parents, sets, floors) in cases.items():
        with pytest.raises(capi.SrError) as e:
            capi.commit_points(model, parents, sets, floors)
        assert e.value.code == SR_EINVAL, name
    assert len(capi.commit_points(model, [], [])) == 0
