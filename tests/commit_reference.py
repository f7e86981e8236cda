"""The commit point of a set of nodes in an append-only tree (csrc/commit_point.h), restated in plain Python.

A tree is its parent array: parent[0] = 0 is the root, parent[j] < j.  The nearest common ancestor of a set is found by folding
it pairwise with `lca`; `brute_force` finds the same node as the deepest member of the intersection of the ancestor chains and
is what the fold is held against (tests/test_stream_stable_cpu.py)."""
import numpy as np


def lca(parent, a, b):
    a, b = int(a), int(b)
    while a != b:
        if a > b:
            a = int(parent[a])
        else:
            b = int(parent[b])
    return a


def commit_point(parent, nodes, floor=0):
    """The nearest common ancestor of `nodes`; an empty set leaves the commit point where it was (`floor`)."""
    nodes = [int(x) for x in nodes]
    if not nodes:
        return int(floor)
    c = nodes[0]
    for x in nodes[1:]:
        c = lca(parent, c, x)
    return c


def chain(parent, c):
    """c and its ancestors, up to the root"""
    c = int(c)
    out = [c]
    while c != 0:
        c = int(parent[c])
        out.append(c)
    return out


def brute_force(parent, nodes):
    common = None
    for x in nodes:
        s = set(chain(parent, x))
        common = s if common is None else common & s
    return max(common)  # ancestors of one node form a chain on which the index falls towards the root: the nearest is the largest


def random_forest(rng, n_nodes, depth_bias=0.0):
    """parent array of n_nodes nodes; depth_bias in [0, 1): how strongly a node prefers a recent parent (deep, narrow trees)"""
    parent = np.zeros(n_nodes, np.uint32)
    for j in range(1, n_nodes):
        lo = int(depth_bias * (j - 1))
        parent[j] = rng.integers(lo, j)
    return parent
