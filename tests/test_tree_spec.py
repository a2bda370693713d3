"""tree_spec.py on the CPU: the restated LBVH and PLOC trees are well formed on every input family of shared_inputs.py,
and the conditions that test_gpu_tree_spec.py relies on hold from the spec alone (which inputs are refused for their
depth, how deep tied clusters get, how many rounds regular tessellation takes)."""
import math

import numpy as np
import pytest

import tree_spec as T
from shared_inputs import TREE_FAMILY_NAMES, deep_lbvh, nan_cycle, numpy_boxes, tree_family, uniform_soup

SIZES = (1, 2, 3, 63, 64, 65, 1000, 4096)
LEAF_SIZES = (1, 4, 31)
BUILDERS = ("lbvh", "ploc")


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def check_tree(t, pos, leaf_size):
    n = np.asarray(pos).reshape(-1, 9).shape[0]
    assert sorted(t["prim_order"].tolist()) == list(range(n))
    leaf = t["right_offset"] == 0
    order = np.argsort(t["start"][leaf], kind="stable")
    st, cnt = t["start"][leaf][order].astype(np.int64), t["nprims"][leaf][order].astype(np.int64)
    assert st[0] == 0 and np.array_equal(st[1:], np.cumsum(cnt)[:-1]) and cnt.sum() == n  # leaves partition the slots
    assert cnt.max() <= leaf_size and cnt.min() >= 1
    assert np.all(t["nprims"][~leaf] > leaf_size)
    assert np.array_equal(bits(t["bbox"]), bits(numpy_boxes(t, pos)))
    # pre-order with the left child next: every inner node's children tile its range
    for i in np.nonzero(~leaf)[0]:
        l, r = i + 1, i + int(t["right_offset"][i])
        assert t["start"][l] == t["start"][i] and t["start"][r] == t["start"][l] + t["nprims"][l]
        assert t["nprims"][l] + t["nprims"][r] == t["nprims"][i]


@pytest.mark.parametrize("builder", BUILDERS)
@pytest.mark.parametrize("family", TREE_FAMILY_NAMES)
def test_trees_are_well_formed_and_within_the_stack(family, builder):
    for n in SIZES:
        for seed in (0, 1):  # the member a scene is created with, and the one it is rebuilt to
            pos, _ = tree_family(family, n, seed)
            assert np.isfinite(pos).all()
            for leaf_size in LEAF_SIZES if seed == 0 else (4,):
                t = T.BUILD[builder](pos, leaf_size)
                check_tree(t, pos, leaf_size)
                assert t.height <= 62 and not T.refused(t.height), (n, seed, t.height)
                assert len(t["start"]) == 1 if n <= leaf_size else len(t["start"]) >= 3


def test_keys_of_known_cells():
    pos, _ = deep_lbvh()
    keys = T.morton_keys(pos)
    assert keys == [0] + [1 << k for k in range(63)] + [(1 << 63) - 1]
    assert T.spread(0x1fffff) == 0x1249249249249249
    # an axis on which all centroids agree quantises to cell 0
    flat, _ = tree_family("zero_extent", 64)
    assert all(k & 0x1249249249249249 == 0 for k in T.morton_keys(flat))  # z: bits 0, 3, 6, ...
    # most of one_cell shares one key
    keys = T.morton_keys(tree_family("one_cell", 1000)[0])
    assert max(keys.count(k) for k in set(keys)) >= 990


def test_equal_keys_are_ordered_by_triangle():
    pos, _ = tree_family("coincident", 65)
    keys, order = T.morton_order(pos)
    assert len(set(keys)) == 1 and order.tolist() == list(range(65))
    t = T.lbvh(pos, 1)
    assert t["prim_order"].tolist() == list(range(65)) and t.height == 7  # a radix tree over the positions 0 .. 64


def test_deep_lbvh_is_refused_for_lbvh_only():
    pos, _ = deep_lbvh()
    t = T.lbvh(pos, 4)
    assert t.height >= 63 and T.refused(t.height) and T.build("lbvh", pos) is None
    check_tree(t, pos, 4)
    p = T.ploc(pos, 4)
    check_tree(p, pos, 4)
    assert p.height <= 62 and T.build("ploc", pos) is not None


@pytest.mark.parametrize("family", ["coincident", "same_box"])
@pytest.mark.parametrize("n", [64, 65, 1000, 4096])
def test_tied_clusters_pair_up(family, n):
    """equal union boxes everywhere: any rule that merges a constant fraction of the clusters per round is far inside
    2 ceil(log2 n); sending every cluster to its leftmost candidate gives n - 1"""
    pos, _ = tree_family(family, n)
    t = T.ploc(pos, 4)
    bound = 2 * math.ceil(math.log2(n))
    assert t.height <= bound and t.rounds <= bound, (t.height, t.rounds)


@pytest.mark.parametrize("family", ["strip", "grid"])
def test_regular_tessellation_takes_no_more_rounds_than_twice_a_random_soup(family):
    n = 4096
    yardstick = T.ploc(uniform_soup(n)[0]).rounds
    rounds = T.ploc(tree_family(family, n)[0]).rounds
    print(family, "rounds", rounds, "uniform random soup", yardstick)
    assert rounds <= 2 * yardstick


def pair_key(cost, lo, hi):
    return (cost, 0 if lo ^ 1 == hi else 1, lo, hi)


@pytest.mark.parametrize("family,n", [("coincident", 40), ("same_box", 40), ("strip", 70), ("grid", 70), ("duplicates", 90),
                                      ("huge", 50), ("scales", 90)])
def test_partner_scan_is_the_minimum_of_the_order_on_pairs(family, n):
    """the spec's scan in order of preference against the order written out pair by pair, and the best pair is mutual"""
    pos, _ = tree_family(family, n)
    _, tri = T.morton_order(pos)
    box = T.leaf_boxes(pos, tri)
    partner = T.nearest(box)
    keys = {}
    for i in range(n):
        for j in range(i + 1, min(i + T.RADIUS, n - 1) + 1):
            keys[(i, j)] = pair_key(float(T.half_area(box[i:i + 1], box[j:j + 1])[0]), i, j)
    for i in range(n):
        mine = [k for k in keys if i in k]
        best = min(mine, key=keys.get)
        assert partner[i] == best[0] + best[1] - i, i
    lo, hi = min(keys, key=keys.get)
    assert partner[lo] == hi and partner[hi] == lo


def test_nan_half_area_counts_as_the_worst():
    """three finite triangles whose outer pair unites to inf * 0: a NaN that no comparison removes leaves 0 -> 1 -> 2 -> 0
    and nothing to merge; as the worst cost the middle and right triangles merge first"""
    pos, _ = nan_cycle()
    _, tri = T.morton_order(pos)
    assert tri.tolist() == [0, 1, 2]
    box = T.leaf_boxes(pos, tri)
    with np.errstate(all="ignore"):
        dx, dy = box[2, 3] - box[0, 0], box[2, 4] - box[0, 1]
        assert np.isinf(dx) and dy == 0 and np.isnan(dx * dy)
    assert T.half_area(box[0:1], box[2:3])[0] == np.inf
    assert T.half_area(box[1:2], box[2:3])[0] < T.half_area(box[0:1], box[1:2])[0] < np.inf
    assert T.nearest(box).tolist() == [1, 2, 1]
    t = T.ploc(pos, 1)
    check_tree(t, pos, 1)
    assert t.rounds == 2 and t["prim_order"].tolist() == [0, 1, 2] and t["nprims"].tolist() == [3, 1, 2, 1, 1]
