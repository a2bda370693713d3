"""A float32 numpy restatement of the two tree builders that run on the GPU (vermilion_amd/csrc/lbvh_build.hip), shared by
test_tree_spec.py (CPU) and test_gpu_tree_spec.py (the device's trees, bit for bit).

The library is compiled without FMA contraction, so float32 numpy with the same operation order gives the same bits.
Everything here is written for reading, not for speed, and none of it follows the kernels' formulation: the radix tree
is split top-down (the kernel searches ranges per node), a PLOC cluster scans its candidates in order of preference (the
kernel compares pairs), boxes are reduced over children after the fact.  Inputs are finite positions without negative
zeros (numpy's minimum and the device's fminf need not agree on the sign of a zero).

    lbvh(pos, leaf_size) / ploc(pos, leaf_size)  ->  Tree: the five arrays Scene.bvh() returns, height, rounds
"""
import numpy as np

RADIUS = 16              # VMX_PLOC_RADIUS: neighbours searched on each side
MAX_STACK = 64           # kMaxStack: build_device refuses height + 2 > 64
THIRD = np.float32(1.0) / np.float32(3.0)
GRID = np.float32(2097151.0)  # 2^21 - 1 cells per axis
TREE_KEYS = ("start", "nprims", "right_offset", "bbox", "prim_order")


class Tree(dict):
    """the flat arrays under their Scene.bvh() names, plus .height (edges from the root to the deepest triangle of the
    binary tree, before leaves are collapsed), .rounds (PLOC; 0 for the radix tree) and .root (binary node index)"""


def refused(height):
    """build_device's depth rule"""
    return height + 2 > MAX_STACK


# ---- centroids, Morton keys, the sort ---------------------------------------------------------------------------------
def centroids(pos):
    p = np.asarray(pos, np.float32).reshape(-1, 3, 3)
    with np.errstate(over="ignore"):
        return ((p[:, 0] + p[:, 1]) + p[:, 2]) * THIRD


def spread(q):
    """bit b of q -> bit 3b"""
    out = 0
    for b in range(21):
        out |= ((q >> b) & 1) << (3 * b)
    return out


def morton_keys(pos):
    c = centroids(pos)
    lo, hi = c.min(axis=0), c.max(axis=0)
    with np.errstate(all="ignore"):
        scale = np.where(hi > lo, GRID / (hi - lo), np.float32(0)).astype(np.float32)
        cell = (c - lo) * scale  # inf * 0 and inf - inf are NaN; fmax / fmin drop a NaN operand, as fmaxf / fminf do
        cell = np.fmin(np.fmax(cell, np.float32(0)), GRID)
    q = cell.astype(np.uint32)  # truncation
    return [spread(int(x)) << 2 | spread(int(y)) << 1 | spread(int(z)) for x, y, z in q]


def morton_order(pos):
    """(sorted keys, triangle of every sorted position): a stable sort, so equal keys keep the triangles' order"""
    keys = morton_keys(pos)
    order = sorted(range(len(keys)), key=lambda t: keys[t])  # sorted() is stable
    return [keys[t] for t in order], np.array(order, np.uint32)


def leaf_boxes(pos, tri_of_slot):
    p = np.asarray(pos, np.float32).reshape(-1, 3, 3)[tri_of_slot]
    return np.concatenate([p.min(axis=1), p.max(axis=1)], axis=1)


# ---- binary trees: children are node indices, or ~slot (negative) for the triangle at Morton position `slot` ---------
def radix_tree(keys):
    """The binary radix tree over the strings (key, position): all different, and sorted.  A range splits where the
    highest bit in which its first and last string differ changes from 0 to 1."""
    n = len(keys)
    word = [(k << 32) | i for i, k in enumerate(keys)]
    left, right = [], []

    def node(f, l):  # -> child reference of the range [f, l]
        if f == l:
            return ~f
        me = len(left)
        left.append(None), right.append(None)
        top = (word[f] ^ word[l]).bit_length() - 1
        split = f
        while not (word[split + 1] >> top) & 1:  # the last string whose bit `top` is 0
            split += 1
        todo.append((me, f, split, l))
        return me

    todo = []
    root = node(0, n - 1)
    while todo:
        me, f, split, l = todo.pop()
        left[me], right[me] = node(f, split), node(split + 1, l)
    return left, right, root


def half_area(a, b):
    """of the union box, in the kernel's operation order; a NaN (inf * 0 at overflowing extents) counts as the worst"""
    with np.errstate(all="ignore"):
        dx = np.maximum(a[:, 3], b[:, 3]) - np.minimum(a[:, 0], b[:, 0])
        dy = np.maximum(a[:, 4], b[:, 4]) - np.minimum(a[:, 1], b[:, 1])
        dz = np.maximum(a[:, 5], b[:, 5]) - np.minimum(a[:, 2], b[:, 2])
        area = (dx * dy + dy * dz) + dz * dx
    return np.where(np.isnan(area), np.float32(np.inf), area).astype(np.float32)


def nearest(box):
    """every cluster's partner.  Pairs are ordered by (cost, not a pair of positions 2k and 2k + 1, lower position,
    higher position): a strict total order, so the best pair overall is chosen from both sides and every round merges.
    Seen from cluster i that is: the partner i ^ 1 first, then the others by rising position, and a later candidate
    wins only with a strictly smaller cost."""
    nc = len(box)
    me = np.arange(nc)
    best = np.full(nc, np.inf, np.float32)
    partner = np.full(nc, -1)
    candidates = [me ^ 1] + [me + d for d in range(-RADIUS, RADIUS + 1) if d != 0]
    for j in candidates:
        ok = (j >= 0) & (j < nc)
        jj = np.where(ok, j, me)
        cost = half_area(box, box[jj])
        take = ok & ((partner < 0) | (cost < best))
        best = np.where(take, cost, best)
        partner = np.where(take, j, partner)
    return partner


def ploc_tree(box):
    """rounds of: nearest partner, mutual pairs merge (the lower position leads and keeps its place), the rest stay, order
    kept.  Node indices are handed out from the top: a round's merges take the indices below the previous round's, in
    position order from the highest down, so the last merge is node 0."""
    n = len(box)
    left, right = [None] * max(n - 1, 0), [None] * max(n - 1, 0)
    node = [~s for s in range(n)]
    box = np.array(box, np.float32)
    base, rounds = n - 1, 0
    while len(node) > 1:
        partner = nearest(box)
        new_node, new_box, merged = [], [], 0
        for i, j in enumerate(partner):
            mutual = partner[j] == i
            if mutual and i > j:
                continue  # absorbed by its partner
            if not mutual:
                new_node.append(node[i]), new_box.append(box[i])
                continue
            idx = base - 1 - merged
            merged += 1
            left[idx], right[idx] = node[i], node[j]
            new_node.append(idx)
            new_box.append(np.concatenate([np.minimum(box[i, :3], box[j, :3]), np.maximum(box[i, 3:], box[j, 3:])]))
        if merged == 0:
            raise RuntimeError("PLOC builder: a round merged nothing")
        node, box, base, rounds = new_node, np.array(new_box, np.float32), base - merged, rounds + 1
    assert base == 0 and (n == 1 or node[0] == 0)
    return left, right, node[0], rounds


# ---- the flat export ----------------------------------------------------------------------------------------------------
def flatten(left, right, root, tri_of_slot, pos, leaf_size):
    """Pre-order, left child at i + 1, right child at i + right_offset; a subtree of at most leaf_size triangles is one
    leaf (right_offset 0).  Leaf order is the depth-first order of the binary tree, start / nprims of every node cover
    its subtree, boxes are tight."""
    n = len(tri_of_slot)
    slot_box = leaf_boxes(pos, tri_of_slot)
    # depth first, left before right: the leaf order, and every node's range in it
    dfs_slots, first, count, height, box = [], {}, {}, {}, {}
    walk = [(root, False)]
    while walk:
        c, done = walk.pop()
        if c < 0:
            first[c], count[c], height[c], box[c] = len(dfs_slots), 1, 0, slot_box[~c]
            dfs_slots.append(~c)
        elif not done:
            walk += [(c, True), (right[c], False), (left[c], False)]
        else:
            l, r = left[c], right[c]
            first[c], count[c], height[c] = first[l], count[l] + count[r], max(height[l], height[r]) + 1
            box[c] = np.concatenate([np.minimum(box[l][:3], box[r][:3]), np.maximum(box[l][3:], box[r][3:])])
    assert len(dfs_slots) == n
    start, nprims, roff, bbox = [], [], [], []
    walk = [(root, None)]
    while walk:
        c, right_of = walk.pop()
        me = len(start)
        start.append(first[c]), nprims.append(count[c]), roff.append(0), bbox.append(box[c])
        if right_of is not None:
            roff[right_of] = me - right_of
        if count[c] > leaf_size:
            walk += [(right[c], me), (left[c], None)]
    t = Tree(start=np.array(start, np.uint32), nprims=np.array(nprims, np.uint32), right_offset=np.array(roff, np.uint32),
             bbox=np.array(bbox, np.float32).reshape(-1, 6), prim_order=np.asarray(tri_of_slot, np.uint32)[dfs_slots])
    t.height, t.root = height[root], root
    return t


def lbvh(pos, leaf_size=4):
    """VMX_BVH_LBVH"""
    keys, tri_of_slot = morton_order(pos)
    left, right, root = radix_tree(keys)
    t = flatten(left, right, root, tri_of_slot, pos, leaf_size)
    t.rounds = 0
    return t


def ploc(pos, leaf_size=4):
    """VMX_BVH_PLOC"""
    _, tri_of_slot = morton_order(pos)
    left, right, root, rounds = ploc_tree(leaf_boxes(pos, tri_of_slot))
    t = flatten(left, right, root, tri_of_slot, pos, leaf_size)
    t.rounds = rounds
    return t


BUILD = {"lbvh": lbvh, "ploc": ploc}


def build(builder, pos, leaf_size=4):
    """the tree, or None where build_device refuses it for its depth"""
    t = BUILD[builder](pos, leaf_size)
    return None if refused(t.height) else t
