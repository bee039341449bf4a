"""A plain restatement of the accelerator's binary tree (csrc/bvh_build.hpp, csrc/bvh_device.hip) in f64 numpy with np.float32 casts: the
stored box of a child (`ref_store`), the invariants every tree of this format satisfies whoever built it (`check_tree`), and the device's
linear BVH the slow, obvious way (`ref_lbvh`).  Test infrastructure: it neither imports nor calls the library."""
import bisect

import numpy as np

# csrc/device_scene.h DBvhNode: 64 bytes, both children's boxes (f32, relative to the tree's centre) and their references
NODE = np.dtype([("lo0", "<f4", 3), ("hi0", "<f4", 3), ("lo1", "<f4", 3), ("hi1", "<f4", 3), ("c0", "<i4"), ("c1", "<i4"), ("pad", "<i4", 2)])
assert NODE.itemsize == 64
KEY_BITS = 63


class TreeError(AssertionError):
    pass


def _need(cond, msg, *args):
    if not cond:
        raise TreeError(msg % args if args else msg)


def ref_store(box, center):
    """bvh::Builder::store: box[..., 0:3] = lo, box[..., 3:6] = hi (f64) -> (lo, hi) as f32, relative to `center`: padded by
    1e-9 * (|v| + ext) + 1e-30 with ext the box's longest side, the centre subtracted, cast to f32, and one ulp outward wherever the
    cast rounded inward."""
    box = np.asarray(box, dtype=np.float64)
    center = np.asarray(center, dtype=np.float64)
    lo, hi = box[..., 0:3], box[..., 3:6]
    with np.errstate(invalid="ignore", over="ignore"):
        ext = np.maximum(0.0, (hi - lo).max(axis=-1))[..., None]   # std::max(0.0, ...) over the three sides
        pl = 1e-9 * (np.abs(lo) + ext) + 1e-30
        ph = 1e-9 * (np.abs(hi) + ext) + 1e-30
        vlo = (lo - pl) - center
        vhi = (hi + ph) - center
        flo = vlo.astype(np.float32)
        fhi = vhi.astype(np.float32)
        flo = np.where(flo.astype(np.float64) > vlo, np.nextafter(flo, np.float32(-np.inf)), flo).astype(np.float32)
        fhi = np.where(fhi.astype(np.float64) < vhi, np.nextafter(fhi, np.float32(np.inf)), fhi).astype(np.float32)
    return flo, fhi


def ref_frame(boxes):
    """Centre and inf-norm radius of the items' bounds: bvh::build's frame[4]."""
    boxes = np.asarray(boxes, dtype=np.float64)
    lo, hi = boxes[:, 0:3].min(axis=0), boxes[:, 3:6].max(axis=0)
    center = 0.5 * (lo + hi)
    rad = max(0.0, float(np.maximum(np.abs(hi - center), np.abs(lo - center)).max()))
    return np.array([center[0], center[1], center[2], rad * (1.0 + 1e-6) + 1e-30])


def leaf_ref(first, count):
    """~(int32)((first << 3) | (count - 1)) as the builders write it."""
    u = np.uint32(((int(first) << 3) | (int(count) - 1)) & 0xFFFFFFFF)
    return int((~u).astype(np.uint32).view(np.int32))


def decode_leaf(ref):
    u = (~np.int32(ref)).view(np.uint32)
    return int(u >> np.uint32(3)), int(u & np.uint32(7)) + 1


def _present(lo, hi):
    return bool((lo <= hi).all())


def clamp_leaf(leaf_max):
    return 1 if leaf_max < 1 else (8 if leaf_max > 8 else int(leaf_max))


def check_tree(nodes, root, order, boxes, base, leaf_max, frame):
    """Raises TreeError unless (nodes, root, order) is a sound tree of this format over `boxes` (n x 6 f64): `order` a permutation, every
    node record reached exactly once from the root, every leaf 1..leaf_max items and the leaves tiling [base, base + n) once, every
    child box bit for bit ref_store of the exact union of the items below that child, `frame` the centre and padded radius.
    `leaf_max` is the value the builders use (already clamped to 1..8).  Returns the number of leaves."""
    nodes = np.asarray(nodes)
    _need(nodes.dtype == NODE and nodes.ndim == 1, "nodes must be a 1-D array of 64-byte records")
    boxes = np.asarray(boxes, dtype=np.float64)
    order = np.asarray(order)
    n, m = len(boxes), len(nodes)
    _need(len(order) == n and np.array_equal(np.sort(order.astype(np.int64)), np.arange(n)), "order is not a permutation of 0..%d", n - 1)
    want_frame = ref_frame(boxes)
    _need(np.array_equal(np.asarray(frame, dtype=np.float64).view(np.uint64), want_frame.view(np.uint64)), "frame %s, want %s", list(frame), list(want_frame))
    center = want_frame[0:3]
    _need(0 <= root < m, "root %d outside the %d node records", root, m)
    c = np.stack([nodes["c0"], nodes["c1"]], axis=1).astype(np.int64)
    lo = np.stack([nodes["lo0"], nodes["lo1"]], axis=1)
    hi = np.stack([nodes["hi0"], nodes["hi1"]], axis=1)
    # the walk: preorder list of nodes, every record exactly once
    seen = np.zeros(m, dtype=bool)
    seen[root] = True
    pre = [int(root)]
    todo = [int(root)]
    slots = []         # (node, side) of every present child
    while todo:
        i = todo.pop()
        for q in (0, 1):
            if not _present(lo[i, q], hi[i, q]):
                _need(i == root and q == 1 and n <= leaf_max, "node %d child %d is absent (inverted box) in a tree of %d items", i, q, n)
                continue
            slots.append((i, q))
            r = int(c[i, q])
            if r >= 0:
                _need(r < m, "node %d child %d refers to node %d of %d", i, q, r, m)
                _need(not seen[r], "node %d is reached twice (a cycle or a shared child)", r)
                seen[r] = True
                pre.append(r)
                todo.append(r)
    _need(seen.all(), "%d node records are not reachable from the root, first %d", int((~seen).sum()), int(np.argmin(seen)))
    # leaves: 1..leaf_max items each, tiling [base, base + n) exactly once
    leaves = [(i, q) + decode_leaf(c[i, q]) for (i, q) in slots if c[i, q] < 0]
    for (i, q, first, count) in leaves:
        _need(1 <= count <= leaf_max, "node %d child %d: a leaf of %d items, leaf_max is %d", i, q, count, leaf_max)
    leaves.sort(key=lambda t: t[2])
    at = base
    for (i, q, first, count) in leaves:
        _need(first == at, "the leaves do not tile [%d, %d): node %d child %d starts at item %d, the one before ends at %d (%s)", base, base + n, i, q, first, at,
              "overlap" if first < at else "gap")
        at = first + count
    _need(at == base + n, "the leaves end at item %d, want %d (items missing or in excess)", at, base + n)
    # exact unions bottom-up: a leaf's from its items, a node's from its two children's (min / max are exact and order-independent)
    sorted_boxes = boxes[order.astype(np.int64)]
    starts = np.array([t[2] - base for t in leaves], dtype=np.int64)
    leaf_lo = np.minimum.reduceat(sorted_boxes[:, 0:3], starts, axis=0)
    leaf_hi = np.maximum.reduceat(sorted_boxes[:, 3:6], starts, axis=0)
    child_box = np.empty((m, 2, 6), dtype=np.float64)
    child_box[:, 1, 0:3] = np.inf    # an absent child adds nothing to a union
    child_box[:, 1, 3:6] = -np.inf
    for k, (i, q, first, count) in enumerate(leaves):
        child_box[i, q, 0:3] = leaf_lo[k]
        child_box[i, q, 3:6] = leaf_hi[k]
    parent = {}
    for (i, q) in slots:
        if c[i, q] >= 0:
            parent[int(c[i, q])] = (i, q)
    for i in reversed(pre):      # children before parents
        if i == root:
            continue
        pi, pq = parent[i]
        child_box[pi, pq, 0:3] = np.minimum(child_box[i, 0, 0:3], child_box[i, 1, 0:3])
        child_box[pi, pq, 3:6] = np.maximum(child_box[i, 0, 3:6], child_box[i, 1, 3:6])
    idx = np.array(slots, dtype=np.int64)
    want_lo, want_hi = ref_store(child_box[idx[:, 0], idx[:, 1]], center)
    got_lo, got_hi = lo[idx[:, 0], idx[:, 1]], hi[idx[:, 0], idx[:, 1]]
    bad = (got_lo.view(np.uint32) != want_lo.view(np.uint32)).any(axis=1) | (got_hi.view(np.uint32) != want_hi.view(np.uint32)).any(axis=1)
    if bad.any():
        k = int(np.argmax(bad))
        small = bool((got_lo[k] > want_lo[k]).any() or (got_hi[k] < want_hi[k]).any())
        raise TreeError("%d of %d child boxes are not ref_store of the union of their items, first: node %d child %d is too %s: lo %s hi %s, want lo %s hi %s" % (
            int(bad.sum()), len(idx), idx[k, 0], idx[k, 1], "small" if small else "large", got_lo[k], got_hi[k], want_lo[k], want_hi[k]))
    return len(leaves)


# ---- the device's linear BVH (csrc/bvh_device.hip) --------------------------------------------------------------------------------------
def extent_bisection(ext):
    """The 63 bisections of the key: always the longest side of the current cell (the lower axis on a tie); an axis that already has
    30 bits hands the bit to the longest of the others.  Returns (bits per axis, the axis of each key bit, most significant first)."""
    cell = [e if (e > 0.0 and np.isfinite(e)) else 0.0 for e in (float(x) for x in ext)]
    bits, seq = [0, 0, 0], []
    for _ in range(KEY_BITS):
        a = 0
        for q in (1, 2):
            if cell[q] > cell[a]:
                a = q
        if bits[a] >= 30:
            best = -1
            for q in range(3):
                if bits[q] < 30 and (best < 0 or cell[q] > cell[best]):
                    best = q
            a = best
        bits[a] += 1
        cell[a] *= 0.5
        seq.append(a)
    return bits, seq


def ref_keys(boxes):
    """The 63-bit key of every item: the cell of its centroid in the bisection of the centroids' bounds."""
    boxes = np.asarray(boxes, dtype=np.float64)
    cen = 0.5 * (boxes[:, 0:3] + boxes[:, 3:6])
    clo, chi = cen.min(axis=0), cen.max(axis=0)
    ext = chi - clo
    bits, seq = extent_bisection(ext)
    q = []
    for a in range(3):
        scale = float(1 << bits[a]) / ext[a] * (1.0 - 1e-12) if (ext[a] > 0.0 and np.isfinite(ext[a])) else 0.0
        t = (cen[:, a] - clo[a]) * scale
        top = float((1 << bits[a]) - 1)
        t = np.where(t >= 0.0, t, 0.0)      # NaN / below
        t = np.where(t > top, top, t)
        q.append(t.astype(np.uint64))       # truncation
    rem = list(bits)
    key = np.zeros(len(boxes), dtype=np.uint64)
    for a in seq:
        rem[a] -= 1
        key = (key << np.uint64(1)) | ((q[a] >> np.uint64(rem[a])) & np.uint64(1))
    return key


def ref_lbvh(boxes, leaf_max, base):
    """The tree bvh_device.hip must produce, byte for byte: keys, a stable sort, a top-down split of [first, last] at the highest
    differing bit of the composite key (key, position), ranges of at most leaf_max items as leaves, kept nodes numbered in ascending
    order of their Karras index (root 0; the children of a split after position g are nodes g and g + 1).
    Returns (nodes, order, sorted keys, frame); None when the device builder declines (n < 2 or n <= leaf_max)."""
    boxes = np.asarray(boxes, dtype=np.float64)
    n = len(boxes)
    leaf_max = clamp_leaf(leaf_max)
    if n < 2 or n <= leaf_max:
        return None
    key = ref_keys(boxes)
    order = np.argsort(key, kind="stable").astype(np.uint32)
    skey = key[order]
    keys = [int(k) for k in skey]
    frame = ref_frame(boxes)

    def split(first, last):
        a, b = keys[first], keys[last]
        if a != b:
            bit = (a ^ b).bit_length() - 1
            return bisect.bisect_left(keys, (b >> bit) << bit, first, last + 1) - 1
        bit = (first ^ last).bit_length() - 1           # equal keys: told apart by position
        return ((last >> bit) << bit) - 1

    kept = []                      # (Karras index, (first, g), (g + 1, last))
    todo = [(0, 0, n - 1)]
    while todo:
        idx, first, last = todo.pop()
        g = split(first, last)
        kept.append((idx, (first, g), (g + 1, last)))
        if g - first + 1 > leaf_max:
            todo.append((g, first, g))
        if last - g > leaf_max:
            todo.append((g + 1, g + 1, last))
    created = [k[0] for k in kept]                      # parents before children
    new_index = {k: i for i, k in enumerate(sorted(created))}
    nodes = np.zeros(len(kept), dtype=NODE)
    sb = boxes[order.astype(np.int64)]
    union = {}                                          # Karras index -> exact box of the node's range
    child_boxes = np.empty((len(kept), 2, 6), dtype=np.float64)
    for (idx, left, right) in reversed(kept):           # children before parents
        me = new_index[idx]
        for q, (f, l) in enumerate((left, right)):
            if l - f + 1 > leaf_max:
                kid = l if q == 0 else f
                child_boxes[me, q] = union[kid]
                nodes["c%d" % q][me] = new_index[kid]
            else:
                child_boxes[me, q, 0:3] = sb[f:l + 1, 0:3].min(axis=0)
                child_boxes[me, q, 3:6] = sb[f:l + 1, 3:6].max(axis=0)
                nodes["c%d" % q][me] = leaf_ref(base + f, l - f + 1)
        union[idx] = np.concatenate([np.minimum(child_boxes[me, 0, 0:3], child_boxes[me, 1, 0:3]), np.maximum(child_boxes[me, 0, 3:6], child_boxes[me, 1, 3:6])])
    for q in (0, 1):
        flo, fhi = ref_store(child_boxes[:, q], frame[0:3])
        nodes["lo%d" % q] = flo
        nodes["hi%d" % q] = fhi
    return nodes, order, skey, frame
