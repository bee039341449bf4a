"""Inputs for the builder tests (test_bvh_builder_cpu.py, test_bvh_builder_gpu.py) and the ctypes side of the library's builder hook
(include/rtc.h rtc_bvh_build_raw / rtc_bvh_collapse_raw).  Every family is a function of (n, seed): n small boxes around centroids that
stress one special case of csrc/bvh_device.hip."""
import ctypes as C
import functools

import numpy as np

import bvh_ref

vp = C.c_void_p
RTC_BVH_STACK = 64      # csrc/device_scene.h: a tree whose stack_need exceeds RTC_BVH_STACK - 1 is not traversed


# ---- the hook -------------------------------------------------------------------------------------------------------------------------
class Built:
    def __init__(self, rc, nodes=None, root=-1, order=None, keys=None, frame=None, depth=0, stack_need=0, n_nodes=0):
        self.rc, self.nodes, self.root, self.order, self.keys, self.frame = rc, nodes, root, order, keys, frame
        self.depth, self.stack_need, self.n_nodes = depth, stack_need, n_nodes


def build_raw(lib, boxes, leaf_max, base, where, nodes_cap=None, order_cap=None, keys_cap=None):
    """One call of the hook.  Default capacities: n node records, n order entries, n keys (where = 1)."""
    boxes = np.ascontiguousarray(boxes, dtype=np.float64)
    n = len(boxes)
    nodes_cap = n if nodes_cap is None else nodes_cap
    order_cap = n if order_cap is None else order_cap
    keys_cap = (n if where == 1 else 0) if keys_cap is None else keys_cap
    guard = 0x5A
    nodes = np.full(max(nodes_cap, 1), guard, dtype=np.uint8).repeat(64).view(bvh_ref.NODE)
    order = np.full(max(order_cap, 1), 0x5A5A5A5A, dtype=np.uint32)
    keys = np.full(max(keys_cap, 1), 0x5A5A5A5A5A5A5A5A, dtype=np.uint64)
    n_nodes, root, depth, need = C.c_uint32(0), C.c_int32(-7), C.c_int32(-7), C.c_int32(-7)
    frame = np.zeros(4)
    rc = lib.rtc_bvh_build_raw(boxes.ctypes.data, n, leaf_max, base, where, nodes.ctypes.data, nodes_cap, C.addressof(n_nodes), order.ctypes.data, order_cap,
                               keys.ctypes.data if keys_cap else None, keys_cap, C.addressof(root), frame.ctypes.data, C.addressof(depth), C.addressof(need))
    if rc != 0:
        untouched = bool((nodes.view(np.uint8) == guard).all() and (order == 0x5A5A5A5A).all() and (keys == 0x5A5A5A5A5A5A5A5A).all())
        b = Built(rc, n_nodes=n_nodes.value)
        b.untouched = untouched
        return b
    return Built(rc, nodes[:n_nodes.value].copy(), root.value, order[:n].copy(), keys[:n].copy() if keys_cap else None, frame, depth.value, need.value, n_nodes.value)


def collapse_raw(lib, nodes, root):
    """(rc, depth, stack_need) of bvh::collapse4 on a node array."""
    nodes = np.ascontiguousarray(nodes)
    depth, need = C.c_int32(-7), C.c_int32(-7)
    rc = lib.rtc_bvh_collapse_raw(nodes.ctypes.data, len(nodes), root, C.addressof(depth), C.addressof(need))
    return rc, depth.value, need.value


# ---- the input families ---------------------------------------------------------------------------------------------------------------
def _boxes(cen, half):
    return np.concatenate([cen - half, cen + half], axis=1)


def _dyadic(rng, shape, hi=1024, scale=1.0 / 1024):
    """Random multiples of 2^-10 in (0, 1]: sums and differences of such centroids and half sizes are exact, so 'the same centroid' is."""
    return rng.randint(1, hi + 1, size=shape).astype(np.float64) * scale


def fam_a(n, rng):
    """uniform random in a cube"""
    return _boxes(rng.uniform(-3.0, 5.0, (n, 3)), rng.uniform(0.0, 0.05, (n, 3)))


def fam_b(n, rng):
    """all centroids identical, box sizes differ: every key equal, the tree is decided by position alone"""
    return _boxes(np.tile(np.array([1.5, -2.25, 3.0]), (n, 1)), _dyadic(rng, (n, 3)))


def fam_c(n, rng):
    """37 distinct centroids, each repeated a random 1..600 times (scaled so that the runs add up to n), shuffled: runs of equal
    keys that cross block boundaries"""
    reps = rng.randint(1, 601, size=37).astype(np.float64)
    reps = np.maximum(1, np.floor(reps * (n / reps.sum()))).astype(np.int64) if n >= 37 else (np.arange(37) < n).astype(np.int64)
    while reps.sum() > n:
        reps[np.argmax(reps)] -= 1
    reps[0] += n - reps.sum()
    cen = (rng.randint(-2 ** 20, 2 ** 20, size=(37, 3)).astype(np.float64) / 1024.0).repeat(reps, axis=0)
    out = _boxes(cen, _dyadic(rng, (n, 3), hi=64))
    return out[rng.permutation(n)]


def fam_d(n, rng):
    """flat: the y extent of the centroids (and of the boxes) is exactly 0"""
    cen = rng.uniform(-10.0, 10.0, (n, 3))
    half = rng.uniform(0.0, 0.1, (n, 3))
    cen[:, 1] = 0.0
    half[:, 1] = 0.0
    return _boxes(cen, half)


def fam_e(n, rng):
    """a line: y and z extents exactly 0"""
    cen = rng.uniform(-10.0, 10.0, (n, 3))
    half = rng.uniform(0.0, 0.1, (n, 3))
    cen[:, 1:] = 0.0
    half[:, 1:] = 0.0
    return _boxes(cen, half)


def fam_f(n, rng):
    """the x extent is 2^40 times the others: x reaches 30 bits and hands the rest to y and z"""
    cen = rng.uniform(0.0, 1.0, (n, 3))
    cen[:, 0] *= 2.0 ** 40
    cen[0] = 0.0
    cen[n - 1] = (2.0 ** 40, 1.0, 1.0)
    return _boxes(cen, rng.uniform(0.0, 0.01, (n, 3)))


def fam_g(n, rng):
    """two clusters nine decades apart in scale: one 1e3 wide, one 1e-6 wide"""
    k = n // 2
    big = rng.uniform(-500.0, 500.0, (k, 3))
    small = np.array([123.0, -77.0, 41.0]) + rng.uniform(0.0, 1e-6, (n - k, 3))
    cen = np.concatenate([big, small])
    half = np.concatenate([rng.uniform(0.0, 1.0, (k, 3)), rng.uniform(0.0, 1e-8, (n - k, 3))])
    p = rng.permutation(n)
    return _boxes(cen[p], half[p])


H_BITS = 21         # the unit cube's bisection gives every axis 21 of the 63 bits
H_CHAIN = 2 + 3 * H_BITS


def chain_centroids(n):
    """Family (h): sorted keys with pairwise distinct highest set bits.  The low corner (key 0) and the high corner (all ones) of the
    unit cube pin the bounds; on each axis one item at distance 2^-j (1 + 1e-3) from the low corner for j = 1..21: its cell index on
    that axis is 2^(21 - j) plus low bits, 0 on the others, so its key's highest set bit is that axis's bit j.  Each split then peels
    one item off: a chain of about 60 binary levels.  The n - 65 remaining items are copies of the low corner's centroid (key 0): a
    balanced subtree (split by position) at the chain's lower end.  Fewer than 65 items: the corners and the first n - 2 of the chain."""
    pts = [(0.0, 0.0, 0.0), (1.0, 1.0, 1.0)]
    for j in range(1, H_BITS + 1):
        for a in range(3):
            p = [0.0, 0.0, 0.0]
            p[a] = 2.0 ** -j * (1.0 + 1e-3)
            pts.append(tuple(p))
    pts = pts[:max(2, min(n, H_CHAIN))]
    return np.array(pts + [(0.0, 0.0, 0.0)] * (n - len(pts)))


def fam_h(n, rng):
    """the deep chain (chain_centroids)"""
    cen = chain_centroids(n)
    half = rng.randint(1, 1025, size=(n, 3)).astype(np.float64) * 2.0 ** -40    # exact: every centroid is what chain_centroids says
    p = rng.permutation(n)
    return _boxes(cen[p], half[p])


def fam_i(n, rng):
    """a regular grid with a smooth height: the height-field pattern"""
    nx = int(np.ceil(np.sqrt(n)))
    j, i = np.divmod(np.arange(n), nx)
    x, z = -20.0 + 40.0 * i / max(nx - 1, 1), -20.0 + 40.0 * j / max(nx - 1, 1)
    cen = np.stack([x, 0.7 * np.sin(0.3 * x + 0.2 * z), z], axis=1)
    return _boxes(cen, np.full((n, 3), 20.0 / max(nx - 1, 1)) * np.array([1.0, 0.2, 1.0]))


FAMILIES = {"a_uniform": fam_a, "b_one_centroid": fam_b, "c_runs": fam_c, "d_flat": fam_d, "e_line": fam_e, "f_long_x": fam_f, "g_two_scales": fam_g, "h_chain": fam_h,
            "i_grid": fam_i}
SIZES = [5, 255, 256, 257, 513, 4099, 65537]     # leaf_max + 1, around the 256-thread block, several blocks, 257 blocks
LEAF_SWEEP = [1, 2, 8]                           # families (a) and (c) besides leaf_max = 4
H_DEEP = 4099                                    # the size at which family (h) outgrows the traversal stack (test_bvh_builder_cpu.py)


@functools.lru_cache(maxsize=None)
def boxes_of(family, n, seed=20240607):
    b = FAMILIES[family](n, np.random.RandomState((seed + 7919 * sorted(FAMILIES).index(family) + n) % (2 ** 32)))
    b.setflags(write=False)
    return b


def cases(max_n):
    """(family, n, leaf_max, base): every family at leaf_max 4 and every size up to max_n; 2 and 3 items at leaf_max 1; families (a) and
    (c) at leaf sizes 1, 2, 8 (at leaf_max + 1 items and at two larger sizes); a second base."""
    out = []
    for f in sorted(FAMILIES):
        out += [(f, n, 4, 0) for n in SIZES if n <= max_n]
        out += [(f, 2, 1, 0), (f, 3, 1, 0)]
    for f in ("a_uniform", "c_runs"):
        for lm in LEAF_SWEEP:
            out += [(f, n, lm, 0) for n in (lm + 1, 257, 4099) if n <= max_n]
        out += [(f, 513, 4, 12345), (f, 257, 8, 12345)]
    return out


def case_id(c):
    return "%s-n%d-leaf%d-base%d" % c


@functools.lru_cache(maxsize=None)
def reference(family, n, leaf_max, base):
    """ref_lbvh of a case: computed once, shared by the tests of a session, never modified."""
    out = bvh_ref.ref_lbvh(boxes_of(family, n), leaf_max, base)
    if out is not None:
        for a in out:
            a.setflags(write=False)
    return out


# ---- meshes for the render-level tests --------------------------------------------------------------------------------------------------
def tris_around(cen, half):
    """One triangle per centroid whose bounding box is centroid +- half: (-, -, -), (+, -, +), (0, +, 0) corners."""
    cen, half = np.asarray(cen, dtype=np.float64), np.broadcast_to(np.asarray(half, dtype=np.float64), np.shape(cen))
    s = np.array([[-1.0, -1.0, -1.0], [1.0, -1.0, 1.0], [0.0, 1.0, 0.0]])
    return cen[:, None, :] + s[None, :, :] * half[:, None, :]


def tri_boxes(tris):
    """The bounds the scene builder gives a triangle (p1, p1 + e1, p1 + e2 with the edges e = p - p1, as the flattened scene holds them)."""
    p1 = tris[:, 0]
    v = np.stack([p1, p1 + (tris[:, 1] - p1), p1 + (tris[:, 2] - p1)], axis=1)
    return np.concatenate([v.min(axis=1), v.max(axis=1)], axis=1)


def write_obj(path, tris, group="Mesh"):
    """m x 3 x 3 vertices as one OBJ group of m faces (%.17g: the parser reads back the same doubles)."""
    tris = np.asarray(tris, dtype=np.float64)
    with open(path, "w") as f:
        f.write("g %s\n" % group)
        np.savetxt(f, tris.reshape(-1, 3), fmt="v %.17g %.17g %.17g")
        np.savetxt(f, np.arange(1, 3 * len(tris) + 1).reshape(-1, 3), fmt="f %d %d %d")
    return path


def mesh_repeated(rng):
    """one triangle 300 times, then 200 distinct ones"""
    one = np.array([[[-1.0, 0.0, 0.5], [1.0, 0.0, 0.5], [0.0, 1.5, 0.25]]]).repeat(300, axis=0)
    return np.concatenate([one, tris_around(rng.uniform(-2.0, 2.0, (200, 3)), rng.uniform(0.05, 0.3, (200, 3)))])[rng.permutation(500)]


def mesh_flat_grid(cells=12, size=4.0):
    """an exactly flat grid at y = 0: two triangles per cell"""
    x = np.linspace(-size, size, cells + 1)
    i, j = np.meshgrid(np.arange(cells), np.arange(cells), indexing="ij")
    i, j = i.ravel(), j.ravel()
    p = lambda a, b: np.stack([x[a], np.zeros(len(a)), x[b]], axis=1)
    return np.concatenate([np.stack([p(i, j), p(i, j + 1), p(i + 1, j)], axis=1), np.stack([p(i + 1, j), p(i, j + 1), p(i + 1, j + 1)], axis=1)])


def mesh_chain(n):
    """family (h) as a mesh: chain_centroids with a large triangle on the two corners (and on every copy of the low one) so that a
    camera sees something, small ones along the chain"""
    cen = chain_centroids(n)
    half = np.full((n, 3), 2.0 ** -6)
    half[(cen == 0.0).all(axis=1) | (cen == 1.0).all(axis=1)] = 0.25
    return tris_around(cen, half)
