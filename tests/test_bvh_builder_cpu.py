"""The accelerator's binary tree checked structurally, the parts that need no GPU: the checker and ref_store (tests/bvh_ref.py) pinned bit
for bit against the host builder through the library's builder hook (include/rtc.h rtc_bvh_build_raw, where = 0), the restatement of the
device's linear BVH held to the same invariants, the deep-chain input shown to outgrow the traversal stack, and the checker shown to
reject corrupted trees.  test_bvh_builder_gpu.py runs the device builder against all of it."""
import os

import numpy as np
import pytest

import bvh_cases
import bvh_ref
from bvh_cases import RTC_BVH_STACK, boxes_of, build_raw, case_id, collapse_raw, reference
from raytracer_challenge_amd.backend import Backend

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIB = os.path.join(ROOT, "raytracer_challenge_amd", "csrc", "librtc_amd.so")
CASES = bvh_cases.cases(4099)


@pytest.fixture(scope="module")
def lib():
    """librtc_amd.so without a device: loading it and the host-only entry points need none."""
    return Backend(LIB).lib


# ---- ref_store's rounding rule, on values whose answer is known -----------------------------------------------------------------------
def test_ref_store_rounds_outward_by_at_most_one_ulp():
    rng = np.random.RandomState(5)
    box = np.concatenate([rng.uniform(-1e3, 0.0, (4096, 3)), rng.uniform(0.0, 1e3, (4096, 3))], axis=1)
    box[:64] = np.round(box[:64])                       # values a float holds exactly: only the pad moves them
    center = np.array([0.25, -3.0, 17.0])
    lo, hi = bvh_ref.ref_store(box, center)
    assert lo.dtype == np.float32 and hi.dtype == np.float32
    ext = (box[:, 3:6] - box[:, 0:3]).max(axis=1)[:, None]
    vlo = (box[:, 0:3] - (1e-9 * (np.abs(box[:, 0:3]) + ext) + 1e-30)) - center
    vhi = (box[:, 3:6] + (1e-9 * (np.abs(box[:, 3:6]) + ext) + 1e-30)) - center
    assert (lo.astype(np.float64) <= vlo).all() and (hi.astype(np.float64) >= vhi).all()               # never inward
    assert (np.nextafter(lo, np.float32(np.inf)).astype(np.float64) > vlo).all()                         # and the nearest such float
    assert (np.nextafter(hi, np.float32(-np.inf)).astype(np.float64) < vhi).all()


# ---- the host builder through the hook: pins check_tree and ref_store bit for bit ------------------------------------------------------
@pytest.mark.parametrize("case", CASES, ids=case_id)
def test_host_tree_passes_the_checker(lib, case):
    family, n, leaf_max, base = case
    boxes = boxes_of(family, n)
    t = build_raw(lib, boxes, leaf_max, base, 0)
    assert t.rc == 0, lib.rtc_last_error()
    leaves = bvh_ref.check_tree(t.nodes, t.root, t.order, boxes, base, leaf_max, t.frame)
    assert leaves >= (n + leaf_max - 1) // leaf_max
    rc, depth, need = collapse_raw(lib, t.nodes, t.root)         # the collapse-only call agrees with the build call's figures
    assert (rc, depth, need) == (0, t.depth, t.stack_need)


@pytest.mark.parametrize("leaf_max,used", [(0, 1), (9, 8), (16, 8), (-3, 1)])
def test_host_builder_clamps_leaf_max(lib, leaf_max, used):
    boxes = boxes_of("a_uniform", 513)
    t = build_raw(lib, boxes, leaf_max, 0, 0)
    assert t.rc == 0
    bvh_ref.check_tree(t.nodes, t.root, t.order, boxes, 0, used, t.frame)
    same = build_raw(lib, boxes, used, 0, 0)
    assert np.array_equal(t.nodes.view(np.uint8), same.nodes.view(np.uint8)) and np.array_equal(t.order, same.order)


def test_hook_reports_errors_instead_of_crashing(lib):
    boxes = boxes_of("a_uniform", 257)
    full = build_raw(lib, boxes, 4, 0, 0)
    assert full.rc == 0 and 0 < full.n_nodes <= 257
    short = build_raw(lib, boxes, 4, 0, 0, nodes_cap=full.n_nodes - 1)
    assert short.rc == 1 and short.untouched and short.n_nodes == full.n_nodes and b"capacity" in lib.rtc_last_error()
    short = build_raw(lib, boxes, 4, 0, 0, order_cap=256)
    assert short.rc == 1 and short.untouched
    exact = build_raw(lib, boxes, 4, 0, 0, nodes_cap=full.n_nodes)
    assert exact.rc == 0 and np.array_equal(exact.nodes.view(np.uint8), full.nodes.view(np.uint8))
    assert build_raw(lib, boxes, 4, 0, 2).rc == 1                      # no such builder
    assert build_raw(lib, boxes[:0], 4, 0, 0).rc == 1                  # no items
    null = lib.rtc_bvh_build_raw(None, 5, 4, 0, 0, None, 0, None, None, 0, None, 0, None, None, None, None)
    assert null == 1
    # the collapse-only call refuses an array it cannot walk
    bad = full.nodes.copy()
    inner = int(np.flatnonzero(bad["c0"] >= 0)[0])
    bad["c0"][inner] = len(bad)                                        # a reference outside the array
    assert collapse_raw(lib, bad, full.root)[0] == 1
    bad = full.nodes.copy()
    bad["c0"][inner] = full.root                                       # a cycle
    assert collapse_raw(lib, bad, full.root)[0] == 1
    assert collapse_raw(lib, full.nodes, len(full.nodes))[0] == 1      # a root outside the array
    assert lib.rtc_bvh_collapse_raw(None, 0, 0, None, None) == 1


# ---- the restatement of the device's tree satisfies the same invariants ----------------------------------------------------------------
@pytest.mark.parametrize("case", CASES, ids=case_id)
def test_reference_lbvh_passes_the_checker(case):
    family, n, leaf_max, base = case
    boxes = boxes_of(family, n)
    ref = reference(*case)
    if n <= leaf_max:
        assert ref is None
        return
    nodes, order, keys, frame = ref
    bvh_ref.check_tree(nodes, 0, order, boxes, base, leaf_max, frame)
    assert (np.diff(keys.astype(np.int64)) >= 0).all() and int(keys.max()) < 2 ** 63
    assert np.array_equal(keys, bvh_ref.ref_keys(boxes)[order])
    eq = np.flatnonzero(np.diff(keys.astype(np.int64)) == 0)
    assert (order[eq] < order[eq + 1]).all(), "the sort is stable: equal keys keep the items' order"


def test_families_stress_what_they_claim():
    """The special cases of bvh_device.hip the families exist for are really taken."""
    bits = lambda f, n=4099: bvh_ref.extent_bisection(np.ptp(0.5 * (boxes_of(f, n)[:, 0:3] + boxes_of(f, n)[:, 3:6]), axis=0))[0]
    assert len(set(reference("b_one_centroid", 4099, 4, 0)[2].tolist())) == 1                            # every key equal
    keys_c = reference("c_runs", 4099, 4, 0)[2]
    runs = np.diff(np.flatnonzero(np.concatenate([[True], np.diff(keys_c.astype(np.int64)) != 0, [True]])))
    ends = np.cumsum(runs)
    crossed = sum(1 for s, e in zip(ends - runs, ends) if (e - 1) // 256 > s // 256)
    assert len(runs) == 37 and crossed >= 12, (runs, crossed)                                             # runs of equal keys across block boundaries
    assert np.ptp(boxes_of("d_flat", 4099)[:, [1, 4]]) == 0.0 and np.ptp(boxes_of("e_line", 4099)[:, [1, 2, 4, 5]]) == 0.0
    assert bits("d_flat") == [30, 3, 30] and bits("e_line") == [30, 30, 3]                                # an axis with scale 0
    assert bits("f_long_x") == [30, 17, 16]                                                               # the bits >= 30 branch
    assert bits("h_chain") == [bvh_cases.H_BITS] * 3
    keys_h = [int(k) for k in reference("h_chain", 4099, 4, 0)[2]]
    tops = [k.bit_length() for k in keys_h if k]
    assert len(tops) == bvh_cases.H_CHAIN - 1 and len(set(tops[:-1])) == len(tops) - 1, "family (h): pairwise distinct highest set bits"
    assert keys_h.count(0) == 4099 - bvh_cases.H_CHAIN + 1


def test_deep_chain_outgrows_the_traversal_stack(lib):
    """Family (h) at H_DEEP items: the device's tree for it needs more traversal stack than a lane has, which is what sends build_tree to
    its second attempt (test_bvh_builder_gpu.py renders that).  The chain alone (no copies) stays just inside: the copies' subtree is
    what tips it, so the copy count matters and is pinned here."""
    def need(n):
        nodes, order, keys, frame = reference("h_chain", n, 4, 0)
        rc, depth, stack_need = collapse_raw(lib, nodes, 0)
        assert rc == 0
        return stack_need
    figures = {n: need(n) for n in (bvh_cases.H_CHAIN, 257, 513, bvh_cases.H_DEEP)}
    print("family (h): stack_need by item count", figures)
    assert figures[bvh_cases.H_DEEP] > RTC_BVH_STACK - 1, figures
    # the host builder's tree of the same input fits: the fallback exists
    host = build_raw(lib, boxes_of("h_chain", bvh_cases.H_DEEP), 4, 0, 0)
    assert host.rc == 0 and 0 < host.stack_need <= RTC_BVH_STACK - 1


# ---- the checker can fail --------------------------------------------------------------------------------------------------------------
def _ulp(x, up):
    return np.nextafter(np.float32(x), np.float32(np.inf if up else -np.inf))


def _corrupt(kind, nodes, order, boxes, base):
    nodes, order = nodes.copy(), order.copy()
    leaf_nodes = np.flatnonzero(nodes["c0"] < 0)
    k = int(leaf_nodes[len(leaf_nodes) // 2])
    if kind == "shrunk":            # one box one f32 ulp too small
        nodes["hi1"][k, 2] = _ulp(nodes["hi1"][k, 2], up=False)
    elif kind == "grown":           # one box one ulp too large
        nodes["lo0"][k, 0] = _ulp(nodes["lo0"][k, 0], up=False)
    elif kind == "overlap":         # a leaf range that starts one item early: it overlaps the one before
        first, count = bvh_ref.decode_leaf(nodes["c0"][k])
        assert first > base
        nodes["c0"][k] = bvh_ref.leaf_ref(first - 1, count)
    elif kind == "missing":         # a leaf range one item short: an item is in no leaf
        first, count = max((bvh_ref.decode_leaf(c) for c in nodes["c0"][leaf_nodes]), key=lambda t: t[1])
        assert count >= 2
        j = int(np.flatnonzero(nodes["c0"] == bvh_ref.leaf_ref(first, count))[0])
        nodes["c0"][j] = bvh_ref.leaf_ref(first, count - 1)
    elif kind == "count":           # a leaf of more items than leaf_max (the last item of the tree grows a leaf past the end as well)
        first, count = bvh_ref.decode_leaf(nodes["c0"][k])
        nodes["c0"][k] = bvh_ref.leaf_ref(first, 5)
    elif kind == "not a permutation":
        order[0] = order[1]
    elif kind == "orphan":          # a child reference replaced by a leaf: the subtree below is unreachable
        j = int(np.flatnonzero(nodes["c1"] >= 0)[0])
        nodes["c1"][j] = nodes["c0"][k]
    elif kind == "cycle":
        j = int(np.flatnonzero(nodes["c1"] >= 0)[-1])
        nodes["c1"][j] = 0
    elif kind == "swapped items":   # two items of different leaves exchanged in `order`: every range intact, two boxes wrong
        order[[0, len(order) - 1]] = order[[len(order) - 1, 0]]
    return nodes, order


@pytest.mark.parametrize("builder", ["host", "reference"])
@pytest.mark.parametrize("kind,message", [("shrunk", "too small"), ("grown", "too large"), ("overlap", "overlap"), ("missing", "gap|missing"), ("count", "leaf_max"),
                                          ("not a permutation", "permutation"), ("orphan", "not reachable"), ("cycle", "reached twice"),
                                          ("swapped items", "child boxes")])
def test_checker_rejects_corrupted_trees(lib, builder, kind, message):
    boxes, base = boxes_of("a_uniform", 513), 12345
    if builder == "host":
        t = build_raw(lib, boxes, 4, base, 0)
        nodes, root, order, frame = t.nodes, t.root, t.order, t.frame
    else:
        nodes, order, _, frame = reference("a_uniform", 513, 4, base)
        root = 0
    bvh_ref.check_tree(nodes, root, order, boxes, base, 4, frame)          # sound before the corruption
    bad_nodes, bad_order = _corrupt(kind, nodes, order, boxes, base)
    with pytest.raises(bvh_ref.TreeError, match=message):
        bvh_ref.check_tree(bad_nodes, root, bad_order, boxes, base, 4, frame)
    with pytest.raises(bvh_ref.TreeError, match="frame"):
        bvh_ref.check_tree(nodes, root, order, boxes, base, 4, np.nextafter(np.asarray(frame), np.inf))
