"""The culling predicates of the ray kernels (csrc/rtc_device.hpp: make_frame / t_interval32 / slab32c, make_frame_point / point_in_box,
group_box_hit, plane_behind, light_is_behind), each alone, against exact arithmetic (tests/cull_cases.py), through the CPU emulator's
rtc_cull_probe_raw: the kernel source itself in a host loop.  A predicate may only skip what the exact test would have rejected; a
scene shows a wrong skip only when one of its rays happens to meet it, these records are aimed at the places where one can occur."""
import numpy as np
import pytest

import cull_cases as cc


@pytest.fixture(scope="module")
def probe():
    from emu_lib import emu
    be = emu()
    return lambda kind, rec: be.cull_probe(kind, rec)


def check_slab_soundness(probe, family):
    rec, fam, exact, _ = cc.slab_cases()
    sel = fam == family
    rec, exact = rec[sel], exact[sel]
    big, maybe_big = cc.slab_big_frames(rec)
    got = probe(cc.SLAB, rec)
    must = exact & ~maybe_big
    assert must.sum() >= 1000, family
    bad = must & ~got
    assert not bad.any(), "%s: %d of %d boxes that the exact ray enters are rejected, e.g. %r" % (family, bad.sum(), must.sum(), rec[bad][0].tolist())
    assert got[big].all(), "%s: a frame with |of| + R >= 1e30 rejects a box" % family


def check_slab_usefulness(probe):
    rec, fam, _, miss = cc.slab_cases()
    assert miss.sum() >= 2000
    got = probe(cc.SLAB, rec[miss])
    assert not got.any(), "%d of %d boxes that the ray misses by more than 16 eps are taken, e.g. %r" % (got.sum(), miss.sum(), rec[miss][got][0].tolist())


def check_slab_unbounded(probe, label):
    rec, lab = cc.slab_unbounded_cases()
    rec = rec[lab == label]
    assert len(rec) >= 1000
    got = probe(cc.SLAB, rec)
    assert got.all(), "%s: %d of %d records reject their box, e.g. %r" % (label, (~got).sum(), len(rec), rec[~got][0].tolist())


def check_point(probe):
    rec, exact = cc.point_cases()
    assert len(rec) >= 20000 and 4000 < exact.sum() < 16000
    got = probe(cc.POINT, rec)
    bad = exact & ~got
    assert not bad.any(), "%d of %d hit points inside their box are called outside, e.g. %r" % (bad.sum(), exact.sum(), rec[bad][0].tolist())
    odd = cc.point_unbounded_cases()
    got = probe(cc.POINT, odd)
    assert got.all(), "%d of %d NaN, infinite or over-large points are called outside, e.g. %r" % ((~got).sum(), len(odd), odd[~got][0].tolist())


def check_gate(probe):
    rec, want = cc.gate_cases()
    assert len(rec) >= 108000 and 20000 < want.sum() < 100000
    got = probe(cc.GATE, rec)
    bad = got != want
    assert not bad.any(), "%d of %d gates differ from BoundingBox::intersects, e.g. %r (want %r)" % (bad.sum(), len(rec), rec[bad][0].tolist(), bool(want[bad][0]))


def check_plane(probe):
    rec, q = cc.plane_cases()
    assert len(rec) >= 20000
    got = probe(cc.PLANE, rec)
    oy, dy, mode = rec[:, 0], rec[:, 1], rec[:, 2]
    assert got.sum() >= 1000
    bad = got & ~(q < 0.0)   # -0.0 < 0.0 is false, and so is NaN < 0.0: a skipped plane's t is a negative number that fails `t >= 0`
    assert not bad.any(), "%d skipped planes whose -oy / dy is not negative, e.g. %r -> %r" % (bad.sum(), rec[bad][0].tolist(), q[bad][0])
    assert not got[mode == 3].any(), "a container pass skips a plane"
    # ordinary operands: both finite, |oy| at least 1e-289, |dy| from EPSILON (below it the reference reports no intersection and the
    # kernels never ask) to 1e16: a decade inside each of the predicate's own limits
    with np.errstate(invalid="ignore"):
        must = (q <= -1e-280) & (mode != 3) & np.isfinite(oy) & np.isfinite(dy) & (np.abs(oy) >= 1e-289) & (np.abs(dy) >= cc.EPSILON) & (np.abs(dy) <= 1e16)
    assert must.sum() >= 1000
    assert got[must].all(), "%d of %d planes behind the origin are not skipped, e.g. %r" % ((~got[must]).sum(), must.sum(), rec[must][~got[must]][0].tolist())


def check_behind(probe):
    rec, dot, mag = cc.behind_cases()
    assert len(rec) >= 20000
    got = probe(cc.BEHIND, rec)
    assert got.sum() >= 2000
    bad = got & ~(dot < 0.0)
    assert not bad.any(), "%d skipped shadow rays whose light . normal is not below 0, e.g. %r -> %r" % (bad.sum(), rec[bad][0].tolist(), dot[bad][0])
    nan = np.isnan(rec).any(axis=1)
    assert nan.sum() >= 500 and not got[nan].any(), "a NaN operand skips a shadow ray"
    with np.errstate(invalid="ignore"):
        must = (dot < -1e-3) & np.isfinite(rec).all(axis=1) & (mag < 1e25)
    assert must.sum() >= 2000
    assert got[must].all(), "%d of %d lights well behind the surface are not skipped, e.g. %r" % ((~got[must]).sum(), must.sum(), rec[must][~got[must]][0].tolist())


@pytest.mark.parametrize("family", list(cc.SLAB_FAMILIES))
def test_the_slab_test_takes_every_box_the_exact_ray_enters(probe, family):
    check_slab_soundness(probe, family)


def test_the_slab_test_rejects_boxes_missed_by_16_eps(probe):
    check_slab_usefulness(probe)


@pytest.mark.parametrize("label", ["big_frame", "nan_origin", "nan_dir", "inf_dir"])
def test_unbounded_rays_and_frames_take_every_box(probe, label):
    check_slab_unbounded(probe, label)


def test_a_hit_point_inside_the_box_is_called_inside(probe):
    check_point(probe)


def test_the_gate_equals_the_references_box_test(probe):
    check_gate(probe)


def test_a_skipped_plane_lies_behind_the_origin(probe):
    check_plane(probe)


def test_a_skipped_light_is_behind_the_surface(probe):
    check_behind(probe)


def test_the_records_hold_what_their_families_promise():
    """The generators themselves: every family is there in numbers, both answers occur, and the families that reach past the f32 range
    do reach past it."""
    rec, fam, exact, miss = cc.slab_cases()
    assert len(rec) >= 20000
    for name in cc.SLAB_FAMILIES:
        assert 1000 <= exact[fam == name].sum() <= 0.9 * (fam == name).sum(), name
    far = rec[fam == "parallel_far"]
    assert (far[:, 3] > 3.4e8).all() and ((far[:, 7:10] == 0.0).sum(axis=1) >= 1).mean() > 0.5
    comp = rec[fam == "components"][:, 7:10]
    for v in cc.SPECIAL_COMPONENTS:
        assert ((comp == v) & (np.signbit(comp) == np.signbit(v))).any(), v
    tiny = rec[fam == "tiny_dir"]
    big = np.abs(tiny[:, 7:10]).max(axis=1)
    assert (big <= 1e-22).all() and (big >= 1e-30).all() and (big < 1 / 2.3e22).sum() > 2000
    assert ((np.abs(tiny[:, 4:7]).max(axis=1) + tiny[:, 3]) * 1e30 < 1e37).all()   # no scaled origin overflows: only the direction's size sets these frames apart
    iv = rec[fam == "intervals"]
    assert (iv[:, 10] == -np.inf).sum() > 1000 and (iv[:, 11] < iv[:, 10]).sum() > 1000 and ((iv[:, 10] == 0.0) & np.isfinite(iv[:, 11])).sum() > 1000
    assert cc.slab_exact(np.array([0, 0, 0, 1.0, 0.5, 0.5, -5, 0.0, -0.0, 1, 0, np.inf, 0, 0, 0, 1, 1, 1]))
    assert not cc.slab_exact(np.array([0, 0, 0, 1.0, 1.5, 0.5, -5, 0.0, -0.0, 1, 0, np.inf, 0, 0, 0, 1, 1, 1]))
    assert not cc.slab_exact(np.array([0, 0, 0, 1.0, 0.5, 0.5, -5, 0.0, 0.0, 1, 0, 4.5, 0, 0, 0, 1, 1, 1]))
    assert cc.slab_exact(np.array([0, 0, 0, 1.0, 0.5, 0.5, 5, 0.0, 0.0, 1, -np.inf, 0.0, 0, 0, 0, 1, 1, 1]))
