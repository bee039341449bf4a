"""The records of test_cull_predicates_cpu.py through the device's probe kernel (csrc/rtc_probe.hip): the same functions as compiled for
gfx950 -- the hardware's V_RCP_F64 in the group gate, the compiler's f32 division and denormal mode in the slab test -- held to the same
exact references.  Each test also prints how many records the device and the CPU emulator answer differently (DESIGN.md records the
counts); only the properties are asserted."""
import numpy as np
import pytest

import cull_cases as cc
import test_cull_predicates_cpu as props

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def probe(hip):
    from cases import bvh_only_world
    nw = hip.build_world(bvh_only_world())   # (any scene: it names the device and the stream)
    return lambda kind, rec: hip.cull_probe(kind, rec, nw)


@pytest.fixture(scope="module")
def emu_probe():
    from emu_lib import emu
    be = emu()
    return lambda kind, rec: be.cull_probe(kind, rec)


def report(family, kind, rec, probe, emu_probe):
    differ = int((probe(kind, rec) != emu_probe(kind, rec)).sum())
    print("cull probe, %s: device and emulator differ on %d of %d records" % (family, differ, len(rec)))


@pytest.mark.parametrize("family", list(cc.SLAB_FAMILIES))
def test_hip_slab_takes_every_box_the_exact_ray_enters(probe, family):
    props.check_slab_soundness(probe, family)


def test_hip_slab_rejects_boxes_missed_by_16_eps(probe, emu_probe):
    props.check_slab_usefulness(probe)
    report("slab", cc.SLAB, cc.slab_cases()[0], probe, emu_probe)


@pytest.mark.parametrize("label", ["big_frame", "nan_origin", "nan_dir", "inf_dir"])
def test_hip_unbounded_rays_and_frames_take_every_box(probe, label):
    props.check_slab_unbounded(probe, label)


def test_hip_hit_point_inside_the_box_is_called_inside(probe, emu_probe):
    props.check_point(probe)
    report("slab, unbounded", cc.SLAB, cc.slab_unbounded_cases()[0], probe, emu_probe)
    report("point", cc.POINT, np.concatenate([cc.point_cases()[0], cc.point_unbounded_cases()]), probe, emu_probe)


def test_hip_gate_equals_the_references_box_test(probe, emu_probe):
    props.check_gate(probe)
    report("gate", cc.GATE, cc.gate_cases()[0], probe, emu_probe)


def test_hip_skipped_plane_lies_behind_the_origin(probe, emu_probe):
    props.check_plane(probe)
    report("plane", cc.PLANE, cc.plane_cases()[0], probe, emu_probe)


def test_hip_skipped_light_is_behind_the_surface(probe, emu_probe):
    props.check_behind(probe)
    report("behind", cc.BEHIND, cc.behind_cases()[0], probe, emu_probe)


def test_hip_probe_refuses_what_it_cannot_run(hip):
    from cases import bvh_only_world
    lib = hip.lib
    nw = hip.build_world(bvh_only_world())
    assert hip.cull_probe(cc.PLANE, np.zeros((0, 3)), nw).shape == (0,)
    rec, out = np.zeros((1, 3)), np.zeros(1, dtype=np.uint8)   # (cull_probe above has set the entry's argument types)
    assert lib.rtc_cull_probe_raw(None, 7, rec.ctypes.data, 1, out.ctypes.data) == 1 and b"no such predicate" in lib.rtc_last_error()
    with pytest.raises(Exception, match="NULL"):   # a device is needed: no scene, no answer
        hip.cull_probe(cc.PLANE, np.zeros((1, 3)))
    # more records than one grid-stride pass covers (8192 blocks of 256), and a count that is no multiple of the block
    rec, q = cc.plane_cases()
    many = np.tile(rec, (53, 1))[:8192 * 256 + 77]
    got = hip.cull_probe(cc.PLANE, many, nw)
    assert np.array_equal(got, np.tile(hip.cull_probe(cc.PLANE, rec, nw), 53)[:len(many)])
