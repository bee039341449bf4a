"""What a wrong box rejection looks like from a scene (the predicates themselves: test_cull_predicates_*.py).  Two worlds without a
plane, so that a ray meets what it meets through the analytic BVH alone:
huge_world(S) -- at S = 1e9 and 1e12 the scaled origin of an axis-parallel ray overflows f32 in the BVH's frame (make_frame), and a
frame built from it rejected every box: the ray of the report went through the sphere in front of it unseen.  S = 1e3 and 1e8 are the controls.
bvh_only_world() -- rays with one NaN or infinite direction component: the reference pushes a NaN t per sphere and panics in its sort,
whatever the two finite axes do; a slab test that goes on culling with those two axes returns an ordinary miss instead."""
import numpy as np
import pytest

import cases
from parity import assert_parity, assert_ray_parity, assert_ray_parity_with_panics

SIZES = [1e3, 1e8, 1e9, 1e12]


@pytest.fixture(scope="module")
def emu():
    from emu_lib import emu as _emu
    return _emu()


def check_huge(be, orc, S, label):
    world, rays = cases.huge_world(S), cases.huge_world_rays(S)
    assert rays.shape[0] >= 300
    assert_ray_parity(be, orc, world, rays, 3, label="%s: huge_world(%g)" % (label, S))
    _, hits = be.color_at(be.build_world(world), rays[:1], 0)   # the ray of the report enters the first small sphere 1e-3 S off its axis
    assert hits["prim"][0] == 0 and abs(hits["t"][0] / S - 0.480025) < 1e-6, hits
    assert_parity(be, orc, world, cases.huge_world_camera(S), 3, label="%s: huge_world(%g), 9 x 9 down -z" % (label, S))


def check_bvh_only(be, orc, label):
    world, rays = cases.bvh_only_world(), cases.bvh_only_rays()
    _, n_panics = assert_ray_parity_with_panics(be, orc, world, rays, 3, label=label + ": bvh_only_world", max_panics=len(rays))
    assert n_panics >= 30, n_panics   # (the oracle refuses the rays with a NaN or infinite component: the test is about them)


@pytest.mark.parametrize("path", ["1", "4"])
@pytest.mark.parametrize("S", SIZES)
def test_huge_world_in_the_emulator(emu, orc, monkeypatch, S, path):
    monkeypatch.setenv("RTC_KERNEL", path)
    check_huge(emu, orc, S, "emulator, path " + path)


@pytest.mark.parametrize("path", ["1", "4"])
def test_non_finite_directions_in_the_emulator(emu, orc, monkeypatch, path):
    monkeypatch.setenv("RTC_KERNEL", path)
    check_bvh_only(emu, orc, "emulator, path " + path)


@pytest.mark.gpu
@pytest.mark.parametrize("path", ["1", "4"])
@pytest.mark.parametrize("S", SIZES)
def test_hip_huge_world(hip, orc, monkeypatch, S, path):
    monkeypatch.setenv("RTC_KERNEL", path)
    check_huge(hip, orc, S, "path " + path)


@pytest.mark.gpu
@pytest.mark.parametrize("path", ["1", "4"])
def test_hip_non_finite_directions(hip, orc, monkeypatch, path):
    monkeypatch.setenv("RTC_KERNEL", path)
    check_bvh_only(hip, orc, "path " + path)
