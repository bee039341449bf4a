"""wf_ts's own memory round trips -- chunk cursor, container-pass decision, the shade record's indices -- through the CPU emulation of
the kernel source (tests/cpu_emu): cases and reasoning in wf_ts_round_trips.py.  The emulator holds no LDS-resident build and no
area-light entry point; test_wf_ts_round_trips_gpu.py covers those."""
import os
import subprocess

import numpy as np
import pytest

import wf_ts_round_trips as rt


@pytest.fixture(scope="module")
def emu():
    from emu_lib import emu as _emu
    return _emu()


@pytest.fixture(scope="module")
def simt():
    """One thread per lane, 64-lane waves: lane 0 fetches the cursor and the wave's lanes exchange it."""
    from emu_lib import EMU_DIR
    from raytracer_challenge_amd.backend import Backend
    subprocess.run(["make", "-s", "-C", EMU_DIR, "simt"], check=True)
    return Backend(os.path.join(EMU_DIR, "_build", "librtc_emu_simt.so"))


def _host_buffer(n):
    import torch
    return torch.zeros(n, dtype=torch.float64)


@pytest.mark.parametrize("frame", rt.CURSOR_FRAMES, ids=lambda f: "%dx%d" % f)
def test_cursor_chunk_counts(emu, simt, orc, monkeypatch, frame):
    """1, 7, 8 and 9 chunks of level 0, in the one-lane geometry (every lane its own wave: 64 cursor fetches per chunk's worth of
    work) and in 64-lane waves."""
    cam, world = rt.glass_and_mirror(*frame)
    one_lane = rt.check(emu, orc, monkeypatch, cam, world, 5, "cursor %dx%d" % frame)
    waves = rt.check(simt, orc, monkeypatch, cam, world, 5, "cursor %dx%d, 64-lane waves" % frame, ask_oracle=False)
    assert np.array_equal(one_lane[0].view(np.uint64), waves[0].view(np.uint64)) and one_lane[1].tobytes() == waves[1].tobytes()
    assert np.array_equal(one_lane[2], waves[2])


@pytest.mark.parametrize("frame", ((8, 8), (72, 8)), ids=lambda f: "%dx%d" % f)
def test_cursor_empty_world(emu, orc, monkeypatch, frame):
    cam, world = rt.empty_world(*frame)
    rgb, hits, _ = rt.check(emu, orc, monkeypatch, cam, world, 5, "empty world %dx%d" % frame)
    assert (hits["prim"] == -1).all() and not rgb.any()


@pytest.mark.parametrize("fuel", (0, rt.MAX_FUEL))
def test_cursor_fuel_limits(emu, orc, monkeypatch, fuel):
    cam, world = rt.glass_and_mirror(8, 8)
    rt.check(emu, orc, monkeypatch, cam, world, fuel, "8x8 fuel %d" % fuel)


def test_cursor_trace_and_shadow_chunks_share_launches(emu, orc, monkeypatch):
    cam, world = rt.glass_and_mirror(48, 32)
    rt.check(emu, orc, monkeypatch, cam, world, 5, "glass and mirror 48x32")


def test_cursor_three_frames_back_to_back(emu, monkeypatch):
    cam, world = rt.glass_and_mirror(48, 32)
    rt.three_frames_back_to_back(emu, world, cam, 5, monkeypatch, _host_buffer, _cpu_standin=True)


@pytest.mark.parametrize("fuel", (5, 1))
@pytest.mark.parametrize("switch", sorted(rt.SWITCHES))
@pytest.mark.parametrize("scene", sorted(rt.TRANSPARENCY_SCENES))
def test_transparent_hits(emu, orc, monkeypatch, scene, switch, fuel):
    cam, world = rt.TRANSPARENCY_SCENES[scene]()
    rt.set_switch(monkeypatch, switch)
    rt.check(emu, orc, monkeypatch, cam, world, fuel, "%s %s fuel %d" % (scene, switch, fuel))


@pytest.mark.parametrize("fuel", (5, 1))
def test_transparent_mesh_triangles(emu, orc, monkeypatch, fuel):
    cam, world = rt.glass_teapot()
    rt.check(emu, orc, monkeypatch, cam, world, fuel, "glass teapot fuel %d" % fuel)


@pytest.mark.parametrize("fuel", (5, 1))
def test_transparent_csg_child(emu, orc, monkeypatch, fuel):
    cam, world = rt.csg_with_glass()
    rt.check(emu, orc, monkeypatch, cam, world, fuel, "csg fuel %d" % fuel)


def test_negative_zero_transparency_makes_no_container_pass(emu, orc, monkeypatch):
    cam, world = rt.glass_solids(transparency=-0.0)
    rt.check(emu, orc, monkeypatch, cam, world, 5, "transparency -0.0")
    assert rt.container_rays(emu, world, cam, 5, monkeypatch, _host_buffer, _cpu_standin=True) == {"1": 0, "4": 0}


def test_nan_transparency_is_transparent_on_both_paths(emu, orc, monkeypatch):
    cam, world = rt.glass_solids(transparency=float("nan"))
    rt.check(emu, orc, monkeypatch, cam, world, 5, "transparency NaN", ask_oracle=False)
    n = rt.container_rays(emu, world, cam, 5, monkeypatch, _host_buffer, _cpu_standin=True)
    assert n["1"] == n["4"] > 0


@pytest.mark.parametrize("fuel", (0, 5))
@pytest.mark.parametrize("scene", sorted(rt.PHONG_SCENES))
def test_phong_phase(emu, orc, monkeypatch, scene, fuel):
    """Fuel 0: level 0's records only (their eye vector is the camera ray's); fuel 5: records of the levels below, read from the queue."""
    rt.check_phong(emu, orc, monkeypatch, scene, fuel)
