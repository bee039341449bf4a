"""The wavefront path's two-ended queues through the CPU emulation of the kernel source (cases and reasoning: wf_level_classes.py):
both device paths bit for bit -- pixels, hit records, digests -- and the oracle."""
import pytest

import wf_level_classes as lc


@pytest.fixture(scope="module")
def emu():
    from emu_lib import emu as _emu
    return _emu()


def _host_tensor(n):
    import torch
    return torch.empty(n, dtype=torch.float64)


@pytest.mark.parametrize("scene,camera,fuel,ask_oracle", lc.case_list(), ids=lambda v: str(v))
def test_level_classes_emulated(emu, orc, monkeypatch, scene, camera, fuel, ask_oracle):
    lc.check_case(emu, orc, monkeypatch, scene, camera, fuel, ask_oracle)


def test_the_cuts_empty_the_end_they_are_meant_to(emu, monkeypatch):
    """What the scene variants are for, read from the ray counters of the 64x36 frame at fuel 5 (and, small_parts, of the 7x5 frame at
    fuel 1, whose counters are level 1's two parts)."""
    st = {s: lc.ray_counters(emu, lc.scene_camera(s, "64x36")[1], lc.scene_camera(s, "64x36")[0], 5, "4", monkeypatch, _host_tensor)[0]
          for s in ("base", "no_glass", "glass_only", "planes_only")}
    assert st["base"]["rays_reflect"] > 64 and st["base"]["rays_refract"] > 64
    assert st["no_glass"]["rays_refract"] == 0 and st["no_glass"]["rays_container"] == 0 and st["no_glass"]["rays_reflect"] > 64
    assert st["glass_only"]["rays_refract"] > 64
    assert st["planes_only"]["rays_refract"] == 0 and st["planes_only"]["rays_reflect"] > 64
    cam, world = lc.scene_camera("small_parts", "7x5")
    small = lc.ray_counters(emu, world, cam, 1, "4", monkeypatch, _host_tensor)[0]
    assert 0 < small["rays_reflect"] < 64 and 0 < small["rays_refract"] < 64, small


def test_simt_emulation_of_the_two_ended_queues(orc, monkeypatch):
    """One thread per lane (64-lane blocks, real ballots and barriers): the far-end reservations of several blocks, 576 work ids."""
    import os
    import subprocess
    from emu_lib import EMU_DIR
    from raytracer_challenge_amd.backend import Backend
    subprocess.run(["make", "-s", "-C", EMU_DIR, "simt"], check=True)
    simt = Backend(os.path.join(EMU_DIR, "_build", "librtc_emu_simt.so"))
    for scene in ("base", "glass_only"):
        lc.check_case(simt, orc, monkeypatch, scene, "23x23", 5, True)


@pytest.mark.parametrize("over", [False, True], ids=["exactly_at_cap", "one_over"])
def test_ends_meet_emulated(emu, monkeypatch, over):
    """The emulator's queues hold max(ceil(9 n / 8), 256) items (tests/cpu_emu/emu_rtc.cpp): 200 rays, 256 items.  Exactly at cap the frame
    is the one-kernel path's; one over, the frame rendered again in larger queues is."""
    lc.check_ends_meet(emu, monkeypatch, 200, 256, over)
