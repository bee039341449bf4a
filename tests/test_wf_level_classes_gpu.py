"""The wavefront path's two-ended queues on an MI355X (cases and reasoning: wf_level_classes.py): the synthetic analytic scene and its
cuts at 64x36 and at 67x35 (off the 8x8 tile), both pinned device paths, the plain and the counting kernels: frames, primary hits and
digests byte-equal between the paths, the ray counters those of the emulated kernels."""
import numpy as np
import pytest

import wf_level_classes as lc
import wf_shade_queues as q

pytestmark = pytest.mark.gpu
SIZES = {"64x36": (64, 36), "67x35": (67, 35)}


@pytest.fixture(scope="module")
def emu():
    from emu_lib import emu as _emu
    return _emu()


def _host_tensor(n):
    import torch
    return torch.empty(n, dtype=torch.float64)


def _device_tensor(n):
    import torch
    return torch.empty(n, dtype=torch.float64, device="cuda:0")


@pytest.mark.parametrize("size", sorted(SIZES))
@pytest.mark.parametrize("scene", sorted(lc.SCENES))
def test_level_classes(hip, emu, monkeypatch, scene, size):
    cam, world = lc.scene_camera(scene, SIZES[size])
    rgb, _, _ = q.both_paths(hip, world, cam, 5, monkeypatch)          # the plain kernels; the digests come from the counting ones
    for path in ("1", "4"):
        got, frame = lc.ray_counters(hip, world, cam, 5, path, monkeypatch, _device_tensor)
        want, _ = lc.ray_counters(emu, world, cam, 5, path, monkeypatch, _host_tensor)
        assert got == want, "path %s: ray counters %s, the emulator's %s" % (path, got, want)
        assert np.array_equal(frame.view(np.uint64), rgb.view(np.uint64)), "path %s: the counting kernels' frame differs" % path


@pytest.mark.parametrize("over", [False, True], ids=["exactly_at_cap", "one_over"])
def test_ends_meet(hip, monkeypatch, capfd, over):
    """The product's queues hold max(ceil(9 n / 8), 4096) items (rtc_scene.cpp wave_cap): 3 000 rays, 4 096 items.  The counts of every
    attempt of the launch are read from RTC_WF_DUMP_COUNTS: exactly at cap one attempt, both queues of level 1 full to the last item;
    one over, a first attempt whose ray queue's ends crossed and a second one in larger queues.  The frame is the one-kernel path's
    both times and no error state is left (check_ends_meet)."""
    n, cap = 3000, 4096
    g = cap - n + (1 if over else 0)
    monkeypatch.setenv("RTC_WF_DUMP_COUNTS", "1")
    capfd.readouterr()
    lc.check_ends_meet(hip, monkeypatch, n, cap, over)
    dumps = [l for l in capfd.readouterr().err.splitlines() if l.startswith("[rtc-wf]")]
    level1 = " 1: %d + %d / %d + %d;" % (2 * g, n - g, g, n)   # rays far + near / shade records far + near
    assert len(dumps) == (2 if over else 1), dumps
    assert all(" 1: %d + %d /" % (2 * g, n - g) in d for d in dumps), dumps   # (a crossed attempt traces, and so records, only what lies apart)
    assert level1 in dumps[-1], (level1, dumps)
    assert (g + n > cap) == over
