"""Light-grid cells built from primitive silhouettes, on an MI355X: with the tight lists (default) and with the rectangle lists
(RTC_LIGHT_GRID_TIGHT=0) and without grids both device paths must give the same pixels and hit records bit for bit, and the oracle's."""
import numpy as np
import pytest

from parity import assert_parity
from raytracer_challenge_amd import scenes
from light_grid_cases import both_ways, lights_inside_scene


@pytest.mark.gpu
def test_hip_tight_lists_are_results_neutral_on_the_benchmark_scene(hip, orc, monkeypatch):
    cam, world = scenes.synthetic_analytic(n_primitives=512, seed=12345, hsize=480, vsize=270)
    both_ways(hip, world, cam, 5, monkeypatch)
    assert_parity(hip, orc, world, cam, 5, np.arange(0, 480 * 270, 7, dtype=np.uint64), label="config-2 scene at 480x270, tight light grids")


@pytest.mark.gpu
def test_hip_five_lights(hip, orc, monkeypatch):
    """More than four lights: 128 cells per face edge."""
    from raytracer_challenge_amd.scene import Color, PointLight, Vector
    cam, world = scenes.synthetic_analytic(n_primitives=96, seed=7, hsize=96, vsize=54)
    for at in ((0.0, 60.0, 0.0), (40.0, 8.0, -30.0), (-25.0, 30.0, 45.0)):
        world.lights.append(PointLight(Color.new(0.3, 0.3, 0.3), Vector.point(*at)))
    assert len(world.lights) == 5
    both_ways(hip, world, cam, 3, monkeypatch)
    assert_parity(hip, orc, world, cam, 3, label="five lights, tight light grids")


@pytest.mark.gpu
def test_hip_light_inside_the_cloud(hip, orc, monkeypatch):
    cam, world = lights_inside_scene()
    both_ways(hip, world, cam, 2, monkeypatch)
    assert_parity(hip, orc, world, cam, 2, label="lights inside bounds / on a surface, tight light grids")
