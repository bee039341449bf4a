"""Area lights (include/rtc.h rtc_light_ex), the parts that need no GPU: the Python API, the numpy restatement of the sample
positions and of the jitter hash that the GPU tests (test_area_lights_gpu.py) compare the device against, the exports of
librtc_amd.so, the refusal of the CPU oracle (the reference has no area lights), the emulator library, and the Rust mirror of the
record."""
import ctypes as C
import os
import struct

import numpy as np
import pytest

from raytracer_challenge_amd.cabi import RtcSceneDesc, load
from raytracer_challenge_amd.backend import RtwError
from raytracer_challenge_amd.scene import AreaLight, Color, Element, PointLight, ShapeArgs, Vector, World
from test_shim_layout import c_struct, rust_struct

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIB = os.path.join(ROOT, "raytracer_challenge_amd", "csrc", "librtc_amd.so")
M64 = (1 << 64) - 1


# ---- the numpy restatement of include/rtc.h rtc_light_ex (shared with test_area_lights_gpu.py) ------------------------------------
def splitmix64(z: int) -> int:
    """SplitMix64's finaliser (csrc/device_scene.h rtc_splitmix64)."""
    z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & M64
    z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & M64
    return z ^ (z >> 31)


def f64_bits(x: float) -> int:
    return struct.unpack("<Q", struct.pack("<d", float(x)))[0]


def area_hash(light_index: int, x: float, y: float, z: float) -> int:
    """h = m(m(m(m(light) ^ bits(x)) ^ bits(y)) ^ bits(z)) over the shading point's over_point."""
    return splitmix64(splitmix64(splitmix64(splitmix64(light_index) ^ f64_bits(x)) ^ f64_bits(y)) ^ f64_bits(z))


def jitter(h: int, j: int) -> float:
    """Draw j (2k: ju of sample k, 2k + 1: jv) in [0, 1): 53 bits times 2^-53."""
    return float(splitmix64(h ^ j) >> 11) * 2.0 ** -53


def sample_positions(light: AreaLight, light_index: int = 0, over_point=None) -> np.ndarray:
    """p_k = (corner + uc (u + ju)) + vc (v + jv) for k = v * usteps + u, componentwise f64 (one rounding per operation)."""
    corner = np.array(light.corner[:3], dtype=np.float64)
    uc = np.array(light.uvec[:3], dtype=np.float64) / float(light.usteps)
    vc = np.array(light.vvec[:3], dtype=np.float64) / float(light.vsteps)
    h = area_hash(light_index, *over_point[:3]) if light.jitter else 0
    out = []
    for v in range(light.vsteps):
        for u in range(light.usteps):
            k = v * light.usteps + u
            ju, jv = (jitter(h, 2 * k), jitter(h, 2 * k + 1)) if light.jitter else (0.5, 0.5)
            out.append((corner + uc * (float(u) + ju)) + vc * (float(v) + jv))
    return np.array(out, dtype=np.float64)


def equivalent_point_lights(light: AreaLight, light_index: int = 0, over_point=None):
    """The N point lights of intensity / N an unjittered area light shades exactly like (for the surface colour)."""
    n = float(light.samples)
    inten = Color(light.intensity.r / n, light.intensity.g / n, light.intensity.b / n)
    return [PointLight(inten, Vector.point(*p)) for p in sample_positions(light, light_index, over_point)]


def square_light(n=2, jit=False):
    return AreaLight(Color(1.0, 0.9, 0.8), Vector.point(0.0, 5.0, 0.0), Vector.vector(2.0, 0.0, 0.0), n, Vector.vector(0.0, 0.0, 2.0), n, jit)


# ---- the API ------------------------------------------------------------------------------------------------------------------------
def test_area_light_api_and_mixed_world():
    a = square_light(2)
    assert (a.usteps, a.vsteps, a.samples, a.jitter) == (2, 2, 4, False)
    b = AreaLight(Color.white(), Vector.point(1, 2, 3), Vector.vector(1, 0, 0), 3, Vector.vector(0, 1, 0), 1, jitter=True)
    assert b.samples == 3 and b.jitter
    p = PointLight(Color.white(), Vector.point(-10, 10, -10))
    w = World([a, p, b], [Element.sphere(ShapeArgs())])
    assert w.lights == [a, p, b]          # any mix, in order
    assert isinstance(w.lights[0], AreaLight) and isinstance(w.lights[1], PointLight)
    with pytest.raises(Exception):
        a.usteps = 3                      # frozen like PointLight


def test_splitmix64_and_hash_against_known_values():
    assert splitmix64(0) == 0
    # SplitMix64 seeded with 0: its first output is the finaliser of the golden-ratio increment
    assert splitmix64(0x9E3779B97F4A7C15) == 0xE220A8397B1DCDAF
    assert f64_bits(1.0) == 0x3FF0000000000000 and f64_bits(-0.0) == 1 << 63
    h = area_hash(0, 0.0, 0.0, 0.0)
    assert h == splitmix64(splitmix64(splitmix64(splitmix64(0))))  # all-zero bits: the chain of finalisers
    assert h == 0
    h1 = area_hash(1, 0.5, 1e-5, -2.0)
    assert h1 == splitmix64(splitmix64(splitmix64(splitmix64(1) ^ 0x3FE0000000000000) ^ f64_bits(1e-5)) ^ 0xC000000000000000)
    assert h1 != area_hash(2, 0.5, 1e-5, -2.0) and h1 != area_hash(1, 0.5, 1e-5, 2.0)
    for j in range(64):
        x = jitter(h1, j)
        assert 0.0 <= x < 1.0 and x * 2.0 ** 53 == float(int(x * 2.0 ** 53))   # 53-bit grid
    assert jitter(0, 0) == 0.0


def test_sample_positions_hand_computed():
    # 2 x 2 over [0, 2] x [0, 2] at y = 5: the cell centres, u inner
    p = sample_positions(square_light(2))
    assert p.tolist() == [[0.5, 5.0, 0.5], [1.5, 5.0, 0.5], [0.5, 5.0, 1.5], [1.5, 5.0, 1.5]]
    # 3 x 1: uc = (1/3, 0, 0): (corner + uc * 0.5) etc., each rounded once
    a = AreaLight(Color.white(), Vector.point(-1.0, 4.0, 2.0), Vector.vector(1.0, 0.0, 0.0), 3, Vector.vector(0.0, 0.0, 3.0), 1)
    third = 1.0 / 3.0
    want = [[(-1.0 + third * 0.5) + 0.0 * 0.5, 4.0, (2.0 + 0.0) + 3.0 * 0.5],   # vsteps = 1: one row at v + 0.5 of vc = (0, 0, 3)
            [(-1.0 + third * 1.5) + 0.0, 4.0, 3.5],
            [(-1.0 + third * 2.5) + 0.0, 4.0, 3.5]]
    assert sample_positions(a).tolist() == want
    # jittered: inside the cells, reproducible, and different at another shading point
    j = square_light(4, jit=True)
    q1 = sample_positions(j, 3, (0.25, 1e-5, -0.5))
    assert np.array_equal(q1, sample_positions(j, 3, (0.25, 1e-5, -0.5)))
    assert not np.array_equal(q1, sample_positions(j, 3, (0.25, 1e-5, -0.25)))
    assert not np.array_equal(q1, sample_positions(j, 2, (0.25, 1e-5, -0.5)))
    cells = np.array([[u * 0.5, v * 0.5] for v in range(4) for u in range(4)])
    assert ((q1[:, [0, 2]] >= cells) & (q1[:, [0, 2]] < cells + 0.5)).all() and (q1[:, 1] == 5.0).all()
    h = area_hash(3, 0.25, 1e-5, -0.5)
    assert q1[5, 0] == 0.0 + 0.5 * (1.0 + jitter(h, 10)) and q1[5, 2] == 0.0 + 0.5 * (1.0 + jitter(h, 11))
    eq = equivalent_point_lights(square_light(2))
    assert len(eq) == 4 and eq[0].intensity == Color(0.25, 0.9 / 4.0, 0.8 / 4.0)


# ---- the libraries -------------------------------------------------------------------------------------------------------------------
def test_product_library_exports_the_ex_entry_points():
    lib = load(LIB)
    for name in ("rtc_scene_create_ex", "rtc_multi_create_ex", "rtw_world_add_area_light"):
        assert hasattr(lib, name), name
    import raytracer_challenge_amd as rt
    assert rt.hip_backend().has_area_lights


def test_oracle_refuses_area_lights(orc):
    assert not orc.has_area_lights
    w = World([PointLight(Color.white(), Vector.point(0, 5, 0)), square_light(2)], [Element.sphere(ShapeArgs())])
    with pytest.raises(RtwError, match="area lights need librtc_amd.so"):
        orc.build_world(w)
    orc.build_world(World([PointLight(Color.white(), Vector.point(0, 5, 0))], [Element.sphere(ShapeArgs())]))   # point lights: as before


def test_emulator_library_still_loads_and_reports_area_lights_missing():
    """tests/cpu_emu links the product's rtw_capi.cpp without rtc_scene_create_ex: the library must still load (the reference to it
    is weak) and render point-light worlds; a world with an area light fails with a message."""
    from emu_lib import emu
    from raytracer_challenge_amd.scene import Camera
    e = emu()
    cam = Camera.new(8, 6, 1.0, Camera.transform(Vector.point(0, 1.5, -5), Vector.point(0, 1, 0), Vector.vector(0, 1, 0)))
    rgb, _ = e.render(e.build_world(World.default()), cam, 1)
    assert np.isfinite(rgb).all() and rgb.max() > 0.0
    nw = e.build_world(World([square_light(2)], [Element.sphere(ShapeArgs())]))
    with pytest.raises(RtwError, match="rtc_scene_create_ex"):
        e.render(nw, cam, 1)


def test_flatten_helpers_refuse_worlds_with_area_lights():
    """rtw_world_flatten_counts / _desc hand out the descriptor of rtc_scene_create; a world with an area light has none (its lights are
    an rtc_light_ex list), so they fail instead of dropping the area lights.  Flattening needs no GPU."""
    import raytracer_challenge_amd as rt
    hip = rt.hip_backend()
    lib = hip.lib
    counts = (C.c_uint32 * 8)()
    desc = RtcSceneDesc()
    point = PointLight(Color.white(), Vector.point(0, 5, 0))
    nw = hip.build_world(World([point], [Element.sphere(ShapeArgs())]))
    assert lib.rtw_world_flatten_counts(nw.handle, counts) == 0 and counts[7] == 1
    assert lib.rtw_world_flatten_desc(nw.handle, desc) == 0
    nw = hip.build_world(World([point, square_light(2)], [Element.sphere(ShapeArgs())]))
    assert lib.rtw_world_flatten_counts(nw.handle, counts) != 0
    assert "area lights" in hip._err()
    assert lib.rtw_world_flatten_desc(nw.handle, desc) != 0


def test_rust_shim_mirrors_rtc_light_ex():
    h = open(os.path.join(ROOT, "include", "rtc.h")).read()
    rs = open(os.path.join(ROOT, "shim", "gpu.rs")).read()
    c, r = c_struct(h, "rtc_light_ex"), rust_struct(rs, "RtcLightEx")
    assert c == r, (c, r)
    assert [f[0] for f in c] == ["kind", "usteps", "vsteps", "flags", "intensity", "corner", "uvec", "vvec"]
    assert "fn rtc_scene_create_ex(" in rs and "fn rtc_multi_create_ex(" in rs
