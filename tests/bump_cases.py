"""Bumped worlds shared by test_bump_gpu.py and the extended oracle's files (ext_cases.py): a world with bump records put on its
materials in the order they are met, and one scene per NP build of the one-kernel path (rtc_bump_info.trace_build 0..11).  Pure scene descriptions; nothing here needs a library."""
import dataclasses

import build_matrix as bm
from raytracer_challenge_amd.scene import Bump, World


def bumped(world, pick):
    """The world with pick(k) as the bump of the k-th material met (shapes, groups' materials and OBJ files, depth first)."""
    k = [0]

    def mat(m):
        if m is None:
            return None
        k[0] += 1
        return dataclasses.replace(m, bump=pick(k[0] - 1))

    def el(e):
        if e.tag == "shape":
            return dataclasses.replace(e, args=dataclasses.replace(e.args, material=mat(e.args.material)))
        if e.tag == "composite":
            return dataclasses.replace(e, material=mat(e.material), children=tuple(el(c) for c in e.children))
        return dataclasses.replace(e, material=mat(e.material))
    return World(world.lights, [el(e) for e in world.elements], world.background)


MIXED = (Bump.simplex(0.08, 2.0), Bump.fractal(3, 0.15, 1.5), Bump.ripple(0.1, 1.3), None)


def mixed(k):
    return MIXED[k % len(MIXED)]


ROWS = {  # row -> (scene of tests/build_matrix.py or the open world with the teapot, with a background?)
    0: ("csg", False), 1: ("area_csg_real", False), 2: ("uv_real", False), 3: ("uv_area_real", False), 4: ("spot_real", False), 5: ("uv_spot_real", False),
    6: ("open", True), 7: ("area_kops_real", True), 8: ("uv_real", True), 9: ("uv_area_real", True), 10: ("spot_real", True), 11: ("uv_spot_real", True),
}


def row_world(row, tmp_path=None):
    """(camera, the unbumped twin) of the scene that takes NP build `row` (rtc_bump_info.trace_build) once it carries a record.  None of these scenes
    writes a file: tmp_path is the build matrix's argument and may stay None."""
    from test_background_gpu import open_world, real_backgrounds
    name, bg = ROWS[row]
    sky = real_backgrounds()[0][1]
    if name == "open":                                                               # a glass-and-mirror ball, a CSG solid and the low teapot
        return bm.camera(), open_world(sky)
    cam, world = bm.BY_NAME[name].make(tmp_path)
    if bg:
        world = World(world.lights, world.elements[:1] + world.elements[2:], sky)   # without the back wall: the sky is in frame
    return cam, world
