"""wf_shade's queues on an MI355X (cases and reasoning: wf_shade_queues.py): the software-pipelined all-Plain build, the pattern build
and the UV build, and the three readers of the shade record -- wf_shadow_rec, wf_shadow_rec_area and, through the colour rows, the
pattern colours.  Both device paths bit for bit; the oracle wherever it can answer."""
import numpy as np
import pytest

import wf_shade_queues as q
from parity import assert_parity
from raytracer_challenge_amd import Texture, UvPattern
from raytracer_challenge_amd.scene import AreaLight, Color, Matrix, Pattern, PointLight, Vector, World

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("scene,camera,fuel,ask_oracle", q.case_list(sorted(q.SCENES)), ids=lambda v: str(v))
def test_wavefront_queues(hip, orc, monkeypatch, scene, camera, fuel, ask_oracle):
    q.check_case(hip, orc, monkeypatch, scene, camera, fuel, ask_oracle)


@pytest.mark.parametrize("camera", sorted(q.CAMERAS))
def test_area_light_reader_of_plain_records(hip, orc, monkeypatch, camera):
    """wf_shadow_rec_area takes a Plain record's colour from the material table.  The oracle has no area lights: a degenerate one
    (uvec = vvec = 0, 2x2 samples) shades like the point light at its corner; a real one must agree between the paths."""
    cam, world = q.all_plain_glass()
    cam = q.sized(cam, camera)
    z = Vector.vector(0.0, 0.0, 0.0)
    degenerate = World([AreaLight(l.intensity, l.origin, z, 2, z, 2) for l in world.lights], world.elements)
    q.both_paths(hip, degenerate, cam, 5, monkeypatch)
    ref = orc.render_with_digest(orc.build_world(world), cam, 5)
    monkeypatch.setenv("RTC_KERNEL", "4")
    assert_parity(hip, orc, degenerate, cam, 5, label="degenerate area light %s" % camera, ref=ref)
    soft = World([AreaLight(Color(1.0, 0.9, 0.8), Vector.point(-6, 8, -8), Vector.vector(2, 0, 0), 3, Vector.vector(0, 0, 2), 2, True),
                  PointLight(Color(0.2, 0.2, 0.3), Vector.point(4, 5, -3))], world.elements)
    q.both_paths(hip, soft, cam, 5, monkeypatch)


@pytest.mark.parametrize("camera", sorted(q.CAMERAS))
def test_uv_build_mixes_plain_and_textured_records(hip, orc, monkeypatch, camera):
    """wf_shade's UV build: textured materials keep their colour rows, Plain ones beside them do not.  The oracle has no textures: a
    one-colour texture shades like Plain(c), and the product must give the all-Plain world's bits."""
    import dataclasses
    cam, plain_world = q.all_plain_glass()
    cam = q.sized(cam, camera)
    c0 = Color(0.6, 0.5, 0.4)
    tex = Pattern.texture_map(Matrix.scaling(0.7, 0.7, 0.7), "spherical", UvPattern.image(Texture(np.broadcast_to(np.array([c0.r, c0.g, c0.b]), (5, 7, 3)))))
    els = [dataclasses.replace(e, args=dataclasses.replace(e.args, material=dataclasses.replace(e.args.material, pattern=tex)))
           if e.args.material.pattern.color == c0 else e for e in plain_world.elements]
    uv_world = World(plain_world.lights, els)
    assert any(e.args.material.pattern.tag == "uv" for e in els) and any(e.args.material.pattern.tag == "plain" for e in els)
    rgb, _, _ = q.both_paths(hip, uv_world, cam, 5, monkeypatch)
    ref = orc.render_with_digest(orc.build_world(plain_world), cam, 5)
    monkeypatch.setenv("RTC_KERNEL", "4")
    assert_parity(hip, orc, uv_world, cam, 5, label="one-colour texture %s" % camera, ref=ref)
    assert np.array_equal(rgb.view(np.uint64), hip.render(hip.build_world(plain_world), cam, 5)[0].view(np.uint64))
