"""The twelve creation entry points of include/rtc.h (rtc_scene_create, _ex, _ext .. _ext4 and rtc_multi_create, _ex, _ext .. _ext4) behind
one calling convention, and the table of faults that each of them answers before it looks for a device.  Shared by
test_create_entry_points_cpu.py (the table against tests/golden/create_entry_points.json) and test_create_entry_points_gpu.py (valid
calls with empty extras).

    python tests/create_cases.py <librtc_amd.so> <commit> <out.json>

writes the golden file: the table's answers from the library of the given commit."""
import ctypes as C
import itertools
import json
import sys

import foreign_flattener as ff
from raytracer_challenge_amd.cabi import RtcBackground, RtcBump, RtcLightCone, RtcLightEx, RtcSceneExt, load  # noqa: F401
from raytracer_challenge_amd.scene import Color, Element, PointLight, ShapeArgs, Vector, World

vp = C.c_void_p
LEVELS = ("", "_ex", "_ext", "_ext2", "_ext3", "_ext4")
ENTRIES = [("rtc_multi_create" if multi else "rtc_scene_create") + level for multi in (False, True) for level in LEVELS]


def small_world():
    """A sphere, a plane, two point lights: one material each (the foreign flattener emits a record per shape)."""
    return World([PointLight(Color.white(), Vector.point(-10, 10, -10)), PointLight(Color(0.5, 0.5, 0.5), Vector.point(5, 8, -6))],
                 [Element.sphere(ShapeArgs()), Element.plane(ShapeArgs())])


def create(lib, entry, desc, out, devices=(0,), lights=None, n_lights=0, ext=None, cones=None, n_cones=0, bg=None, bumps=None, n_bumps=0):
    """One call of `entry` with what it can carry of the keyword arguments (the others must be empty).  Every argument is a ctypes object
    or None for NULL; `out` is a c_void_p to fill or None."""
    level = entry[len("rtc_scene_create"):]
    extras = {"": [], "_ex": [lights, n_lights], "_ext": [ext], "_ext2": [ext, cones, n_cones], "_ext3": [ext, cones, n_cones, bg],
              "_ext4": [ext, cones, n_cones, bg, bumps, n_bumps]}[level]
    assert (level in ("_ext2", "_ext3", "_ext4") or n_cones == 0) and (level in ("_ext3", "_ext4") or bg is None) and (level == "_ext4" or n_bumps == 0), entry
    assert (level == "_ex" or lights is None) and (level not in ("", "_ex") or ext is None), entry
    where = [(C.c_int * len(devices))(*devices), len(devices)] if entry.startswith("rtc_multi") else [devices[0]]
    return getattr(lib, entry)(desc, *extras, *where, out)


# ---- the faults: (group, name) -> keyword arguments of create().  Every one is answered before the device is looked for. ------------
def faults(desc):
    down = (C.c_double * 3)(0.0, -1.0, 0.0)
    cone = lambda light: RtcLightCone(light, 0, down, 0.9, 0.5)  # noqa: E731
    bump = lambda material: RtcBump(material, 0, 0, 0, 0.05, 2.0)  # noqa: E731  (a simplex bump)
    return {
        ("desc", "NULL desc"): {"desc": None},
        ("out", "NULL out"): {"out": None},
        ("cone", "cones NULL"): {"cones": None, "n_cones": 1},
        ("cone", "cone index out of range"): {"cones": (RtcLightCone * 1)(cone(desc.n_lights)), "n_cones": 1},
        ("cone", "duplicate cone light"): {"cones": (RtcLightCone * 2)(cone(1), cone(1)), "n_cones": 2},
        ("bg", "unknown projection"): {"bg": RtcBackground(0, 2)},
        ("bg", "pattern out of range"): {"bg": RtcBackground(int(desc.n_pattern_nodes), 0)},
        ("bump", "bumps NULL"): {"bumps": None, "n_bumps": 1},
        ("bump", "bump material out of range"): {"bumps": (RtcBump * 1)(bump(desc.n_materials)), "n_bumps": 1},
        ("bump", "two bumps on one material"): {"bumps": (RtcBump * 2)(bump(0), bump(0)), "n_bumps": 2},
    }


def carries(entry, group):
    level = entry[len("rtc_scene_create"):]
    return group in ("desc", "out") or (group == "cone" and level in ("_ext2", "_ext3", "_ext4")) or (group == "bg" and level in ("_ext3", "_ext4")) or (
        group == "bump" and level == "_ext4")


def table(desc):
    """[(case id, entry, keyword arguments)]: per entry point every fault it can carry, then every pair of faults from two different
    groups among bump, background, cone and NULL out."""
    F = faults(desc)
    rows = []
    for entry in ENTRIES:
        mine = [k for k in F if carries(entry, k[0])]
        for k in mine:
            rows.append(("%s | %s" % (entry, k[1]), entry, dict(F[k])))
        for a, b in itertools.combinations([k for k in mine if k[0] != "desc"], 2):
            if a[0] != b[0]:
                rows.append(("%s | %s + %s" % (entry, a[1], b[1]), entry, {**F[a], **F[b]}))
    return rows


def answers(lib, desc):
    """{case id: {"rc", "message", "out_cleared"}} of the table on `lib`."""
    out = {}
    for case, entry, kw in table(desc):
        kw = dict(kw)
        handle = vp(0xdead0)  # (never followed: every row fails)
        d = kw.pop("desc", desc)
        o = kw.pop("out", handle)
        rc = create(lib, entry, d, o, **kw)
        out[case] = {"rc": rc, "message": lib.rtc_last_error().decode(), "out_cleared": o is None or not handle.value}
        assert rc != 0, case
    return out


if __name__ == "__main__":
    lib_path, commit, dst = sys.argv[1:4]
    flat = ff.flatten(small_world())
    got = answers(load(lib_path), flat.desc())
    rows = {}
    for case, a in got.items():
        msgs = [a["message"]]
        if case.startswith("rtc_multi") and "NULL desc" in case:  # either wrapper's spelling (see the test)
            msgs = ["NULL argument", "NULL argument / no devices"]
            assert a["message"] in msgs, a
        rows[case] = {"rc": a["rc"], "messages": msgs}
    with open(dst, "w") as f:
        json.dump({"commit": commit, "library": "raytracer_challenge_amd/csrc/librtc_amd.so", "rows": rows}, f, indent=1, sort_keys=True)
        f.write("\n")
    print("%d rows" % len(rows))
