"""The creation matrix without a device: every fault that each of the twelve rtc_*_create* entry points can be handed -- alone, and in
pairs from two different groups (bump records, background, cones, a NULL handle) -- answers the return code and the rtc_last_error()
text recorded in tests/golden/create_entry_points.json, so the order of the checks cannot move unnoticed.  The table holds only faults
that are answered before the device is looked for (create_cases.py): it gives the same answers with and without a GPU."""
import json
import os

import create_cases as cc
import foreign_flattener as ff
from raytracer_challenge_amd.cabi import load

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIB = os.path.join(ROOT, "raytracer_challenge_amd", "csrc", "librtc_amd.so")
GOLDEN = os.path.join(ROOT, "tests", "golden", "create_entry_points.json")


def test_every_fault_and_pair_answers_as_recorded():
    golden = json.load(open(GOLDEN))
    assert len(golden["commit"]) == 40
    flat = ff.flatten(cc.small_world())
    desc = flat.desc()
    assert desc.n_lights == 2 and desc.n_materials == 2 and desc.n_pattern_nodes >= 1
    got = cc.answers(load(LIB), desc)
    assert sorted(got) == sorted(golden["rows"])
    # 12 entry points x (NULL desc, NULL out); cones through 6 of them, a background through 4, bump records through 2
    n_single = 12 * 2 + 6 * 3 + 4 * 2 + 2 * 3
    # pairs with a NULL handle: 3 cone faults (_ext2 up), 2 of the background (_ext3 up), 3 of the bumps (_ext4); cone x background 6,
    # bump x cone 9, bump x background 6; scene and multi
    n_pairs = 2 * (3 * 3 + 2 * 2 + 3 + 6 * 2 + 9 + 6)
    assert sum(" + " not in case for case in got) == n_single and len(got) == n_single + n_pairs
    wrong = {case: (a, golden["rows"][case]) for case, a in got.items()
             if a["rc"] != golden["rows"][case]["rc"] or a["message"] not in golden["rows"][case]["messages"]}
    assert not wrong, wrong
    # the one tolerance: a NULL descriptor through the multi entry points reads "NULL argument" or "NULL argument / no devices" -- the
    # same one through all six
    assert len({a["message"] for case, a in got.items() if case.startswith("rtc_multi") and "NULL desc" in case}) == 1
    # a handle that was passed is NULL after every failure
    assert all(a["out_cleared"] for a in got.values()), [case for case, a in got.items() if not a["out_cleared"]]
    # every row is a refusal of the arguments (RTC_ERR_INVALID), never of the machine
    assert {a["rc"] for a in got.values()} == {1}
