"""wf_shade's queues through the CPU emulation of the kernel source (tests/cpu_emu), which runs the software-pipelined loop of the
all-Plain build and the plain loop of the pattern build: both device paths bit for bit, and the oracle (wf_shade_queues.py).  The
emulator has no entry point for area lights or UV patterns; test_wf_shade_queues_gpu.py covers those readers of the shade record."""
import pytest

import wf_shade_queues as q


@pytest.fixture(scope="module")
def emu():
    from emu_lib import emu as _emu
    return _emu()


@pytest.mark.parametrize("scene,camera,fuel,ask_oracle", q.case_list(sorted(q.SCENES)), ids=lambda v: str(v))
def test_wavefront_queues_emulated(emu, orc, monkeypatch, scene, camera, fuel, ask_oracle):
    q.check_case(emu, orc, monkeypatch, scene, camera, fuel, ask_oracle)


def test_simt_emulation_of_the_pipelined_loop(orc, monkeypatch):
    """One thread per lane (64-lane blocks, real ballots and barriers): the prefetch of lanes without a hit and of lanes past the
    level's end, 23x23 = 576 padded work ids over nine blocks."""
    import os
    import subprocess
    from emu_lib import EMU_DIR
    from raytracer_challenge_amd.backend import Backend
    subprocess.run(["make", "-s", "-C", EMU_DIR, "simt"], check=True)
    simt = Backend(os.path.join(EMU_DIR, "_build", "librtc_emu_simt.so"))
    for scene in ("nested_glass", "plain_and_patterned"):
        q.check_case(simt, orc, monkeypatch, scene, "23x23", 5, True)
