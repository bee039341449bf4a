"""The product's host build under ThreadSanitizer (tests/cpu_emu/threads_tsan.cpp): four threads build worlds through rtw.h at once --
a small analytic one, the low teapot, a generated mesh of 131 072 triangles that starts both internal thread pools -- and have each
flattened and built; the main thread then renders every one and holds it to the frame it rendered before any thread started.  The
program is a plain child process that carries its own sanitizer runtime.  `--racy` is the positive control: an unguarded counter that
ThreadSanitizer must report.  (`make tsan` compiles for about 25 s the first time; the run takes under 10 s.)"""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EMU = os.path.join(ROOT, "tests", "cpu_emu")
PROGRAM = os.path.join(EMU, "_build_tsan", "threads_tsan")
TEAPOT = os.path.join(ROOT, "assets", "obj", "teapot_low.obj")
N_THREADS = 4


@pytest.fixture(scope="module")
def program():
    subprocess.run(["make", "-s", "-C", EMU, "tsan"], check=True)
    return PROGRAM


def run(args):
    return subprocess.run(args, stdout=subprocess.PIPE, stderr=subprocess.PIPE, universal_newlines=True, timeout=300)


def test_concurrent_host_builds_are_race_free_and_render_the_same_bits(program):
    r = run([program, TEAPOT, str(N_THREADS)])
    assert "ThreadSanitizer" not in r.stderr, r.stderr[-4000:]
    assert r.returncode == 0, (r.returncode, r.stdout[-2000:], r.stderr[-2000:])
    lines = r.stdout.splitlines()
    want = ["same bits: %s (thread %d)" % (world, t) for t in range(N_THREADS) for world in ("small", "teapot", "grid131072")]
    assert lines == want, lines


def test_the_sanitizer_reports_a_deliberate_race(program):
    r = run([program, "--racy"])
    assert "ThreadSanitizer: data race" in r.stderr and r.returncode != 0, (r.returncode, r.stderr[-2000:])
