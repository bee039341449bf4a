"""Errors belong to the caller, without a device (include/rtc.h "Threading"): two threads drive the product library through refusals that
are answered before any device is looked for -- the NULL and malformed descriptors of test_create_entry_points_cpu.py for rtc_last_error,
NULL children and a NULL element for rtw_last_error -- and each must read its own text back, every time, whatever the other thread does
meanwhile.  A successful call leaves the text alone.  The GPU twin (test_threads_gpu.py test 8) does the same around real renders."""
import ctypes as C
import os
import threading

import create_cases as cc
import foreign_flattener as ff
from raytracer_challenge_amd.cabi import load

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIB = os.path.join(ROOT, "raytracer_challenge_amd", "csrc", "librtc_amd.so")
ROUNDS = 2000     # calls of microseconds each: the two loops overlap for the whole run
JOIN_S = 60.0


def bound():
    lib = load(LIB)   # (a CDLL call releases the GIL: the two threads are inside the library at the same time)
    vp, d = C.c_void_p, C.c_double
    return lib


def run_pair(a, b):
    """a(slot), b(slot) on two threads that start together; the first exception of either is re-raised here."""
    gate = threading.Barrier(2)
    slots = [{"error": None}, {"error": None}]

    def body(fn, slot):
        try:
            gate.wait(JOIN_S)
            fn(slot)
        except BaseException as ex:  # noqa: BLE001
            slot["error"] = ex

    threads = [threading.Thread(target=body, args=(fn, s), daemon=True) for fn, s in ((a, slots[0]), (b, slots[1]))]
    for t in threads:
        t.start()
    for t in threads:
        t.join(JOIN_S)
        assert not t.is_alive(), "a worker did not finish"
    for s in slots:
        if s["error"] is not None:
            raise s["error"]
    return slots


def test_rtc_last_error_is_the_calling_threads_own():
    """Thread A walks four refusals of rtc_scene_create_ext4 with four different texts; thread B provokes a fifth once, then only makes
    calls that succeed.  A reads its own text after every call, B reads its first text after every call."""
    lib = bound()
    desc = ff.flatten(cc.small_world()).desc()
    F = cc.faults(desc)
    mine = [(F[("cone", "cones NULL")], b"cones is NULL"), (F[("bg", "unknown projection")], b"background: unknown projection"),
            (F[("cone", "duplicate cone light")], b"cone 1: light 1 already has a cone"), ({"desc": None}, b"NULL argument")]
    theirs = (F[("bump", "bumps NULL")], b"bumps is NULL")

    def refuse(kw):
        kw = dict(kw)
        handle = C.c_void_p(0xdead0)   # (never followed: every call fails)
        return cc.create(lib, "rtc_scene_create_ext4", kw.pop("desc", desc), handle, **kw)

    def a(slot):
        for k in range(ROUNDS):
            kw, text = mine[k % len(mine)]
            assert refuse(kw) == 1
            got = lib.rtc_last_error()
            assert got == text, "thread A, call %d: rtc_last_error() = %r, its own refusal reads %r" % (k, got, text)

    def b(slot):
        assert refuse(theirs[0]) == 1 and lib.rtc_last_error() == theirs[1]
        point, down = (C.c_double * 3)(), (C.c_double * 3)(0.0, -1.0, 0.0)
        for k in range(ROUNDS):
            assert lib.rtc_band_rows_owned(32, 5, 0, 1) == 32
            assert lib.rtc_background_point(0, down, point) == 0
            got = lib.rtc_last_error()
            assert got == theirs[1], "thread B, call %d: rtc_last_error() = %r after successful calls, its refusal read %r" % (k, got, theirs[1])

    run_pair(a, b)


def test_rtw_last_error_is_the_calling_threads_own():
    """The same through the world-building API: A alternates three refusals, B is refused once and then builds and releases patterns and
    worlds successfully."""
    lib = bound()
    mine = [(lambda: lib.rtw_pattern_jitter(0, 0, 1.0, 1, None), b"jitter: child is NULL"),
            (lambda: lib.rtw_texture_create(0, 0, None), b"texture: width and height must be at least 1"),
            (lambda: lib.rtw_pattern_mixture(0, None, None, None), b"mixture: child is NULL")]
    theirs = b"add_element: NULL/consumed element"

    def a(slot):
        for k in range(ROUNDS):
            call, text = mine[k % len(mine)]
            assert not call()
            got = lib.rtw_last_error()
            assert got == text, "thread A, call %d: rtw_last_error() = %r, its own refusal reads %r" % (k, got, text)

    def b(slot):
        w = lib.rtw_world_create()
        assert w and lib.rtw_world_add_element(w, None) == 1 and lib.rtw_last_error() == theirs
        lib.rtw_world_release(w)
        for k in range(ROUNDS):
            p, w = lib.rtw_pattern_plain(0.1, 0.2, 0.3), lib.rtw_world_create()
            assert p and w
            lib.rtw_pattern_release(p)
            lib.rtw_world_release(w)
            got = lib.rtw_last_error()
            assert got == theirs, "thread B, call %d: rtw_last_error() = %r after successful calls, its refusal read %r" % (k, got, theirs)

    run_pair(a, b)
