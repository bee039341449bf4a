"""Records and exact references for the culling predicates of the ray kernels (csrc/rtc_device.hpp; include/rtc.h rtc_cull_probe_raw).

Every predicate only SKIPS work that an exact f64 test would have rejected anyway, so each has a one-sided contract -- it may never
skip what the exact arithmetic takes -- and, so that "skip nothing" does not pass, a second side wherever the issue of usefulness is
stated in numbers.  The references here are Python `fractions.Fraction` on the exact binary values of a record, or numpy's correctly
rounded f64 operations where the reference's own rule is an f64 expression.  Nothing of the library is imported.

Record layouts: include/rtc.h RTC_CULL_*.  Generators are seeded and cached: a module computes each family once."""
import functools
import math
from fractions import Fraction

import numpy as np

SLAB, POINT, GATE, PLANE, BEHIND = 0, 1, 2, 3, 4
EPSILON = 0.00001
INF = math.inf
F32_MAX = float(np.finfo(np.float32).max)


def f32(x):
    """x rounded to f32, carried in f64."""
    with np.errstate(over="ignore", invalid="ignore"):
        return np.asarray(x, dtype=np.float64).astype(np.float32).astype(np.float64)


# ---------------------------------------------------------------------------------------------------------------- slab
# fr[4] (centre, radius), o[3], d[3], tlo, thi, lo[3], hi[3]
SPECIAL_COMPONENTS = (0.0, -0.0, 1e-40, -1e-40, 1e-31, -1e-31, 1e-20, -1e-20)
NUDGES = (0.0, 1e-16, 1e-13, 1e-10, 1e-8, 1e-7, 1e-6, 1e-5, 1e-4, 1e-3)


def _frames(rng, n, rad_exp):
    """Radii 10^rad_exp, centres 0 (exact frame coordinates), a few radii or up to 100 radii away from the origin of the space."""
    R = 10.0 ** rng.uniform(rad_exp[0], rad_exp[1], n)
    kind = rng.integers(0, 3, n)
    c = rng.uniform(-1.0, 1.0, (n, 3)) * (R * np.where(kind == 0, 0.0, np.where(kind == 1, 3.0, 100.0)))[:, None]
    return c, R


def _boxes(rng, n, R):
    """f32 boxes within the radius of the centre, sides from 1e-3 to half a radius; lo <= hi."""
    bc = rng.uniform(-0.8, 0.8, (n, 3)) * R[:, None]
    hs = 10.0 ** rng.uniform(-3.0, -0.3, (n, 3)) * R[:, None]
    lo, hi = f32(np.clip(bc - hs, -R[:, None], R[:, None])), f32(np.clip(bc + hs, -R[:, None], R[:, None]))
    return lo, np.maximum(lo, hi)


def _surface_points(rng, lo, hi):
    """A point of each box: per axis at lo, at hi or between (faces, edges, corners, and a few interior points)."""
    pick = rng.integers(0, 3, lo.shape)
    return np.where(pick == 0, lo, np.where(pick == 1, hi, lo + rng.uniform(0, 1, lo.shape) * (hi - lo)))


def _aimed(rng, n, rad_exp=(-3.0, 6.0), dist_exp=(-2.0, 2.0)):
    """Rays aimed at a point p of the box from dist radii away, direction lengths 1e-3 .. 1e3, nudged off by 0 .. 1e-3.
    Returns the pieces: c, R, frame-relative origin, d, lo, hi, the parameter t_p at which the un-nudged ray reaches p."""
    c, R = _frames(rng, n, rad_exp)
    lo, hi = _boxes(rng, n, R)
    p = _surface_points(rng, lo, hi)
    u = rng.normal(size=(n, 3))
    u /= np.linalg.norm(u, axis=1, keepdims=True)
    dist = R * 10.0 ** rng.uniform(dist_exp[0], dist_exp[1], n)
    of = p - u * dist[:, None]
    w = rng.normal(size=(n, 3))
    d = u + rng.choice(NUDGES, n)[:, None] * w
    length = 10.0 ** rng.uniform(-3.0, 3.0, n)
    d *= length[:, None]
    return c, R, of, d, lo, hi, dist / length


def _records(c, R, of, d, tlo, thi, lo, hi):
    n = len(R)
    rec = np.empty((n, 18))
    rec[:, 0:3], rec[:, 3], rec[:, 4:7], rec[:, 7:10] = c, R, c + of, d
    rec[:, 10], rec[:, 11], rec[:, 12:15], rec[:, 15:18] = tlo, thi, lo, hi
    return rec


def _slab_aimed(rng, n):
    c, R, of, d, lo, hi, _ = _aimed(rng, n)
    return _records(c, R, of, d, 0.0, INF, lo, hi)


def _slab_frames(rng, n):
    """Frame radii up to 1e28, origins up to 1e4 radii from the box."""
    c, R, of, d, lo, hi, _ = _aimed(rng, n, rad_exp=(-3.0, 28.0), dist_exp=(-2.0, 4.0))
    return _records(c, R, of, d, 0.0, INF, lo, hi)


def _set_special_axes(rng, c, of, d, lo, hi, R, specials, second=0.3):
    """One axis (sometimes two) of each ray gets a special direction component; on that axis the origin sits exactly on a face (the
    centre's coordinate is made 0 so that o - c is the face), inside the slab, or outside it."""
    n = len(R)
    rows = np.arange(n)
    for rnd in range(2):
        k = rng.integers(0, 3, n)
        on = np.ones(n, dtype=bool) if rnd == 0 else rng.random(n) < second
        around = EPSILON * (1.0 + rng.uniform(-1e-3, 1e-3, n)) * rng.choice([-1.0, 1.0], n)
        val = np.where(rng.random(n) < 0.2, around, rng.choice(specials, n))
        where = rng.integers(0, 5, n)
        lk, hk = lo[rows, k], hi[rows, k]
        pos = np.select([where == 0, where == 1, where == 2, where == 3],
                        [lk, hk, lk + rng.uniform(0, 1, n) * (hk - lk), hk + R * 10.0 ** rng.uniform(-6.0, 1.0, n)],
                        lk - R * 10.0 ** rng.uniform(-6.0, 1.0, n))
        d[rows[on], k[on]] = val[on]
        of[rows[on], k[on]] = pos[on]
        c[rows[on], k[on]] = 0.0
    return c, of, d


def _slab_components(rng, n):
    """Direction components 0, -0, +-1e-40, +-1e-31, +-1e-20 and around EPSILON, in frames of every radius."""
    c, R, of, d, lo, hi, _ = _aimed(rng, n, rad_exp=(-3.0, 28.0))
    c, of, d = _set_special_axes(rng, c, of, d, lo, hi, R, SPECIAL_COMPONENTS)
    return _records(c, R, of, d, 0.0, INF, lo, hi)


def _slab_parallel_far(rng, n):
    """Axis-parallel rays in big frames (radii 4e8 .. 1e28): two components are 0, -0 or +-1e-35, the origin lies inside those two
    slab pairs or on their faces, so the ray enters the box; the scaled origins (o - c) / d exceed the f32 range."""
    c, R, of, d, lo, hi, _ = _aimed(rng, n, rad_exp=(8.6, 28.0), dist_exp=(-1.0, 2.0))
    c[:] = 0.0
    j = rng.integers(0, 3, n)
    rows = np.arange(n)
    for k in range(3):
        par = j != k
        where = rng.integers(0, 3, n)
        pos = np.where(where == 0, lo[:, k], np.where(where == 1, hi[:, k], lo[:, k] + rng.uniform(0, 1, n) * (hi[:, k] - lo[:, k])))
        of[par, k] = pos[par]
        d[par, k] = rng.choice([0.0, -0.0, 0.0, 1e-35, -1e-35], n)[par]
    dj = d[rows, j]
    d[rows, j] = np.where(dj == 0.0, 1.0, dj)
    return _records(c, R, of, d, 0.0, INF, lo, hi)


TINY_MINOR = (0.0, -0.0, 1e-31, -1e-31, 1e-40, -1e-40)


def _slab_tiny_dir(rng, n):
    """Directions that are tiny on ALL three axes: one component of 1e-30 .. 1e-22 in magnitude, heading for the box, the other two 0,
    -0, +-1e-31 or +-1e-40.  On those two axes the origin sits on a face, inside the slab or (a quarter each) outside it.  Frames of
    1e-3 .. 1e3 radii with origins within 10 radii: every scaled origin (o - c) / d stays inside the f32 range, so nothing but the
    direction's own size tells such a frame from an ordinary one -- 1e30 stands for 1 / d on two axes while the third's true 1 / d
    is nearly as large, and the t's of the third axis leave the +-2^-20 m 1e30 that the capped slabs span around 0."""
    c, R, of, d, lo, hi, _ = _aimed(rng, n, rad_exp=(-3.0, 3.0), dist_exp=(-1.0, 1.0))
    c[:] = 0.0
    j = rng.integers(0, 3, n)
    rows = np.arange(n)
    for k in range(3):
        minor = j != k
        where = rng.integers(0, 4, n)
        out = np.where(rng.random(n) < 0.5, hi[:, k] + R * 10.0 ** rng.uniform(-3.0, 0.0, n), lo[:, k] - R * 10.0 ** rng.uniform(-3.0, 0.0, n))
        pos = np.select([where == 0, where == 1, where == 2], [lo[:, k], hi[:, k], lo[:, k] + rng.uniform(0, 1, n) * (hi[:, k] - lo[:, k])], out)
        of[minor, k] = pos[minor]
        d[minor, k] = rng.choice(TINY_MINOR, n)[minor]
    d[rows, j] = np.where(np.signbit(d[rows, j]), -1.0, 1.0) * 10.0 ** rng.uniform(-30.0, -22.0, n)
    return _records(c, R, of, d, 0.0, INF, lo, hi)


def _slab_intervals(rng, n):
    """The passes' intervals: [0, dist] with dist within +-1e-12 of the face the ray is aimed at (shadow rays), (-inf, t] (container
    passes; boxes behind the origin count), and [t, t - 1 ulp] (empty)."""
    c, R, of, d, lo, hi, tp = _aimed(rng, n)
    kind = rng.integers(0, 3, n)
    flip = (kind == 1) & (rng.random(n) < 0.5)   # container pass: the box lies behind the origin
    d[flip] = -d[flip]
    rel = rng.choice([0.0, 1e-16, 1e-14, 1e-13, 1e-12], n) * rng.choice([-1.0, 1.0], n)
    t_shadow = tp * (1.0 + rel)
    t_cont = tp * rng.uniform(0.0, 2.0, n)
    tlo = np.select([kind == 0, kind == 1], [0.0, -INF], tp)
    thi = np.select([kind == 0, kind == 1], [t_shadow, t_cont], np.nextafter(tp, -INF))
    return _records(c, R, of, d, tlo, thi, lo, hi)


SLAB_FAMILIES = {   # name -> (generator, records)
    "aimed": (_slab_aimed, 6000),
    "frames": (_slab_frames, 5000),
    "components": (_slab_components, 6000),
    "parallel_far": (_slab_parallel_far, 3000),
    "intervals": (_slab_intervals, 6000),
    "tiny_dir": (_slab_tiny_dir, 3000),   # (new families go last: each draws from the one generator after those before it)
}


def slab_exact(rec):
    """Some t in [tlo, thi] puts (o - c) + t d inside [lo, hi] on all three axes, in exact arithmetic.  A zero d_k: o_k - c_k inside, or
    the axis is empty.  Finite records only."""
    c, o, d = rec[0:3], rec[4:7], rec[7:10]
    t0 = None if rec[10] == -INF else Fraction(rec[10])
    t1 = None if rec[11] == INF else Fraction(rec[11])
    for k in range(3):
        p = Fraction(o[k]) - Fraction(c[k])
        lo, hi = Fraction(rec[12 + k]), Fraction(rec[15 + k])
        if lo > hi:
            return False
        if d[k] == 0.0:
            if not (lo <= p <= hi):
                return False
            continue
        dk = Fraction(d[k])
        a, b = (lo - p) / dk, (hi - p) / dk
        if a > b:
            a, b = b, a
        t0 = a if t0 is None or a > t0 else t0
        t1 = b if t1 is None or b < t1 else t1
    return t0 is None or t1 is None or t0 <= t1


def slab_eps(rec):
    """eps of make_frame: 2^-20 (|fl32(o - c)|_inf + R), the f64 value (its own f32 roundings are 2^-24 of it)."""
    of = f32(rec[4:7] - rec[0:3])
    return 2.0 ** -20 * (float(np.abs(of).max()) + float(f32(rec[3]))) + 1e-30


def slab_ordinary(rec):
    """The frames the usefulness property is stated for: finite, every direction component 0 or at least 1e-20 in magnitude (not all
    0), and the scaled origins (|of|_inf + R) / |d_k| -- with 1e30 standing for 1 / 0 as in the code -- a decade inside the f32 range."""
    d = rec[7:10]
    if not (np.isfinite(rec[:10]).all() and np.isfinite(rec[12:]).all()):
        return False
    nz = d != 0.0
    if not nz.any() or (np.abs(d[nz]) < 1e-20).any() or (np.abs(d) > 1e30).any():
        return False
    imax = 1e30 if (~nz).any() else 1.0 / float(np.abs(d).min())
    m = slab_eps(rec) * 2.0 ** 20
    return m < 1e30 and m * imax < 1e37


def slab_clear_miss(rec):
    """The exact line misses the box inflated by 16 eps on every side, over [tlo, thi] widened by 2^-16 relative (of max(|t|, 1))."""
    e = Fraction(16.0 * slab_eps(rec))
    w = rec.copy()
    if math.isfinite(w[10]):
        w[10] = w[10] - 2.0 ** -16 * max(abs(w[10]), 1.0)
    if math.isfinite(w[11]):
        w[11] = w[11] + 2.0 ** -16 * max(abs(w[11]), 1.0)
    c, o, d = w[0:3], w[4:7], w[7:10]
    t0 = None if w[10] == -INF else Fraction(w[10])
    t1 = None if w[11] == INF else Fraction(w[11])
    for k in range(3):
        p = Fraction(o[k]) - Fraction(c[k])
        lo, hi = Fraction(w[12 + k]) - e, Fraction(w[15 + k]) + e
        if d[k] == 0.0:
            if not (lo <= p <= hi):
                return True
            continue
        dk = Fraction(d[k])
        a, b = (lo - p) / dk, (hi - p) / dk
        if a > b:
            a, b = b, a
        t0 = a if t0 is None or a > t0 else t0
        t1 = b if t1 is None or b < t1 else t1
    return not (t0 is None or t1 is None or t0 <= t1)


@functools.lru_cache(maxsize=None)
def slab_cases(seed=20261):
    """(records, family name per record, exact answer per record, clear-miss flag per record) of the finite slab families."""
    rng = np.random.default_rng(seed)
    recs, fam = [], []
    for name, (gen, n) in SLAB_FAMILIES.items():
        recs.append(gen(rng, n))
        fam += [name] * n
    rec = np.concatenate(recs)
    assert np.isfinite(rec[:, :10]).all() and np.isfinite(rec[:, 12:]).all()
    assert np.array_equal(f32(rec[:, 12:]), rec[:, 12:]), "boxes are f32 values"
    exact = np.array([slab_exact(r) for r in rec])
    miss = np.array([(not x) and slab_ordinary(r) and slab_clear_miss(r) for r, x in zip(rec, exact)])
    return rec, np.array(fam), exact, miss


def slab_big_frames(rec):
    """|of|_inf + R against 1e30, per record, in f64 on the code's f32 operands: (certainly at or above, possibly at or above).  The frames
    at or above take every box and are the only ones the soundness property leaves out; a factor 1 +- 2^-20 around the threshold,
    where the code's own f32 sum decides, belongs to neither side."""
    with np.errstate(all="ignore"):
        m = np.abs(f32(rec[:, 4:7] - rec[:, 0:3])).max(axis=1) + f32(rec[:, 3])
    return m >= 1e30 * (1 + 2.0 ** -20), ~(m < 1e30 * (1 - 2.0 ** -20))


@functools.lru_cache(maxsize=None)
def slab_unbounded_cases(seed=20262):
    """Records that must take every box, with intervals that hold 0: (records, label per record).
    big_frame: |of|_inf + R >= 1e30 (a huge radius, or an origin that far away).  nan_origin: a NaN origin component.
    nan_dir / inf_dir: a NaN or +-inf direction component; the finite axes miss, graze or cross the box as `aimed` made them."""
    rng = np.random.default_rng(seed)
    out, lab = [], []
    n = 1500
    c, R, of, d, lo, hi, _ = _aimed(rng, n, rad_exp=(-3.0, 28.0))
    big = rng.random(n) < 0.5
    R = np.where(big, 10.0 ** rng.uniform(30.1, 37.0, n), R)
    k = rng.integers(0, 3, n)
    of[~big, k[~big]] = (10.0 ** rng.uniform(30.1, 37.0, n) * rng.choice([-1.0, 1.0], n))[~big]
    c[~big] = 0.0
    out.append(_records(c, R, of, d, 0.0, INF, lo, hi))
    lab += ["big_frame"] * n
    for label, values in (("nan_origin", (math.nan,)), ("nan_dir", (math.nan,)), ("inf_dir", (INF, -INF))):
        c, R, of, d, lo, hi, tp = _aimed(rng, n, rad_exp=(-3.0, 12.0))
        miss = rng.random(n) < 0.5    # half of them: finite axes that miss the box by a wide margin
        of[miss] += (R * rng.uniform(2.0, 20.0, n))[miss, None] * rng.choice([-1.0, 1.0], (n, 3))[miss]
        rec = _records(c, R, of, d, 0.0, np.where(rng.random(n) < 0.5, INF, tp * 2.0), lo, hi)
        col = (4 if label == "nan_origin" else 7) + rng.integers(0, 3, n)
        rec[np.arange(n), col] = rng.choice(values, n)
        two = rng.random(n) < 0.1     # and a second one now and then
        rec[two, (4 if label == "nan_origin" else 7) + rng.integers(0, 3, n)[two]] = values[0]
        out.append(rec)
        lab += [label] * n
    return np.concatenate(out), np.array(lab)


# --------------------------------------------------------------------------------------------------------------- point
# fr[4], o[3], d[3], t_hit, lo[3], hi[3]
def point_exact(rec):
    """o + t_hit d - c lies in [lo, hi], exactly."""
    t = Fraction(rec[10])
    for k in range(3):
        x = Fraction(rec[4 + k]) + t * Fraction(rec[7 + k]) - Fraction(rec[k])
        if not (Fraction(rec[11 + k]) <= x <= Fraction(rec[14 + k])):
            return False
    return True


@functools.lru_cache(maxsize=None)
def point_cases(seed=20263, n=20000):
    """(records, exact answers): hit points on faces, edges and corners of the box, inside it, and nudged out of it by 0 .. 1e-3 of its
    frame's radius; frames of every radius, origins up to 1e4 radii away."""
    rng = np.random.default_rng(seed)
    c, R, of, d, lo, hi, tp = _aimed(rng, n, rad_exp=(-3.0, 28.0), dist_exp=(-2.0, 4.0))
    t = tp * (1.0 + rng.choice([0.0, 1e-16, 1e-13, 1e-9, 1e-6, 1e-3], n) * rng.choice([-1.0, 1.0], n))
    inside = rng.random(n) < 0.25   # a quarter: the ray is aimed at an interior point instead
    q = lo + rng.uniform(0, 1, (n, 3)) * (hi - lo)
    d[inside] = ((q - of) / np.maximum(t, 1e-300)[:, None])[inside]
    rec = np.empty((n, 17))
    rec[:, 0:3], rec[:, 3], rec[:, 4:7], rec[:, 7:10], rec[:, 10], rec[:, 11:14], rec[:, 14:17] = c, R, c + of, d, t, lo, hi
    assert np.isfinite(rec).all()
    return rec, np.array([point_exact(r) for r in rec])


@functools.lru_cache(maxsize=None)
def point_unbounded_cases(seed=20264, n=2000):
    """Records whose point is NaN or infinite, or whose frame is too big for f32 (|X| + |o| + R >= 1e30): every box "contains" them."""
    rng = np.random.default_rng(seed)
    rec = point_cases()[0][rng.integers(0, 20000, n)].copy()
    kind = rng.integers(0, 4, n)
    rows = np.arange(n)
    rec[kind == 0, 10] = rng.choice([math.nan, INF, -INF], n)[kind == 0]                       # t_hit
    col = rng.integers(4, 10, n)
    sel = kind == 1
    rec[rows[sel], col[sel]] = rng.choice([math.nan, INF, -INF], n)[sel]                          # an origin or direction component
    rec[kind == 2, 3] = 10.0 ** rng.uniform(30.1, 37.0, n)[kind == 2]                             # the radius
    sel = kind == 3                                                                               # an origin 1e30 .. 1e37 away
    rec[rows[sel], 4 + rng.integers(0, 3, n)[sel]] = (10.0 ** rng.uniform(30.1, 37.0, n) * rng.choice([-1.0, 1.0], n))[sel]
    rec[sel, 0:3] = 0.0
    rec[sel, 7:10] = 0.0
    return rec


# ---------------------------------------------------------------------------------------------------------------- gate
# lo[3], hi[3], o[3], d[3]
def reference_box_intersects(lo, hi, o, d):
    """BoundingBox::intersects (src/bounding_box.rs:80-106) restated: check_axis with the |d| >= EPSILON rule, f64::max / min that
    ignore a NaN operand, `t_min <= t_max`."""
    EPS = 0.00001

    def axis(origin, direction, mn, mx):
        a_num, b_num = mn - origin, mx - origin
        if abs(direction) >= EPS:
            a, b = a_num / direction, b_num / direction
        else:
            a = a_num * math.inf if a_num != 0.0 else math.nan
            b = b_num * math.inf if b_num != 0.0 else math.nan
        return (b, a) if a > b else (a, b)

    def fmax(a, b):
        return b if a != a else (a if b != b else max(a, b))

    def fmin(a, b):
        return b if a != a else (a if b != b else min(a, b))

    xs, ys, zs = (axis(o[k], d[k], lo[k], hi[k]) for k in range(3))
    return fmax(fmax(xs[0], ys[0]), zs[0]) <= fmin(fmin(xs[1], ys[1]), zs[1])


def gate_rays(n=100000, seed=11):
    """The adversarial rays of tests/test_group_gate.py, one (lo, hi, o, d) at a time: through corners, edges and faces of boxes, nudged by
    0 ... 1e-5, axis-parallel, with components around EPSILON."""
    rng = np.random.default_rng(seed)
    for trial in range(n):
        c = rng.uniform(-20, 20, 3)
        size = rng.uniform(0.01, 10, 3)
        lo, hi = c - size, c + size
        pick = rng.integers(0, 3, 3)
        p = np.where(pick == 0, lo, np.where(pick == 1, hi, lo + rng.uniform(0, 1, 3) * 2 * size))
        o = c + rng.normal(size=3) * rng.uniform(1, 50)
        d = p - o
        d /= np.linalg.norm(d)
        d = d + rng.choice([0.0, 1e-16, 1e-13, 1e-10, 1e-8, 3e-8, 1e-7, 3e-7, 1e-6, 1e-5]) * rng.normal(size=3)
        d /= np.linalg.norm(d)
        m = trial % 8
        if m == 0:
            d[rng.integers(0, 3)] = rng.uniform(-3e-5, 3e-5)
        elif m == 1:
            k = rng.integers(0, 3)
            d[k] = 0.0
            o[k] = rng.choice([lo[k], hi[k], lo[k] + rng.uniform(0, 1) * 2 * size[k]])
        yield lo, hi, o, d


def _reference_gate(rec):
    with np.errstate(all="ignore"):
        return np.array([reference_box_intersects(r[0:3], r[3:6], r[6:9], r[9:12]) for r in rec.tolist()])


@functools.lru_cache(maxsize=None)
def gate_cases():
    """(records, the reference's answers): the 100 000 rays above, 4 000 of them again with a direction component between EPSILON and
    2 EPSILON (where the pre-test hands over to the reference's expression), and 4 000 with an infinite or NaN box bound."""
    rec = np.array([np.concatenate(r) for r in gate_rays()])
    rng = np.random.default_rng(12)
    a = rec[rng.integers(0, len(rec), 4000)].copy()
    a[np.arange(4000), 9 + rng.integers(0, 3, 4000)] = rng.uniform(EPSILON, 2 * EPSILON, 4000) * rng.choice([-1.0, 1.0], 4000)
    a[:200, 9] = np.array([EPSILON, 2 * EPSILON, np.nextafter(2 * EPSILON, 0), np.nextafter(EPSILON, 1)] * 50)
    b = rec[rng.integers(0, len(rec), 4000)].copy()
    col = rng.integers(0, 6, 4000)
    val = rng.choice([INF, -INF, math.nan], 4000)
    val = np.where(rng.random(4000) < 0.6, np.where(col < 3, -INF, INF), val)   # mostly the unbounded boxes scenes do have
    b[np.arange(4000), col] = val
    b[::7, 0:3], b[::7, 3:6] = -INF, INF                                        # a plane's group: everything
    rec = np.concatenate([rec, a, b])
    return rec, _reference_gate(rec)


# --------------------------------------------------------------------------------------------------------------- plane
# oy, dy, mode (3 = containers)
PLANE_MAGNITUDES = (0.0, 5e-324, 1e-310, 1e-300, 1e-291, 9.999e-291, 1e-290, 1.001e-290, 1e-289, 1e-280, 1e-200, 1e-100, 1e-5, 1.0, 7.0, 1e10, 1e16,
                    9.999e16, 1e17, 1.001e17, 1e18, 1e100, 1e290, 1e300, 1.7e308, INF, math.nan)


@functools.lru_cache(maxsize=None)
def plane_cases(seed=20265, n=40000):
    """(records, q): operands from every decade that matters to t = -oy / dy -- zeros of both signs, subnormals, around 1e-290 and 1e17,
    huge, infinite, NaN -- with random mantissas, all four pass modes; q = the correctly rounded f64 quotient -oy / dy."""
    rng = np.random.default_rng(seed)
    mant = np.where(rng.random((n, 2)) < 0.5, 1.0, rng.uniform(1.0, 10.0, (n, 2)))
    with np.errstate(all="ignore"):
        v = rng.choice(PLANE_MAGNITUDES, (n, 2)) * mant * rng.choice([-1.0, 1.0], (n, 2))
        rec = np.column_stack([v, rng.integers(0, 4, n).astype(float)])
        q = -rec[:, 0] / rec[:, 1]
    return rec, q


# -------------------------------------------------------------------------------------------------------------- behind
# point[3], light[3], unit normal[3]
def reference_light_dot_normal(rec):
    """Shape::lighting's `light_vector . normal` in the reference's operation order (src/linalg/vector.rs): v = light - point,
    |v| = sqrt(vx^2 + vy^2 + vz^2), (vx / |v|) nx + (vy / |v|) ny + (vz / |v|) nz, each operation rounded to f64.  Returns (dot, |v|)."""
    with np.errstate(all="ignore"):
        v = rec[:, 3:6] - rec[:, 0:3]
        mag = np.sqrt(v[:, 0] * v[:, 0] + v[:, 1] * v[:, 1] + v[:, 2] * v[:, 2])
        u = v / mag[:, None]
        return u[:, 0] * rec[:, 6] + u[:, 1] * rec[:, 7] + u[:, 2] * rec[:, 8], mag


@functools.lru_cache(maxsize=None)
def behind_cases(seed=20266, n=24000):
    """(records, dot, |v|): lights at 1e-6 .. 1e32 units from the point, in and around the tangent plane -- light . normal from 0 and
    +-1e-17 through the predicate's 1e-6 margin to +-1 --, points up to 1e6 from the origin, unit normals random and axis-aligned; one
    record in twelve has a NaN or infinite operand."""
    rng = np.random.default_rng(seed)
    nrm = rng.normal(size=(n, 3))
    axis = rng.random(n) < 0.2
    nrm[axis] = np.eye(3)[rng.integers(0, 3, n)][axis] * rng.choice([-1.0, 1.0], n)[axis, None]
    nrm /= np.linalg.norm(nrm, axis=1, keepdims=True)
    tan = np.cross(nrm, rng.normal(size=(n, 3)))
    tan /= np.linalg.norm(tan, axis=1, keepdims=True)
    s = rng.choice([0.0, 1e-17, 1e-16, 1e-12, 1e-9, 1e-7, 5e-7, 9.9e-7, 1e-6, 1.01e-6, 2e-6, 1e-5, 1e-3, 2e-3, 0.1, 1.0], n) * rng.choice([-1.0, 1.0], n)
    length = 10.0 ** np.where(rng.random(n) < 0.8, rng.uniform(-6.0, 6.0, n), rng.uniform(6.0, 32.0, n))
    v = (tan * np.sqrt(np.maximum(0.0, 1.0 - s * s))[:, None] + nrm * s[:, None]) * length[:, None]
    p = rng.normal(size=(n, 3)) * (10.0 ** rng.uniform(-3.0, 6.0, n) * (rng.random(n) < 0.8))[:, None]
    rec = np.column_stack([p, p + v, nrm])
    odd = np.arange(0, n, 12)
    rec[odd, rng.integers(0, 9, len(odd))] = rng.choice([math.nan, math.nan, INF, -INF], len(odd))
    dot, mag = reference_light_dot_normal(rec)
    return rec, dot, mag
