"""Inputs, float64 statement, fp32 model and census of the projected-gradient step under the L2 budget
(pcfa_pgd_l2_step, pcfa_amd/csrc/attack_math.hip; attack_FGSM.pgd_l2_attack_step).  Not a test; no GPU.
tests/test_pgd_l2_step_gpu.py judges the kernel with it, tests/test_pgd_l2_host_cpu.py checks it on the CPU first.

A case of n elements is the first n entries of ONE table per KIND (the head of every table is crafted, the rest seeded):

    mixed      clean images at 0, at 1 and inside; iterates x within a few 1e-3 of them (an attack under way), a fifth of
               them still at the image; gradients +-0, tiny (1e-30 N(0,1)) and 1e6 N(0,1)
    nan        mixed with ONE NaN gradient (g2[0])          -> G is NaN, a = 0
    inf        mixed with ONE +Inf gradient (g1[0])         -> G is Inf, a = 0
    zero       every gradient +-0, and one NaN pixel x1[1]  -> G is 0, a = 0; the NaN pixel stays one, E is NaN, s = 1
    opposed    g2 = -g1: under `joint` 0.5f * (g1 + g2) is 0 everywhere -> G = 0; without `joint` an ordinary step

The float64 statement (`statement64`) is section 1 of the feature's description evaluated in float64 on the fp32 inputs
with NO intermediate rounding; `bounds` is what the kernel's fp32 roundings may add to it, element by element:

    u = 2^-24, t = 2^-149 (a product may be subnormal).  m = a g, the move.
    a       one rounding of a double expression whose only inexact input is G (relative error <= depth 2^-53 << u):
            a32 = a (1 + da), |da| <= 1.01 u
    m^      fl(a32 g): |m^ - m| <= 2.02 u |m| + t
    y^      clamp(fl(x - m^)): |y^ - y| <= ty = 2.03 u |m| + 1.01 u |x - m| + t        (the clamp moves nothing apart)
    e^      fl(y^ - img): |e^ - e| <= te = 1.01 ty + u |e|
    s = 1:  x and d carry ty and te.
    s < 1:  E^ = sum e^^2 in double: |E^ - E| <= dE = sum te (2 |e| + te) + depth 2^-53 E;  r = sqrt(E / N), s = b / r:
            s32 = s (1 + ds), |ds| <= ts = 1.01 u + 0.51 dE / E
    p^      fl(s32 e^): |p^ - s e| <= tp = 1.01 (|s e| (ts + u) + s te) + t
    x^      clamp(fl(img + p^)): |x^ - x| <= tx = 1.01 tp + u |img + s e|
    d^      fl(x^ - img): |d^ - d| <= td = 1.01 tx + u |d|

A bound of this kind cannot tell a contracted `x - a g` (one rounding) from the stated two roundings: the contracted result
is the correctly rounded one and lies inside every sound bound.  What does tell them apart is `model32`, the stated fp32
sequence itself, which the kernel has to equal bit for bit with the a and s it reports (tests/test_pgd_l2_step_gpu.py);
tests/test_pgd_l2_host_cpu.py shows on the CPU that the contracted model differs from it on the crafted inputs."""
import math

import numpy as np

U = 2.0 ** -24
T = 2.0 ** -149
SETTINGS = ((0.00025, 0.005), (0.002, 0.003), (0.3, 0.005), (0.01, 1e-4))
KINDS = ("mixed", "nan", "inf", "zero", "opposed")
SMALL = (1, 3, 4, 5, 255, 256, 257, 1025)
WORKGROUP = 256                 # threads per workgroup of the three kernels; a thread takes one quad (4 floats) per trip
SPREAD = 0.0035                 # rms of the iterates' distance from the clean images before the clamp

_HEAD_IMG = (0.0, 1.0, 0.5, 0.0, 1.0, 1.0, 0.0, 0.25)
_HEAD_G = (1.0e6, 0.0, 1.0e-30, -0.0, -2.0e6, -1.0e-30, 5.0e5, -1.5e6)


def f32(v):
    with np.errstate(over="ignore"):
        return float(np.float32(v))


def budget(bound):
    """The cap every output has to satisfy, measured in float64: b (1 + 2u) + 2u with b the fp32 value of the bound
    (s is one rounding of a double quotient; img + s e and x - img round values of at most 1)."""
    return f32(bound) * (1 + 2 * U) + 2 * U


_BASE = {}


def _base(n):
    if "t" not in _BASE or len(_BASE["t"][0]) < n:
        m = max(n, 4096)
        rng = np.random.RandomState(20250217)
        out = []
        for which in range(2):
            img = rng.uniform(0, 1, m)
            pick = rng.uniform(0, 1, m)
            img[pick < 0.2] = 0.0
            img[pick > 0.8] = 1.0
            img[:len(_HEAD_IMG)] = np.roll(_HEAD_IMG, which)
            x = np.clip(img + SPREAD * rng.standard_normal(m), 0, 1)
            still = rng.uniform(0, 1, m) < 0.2
            x[still] = img[still]
            g = 1.0e6 * rng.standard_normal(m)
            pick = rng.uniform(0, 1, m)
            g[pick < 0.1] = np.where(rng.uniform(0, 1, m) < 0.5, 0.0, -0.0)[pick < 0.1]
            g[pick > 0.9] = (1.0e-30 * rng.standard_normal(m))[pick > 0.9]
            g[:len(_HEAD_G)] = np.roll(_HEAD_G, 3 * which)
            out.append((x.astype(np.float32), g.astype(np.float32), img.astype(np.float32)))
        (x1, g1, i1), (x2, g2, i2) = out
        _BASE["t"] = (x1, x2, g1, g2, i1, i2)
    return _BASE["t"]


def table(n, kind="mixed", gscale=1.0):
    """(x1, x2, g1, g2, img1, img2): the first n entries of the table of `kind` as float32 numpy arrays (copies)."""
    x1, x2, g1, g2, i1, i2 = (a[:n].copy() for a in _base(n))
    if gscale != 1.0:
        g1, g2 = (g1 * np.float32(gscale)).astype(np.float32), (g2 * np.float32(gscale)).astype(np.float32)
    if kind == "nan":
        g2[0] = np.nan
    elif kind == "inf":
        g1[0] = np.inf
    elif kind == "zero":
        g1, g2 = np.copysign(np.float32(0), g1), np.copysign(np.float32(0), g2)
        if n > 1:
            x1[1] = np.nan
    elif kind == "opposed":
        g2 = -g1
    elif kind != "mixed":
        raise ValueError(kind)
    return x1, x2, g1, g2, i1, i2


def _joint32(g1, g2, joint):
    if not joint:
        return g1, g2
    with np.errstate(invalid="ignore", over="ignore"):
        g = (np.float32(0.5) * (g1 + g2)).astype(np.float32)        # the fp32 sum is rounded first
    return g, g


def _fsum_sq(a, b):
    a, b = a.astype(np.float64), b.astype(np.float64)
    with np.errstate(invalid="ignore", over="ignore"):
        sq = np.concatenate([a * a, b * b])
    if not np.isfinite(sq).all():
        return float(np.sum(sq))
    return math.fsum(sq.tolist())


def step_factor(G, n_total, eps):
    """(a in double, a as the fp32 the step uses): 0 where G is 0, NaN or Inf or the fp32 value is not finite."""
    if not 0.0 < G < math.inf:
        return 0.0, 0.0
    a = f32(eps) * math.sqrt(n_total / G)
    return (a, f32(a)) if math.isfinite(f32(a)) else (0.0, 0.0)


def sum_depth(n, max_threads):
    """The longest chain of double additions behind one of the kernel's sums of 2n squares: a thread's quads (8 squares a
    trip), 6 shuffles, 3 waves, then the partials lane-strided, 6 shuffles, 3 waves."""
    quads = (n + 3) // 4
    blocks = min((quads + WORKGROUP - 1) // WORKGROUP, max_threads // WORKGROUP)
    trips = (quads + blocks * WORKGROUP - 1) // (blocks * WORKGROUP)
    return 8 * trips + 9 + (blocks + WORKGROUP - 1) // WORKGROUP + 9


def statement64(x1, x2, g1, g2, i1, i2, eps, bound, joint):
    """Section 1 in float64 without intermediate roundings.  Returns a dict: x1, x2, d1, d2 (float64 arrays), G, a, E, s,
    r, and y1, y2, e1, e2, m1, m2 (the step before the projection, the moves)."""
    eps, bound = f32(eps), f32(bound)
    g1, g2 = _joint32(g1, g2, joint)
    n_total = float(2 * len(x1))
    G = _fsum_sq(g1, g2)
    a, _ = step_factor(G, n_total, eps)
    X = [x1.astype(np.float64), x2.astype(np.float64)]
    I = [i1.astype(np.float64), i2.astype(np.float64)]
    with np.errstate(invalid="ignore", over="ignore"):
        M = [a * g.astype(np.float64) if a != 0.0 else np.zeros(len(g)) for g in (g1, g2)]
    Y = [np.clip(x - m, 0.0, 1.0) for x, m in zip(X, M)]
    Ee = [y - i for y, i in zip(Y, I)]
    E = _fsum_sq(*Ee)
    s, r = 1.0, float("nan")
    if E < math.inf:
        r = math.sqrt(E / n_total)
        if r > bound:
            s = bound / r
    if s != 1.0:
        P = [np.clip(i + s * e, 0.0, 1.0) for i, e in zip(I, Ee)]
        D = [p - i for p, i in zip(P, I)]
    else:
        P, D = Y, Ee
    return {"x1": P[0], "x2": P[1], "d1": D[0], "d2": D[1], "G": G, "a": a, "E": E, "s": s, "r": r, "y1": Y[0], "y2": Y[1],
            "e1": Ee[0], "e2": Ee[1], "m1": M[0], "m2": M[1], "x_in": X, "img": I}


def bounds(ref, depth):
    """(bx1, bx2, bd1, bd2, dE): the element bounds of the module docstring for the statement `ref`; NaN where the
    statement is NaN (there the output has to be NaN).  dE: what the kernel's E may differ by from the statement's."""
    eps53 = depth * 2.0 ** -53
    ty = [2.03 * U * np.abs(m) + 1.01 * U * np.abs(x - m) + T for x, m in zip(ref["x_in"], (ref["m1"], ref["m2"]))]
    te = [1.01 * t + U * np.abs(e) for t, e in zip(ty, (ref["e1"], ref["e2"]))]
    E = ref["E"]
    dE = float("nan")
    if math.isfinite(E):
        dE = sum(float(np.sum(t * (2 * np.abs(e) + t))) for t, e in zip(te, (ref["e1"], ref["e2"]))) + eps53 * E
    if ref["s"] == 1.0:
        return ty[0], ty[1], te[0], te[1], dE
    s = ref["s"]
    ts = 1.01 * U + 0.51 * dE / E
    out_x, out_d = [], []
    for t, e, img, d in zip(te, (ref["e1"], ref["e2"]), ref["img"], (ref["d1"], ref["d2"])):
        tp = 1.01 * (np.abs(s * e) * (ts + U) + s * t) + T
        tx = 1.01 * tp + U * np.abs(img + s * e)
        out_x.append(tx)
        out_d.append(1.01 * tx + U * np.abs(d))
    return out_x[0], out_x[1], out_d[0], out_d[1], dE


def worst_excess(got, ref, bnd):
    """max over the elements of |got - ref| / bound (NaN must meet NaN; a NaN on one side only counts as inf)."""
    got = np.asarray(got, np.float64)
    nan_ref, nan_got = np.isnan(ref), np.isnan(got)
    if (nan_ref != nan_got).any():
        return math.inf
    ok = ~nan_ref
    if not ok.any():
        return 0.0
    return float(np.max(np.abs(got[ok] - ref[ok]) / bnd[ok]))


def model32(x1, x2, g1, g2, i1, i2, eps, bound, joint, a=None, s=None, g_from_g1=False, contract=False):
    """The stated sequence in fp32 (numpy: every operation rounds once, nothing is contracted).  a / s: use these fp32
    values (as read back from the kernel's workspace) instead of forming them.  The two wrong models of the tests:
    g_from_g1 forms G from g1 alone; contract rounds x - a g once (an fma).
    Returns (x1', x2', d1, d2, (G, a, E, s)); sums in double, numpy's order."""
    eps, bound = f32(eps), f32(bound)
    g1, g2 = _joint32(g1, g2, joint)
    n_total = float(2 * len(x1))
    G = _fsum_sq(g1, np.zeros(0, np.float32) if g_from_g1 else g2)
    if a is None:
        _, a = step_factor(G, n_total, eps)
    a32 = np.float32(a)
    with np.errstate(invalid="ignore", over="ignore", under="ignore"):
        if a == 0.0:
            y = [np.clip(x, np.float32(0), np.float32(1)) for x in (x1, x2)]
        elif contract:
            y = [np.clip((x.astype(np.float64) - float(a32) * g.astype(np.float64)).astype(np.float32), np.float32(0),
                         np.float32(1)) for x, g in ((x1, g1), (x2, g2))]
        else:
            y = [np.clip(x - a32 * g, np.float32(0), np.float32(1)) for x, g in ((x1, g1), (x2, g2))]
        e = [yy - img for yy, img in zip(y, (i1, i2))]
        E = _fsum_sq(*e)
        if s is None:
            s = 1.0
            if E < math.inf:
                r = math.sqrt(E / n_total)
                if r > bound:
                    s = f32(bound / r)
        if s == 1.0:
            return y[0], y[1], e[0], e[1], (G, float(a), E, 1.0)
        s32 = np.float32(s)
        p = [np.clip(img + s32 * ee, np.float32(0), np.float32(1)) for img, ee in zip((i1, i2), e)]
        d = [pp - img for pp, img in zip(p, (i1, i2))]
    return p[0], p[1], d[0], d[1], (G, float(a), E, float(s))


def norm64(d1, d2):
    """two_norm_avg_delta in float64 (NaN elements left out: they were NaN pixels of x)."""
    d = np.concatenate([np.asarray(d1, np.float64), np.asarray(d2, np.float64)])
    ok = ~np.isnan(d)
    return math.sqrt(math.fsum((d[ok] * d[ok]).tolist()) / len(d))


def census(sizes=SMALL, kinds=KINDS):
    """(branch -> number of cases, the smallest |r / b - 1| over the cases with a finite r): every (size, kind, setting,
    joint) once, from the float64 statement.  Branches: "s = 1", "s < 1", "a = 0"."""
    counts = {"s = 1": 0, "s < 1": 0, "a = 0": 0}
    margin = math.inf
    for n in sizes:
        for kind in kinds:
            for eps, bound in SETTINGS:
                for joint in (0, 1):
                    ref = statement64(*table(n, kind), eps, bound, joint)
                    counts["s < 1" if ref["s"] < 1.0 else "s = 1"] += 1
                    counts["a = 0"] += ref["a"] == 0.0
                    if math.isfinite(ref["r"]) and ref["r"] > 0:
                        margin = min(margin, abs(ref["r"] / f32(bound) - 1))
    return counts, margin
