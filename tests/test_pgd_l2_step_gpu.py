"""pcfa_pgd_l2_step (pcfa_amd/csrc/attack_math.hip) through the C-ABI on fenced buffers: the projected-gradient step under
the averaged-L2 budget against its float64 statement and against the stated fp32 sequence (tests/pgd_cases.py), at every
size at which the launch changes (below / at / past one quad, one workgroup, two partials, a second trip of the grid-stride
loop), aligned pointers, all pointers one float off, each single pointer off, both `joint` modes, four (epsilon, bound)
settings that take both branches of s, and the crafted kinds (a NaN or Inf gradient, no gradient, opposed gradients).

Judged per case:
  * x1, x2, d1, d2 against the float64 statement within the ELEMENT BOUND of tests/pgd_cases.py (one rounding of a, the
    product, the difference, the clamp, one rounding of s, the product, the sum, the difference -- derived there, checked
    on the CPU in tests/test_pgd_l2_host_cpu.py before it is used here); a within 1.01 u, s within its derived ts;
  * G against the exact sum of the fp32 squares and E against the exact sum of the squares of the fp32 e, both within
    depth * 2^-53 (pgd_cases.sum_depth: the longest chain of double additions in the kernel's stated order), not fp32;
  * x and d against the stated fp32 sequence in torch on the device, with the a and s read back from the workspace,
    BIT FOR BIT -- in the s = 1 branch that is clamp(x - a g, 0, 1) and x' - img untouched by the third launch;
  * the properties: 0 <= x <= 1, d == x - img bitwise, two_norm_avg_delta(d1, d2) <= b (1 + 2u) + 2u in float64;
  * inputs and fences untouched, every output element written, a second call gives the same bits."""
import ctypes
import functools
import math

import numpy as np
import pytest
import torch

from tests import fenced, pgd_cases
from tests.fenced import DEV, NAN_BITS, PCFA_ERR_INVALID_ARG, SENTINEL, Fenced
from tests.pgd_cases import SETTINGS, SMALL, U, WORKGROUP

pytestmark = pytest.mark.gpu

WS_FENCE = 64
WS_FILL = 0x7FF8BEEF7FF8BEEF        # a quiet NaN as a double


def _lib():
    from pcfa_amd import _hip
    return _hip.load()


def _max_threads():
    return _lib().pcfa_pgd_l2_max_threads()


def _second_trip():
    """The first n at which a thread runs its loop twice: one quad more than all threads of the largest launch take."""
    return 4 * _max_threads() + 1


def _bits(t):
    return t.contiguous().view(torch.int32)


class _Call:
    """Eight fenced operands of n floats, `shifts[i]` floats off 16-byte alignment -- x1, x2 (in / out), g1, g2, img1, img2
    (inputs, NaN fill), d1, d2 (outputs, sentinel fill) -- and a fenced workspace."""

    def __init__(self, n, shifts, kind="mixed"):
        self.n = n
        self.host = pgd_cases.table(n, kind)
        fills = (NAN_BITS,) * 6 + (SENTINEL, SENTINEL)
        self.ops = [Fenced((n,), (1,), fill, shift=s) for fill, s in zip(fills, shifts)]
        for op, src in zip(self.ops[:6], self.host):
            op.write(torch.from_numpy(src))
        self.ws_words = _lib().pcfa_pgd_l2_workspace_bytes() // 8
        self.ws = torch.full((self.ws_words + 2 * WS_FENCE,), WS_FILL, dtype=torch.int64, device=DEV)

    def reset(self):
        self.ops[0].write(torch.from_numpy(self.host[0]))
        self.ops[1].write(torch.from_numpy(self.host[1]))
        for op in self.ops[6:]:
            op.buf.view(torch.int32).fill_(SENTINEL)
            op.bits0 = op.buf.view(torch.int32).clone()
        self.ws.fill_(WS_FILL)

    def run(self, joint, eps, bound, n=None, null=None, off=None, ws_off=0):
        ptrs = [op.ptr() for op in self.ops]
        if null is not None and null < 8:
            ptrs[null] = ctypes.c_void_p(0)
        if off is not None:
            ptrs[off] = ctypes.c_void_p(ptrs[off].value + 2)
        ws = ctypes.c_void_p(0 if null == 8 else self.ws.data_ptr() + 8 * WS_FENCE + ws_off)
        status = _lib().pcfa_pgd_l2_step(*ptrs, ctypes.c_float(eps), ctypes.c_float(bound), int(joint),
                                         self.n if n is None else n, ws, fenced.stream())
        torch.cuda.synchronize()
        return status

    def outputs(self):
        return [self.ops[i].view().clone() for i in (0, 1, 6, 7)]

    def scalars(self):
        return self.ws[WS_FENCE:WS_FENCE + 4].view(torch.float64).tolist()

    def ws_fence_intact(self):
        return bool((self.ws[:WS_FENCE] == WS_FILL).all()) and bool((self.ws[WS_FENCE + self.ws_words:] == WS_FILL).all())

    def all_bits(self):
        return [op.buf.view(torch.int32).clone() for op in self.ops] + [self.ws.clone()]


@functools.lru_cache(maxsize=4)
def _reference(n, kind, eps, bound, joint):
    """The float64 statement and its element bounds, computed once per case and shared (never modified)."""
    ref = pgd_cases.statement64(*pgd_cases.table(n, kind), eps, bound, joint)
    return ref, pgd_cases.bounds(ref, pgd_cases.sum_depth(n, _max_threads()))


def torch_sequence(x1, x2, g1, g2, i1, i2, a, s, joint):
    """The stated fp32 sequence in torch on the device of its inputs, one rounding per operation, with the a and s given."""
    if joint:
        g1 = g2 = 0.5 * (g1 + g2)
    if a == 0.0:
        y1, y2 = torch.clamp(x1, 0., 1.), torch.clamp(x2, 0., 1.)
    else:
        m1, m2 = a * g1, a * g2
        y1, y2 = torch.clamp(x1 - m1, 0., 1.), torch.clamp(x2 - m2, 0., 1.)
    e1, e2 = y1 - i1, y2 - i2
    if s == 1.0:
        return (y1, y2, e1, e2), (e1, e2)
    q1, q2 = s * e1, s * e2
    p1, p2 = torch.clamp(i1 + q1, 0., 1.), torch.clamp(i2 + q2, 0., 1.)
    return (p1, p2, p1 - i1, p2 - i2), (e1, e2)


def _close_sum(got, exact, depth):
    if math.isnan(exact) or math.isinf(exact) or exact == 0.0:
        return (math.isnan(got) and math.isnan(exact)) or got == exact
    return abs(got - exact) <= (depth + 1) * 2.0 ** -53 * exact


def _check(n, shifts, joint, kind, eps, bound):
    tag = (n, shifts, joint, kind, eps, bound)
    c = _Call(n, shifts, kind)
    assert all((op.ptr().value % 16 == 0) == (s % 4 == 0) for op, s in zip(c.ops, shifts))
    dev = [torch.from_numpy(a).to(DEV) for a in c.host]
    inputs0 = [op.buf.view(torch.int32).clone() for op in c.ops[2:6]]
    assert c.run(joint, eps, bound) == 0
    got = c.outputs()
    G, a, E, s = c.scalars()
    scalar_bits = c.ws[WS_FENCE:WS_FENCE + 4].clone()
    print("case %s: G %r a %r E %r s %r" % (tag, G, a, E, s))
    ref, (bx1, bx2, bd1, bd2, dE) = _reference(n, kind, eps, bound, joint)
    depth = pgd_cases.sum_depth(n, _max_threads())

    # ---- the scalars
    assert _close_sum(G, ref["G"], depth), (tag, G, ref["G"])
    if ref["a"] == 0.0:
        assert a == 0.0, (tag, a)
    else:
        assert a == pgd_cases.f32(a) and abs(a - ref["a"]) <= 1.01 * U * ref["a"], (tag, a, ref["a"])
    assert (s < 1.0) == (ref["s"] < 1.0) and s == pgd_cases.f32(s), (tag, s, ref["s"])
    if math.isfinite(ref["E"]):
        assert abs(E - ref["E"]) <= dE, (tag, E, ref["E"], dE)
        if s < 1.0:
            assert abs(s - ref["s"]) <= (1.01 * U + 0.51 * dE / ref["E"]) * ref["s"], (tag, s, ref["s"])
    else:
        assert math.isnan(E) and s == 1.0, (tag, E, s)

    # ---- the elements against the float64 statement
    for name, g, b in zip(("x1", "x2", "d1", "d2"), got, (bx1, bx2, bd1, bd2)):
        worst = pgd_cases.worst_excess(g.cpu().numpy(), ref[name], b)
        print("   %s: worst |got - f64| / bound = %.3f" % (name, worst))
        assert worst <= 1.0, (tag, name, worst)

    # ---- bit for bit against the stated fp32 sequence with the a and s read back; E against the exact sum of its e
    want, (e1, e2) = torch_sequence(*dev, a, s, joint)
    for name, g, w in zip(("x1", "x2", "d1", "d2"), got, want):
        same = (_bits(g) == _bits(w)) | (torch.isnan(g) & torch.isnan(w))
        assert bool(same.all()), (tag, name, int((~same).sum()), int((~same).nonzero()[0]))
    e = torch.cat([e1, e2]).double()
    if math.isfinite(ref["E"]):
        assert _close_sum(E, math.fsum((e * e).cpu().tolist()), depth), (tag, E)

    # ---- the properties, in float64 from the outputs
    x_in_nan = [torch.isnan(t) for t in dev[:2]]
    for g, was_nan in zip(got[:2], x_in_nan):
        assert torch.equal(torch.isnan(g), was_nan), tag            # no NaN appears that was not in x
        ok = ~was_nan
        assert bool(((g[ok] >= 0) & (g[ok] <= 1)).all()), tag
    for x, img, d in ((got[0], dev[4], got[2]), (got[1], dev[5], got[3])):
        ok = ~torch.isnan(x)
        assert torch.equal(_bits((x - img)[ok]), _bits(d[ok])), tag
    r = pgd_cases.norm64(got[2].cpu().numpy(), got[3].cpu().numpy())
    print("   norm %.9g  budget %.9g" % (r, pgd_cases.budget(bound)))
    if math.isfinite(ref["E"]):           # (a NaN pixel makes E NaN, which by the statement leaves the step unprojected)
        assert r <= pgd_cases.budget(bound), (tag, r)

    # ---- the launch's manners
    for op in c.ops:
        assert op.fence_intact(), tag
    assert c.ws_fence_intact(), tag
    for op, b0 in zip(c.ops[2:6], inputs0):                     # gradients and clean images are only read
        assert torch.equal(op.buf.view(torch.int32), b0)
    for g in got[2:]:                                           # every output element was written
        assert not bool((_bits(g) == SENTINEL).any())
    c.reset()                                                   # a second call from the same state: the same bits
    assert c.run(joint, eps, bound) == 0
    for g, g2 in zip(got, c.outputs()):
        assert torch.equal(_bits(g), _bits(g2))
    assert torch.equal(c.ws[WS_FENCE:WS_FENCE + 4], scalar_bits)
    return got, (G, a, E, s)


@pytest.mark.parametrize("joint", [0, 1])
@pytest.mark.parametrize("shift", [0, 1])
@pytest.mark.parametrize("n", SMALL)
def test_step_against_float64_and_the_stated_sequence(n, shift, joint):
    seen = set()
    for eps, bound in SETTINGS:
        _, (_, _, _, s) = _check(n, (shift,) * 8, joint, "mixed", eps, bound)
        seen.add(s < 1.0)
    if n >= 255:
        assert seen == {True, False}                           # both branches of s were taken


@pytest.mark.parametrize("joint", [0, 1])
@pytest.mark.parametrize("kind", [k for k in pgd_cases.KINDS if k != "mixed"])
def test_crafted_kinds(kind, joint):
    """One NaN or +Inf gradient, no gradient at all (and a NaN pixel), g1 = -g2: a = 0 moves nothing and makes no NaN."""
    for n in (5, 257, 1025):
        for eps, bound in SETTINGS:
            got, (G, a, _, _) = _check(n, (0,) * 8, joint, kind, eps, bound)
            if kind in ("nan", "inf", "zero") or joint:
                assert a == 0.0 and not (0.0 < G < math.inf), (kind, joint, G, a)
            else:
                assert a > 0.0


def test_two_partials_start_at_the_size_the_tests_use():
    """1025 floats are 257 quads: the first n with two workgroups, hence two partials; the workspace holds 4 scalars and
    two partials for every workgroup of the largest launch."""
    assert 4 * WORKGROUP + 1 in SMALL and 4 * WORKGROUP in [n - 1 for n in SMALL]
    assert _lib().pcfa_pgd_l2_workspace_bytes() == 8 * (4 + 2 * _max_threads() // WORKGROUP)


@pytest.mark.parametrize("joint", [0, 1])
@pytest.mark.parametrize("shift", [0, 1])
def test_second_trip_of_the_grid_stride_loop(shift, joint):
    n = _second_trip()
    assert n % 4 != 0 and (n + 3) // 4 == _max_threads() + 1
    eps, bound = SETTINGS[joint]                               # (0.00025, 0.005): s = 1;  (0.002, 0.003): s < 1
    _, (_, _, _, s) = _check(n, (shift,) * 8, joint, "mixed", eps, bound)
    assert (s < 1.0) == bool(joint)


@pytest.mark.parametrize("odd", range(8))
def test_one_unaligned_pointer_takes_the_scalar_path(odd):
    """Static buffers may be views: a single pointer that is only 4-byte aligned switches ALL accesses to scalar ones --
    and since the grid and the order of the sums depend on n alone, to the very bits of the aligned call."""
    shifts = tuple(1 if i == odd else 0 for i in range(8))
    eps, bound = SETTINGS[1 + odd % 2]
    got, scal = _check(1025, shifts, odd % 2, "mixed", eps, bound)
    base, scal0 = _check(1025, (0,) * 8, odd % 2, "mixed", eps, bound)
    assert scal == scal0
    for g, b in zip(got, base):
        assert torch.equal(_bits(g), _bits(b))


def test_two_streams_with_their_own_workspaces_give_the_solo_bits():
    n = 64 * 1024 + 3
    settings = (SETTINGS[1], SETTINGS[0])
    solo = []
    for k in range(2):
        c = _Call(n, (0,) * 8)
        assert c.run(k, *settings[k]) == 0
        solo.append((c.outputs(), c.scalars()))
    calls = [_Call(n, (0,) * 8), _Call(n, (0,) * 8)]
    streams = [torch.cuda.Stream(), torch.cuda.Stream()]
    torch.cuda.synchronize()
    for _ in range(3):                                         # a few rounds back to back, so that the two streams overlap
        for k in range(2):
            calls[k].reset()
        torch.cuda.synchronize()
        for k in range(2):
            with torch.cuda.stream(streams[k]):
                ptrs = [op.ptr() for op in calls[k].ops]
                ws = ctypes.c_void_p(calls[k].ws.data_ptr() + 8 * WS_FENCE)
                assert _lib().pcfa_pgd_l2_step(*ptrs, ctypes.c_float(settings[k][0]), ctypes.c_float(settings[k][1]), k, n,
                                               ws, fenced.stream()) == 0
        torch.cuda.synchronize()
        for k in range(2):
            assert calls[k].scalars() == solo[k][1]
            for g, w in zip(calls[k].outputs(), solo[k][0]):
                assert torch.equal(_bits(g), _bits(w))


def test_invalid_arguments_launch_nothing():
    c = _Call(257, (0,) * 8)
    before = c.all_bits()
    eps, bound = SETTINGS[1]
    assert c.run(0, eps, bound, n=-1) == PCFA_ERR_INVALID_ARG
    for k in range(9):                                          # the eight arrays and the workspace
        assert c.run(1, eps, bound, null=k) == PCFA_ERR_INVALID_ARG, k
    for k in range(8):                                          # a pointer that is not 4-byte aligned
        assert c.run(0, eps, bound, off=k) == PCFA_ERR_INVALID_ARG, k
    assert c.run(0, eps, bound, ws_off=4) == PCFA_ERR_INVALID_ARG
    assert c.run(2, eps, bound) == PCFA_ERR_INVALID_ARG
    assert c.run(-1, eps, bound) == PCFA_ERR_INVALID_ARG
    for bad in (0.0, -0.001, float("inf"), float("nan")):
        assert c.run(0, bad, bound) == PCFA_ERR_INVALID_ARG, bad
        assert c.run(0, eps, bad) == PCFA_ERR_INVALID_ARG, bad
    assert c.run(0, eps, bound, n=0) == 0                       # nothing to do is not an error -- and writes nothing
    for b, b0 in zip(c.all_bits(), before):
        assert torch.equal(b, b0)


def test_operator_checks_its_tensors_and_keeps_a_workspace_per_lane():
    from pcfa_amd import hip_ops, ops
    tab = [torch.from_numpy(a).to(DEV) for a in pgd_cases.table(1025)]
    x1, x2, g1, g2, i1, i2 = tab
    d1, d2 = torch.empty_like(x1), torch.empty_like(x2)
    eps, bound = SETTINGS[1]
    hip_ops.pgd_l2_step(x1, x2, g1, g2, i1, i2, d1, d2, eps, bound, False)
    ws0 = hip_ops.pgd_l2_workspace(DEV)
    G, a, E, s = ws0[:4].tolist()
    c = _Call(1025, (0,) * 8)
    assert c.run(0, eps, bound) == 0
    assert c.scalars() == [G, a, E, s] and s < 1.0
    for g, w in zip(c.outputs(), (x1, x2, d1, d2)):
        assert torch.equal(_bits(g), _bits(w))
    assert hip_ops.pgd_l2_workspace(DEV).data_ptr() == ws0.data_ptr()          # allocated once per lane
    with ops.core.lane(1):
        ws1 = hip_ops.pgd_l2_workspace(DEV)
    assert ws1.data_ptr() != ws0.data_ptr() and ws1.numel() == ws0.numel() == c.ws_words
    x = [torch.zeros(8, device=DEV) for _ in range(8)]
    hip_ops.pgd_l2_step(*x, 0.01, 0.005, False)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        hip_ops.pgd_l2_step(*[t.cpu() for t in x], 0.01, 0.005, False)
    with pytest.raises(ValueError):
        hip_ops.pgd_l2_step(*x[:7], torch.zeros(9, device=DEV), 0.01, 0.005, False)
    with pytest.raises(ValueError):
        hip_ops.pgd_l2_step(torch.zeros(16, device=DEV)[::2], *x[1:], 0.01, 0.005, False)
    with pytest.raises(RuntimeError, match="invalid argument"):
        hip_ops.pgd_l2_step(*x, 0.01, 0.0, False)
