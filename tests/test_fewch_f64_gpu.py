"""The few-channel convolutions (csrc/conv3x3_fewout.hip: the 3x3 and the transposed 4x4 / stride 2 with 1..4 output
channels, forward and data gradient; csrc/conv_fewin.hip: un-packed and packed) and the element-wise entry points
pcfa_flow_step, pcfa_sum_n, pcfa_bias_relu_fwd, pcfa_leaky_relu_fwd/_bwd through the C-ABI on fenced buffers
(tests/fenced.py), against float64 computed from the same fp32 inputs, on every path the host code dispatches to.

Each convolution call checks: the status; every input (x, w, bias, addend, grad_out, the packed buffer) and every fence,
the workspace's included, bit-unchanged (inputs sit between NaN, so a read past an operand that is not masked poisons the
result); no sentinel left in the output and every element finite; the elementwise gate
|Y - Y64| <= 2 gamma(n + 2) P + (n + 2) 2^-126 with n the terms an element sums (3x3 forward 9 K + 1, its gradient 9 N + 1,
transposed forward 4 K + 1, its gradient 16 N, conv_fewin Cin k k + 1; the bound holds for any order of summation, so the
splits and the wave-order reduction add nothing; ReLU is 1-Lipschitz and applied to the float64 pre-activation); the
statistical gate of tests/gates.py against the fp32 emulation in the kernel's order (tests/fewch.py) globally, per
32-channel block and over first / last row and column, the tile seams, the last pixel tile and the transposed
convolution's four output classes; and a second call onto an output filled with -7 gives identical bits.  The path label
(from the Python mirror of the host rules in tests/fewch.py) and both ratios are recorded as junit properties
(--junitxml=FILE -o junit_family=xunit1).

Beyond the tables: every tap with a one-hot weight, exactly; the packing against the mirror's layout; inf / NaN in the
input reach only the outputs whose window holds them; refused calls leave the output untouched; the element-wise entry
points bit for bit against their fp32 statement on the CPU.
"""
import ctypes

import pytest
import torch
import torch.nn.functional as F

from pcfa_amd import _hip
from tests import fewch as fc
from tests.fenced import (NAN_BITS, PCFA_ERR_INVALID_ARG, PCFA_ERR_UNSUPPORTED, PCFA_ERR_WORKSPACE, SENTINEL, Fenced,
                          stream)
from tests.gates import dense_stride, gates, unchanged

pytestmark = pytest.mark.gpu
torch.set_num_threads(min(16, torch.get_num_threads()))


def _lib():
    return _hip.load()


def _fenced(t, fill=NAN_BITS, shift=0):
    return Fenced(t.shape, dense_stride(t.shape), fill, shift).write(t)


def _out(shape, shift=0):
    return Fenced(shape, dense_stride(shape), SENTINEL, shift)


def _p(f):
    return f.ptr() if f is not None else None


def _bits(t):
    return t.contiguous().view(torch.int32)


def _twice(call, outs, ins, scratch=()):
    """The per-call checks of every direction; returns the outputs of the first call on the CPU.  scratch: fenced
    buffers the call may write (the workspace): only their fences are checked."""
    assert call() == 0
    torch.cuda.synchronize()
    got = [f.view().clone() for f in outs]
    assert all(unchanged(f) for f in ins), "an input was written"
    assert all(f.fence_intact() for f in list(outs) + list(scratch)), "a store landed outside the output or the workspace"
    assert all(bool(torch.isfinite(g).all()) for g in got), "non-finite output: a sentinel, or a NaN read from a fence"
    for f in outs:
        f.view().fill_(-7.0)
    assert call() == 0
    torch.cuda.synchronize()
    assert all(torch.equal(_bits(f.view()), _bits(g)) for f, g in zip(outs, got)), "not repeatable bit for bit"
    assert all(unchanged(f) for f in ins) and all(f.fence_intact() for f in list(outs) + list(scratch))
    return [g.cpu() for g in got]


def _workspace(nbytes):
    assert nbytes % 4 == 0
    return Fenced((nbytes // 4,), (1,), NAN_BITS) if nbytes else None


def _gate(record_property, got, want, P, n, emu, H, W, px=fc.FO_PX, up=1):
    return gates(got, want, P, n, emu, up, record_property, regions=fc.regions, extra=fc.extra_groups(H, W, px, up))


def _cid(c):
    return "%s-%s" % (c[-1], fc.sid(c[0]))


# --------------------------------------------------------------------------- the callers
def fewout_fwd(kind, fx, fw, fb, fo, fws, shape):
    lib = _lib()
    f = lib.pcfa_conv3x3_fewout_fwd if kind == "conv3_fwd" else lib.pcfa_deconv4s2_fewout_fwd
    return lambda ws=True: f(fx.ptr(), fw.ptr(), _p(fb), fo.ptr(), _p(fws) if ws else None, *shape, stream())


def fewout_buffers(kind, x, w, b, shape, x_shift=0):
    """Fenced operands, output and workspace (of exactly *_workspace_bytes) of a forward call."""
    lib = _lib()
    B, K, N, H, W = shape
    up = 2 if kind == "deconv_fwd" else 1
    wsb = (lib.pcfa_conv3x3_fewout_workspace_bytes if up == 1 else lib.pcfa_deconv4s2_fewout_workspace_bytes)(*shape)
    assert int(wsb) == fc.workspace_bytes(*shape, deconv=up == 2)
    fx, fw, fb = _fenced(x, shift=x_shift), _fenced(w), _fenced(b) if b is not None else None
    return fx, fw, fb, _out((B, N, up * H, up * W)), _workspace(int(wsb))


def run_fewout_fwd(record_property, kind, shape, bias, x_shift, label):
    B, K, N, H, W = shape
    assert fc.path(kind, *shape, x_aligned=x_shift % 4 == 0) == label
    record_property("path", label)
    problem = fc.conv3_fwd_problem if kind == "conv3_fwd" else fc.deconv_fwd_problem
    x, w, b, want, P, emu = problem(B, K, N, H, W, bias)
    fx, fw, fb, fo, fws = fewout_buffers(kind, x, w, b, shape, x_shift)
    assert (fx.buf.data_ptr() + 4 * fx.off) % 16 == 4 * (x_shift % 4)
    call = fewout_fwd(kind, fx, fw, fb, fo, fws, shape)
    assert (fws is not None) == label.endswith("split")
    if fws is not None:     # without its workspace the call is refused before any launch
        assert call(ws=False) == PCFA_ERR_WORKSPACE
        torch.cuda.synchronize()
        assert unchanged(fo)
    got, = _twice(call, [fo], [f for f in (fx, fw, fb) if f is not None], [fws] if fws is not None else [])
    return _gate(record_property, got, want, P, fc.TERMS[kind](K, N), emu, H, W, up=2 if kind == "deconv_fwd" else 1)


def run_fewout_bwd(record_property, kind, shape, addend, label):
    lib = _lib()
    B, K, N, H, W = shape
    assert fc.path(kind, *shape) == label
    record_property("path", label)
    if kind == "conv3_bwd":
        g, w, a, want, P, emu = fc.conv3_bwd_problem(B, K, N, H, W, addend)
    else:
        g, w, want, P, emu = fc.deconv_bwd_problem(B, K, N, H, W)
        a = None
    fg, fw, fa, fo = _fenced(g), _fenced(w), _fenced(a) if a is not None else None, _out((B, K, H, W))

    def call():
        if kind == "conv3_bwd":
            return lib.pcfa_conv3x3_fewout_bwd(fg.ptr(), fw.ptr(), _p(fa), fo.ptr(), B, K, N, H, W, stream())
        return lib.pcfa_deconv4s2_fewout_bwd(fg.ptr(), fw.ptr(), fo.ptr(), B, K, N, H, W, stream())

    got, = _twice(call, [fo], [f for f in (fg, fw, fa) if f is not None])
    return _gate(record_property, got, want, P, fc.TERMS[kind](K, N), emu, H, W)


def pack_fewin(w):
    """pcfa_conv_fewin_pack into a NaN-fenced buffer of exactly packed_floats: (fenced w, fenced packed), checked against
    the mirror's layout element for element."""
    lib = _lib()
    N, Cin, k, _ = w.shape
    n = int(lib.pcfa_conv_fewin_packed_floats(Cin, N, k))
    assert n == fc.packed_floats(Cin, N, k) > 0
    fw, fp = _fenced(w), Fenced((n,), (1,), NAN_BITS)
    assert lib.pcfa_conv_fewin_pack(fw.ptr(), fp.ptr(), Cin, N, k, stream()) == 0
    torch.cuda.synchronize()
    assert unchanged(fw) and fp.fence_intact(), "packing wrote outside its buffer"
    P = fp.view().cpu()
    assert bool(torch.isfinite(P).all()), "packing left a NaN"
    assert torch.equal(_bits(P), _bits(fc.pack_reference(w))), "the packed layout is not the mirror's"
    fp.bits0 = fp.buf.view(torch.int32).clone()
    return fw, fp


def fewin_call(packed, fx, fwp, fb, fo, shape, relu):
    lib = _lib()
    B, Cin, N, k, H, W = shape
    f = lib.pcfa_conv_fewin_packed_fwd if packed else lib.pcfa_conv_fewin_fwd
    return lambda: f(_p(fx), _p(fwp), _p(fb), _p(fo), B, Cin, N, H, W, k, int(relu), stream())


def run_fewin(record_property, packed, shape, bias, relu, label):
    B, Cin, N, k, H, W = shape
    assert fc.path("fewin_packed" if packed else "fewin", B, Cin, N, H, W, k) == label
    record_property("path", label)
    x, w, b, want, P, emu = fc.fewin_problem(B, Cin, N, k, H, W, bias, relu)
    fw, fp = pack_fewin(w) if packed else (_fenced(w), None)
    fx, fb, fo = _fenced(x), _fenced(b) if bias else None, _out((B, N, H, W))
    got, = _twice(fewin_call(packed, fx, fp if packed else fw, fb, fo, shape, relu), [fo],
                  [f for f in (fx, fw, fp, fb) if f is not None])
    return _gate(record_property, got, want, P, fc.fewin_terms(Cin, k), emu, H, W, fc.FP_PX if packed else fc.FI_PX)


# --------------------------------------------------------------------------- 1. the tables
def test_host_rules_match_the_mirror():
    bad = fc.host_rule_mismatches(_lib())
    assert not bad, bad[:10]


@pytest.mark.parametrize("case", fc.CONV3_FWD, ids=_cid)
def test_conv3x3_fewout_fwd(record_property, case):
    run_fewout_fwd(record_property, "conv3_fwd", *case)


@pytest.mark.parametrize("case", fc.CONV3_BWD, ids=_cid)
def test_conv3x3_fewout_bwd(record_property, case):
    run_fewout_bwd(record_property, "conv3_bwd", *case)


@pytest.mark.parametrize("case", fc.DECONV_FWD, ids=_cid)
def test_deconv4s2_fewout_fwd(record_property, case):
    shape, bias, label = case
    run_fewout_fwd(record_property, "deconv_fwd", shape, bias, 0, label)


@pytest.mark.parametrize("case", fc.DECONV_BWD, ids=_cid)
def test_deconv4s2_fewout_bwd(record_property, case):
    shape, label = case
    run_fewout_bwd(record_property, "deconv_bwd", shape, False, label)


@pytest.mark.parametrize("case", fc.FEWIN_TABLE, ids=_cid)
def test_conv_fewin_fwd(record_property, case):
    """The un-packed kernel (150 KB of dynamic LDS, weights staged in one or two passes)."""
    run_fewin(record_property, False, *case)


@pytest.mark.parametrize("case", fc.FEWIN_TABLE, ids=lambda c: "packed-" + fc.sid(c[0]))
def test_conv_fewin_packed_fwd(record_property, case):
    shape, bias, relu, _ = case
    run_fewin(record_property, True, shape, bias, relu, "packed")


# --------------------------------------------------------------------------- 2. every tap, exactly
ONE_HOT_FWD = [((1, 40, 2, 9, 12), 0, "lds_s1"), ((1, 40, 3, 9, 11), 0, "plain_s1"), ((1, 270, 2, 6, 12), 0, "lds_split"),
               ((1, 270, 4, 7, 11), 0, "plain_split"), ((1, 40, 2, 9, 12), 1, "plain_s1")]


@pytest.mark.parametrize("case", ONE_HOT_FWD, ids=_cid)
def test_conv3x3_fewout_fwd_one_hot_taps(case):
    """w = 1.0 at one (o, c, ky, kx): out[o] is x[c] shifted by (ky - 1, kx - 1) bit for bit and the other outputs are
    zero -- the other waves and splits contribute exact zeros."""
    shape, x_shift, label = case
    B, K, N, H, W = shape
    assert fc.path("conv3_fwd", *shape, x_aligned=x_shift == 0) == label
    x = torch.randn(B, K, H, W, generator=torch.Generator().manual_seed(3))
    for t in range(9):
        o, c = t % N, (37 * t + 5) % K
        w = fc.one_hot((N, K, 3, 3), (o, c, t // 3, t % 3))
        fx, fw, _, fo, fws = fewout_buffers("conv3_fwd", x, w, None, shape, x_shift)
        assert fewout_fwd("conv3_fwd", fx, fw, None, fo, fws, shape)() == 0
        torch.cuda.synchronize()
        assert unchanged(fx) and unchanged(fw) and fo.fence_intact()
        assert torch.equal(fo.view().cpu(), fc.conv3_f64(x.double(), w.double()).float()), (t, o, c)


@pytest.mark.parametrize("case", [((1, 40, 3, 9, 11), "deconv_s1"), ((1, 270, 2, 6, 11), "deconv_split")], ids=_cid)
def test_deconv4s2_fewout_fwd_one_hot_taps(case):
    """w = 1.0 at one (c, o, ky, kx): out[o][2y - 1 + ky][2x - 1 + kx] = x[c][y][x], everything else zero, bit for bit."""
    shape, label = case
    B, K, N, H, W = shape
    assert fc.path("deconv_fwd", *shape) == label
    x = torch.randn(B, K, H, W, generator=torch.Generator().manual_seed(4))
    for t in range(16):
        o, c = t % N, (37 * t + 5) % K
        w = fc.one_hot((K, N, 4, 4), (c, o, t // 4, t % 4))
        fx, fw, _, fo, fws = fewout_buffers("deconv_fwd", x, w, None, shape)
        assert fewout_fwd("deconv_fwd", fx, fw, None, fo, fws, shape)() == 0
        torch.cuda.synchronize()
        assert unchanged(fx) and unchanged(fw) and fo.fence_intact()
        assert torch.equal(fo.view().cpu(), fc.deconv_f64(x.double(), w.double()).float()), (t, o, c)


@pytest.mark.parametrize("case", [((1, 12, 3, 9, 11), "c1"), ((1, 70, 2, 9, 11), "c8")], ids=_cid)
def test_fewout_bwd_one_hot_taps(case):
    """Both data gradients with a one-hot weight: grad_x[c] is the shifted (the strided) grad_out[o], the other
    channels exact zeros."""
    lib = _lib()
    shape, lab = case
    B, K, N, H, W = shape
    assert fc.path("conv3_bwd", *shape) == "bwd_" + lab and fc.path("deconv_bwd", *shape) == "deconv_bwd_" + lab
    gen = torch.Generator().manual_seed(6)
    g3, g4 = torch.randn(B, N, H, W, generator=gen), torch.randn(B, N, 2 * H, 2 * W, generator=gen)
    fg3, fg4 = _fenced(g3), _fenced(g4)
    for t in range(16):
        o, c = t % N, (37 * t + 5) % K
        fo = _out((B, K, H, W))
        if t < 9:
            w = fc.one_hot((N, K, 3, 3), (o, c, t // 3, t % 3))
            fw = _fenced(w)
            assert lib.pcfa_conv3x3_fewout_bwd(fg3.ptr(), fw.ptr(), None, fo.ptr(), B, K, N, H, W, stream()) == 0
            torch.cuda.synchronize()
            assert unchanged(fg3) and unchanged(fw) and fo.fence_intact()
            assert torch.equal(fo.view().cpu(), fc.conv3_grad_f64(g3.double(), w.double()).float()), (t, o, c)
            fo = _out((B, K, H, W))
        w = fc.one_hot((K, N, 4, 4), (c, o, t // 4, t % 4))
        fw = _fenced(w)
        assert lib.pcfa_deconv4s2_fewout_bwd(fg4.ptr(), fw.ptr(), fo.ptr(), B, K, N, H, W, stream()) == 0
        torch.cuda.synchronize()
        assert unchanged(fg4) and unchanged(fw) and fo.fence_intact()
        assert torch.equal(fo.view().cpu(), fc.deconv_grad_f64(g4.double(), w.double()).float()), (t, o, c)


@pytest.mark.parametrize("packed", [False, True], ids=["unpacked", "packed"])
@pytest.mark.parametrize("inst", [(2, 3), (1, 7)], ids=lambda i: "cin%d_k%d" % i)
def test_conv_fewin_one_hot_taps(inst, packed):
    """All Cin k k taps, one at a time: an MFMA product by 1.0 plus zeros is exact, so out[n] is the shifted x[c]."""
    Cin, k = inst
    shape = (1, Cin, 37, k, 7, 11)
    B, _, N, _, H, W = shape
    x = torch.randn(B, Cin, H, W, generator=torch.Generator().manual_seed(8))
    fx = _fenced(x)
    for t in range(Cin * k * k):
        n = (7 * t + 3) % N
        w = fc.one_hot((N, Cin, k, k), (n, t // (k * k), (t // k) % k, t % k))
        fw, fp = pack_fewin(w) if packed else (_fenced(w), None)
        fo = _out((B, N, H, W))
        assert fewin_call(packed, fx, fp if packed else fw, None, fo, shape, 0)() == 0
        torch.cuda.synchronize()
        assert unchanged(fx) and unchanged(fw) and fo.fence_intact()
        assert torch.equal(fo.view().cpu(), F.conv2d(x.double(), w.double(), padding=k // 2).float()), (t, n)


# --------------------------------------------------------------------------- 3. non-finite locality
def _poison(x, flip):
    """One +inf and one NaN in an interior element and a corner, a NaN in the first column of a middle row (its flat
    neighbour is the last column of the row above): returns the poisoned copy and the mask of poisoned elements."""
    B, C, H, W = x.shape
    bad = x.clone()
    v = (float("nan"), float("inf")) if flip else (float("inf"), float("nan"))
    bad[0, C // 2, H // 2, W // 2] = v[0]
    bad[B - 1, 0, 0, 0] = v[1]
    bad[0, C - 1, H // 2 + 2, 0] = float("nan")
    bad[B - 1, C - 1, H - 1, W - 1] = v[0]
    return bad, ~torch.isfinite(bad)


def _locality(run, x, reach, relu=False):
    """run(x) -> output on the CPU.  reach(mask) -> outputs whose window holds a poisoned element.  Outputs outside
    equal the finite run bit for bit; those inside are non-finite (not asserted under a ReLU, whose fmaxf turns NaN
    into 0)."""
    clean = run(x)
    assert bool(torch.isfinite(clean).all())
    for flip in (False, True):
        bad, mask = _poison(x, flip)
        hit = reach(mask.double()) > 0
        got = run(bad)
        assert 0 < int(hit.sum()) < hit.numel()
        assert torch.equal(_bits(got)[~hit], _bits(clean)[~hit]), "a non-finite input reached an output outside its window"
        if not relu:
            assert not bool(torch.isfinite(got[hit]).any()), "an output whose window holds inf / NaN is finite"


@pytest.mark.parametrize("case", [((2, 40, 2, 9, 12), 0, "lds_s1"), ((2, 40, 3, 9, 11), 0, "plain_s1"),
                                  ((1, 270, 2, 10, 12), 0, "lds_split"), ((1, 270, 2, 9, 11), 0, "plain_split")], ids=_cid)
def test_conv3x3_fewout_fwd_nonfinite_locality(case):
    """Out-of-range taps are masked by a select on a clamped address, not by a product: an inf or NaN reaches exactly
    the outputs whose 3x3 window holds it, the wrapped columns of the flat tile not among them."""
    shape, x_shift, label = case
    B, K, N, H, W = shape
    assert fc.path("conv3_fwd", *shape) == label
    gen = torch.Generator().manual_seed(9)
    x, w = torch.randn(B, K, H, W, generator=gen), torch.randn(N, K, 3, 3, generator=gen) + 2.0
    b = torch.randn(N, generator=gen)

    def run(xv):
        fx, fw, fb, fo, fws = fewout_buffers("conv3_fwd", xv, w, b, shape)
        assert fewout_fwd("conv3_fwd", fx, fw, fb, fo, fws, shape)() == 0
        torch.cuda.synchronize()
        assert unchanged(fx) and fo.fence_intact()
        return fo.view().cpu()

    _locality(run, x, lambda m: fc.conv3_f64(m, torch.ones(N, K, 3, 3, dtype=torch.float64)))


@pytest.mark.parametrize("case", [((2, 40, 3, 9, 11), "deconv_s1"), ((1, 270, 2, 9, 11), "deconv_split")], ids=_cid)
def test_deconv4s2_fewout_fwd_nonfinite_locality(case):
    shape, label = case
    B, K, N, H, W = shape
    assert fc.path("deconv_fwd", *shape) == label
    gen = torch.Generator().manual_seed(10)
    x, w = torch.randn(B, K, H, W, generator=gen), torch.randn(K, N, 4, 4, generator=gen) + 2.0

    def run(xv):
        fx, fw, _, fo, fws = fewout_buffers("deconv_fwd", xv, w, None, shape)
        assert fewout_fwd("deconv_fwd", fx, fw, None, fo, fws, shape)() == 0
        torch.cuda.synchronize()
        assert unchanged(fx) and fo.fence_intact()
        return fo.view().cpu()

    _locality(run, x, lambda m: fc.deconv_f64(m, torch.ones(K, N, 4, 4, dtype=torch.float64)))


@pytest.mark.parametrize("shape", [(2, 12, 3, 9, 11), (1, 70, 2, 9, 12)], ids=fc.sid)
def test_fewout_bwd_nonfinite_locality(shape):
    """inf / NaN in grad_out, both data gradients; the 3x3 with an addend, which stays finite."""
    lib = _lib()
    B, K, N, H, W = shape
    gen = torch.Generator().manual_seed(12)
    g3, g4 = torch.randn(B, N, H, W, generator=gen), torch.randn(B, N, 2 * H, 2 * W, generator=gen)
    w3, w4 = torch.randn(N, K, 3, 3, generator=gen) + 2.0, torch.randn(K, N, 4, 4, generator=gen) + 2.0
    fa = _fenced(torch.randn(B, K, H, W, generator=gen))
    fw3, fw4 = _fenced(w3), _fenced(w4)

    def run3(gv):
        fg, fo = _fenced(gv), _out((B, K, H, W))
        assert lib.pcfa_conv3x3_fewout_bwd(fg.ptr(), fw3.ptr(), fa.ptr(), fo.ptr(), B, K, N, H, W, stream()) == 0
        torch.cuda.synchronize()
        assert unchanged(fg) and unchanged(fa) and fo.fence_intact()
        return fo.view().cpu()

    def run4(gv):
        fg, fo = _fenced(gv), _out((B, K, H, W))
        assert lib.pcfa_deconv4s2_fewout_bwd(fg.ptr(), fw4.ptr(), fo.ptr(), B, K, N, H, W, stream()) == 0
        torch.cuda.synchronize()
        assert unchanged(fg) and fo.fence_intact()
        return fo.view().cpu()

    _locality(run3, g3, lambda m: fc.conv3_grad_f64(m, torch.ones(N, K, 3, 3, dtype=torch.float64)))
    _locality(run4, g4, lambda m: fc.deconv_grad_f64(m, torch.ones(K, N, 4, 4, dtype=torch.float64)))


@pytest.mark.parametrize("relu", [False, True], ids=["linear", "relu"])
@pytest.mark.parametrize("packed", [False, True], ids=["unpacked", "packed"])
@pytest.mark.parametrize("inst", [(2, 7), (2, 3)], ids=lambda i: "cin%d_k%d" % i)
def test_conv_fewin_nonfinite_locality(inst, packed, relu):
    """The flat input range in LDS holds the neighbouring rows' ends: the column mask must select, not multiply.  Under the
    ReLU fmaxf(NaN, 0) = 0, so there only the outputs outside the windows are asserted."""
    Cin, k = inst
    shape = (2, Cin, 40, k, 9, 13)
    B, _, N, _, H, W = shape
    gen = torch.Generator().manual_seed(13)
    x, w = torch.randn(B, Cin, H, W, generator=gen), torch.randn(N, Cin, k, k, generator=gen) + 2.0
    b = torch.randn(N, generator=gen)
    fw, fp = pack_fewin(w) if packed else (_fenced(w), None)
    fb = _fenced(b)

    def run(xv):
        fx, fo = _fenced(xv), _out((B, N, H, W))
        assert fewin_call(packed, fx, fp if packed else fw, fb, fo, shape, relu)() == 0
        torch.cuda.synchronize()
        assert unchanged(fx) and fo.fence_intact()
        return fo.view().cpu()

    _locality(run, x, lambda m: F.conv2d(m, torch.ones(N, Cin, k, k, dtype=torch.float64), padding=k // 2), relu)


# --------------------------------------------------------------------------- 4. refusals
def test_fewout_refusals():
    """N = 0 or 5 outputs and null pointers: the documented status, the output and every fence untouched."""
    lib = _lib()
    gen = torch.Generator().manual_seed(14)
    B, K, H, W = 1, 20, 6, 8

    def call(kind, N, null=()):
        Nb = max(N, 1)
        up = 2 if kind.startswith("deconv") else 1
        fwd = kind.endswith("fwd")
        src = torch.randn(B, K if fwd else Nb, (up if not fwd else 1) * H, (up if not fwd else 1) * W, generator=gen)
        dst = (B, Nb, up * H, up * W) if fwd else (B, K, H, W)
        fs, fw, fo = _fenced(src), _fenced(torch.randn(Nb * K * (16 if up == 2 else 9), generator=gen)), _out(dst)
        a = {"src": fs.ptr(), "w": fw.ptr(), "dst": fo.ptr()}
        a.update({name: None for name in null})
        if kind == "conv3_fwd":
            st = lib.pcfa_conv3x3_fewout_fwd(a["src"], a["w"], None, a["dst"], None, B, K, N, H, W, stream())
        elif kind == "deconv_fwd":
            st = lib.pcfa_deconv4s2_fewout_fwd(a["src"], a["w"], None, a["dst"], None, B, K, N, H, W, stream())
        elif kind == "conv3_bwd":
            st = lib.pcfa_conv3x3_fewout_bwd(a["src"], a["w"], None, a["dst"], B, K, N, H, W, stream())
        else:
            st = lib.pcfa_deconv4s2_fewout_bwd(a["src"], a["w"], a["dst"], B, K, N, H, W, stream())
        torch.cuda.synchronize()
        assert all(unchanged(f) for f in (fs, fw, fo)), "a refused call touched a buffer"
        return st

    for kind in ("conv3_fwd", "deconv_fwd", "conv3_bwd", "deconv_bwd"):
        for N in (0, 5):
            assert call(kind, N) == PCFA_ERR_UNSUPPORTED, (kind, N)
        for name in ("src", "w", "dst"):
            assert call(kind, 2, null=(name,)) == PCFA_ERR_INVALID_ARG, (kind, name)


def test_conv_fewin_refusals():
    """Unsupported (Cin, k), null pointers, shapes over the LDS limits of either kernel, a packed buffer or an un-packed
    weight that is not 16-B aligned: each returns before any launch and leaves the output untouched."""
    gen = torch.Generator().manual_seed(15)

    def call(shape, packed, null=(), w_shift=0, n_w=None):
        B, Cin, N, k, H, W = shape
        n_w = n_w or (max(fc.packed_floats(Cin, N, k), 256) if packed else N * Cin * k * k)
        fx, fw = _fenced(torch.randn(B, Cin, H, W, generator=gen)), _fenced(torch.randn(n_w, generator=gen), shift=w_shift)
        fo = _out((B, N, H, W))
        a = {"x": fx, "w": fw, "out": fo}
        a.update({name: None for name in null})
        st = fewin_call(packed, a["x"], a["w"], None, a["out"], shape, 1)()
        torch.cuda.synchronize()
        assert all(unchanged(f) for f in (fx, fw, fo)), "a refused call touched a buffer"
        return st

    ok = (1, 2, 8, 7, 5, 9)
    for packed in (False, True):
        for name in ("x", "w", "out"):
            assert call(ok, packed, null=(name,)) == PCFA_ERR_INVALID_ARG, (packed, name)
        for Cin, k in ((3, 3), (4, 7), (2, 9), (1, 3), (1, 5), (2, 1)):
            assert call((1, Cin, 8, k, 5, 9), packed, n_w=4096) == PCFA_ERR_UNSUPPORTED, (packed, Cin, k)
        assert call(ok, packed, w_shift=1) == PCFA_ERR_INVALID_ARG, packed          # w / packed 16-B aligned
        assert call(ok, packed, w_shift=2) == PCFA_ERR_INVALID_ARG, packed
    B, Cin, N, k, H, W = fc.FEWIN_OVER_LDS
    assert not fc.fewin_supported(Cin, N, k, W) and fc.fewin_supported(Cin, N, k, 8)
    assert call(fc.FEWIN_OVER_LDS, False) == PCFA_ERR_UNSUPPORTED
    B, Cin, N, k, H, W = fc.FEWIN_PACKED_OVER_LDS
    assert not fc.fewin_supported(Cin, N, k, W, packed=True)
    assert call(fc.FEWIN_PACKED_OVER_LDS, True) == PCFA_ERR_UNSUPPORTED
    lib = _lib()
    assert lib.pcfa_conv_fewin_packed_floats(3, 8, 3) == -1 and lib.pcfa_conv_fewin_packed_floats(2, 0, 7) == -1
    fw, fp = _fenced(torch.randn(72, generator=gen)), Fenced((1024,), (1,), NAN_BITS)
    assert lib.pcfa_conv_fewin_pack(fw.ptr(), fp.ptr(), 3, 8, 3, stream()) == PCFA_ERR_UNSUPPORTED
    assert lib.pcfa_conv_fewin_pack(None, fp.ptr(), 2, 4, 3, stream()) == PCFA_ERR_INVALID_ARG
    assert lib.pcfa_conv_fewin_pack(fw.ptr(), None, 2, 4, 3, stream()) == PCFA_ERR_INVALID_ARG
    torch.cuda.synchronize()
    assert unchanged(fw) and unchanged(fp)


# --------------------------------------------------------------------------- 5. the element-wise entry points
SIZES = [1, 3, 4, 5, 6, 1027]
CAPPED = 4096 * 256 + 259        # past the 4096-block grid of the leaky pair: the grid-stride loop's second round


def _rand(n, seed):
    return torch.randn(n, generator=torch.Generator().manual_seed(seed))


def _exact(call, outs, ins, want):
    got = _twice(call, outs, ins)
    for g, w in zip(got, want):
        assert torch.equal(_bits(g), _bits(w)), "not the fp32 statement bit for bit"


@pytest.mark.parametrize("shift", [0, 1], ids=["aligned", "off1"])
@pytest.mark.parametrize("n", SIZES)
def test_flow_step_exact(n, shift):
    """coords1_new = coords1 + delta; flow_new = coords1_new - coords0: one rounding each."""
    lib = _lib()
    c1, d, c0 = _rand(n, 1) * 50, _rand(n, 2), _rand(n, 3) * 50
    f1, fd, f0 = _fenced(c1), _fenced(d, shift=shift), _fenced(c0)
    o1, o2 = _out((n,)), _out((n,), shift)
    v = c1 + d
    _exact(lambda: lib.pcfa_flow_step(f1.ptr(), fd.ptr(), f0.ptr(), o1.ptr(), o2.ptr(), n, stream()), [o1, o2], [f1, fd, f0],
           [v, v - c0])
    for null in range(5):
        a = [f.ptr() for f in (f1, fd, f0, o1, o2)]
        a[null] = None
        assert lib.pcfa_flow_step(*a, n, stream()) == PCFA_ERR_INVALID_ARG
    assert lib.pcfa_flow_step(f1.ptr(), fd.ptr(), f0.ptr(), o1.ptr(), o2.ptr(), 0, stream()) == PCFA_ERR_INVALID_ARG


@pytest.mark.parametrize("shift", [0, 1], ids=["vector", "scalar"])
@pytest.mark.parametrize("k", [1, 2, 12, 16])
@pytest.mark.parametrize("n", SIZES)
def test_sum_n_exact(n, k, shift):
    """k sources added in index order; the scalar path by one source one float into its fence."""
    lib = _lib()
    src = [_rand(n, 20 + i) * (1 + i) for i in range(k)]
    fs = [_fenced(s, shift=shift if i == k - 1 else 0) for i, s in enumerate(src)]
    fo = _out((n,))
    want = src[0].clone()
    for s in src[1:]:
        want = want + s
    arr = (ctypes.c_void_p * k)(*[f.ptr().value for f in fs])
    _exact(lambda: lib.pcfa_sum_n(arr, k, fo.ptr(), n, stream()), [fo], fs, [want])


def test_sum_n_and_bias_relu_past_the_capped_grid():
    """for_each4 launches at most 2048 blocks of 256 threads: 4 (2048 * 256 + 300) + 3 elements take the vector loop's
    second round and the first block's tail."""
    lib = _lib()
    C, plane = 3, 699453
    n = C * plane
    assert n > 4 * 2048 * 256 and n % 4 == 3
    a, b, bias = _rand(n, 51), _rand(n, 52), _rand(C, 53)
    fa, fb, fbias, fo = _fenced(a), _fenced(b), _fenced(bias), _out((n,))
    arr = (ctypes.c_void_p * 2)(fa.ptr().value, fb.ptr().value)
    _exact(lambda: lib.pcfa_sum_n(arr, 2, fo.ptr(), n, stream()), [fo], [fa, fb], [a + b])
    fo = _out((n,))
    _exact(lambda: lib.pcfa_bias_relu_fwd(fa.ptr(), fbias.ptr(), fo.ptr(), n, plane, C, stream()), [fo], [fa, fbias],
           [torch.clamp_min(a.view(C, plane) + bias.view(C, 1), 0.0).reshape(n)])


def test_sum_n_refusals():
    lib = _lib()
    fs = [_fenced(_rand(8, i)) for i in range(17)]
    fo = _out((8,))
    arr = (ctypes.c_void_p * 17)(*[f.ptr().value for f in fs])
    assert lib.pcfa_sum_n(arr, 0, fo.ptr(), 8, stream()) == PCFA_ERR_INVALID_ARG
    assert lib.pcfa_sum_n(arr, 17, fo.ptr(), 8, stream()) == PCFA_ERR_INVALID_ARG
    assert lib.pcfa_sum_n(arr, 2, None, 8, stream()) == PCFA_ERR_INVALID_ARG
    assert lib.pcfa_sum_n(arr, 2, fo.ptr(), 0, stream()) == PCFA_ERR_INVALID_ARG
    arr[1] = None
    assert lib.pcfa_sum_n(arr, 2, fo.ptr(), 8, stream()) == PCFA_ERR_INVALID_ARG
    torch.cuda.synchronize()
    assert unchanged(fo) and all(unchanged(f) for f in fs)


@pytest.mark.parametrize("shift", [0, 1], ids=["vector", "scalar"])
@pytest.mark.parametrize("bias", [True, False], ids=["bias", "nobias"])
@pytest.mark.parametrize("shape", [(1, 1, 1), (1, 3, 1), (1, 1, 4), (1, 1, 5), (2, 3, 5), (1, 13, 79)], ids=fc.sid)
def test_bias_relu_fwd_exact(shape, bias, shift):
    """out = max(x + bias[c], 0); plane = 5: a 16-B group straddles two channels; 13 x 79 = 1027 elements."""
    lib = _lib()
    B, C, plane = shape
    n = B * C * plane
    x, b = _rand(n, 31), _rand(C, 32)
    fx, fb, fo = _fenced(x, shift=shift), _fenced(b) if bias else None, _out((n,))
    want = x.view(B, C, plane) + b.view(1, C, 1) if bias else x.view(B, C, plane)
    _exact(lambda: lib.pcfa_bias_relu_fwd(fx.ptr(), _p(fb), fo.ptr(), n, plane, C, stream()), [fo],
           [f for f in (fx, fb) if f is not None], [torch.clamp_min(want, 0.0).reshape(n)])


@pytest.mark.parametrize("slope", [0.1, 0.0])
@pytest.mark.parametrize("n", SIZES + [CAPPED])
def test_leaky_relu_exact(n, slope):
    """y = x > 0 ? x : x * slope, and from the OUTPUT dx = out > 0 ? g : g * slope -- a product at slope 0 too."""
    lib = _lib()
    sl = torch.tensor(slope, dtype=torch.float32)
    x, g = _rand(n, 41), _rand(n, 42)
    x[::7] = 0.0
    fx, fg, fy, fd = _fenced(x), _fenced(g), _out((n,)), _out((n,))
    y = torch.where(x > 0, x, x * sl)
    _exact(lambda: lib.pcfa_leaky_relu_fwd(fx.ptr(), fy.ptr(), float(sl), n, stream()), [fy], [fx], [y])
    fyi = _fenced(y)
    _exact(lambda: lib.pcfa_leaky_relu_bwd(fyi.ptr(), fg.ptr(), fd.ptr(), float(sl), n, stream()), [fd], [fyi, fg],
           [torch.where(y > 0, g, g * sl)])
