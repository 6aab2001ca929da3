"""The stride-2 convolutions (csrc/conv_strided.hip: the 7x7 stem, the 3x3 with and without the fused 1x1 downsample,
and their data gradients) through the C-ABI on fenced buffers (tests/fenced.py), against float64 computed from the same
fp32 inputs, on every kernel configuration the host code dispatches to.

Each call checks: the status; the weight, the packed buffer, x or grad_out, the biases and every fence bit-unchanged
(inputs sit between NaN, so a read past an operand that is not masked poisons the result); no sentinel left in the output
and every element finite; the packing wrote only its *_packed_floats and left no NaN; the elementwise gate
|Y - Y64| <= 2 gamma(n + 2) P + (n + 2) 2^-126 with n the most terms an element sums (forward Cin k k + 1, the fused 1x1
Cin + 1, the 3x3 gradient 4 N [+ N with the 1x1's], the stem's 16 N) -- the activation is applied to the float64
pre-activation: ReLU and leaky ReLU are 1-Lipschitz, the bound carries over; the statistical gate of tests/gates.py
against the fp32 emulation in the kernel's order of summation (tests/strided.py), over the groups of strided.regions;
and a second call with the output pre-filled with -7 gives identical bits.  The ratios and the path label are recorded
as junit properties (--junitxml=FILE -o junit_family=xunit1).

The path of a shape comes from the Python mirror of the host rules (tests/strided.py); test_dev_switches runs this
module again with three rows per workgroup (PCFA_S2_RPW=3), which no table shape reaches by the policy alone.
"""
import os
import signal
import subprocess
import sys

import pytest
import torch

from pcfa_amd import _hip
from tests import strided as st
from tests.fenced import NAN_BITS, PCFA_ERR_INVALID_ARG, PCFA_ERR_UNSUPPORTED, SENTINEL, Fenced, stream
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


def pack(kind, w, wd, Cin, N, k):
    """pcfa_conv_s2[_ds][_bwd]_pack into a NaN-fenced buffer of the documented size: (fenced weights, fenced packed)."""
    lib = _lib()
    floats, want = {"fwd": (lib.pcfa_conv_s2_packed_floats(Cin, N, k), st.packed_floats(Cin, N, k)),
                    "ds": (lib.pcfa_conv_s2_ds_packed_floats(Cin, N), st.ds_packed_floats(Cin, N)),
                    "bwd": (lib.pcfa_conv_s2_bwd_packed_floats(Cin, N, k), st.bwd_packed_floats(Cin, N, k)),
                    "ds_bwd": (lib.pcfa_conv_s2_ds_bwd_packed_floats(Cin, N), st.ds_bwd_packed_floats(Cin, N))}[kind]
    assert int(floats) == want > 0
    fw = [_fenced(w)] + ([_fenced(wd)] if kind.startswith("ds") else [])
    fp = Fenced((want,), (1,), NAN_BITS)
    status = {"fwd": lambda: lib.pcfa_conv_s2_pack(fw[0].ptr(), fp.ptr(), Cin, N, k, stream()),
              "ds": lambda: lib.pcfa_conv_s2_ds_pack(fw[0].ptr(), fw[1].ptr(), fp.ptr(), Cin, N, stream()),
              "bwd": lambda: lib.pcfa_conv_s2_bwd_pack(fw[0].ptr(), fp.ptr(), Cin, N, k, stream()),
              "ds_bwd": lambda: lib.pcfa_conv_s2_ds_bwd_pack(fw[0].ptr(), fw[1].ptr(), fp.ptr(), Cin, N, stream())}[kind]()
    assert status == 0
    torch.cuda.synchronize()
    assert all(unchanged(f) for f in fw) and fp.fence_intact(), "packing wrote outside its buffer"
    assert bool(torch.isfinite(fp.view()).all()), "packing left a NaN"
    fp.bits0 = fp.buf.view(torch.int32).clone()
    return fw, fp


def _twice(call, outs, ins):
    """The per-call checks of both directions; returns the outputs of the first call on the CPU."""
    assert call() == 0
    torch.cuda.synchronize()
    got = [f.view().clone() for f in outs]
    assert all(unchanged(f) for f in ins), "an input was written"
    assert all(f.fence_intact() for f in outs), "a store landed outside the output"
    assert all(bool(torch.isfinite(g).all()) for g in got), "non-finite output: a sentinel, or a NaN read from a fence"
    for f in outs:
        f.view().fill_(-7.0)
    assert call() == 0
    torch.cuda.synchronize()
    assert all(torch.equal(f.view().view(torch.int32), g.view(torch.int32)) for f, g in zip(outs, got)), \
        "not repeatable bit for bit"
    assert all(unchanged(f) for f in ins) and all(f.fence_intact() for f in outs)
    return [g.cpu() for g in got]


def run_fwd(record_property, shape, label, act=0, bias=True, seed=0):
    """One pcfa_conv_s2_fwd (label stem / res_wn*) or pcfa_conv_s2_ds_fwd (ds_wn*) call on fenced buffers."""
    lib = _lib()
    B, Cin, N, k, H, W = shape
    ds = label.startswith("ds")
    assert st.fwd_path(Cin, N, k, ds) == label and lib.pcfa_conv_s2_supported(Cin, N, k, H, W)
    Ho, Wo = st.out_hw(k, H, W)
    rpw = st.rows_per_workgroup(label, B, N, Ho, Wo)
    record_property("path", label)
    record_property("rpw", rpw)
    x, w, wd, b, bd, refs = st.fwd_problem(B, Cin, N, k, H, W, ds, seed)
    fw, fp = pack("ds" if ds else "fwd", w, wd, Cin, N, k)
    fx = _fenced(x)
    fb = _fenced(b) if bias else None
    fbd = _fenced(bd) if bias and ds else None
    fo = _out((B, N, Ho, Wo))
    fod = _out((B, N, Ho, Wo)) if ds else None

    def call():
        if ds:
            return lib.pcfa_conv_s2_ds_fwd(fx.ptr(), fp.ptr(), _p(fb), fo.ptr(), _p(fbd), fod.ptr(), B, Cin, N, H, W, act,
                                           st.SLOPE, stream())
        return lib.pcfa_conv_s2_fwd(fx.ptr(), fp.ptr(), _p(fb), fo.ptr(), B, Cin, N, H, W, k, act, st.SLOPE, stream())

    got = _twice(call, [fo] + ([fod] if ds else []), [f for f in fw + [fp, fx, fb, fbd] if f is not None])
    rg = lambda h, w_, m: st.regions(label, h, w_, rpw)  # noqa: E731
    res = []
    for i, (y, (want, P, emu)) in enumerate(zip(got, refs)):
        bb = (bd if i else b).view(1, -1, 1, 1) if bias else torch.zeros(1, N, 1, 1)
        a = 0 if i else act                       # the 1x1's output: bias only
        res.append(gates(y, st.activate(want + bb.double(), a), P + bb.double().abs(), Cin + 1 if i else st.fwd_terms(Cin, k),
                         st.activate(emu + bb, a), 0, record_property, prefix="d_" if i else "", regions=rg))
    return res


def run_bwd(record_property, shape, label, seed=0):
    """One pcfa_conv_s2_bwd (stem_bwd / res_bwd_wn*) or pcfa_conv_s2_ds_bwd (ds_bwd_wn*) call on fenced buffers."""
    lib = _lib()
    B, Cin, N, k, H, W = shape
    ds = label.startswith("ds")
    assert st.bwd_path(Cin, N, k, ds) == label and lib.pcfa_conv_s2_bwd_supported(Cin, N, k, H, W)
    record_property("path", label)
    g, gd, w, wd, want, P, emu = st.bwd_problem(B, Cin, N, k, H, W, ds, seed)
    fw, fp = pack("ds_bwd" if ds else "bwd", w, wd, Cin, N, k)
    fg = _fenced(g)
    fgd = _fenced(gd) if ds else None
    fo = _out((B, Cin, H, W))

    def call():
        if ds:
            return lib.pcfa_conv_s2_ds_bwd(fg.ptr(), fgd.ptr(), fp.ptr(), fo.ptr(), B, Cin, N, H, W, stream())
        return lib.pcfa_conv_s2_bwd(fg.ptr(), fp.ptr(), fo.ptr(), B, Cin, N, H, W, k, stream())

    got, = _twice(call, [fo], [f for f in fw + [fp, fg, fgd] if f is not None])
    return gates(got, want, P, st.bwd_terms(Cin, N, k, ds), emu, 0, record_property,
                 regions=lambda h, w_, m: st.regions(label, h, w_))


# --------------------------------------------------------------------------- 1. the path tables
def _cid(c):
    return "%s-%s" % (c[1], st.sid(c[0]))


def test_path_table_covers_every_label():
    """The shape tables reach every configuration of the host dispatch: a policy change that moves a path's last shape
    off it fails here by name."""
    for table, ds, path, labels in ((st.FWD, False, st.fwd_path, st.FWD_LABELS), (st.DS, True, st.fwd_path, st.DS_LABELS),
                                    (st.BWD, False, st.bwd_path, st.BWD_LABELS),
                                    (st.DS_BWD, True, st.bwd_path, st.DS_BWD_LABELS)):
        for (B, Cin, N, k, H, W), lab in table:
            assert path(Cin, N, k, ds) == lab, ((B, Cin, N, k, H, W), lab)
        assert {lab for _, lab in table} == labels, sorted(labels - {lab for _, lab in table})


def test_host_rules_match_the_mirror():
    """pcfa_conv_s2_supported, pcfa_conv_s2_bwd_supported and every *_packed_floats entry point over a grid that holds
    every table shape and both sides of the 2^31 - 1 rule (nothing is allocated or launched for those)."""
    bad = st.host_rule_mismatches(_lib())
    assert not bad, bad[:10]


VARIANTS = [(0, False), (1, True), (2, True), (2, False)]   # (act, bias)


@pytest.mark.parametrize("variant", VARIANTS, ids=lambda v: "act%d-bias%d" % v)
@pytest.mark.parametrize("case", st.FWD, ids=_cid)
def test_conv_s2_fwd(record_property, case, variant):
    run_fwd(record_property, *case, act=variant[0], bias=variant[1])


@pytest.mark.parametrize("variant", VARIANTS, ids=lambda v: "act%d-bias%d" % v)
@pytest.mark.parametrize("case", st.DS, ids=_cid)
def test_conv_s2_ds_fwd(record_property, case, variant):
    """The 3x3 and the fused 1x1 of the same input: both outputs through both gates."""
    run_fwd(record_property, *case, act=variant[0], bias=variant[1])


@pytest.mark.parametrize("case", st.BWD, ids=_cid)
def test_conv_s2_bwd(record_property, case):
    run_bwd(record_property, *case)


@pytest.mark.parametrize("case", st.DS_BWD, ids=_cid)
def test_conv_s2_ds_bwd(record_property, case):
    run_bwd(record_property, *case)


def test_conv_s2_fwd_rows_per_workgroup(record_property):
    """The one shape here the policy itself gives more than one row per workgroup: 4 * 96 * 1 * 4 = 1536 workgroups at
    two rows each are still 6 per CU, so rpw = 2."""
    B, Cin, N, k, H, W = st.RPW_SHAPE
    assert st.fwd_path(Cin, N, k, env={}) == "res_wn4"
    assert st.rows_per_workgroup("res_wn4", B, N, H // 2, W // 2, env={}) == 2
    run_fwd(record_property, st.RPW_SHAPE, "res_wn4", act=1, bias=True)


# --------------------------------------------------------------------------- 2. refusals
def test_conv_s2_refusals():
    """Refused calls return their documented status and leave out and every fence untouched (the host code rejects
    each of them before any launch)."""
    lib = _lib()
    gen = torch.Generator().manual_seed(11)

    def fwd(shape, ds=False, act=0, null=(), x_shift=0):
        B, Cin, N, k, H, W = shape
        Ho, Wo = st.out_hw(k, H, W)
        fx = _fenced(torch.randn(B, Cin, H, W, generator=gen), shift=x_shift)
        n = max(st.ds_packed_floats(Cin, N) if ds else st.packed_floats(Cin, N, k), 64)
        fp = _fenced(torch.randn(n, generator=gen))
        fo, fod = _out((B, N, Ho, Wo)), _out((B, N, Ho, Wo))
        a = {"x": fx.ptr(), "packed": fp.ptr(), "out": fo.ptr(), "out_d": fod.ptr()}
        a.update({name: None for name in null})
        if ds:
            status = lib.pcfa_conv_s2_ds_fwd(a["x"], a["packed"], None, a["out"], None, a["out_d"], B, Cin, N, H, W, act,
                                             st.SLOPE, stream())
        else:
            status = lib.pcfa_conv_s2_fwd(a["x"], a["packed"], None, a["out"], B, Cin, N, H, W, k, act, st.SLOPE, stream())
        torch.cuda.synchronize()
        assert all(unchanged(f) for f in (fx, fp, fo, fod)), "a refused call touched a buffer"
        return status

    def bwd(shape, ds=False, null=(), g_shift=0, gd_shift=0, dx_shift=0):
        B, Cin, N, k, H, W = shape
        Ho, Wo = st.out_hw(k, H, W)
        fg = _fenced(torch.randn(B, N, Ho, Wo, generator=gen), shift=g_shift)
        fgd = _fenced(torch.randn(B, N, Ho, Wo, generator=gen), shift=gd_shift)
        n = max(st.ds_bwd_packed_floats(Cin, N) if ds else st.bwd_packed_floats(Cin, N, k), 64)
        fp = _fenced(torch.randn(n, generator=gen))
        fo = _out((B, Cin, H, W), shift=dx_shift)
        a = {"grad_out": fg.ptr(), "grad_out_d": fgd.ptr(), "packed": fp.ptr(), "grad_x": fo.ptr()}
        a.update({name: None for name in null})
        if ds:
            status = lib.pcfa_conv_s2_ds_bwd(a["grad_out"], a["grad_out_d"], a["packed"], a["grad_x"], B, Cin, N, H, W,
                                             stream())
        else:
            status = lib.pcfa_conv_s2_bwd(a["grad_out"], a["packed"], a["grad_x"], B, Cin, N, H, W, k, stream())
        torch.cuda.synchronize()
        assert all(unchanged(f) for f in (fg, fgd, fp, fo)), "a refused call touched a buffer"
        return status

    res, stem = (1, 8, 40, 3, 6, 16), (1, 3, 16, 7, 6, 16)
    for shape in (res, stem):
        for name in ("x", "packed", "out"):
            assert fwd(shape, null=(name,)) == PCFA_ERR_INVALID_ARG, (shape, name)
        assert fwd(shape, act=3) == PCFA_ERR_INVALID_ARG
        assert fwd(shape, x_shift=1) == PCFA_ERR_INVALID_ARG
        for name in ("grad_out", "packed", "grad_x"):
            assert bwd(shape, null=(name,)) == PCFA_ERR_INVALID_ARG, (shape, name)
        assert bwd(shape, g_shift=1) == PCFA_ERR_INVALID_ARG
        assert bwd(shape, dx_shift=1) == PCFA_ERR_INVALID_ARG
    for name in ("x", "packed", "out", "out_d"):
        assert fwd(res, ds=True, null=(name,)) == PCFA_ERR_INVALID_ARG, name
    assert fwd(res, ds=True, act=3) == PCFA_ERR_INVALID_ARG
    assert fwd(res, ds=True, x_shift=1) == PCFA_ERR_INVALID_ARG
    assert bwd(res, ds=True, null=("grad_out_d",)) == PCFA_ERR_INVALID_ARG
    assert bwd(res, ds=True, g_shift=1) == PCFA_ERR_INVALID_ARG
    assert bwd(res, ds=True, gd_shift=1) == PCFA_ERR_INVALID_ARG
    assert bwd(res, ds=True, dx_shift=1) == PCFA_ERR_INVALID_ARG
    B, Cin, N, k, H, W = res
    assert fwd((B, Cin, N, k, H, 18)) == PCFA_ERR_UNSUPPORTED          # W % 4
    assert fwd((B, Cin, N, k, H, 18), ds=True) == PCFA_ERR_UNSUPPORTED
    assert bwd((B, Cin, N, k, H, 20)) == PCFA_ERR_UNSUPPORTED          # W % 8
    assert bwd((B, Cin, N, k, H, 20), ds=True) == PCFA_ERR_UNSUPPORTED
    assert bwd((1, 3, 16, 7, 6, 20)) == PCFA_ERR_UNSUPPORTED
    for f in (fwd, bwd):
        assert f((B, Cin, N, k, 1, W)) == PCFA_ERR_UNSUPPORTED         # H = 1
        assert f((B, Cin, N, 5, H, W)) == PCFA_ERR_UNSUPPORTED         # ksize = 5
        assert f((B, 4, N, 7, H, W)) == PCFA_ERR_UNSUPPORTED           # 7x7 is the 3-channel stem only


# --------------------------------------------------------------------------- 3. the dev switch of the row loop
@pytest.mark.skipif(bool(os.environ.get("PCFA_STRIDED_CHILD")), reason="(the child run itself)")
def test_dev_switches():
    """This module once more in one fresh child process with three rows per workgroup (the variable is read once per
    process; the mirror reads the same environment): every forward shape with Ho % 3 != 0 ends on a short row block.
    A child that ends by a signal or a timeout fails the test."""
    for extra in [dict(PCFA_S2_RPW="3")]:
        env = dict(os.environ, PCFA_STRIDED_CHILD="1", **extra)
        cmd = [sys.executable, "-m", "pytest", os.path.abspath(__file__), "-q", "-x", "-rfE", "-m", "gpu",
               "-p", "no:cacheprovider",
               "-k", "not test_dev_switches"]
        try:
            r = subprocess.run(cmd, env=env, capture_output=True, text=True, timeout=600)
        except subprocess.TimeoutExpired:
            pytest.fail("child %s timed out" % extra)
        assert r.returncode >= 0, "child %s ended by signal %s" % (extra, signal.Signals(-r.returncode).name)
        assert r.returncode == 0, (extra, r.stdout[-4000:])
        assert " passed" in r.stdout and " failed" not in r.stdout, (extra, r.stdout[-2000:])
