"""The warps and Resample2d through the C-ABI on fenced buffers (tests/fenced.py), against float64 computed from the
mirrored fp32 sample positions, with pixels steered onto every tap pattern, integer position, mask threshold, window edge
and channel tail: pcfa_pwc_warp_fwd / _bwd / _bwd_det, pcfa_spynet_warp_fwd / _bwd (csrc/warp_ops.hip),
pcfa_resample2d_fwd / _bwd (csrc/flownet_ops.hip) and pcfa_resample2d_bwd_det (warp_ops.hip).  The mirrors, references,
census, case table and gates are those of tests/warp.py (the derivation of every n is in its docstring);
tests/test_warp_host_cpu.py shows on the CPU that the cases reach their classes and that a plain fp32 implementation passes
every gate.

Inputs sit between NaN, outputs and the workspace (exactly *_workspace_bytes() long) are pre-filled with a sentinel NaN.
Each call checks (_twice): the status; every input and every fence bit-unchanged; no sentinel or non-finite value left in
an output; a second call from the same initial state gives identical bits -- for the hardware-atomic paths
(pcfa_pwc_warp_bwd, grad_in1 of pcfa_resample2d_bwd) the second call passes the gates instead.  Ratios and worst classes
are recorded as junit properties (--junitxml=FILE -o junit_family=xunit1).

Kernel by kernel: pwc_warp_fwd_kernel<false / true> -- every PWC / SpyNet case; pwc_warp_bwd_kernel -- every PWC case
(grad_out `one` and `zero`); pwc_warp_bwd_det_kernel<false / true> -- the cases with plane < 256 and, through the child
process with PCFA_WARP_SCATTER=global, the window cases (bit-equal to the window kernel's gated results);
pwc_warp_bwd_det_lds_kernel<false / true> -- the cases with plane >= 256; zero_ll_max_kernel and pwc_warp_finish_kernel --
every fixed-point call (G = 1, 2, 4 partials; the five grad_out variants move the unit); resample2d_fwd_kernel,
resample2d_bwd_kernel -- every Resample2d case; resample2d_bwd_det_kernel -- those whose input has the flow's size.

Out-of-range and non-finite flows (the `wild` cases: +-inf, NaN, +-3e38, +-1e10, the tile-centre pixel included).  Every
address is in range for any float:
  - warp_taps forms x0, y0 with tap_index (resample2d_taps.hpp): the floor clamped to +-1e8 before the conversion, NaN ->
    -1e8 (fmaxf / fminf return the other operand).  x0 + 1, y0 + 1, the centre's x0 - 15 and lx = x0 - wx0 (wx0 in
    [-1, max(W - 31, -1)]) therefore cannot overflow.
  - The tap offsets onw .. ose are y0 W + x0 only under the tap's validity (0 <= x0 < W, 0 <= y0 < H), else 0: every load
    xc[s.o..] and every global atomic gc + o is inside the plane.
  - A window cell is ly 32 + lx only under 0 <= ly, lx < 32, else -1 (the global path, whose offset is valid as above).
  - s_org is clamped to [-1, max(size - 31, -1)], and a cell is non-zero only after a valid tap hit it, so the flush's
    (wy0 + cell / 32) W + wx0 + cell % 32 is that tap's texel.
  - gfpart, grad_flo and grad_x are indexed by the pixel / element index alone.
  - rs_taps clamps tap_index(fx), tap_index(fx + 1) to [0, size - 1] one by one; a1 = xf - truncf(xf) converts nothing.
What a poisoned pixel leaves: PWC-Net -- no valid tap, mask sum 0, nothing scattered; SpyNet -- the clamp returns every
value but NaN to the border (a legitimate position, gated), NaN has no valid tap; Resample2d -- a non-finite position puts
NaN weights on its clamped texels.  The wild cases assert fences and inputs intact, the gates on every pixel and texel no
poisoned pixel decides, and bit-repeatability of those; what the poisoned pixels and their texels hold is recorded.
"""
import os
import subprocess
import sys
import tempfile

import pytest
import torch

from pcfa_amd import _hip, hip_ops
from tests import warp as wp
from tests.fenced import NAN_BITS, PCFA_ERR_INVALID_ARG, PCFA_ERR_UNSUPPORTED, PCFA_ERR_WORKSPACE, SENTINEL, Fenced, stream
from tests.gates import dense_stride, unchanged

pytestmark = pytest.mark.gpu
torch.set_num_threads(min(16, torch.get_num_threads()))
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _lib():
    return _hip.load()


def _fenced(t, fill=NAN_BITS):
    return Fenced(t.shape, dense_stride(t.shape), fill).write(t)


def _out(shape):
    return Fenced(tuple(shape), dense_stride(tuple(shape)), SENTINEL)


def _ws(nbytes, shift=0):
    assert nbytes % 4 == 0
    return Fenced((nbytes // 4,), (1,), SENTINEL, shift)


def _bits(t):
    return t.contiguous().view(torch.int32)


def _reset(f):
    f.buf.view(torch.int32).copy_(f.bits0)


def _twice(call, outs, ins, ws=None, decided=None, repeatable=True):
    """The per-call checks; returns the outputs of the first call (and of the second, for the atomic paths) on the CPU.
    decided: per output, the elements that must be finite and repeat (default: all)."""
    scratch = [ws] if ws is not None else []
    res = []
    for rnd in range(2):
        for f in outs + scratch:
            _reset(f)
        assert call() == 0
        torch.cuda.synchronize()
        assert all(unchanged(f) for f in ins), "an input was written"
        assert all(f.fence_intact() for f in outs + scratch), "a store landed outside an output or the workspace"
        res.append([f.view().clone().cpu() for f in outs])
    dec = decided or [None] * len(outs)
    for a, b, d in zip(res[0], res[1], dec):
        d = torch.ones_like(a, dtype=torch.bool) if d is None else d.expand_as(a)
        assert bool((torch.isfinite(a) | ~d).all()), "non-finite output: a sentinel, or a NaN read from a fence"
        if repeatable:
            assert torch.equal(_bits(a)[d], _bits(b)[d]), "not repeatable bit for bit"
    return res if not repeatable else res[0]


def _decided(case, fs):
    """(pixels, texels) masks [B][1][..] of the elements no poisoned flow decides; None for the finite cases."""
    if case.builder != "wild":
        return None, None
    pix, tex = wp.poisoned(case, fs)
    return ~pix.unsqueeze(1), ~tex


def _record_poisoned(record, name, got, mask):
    if mask is not None and bool((~mask).any()):
        v = got[(~mask).expand_as(got)]
        record(name, "%d: %d nan, %d inf, %d zero, %d other" % (v.numel(), int(v.isnan().sum()), int(v.isinf().sum()),
                                                               int((v == 0).sum()), int((torch.isfinite(v) & (v != 0)).sum())))


# --------------------------------------------------------------------------- one call of every entry point
def _warp_operands(case, fs):
    x, flo = wp.inputs(case, fs)
    ops = [_fenced(x), _fenced(flo)]
    if case.kind == "spy":
        hor, ver, sx, sy = wp.spy_args(case)
        return ops + [_fenced(hor), _fenced(ver)], (sx, sy)
    return ops, (case.thr, fs)


def run_fwd(case, fs=1.0):
    lib = _lib()
    B, C, H, W = case.shape
    pix, _ = _decided(case, fs)
    if case.kind == "rs":
        x, flow = wp.inputs(case)
        fx, ff, fo = _fenced(x), _fenced(flow), _out((B, C, H, W))
        iH, iW = case.ishape
        return _twice(lambda: lib.pcfa_resample2d_fwd(fx.ptr(), ff.ptr(), fo.ptr(), B, C, iH, iW, H, W, 1, 1, stream()), [fo], [fx, ff],
                      decided=[pix])[0]
    ins, scal = _warp_operands(case, fs)
    fo = _out((B, C, H, W))
    name = "pcfa_spynet_warp_fwd" if case.kind == "spy" else "pcfa_pwc_warp_fwd"
    return _twice(lambda: getattr(lib, name)(*[f.ptr() for f in ins], fo.ptr(), B, C, H, W, *scal, stream()), [fo], ins,
                  decided=[pix])[0]


def run_bwd(case, fs=1.0, variant="one", fixed=True, ws_bytes=None, ws_shift=0):
    """(grad_x, grad_flo) of one call; the atomic paths return both calls' results."""
    lib = _lib()
    B, C, H, W = case.shape
    iH, iW = case.ishape
    pix, tex = _decided(case, fs)
    fg = _fenced(wp.gout(case, variant))
    fgx, fgf = _out((B, C, iH, iW)), _out((B, 2, H, W))
    if case.kind == "rs":
        x, flow = wp.inputs(case)
        ins = [_fenced(x), _fenced(flow), fg]
        if not fixed:
            return _twice(lambda: lib.pcfa_resample2d_bwd(*[f.ptr() for f in ins], fgx.ptr(), fgf.ptr(), B, C, iH, iW, H, W, 1, 1,
                                                          stream()), [fgx, fgf], ins, decided=[tex, pix], repeatable=False)
        ws = _ws(int(lib.pcfa_resample2d_bwd_det_workspace_bytes(B, C, H, W)))
        return _twice(lambda: lib.pcfa_resample2d_bwd_det(*[f.ptr() for f in ins], fgx.ptr(), fgf.ptr(), ws.ptr(), 4 * ws.size[0],
                                                          B, C, H, W, stream()), [fgx, fgf], ins, ws, decided=[tex, pix])
    ins, scal = _warp_operands(case, fs)
    ins = ins + [fg]
    if not fixed:
        assert case.kind == "pwc"
        return _twice(lambda: lib.pcfa_pwc_warp_bwd(*[f.ptr() for f in ins], fgx.ptr(), fgf.ptr(), B, C, H, W, *scal, stream()),
                      [fgx, fgf], ins, decided=[tex, pix], repeatable=False)
    stem = "pcfa_spynet_warp_bwd" if case.kind == "spy" else "pcfa_pwc_warp_bwd_det"
    ws = _ws(int(getattr(lib, stem + "_workspace_bytes")(B, C, H, W)))
    return _twice(lambda: getattr(lib, stem)(*[f.ptr() for f in ins], fgx.ptr(), fgf.ptr(), ws.ptr(), 4 * ws.size[0], B, C, H, W,
                                             *scal, stream()), [fgx, fgf], ins, ws, decided=[tex, pix])


# --------------------------------------------------------------------------- the gates on every case
def _check_case(record, case):
    det = case.ishape == case.shape[2:]
    atomic = case.kind != "spy"
    for fs in case.fs:
        tag = "fs%g_" % fs
        pix, tex = _decided(case, fs)
        out = run_fwd(case, fs)
        _record_poisoned(record, tag + "poisoned_out", out, pix)
        wp.check_fwd(case, fs, out, record, tag + "fwd_")
        for variant in wp.GOUTS:
            if det:
                gx, gf = run_bwd(case, fs, variant)
                if variant == "one":
                    _record_poisoned(record, tag + "poisoned_gx", gx, tex)
                    _record_poisoned(record, tag + "poisoned_gf", gf, pix)
                wp.check_bwd(case, fs, variant, gx, gf, True, record, tag + variant + "_fix_")
            if atomic and variant in ("one", "zero"):
                for rnd, (gx, gf) in enumerate(run_bwd(case, fs, variant, fixed=False)):
                    wp.check_bwd(case, fs, variant, gx, gf, False, record, tag + variant + "_atomic%d_" % rnd)


@pytest.mark.parametrize("case", wp.cases("pwc"), ids=lambda c: c.name)
def test_pwc_warp(record_property, case):
    """pcfa_pwc_warp_fwd, _bwd_det (five grad_out variants) and _bwd (`one`, `zero`) at flow_scale 1, 0.625 and 5."""
    _check_case(record_property, case)


@pytest.mark.parametrize("case", wp.cases("spy"), ids=lambda c: c.name)
def test_spynet_warp(record_property, case):
    """pcfa_spynet_warp_fwd and _bwd (five grad_out variants)."""
    _check_case(record_property, case)


@pytest.mark.parametrize("case", wp.cases("rs"), ids=lambda c: c.name)
def test_resample2d(record_property, case):
    """pcfa_resample2d_fwd, _bwd and (input of the flow's size) _bwd_det."""
    _check_case(record_property, case)


# --------------------------------------------------------------------------- refusals write nothing
def test_refusals_write_nothing():
    lib = _lib()
    case = wp.CASES["pwc-2x11x18x20-smooth"]
    B, C, H, W = case.shape
    x, flo = wp.inputs(case)
    hor, ver, sx, sy = wp.spy_args(case)
    fx, ff, fg = _fenced(x), _fenced(flo), _fenced(wp.gout(case))
    fh, fv = _fenced(hor), _fenced(ver)
    fo, fgx, fgf = _out((B, C, H, W)), _out((B, C, H, W)), _out((B, 2, H, W))
    nb = int(lib.pcfa_pwc_warp_bwd_det_workspace_bytes(B, C, H, W))
    assert nb == int(lib.pcfa_spynet_warp_bwd_workspace_bytes(B, C, H, W)) == \
        B * C * H * W * 8 + wp.channel_groups(H * W, C) * B * 2 * H * W * 4 + 4096 * 4
    nr = int(lib.pcfa_resample2d_bwd_det_workspace_bytes(B, C, H, W))
    assert nr == B * C * H * W * 8 + 4096 * 4
    assert int(lib.pcfa_pwc_warp_bwd_det_workspace_bytes(B, 0, H, W)) == 0
    ws, odd = _ws(nb), _ws(nb + 8, shift=1)
    every = [fx, ff, fg, fh, fv, fo, fgx, fgf, ws, odd]

    def refused(status, want):
        torch.cuda.synchronize()
        assert status == want, (status, want)
        assert all(unchanged(f) for f in every), "a refused call touched a buffer"

    p = lambda f: f.ptr()   # noqa: E731
    s = stream()
    pwc = (p(fx), p(ff), p(fg), p(fgx), p(fgf))
    spy = (p(fx), p(ff), p(fh), p(fv), p(fg), p(fgx), p(fgf))
    # a short workspace, a workspace pointer off by 4
    refused(lib.pcfa_pwc_warp_bwd_det(*pwc, p(ws), nb - 8, B, C, H, W, case.thr, 1.0, s), PCFA_ERR_WORKSPACE)
    refused(lib.pcfa_spynet_warp_bwd(*spy, p(ws), nb - 8, B, C, H, W, sx, sy, s), PCFA_ERR_WORKSPACE)
    refused(lib.pcfa_resample2d_bwd_det(*pwc, p(ws), nr - 8, B, C, H, W, s), PCFA_ERR_WORKSPACE)
    refused(lib.pcfa_pwc_warp_bwd_det(*pwc, p(odd), nb, B, C, H, W, case.thr, 1.0, s), PCFA_ERR_INVALID_ARG)
    refused(lib.pcfa_spynet_warp_bwd(*spy, p(odd), nb, B, C, H, W, sx, sy, s), PCFA_ERR_INVALID_ARG)
    refused(lib.pcfa_resample2d_bwd_det(*pwc, p(odd), nr, B, C, H, W, s), PCFA_ERR_INVALID_ARG)
    # a null operand, a zero dimension
    refused(lib.pcfa_pwc_warp_fwd(p(fx), None, p(fo), B, C, H, W, case.thr, 1.0, s), PCFA_ERR_INVALID_ARG)
    refused(lib.pcfa_pwc_warp_fwd(p(fx), p(ff), p(fo), B, C, 0, W, case.thr, 1.0, s), PCFA_ERR_INVALID_ARG)
    refused(lib.pcfa_pwc_warp_bwd(p(fx), p(ff), None, p(fgx), p(fgf), B, C, H, W, case.thr, 1.0, s), PCFA_ERR_INVALID_ARG)
    refused(lib.pcfa_pwc_warp_bwd(*pwc, B, C, H, 0, case.thr, 1.0, s), PCFA_ERR_INVALID_ARG)
    refused(lib.pcfa_pwc_warp_bwd_det(*pwc, None, nb, B, C, H, W, case.thr, 1.0, s), PCFA_ERR_INVALID_ARG)
    refused(lib.pcfa_pwc_warp_bwd_det(*pwc, p(ws), nb, 0, C, H, W, case.thr, 1.0, s), PCFA_ERR_INVALID_ARG)
    refused(lib.pcfa_spynet_warp_fwd(p(fx), p(ff), None, p(fv), p(fo), B, C, H, W, sx, sy, s), PCFA_ERR_INVALID_ARG)
    refused(lib.pcfa_spynet_warp_fwd(p(fx), p(ff), p(fh), p(fv), p(fo), B, 0, H, W, sx, sy, s), PCFA_ERR_INVALID_ARG)
    refused(lib.pcfa_spynet_warp_bwd(p(fx), p(ff), p(fh), None, p(fg), p(fgx), p(fgf), p(ws), nb, B, C, H, W, sx, sy, s),
            PCFA_ERR_INVALID_ARG)
    refused(lib.pcfa_spynet_warp_bwd(*spy, p(ws), nb, B, C, H, 0, sx, sy, s), PCFA_ERR_INVALID_ARG)
    refused(lib.pcfa_resample2d_fwd(None, p(ff), p(fo), B, C, H, W, H, W, 1, 1, s), PCFA_ERR_INVALID_ARG)
    refused(lib.pcfa_resample2d_fwd(p(fx), p(ff), p(fo), B, C, H, W, 0, W, 1, 1, s), PCFA_ERR_INVALID_ARG)
    refused(lib.pcfa_resample2d_bwd(p(fx), p(ff), p(fg), None, p(fgf), B, C, H, W, H, W, 1, 1, s), PCFA_ERR_INVALID_ARG)
    refused(lib.pcfa_resample2d_bwd(*pwc, B, C, 0, W, H, W, 1, 1, s), PCFA_ERR_INVALID_ARG)
    refused(lib.pcfa_resample2d_bwd_det(p(fx), None, p(fg), p(fgx), p(fgf), p(ws), nr, B, C, H, W, s), PCFA_ERR_INVALID_ARG)
    refused(lib.pcfa_resample2d_bwd_det(*pwc, p(ws), nr, B, C, H, 0, s), PCFA_ERR_INVALID_ARG)
    # kernel_size 3, an input smaller than the flow
    refused(lib.pcfa_resample2d_fwd(p(fx), p(ff), p(fo), B, C, H, W, H, W, 3, 1, s), PCFA_ERR_UNSUPPORTED)
    refused(lib.pcfa_resample2d_bwd(*pwc, B, C, H, W, H, W, 3, 1, s), PCFA_ERR_UNSUPPORTED)
    refused(lib.pcfa_resample2d_fwd(p(fx), p(ff), p(fo), B, C, H - 1, W, H, W, 1, 1, s), PCFA_ERR_UNSUPPORTED)


# --------------------------------------------------------------------------- the global-scatter form on the same cases
def _window_cases():
    return [c for c in wp.cases(window=True) if c.kind != "rs" and c.builder != "wild"]


def _child(path):
    """Runs in a fresh process with PCFA_WARP_SCATTER=global: the fixed-point backward of every window case."""
    assert os.environ.get("PCFA_WARP_SCATTER") == "global"
    res = {}
    for case in _window_cases():
        for fs in case.fs:
            gx, gf = run_bwd(case, fs)
            res["%s/%g" % (case.name, fs)] = (_bits(gx), _bits(gf))
    torch.save(res, path)


def test_global_scatter_gives_the_window_kernels_bits(record_property):
    """pwc_warp_bwd_det_kernel at plane >= 256 (PCFA_WARP_SCATTER=global, read once per process: a fresh child): grad_x and
    grad_flo bit-equal to the window kernel's results here, which pass the float64 gates."""
    assert os.environ.get("PCFA_WARP_SCATTER") is None
    with tempfile.TemporaryDirectory() as tmp:
        path = os.path.join(tmp, "bits.pt")
        env = dict(os.environ, PCFA_WARP_SCATTER="global", PYTHONPATH=ROOT + os.pathsep + os.environ.get("PYTHONPATH", ""))
        p = subprocess.run([sys.executable] + (["-s"] if sys.flags.no_user_site else []) +
                           ["-c", "import sys; from tests import test_warp_f64_gpu as t; t._child(sys.argv[1])", path],
                           cwd=ROOT, env=env, capture_output=True, text=True, timeout=300)
        assert p.returncode == 0, p.stderr[-3000:]
        theirs = torch.load(path)
    assert len(theirs) == sum(len(c.fs) for c in _window_cases()) >= 20
    for case in _window_cases():
        for fs in case.fs:
            gx, gf = run_bwd(case, fs)
            wp.check_bwd(case, fs, "one", gx, gf, True, lambda *_: None)
            tx, tf = theirs["%s/%g" % (case.name, fs)]
            assert torch.equal(_bits(gx), tx) and torch.equal(_bits(gf), tf), (case.name, fs)
    record_property("cases", len(theirs))


# --------------------------------------------------------------------------- the operators return the C-ABI call's bits
def _dev(*ts):
    return [t.cuda() for t in ts]


def test_pwc_warp_operator(record_property):
    case = wp.CASES["pwc-2x11x18x20-smooth"]
    fs = 0.625
    x, flo = wp.inputs(case, fs)
    out, (gx, gf) = run_fwd(case, fs), run_bwd(case, fs)
    for deterministic in (True, False):
        xd, fd = (t.requires_grad_() for t in _dev(x, flo))
        o = hip_ops.pwc_warp(xd, fd, case.thr, deterministic, fs)
        a, b = torch.autograd.grad(o, (xd, fd), wp.gout(case).cuda())
        assert torch.equal(_bits(o.detach().cpu()), _bits(out))
        if deterministic:
            assert torch.equal(_bits(a.cpu()), _bits(gx)) and torch.equal(_bits(b.cpu()), _bits(gf))
        else:
            wp.check_bwd(case, fs, "one", a.cpu(), b.cpu(), False, record_property, "atomic_")


def test_spynet_warp_operator():
    case = wp.CASES["spy-2x11x18x20-tearing"]
    x, flo = wp.inputs(case)
    hor, ver, _, _ = wp.spy_args(case)
    out, (gx, gf) = run_fwd(case), run_bwd(case)
    xd, fd = (t.requires_grad_() for t in _dev(x, flo))
    o = hip_ops.spynet_warp(xd, fd, *_dev(hor, ver))
    a, b = torch.autograd.grad(o, (xd, fd), wp.gout(case).cuda())
    assert torch.equal(_bits(o.detach().cpu()), _bits(out))
    assert torch.equal(_bits(a.cpu()), _bits(gx)) and torch.equal(_bits(b.cpu()), _bits(gf))


def test_resample2d_operators(record_property):
    case = wp.CASES["rs-2x3x13x27-tearing"]
    x, flow = wp.inputs(case)
    out, (gx, gf) = run_fwd(case), run_bwd(case)
    for op in (hip_ops.resample2d_det, hip_ops.resample2d):
        xd, fd = (t.requires_grad_() for t in _dev(x, flow))
        o = op(xd, fd)
        a, b = torch.autograd.grad(o, (xd, fd), wp.gout(case).cuda())
        assert torch.equal(_bits(o.detach().cpu()), _bits(out)) and torch.equal(_bits(b.cpu()), _bits(gf))
        if op is hip_ops.resample2d_det:
            assert torch.equal(_bits(a.cpu()), _bits(gx))
        else:
            wp.check_bwd(case, 1.0, "one", a.cpu(), b.cpu(), False, record_property, "atomic_")
