"""Instance norm and the exact streaming kernels through the C-ABI on fenced buffers (tests/fenced.py), against float64:
pcfa_instnorm_fwd / _bwd / _workspace_bytes, pcfa_add_relu_fwd (csrc/norm_ops.hip), pcfa_relu_bwd / pcfa_relu_bwd2
(csrc/gru_math.hip).  The plan mirror, reference, emulation, inputs, case table and gates are those of tests/norm.py (every
bound is derived in its docstring, which also names the cases that reach each kernel); tests/test_norm_host_cpu.py shows on
the CPU that the cases reach their paths, that nothing is undecided at the ReLU and that the kernel's arithmetic passes every
gate.

Inputs sit between NaN; outputs and the workspace (exactly pcfa_instnorm_workspace_bytes() long) are pre-filled with a
sentinel NaN.  Each call checks (_twice of tests/test_warp_f64_gpu.py): the status; every input and every fence
bit-unchanged; no sentinel or non-finite value left in an output; a second call from the same state gives identical bits
(no kernel here uses atomics).  Ratios and worst groups are recorded as junit properties.

The wild case (NaN, +inf, -inf in one element of three planes): fences, inputs and statuses as everywhere, the gates on every
other plane -- a plane's statistics are its own --, and what the poisoned planes hold is recorded.
"""
import os
import subprocess
import sys
import tempfile

import pytest
import torch

from pcfa_amd import _hip
from tests import norm as nm
from tests.fenced import NAN_BITS, PCFA_ERR_INVALID_ARG, PCFA_ERR_UNSUPPORTED, PCFA_ERR_WORKSPACE, SENTINEL, Fenced, stream
from tests.gates import dense_stride, unchanged
from tests.test_warp_f64_gpu import _bits, _twice, _ws

pytestmark = pytest.mark.gpu
torch.set_num_threads(min(16, torch.get_num_threads()))
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _lib():
    return _hip.load()


def _in(t, shift=0):
    return Fenced(t.shape, dense_stride(t.shape), NAN_BITS, shift).write(t)


def _out(shape, shift=0):
    return Fenced(tuple(shape), dense_stride(tuple(shape)), SENTINEL, shift)


def _workspace(case):
    nb = int(_lib().pcfa_instnorm_workspace_bytes(case.planes, case.plane))
    assert nb == nm.case_plan(case).ws_bytes
    return _ws(nb)


def run_fwd(case, eps, relu, shift=(0, 0), wild=False):
    """(y, mean_rstd fenced buffer, its values) of one forward call; shift: floats of misalignment of (x, y)."""
    lib = _lib()
    x = nm.inputs(case, eps, wild)
    fx, fy, fm, ws = _in(x, shift[0]), _out(x.shape, shift[1]), _out((case.planes, 2)), _workspace(case)
    dec = None
    if wild:
        keep = torch.isfinite(x).all(1, keepdim=True)
        dec = [keep, keep]
    y, mr = _twice(lambda: lib.pcfa_instnorm_fwd(fx.ptr(), fy.ptr(), fm.ptr(), ws.ptr(), case.planes, case.plane, eps, relu,
                                                 stream()), [fy, fm], [fx], ws, decided=dec)
    return y, fm, mr


def run_bwd(case, eps, relu, variant, fm, shift=(0, 0, 0), wild=False):
    """grad_x of one backward call on the forward's mean_rstd buffer (an input here: bit-unchanged)."""
    lib = _lib()
    x, dy = nm.inputs(case, eps, wild), nm.gout(case, variant, eps)
    fm.bits0 = fm.buf.view(torch.int32).clone()
    fx, fg, fgx, ws = _in(x, shift[0]), _in(dy, shift[1]), _out(x.shape, shift[2]), _workspace(case)
    dec = [torch.isfinite(x).all(1, keepdim=True)] if wild else None
    return _twice(lambda: lib.pcfa_instnorm_bwd(fx.ptr(), fm.ptr(), fg.ptr(), fgx.ptr(), ws.ptr(), case.planes, case.plane,
                                                relu, stream()), [fgx], [fx, fm, fg], ws, decided=dec)[0]


def _check_case(record, case, p, tag="", fshift=(0, 0), bshift=(0, 0, 0), pf=None):
    """p: the plan the calls run on; pf: the forward's, where it differs (only the backward's operands are shifted)."""
    pf = pf or p
    fwd, bwd = nm.runs(case)
    fms = {}
    for eps, relu in fwd:
        y, fm, mr = run_fwd(case, eps, relu, fshift)
        fms[eps, relu] = fm
        nm.check_fwd(case, eps, relu, y, mr, pf, record, "%seps%g_relu%d_fwd_%s_" % (tag, eps, relu, pf.label))
    for eps, relu, variant in bwd:
        dx = run_bwd(case, eps, relu, variant, fms[eps, relu], bshift)
        nm.check_bwd(case, eps, relu, variant, dx, p, record, "%seps%g_relu%d_%s_bwd_" % (tag, eps, relu, variant))


@pytest.mark.parametrize("case", nm.TABLE, ids=lambda c: c.name)
def test_instnorm(record_property, case):
    """pcfa_instnorm_fwd and _bwd on the path the case is in the table for: relu 0 / 1, eps 1e-5 / 0, grad_out random, zero
    and one-hot."""
    assert os.environ.get("PCFA_INSTNORM_FUSED") is None
    p = nm.case_plan(case)
    assert p.label == case.label
    record_property("path", p.label)
    _check_case(record_property, case, p)


@pytest.mark.parametrize("name", nm.MISALIGNED)
@pytest.mark.parametrize("which", ["x", "outputs"])
def test_instnorm_misaligned_takes_the_scalar_path(record_property, name, which):
    """plane % 4 == 0 with x, or y / grad_out / grad_x, 4 bytes off a 16-byte boundary: the scalar two-launch form."""
    case = nm.CASES[name]
    p = nm.case_plan(case, vec=False)
    assert p.label == "two_scalar" and case.plane % 4 == 0
    if which == "x":
        _check_case(record_property, case, p, "shift_x_", (1, 0), (1, 0, 0))
    else:
        _check_case(record_property, case, p, "shift_y_", (0, 1), (0, 0, 3))
        # grad_out alone is shifted: the forward that feeds this backward runs, and is gated, on the case's own path
        _check_case(record_property, case, p, "shift_g_", (0, 0), (0, 2, 0), pf=nm.case_plan(case))


def test_instnorm_wild(record_property):
    case = nm.CASES[nm.WILD]
    p = nm.case_plan(case)
    x = nm.inputs(case, nm.EPS, True)
    keep = torch.isfinite(x).all(1)
    assert int((~keep).sum()) == 3
    for relu in (0, 1):
        y, fm, mr = run_fwd(case, nm.EPS, relu, wild=True)
        nm.check_fwd(case, nm.EPS, relu, y, mr, p, record_property, "wild_relu%d_fwd_" % relu, keep)
        dx = run_bwd(case, nm.EPS, relu, "random", fm, wild=True)
        nm.check_bwd(case, nm.EPS, relu, "random", dx, p, record_property, "wild_relu%d_bwd_" % relu, keep)
        for nme, t in (("y", y), ("mean_rstd", mr), ("grad_x", dx)):
            v = t[~keep]
            record_property("wild_relu%d_poisoned_%s" % (relu, nme), "%d: %d nan, %d inf, %d zero, %d other" % (
                v.numel(), int(v.isnan().sum()), int(v.isinf().sum()), int((v == 0).sum()),
                int((torch.isfinite(v) & (v != 0)).sum())))


# --------------------------------------------------------------------------- the one-launch form switched off
def _child(path):
    """Runs in a fresh process with PCFA_INSTNORM_FUSED=0 (read once per process): both FUSED_OFF cases, forward and
    backward, through the same per-call checks."""
    assert os.environ.get("PCFA_INSTNORM_FUSED") == "0"
    res = {}
    for name in nm.FUSED_OFF:
        case = nm.CASES[name]
        for relu in (0, 1):
            y, fm, mr = run_fwd(case, nm.EPS, relu)
            res[name, relu] = (y, mr, run_bwd(case, nm.EPS, relu, "random", fm))
    torch.save(res, path)


def test_instnorm_two_launch_form_on_the_one_launch_cases(record_property):
    """One case per one-launch kernel on the two-launch form, gated against float64 (its fp64 summation order differs from
    the one-launch form's: no bit equality asked)."""
    assert os.environ.get("PCFA_INSTNORM_FUSED") is None
    with tempfile.TemporaryDirectory() as tmp:
        path = os.path.join(tmp, "res.pt")
        env = dict(os.environ, PCFA_INSTNORM_FUSED="0", PYTHONPATH=ROOT + os.pathsep + os.environ.get("PYTHONPATH", ""))
        try:
            r = subprocess.run([sys.executable] + (["-s"] if sys.flags.no_user_site else []) +
                               ["-c", "import sys; from tests import test_norm_f64_gpu as t; t._child(sys.argv[1])", path],
                               cwd=ROOT, env=env, capture_output=True, text=True, timeout=300)
        except subprocess.TimeoutExpired as ex:      # a hang: the child has been killed, the card is suspect
            pytest.exit("the PCFA_INSTNORM_FUSED=0 child hung and was killed after %g s: nothing more is started on the GPU\n%s"
                        % (ex.timeout, (ex.stderr or "")[-3000:]), returncode=1)
        if r.returncode < 0 or r.returncode in (134, 139):
            pytest.exit("the PCFA_INSTNORM_FUSED=0 child ended abnormally (%d): nothing more is started on the GPU\n%s"
                        % (r.returncode, r.stderr[-3000:]), returncode=1)
        assert r.returncode == 0, r.stderr[-3000:]
        theirs = torch.load(path)
    assert len(theirs) == 4
    for (name, relu), (y, mr, dx) in theirs.items():
        case = nm.CASES[name]
        p = nm.case_plan(case, fused=False)
        assert p.label == "two_vec" and p.chunks > 1
        nm.check_fwd(case, nm.EPS, relu, y, mr, p, record_property, "%s_relu%d_fwd_" % (name, relu))
        nm.check_bwd(case, nm.EPS, relu, "random", dx, p, record_property, "%s_relu%d_bwd_" % (name, relu))


# --------------------------------------------------------------------------- statuses; refusals write nothing
def test_instnorm_statuses():
    lib = _lib()
    case = nm.CASES["5x7x9"]
    P, n = case.planes, case.plane
    x, dy = nm.inputs(case), nm.gout(case)
    fx, fg, fy, fgx, fm = _in(x), _in(dy), _out(x.shape), _out(x.shape), _out((P, 2))
    nb = int(lib.pcfa_instnorm_workspace_bytes(P, n))
    ws, odd = _ws(nb), _ws(nb + 16, shift=1)
    every = [fx, fg, fy, fgx, fm, ws, odd]
    s = stream()

    def refused(status, want):
        torch.cuda.synchronize()
        assert status == want, (status, want)
        assert all(unchanged(f) for f in every), "a refused call touched a buffer"

    p = lambda f: f.ptr()   # noqa: E731
    fwd = lambda a=p(fx), b=p(fy), c=p(fm), w=p(ws), P_=P, n_=n, eps=1e-5: lib.pcfa_instnorm_fwd(a, b, c, w, P_, n_, eps, 1, s)   # noqa: E731
    bwd = lambda a=p(fx), m=p(fm), g=p(fg), o=p(fgx), w=p(ws), P_=P, n_=n: lib.pcfa_instnorm_bwd(a, m, g, o, w, P_, n_, 1, s)   # noqa: E731
    for k in "abcw":
        refused(fwd(**{k: None}), PCFA_ERR_INVALID_ARG)
    for k in "amgow":
        refused(bwd(**{k: None}), PCFA_ERR_INVALID_ARG)
    for kw in (dict(P_=0), dict(P_=-1), dict(n_=0), dict(n_=-5)):
        refused(fwd(**kw), PCFA_ERR_INVALID_ARG)
        refused(bwd(**kw), PCFA_ERR_INVALID_ARG)
    refused(fwd(eps=-1e-5), PCFA_ERR_INVALID_ARG)
    refused(fwd(eps=float("nan")), PCFA_ERR_INVALID_ARG)
    refused(fwd(w=p(odd)), PCFA_ERR_WORKSPACE)
    refused(bwd(w=p(odd)), PCFA_ERR_WORKSPACE)
    # planes is a grid's y extent: refused before any launch, whatever the buffers hold
    refused(fwd(P_=65536, n_=5), PCFA_ERR_UNSUPPORTED)
    refused(bwd(P_=65536, n_=5), PCFA_ERR_UNSUPPORTED)
    assert int(lib.pcfa_instnorm_workspace_bytes(0, n)) == 0 and int(lib.pcfa_instnorm_workspace_bytes(P, 0)) == 0
    for planes, plane in [(1, 1), (2048, 4096), (2049, 8193), (31, 262145), (65535, 5), (96, 28676)] + \
            [(c.planes, c.plane) for c in nm.TABLE]:
        assert int(lib.pcfa_instnorm_workspace_bytes(planes, plane)) == nm.plan(planes, plane).ws_bytes


# --------------------------------------------------------------------------- the exact kernels, bit for bit
def _exact_call(lib, name, tensors, n_out, shifts):
    ins = [_in(t, sh) for t, sh in zip(tensors, shifts)]
    outs = [_out(tensors[0].shape, sh) for sh in shifts[len(tensors):]]
    assert len(outs) == n_out
    n = tensors[0].numel()
    return _twice(lambda: getattr(lib, name)(*[f.ptr() for f in ins + outs], n, stream()), outs, ins)


@pytest.mark.parametrize("n", nm.EXACT_N)
def test_exact_kernels(record_property, n):
    """pcfa_add_relu_fwd, pcfa_relu_bwd, pcfa_relu_bwd2 against the torch expression, aligned and with each operand 4, 8 or
    12 bytes off in turn.  At the largest n the grid-stride loops of relu_bwd_kernel and relu_bwd2_kernel (2048 blocks) and of
    add_relu_kernel's scalar form wrap; add_relu_kernel's float4 loop (8192 blocks) would need more than 8.4 M floats, over
    the size limit of a test tensor, and does not wrap in any case.  Where a = b = -0 the sign of relu(-0) is left free
    (fmaxf(-0, 0) may return either zero; torch's CPU kernel returns -0): the value must be 0, the sign the device returns
    is recorded."""
    lib = _lib()
    a, b, out, out2, g = nm.exact_operands(n)
    for name, tensors, n_out, want in (("pcfa_add_relu_fwd", (a, b), 1, (nm.add_relu_ref(a, b),)),
                                       ("pcfa_relu_bwd", (out, g), 1, (nm.relu_bwd_ref(out, g),)),
                                       ("pcfa_relu_bwd2", (out, out2, g), 2, nm.relu_bwd2_ref(out, out2, g))):
        k = len(tensors) + n_out
        for shifts in [(0,) * k] + [tuple((1 + i) % 4 or 1 if j == i else 0 for j in range(k)) for i in range(k)]:
            got = _exact_call(lib, name, tensors, n_out, shifts)
            for gt, wt in zip(got, want):
                if name == "pcfa_add_relu_fwd":     # relu(-0): torch's own CPU and GPU kernels differ in the zero's sign
                    free = (a == 0) & (b == 0) & torch.signbit(a) & torch.signbit(b)
                    assert int(free.sum()) >= n // 11 and bool((gt[free] == 0).all())
                    record_property("add_relu_shifts%s_negative_zeros" % "".join(map(str, shifts)),
                                    "%d of %d" % (int(torch.signbit(gt[free]).sum()), int(free.sum())))
                    gt, wt = gt[~free], wt[~free]
                assert torch.equal(_bits(gt), _bits(wt)), (name, shifts)


def test_exact_kernels_statuses():
    lib = _lib()
    a, b, out, out2, g = nm.exact_operands(5)
    fa, fb, fo, fo2 = _in(a), _in(b), _out(a.shape), _out(a.shape)
    s = stream()
    p = lambda f: f.ptr()   # noqa: E731
    calls = [lib.pcfa_add_relu_fwd(None, p(fb), p(fo), 5, s), lib.pcfa_add_relu_fwd(p(fa), p(fb), None, 5, s),
             lib.pcfa_add_relu_fwd(p(fa), p(fb), p(fo), 0, s), lib.pcfa_relu_bwd(p(fa), None, p(fo), 5, s),
             lib.pcfa_relu_bwd(p(fa), p(fb), p(fo), 0, s), lib.pcfa_relu_bwd2(p(fa), p(fb), p(fb), p(fo), None, 5, s),
             lib.pcfa_relu_bwd2(p(fa), p(fb), p(fb), p(fo), p(fo2), -1, s)]
    torch.cuda.synchronize()
    assert calls == [PCFA_ERR_INVALID_ARG] * len(calls)
    assert all(unchanged(f) for f in (fa, fb, fo, fo2))
