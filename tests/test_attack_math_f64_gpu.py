"""The attack math through the C-ABI on fenced buffers (tests/fenced.py) against float64 (pcfa_amd/csrc/attack_math.hip): the reductions
pcfa_flow_loss_fwd, pcfa_avg_epe, pcfa_sum_squares, the loss gradient pcfa_flow_loss_bwd, and the element-wise
pcfa_box_transform_fwd / _bwd, pcfa_extract_deltas_fwd / _bwd, pcfa_extract_deltas_joint_fwd / _bwd, pcfa_pm1_pair_fwd / _bwd.
The references, emulations, case tables, census and the derivation of every bound are in tests/optim.py;
tests/test_optim_host_cpu.py shows on the CPU that the cases reach their classes, that the fp32 emulations pass every gate
and that one-line faults fail one.

Inputs sit between NaN (a strided operand's gaps are NaN too); outputs and the workspace (exactly
pcfa_flow_loss_workspace_bytes() long) are pre-filled with a sentinel NaN.  Each call checks (_twice): the status
(hip_ops._call raises on any but 0); every input and every fence bit-unchanged; no sentinel left in an output; a second call
from the same initial state gives identical bits (no atomics anywhere).  Ratios are junit properties.

Kernel by kernel:
  loss_partial_kernel / loss_final_kernel -- mode 0 on every loss case (a second trip over the pixels: crop_436; over the
    deltas: long_delta2; the crop, channels-last, zero-stride and 3-D views; n1 != n2), modes 1 and 2 and every sum of mode 0 on
    one-hot inputs at 0, 255, 256, 262143, 262144 and N - 1, which must come out exact.
  loss_bwd_flow_kernel -- the three f_type on every case with grad_loss 1 and 0.37; NaN exactly where float64 autograd's AEE
    has it.  Second trip of its grid-stride loop: bwd_second_trip (525,312 pixels > 524,288 threads).
  loss_bwd_delta_kernel -- above the bound, below it (exact zeros), the exact tie (half), a second trip (big_delta), joint.
  box_fwd_kernel, box_bwd_kernel, deltas_*_kernel, deltas_joint_*_kernel -- (2,3,300,301): second trip of the loops over all
    elements; (2,3,420,420): second trip of box_bwd_kernel's loop over a sample; (3,3,1,1), (1,1,1,5): one ragged wave.
  pm1_pair_fwd_kernel / _bwd_kernel -- (2,3,300,301) and (1,1,1,5), with and without grad_ctx.
"""
import ctypes

import numpy as np
import pytest
import torch

from oracle import ops as oracle_ops
from pcfa_amd import _hip, hip_ops
from tests import optim as op
from tests.fenced import NAN_BITS, PCFA_ERR_INVALID_ARG, SENTINEL, TINY, Fenced, gamma, stream
from tests.gates import dense_stride, unchanged

pytestmark = pytest.mark.gpu
torch.set_num_threads(min(16, torch.get_num_threads()))
_call = hip_ops._call
F32, F64 = torch.float32, torch.float64


def _lib():
    return _hip.load()


def _buf(shape, fill):
    shape = tuple(shape)
    return Fenced(shape, dense_stride(shape), fill)


def _in(t):
    return _buf(t.shape, NAN_BITS).write(t)


def _out(shape):
    return _buf(shape, SENTINEL)


def _bits(t):
    return t.contiguous().view(torch.int32)


def _ws():
    n = int(_lib().pcfa_flow_loss_workspace_bytes())
    assert n == 1024 * 8 * 4
    return _out((n // 4,))


def _twice(call, outs, ins, ws=None):
    """The per-call checks; the outputs of the first call on the CPU"""
    scratch = [ws] if ws is not None else []
    res = []
    for _ in range(2):
        for f in outs + scratch:
            f.buf.view(torch.int32).copy_(f.bits0)
        call()
        torch.cuda.synchronize()
        assert all(unchanged(f) for f in ins), "an input was written"
        assert all(f.fence_intact() for f in outs + scratch), "a store landed outside an output or the workspace"
        res.append([f.view().clone().cpu() for f in outs])
    for a, b in zip(*res):
        assert not bool((_bits(a) == SENTINEL).any()), "an element was never written"
        assert torch.equal(_bits(a), _bits(b)), "not repeatable bit for bit"
    return res[0]


class _Flow:
    """An optim.Operand on the device: its base between NaN, the pointer of its first element, its strides"""

    def __init__(self, o):
        self.f = _in(o.base)
        self.ptr = ctypes.c_void_p(self.f.ptr().value + 4 * o.off)
        self.strides = (ctypes.c_longlong * 4)(*o.stride)
        self.B, _, self.H, self.W = o.size


# --------------------------------------------------------------------------- reductions
@pytest.mark.parametrize("at", op.RED_ONE_HOT_AT)
def test_one_hot_sums_are_exact(at):
    """An element a reduction drops is invisible to a value gate over 2.7 M terms; alone it is the whole sum"""
    ws = _ws()
    x = torch.zeros(op.ONE_HOT_N)
    x[at] = 2.0 ** -3
    fx, out = _in(x), _out((1,))
    [s] = _twice(lambda: _call("pcfa_sum_squares", fx.ptr(), x.numel(), out.ptr(), ws.ptr()), [out], [fx], ws)
    assert float(s) == 2.0 ** -6
    B, _, H, W = op.ONE_HOT_FLOW
    npix = np.float32(B * H * W)
    d1 = _in(torch.zeros(4))
    for ch in (0, 1):
        p, t = torch.zeros(op.ONE_HOT_FLOW), torch.zeros(op.ONE_HOT_FLOW)
        p.view(2, -1)[ch, at], t.view(2, -1)[ch, at] = 4.0, 2.0
        fp, ft = _Flow(op.Operand(p)), _Flow(op.Operand(t))
        [e] = _twice(lambda: _call("pcfa_avg_epe", fp.ptr, fp.strides, ft.ptr, ft.strides, B, H, W, out.ptr(), ws.ptr()), [out],
                     [fp.f, ft.f], ws)
        assert np.float32(float(e)) == np.float32(2) / npix
        scal = _out((7,))
        for f_type, sim in (("aee", np.float32(2) / npix), ("mse", np.float32(4) / (np.float32(2) * npix)),
                            ("cosim", np.float32(1) - np.float32(8) / np.float32(4) * np.float32(2))):
            [v] = _twice(lambda: _call("pcfa_flow_loss_fwd", fp.ptr, fp.strides, ft.ptr, ft.strides, B, H, W, d1.ptr(), 4, d1.ptr(), 4,
                                       1.0, 0.0, _hip.PCFA_LOSS[f_type], scal.ptr(), ws.ptr()), [scal], [fp.f, ft.f, d1], ws)
            assert v.tolist()[3:6] == [8.0, 16.0, 4.0] and np.float32(v[1].item()) == sim and v[2].item() == 0.0


def _loss_fwd(case, f_type, mu=op.MU):
    po, to, d1, d2, bound = op.loss_case(case.name)
    fp, ft, f1, f2 = _Flow(po), _Flow(to), _in(d1), _in(d2)
    scal, ws = _out((7,)), _ws()
    [v] = _twice(lambda: _call("pcfa_flow_loss_fwd", fp.ptr, fp.strides, ft.ptr, ft.strides, fp.B, fp.H, fp.W, f1.ptr(), d1.numel(),
                               f2.ptr(), d2.numel(), bound, mu, _hip.PCFA_LOSS[f_type], scal.ptr(), ws.ptr()),
                 [scal], [fp.f, ft.f, f1, f2], ws)
    return v, (fp, ft, f1, f2)


@pytest.mark.parametrize("f_type", op.F_TYPES)
@pytest.mark.parametrize("case", op.LOSS_CASES, ids=lambda c: c.name)
def test_loss(record_property, case, f_type):
    """pcfa_flow_loss_fwd term by term, pcfa_flow_loss_bwd elementwise, against oracle.ops on double inputs"""
    name = case.name
    po, to, d1, d2, bound = op.loss_case(name)
    b = op.loss_bounds(name, f_type)
    v, (fp, ft, f1, f2) = _loss_fwd(case, f_type)
    ref, _, _, _ = op.loss_ref64(oracle_ops, name, f_type)
    r = {"sim": abs(float(v[1]) - ref["sim"]) / b["sim"], "msq": abs(float(v[2]) - ref["msq"]) / b["msq"],
         "loss": abs(float(v[0]) - ref["loss"]) / op.loss_total_bound(b, ref)}
    for k, i in (("pt", 3), ("pp", 4), ("tt", 5)):
        r[k] = abs(float(v[i]) - b["sums"][k]) / (gamma(b["D"] + 2 + op.TERM_R[k]) * b["abs"][k])
    for k, x in r.items():
        record_property(k + "_ratio", "%.3g" % x)
        assert x <= 1, (k, x)          # one by one: max() over a dict passes over a NaN that is not its first value
    assert bool(torch.isfinite(v).all()), v
    assert (float(v[6]) > 0, float(v[6]) == 0) == (case.regime == "above", case.regime == "tie")
    if case.regime == "tie":
        assert float(v[2]) == 0.25
    fscal = _in(v)
    B, H, W = fp.B, fp.H, fp.W
    for gl in op.GRAD_LOSSES:
        _, gp64, ga64, gb64 = op.loss_ref64(oracle_ops, name, f_type, gl)
        fgl = _in(torch.tensor([gl], dtype=F32))
        gp, g1, g2 = _out((B, 2, H, W)), _out((d1.numel(),)), _out((d2.numel(),))
        got = _twice(lambda: _call("pcfa_flow_loss_bwd", fp.ptr, fp.strides, ft.ptr, ft.strides, B, H, W, f1.ptr(), d1.numel(),
                                   f2.ptr(), d2.numel(), op.MU, _hip.PCFA_LOSS[f_type], 0, fscal.ptr(), fgl.ptr(), gp.ptr(),
                                   g1.ptr(), g2.ptr()), [gp, g1, g2], [fp.f, ft.f, f1, f2, fscal, fgl])
        kgp = got[0][0] if po.dims3 else got[0]
        nan = torch.isnan(gp64)
        assert torch.equal(torch.isnan(kgp), nan) and bool(torch.isfinite(kgp[~nan]).all()), "NaN elsewhere than float64 autograd"
        assert bool(nan.any()) == (f_type == "aee" and case.equal_pixels > 0)
        e = float(((kgp.double() - gp64).abs() / op.flow_grad_bound(name, f_type, gp64, gl))[~nan].max())
        record_property("grad_pred_ratio_gl%g" % gl, "%.3g" % e)
        assert e <= 1, e
        for tag, k_, w_ in (("d1", got[1], ga64), ("d2", got[2], gb64)):
            if case.regime == "below":
                assert float(k_.abs().max()) == 0.0 and float(w_.abs().max()) == 0.0
                continue
            e = float(((k_.double() - w_).abs() / (gamma(4) * w_.abs() + TINY)).max())
            record_property("grad_%s_ratio_gl%g" % (tag, gl), "%.3g" % e)
            assert e <= 1, (tag, e)
        if case.regime == "tie":        # half of the gradient above the bound, exactly
            full = np.float32(gl) * np.float32(op.MU) * np.float32(0.5) / np.float32(d1.numel() + d2.numel())
            assert torch.equal(got[1], torch.tensor(float(full)) * (2 * d1))


def test_joint_doubles_the_delta_gradient(record_property):
    """joint = 1 of the C-ABI doubles grad_delta1 bit for bit; the same tensor in both slots of the operator gives float64
    autograd's doubled gradient"""
    case = next(c for c in op.LOSS_CASES if c.name == "small")
    po, to, d1, _, bound = op.loss_case(case.name)
    fp, ft, f1 = _Flow(po), _Flow(to), _in(d1)
    scal, ws = _out((7,)), _ws()
    n = d1.numel()
    [v] = _twice(lambda: _call("pcfa_flow_loss_fwd", fp.ptr, fp.strides, ft.ptr, ft.strides, fp.B, fp.H, fp.W, f1.ptr(), n, f1.ptr(), n,
                               bound, op.MU, 1, scal.ptr(), ws.ptr()), [scal], [fp.f, ft.f, f1], ws)
    fscal, fgl = _in(v), _in(torch.tensor([0.37]))
    res = []
    for joint in (0, 1):
        g1 = _out((n,))
        res += _twice(lambda: _call("pcfa_flow_loss_bwd", fp.ptr, fp.strides, ft.ptr, ft.strides, fp.B, fp.H, fp.W, f1.ptr(), n,
                                    f1.ptr(), n, op.MU, 1, joint, fscal.ptr(), fgl.ptr(), None, g1.ptr(), None), [g1],
                      [fp.f, ft.f, f1, fscal, fgl])
    assert torch.equal(res[1], 2 * res[0]) and float(res[0].abs().max()) > 0
    p64, t64 = po.view().double(), to.view().double()
    x = d1.double().requires_grad_(True)
    oracle_ops.loss_delta_constraint(p64, t64, x, x, None, bound, op.MU, "mse").backward(torch.tensor(float(np.float32(0.37)), dtype=F64))
    xd = d1.cuda().requires_grad_(True)
    hip_ops.loss_delta_constraint(po.view().cuda(), to.view().cuda(), xd, xd, None, bound, op.MU, "mse").backward(
        torch.tensor(0.37, device="cuda"))
    e = float(((xd.grad.cpu().double() - x.grad).abs() / (gamma(5) * x.grad.abs() + TINY)).max())
    record_property("joint_ratio", "%.3g" % e)
    assert e <= 1 and torch.equal(xd.grad.cpu(), res[1])


def test_loss_refusals():
    lib = _lib()
    case = op.LOSS_CASES[1]
    po, to, d1, d2, bound = op.loss_case(case.name)
    fp, ft, f1, f2 = _Flow(po), _Flow(to), _in(d1), _in(d2)
    scal, ws, out = _out((7,)), _ws(), _out((1,))
    every = [fp.f, ft.f, f1, f2, scal, ws, out]
    s = stream()

    def refused(status):
        torch.cuda.synchronize()
        assert status == PCFA_ERR_INVALID_ARG, status
        assert all(unchanged(f) for f in every), "a refused call touched a buffer"

    def fwd(p=fp.ptr, B=fp.B, H=fp.H, n1=d1.numel(), ft_=0, w=ws.ptr()):
        return lib.pcfa_flow_loss_fwd(p, fp.strides, ft.ptr, ft.strides, B, H, fp.W, f1.ptr(), n1, f2.ptr(), d2.numel(), bound, op.MU,
                                      ft_, scal.ptr(), w, s)
    for kw in (dict(p=None), dict(B=0), dict(H=0), dict(n1=0), dict(ft_=3), dict(ft_=-1), dict(w=None)):
        refused(fwd(**kw))
    refused(lib.pcfa_avg_epe(fp.ptr, fp.strides, ft.ptr, ft.strides, fp.B, fp.H, 0, out.ptr(), ws.ptr(), s))
    refused(lib.pcfa_avg_epe(fp.ptr, fp.strides, None, ft.strides, fp.B, fp.H, fp.W, out.ptr(), ws.ptr(), s))
    refused(lib.pcfa_sum_squares(f1.ptr(), 0, out.ptr(), ws.ptr(), s))
    refused(lib.pcfa_sum_squares(f1.ptr(), d1.numel(), None, ws.ptr(), s))
    refused(lib.pcfa_flow_loss_bwd(fp.ptr, fp.strides, ft.ptr, ft.strides, fp.B, fp.H, fp.W, f1.ptr(), d1.numel(), f2.ptr(), d2.numel(),
                                   op.MU, 5, 0, scal.ptr(), out.ptr(), None, None, None, s))
    refused(lib.pcfa_flow_loss_bwd(fp.ptr, fp.strides, ft.ptr, ft.strides, fp.B, fp.H, fp.W, f1.ptr(), d1.numel(), f2.ptr(), d2.numel(),
                                   op.MU, 0, 0, None, out.ptr(), None, None, None, s))


@pytest.mark.parametrize("case", [c for c in op.LOSS_CASES if c.name in ("small", "flow3d", "crop_436", "channels_last", "expanded_target")],
                         ids=lambda c: c.name)
def test_avg_epe_and_sum_squares(record_property, case):
    po, to, d1, d2, _ = op.loss_case(case.name)
    b = op.loss_bounds(case.name, "aee")
    fp, ft, out, ws = _Flow(po), _Flow(to), _out((1,)), _ws()
    [e] = _twice(lambda: _call("pcfa_avg_epe", fp.ptr, fp.strides, ft.ptr, ft.strides, fp.B, fp.H, fp.W, out.ptr(), ws.ptr()), [out],
                 [fp.f, ft.f], ws)
    want = float(oracle_ops.avg_epe(po.view().double(), to.view().double()))
    record_property("avg_epe_ratio", "%.3g" % (abs(float(e) - want) / b["sim"]))
    assert abs(float(e) - want) <= b["sim"]
    x = po.view().contiguous().reshape(-1)          # a dense vector of the flow's size: 892,928 elements for the crop
    fx = _in(x)
    [s_] = _twice(lambda: _call("pcfa_sum_squares", fx.ptr(), x.numel(), out.ptr(), ws.ptr()), [out], [fx], ws)
    want = float((x.double() ** 2).sum())
    bd = gamma(op.red_depth(x.numel()) + 2 + op.TERM_R["d"]) * want
    record_property("sum_squares_ratio", "%.3g" % (abs(float(s_) - want) / bd))
    assert abs(float(s_) - want) <= bd


# --------------------------------------------------------------------------- element-wise kernels
def _ids(s):
    return "x".join(map(str, s))


def _box(image, delta, go, cov, eps, scale):
    """(out, grad_image, grad_delta) of pcfa_box_transform_fwd / _bwd, each call checked"""
    B, n = image.shape[0], image[0].numel()
    fi, fgo = _in(image), _in(go)
    fdl = None if delta is None else _in(delta)
    pd = None if delta is None else fdl.ptr()
    ins = [fi, fgo] + ([] if delta is None else [fdl])
    o, gi, gd = _out(image.shape), _out(image.shape), _out((1,) + image.shape[1:])
    [out] = _twice(lambda: _call("pcfa_box_transform_fwd", fi.ptr(), pd, o.ptr(), B, n, int(cov), eps, scale), [o], ins)
    outs = [gi] + ([] if delta is None else [gd])
    got = _twice(lambda: _call("pcfa_box_transform_bwd", fi.ptr(), pd, fgo.ptr(), gi.ptr(), None if delta is None else gd.ptr(), B, n,
                               int(cov), eps, scale), outs, ins)
    return out, got[0], (got[1] if delta is not None else None)


@pytest.mark.parametrize("shape", op.EW_SHAPES, ids=_ids)
def test_clipping_is_bit_exact(shape):
    """Multiples of 1/64 with 0 and 1 among them: forward and gradients bit-equal to float64 rounded, pass-through on the edges"""
    n = int(np.prod(shape))
    for with_delta in (False, True):
        image, delta, go = op.clip_inputs(shape, with_delta)
        for scale in (1.0, 255.0):
            out, gi, gd = _box(image, delta, go, False, 0.0, scale)
            wi, wd = op.box_bwd(image, delta, go, False, 0., scale, F64)
            assert torch.equal(_bits(out), _bits(op.box_fwd(image, delta, False, 0., scale, F64).float()))
            assert torch.equal(_bits(gi), _bits(wi.float())) and (gd is None or torch.equal(_bits(gd), _bits(wd.float())))
        w = image + delta if with_delta else image
        img = op.clip_inputs(shape, True)[0]
        fw, fi, fgo, o, gw = _in(w), _in(img), _in(go), _out(shape), _out(shape)
        [dl] = _twice(lambda: _call("pcfa_extract_deltas_fwd", fw.ptr(), fi.ptr(), o.ptr(), n, 0, 0.0), [o], [fw, fi])
        [g] = _twice(lambda: _call("pcfa_extract_deltas_bwd", fw.ptr(), fgo.ptr(), gw.ptr(), n, 0, 0.0), [gw], [fw, fgo])
        assert torch.equal(_bits(dl), _bits(op.deltas_fwd(w, img, False, 0., F64).float()))
        assert torch.equal(_bits(g), _bits(op.deltas_bwd(w, go, False, 0., F64).float()))


@pytest.mark.parametrize("shape", op.EW_SHAPES, ids=_ids)
def test_joint_is_bit_exact(shape):
    n = int(np.prod(shape))
    nd, imax, imin, go = op.joint_inputs(shape)
    fn, fx, fm, fgo, o, g = _in(nd), _in(imax), _in(imin), _in(go), _out(shape), _out(shape)
    [dl] = _twice(lambda: _call("pcfa_extract_deltas_joint_fwd", fn.ptr(), fx.ptr(), fm.ptr(), o.ptr(), n), [o], [fn, fx, fm])
    [gn] = _twice(lambda: _call("pcfa_extract_deltas_joint_bwd", fn.ptr(), fx.ptr(), fm.ptr(), fgo.ptr(), g.ptr(), n), [g],
                  [fn, fx, fm, fgo])
    assert torch.equal(_bits(dl), _bits(op.joint_fwd(nd, imax, imin, F64).float()))
    assert torch.equal(_bits(gn), _bits(op.joint_bwd(nd, imax, imin, go, F64).float()))


@pytest.mark.parametrize("shape", op.EW_SHAPES, ids=_ids)
def test_change_of_variables(record_property, shape):
    """Interior, saturated and infinite arguments, no element excluded: forward within 2e-7 (x scale), gradient within the
    bound from the measured tanh error, exactly 0 at saturation"""
    n = int(np.prod(shape))
    worst = {}
    for with_delta in (False, True):
        image, delta, go, _ = op.cov_inputs(shape, with_delta)
        x = image + delta if with_delta else image
        sat = x.abs() >= 12
        e_t = op.tanh_error(x)
        for eps in (0.0, 1e-7):
            k = op.box_k_c(eps, F64)[0]
            for scale in (1.0, 255.0):
                out, gi, gd = _box(image, delta, go, True, eps, scale)
                want = op.box_fwd(image, delta, True, eps, scale, F64)
                assert bool(torch.isfinite(out).all()), "the forward is not finite at a saturated or infinite argument"
                op.fold(worst, "fwd", op.worst_ratio(out, want, 2e-7 * scale))
                wi, wd = op.box_bwd(image, delta, go, True, eps, scale, F64)
                bi = op.cov_grad_bound(x, go * scale, k, wi, e_t)
                op.fold(worst, "grad", op.worst_ratio(gi, wi, bi))
                assert float(gi[sat].abs().max()) == 0.0
                if gd is not None:
                    bd = bi.sum(0, keepdim=True) + gamma(shape[0]) * wi.abs().sum(0, keepdim=True)
                    op.fold(worst, "grad_delta", op.worst_ratio(gd, wd, bd))
            img = op.clip_inputs(shape, True)[0]
            fw, fi, fgo, o, gw = _in(x), _in(img), _in(go), _out(shape), _out(shape)
            [dl] = _twice(lambda: _call("pcfa_extract_deltas_fwd", fw.ptr(), fi.ptr(), o.ptr(), n, 1, eps), [o], [fw, fi])
            [g] = _twice(lambda: _call("pcfa_extract_deltas_bwd", fw.ptr(), fgo.ptr(), gw.ptr(), n, 1, eps), [gw], [fw, fgo])
            assert bool(torch.isfinite(dl).all()), "the forward is not finite at a saturated or infinite argument"
            op.fold(worst, "deltas_fwd", op.worst_ratio(dl, op.deltas_fwd(x, img, True, eps, F64), 2e-7))
            wg = op.deltas_bwd(x, go, True, eps, F64)
            op.fold(worst, "deltas_grad", op.worst_ratio(g, wg, op.cov_grad_bound(x, go, k, wg, e_t)))
            assert float(g[sat].abs().max()) == 0.0
    for k_, v in worst.items():
        record_property(k_ + "_ratio", "%.3g" % v)
    assert set(worst) == {"fwd", "grad", "grad_delta", "deltas_fwd", "deltas_grad"}


@pytest.mark.parametrize("shape", (op.EW_SHAPES[0], op.EW_SHAPES[3]), ids=_ids)
def test_pm1_pair_is_torch_bit_for_bit(shape):
    gen = torch.Generator().manual_seed(shape[-1])
    B, n = shape[0], int(np.prod(shape[1:]))
    a, b = (255 * torch.rand(shape, generator=gen) for _ in range(2))
    gpair, gctx = torch.randn((2 * B,) + shape[1:], generator=gen), torch.randn(shape, generator=gen)
    fa, fb, pair, ctx = _in(a), _in(b), _out((2 * B,) + shape[1:]), _out(shape)
    kp, kc = _twice(lambda: _call("pcfa_pm1_pair_fwd", fa.ptr(), fb.ptr(), pair.ptr(), ctx.ptr(), B, n), [pair, ctx], [fa, fb])
    ad, bd = a.cuda().requires_grad_(True), b.cuda().requires_grad_(True)
    wp, wc = oracle_ops.pm1_pair(ad, bd)
    assert torch.equal(_bits(kp), _bits(wp.detach().cpu())) and torch.equal(_bits(kc), _bits(wc.detach().cpu()))
    fgp, fgc = _in(gpair), _in(gctx)
    for with_ctx in (True, False):
        ga, gb = _out(shape), _out(shape)
        ka, kb = _twice(lambda: _call("pcfa_pm1_pair_bwd", fgp.ptr(), fgc.ptr() if with_ctx else None, ga.ptr(), gb.ptr(), B, n),
                        [ga, gb], [fgp, fgc])
        outs, grads = ((wp, wc), (gpair.cuda(), gctx.cuda())) if with_ctx else ((wp,), (gpair.cuda(),))
        wa, wb = torch.autograd.grad(outs, (ad, bd), grads, retain_graph=True)
        assert torch.equal(_bits(ka), _bits(wa.cpu())) and torch.equal(_bits(kb), _bits(wb.cpu()))
