"""SpyNet operators (Config.spynet_ops = "hip"): the 7x7 convolutions of Basic (models/SpyNet/SpyNet.py:56-84) with their data
gradients, and the clamped backward warp (SpyNet.py:86-102) with a deterministic backward.  The flow up-sampling is
ops.pwc.upsample_bilinear (gather backward)."""
import ctypes

import numpy as np
import torch

from .. import _hip
from .core import _call, _dev, _ptr, cached_pack, scratch_for
from .flownet2 import gather_pack, gather_tile

__all__ = ["conv7x7", "conv7x7_dgrad_weight", "conv7x7_pack", "conv7x7_tile", "spynet_warp", "spynet_warp_scales"]

conv7x7_tile = gather_tile   # pcfa_conv7x7 is the 7x7 / stride-1 instance of pcfa_conv_gather: one tile rule, one packer


def conv7x7_dgrad_weight(w):
    """The weight whose 7x7 / pad 3 convolution of grad_out is the data gradient of conv2d(., w, padding=3): rotated by 180
    degrees and channel-transposed, [Cout, Cin, 7, 7] -> [Cin, Cout, 7, 7]."""
    return w.transpose(0, 1).flip(2, 3)


def conv7x7_pack(w):
    """[Cout, Cin, 7, 7] -> pcfa_conv7x7's operand order (flat): [Cout/cot][Cin/4][cot/mt][4/ks][7][7][ks][mt], ks = 64/mt
    k per MFMA step; Cout is padded to cot and Cin to 4 with zeros (ops.flownet2.gather_pack of one 7x7 window)."""
    return gather_pack(w)


def _conv7_packed(weight):
    """(forward, data-gradient) packs of a frozen 7x7 weight, cached per tensor version."""
    def make(w):
        lib = _hip.load()
        w = w.float()
        fwd, bwd = conv7x7_pack(w), conv7x7_pack(conv7x7_dgrad_weight(w))
        cout, cin = w.shape[:2]
        for p, (ci, co) in ((fwd, (cin, cout)), (bwd, (cout, cin))):
            mt, cot = ctypes.c_int(), ctypes.c_int()
            _hip.check(lib.pcfa_conv7x7_tile(co, ctypes.byref(mt), ctypes.byref(cot)), "pcfa_conv7x7_tile")
            if (mt.value, cot.value) != conv7x7_tile(co) or p.numel() != int(lib.pcfa_conv7x7_packed_floats(ci, co)):
                raise RuntimeError("conv7x7: host packing does not match the library's tiling")
        return fwd, bwd
    return cached_pack("conv7x7", (weight,), make)


class _Conv7x7(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, weight, bias, relu, addend):
        x = x.contiguous()
        B, cin, H, W = x.shape
        cout = weight.shape[0]
        fwd, bwd = _conv7_packed(weight)
        out = torch.empty((B, cout, H, W), device=x.device, dtype=torch.float32)
        if addend is not None:
            addend = addend.contiguous()
        _call("pcfa_conv7x7", _ptr(x), None, _ptr(fwd), _ptr(bias), _ptr(addend), _ptr(out), B, cin, cout, H, W,
              int(bool(relu)))
        ctx.relu, ctx.has_addend = bool(relu), addend is not None
        ctx.dims = (B, cin, cout, H, W)
        ctx.pack = bwd
        if relu:
            ctx.save_for_backward(out)
        return out

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, g):
        if ctx.needs_input_grad[1] or ctx.needs_input_grad[2]:
            raise RuntimeError("conv7x7 is the frozen-weight path: no weight / bias gradient")
        B, cin, cout, H, W = ctx.dims
        g = g.contiguous()
        mask = ctx.saved_tensors[0] if ctx.relu else None
        gx = None
        if ctx.needs_input_grad[0]:
            gx = torch.empty((B, cin, H, W), device=g.device, dtype=torch.float32)
            _call("pcfa_conv7x7", _ptr(g), _ptr(mask), _ptr(ctx.pack), None, None, _ptr(gx), B, cout, cin, H, W, 0)
        return gx, None, None, None, (g if ctx.has_addend and ctx.needs_input_grad[4] else None)


def conv7x7(x, weight, bias=None, relu=False, addend=None):
    """act(conv2d(x, weight, bias, padding=3)) [+ addend] for a frozen [Cout, Cin, 7, 7] weight (SpyNet's Basic layers; the
    last one adds the up-sampled flow, SpyNet.py:153, as `addend`).  Backward: the data gradient (and addend's identity);
    the ReLU backward is applied where the gradient is loaded.  Fixed summation order, no atomics."""
    _dev(x, weight, bias, addend)
    if weight.requires_grad or (bias is not None and bias.requires_grad):
        raise RuntimeError("conv7x7: frozen parameters only")
    if weight.dim() != 4 or tuple(weight.shape[2:]) != (7, 7) or x.dim() != 4 or x.shape[1] != weight.shape[1]:
        raise ValueError("conv7x7: weight %s does not fit input %s" % (tuple(weight.shape), tuple(x.shape)))
    if x.dtype != torch.float32 or weight.dtype != torch.float32:
        raise ValueError("conv7x7: float32 only")
    if relu and addend is not None:
        raise ValueError("conv7x7: relu and addend are not combined (no SpyNet layer has both)")
    if addend is not None and tuple(addend.shape) != (x.shape[0], weight.shape[0]) + tuple(x.shape[2:]):
        raise ValueError("conv7x7: addend %s does not fit the output" % (tuple(addend.shape),))
    return _Conv7x7.apply(x, weight, bias, bool(relu), addend)


def spynet_warp_scales(H, W):
    """(sx, sy): fp32 1 / ((W - 1) / 2) and 1 / ((H - 1) / 2) -- what ATen's GPU division of the flow by the Python scalar
    (W - 1.0) / 2.0 multiplies by (the scalar cast to fp32, its reciprocal taken in fp32)."""
    one = np.float32(1.0)
    return float(one / np.float32((W - 1.0) / 2.0)), float(one / np.float32((H - 1.0) / 2.0))


class _SpyNetWarp(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, flo, hor, ver):
        x, flo = x.contiguous(), flo.contiguous()
        hor, ver = hor.contiguous(), ver.contiguous()
        B, C, H, W = x.shape
        sx, sy = spynet_warp_scales(H, W)
        out = torch.empty_like(x)
        ctx.params = (B, C, H, W, sx, sy)
        _call("pcfa_spynet_warp_fwd", _ptr(x), _ptr(flo), _ptr(hor), _ptr(ver), _ptr(out), *ctx.params)
        ctx.save_for_backward(x, flo, hor, ver)
        return out

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, g):
        x, flo, hor, ver = ctx.saved_tensors
        B, C, H, W, sx, sy = ctx.params
        g = g.contiguous()
        gx, gf = torch.empty_like(x), torch.empty_like(flo)
        ws, nws = scratch_for("pcfa_spynet_warp_bwd_workspace_bytes", (B, C, H, W), x.device)
        _call("pcfa_spynet_warp_bwd", _ptr(x), _ptr(flo), _ptr(hor), _ptr(ver), _ptr(g), _ptr(gx), _ptr(gf), _ptr(ws), nws,
              *ctx.params)
        return gx, gf, None, None


def spynet_warp(x, flo, hor=None, ver=None):
    """SpyNet's backward_warp (nets/spynet.py, SpyNet.py:86-102): grid_sample(x, clamp(linspace grid + flo / ((W-1)/2), -1, 1))
    with bilinear taps, zero padding, align_corners=False.  hor / ver: the linspace(-1, 1, W) / (-1, 1, H) vectors (made
    here when not given).  Backward: fixed-point scatter for x, gather through the clamp mask for flo -- bit-reproducible."""
    _dev(x, flo)
    if x.dim() != 4 or tuple(flo.shape) != (x.shape[0], 2) + tuple(x.shape[2:]):
        raise ValueError("spynet_warp: flow %s does not match features %s" % (tuple(flo.shape), tuple(x.shape)))
    H, W = x.shape[2:]
    if hor is None:
        hor = torch.linspace(-1.0, 1.0, W, device=x.device)
    if ver is None:
        ver = torch.linspace(-1.0, 1.0, H, device=x.device)
    if hor.numel() != W or ver.numel() != H:
        raise ValueError("spynet_warp: linspace vectors of %d / %d elements for a %dx%d plane" % (hor.numel(), ver.numel(), H, W))
    return _SpyNetWarp.apply(x, flo, hor, ver)
