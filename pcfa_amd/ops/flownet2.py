"""FlowNet2 operators of Config.flownet2_ops = "hip" (models/FlowNet/submodules.py:7-36, FlowNet2.py:115-177): the stride-2
convolutions and ConvTranspose2d(4, 2, 1) layers with LeakyReLU, both directions on pcfa_conv_gather (the existing
pcfa_conv_s2 kernels where they apply), Resample2d with a fixed-point backward, the nearest x4 flow up-sampling and the
LeakyReLU of conv_redir.  No atomics on float data and no library kernel: the same bits on every call.

The weight transforms are plain tensor ops (tested on the host in float64):
  gather_pack        [Cout, Cin, T, T] (or [4, Cout, Cin, T, T]) -> pcfa_conv_gather's operand order;
  parity_weights     a stride-2 transposed convolution as four stride-1 T x T sub-kernels, one per output parity;
  parity_offsets     the input offset of each parity's window.
"""
import torch

from .. import _hip
from .core import _call, _dev, _ptr, cached_pack, scratch_for

__all__ = ["GATHER_CK", "gather_tile", "gather_pack", "parity_offsets", "parity_weights", "conv_s2_leaky",
           "deconv4s2_leaky", "resample2d_det", "upsample_nearest4", "leaky_relu", "conv_s2_leaky_covers"]

GATHER_CK = 4   # input channels per chunk of pcfa_conv_gather and pcfa_conv7x7 (include/pcfa_hip.h)


def gather_tile(cout):
    """(mt, cot) of pcfa_conv_gather / pcfa_conv7x7 for `cout` output channels: MFMA rows per tile and output channels per
    workgroup (the library's rule, checked against it by ops.spynet)."""
    return (16, 16) if cout <= 16 else (32, 32) if cout <= 32 else (32, 64)


def gather_pack(w):
    """[Cout, Cin, T, T] (one window) or [npar, Cout, Cin, T, T] -> flat [npar][Cout/cot][Cin/4][cot/mt][4/ks][T][T][ks][mt],
    ks = 64 / mt; Cout padded to cot and Cin to 4 with zeros."""
    if w.dim() == 4:
        w = w.unsqueeze(0)
    npar, cout, cin, t, _ = (int(s) for s in w.shape)
    mt, cot = gather_tile(cout)
    ks = 64 // mt
    cop, cip = -(-cout // cot) * cot, -(-cin // GATHER_CK) * GATHER_CK
    wp = w.new_zeros((npar, cop, cip, t * t))
    wp[:, :cout, :cin] = w.reshape(npar, cout, cin, t * t)
    wp = wp.view(npar, cop // cot, cot // mt, mt, cip // GATHER_CK, GATHER_CK // ks, ks, t * t)
    return wp.permute(0, 1, 4, 2, 5, 7, 6, 3).contiguous().view(-1)


def parity_offsets(k, pad):
    """(off_0, off_1): output row 2 a + r of a stride-2 transposed k x k convolution with padding `pad` reads input rows
    a + off_r .. a + off_r + T - 1 (T = ceil(k / 2)); off_r = ceil((r + pad - k + 1) / 2)."""
    return tuple(-((k - 1 - r - pad) // 2) for r in (0, 1))


def parity_weights(w, pad):
    """The four stride-1 sub-kernels of conv_transpose2d(., w, stride=2, padding=pad) for w: [Cin, Cout, k, k] (a
    ConvTranspose2d weight, or the weight of the stride-2 Conv2d whose data gradient is wanted: the same operation).
    Returns [4, Cout, Cin, T, T], parity p = 2 ry + rx: tap (ty, tx) of parity (ry, rx) is w[.., ry + pad - 2 (off_ry + ty),
    rx + pad - 2 (off_rx + tx)] (zero where that leaves the kernel: the shorter parities of an odd k)."""
    k = int(w.shape[-1])
    t = (k + 1) // 2
    offs = parity_offsets(k, pad)
    a = w.transpose(0, 1)   # [Cout, Cin, k, k]: output channels first
    out = w.new_zeros((4,) + tuple(a.shape[:2]) + (t, t))
    for ry in (0, 1):
        for rx in (0, 1):
            for ty in range(t):
                ky = ry + pad - 2 * (offs[ry] + ty)
                if not 0 <= ky < k:
                    continue
                for tx in range(t):
                    kx = rx + pad - 2 * (offs[rx] + tx)
                    if 0 <= kx < k:
                        out[2 * ry + rx, :, :, ty, tx] = a[:, :, ky, kx]
    return out


def _checked(packed, cin, cout, taps, npar):
    lib = _hip.load()
    if packed.numel() != int(lib.pcfa_conv_gather_packed_floats(cin, cout, taps, npar)):
        raise RuntimeError("conv_gather: host packing does not match the library's tiling")
    return packed


def _gather(x, mask, mask_slope, packed, bias, out, cin, cout, stride, taps, npar, offs, act, slope):
    B, _, H, W = x.shape
    _call("pcfa_conv_gather", _ptr(x), _ptr(mask), float(mask_slope), _ptr(packed), _ptr(bias), _ptr(out), B, cin, H, W,
          cout, out.shape[2], out.shape[3], stride, taps, npar, offs[0], offs[1], act, float(slope))


def _aligned(t):
    t = t.contiguous()
    return t if t.data_ptr() % 16 == 0 else t.clone()


def conv_s2_leaky_covers(k, H, W):
    """True when conv_s2_leaky runs a k x k stride-2 layer on an H x W input (every size for k in {3, 5, 7})."""
    return k in (3, 5, 7) and H >= 1 and W >= 1


class _ConvS2Leaky(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, weight, bias, slope):
        x = _aligned(x)
        B, cin, H, W = x.shape
        cout, _, k, _ = weight.shape
        pad = k // 2
        OH, OW = (H + 2 * pad - k) // 2 + 1, (W + 2 * pad - k) // 2 + 1
        lib = _hip.load()
        out = torch.empty((B, cout, OH, OW), device=x.device, dtype=torch.float32)
        if lib.pcfa_conv_s2_supported(cin, cout, k, H, W):   # the existing fast path (3-channel stem, 3x3 with W % 4 == 0)
            from .conv import _s2_packed
            _call("pcfa_conv_s2_fwd", _ptr(x), _ptr(_s2_packed(weight)), _ptr(bias), _ptr(out), B, cin, cout, H, W, k, 2,
                  float(slope))
        else:
            fwd = cached_pack("s2f", (weight,), lambda w: _checked(gather_pack(w), cin, cout, k, 1))
            _gather(x, None, 0., fwd, bias, out, cin, cout, 2, k, 1, (-pad, 0), 2, slope)
        ctx.slope, ctx.xshape = float(slope), tuple(x.shape)
        ctx.save_for_backward(weight, out)
        return out

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, g):
        if ctx.needs_input_grad[1] or ctx.needs_input_grad[2]:
            raise RuntimeError("conv_s2_leaky is the frozen-weight path: no weight / bias gradient")
        weight, out = ctx.saved_tensors
        B, cin, H, W = ctx.xshape
        cout, _, k, _ = weight.shape
        g = _aligned(g)
        gx = torch.empty(ctx.xshape, device=g.device, dtype=torch.float32)
        lib = _hip.load()
        if lib.pcfa_conv_s2_bwd_supported(cin, cout, k, H, W):
            from .conv import _act_bwd, _s2_bwd_packed
            gm = _act_bwd(out, g, 2, ctx.slope)
            _call("pcfa_conv_s2_bwd", _ptr(gm), _ptr(_s2_bwd_packed(weight)), _ptr(gx), B, cin, cout, H, W, k)
        else:
            t = (k + 1) // 2
            bwd = cached_pack("s2b", (weight,),
                              lambda w: _checked(gather_pack(parity_weights(w, k // 2)), cout, cin, t, 4))
            _gather(g, out, ctx.slope, bwd, None, gx, cout, cin, 1, t, 4, parity_offsets(k, k // 2), 0, 0.)
        return gx, None, None, None


def conv_s2_leaky(x, weight, bias, slope=0.1):
    """leaky_relu(conv2d(x, weight, bias, stride=2, padding=k//2), slope) for a frozen k x k weight, k in {3, 5, 7} (FlowNet's
    conv(..., stride=2)).  Data gradient: the LeakyReLU backward applied where the gradient is loaded, then the parity
    kernel.  The pcfa_conv_s2 kernels take the shapes they cover."""
    _dev(x, weight, bias)
    if weight.requires_grad or (bias is not None and bias.requires_grad):
        raise RuntimeError("conv_s2_leaky: frozen parameters only")
    if weight.dim() != 4 or x.dim() != 4 or x.shape[1] != weight.shape[1] or weight.shape[2] != weight.shape[3]:
        raise ValueError("conv_s2_leaky: weight %s does not fit input %s" % (tuple(weight.shape), tuple(x.shape)))
    if not conv_s2_leaky_covers(int(weight.shape[2]), int(x.shape[2]), int(x.shape[3])):
        raise ValueError("conv_s2_leaky: no own kernel for a %dx%d stride-2 layer on a %dx%d map"
                         % (weight.shape[2], weight.shape[3], x.shape[2], x.shape[3]))
    if x.dtype != torch.float32 or weight.dtype != torch.float32:
        raise ValueError("conv_s2_leaky: float32 only")
    return _ConvS2Leaky.apply(x, weight, bias, float(slope))


class _Deconv4s2Leaky(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, weight, bias, slope):
        x = _aligned(x)
        B, cin, H, W = x.shape
        cout = int(weight.shape[1])
        fwd = cached_pack("dcf", (weight,), lambda w: _checked(gather_pack(parity_weights(w, 1)), cin, cout, 2, 4))
        out = torch.empty((B, cout, 2 * H, 2 * W), device=x.device, dtype=torch.float32)
        _gather(x, None, 0., fwd, bias, out, cin, cout, 1, 2, 4, parity_offsets(4, 1), 2, slope)
        ctx.slope, ctx.xshape = float(slope), tuple(x.shape)
        ctx.save_for_backward(weight, out)
        return out

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, g):
        if ctx.needs_input_grad[1] or ctx.needs_input_grad[2]:
            raise RuntimeError("deconv4s2_leaky is the frozen-weight path: no weight / bias gradient")
        weight, out = ctx.saved_tensors
        B, cin, H, W = ctx.xshape
        cout = int(weight.shape[1])
        g = _aligned(g)
        # the data gradient of conv_transpose2d(., w, stride 2, padding 1) is conv2d(., w, stride 2, padding 1): w as it is
        bwd = cached_pack("dcb", (weight,), lambda w: _checked(gather_pack(w), cout, cin, 4, 1))
        gx = torch.empty(ctx.xshape, device=g.device, dtype=torch.float32)
        _gather(g, out, ctx.slope, bwd, None, gx, cout, cin, 2, 4, 1, (-1, 0), 0, 0.)
        return gx, None, None, None


def deconv4s2_leaky(x, weight, bias, slope=0.1):
    """leaky_relu(conv_transpose2d(x, weight, bias, stride=2, padding=1), slope) for a frozen [Cin, Cout, 4, 4] weight
    (FlowNet's deconv(), submodules.py:36).  Forward: four 2x2 parity windows; data gradient: a stride-2 4x4 gather with
    the LeakyReLU backward applied where the gradient is loaded."""
    _dev(x, weight, bias)
    if weight.requires_grad or (bias is not None and bias.requires_grad):
        raise RuntimeError("deconv4s2_leaky: frozen parameters only")
    if weight.dim() != 4 or tuple(weight.shape[2:]) != (4, 4) or x.dim() != 4 or x.shape[1] != weight.shape[0]:
        raise ValueError("deconv4s2_leaky: weight %s does not fit input %s" % (tuple(weight.shape), tuple(x.shape)))
    if x.dtype != torch.float32 or weight.dtype != torch.float32:
        raise ValueError("deconv4s2_leaky: float32 only")
    return _Deconv4s2Leaky.apply(x, weight, bias, float(slope))


class _Resample2dDet(torch.autograd.Function):
    @staticmethod
    def forward(ctx, input1, input2):
        B, C, H, W = input1.shape
        out = torch.empty((B, C, H, W), device=input1.device, dtype=torch.float32)
        ctx.dims = (B, C, H, W)
        _call("pcfa_resample2d_fwd", _ptr(input1), _ptr(input2), _ptr(out), B, C, H, W, H, W, 1, 1)
        ctx.save_for_backward(input1, input2)
        return out

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, g):
        input1, input2 = ctx.saved_tensors
        B, C, H, W = ctx.dims
        g = g.contiguous()
        g1, g2 = torch.empty_like(input1), torch.empty_like(input2)
        ws, nws = scratch_for("pcfa_resample2d_bwd_det_workspace_bytes", (B, C, H, W), g.device)
        _call("pcfa_resample2d_bwd_det", _ptr(input1), _ptr(input2), _ptr(g), _ptr(g1), _ptr(g2), _ptr(ws), nws, B, C, H, W)
        return g1, g2


def resample2d_det(input1, input2):
    """Resample2d (kernel_size 1, bilinear; ops.flownet.resample2d's forward) whose input gradient is a fixed-point int64
    scatter (unit 2^(floor(log2 max|grad_out|) - 40), pcfa_resample2d_bwd_det) instead of fp32 atomics: the same bits on
    every call.  input1 must have the flow's size (FlowNet2 warps full-size images)."""
    _dev(input1, input2)
    input1, input2 = input1.contiguous(), input2.contiguous()
    if input1.dim() != 4 or tuple(input2.shape) != (input1.shape[0], 2) + tuple(input1.shape[2:]):
        raise ValueError("resample2d_det: flow %s does not match input %s" % (tuple(input2.shape), tuple(input1.shape)))
    return _Resample2dDet.apply(input1, input2)


class _UpsampleNearest4(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, s, div):
        x = x.contiguous()
        B, C, H, W = x.shape
        out = torch.empty((B, C, 4 * H, 4 * W), device=x.device, dtype=torch.float32)
        _call("pcfa_upsample_nearest4_fwd", _ptr(x), _ptr(out), B * C, H, W, s, int(div))
        ctx.dims = (B, C, H, W, s, int(div))
        return out

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, g):
        B, C, H, W, s, div = ctx.dims
        g = g.contiguous()
        gx = torch.empty((B, C, H, W), device=g.device, dtype=torch.float32)
        _call("pcfa_upsample_nearest4_bwd", _ptr(g), _ptr(gx), B * C, H, W, s, div)
        return gx, None, None


def upsample_nearest4(x, s=1.0, div=False):
    """nn.Upsample(scale_factor=4, mode='nearest')(x / s if div else x * s) (FlowNet2's upsample3 / upsample4 of the flow
    divided / multiplied by div_flow).  Backward: a gather of the 16 gradients of each pixel (fp64 sum, rounded once)."""
    _dev(x)
    if x.dim() != 4 or x.dtype != torch.float32:
        raise ValueError("upsample_nearest4: float32 [B, C, H, W] expected, got %s %s" % (x.dtype, tuple(x.shape)))
    return _UpsampleNearest4.apply(x, float(s), bool(div))


class _LeakyReLU(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, slope):
        x = x.contiguous()
        y = torch.empty_like(x)
        _call("pcfa_leaky_relu_fwd", _ptr(x), _ptr(y), slope, x.numel())
        ctx.slope = slope
        ctx.save_for_backward(y)
        return y

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, g):
        (y,) = ctx.saved_tensors
        g = g.contiguous()
        gx = torch.empty_like(g)
        _call("pcfa_leaky_relu_bwd", _ptr(y), _ptr(g), _ptr(gx), ctx.slope, g.numel())
        return gx, None


def leaky_relu(x, slope=0.1):
    """F.leaky_relu(x, slope) on the package's elementwise kernels (conv_redir's activation after ops.conv1x1)."""
    _dev(x)
    return _LeakyReLU.apply(x, float(slope))
