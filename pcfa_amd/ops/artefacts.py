"""Picture artefacts: the device half of `--save_png` (csrc/artefact_ops.hip).

Packed 8-bit RGB from fp32 tensors, one launch per picture; every scale is a device tensor, so converting a pair's ten
pictures needs no host read.  No gradients: these are outputs for people to look at.
"""
import torch

from .. import _hip
from .core import _call, _dev, _ptr

__all__ = ["flow_maxlen", "absmax", "flow_to_rgb8", "image_to_rgb8"]


def _flow4(flow):
    f = flow.detach()
    if f.dim() == 3:
        f = f.unsqueeze(0)
    if f.dim() != 4 or f.shape[1] != 2:
        raise ValueError("flow must be [B,2,H,W] or [2,H,W], got %s" % (tuple(flow.shape),))
    return f


def _image4(x, what):
    t = x.detach()
    if t.dim() == 3:
        t = t.unsqueeze(0)
    if t.dim() != 4 or t.shape[1] != 3:
        raise ValueError("%s must be [B,3,H,W] or [3,H,W], got %s" % (what, tuple(x.shape)))
    return t


def _nonempty(t):
    if t.numel() == 0:
        raise ValueError("empty tensor %s" % (tuple(t.shape),))


def flow_maxlen(flow):
    """[B] lengths of each item's longest flow vector, fp32 sqrt(u*u + v*v) as numpy rounds it; NaN pixels count as 0.
    Views are fine.  The true length -- ownutilities.flow_length, not the reference's sqrt(u + v)."""
    _dev(flow)
    f = _flow4(flow)
    _nonempty(f)
    B, _, H, W = f.shape
    out = torch.empty(B, device=f.device, dtype=torch.float32)
    _call("pcfa_flow_maxlen_items", _ptr(f), _hip.strides4(f), B, H, W, _ptr(out))
    return out


def absmax(x):
    """[B] values max |x[b]| (B = x.shape[0]): the reference's `max_delta`, one perturbation's half."""
    _dev(x)
    xc = x.detach().contiguous()
    _nonempty(xc)
    B = xc.shape[0]
    out = torch.empty(B, device=xc.device, dtype=torch.float32)
    _call("pcfa_absmax_items", _ptr(xc), B, xc.numel() // B, _ptr(out))
    return out


def flow_to_rgb8(flow, scale):
    """uint8 [B,H,W,3]: the Middlebury colour code of flow_library's colorplot_light, item b scaled by scale[b] (a device
    tensor of B values, or of one value for all items): vectors up to the scale fade from white into the wheel's colour,
    longer ones are darkened.  NaN pixels are black; a zero scale gives a white picture, as in the reference.

    Limit, shared with the reference's fp32 arithmetic: the step between the two branches sits at scaled length 1, and
    under a picture's OWN maximum m the longest vector has length m / (m + 1e-5) -- below 1 by 1e-5 / m.  The fp32 error of
    that length is up to about 4 * 2^-24, so for m above roughly 20 the guard is no longer safely larger than the error
    (above about 256 it vanishes in m + 1e-5 altogether) and the pixels of the longest vector may come out darkened
    (colour * 0.75) instead of fully saturated.  Every other pixel is unaffected; a scale a little above the maximum
    avoids it."""
    _dev(flow, scale)
    f = _flow4(flow)
    _nonempty(f)
    B, _, H, W = f.shape
    s = scale.detach().reshape(-1)
    if s.numel() == 1 and B > 1:
        s = s.expand(B)
    if s.numel() != B:
        raise ValueError("one scale per item: %d items, %d scales" % (B, s.numel()))
    s = s.contiguous()
    out = torch.empty((B, H, W, 3), device=f.device, dtype=torch.uint8)
    _call("pcfa_flow_colour_u8", _ptr(f), _hip.strides4(f), _ptr(s), B, H, W, _ptr(out))
    return out


def image_to_rgb8(x, add=None, normalize_max=None, unit_input=True):
    """uint8 [B,H,W,3] of (x [+ add]) * 255, or with normalize_max = m (a device tensor of one value or of B values) of
    ((x [+ add]) / m / 2 + 0.5) * 255 -- the reference's save_image (helper_functions/logging.py:307-313) followed by
    quickvis_tensor's cast.  unit_input=False (without normalize_max): the input is in levels already, no factor 255.
    `add` broadcasts over the items ([1,3,H,W] or [3,H,W]: one perturbation for all).

    The cast truncates toward zero and SATURATES: NaN and negative values give 0, values above 255 give 255.  The
    reference's `astype(np.uint8)` wraps out-of-range values instead; the box constraint keeps real attacks in range, and
    saturation is the defined behaviour here.  The plain and the `add` path round exactly as fp32 x * 255 and
    (x + add) * 255."""
    _dev(x, add, normalize_max)
    t = _image4(x, "image")
    _nonempty(t)
    B, _, H, W = t.shape
    a = a_strides = None
    if add is not None:
        a = _image4(add, "add")
        if a.shape[0] == 1 and B > 1:
            a = a.expand(B, -1, -1, -1)   # item stride 0
        if a.shape != t.shape:
            raise ValueError("add %s does not match image %s" % (tuple(add.shape), tuple(x.shape)))
        a_strides = _hip.strides4(a)
    m, m_stride = None, 0
    if normalize_max is not None:
        m = normalize_max.detach().reshape(-1).contiguous()
        if m.numel() not in (1, B):
            raise ValueError("normalize_max: one value, or one per item (%d), got %d" % (B, m.numel()))
        m_stride = 1 if (m.numel() == B and B > 1) else 0
    out = torch.empty((B, H, W, 3), device=t.device, dtype=torch.uint8)
    _call("pcfa_image_u8", _ptr(t), _hip.strides4(t), _ptr(a), a_strides, _ptr(m), m_stride, int(bool(unit_input)), B, H, W,
          _ptr(out))
    return out
