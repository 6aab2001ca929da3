"""Dataset ingest: the device half of reading a PNG file (csrc/ingest_ops.hip), the other direction of ops.artefacts.

The host reads the file and inflates it (helper_functions/png.decode_header_and_scanlines); `png_unfilter` undoes the
scanline filters and `samples_to_planar` unpacks the samples into the planar fp32 tensor the attack works on, padded or
cropped on the way -- two launches per file, no torch kernel behind them.  No gradients: these are inputs.
"""
import torch

from .core import _call, _ptr

__all__ = ["png_unfilter", "samples_to_planar", "SAMPLE_KINDS"]

# kind -> (the entry point's code, bytes per pixel)
SAMPLE_KINDS = {"rgb8": (0, 3), "grey8": (1, 1), "rgba8": (2, 4), "kitti_flow16": (3, 6)}


def _bytes_on_device(t, what):
    if not t.is_cuda:
        raise RuntimeError("pcfa_amd HIP operator called with a %s tensor: the MI355X path has no CPU fallback" % t.device)
    if t.dtype != torch.uint8:
        raise TypeError("%s is a uint8 tensor, got %s" % (what, t.dtype))
    if not t.is_contiguous():
        raise ValueError("%s must be contiguous" % what)


def png_unfilter(filtered, H, row_bytes, bpp, out=None):
    """uint8 [H * row_bytes]: the reconstructed bytes of H filtered PNG scanlines (uint8 [H * (1 + row_bytes)] on the
    device: per row one filter-type byte, which the caller has checked to be <= 4, and row_bytes filtered bytes); bpp =
    bytes per complete pixel, one of 1, 3, 4, 6.  `out`: a contiguous uint8 tensor of H * row_bytes elements to write into
    (a view into a larger buffer is fine) instead of a new one."""
    _bytes_on_device(filtered, "filtered")
    H, row_bytes, bpp = int(H), int(row_bytes), int(bpp)
    if H < 1 or row_bytes < 1 or filtered.numel() != H * (1 + row_bytes):
        raise ValueError("%d filtered bytes are not %d rows of 1 + %d" % (filtered.numel(), H, row_bytes))
    if out is None:
        out = torch.empty(H * row_bytes, device=filtered.device, dtype=torch.uint8)
    else:
        _bytes_on_device(out, "out")
        if out.numel() != H * row_bytes or out.device != filtered.device:
            raise ValueError("out holds %d bytes on %s, %d on %s expected" % (out.numel(), out.device, H * row_bytes,
                                                                              filtered.device))
    _call("pcfa_png_unfilter", _ptr(filtered), _ptr(out), H, row_bytes, bpp)
    return out


def samples_to_planar(raw, H, W, kind, Hp=None, Wp=None, out=None):
    """fp32 [3,Hp,Wp] from the uint8 samples `raw` of an [H,W] picture of `kind`:
      "rgb8" / "grey8" / "rgba8"   the three colour planes in levels [0, 255]; grey tiled to three planes, alpha dropped
      "kitti_flow16"               big-endian 16-bit R, G, B -> (u, v, valid) = ((R - 32768) / 64, (G - 32768) / 64, B), exact
    Hp, Wp (default H, W) are the target of F.pad(x, (0, Wp - W, 0, Hp - H), "constant", 0), negative differences included:
    zero outside the source, source beyond the target cropped.  `out`: a contiguous fp32 [3,Hp,Wp] tensor to write into
    (a view into a larger buffer at any 4-byte offset is fine) instead of a new one."""
    _bytes_on_device(raw, "raw")
    if kind not in SAMPLE_KINDS:
        raise ValueError("kind %r: one of %s" % (kind, ", ".join(sorted(SAMPLE_KINDS))))
    code, bpp = SAMPLE_KINDS[kind]
    H, W = int(H), int(W)
    Hp, Wp = int(H if Hp is None else Hp), int(W if Wp is None else Wp)
    if H < 1 or W < 1 or Hp < 1 or Wp < 1 or raw.numel() != H * W * bpp:
        raise ValueError("%d bytes are not a %d x %d picture of %d bytes per pixel (target %d x %d)"
                         % (raw.numel(), H, W, bpp, Hp, Wp))
    if out is None:
        out = torch.empty((3, Hp, Wp), device=raw.device, dtype=torch.float32)
    elif (not out.is_cuda or out.dtype != torch.float32 or tuple(out.shape) != (3, Hp, Wp) or not out.is_contiguous()
          or out.device != raw.device):
        raise ValueError("out must be a contiguous fp32 [3,%d,%d] tensor on %s" % (Hp, Wp, raw.device))
    _call("pcfa_samples_to_planar", _ptr(raw), H, W, code, _ptr(out), Hp, Wp)
    return out
