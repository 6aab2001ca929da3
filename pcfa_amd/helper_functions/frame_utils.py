"""File readers for the datasets: Sintel / KITTI-15 frames (PNG), KITTI-15's 16-bit flow PNGs and Middlebury `.flo` files.

The reference reads frames with PIL and KITTI's flow with OpenCV (helper_functions/frame_utils.py: read_gen,
readFlowKITTI); this package has no imaging dependency.  A PNG is read in two halves instead:

  host     the file, its chunks and CRCs, zlib inflate (png.decode_header_and_scanlines): serial by nature
  device   the scanline filters undone (ops.png_unfilter: a skewed wavefront, thread = row) and the samples unpacked
           into planar fp32, padded or cropped to the pad target on the way (ops.samples_to_planar): ONE upload of the
           inflated scanlines and two launches per file, no torch kernel afterwards

On a CPU device the same values come from png.unfilter_reference (a plain loop, seconds per frame) and numpy.  Both
paths work on the caller's current stream and do not synchronise: a caller that hands the tensors to another stream
synchronises first (datasets.py does, once per sample).
"""
import numpy as np
import torch

from . import png

FLO_MAGIC = 202021.25   # "PIEH" read as a little-endian float


def _read_png(path, served):
    with open(path, "rb") as f:
        data = f.read()
    try:
        w, h, depth, ctype, scanlines = png.decode_header_and_scanlines(data)
    except ValueError as e:
        raise ValueError("%s: %s" % (path, e))
    bpp, name = png.FORMATS[(ctype, depth)]
    if name not in served:
        raise ValueError("%s: a %d-bit PNG of colour type %d where %s is expected" % (path, depth, ctype, " / ".join(served)))
    return w, h, bpp, name, scanlines


def _planar_numpy(raw, h, w, kind, hp, wp):
    """ops.samples_to_planar in numpy: fp32 [3,hp,wp]."""
    px = np.frombuffer(raw, np.uint8).reshape(h, w, -1)
    if kind == "kitti_flow16":
        s = (px[..., 0::2].astype(np.int32) << 8) | px[..., 1::2]          # big-endian 16-bit R, G, B
        planes = np.stack([(s[..., 0] - 32768) / 64.0, (s[..., 1] - 32768) / 64.0, s[..., 2]]).astype(np.float32)
    elif kind == "grey8":
        planes = np.repeat(px[..., 0][None], 3, axis=0).astype(np.float32)
    else:
        planes = np.ascontiguousarray(np.transpose(px[..., :3], (2, 0, 1))).astype(np.float32)
    out = np.zeros((3, hp, wp), np.float32)
    out[:, :min(h, hp), :min(w, wp)] = planes[:, :min(h, hp), :min(w, wp)]
    return out


def _decode(path, served, kind_of, device, pad_to):
    w, h, bpp, name, scanlines = _read_png(path, served)
    kind = kind_of(name)
    hp, wp = (h, w) if pad_to is None else (int(pad_to[0]), int(pad_to[1]))
    device = torch.device(device)
    if device.type == "cuda":
        from .. import ops
        # a bytearray: torch wants a writable buffer; the copy is one pass over a megabyte
        filtered = torch.frombuffer(bytearray(scanlines), dtype=torch.uint8).to(device)
        table = ops.get()
        return table.samples_to_planar(table.png_unfilter(filtered, h, w * bpp, bpp), h, w, kind, hp, wp)
    raw = png.unfilter_reference(scanlines, h, w * bpp, bpp)
    return torch.from_numpy(_planar_numpy(raw, h, w, kind, hp, wp)).to(device)


def read_image(path, device="cpu", pad_to=None):
    """fp32 [3,H,W] in levels [0, 255] on `device` from an 8-bit RGB, grey (tiled to three channels, as the reference does)
    or RGBA (alpha dropped) PNG.  pad_to = (Hp, Wp): zero-padded at the bottom / right or cropped to [3,Hp,Wp], the
    reference's F.pad(img, (0, Wp - W, 0, Hp - H)) with negative differences."""
    return _decode(path, ("rgb8", "grey8", "rgba8"), lambda name: name, device, pad_to)


def read_flow_kitti(path, device="cpu", pad_to=None):
    """(flow fp32 [2,H,W], valid fp32 [H,W]) from a KITTI-15 flow PNG: 16-bit RGB with u = (R - 2^15) / 64,
    v = (G - 2^15) / 64 and valid = B (devkit readme; the reference's readFlowKITTI).  Both are views of one [3,H,W] tensor.
    pad_to as read_image: flow and valid are padded with zeros alike."""
    planes = _decode(path, ("rgb16",), lambda name: "kitti_flow16", device, pad_to)
    return planes[:2], planes[2]


def read_flow_sintel(path, device="cpu"):
    """(flow fp32 [2,H,W], valid bool [H,W]) on `device` from a Sintel `.flo` file, valid = |u| < 1000 & |v| < 1000 (the
    reference's rule for dense ground truth).  On a GPU the interleaved pairs go up as they lie in the file, in one copy
    from a buffer of the interpreter's own heap, and are split into planes there.  Measured (profiles/dataset_readers):
    planes and mask made with numpy and uploaded as two freshly allocated arrays took 30 ms per file (20-42), this form
    0.53 ms."""
    flow = read_flo(path)
    device = torch.device(device)
    if device.type == "cuda":
        pairs = torch.frombuffer(bytearray(flow.tobytes()), dtype=torch.float32).to(device).view(flow.shape)
        planes = pairs.permute(2, 0, 1).contiguous()
    else:
        planes = torch.from_numpy(np.ascontiguousarray(np.transpose(flow, (2, 0, 1))))
    return planes, (planes[0].abs() < 1000) & (planes[1].abs() < 1000)


def read_flo(path):
    """float32 [H,W,2] (u, v) from a Middlebury `.flo` file: the float 202021.25, int32 width and height, then H * W
    interleaved little-endian (u, v) pairs."""
    with open(path, "rb") as f:
        head = f.read(12)
        if len(head) != 12 or np.frombuffer(head, "<f4", 1)[0] != FLO_MAGIC:
            raise ValueError("%s: not a .flo file (magic number)" % path)
        w, h = (int(v) for v in np.frombuffer(head, "<i4", 2, 4))
        if w < 1 or h < 1:
            raise ValueError("%s: .flo size %d x %d" % (path, w, h))
        body = f.read(8 * w * h)
    if len(body) != 8 * w * h:
        raise ValueError("%s: .flo data truncated (%d of %d bytes)" % (path, len(body), 8 * w * h))
    return np.frombuffer(body, "<f4").reshape(h, w, 2).astype(np.float32)
