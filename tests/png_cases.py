"""Test-side PNG encoder and the cases of the reader tests (tests/test_ingest_*.py).

The encoder applies a GIVEN filter type to every row.  Forward filtering needs the original pixels only -- Filt(x) =
Orig(x) - predictor(Orig(a), Orig(b), Orig(c)) -- so it is a few numpy lines with no recurrence: a statement of the five
filters that is independent of the reconstruction loop in pcfa_amd.helper_functions.png and of the device kernel.
"""
import os
import struct
import zlib

import numpy as np

SIGNATURE = b"\x89PNG\r\n\x1a\n"
# name -> (colour type, bit depth, channels, bytes per pixel)
FORMATS = {"rgb8": (2, 8, 3, 3), "grey8": (0, 8, 1, 1), "rgba8": (6, 8, 4, 4), "rgb16": (2, 16, 3, 6)}
BPP_FORMAT = {3: "rgb8", 1: "grey8", 4: "rgba8", 6: "rgb16"}
EDGE_BYTES = np.array([0, 1, 2, 127, 128, 254, 255], np.uint8)   # wrap-around and the Paeth ties pa == pb, pb == pc


def chunk(kind, body):
    return struct.pack(">I", len(body)) + kind + body + struct.pack(">I", zlib.crc32(kind + body) & 0xffffffff)


def filter_rows(raw, bpp, plan):
    """The filtered scanlines (bytes: per row the filter type, then the filtered bytes) of raw uint8 [H, row_bytes] with
    row y filtered by type plan[y]."""
    h, row_bytes = raw.shape
    cur = raw.astype(np.int32)
    a = np.zeros_like(cur)                       # left
    a[:, bpp:] = cur[:, :-bpp] if row_bytes > bpp else 0
    b = np.zeros_like(cur)                       # up
    b[1:] = cur[:-1]
    c = np.zeros_like(cur)                       # upper left
    c[:, bpp:] = b[:, :-bpp] if row_bytes > bpp else 0
    p = a + b - c
    pa, pb, pc = np.abs(p - a), np.abs(p - b), np.abs(p - c)
    paeth = np.where((pa <= pb) & (pa <= pc), a, np.where(pb <= pc, b, c))
    pred = np.stack([np.zeros_like(cur), a, b, (a + b) // 2, paeth])             # [5, H, row_bytes]
    plan = np.asarray(plan, np.int64)
    filt = ((cur - pred[plan, np.arange(h)]) & 255).astype(np.uint8)
    return np.concatenate([plan.astype(np.uint8)[:, None], filt], axis=1).tobytes()


def sample_bytes(samples):
    """uint8 [H, row_bytes] of samples [H,W,C] uint8, or uint16 (written big-endian, as PNG stores them)."""
    s = np.asarray(samples)
    if s.dtype == np.uint16:
        s = s.astype(">u2").view(np.uint8)
    elif s.dtype != np.uint8:
        raise TypeError(s.dtype)
    return np.ascontiguousarray(s).reshape(s.shape[0], -1)


def encode(samples, fmt, plan, idat_chunks=1, interlace=0, ihdr_override=None, scanlines=None):
    """PNG file bytes of samples [H,W,C] in format `fmt` (FORMATS) with row y filtered by plan[y], the compressed stream
    split over `idat_chunks` IDAT chunks.  `scanlines` replaces the filtered stream (container tests)."""
    ctype, depth, channels, bpp = FORMATS[fmt]
    h, w = samples.shape[:2]
    assert samples.shape[2] == channels and samples.dtype == (np.uint16 if depth == 16 else np.uint8)
    if scanlines is None:
        scanlines = filter_rows(sample_bytes(samples), bpp, plan)
    ihdr = ihdr_override or struct.pack(">IIBBBBB", w, h, depth, ctype, 0, 0, interlace)
    z = zlib.compress(scanlines, 6)
    cuts = [len(z) * i // idat_chunks for i in range(idat_chunks + 1)]
    idat = b"".join(chunk(b"IDAT", z[cuts[i]:cuts[i + 1]]) for i in range(idat_chunks))
    return SIGNATURE + chunk(b"IHDR", ihdr) + idat + chunk(b"IEND", b"")


def write(path, samples, fmt, plan=None, idat_chunks=1):
    h = samples.shape[0]
    plan = [(y + 1) % 5 for y in range(h)] if plan is None else plan
    os.makedirs(os.path.dirname(path), exist_ok=True)
    with open(path, "wb") as f:
        f.write(encode(samples, fmt, plan, idat_chunks))
    return path


def plans(h, rng):
    """(name, filter type per row): each type on its own, cycling over the rows, random per row."""
    for t in range(5):
        yield "type%d" % t, [t] * h
    yield "cycle", [y % 5 for y in range(h)]
    yield "random", list(rng.randint(0, 5, h))


def raw_bytes(h, row_bytes, alphabet, rng):
    """uint8 [h, row_bytes]: 'edge' draws from EDGE_BYTES, 'uniform' from 0..255."""
    if alphabet == "edge":
        return EDGE_BYTES[rng.randint(0, len(EDGE_BYTES), (h, row_bytes))]
    return rng.randint(0, 256, (h, row_bytes)).astype(np.uint8)


def unfilter_cases(h, w, bpp, seed=0):
    """(name, filtered scanlines, the original uint8 [h, w * bpp]) for every plan and both alphabets."""
    rng = np.random.RandomState(seed + 1000 * h + 10 * w + bpp)
    for alphabet in ("edge", "uniform"):
        for name, plan in plans(h, rng):
            raw = raw_bytes(h, w * bpp, alphabet, rng)
            yield "%s/%s" % (alphabet, name), filter_rows(raw, bpp, plan), raw


def random_samples(fmt, h, w, rng):
    _, depth, channels, _ = FORMATS[fmt]
    if depth == 16:
        return rng.randint(0, 65536, (h, w, channels)).astype(np.uint16)
    return rng.randint(0, 256, (h, w, channels)).astype(np.uint8)


def planes_of(samples, fmt):
    """What a reader returns for `samples`: float32 [3,H,W] -- RGB, grey tiled, alpha dropped; 16-bit: (u, v, valid)."""
    s = np.asarray(samples)
    if fmt == "rgb16":
        s = s.astype(np.float64)
        return np.stack([(s[..., 0] - 32768) / 64, (s[..., 1] - 32768) / 64, s[..., 2]]).astype(np.float32)
    if fmt == "grey8":
        s = np.repeat(s, 3, axis=2)
    return np.ascontiguousarray(np.transpose(s[..., :3], (2, 0, 1))).astype(np.float32)


def write_flo(path, flow):
    """Middlebury .flo of flow float32 [H,W,2]."""
    os.makedirs(os.path.dirname(path), exist_ok=True)
    h, w = flow.shape[:2]
    with open(path, "wb") as f:
        f.write(struct.pack("<fii", 202021.25, w, h))
        f.write(np.ascontiguousarray(flow, "<f4").tobytes())
    return path


# ---------------------------------------------------------------------------------------------- dataset trees
def sintel_tree(root, scenes, h, w, split="training", dstype="final", seed=0, with_flow=True):
    """root/<split>/<dstype>/<scene>/frame_NNNN.png (+ flow/<scene>/frame_NNNN.flo) for scenes = {name: frames}.
    Returns {scene: (frames uint8 [n,H,W,3], flows float32 [n-1,H,W,2])}."""
    rng = np.random.RandomState(seed)
    made = {}
    for scene, n in scenes.items():
        # smooth content (low-pass noise), so that a flow network sees structure, shifted a little from frame to frame
        base = rng.randint(0, 256, (h + 8, w + 8 + 2 * n, 3)).astype(np.float32)
        for _ in range(2):
            base = (base + np.roll(base, 1, 0) + np.roll(base, 1, 1) + np.roll(base, (1, 1), (0, 1))) / 4
        frames = np.stack([np.clip(base[4:4 + h, 4 + 2 * i:4 + 2 * i + w], 0, 255).astype(np.uint8) for i in range(n)])
        flows = rng.uniform(-3, 3, (max(n - 1, 0), h, w, 2)).astype(np.float32)
        for i in range(n):
            write(os.path.join(root, split, dstype, scene, "frame_%04d.png" % (i + 1)), frames[i], "rgb8", idat_chunks=2)
        if with_flow:
            os.makedirs(os.path.join(root, split, "flow", scene), exist_ok=True)
            for i in range(n - 1):
                write_flo(os.path.join(root, split, "flow", scene, "frame_%04d.flo" % (i + 1)), flows[i])
        made[scene] = (frames, flows)
    return made


def kitti_tree(root, sizes, split="training", seed=0, with_flow=True):
    """root/<split>/image_2/NNNNNN_10.png, _11.png (+ flow_occ/NNNNNN_10.png) with pair i of size sizes[i].
    Returns [(frame1, frame2, flow samples uint16 [H,W,3])]."""
    rng = np.random.RandomState(seed)
    made = []
    for i, (h, w) in enumerate(sizes):
        f1, f2 = random_samples("rgb8", h, w, rng), random_samples("rgb8", h, w, rng)
        fl = random_samples("rgb16", h, w, rng)
        fl[..., 2] = rng.randint(0, 2, (h, w))
        plan = list(rng.randint(0, 5, h))
        write(os.path.join(root, split, "image_2", "%06d_10.png" % i), f1, "rgb8", plan)
        write(os.path.join(root, split, "image_2", "%06d_11.png" % i), f2, "rgb8", plan)
        if with_flow:
            write(os.path.join(root, split, "flow_occ", "%06d_10.png" % i), fl, "rgb16", plan, idat_chunks=3)
        made.append((f1, f2, fl))
    return made
