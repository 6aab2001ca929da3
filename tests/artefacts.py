"""References, PNG reader and case table of the picture-artefact tests (pcfa_amd/csrc/artefact_ops.hip,
pcfa_amd/helper_functions/png.py).  Not a test; no GPU.

Two statements of the four operators, both written from their description (include/pcfa_hip.h):
  *_f64   float64 numpy: what the GPU tests compare against.  tests/test_artefacts_host_cpu.py shows that flow_colour_f64
          reproduces the reference's colorplot_light bit for bit on tests/golden/flow_colour.npz;
  *_f32   the same arithmetic in plain float32 numpy: the CPU test shows that this alone passes the GPU gates.

Layouts follow the operators: flows [B,2,H,W], images [B,3,H,W], scales [B], pictures uint8 [B,H,W,3].
"""
import struct
import zlib

import numpy as np

NCOLS = 55
EPSILON = 1e-5          # colorplot_light's guard of the scale
RAD_MARGIN = 1e-4       # forced scales: no pixel of a test input may sit this close to the rad = 1 step
MAX_CHANGED_SHARE = 0.02


def wheel():
    """The 55 x 3 Middlebury colour wheel (Baker et al., ICCV 2007), levels 0..255 as float64: six segments
    RY 15, YG 6, GC 4, CB 11, BM 13, MR 6; one channel full, one ramping by floor(255 i / n)."""
    w = np.zeros((NCOLS, 3))
    col = 0
    for n, full, ramp, up in ((15, 0, 1, True), (6, 1, 0, False), (4, 1, 2, True), (11, 2, 1, False), (13, 2, 0, True),
                              (6, 0, 2, False)):
        r = np.floor(255 * np.arange(n) / n)
        w[col:col + n, full] = 255
        w[col:col + n, ramp] = r if up else 255 - r
        col += n
    assert col == NCOLS
    return w


def _colour(flow, scale, dtype):
    flow = np.asarray(flow).astype(dtype)
    B, _, H, W = flow.shape
    scale = np.broadcast_to(np.asarray(scale).astype(dtype).reshape(-1), (B,)).reshape(B, 1, 1)
    u, v = flow[:, 0].copy(), flow[:, 1].copy()
    nan = np.isnan(u) | np.isnan(v)
    u[nan] = 0
    v[nan] = 0
    eps, one = dtype(EPSILON), dtype(1)
    with np.errstate(invalid="ignore", divide="ignore"):
        u = u / (scale + eps)
        v = v / (scale + eps)
        rad = np.sqrt(np.square(u) + np.square(v))
        a = np.arctan2(-v, -u) / dtype(np.pi)
        fk = (a + one) / dtype(2) * dtype(NCOLS - 1)
        k0 = np.floor(fk).astype(np.int32)
        k1 = k0 + 1
        k1[k1 == NCOLS] = 0
        f = fk - k0.astype(dtype)
        out = np.zeros((B, H, W, 3), np.uint8)
        wh = wheel().astype(dtype)
        for c in range(3):
            col0 = wh[k0, c] / dtype(255)
            col1 = wh[k1, c] / dtype(255)
            col = (one - f) * col0 + f * col1
            col = np.where(rad <= one, one - rad * (one - col), col * dtype(0.75))
            out[..., c] = np.floor(dtype(255) * col)
    out[nan] = 0
    return out, np.where(nan, 0, rad)


def flow_colour_f64(flow, scale):
    """(picture, rad): colorplot_light per pixel in float64, item b scaled by scale[b]; rad [B,H,W] is the scaled length
    (0 at NaN pixels) that decides the branch."""
    return _colour(flow, scale, np.float64)


def flow_colour_f32(flow, scale):
    return _colour(flow, scale, np.float32)[0]


def flow_maxlen_f32(flow):
    """[B] fp32: max sqrt(u*u + v*v), every operation rounded once; NaN pixels count as 0."""
    flow = np.asarray(flow, np.float32)
    u, v = flow[:, 0], flow[:, 1]
    with np.errstate(invalid="ignore"):
        length = np.sqrt(u * u + v * v)
    length = np.where(np.isnan(u) | np.isnan(v), np.float32(0), length)
    return length.reshape(len(flow), -1).max(axis=1).astype(np.float32)


def absmax_f32(x):
    x = np.asarray(x, np.float32)
    return np.abs(x).reshape(len(x), -1).max(axis=1)


def _saturate(v):
    with np.errstate(invalid="ignore"):
        v = np.where(np.isnan(v), 0, v)
        return np.trunc(np.clip(v, 0, 255)).astype(np.uint8)


def _image(x, add, m, dtype):
    v = np.asarray(x).astype(dtype)
    B = v.shape[0]
    if add is not None:
        v = v + np.asarray(add).astype(dtype)
    with np.errstate(invalid="ignore", divide="ignore"):
        if m is not None:
            m = np.broadcast_to(np.asarray(m).astype(dtype).reshape(-1), (B,)).reshape(B, 1, 1, 1)
            v = v / m / dtype(2) + dtype(0.5)
        v = v * dtype(255)
    return _saturate(np.transpose(v, (0, 2, 3, 1)))


def image_f64(x, add=None, m=None):
    """(x [+ add]) [/ m / 2 + 0.5] times 255, truncated toward zero and saturated (NaN and negatives 0, above 255: 255)."""
    return _image(x, add, m, np.float64)


def image_f32(x, add=None, m=None):
    return _image(x, add, m, np.float32)


# ------------------------------------------------------------------------------------------------ gates
def check_colour(got, flow, scale, forced, random_normal=False):
    """The colour gate.  Every channel of every pixel within one level of the float64 restatement, NaN pixels exactly black;
    on random-normal inputs at most MAX_CHANGED_SHARE of the pixels differ at all.  Returns (max level difference, share
    of pixels that differ).

    The colour is continuous in the flow except at NaN and, under a forced scale, at rad = 1; fp32 error is far below
    1/255, so a correct kernel can only flip a floor.  Nothing is excluded from the comparison; instead the inputs are
    asserted to stay clear of the step: under a forced scale no pixel has float64 rad within RAD_MARGIN of 1.  Under the
    picture's own maximum there is no step to avoid as long as the fp32 rad of the longest vector stays at or below 1 like
    the float64 one, max / (max + 1e-5): the fp32 error of rad is below 4 * 2^-24 (two divisions, two squares, a sum, a
    root, and the rounding of max + 1e-5), so the inputs are asserted to have rad <= 1 - 5e-7, i.e. a maximum below 20."""
    want, rad = flow_colour_f64(flow, scale)
    if forced:
        assert np.abs(rad - 1).min() > RAD_MARGIN, "test input within %g of the rad = 1 step" % RAD_MARGIN
    else:
        assert rad.max() <= 1 - 5e-7, "test input too long for its own scale: fp32 rad may pass 1"
    got = np.asarray(got)
    assert got.shape == want.shape and got.dtype == np.uint8
    flow = np.asarray(flow)
    nan = np.isnan(flow[:, 0]) | np.isnan(flow[:, 1])
    assert (got[nan] == 0).all(), "NaN pixels must be black"
    diff = np.abs(got.astype(np.int32) - want.astype(np.int32))
    share = float((diff.max(axis=-1) > 0).mean())
    assert diff.max() <= 1, "channel off by %d levels" % diff.max()
    if random_normal:
        assert share <= MAX_CHANGED_SHARE, "%.2f %% of the pixels differ" % (100 * share)
    return int(diff.max()), share


# ------------------------------------------------------------------------------------------------ PNG reader
def read_png(data):
    """uint8 [H,W,3] of an 8-bit RGB, non-interlaced PNG given as bytes (filter types 0-2); checks signature and CRCs."""
    assert data[:8] == b"\x89PNG\r\n\x1a\n"
    pos, chunks = 8, []
    while pos < len(data):
        n, kind = struct.unpack(">I4s", data[pos:pos + 8])
        body = data[pos + 8:pos + 8 + n]
        assert struct.unpack(">I", data[pos + 8 + n:pos + 12 + n])[0] == zlib.crc32(kind + body) & 0xffffffff, kind
        chunks.append((kind, body))
        pos += 12 + n
    assert chunks[0][0] == b"IHDR" and chunks[-1] == (b"IEND", b"")
    w, h, depth, colour, comp, filt, lace = struct.unpack(">IIBBBBB", chunks[0][1])
    assert (depth, colour, comp, filt, lace) == (8, 2, 0, 0, 0)
    raw = zlib.decompress(b"".join(body for kind, body in chunks if kind == b"IDAT"))
    rows = np.frombuffer(raw, np.uint8).reshape(h, 3 * w + 1)
    out = np.zeros((h, 3 * w), np.uint8)
    for y in range(h):
        kind, line = rows[y, 0], rows[y, 1:]
        if kind == 0:
            out[y] = line
        elif kind == 1:     # Sub: add the pixel to the left (3 bytes back), modulo 256
            out[y] = line
            for x in range(3, 3 * w):
                out[y, x] = (int(out[y, x]) + int(out[y, x - 3])) & 0xff
        elif kind == 2:     # Up
            out[y] = line + (out[y - 1] if y else 0)
        else:
            raise AssertionError("filter type %d" % kind)
    return out.reshape(h, w, 3)


def read_png_file(path):
    with open(path, "rb") as f:
        return read_png(f.read())


# ------------------------------------------------------------------------------------------------ cases
SHAPES = ((1, 1, 1), (3, 5, 7), (2, 33, 66))     # (B, H, W): 3 x 5 x 7 = 105 pixels per item -- groups of four straddle the
                                                 # items and a byte tail remains; 2 x 33 x 66 spans several workgroups
SIGMAS = (0.01, 1.0, 3.0)                        # per item: very different maxima


def normal_flow(B, H, W, seed=0):
    rng = np.random.RandomState(1000 + seed)
    f = rng.standard_normal((B, 2, H, W))
    return (f * np.array([SIGMAS[b % 3] for b in range(B)]).reshape(B, 1, 1, 1)).astype(np.float32)


def with_nans(flow, seed=0):
    rng = np.random.RandomState(2000 + seed)
    f = flow.copy()
    B, _, H, W = f.shape
    hit = rng.uniform(size=(B, H, W)) < 0.2
    hit.reshape(-1)[0] = True
    which = rng.randint(0, 3, size=(B, H, W))     # u, v or both
    f[:, 0][hit & (which != 1)] = np.nan
    f[:, 1][hit & (which != 0)] = np.nan
    return f


def integer_grid():
    """[2,2,7,7]: every integer vector of [-3, 3]^2; item 1 writes its zeros as -0.0 -- v = +-0 with u of either sign is the
    atan2 seam k0 = 54 -> k1 = 0."""
    r = np.arange(-3, 4, dtype=np.float32)
    u, v = np.meshgrid(r, r)
    pos = np.stack([u, v])
    neg = pos.copy()
    neg[neg == 0] = -0.0
    return np.stack([pos, neg]).astype(np.float32)


def bin_centres():
    """[1,2,4,55]: vectors whose angle sits exactly on a wheel entry (fk an integer up to rounding), at four lengths."""
    k = np.arange(NCOLS, dtype=np.float64)
    a = (2 * k / (NCOLS - 1) - 1) * np.pi            # atan2(-v, -u) = a
    f = np.zeros((1, 2, 4, NCOLS), np.float32)
    for i, length in enumerate((0.25, 1.0, 2.5, 7.0)):
        f[0, 0, i] = -length * np.cos(a)
        f[0, 1, i] = -length * np.sin(a)
    return f


def strided_view(make, B, C, H, W):
    """A [B,C,H,W] slice of a wider array holding make(B, C, H, W): (wide, index) -- wide[index] is the view."""
    wide = np.full((B, C + 3, H + 1, W + 3), np.float32(777))
    index = (slice(None), slice(1, 1 + C), slice(0, H), slice(2, 2 + W))
    wide[index] = make
    return wide, index


def unit_images(B, H, W, seed=0):
    rng = np.random.RandomState(3000 + seed)
    x = rng.uniform(0, 1, (B, 3, H, W)).astype(np.float32)
    x.reshape(-1)[:2] = (0.0, 1.0)
    # a perturbation that keeps x + d inside [0, 1]
    d = ((rng.uniform(0, 1, x.shape).astype(np.float32) - x) * np.float32(0.05)).astype(np.float32)
    return x, d


OUT_OF_RANGE = np.array([-0.5, -1e-3, -0.0, 0.0, 1.0, 1.0 + 1e-3, 1.5, 300.0, np.inf, -np.inf, np.nan, 0.999999],
                        np.float32)
OUT_OF_RANGE_LEVELS = np.array([0, 0, 0, 0, 255, 255, 255, 255, 255, 0, 0, 254], np.uint8)
