"""The few-channel convolutions (csrc/conv3x3_fewout.hip: the 3x3 and the 4x4 / stride-2 transposed convolution with 1..4
output channels and their data gradients; csrc/conv_fewin.hip: the k x k convolution with 1..2 input channels, un-packed
and packed) for the float64 tests: a Python TRANSCRIPTION of the host rules (channel splits, kper, the wide rule, csplit,
the conv_fewin instances, packed sizes and layout, LDS bytes, staging passes -- no GPU, no ctypes), the shape tables of
tests/test_fewch_f64_gpu.py, and the references of each direction: the float64 result, the bound's sum of absolute values
and the fp32 emulation in the kernel's order of summation.

The transcription follows the two .hip files line by line; tests/test_fewch_host_cpu.py checks it against the library's
host-only entry points.
"""
import functools
import itertools

import torch
import torch.nn.functional as F

from tests.winograd import _cdiv

FO_PX, FO_WAVES, FO_FWD_WAVES = 64, 8, 16     # pixels per workgroup, waves of the gradients, waves of the forwards
FI_PX, FP_PX = 64, 32                         # conv_fewin: pixels per workgroup un-packed / packed
FEWIN = ((2, 7), (1, 7), (2, 5), (2, 3))      # the (Cin, ksize) instances
FEWIN_LDS_LIMIT, FEWIN_PACKED_LDS_LIMIT = 150 * 1024, 60 * 1024
WQ, XQ, FI_THREADS = 16, 12, 256              # 16-B weight pieces / input dwords per thread per staging pass


def _rup(a, b):
    return _cdiv(a, b) * b


# --------------------------------------------------------------------------- host rules: conv3x3_fewout.hip
def splits(B, K, plane):
    """fewout_splits / deconv_splits: channel splits of the forward until ~256 workgroups exist, >= 64 channels each, at
    most 64; 1 below a 4-fold split."""
    tiles = _cdiv(plane, FO_PX) * B
    want = min(_cdiv(256, tiles), max(K // 64, 1), 64)
    return 1 if want < 4 else want


def kper(K, s):
    """Channels per split, rounded up to the 16 waves."""
    return _rup(_cdiv(K, s), FO_FWD_WAVES)


def wide(plane, x_aligned=True):
    """The 3x3 forward stages rows through LDS iff every channel plane is 16-B aligned."""
    return plane % 4 == 0 and x_aligned


def csplit(B, K, plane):
    """Both gradients: channel groups over blockIdx.y until 512 workgroups exist, at least 8 channels (one per wave) each."""
    tiles = _cdiv(plane, FO_PX) * B
    c = 1
    while tiles * c < 512 and FO_WAVES * c * 2 <= K:
        c *= 2
    return c


def workspace_bytes(B, K, N, H, W, deconv=False):
    """pcfa_conv3x3_fewout_workspace_bytes / pcfa_deconv4s2_fewout_workspace_bytes"""
    if B < 1 or K < 1 or N < 1 or N > 4 or H < 1 or W < 1:
        return 0
    s = splits(B, K, H * W)
    return s * B * N * H * W * (4 if deconv else 1) * 4 if s > 1 else 0


def window_shifts(W):
    """The LDS kernel's dsh[r] = (p0 + (r - 1) W - 1) mod 4 for a tile start p0 % 64 == 0, r = 0, 1, 2."""
    return {(-W - 1) % 4, 3, (W - 1) % 4}


# --------------------------------------------------------------------------- host rules: conv_fewin.hip
def fewin_taps(Cin, k):
    return Cin * k * k


def fewin_steps(Cin, k):
    """(STEPS, SG, TS): MFMA steps (tap pairs), groups of four steps, the odd LDS row stride > T"""
    T = fewin_taps(Cin, k)
    steps = (T + 1) // 2
    return steps, _cdiv(steps, 4), (T + 1) | 1


def packed_floats(Cin, N, k):
    """pcfa_conv_fewin_packed_floats: P[32-row block][step group][lane][4], the row blocks padded to 128 rows"""
    if N < 1 or (Cin, k) not in FEWIN:
        return -1
    return _cdiv(N, 128) * 4 * fewin_steps(Cin, k)[1] * 64 * 4


def packed_source(Cin, N, k):
    """The packed layout as an index function: for every float e of P the (row n, tap) it holds, and whether it is a
    real weight (zero beyond (N, T)).  Float q of lane l in step group sg of row block nb = W[32 nb + (l & 31)]
    [2 (4 sg + q) + (l >> 5)]."""
    T, (_, SG, _) = fewin_taps(Cin, k), fewin_steps(Cin, k)
    e = torch.arange(packed_floats(Cin, N, k))
    q, lane, blk = e & 3, (e >> 2) & 63, e >> 8
    sg, nb = blk % SG, blk // SG
    n, tap = 32 * nb + (lane & 31), 2 * (4 * sg + q) + (lane >> 5)
    return n, tap, (n < N) & (tap < T)


def pack_reference(w):
    """pcfa_conv_fewin_pack of a [N, Cin, k, k] weight by the mirror's layout"""
    N, Cin, k, _ = w.shape
    n, tap, live = packed_source(Cin, N, k)
    flat = w.reshape(N, -1)
    return torch.where(live, flat[n.clamp(max=N - 1), tap.clamp(max=flat.shape[1] - 1)], torch.zeros(()))


def fewin_lds_bytes(Cin, N, k, W, packed=False):
    """Dynamic LDS of a launch: the flat input range of a tile, and un-packed all weights at stride TS before it."""
    span = (FP_PX if packed else FI_PX) + 2 * (k // 2) * (W + 1)
    if packed:
        return Cin * span * 4
    return (_rup(N, 128) * fewin_steps(Cin, k)[2] + Cin * span) * 4


def fewin_supported(Cin, N, k, W, packed=False):
    if (Cin, k) not in FEWIN:
        return False
    return fewin_lds_bytes(Cin, N, k, W, packed) <= (FEWIN_PACKED_LDS_LIMIT if packed else FEWIN_LDS_LIMIT)


def fewin_passes(Cin, N, k, W):
    """(weight passes, input passes) of the un-packed kernel's staging loop: 16 x 256 16-B pieces of the N T weights and
    12 x 256 dwords of the Cin x span input range per pass."""
    n4 = N * fewin_taps(Cin, k) // 4
    span = FI_PX + 2 * (k // 2) * (W + 1)
    return max(_cdiv(n4, WQ * FI_THREADS), 1), _cdiv(Cin * span, XQ * FI_THREADS)


# --------------------------------------------------------------------------- path labels
def path(kind, B, K, N, H, W, k=3, x_aligned=True):
    """The label of the kernel configuration a call runs.  kind: conv3_fwd, conv3_bwd, deconv_fwd, deconv_bwd (K input
    channels, N <= 4 outputs), fewin, fewin_packed (K = Cin input channels, N outputs, kernel k)."""
    plane = H * W
    if kind == "conv3_fwd":
        return ("lds" if wide(plane, x_aligned) else "plain") + ("_s1" if splits(B, K, plane) == 1 else "_split")
    if kind == "deconv_fwd":
        return "deconv_s1" if splits(B, K, plane) == 1 else "deconv_split"
    if kind == "conv3_bwd":
        return "bwd_c%d" % csplit(B, K, plane)
    if kind == "deconv_bwd":
        return "deconv_bwd_c%d" % csplit(B, K, plane)
    if kind == "fewin":
        return "fewin_w%dx%d" % fewin_passes(K, N, k, W)
    assert kind == "fewin_packed", kind
    return "packed"


# --------------------------------------------------------------------------- the shape tables
# 3x3 forward: ((B, K, N, H, W), bias, shift of x into its fence in floats, label)
CONV3_FWD = [
    ((1, 1, 1, 18, 8), True, 0, "lds_s1"),        # W % 4 = 0: window shifts 3 3 3; K = 1
    ((1, 15, 2, 28, 5), False, 0, "lds_s1"),      # W % 4 = 1: shifts 2 3 0; K below one wave round
    ((1, 17, 3, 22, 6), True, 0, "lds_s1"),       # W % 4 = 2: shifts 1 3 1; K one past the 16 waves
    ((1, 65, 4, 20, 7), True, 0, "lds_s1"),       # W % 4 = 3: shifts 0 3 2; K one past the LDS kernel's 64-channel round
    ((1, 129, 2, 18, 8), True, 1, "plain_s1"),    # the plain kernel at plane % 4 == 0: x one float off; K one past its 128
    ((1, 129, 2, 9, 20), False, 0, "lds_s1"),     # the same K on the LDS kernel, three tiles
    ((2, 17, 4, 31, 66), True, 0, "plain_s1"),    # B = 2, W > 64 (a tile inside a row), 32 tiles, the last of 62 pixels
    ((2, 16, 4, 31, 68), True, 0, "lds_s1"),      # the same on the LDS kernel, the last tile of 60 pixels
    ((1, 33, 4, 88, 3), False, 0, "lds_s1"),      # W = 3: a tile across 21 rows
    ((1, 20, 4, 43, 3), True, 0, "plain_s1"),     # W = 3, plane % 64 == 1
    ((1, 20, 2, 7, 9), True, 0, "plain_s1"),      # plane < 64
    ((1, 20, 1, 8, 8), True, 0, "lds_s1"),        # plane == 64
    ((1, 20, 3, 5, 13), False, 0, "plain_s1"),    # plane % 64 == 1
    ((1, 24, 2, 37, 1), True, 0, "plain_s1"),     # W = 1
    ((1, 24, 2, 1, 40), True, 0, "lds_s1"),       # H = 1
    ((1, 24, 2, 36, 2), False, 0, "lds_s1"),      # W = 2
    ((1, 390, 2, 3, 5), True, 0, "plain_split"),  # 6 splits of 80: the last one starts past K
    ((1, 390, 3, 4, 4), True, 0, "lds_split"),    # the same on the LDS kernel
    ((1, 300, 4, 6, 11), False, 0, "plain_split"),  # 4 splits of 80, the last holds 60; two tiles
    ((2, 300, 1, 4, 8), True, 0, "lds_split"),    # B = 2 under a split
    ((2, 300, 2, 4, 8), True, 1, "plain_split"),  # a split on the plain kernel at plane % 4 == 0; B = 2 with two outputs
]
# 3x3 data gradient: ((B, K, N, H, W), addend, label)
CONV3_BWD = [
    ((1, 15, 2, 18, 8), True, "bwd_c1"),          # K < 16
    ((1, 16, 1, 128, 256), False, "bwd_c1"),      # 512 tiles: the grid is full
    ((1, 65, 3, 20, 7), True, "bwd_c8"),          # K % 64 and K % 256 != 0
    ((1, 33, 4, 7, 9), False, "bwd_c4"),          # plane < 64
    ((1, 17, 2, 8, 8), True, "bwd_c2"),           # plane == 64
    ((1, 40, 1, 5, 13), False, "bwd_c4"),         # plane % 64 == 1
    ((1, 24, 2, 37, 1), True, "bwd_c2"),          # W = 1
    ((1, 24, 3, 1, 40), False, "bwd_c2"),         # H = 1
    ((1, 24, 2, 36, 2), True, "bwd_c2"),          # W = 2
    ((2, 20, 4, 31, 66), False, "bwd_c2"),        # B = 2, W > 64
    ((1, 130, 2, 88, 3), True, "bwd_c16"),        # W = 3
]
# transposed 4x4 / stride 2 forward: ((B, K, N, H, W), bias, label)
DECONV_FWD = [
    ((1, 1, 1, 18, 8), True, "deconv_s1"),
    ((1, 15, 2, 7, 9), False, "deconv_s1"),       # plane < 64, odd H and W
    ((1, 17, 3, 8, 8), True, "deconv_s1"),        # plane == 64
    ((1, 65, 4, 5, 13), True, "deconv_s1"),       # plane % 64 == 1; K one past the 64-channel round
    ((1, 129, 2, 37, 1), False, "deconv_s1"),     # W = 1
    ((1, 24, 2, 1, 40), True, "deconv_s1"),       # H = 1
    ((1, 24, 2, 36, 2), True, "deconv_s1"),       # W = 2
    ((2, 17, 4, 31, 66), True, "deconv_s1"),      # B = 2, W > 64
    ((1, 20, 4, 88, 3), False, "deconv_s1"),      # W = 3
    ((1, 390, 2, 3, 5), True, "deconv_split"),    # 6 splits of 80: the last one starts past K
    ((1, 300, 4, 6, 11), False, "deconv_split"),  # the last split partial
    ((2, 300, 1, 4, 8), True, "deconv_split"),    # B = 2 under a split
    ((1, 300, 3, 4, 8), True, "deconv_split"),
]
DECONV_BWD = [(s, "deconv_" + lab) for s, _, lab in CONV3_BWD]
# conv_fewin, both kernels: ((B, Cin, N, k, H, W), bias, relu, label of the un-packed kernel)
FEWIN_TABLE = [
    ((1, 2, 128, 7, 9, 20), True, True, "fewin_w1x1"),     # N = 128; 3 (6 packed) tiles, the last partial
    ((1, 2, 200, 7, 5, 13), True, True, "fewin_w2x1"),     # N T = 19600 > 16384: two weight passes; N % 32 = 8
    ((1, 2, 4, 7, 2, 300), False, False, "fewin_w1x2"),    # Cin span = 3740 > 3072: two input passes
    ((1, 1, 5, 7, 6, 11), True, False, "fewin_w1x1"),      # odd tap count; N T % 4 = 1
    ((1, 1, 129, 7, 3, 5), False, True, "fewin_w1x1"),     # a second 128-row block; W narrower than the kernel
    ((2, 2, 33, 5, 7, 9), True, True, "fewin_w1x1"),       # B = 2
    ((1, 2, 1, 5, 37, 1), False, False, "fewin_w1x1"),     # N = 1, W = 1
    ((1, 2, 129, 3, 1, 40), True, False, "fewin_w1x1"),    # H = 1
    ((1, 2, 31, 3, 10, 2), True, True, "fewin_w1x1"),      # W narrower than the kernel
    ((1, 1, 128, 7, 1, 70), False, True, "fewin_w1x1"),    # H = 1 on the 7-row window
]
FEWIN_OVER_LDS = (1, 2, 384, 7, 4, 40)           # 152064 B of weights + 2480 B of inputs > 150 KB
FEWIN_PACKED_OVER_LDS = (1, 2, 8, 7, 1, 1300)    # 2 (32 + 6 * 1301) floats > 60 KB

FWD_LABELS = {"lds_s1", "lds_split", "plain_s1", "plain_split"}
DECONV_LABELS = {"deconv_s1", "deconv_split"}


def sid(s):
    return "x".join(map(str, s))


# --------------------------------------------------------------------------- regions
def pixel_masks(H, W, px=FO_PX, up=1):
    """Boolean H x W masks over flat pixel tiles of `px`: the tile seams p % px in {0, px - 1} and the last tile; `up` = 2
    repeats each input pixel over its 2 x 2 output block (the transposed convolution)."""
    p = torch.arange(H * W).view(H, W)
    m = {"seam": (p % px == 0) | (p % px == px - 1), "last_tile": p >= (_cdiv(H * W, px) - 1) * px}
    if up > 1:
        m = {k: v.repeat_interleave(up, 0).repeat_interleave(up, 1) for k, v in m.items()}
    return m


def regions(H, W, m=0):
    """Named (row slice, column slice) groups of an H x W output map for tests/gates.py: first / last row and column;
    m = 2 (the transposed convolution's output): the four output classes (Y & 1, X & 1) too."""
    g = {"row0": (slice(0, 1), slice(None)), "rowN": (slice(H - 1, H), slice(None)),
         "col0": (slice(None), slice(0, 1)), "colN": (slice(None), slice(W - 1, W))}
    if m == 2:
        for a in (0, 1):
            for b in (0, 1):
                g["class%d%d" % (a, b)] = (slice(a, None, 2), slice(b, None, 2))
    return g


def extra_groups(H, W, px=FO_PX, up=1):
    """The pixel-tile groups as indices of a [B, C, up H, up W] output (`extra` of tests/gates.py)."""
    return {k: (slice(None), slice(None), v) for k, v in pixel_masks(H, W, px, up).items()}


def group_sizes(B, C, H, W, px=FO_PX, up=1):
    """Elements of every named group of a [B, C, up H, up W] output: the statistical gate skips groups below 256."""
    t = torch.zeros(B, C, up * H, up * W)
    n = {k: t[(slice(None), slice(None)) + sl].numel() for k, sl in regions(up * H, up * W, up).items()}
    n.update({k: t[idx].numel() for k, idx in extra_groups(H, W, px, up).items()})
    return n


# --------------------------------------------------------------------------- references
def _gen(*key):
    return torch.Generator().manual_seed(sum((i + 3) * 7919 ** (i % 3) * int(v) for i, v in enumerate(key)) % (2 ** 31))


def _wave_order(K, s, kp):
    """Channel index [s, 16, kp / 16] of split, wave, round, and whether the kernel visits it (c < min(K, kend))."""
    sp, wv, j = torch.arange(s).view(-1, 1, 1), torch.arange(FO_FWD_WAVES).view(1, -1, 1), torch.arange(kp // 16).view(1, 1, -1)
    c = sp * kp + wv + FO_FWD_WAVES * j
    return c.clamp(max=K - 1), c < torch.clamp((sp + 1) * kp, max=K)


def _finish(acc, B, s, bias):
    """acc [B, s * 16, N, h, w]: waves in order, then splits in order, then bias."""
    acc = acc.view(B, s, FO_FWD_WAVES, *acc.shape[2:])
    t = torch.zeros_like(acc[:, :, 0])
    for g in range(FO_FWD_WAVES):
        t = t + acc[:, :, g]
    if s > 1:
        u = torch.zeros_like(t[:, 0])
        for i in range(s):
            u = u + t[:, i]
    else:
        u = t[:, 0]
    return u + bias.view(1, -1, 1, 1) if bias is not None else u


def conv3_fwd_emulation(x, w, bias, s, kp):
    """The 3x3 forward in fp32 in the kernel's order: per wave its channels kbeg + wave, + 16, ... with the nine taps in
    order, waves in order, splits in order, bias."""
    B, K, H, W = x.shape
    N = w.shape[0]
    c, valid = _wave_order(K, s, kp)
    xp = F.pad(x, (1, 1, 1, 1))
    acc = torch.zeros(B, s * FO_FWD_WAVES, N, H, W)
    for j in range(c.shape[2]):
        cj, vj = c[:, :, j].reshape(-1), valid[:, :, j].reshape(-1)
        xs = xp[:, cj].unsqueeze(2)
        wj = (w[:, cj] * vj.view(1, -1, 1, 1)).transpose(0, 1)           # [s 16, N, 3, 3]
        for ky in range(3):
            for kx in range(3):
                acc = acc + wj[:, :, ky, kx].view(1, -1, N, 1, 1) * xs[:, :, :, ky:ky + H, kx:kx + W]
    return _finish(acc, B, s, bias)


def deconv_taps(a):
    """The two (input offset d, kernel index k) of output parity a along one axis: (-t, 1 + 2t) for a = 0 and
    (1 - t, 2t) for a = 1, t = 0, 1."""
    return [((1 - t) if a else -t, 2 * t if a else 1 + 2 * t) for t in (0, 1)]


def deconv_fwd_emulation(x, w, bias, s, kp):
    """The transposed convolution in fp32 in the kernel's order: per output class four taps per channel."""
    B, K, H, W = x.shape
    N = w.shape[1]
    c, valid = _wave_order(K, s, kp)
    xp = F.pad(x, (1, 1, 1, 1))
    out = torch.zeros(B, s * FO_FWD_WAVES, N, 2 * H, 2 * W)
    for a in (0, 1):
        for b in (0, 1):
            acc = torch.zeros(B, s * FO_FWD_WAVES, N, H, W)
            for j in range(c.shape[2]):
                cj, vj = c[:, :, j].reshape(-1), valid[:, :, j].reshape(-1)
                xs = xp[:, cj].unsqueeze(2)
                wj = w[cj] * vj.view(-1, 1, 1, 1)                          # [s 16, N, 4, 4]
                for dy, ky in deconv_taps(a):
                    for dx, kx in deconv_taps(b):
                        acc = acc + wj[:, :, ky, kx].view(1, -1, N, 1, 1) * xs[:, :, :, 1 + dy:1 + dy + H, 1 + dx:1 + dx + W]
            out[:, :, :, a::2, b::2] = acc
    return _finish(out, B, s, bias)


def conv3_bwd_emulation(g, w, addend):
    """grad_x[c] = sum over o, then the nine taps in order, of w[o][c][ky][kx] g[o][y + 1 - ky][x + 1 - kx]; + addend"""
    B, N, H, W = g.shape
    K = w.shape[1]
    gp = F.pad(g, (1, 1, 1, 1))
    acc = torch.zeros(B, K, H, W)
    for o in range(N):
        for ky in range(3):
            for kx in range(3):
                acc = acc + w[o, :, ky, kx].view(1, K, 1, 1) * gp[:, o:o + 1, 2 - ky:2 - ky + H, 2 - kx:2 - kx + W]
    return acc + addend if addend is not None else acc


def deconv_bwd_emulation(g, w):
    """grad_x[c][y][x] = sum over o, then the 16 taps in order, of w[c][o][ky][kx] g[o][2y - 1 + ky][2x - 1 + kx]"""
    B, N, H2, W2 = g.shape
    K = w.shape[0]
    gp = F.pad(g, (1, 1, 1, 1))
    acc = torch.zeros(B, K, H2 // 2, W2 // 2)
    for o in range(N):
        for ky in range(4):
            for kx in range(4):
                acc = acc + w[:, o, ky, kx].view(1, K, 1, 1) * gp[:, o:o + 1, ky:ky + H2 - 1:2, kx:kx + W2 - 1:2]
    return acc


def fewin_emulation(x, w):
    """conv_fewin without bias in fp32: the taps of an output in index order (channel, row, column) -- the two k of an
    MFMA step one after the other."""
    B, Cin, H, W = x.shape
    N, _, k, _ = w.shape
    r = k // 2
    xp = F.pad(x, (r, r, r, r))
    acc = torch.zeros(B, N, H, W)
    for c in range(Cin):
        for ky in range(k):
            for kx in range(k):
                acc = acc + w[:, c, ky, kx].view(1, N, 1, 1) * xp[:, c:c + 1, ky:ky + H, kx:kx + W]
    return acc


def conv3_f64(x, w):
    return F.conv2d(x, w, padding=1)


def conv3_grad_f64(g, w):
    return F.conv_transpose2d(g, w, padding=1)


def deconv_f64(x, w):
    return F.conv_transpose2d(x, w, stride=2, padding=1)


def deconv_grad_f64(g, w):
    return F.conv2d(g, w, stride=2, padding=1)


def _d(t):
    return t.double()


@functools.lru_cache(maxsize=4)
def conv3_fwd_problem(B, K, N, H, W, bias=True, seed=0):
    """x, w, bias; float64 result, P and the fp32 emulation, all with the bias."""
    gen = _gen(1, B, K, N, H, W, seed)
    x = torch.randn(B, K, H, W, generator=gen)
    w = torch.randn(N, K, 3, 3, generator=gen) / (9 * K) ** .5
    b = torch.randn(N, generator=gen) if bias else None
    s = splits(B, K, H * W)
    want, P = conv3_f64(_d(x), _d(w)), conv3_f64(_d(x).abs(), _d(w).abs())
    if bias:
        want, P = want + _d(b).view(1, -1, 1, 1), P + _d(b).abs().view(1, -1, 1, 1)
    return x, w, b, want, P, conv3_fwd_emulation(x, w, b, s, kper(K, s))


@functools.lru_cache(maxsize=4)
def deconv_fwd_problem(B, K, N, H, W, bias=True, seed=0):
    gen = _gen(2, B, K, N, H, W, seed)
    x = torch.randn(B, K, H, W, generator=gen)
    w = torch.randn(K, N, 4, 4, generator=gen) / (4 * K) ** .5
    b = torch.randn(N, generator=gen) if bias else None
    s = splits(B, K, H * W)
    want, P = deconv_f64(_d(x), _d(w)), deconv_f64(_d(x).abs(), _d(w).abs())
    if bias:
        want, P = want + _d(b).view(1, -1, 1, 1), P + _d(b).abs().view(1, -1, 1, 1)
    return x, w, b, want, P, deconv_fwd_emulation(x, w, b, s, kper(K, s))


@functools.lru_cache(maxsize=4)
def conv3_bwd_problem(B, K, N, H, W, addend=True, seed=0):
    """grad_out, w, addend; float64 grad_x, P and the emulation, all with the addend."""
    gen = _gen(3, B, K, N, H, W, seed)
    g = torch.randn(B, N, H, W, generator=gen)
    w = torch.randn(N, K, 3, 3, generator=gen) / (9 * N) ** .5
    a = torch.randn(B, K, H, W, generator=gen) if addend else None
    want, P = conv3_grad_f64(_d(g), _d(w)), conv3_grad_f64(_d(g).abs(), _d(w).abs())
    if addend:
        want, P = want + _d(a), P + _d(a).abs()
    return g, w, a, want, P, conv3_bwd_emulation(g, w, a)


@functools.lru_cache(maxsize=4)
def deconv_bwd_problem(B, K, N, H, W, seed=0):
    gen = _gen(4, B, K, N, H, W, seed)
    g = torch.randn(B, N, 2 * H, 2 * W, generator=gen)
    w = torch.randn(K, N, 4, 4, generator=gen) / (16 * N) ** .5
    want, P = deconv_grad_f64(_d(g), _d(w)), deconv_grad_f64(_d(g).abs(), _d(w).abs())
    return g, w, want, P, deconv_bwd_emulation(g, w)


@functools.lru_cache(maxsize=4)
def fewin_problem(B, Cin, N, k, H, W, bias=True, relu=True, seed=0):
    """x, w, bias; float64 result, P and the emulation with bias and ReLU (applied to the float64 pre-activation)."""
    gen = _gen(5, B, Cin, N, k, H, W, seed)
    x = torch.randn(B, Cin, H, W, generator=gen)
    w = torch.randn(N, Cin, k, k, generator=gen) / (Cin * k * k) ** .5
    b = torch.randn(N, generator=gen) if bias else None
    want = F.conv2d(_d(x), _d(w), padding=k // 2)
    P = F.conv2d(_d(x).abs(), _d(w).abs(), padding=k // 2)
    emu = fewin_emulation(x, w)
    if bias:
        want, P, emu = want + _d(b).view(1, -1, 1, 1), P + _d(b).abs().view(1, -1, 1, 1), emu + b.view(1, -1, 1, 1)
    if relu:
        want, emu = torch.relu(want), torch.relu(emu)
    return x, w, b, want, P, emu


TERMS = {"conv3_fwd": lambda K, N: 9 * K + 1, "conv3_bwd": lambda K, N: 9 * N + 1, "deconv_fwd": lambda K, N: 4 * K + 1,
         "deconv_bwd": lambda K, N: 16 * N}


def fewin_terms(Cin, k):
    return Cin * k * k + 1


def one_hot(shape, index):
    w = torch.zeros(shape)
    w[index] = 1.0
    return w


# --------------------------------------------------------------------------- mirror against the host-only entry points
def host_rule_mismatches(lib):
    """Every (arguments, library's answer, mirror's answer) where pcfa_conv3x3_fewout_workspace_bytes,
    pcfa_deconv4s2_fewout_workspace_bytes or pcfa_conv_fewin_packed_floats disagrees with the mirror, over the tables and a
    sweep of (B, K, plane)."""
    bad = []
    shapes = {c[0] for c in CONV3_FWD + CONV3_BWD + DECONV_FWD + DECONV_BWD}
    shapes |= set(itertools.product([1, 2, 5], [1, 63, 64, 255, 256, 257, 390, 1026, 4096, 5000], [1, 2, 4], [1, 3, 7, 14, 55],
                                    [1, 5, 16, 32, 128]))
    shapes |= {(0, 8, 2, 4, 4), (1, 0, 2, 4, 4), (1, 8, 0, 4, 4), (1, 8, 5, 4, 4), (1, 8, 2, 0, 4), (1, 8, 2, 4, 0)}
    for B, K, N, H, W in sorted(shapes):
        got = (int(lib.pcfa_conv3x3_fewout_workspace_bytes(B, K, N, H, W)),
               int(lib.pcfa_deconv4s2_fewout_workspace_bytes(B, K, N, H, W)))
        exp = (workspace_bytes(B, K, N, H, W), workspace_bytes(B, K, N, H, W, True))
        if got != exp:
            bad.append(((B, K, N, H, W), got, exp))
    for Cin, N, k in itertools.product([0, 1, 2, 3, 4], [0, 1, 5, 31, 32, 33, 128, 129, 200, 384, 1000], [1, 3, 5, 7, 9]):
        got, exp = int(lib.pcfa_conv_fewin_packed_floats(Cin, N, k)), packed_floats(Cin, N, k)
        if got != exp:
            bad.append(((Cin, N, k), got, exp))
    return bad
