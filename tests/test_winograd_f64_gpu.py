"""The Winograd convolutions -- conv3x3 F(2x2,3x3) (csrc/conv3x3.hip) and F(4x4,3x3) (csrc/conv3x3_f43.hip), sepconv5's
1-D F(2,5) (csrc/sepconv5_wino.hip) and its direct implicit GEMM (csrc/sepconv5.hip) -- through the C-ABI on fenced
buffers (tests/fenced.py), against float64 computed from the same fp32 inputs, on every dispatch path.

Each call checks: the status; inputs, weights and every fence bit-unchanged; no sentinel left in the output and every
element finite; the elementwise gate |Y - Y64| <= 2 gamma_n P + n 2^-126 with P and n as documented in tests/winograd.py
(+ 2 spare roundings); the statistical gate rel_l2(Y, Y64) <= 3 max(rel_l2(E, Y64), u), E the same algorithm emulated in
fp32 on the CPU in the kernel's order of summation, globally and per group (first / last row and column, the ragged last
tile, the interior, each 32-channel block; groups of fewer than 256 elements are left to the elementwise gate); and a
second call, with the workspace refilled with other garbage and the output with -7, gives identical bits.  The worst
ratios are recorded as junit properties (--junitxml=FILE -o junit_family=xunit1).

The path of a shape comes from the Python mirror of the host rules (tests/winograd.py), checked against
pcfa_conv3x3_algo / pcfa_conv3x3_workspace_bytes; test_dev_switches runs this module again under the dev A/B switches.
"""
import ctypes
import functools
import os
import signal
import subprocess
import sys

import pytest
import torch
import torch.nn.functional as F

from pcfa_amd import _hip
from tests import winograd as wg
from tests.fenced import DEV, NAN_BITS, PCFA_ERR_INVALID_ARG, SENTINEL, Fenced, stream
from tests.gates import dense_stride as _dense_stride, gates, unchanged as _unchanged

pytestmark = pytest.mark.gpu
torch.set_num_threads(min(16, torch.get_num_threads()))
SLOPE = 0.1
GARBAGE_BITS = 0x5F3759DF   # a large finite float: the second call's workspace


def _lib():
    return _hip.load()


def _mask_tensor(shape, gen):
    """negative values, +0.0, -0.0, positive subnormals and positive normals (reference: mask > 0)"""
    m = torch.randn(*shape, generator=gen)
    sel = torch.randint(0, 5, shape, generator=gen)
    m = torch.where(sel == 1, torch.zeros(()), m)
    m = torch.where(sel == 2, torch.full((), -0.0), m)
    m = torch.where(sel == 3, torch.full((), 2.0 ** -140), m)
    return m


def epilogue(pre, bias, act, mask, mslope, addend, mask_channels, P=None):
    """out = act(pre + bias) [x factor where mask <= 0] [+ addend] (mask_channels: channel prefix, after the addend),
    in pre's dtype; with P: the bound's absolute values alongside."""
    y = pre if bias is None else pre + bias.to(pre.dtype).view(1, -1, 1, 1)
    if P is not None and bias is not None:
        P = P + bias.double().abs().view(1, -1, 1, 1)
    if act == 1:
        y = torch.relu(y)
    elif act == 2:
        y = torch.where(y > 0, y, y * torch.tensor(SLOPE, dtype=y.dtype))
    fac = None
    if mask is not None:
        fac = torch.where(mask > 0, torch.ones((), dtype=y.dtype), torch.tensor(mslope, dtype=y.dtype))
        if mask_channels == 0:
            y = y * fac
            P = None if P is None else P * fac.double()
    if addend is not None:
        y = y + addend.to(y.dtype)
        P = None if P is None else P + addend.double().abs()
    if mask is not None and mask_channels > 0:
        c = mask_channels
        y = torch.cat([y[:, :c] * fac[:, :c], y[:, c:]], 1)
        P = None if P is None else torch.cat([P[:, :c] * fac[:, :c].double(), P[:, c:]], 1)
    return y, P


# --------------------------------------------------------------------------- conv3x3 references (cached per shape)
@functools.lru_cache(maxsize=8)
def conv3x3_problem(B, K, N, H, W, backward, seed, algo, partials_key):
    """inputs, effective weights, the float64 result, its bound P, and the fp32 emulation of `algo` with the kernel's
    partial sums (partials_key: chunk_partials splits)."""
    gen = torch.Generator().manual_seed(seed * 7919 + K * 131 + N * 17 + H * W)
    x = torch.randn(B, K, H, W, generator=gen)
    # the Conv2d weight: forward [N][K][3][3]; data gradient of a Conv2d N -> K: [K][N][3][3], flipped and transposed
    wt = torch.randn(*((K, N) if backward else (N, K)), 3, 3, generator=gen) / (9 * K) ** .5
    weff = wt.transpose(0, 1).flip(-1, -2) if backward else wt
    bias = torch.randn(N, generator=gen)
    want = F.conv2d(x.double(), weff.double(), padding=1)
    P = wg.winograd_conv3x3(x.double(), weff.double(), algo, absval=True)
    emu = wg.winograd_conv3x3(x, weff, algo, dtype=torch.float32, partials=wg.chunk_partials(K, list(partials_key)))
    return x, wt, bias, want, P, emu


def pack_conv3x3(wt, K, N, backward):
    """pcfa_conv3x3_pack_weights into a NaN-fenced buffer; checks the fences and that both packings can be made at once."""
    lib = _lib()
    Cout, Cin = (K, N) if backward else (N, K)
    fw = Fenced(wt.shape, _dense_stride(wt.shape), NAN_BITS).write(wt)
    fp = Fenced((int(lib.pcfa_conv3x3_packed_floats(Cin, Cout)),), (1,), NAN_BITS)
    fq = Fenced((int(lib.pcfa_conv3x3_packed_floats(Cout, Cin)),), (1,), NAN_BITS)
    assert lib.pcfa_conv3x3_pack_weights(fw.ptr(), fp.ptr(), fq.ptr(), Cout, Cin, stream()) == 0
    torch.cuda.synchronize()
    assert _unchanged(fw) and fp.fence_intact() and fq.fence_intact(), "packing wrote outside its buffers"
    assert bool(torch.isfinite(fp.view()).all()) and bool(torch.isfinite(fq.view()).all()), "packing left a NaN"
    packed = fq if backward else fp
    packed.bits0 = packed.buf.view(torch.int32).clone()
    return fw, packed


def effective_path(B, K, N, H, W, shift=0, workspace=True):
    """(label, F(2x2,3x3) sub-path that actually runs, algo of the arithmetic, splits, nsplit)"""
    label = wg.conv3x3_path(B, K, N, H, W, aligned=shift == 0, workspace=workspace)
    sub = label
    if label == "f43_fallthrough":
        sub = "f23_ksliced" if (wg.f23_kslices(B, K, N, H, W) > 1 and workspace) else wg.f23_launch_path(B, K, N, H, W)
    splits, nsplit = wg.conv3x3_splits(sub, B, K, N, H, W)
    algo = "f43" if sub in ("f43_split", "f43_direct") else "f23"
    return label, sub, algo, splits, nsplit


def run_conv3x3(record_property, B, K, N, H, W, act=0, bias=True, mask=None, addend=False, mask_channels=0,
                backward=False, shift=0, entry="run", workspace=True, seed=0):
    """One conv3x3 call on fenced buffers through `entry` (run | fwd | act_fwd | masked_fwd | fused_bwd); mask:
    None | 0.0 | SLOPE (the mask's slope)."""
    lib = _lib()
    label, sub, algo, splits, nsplit = effective_path(B, K, N, H, W, shift, workspace)
    if entry != "run":   # the older entry points go straight to the F(2x2,3x3) launcher
        sub = wg.f23_launch_path(B, K, N, H, W)
        algo, (splits, nsplit) = "f23", wg.conv3x3_splits(sub, B, K, N, H, W)
    record_property("path", label if entry == "run" else "f23:" + entry)
    record_property("kernel", sub)
    x, wt, b, want, P, emu = conv3x3_problem(B, K, N, H, W, backward, seed, algo, tuple(splits))
    gen = torch.Generator().manual_seed(seed + 17)
    fw, fp = pack_conv3x3(wt, K, N, backward)
    fx = Fenced(x.shape, _dense_stride(x.shape), NAN_BITS, shift).write(x)
    fb = Fenced((N,), (1,), NAN_BITS).write(b) if bias else None
    mk = _mask_tensor((B, N, H, W), gen) if mask is not None else None
    ad = torch.randn(B, N, H, W, generator=gen) if addend else None
    fm = Fenced(mk.shape, _dense_stride(mk.shape), NAN_BITS).write(mk) if mk is not None else None
    fa = Fenced(ad.shape, _dense_stride(ad.shape), NAN_BITS).write(ad) if ad is not None else None
    fo = Fenced((B, N, H, W), _dense_stride((B, N, H, W)), SENTINEL)
    wbytes = int(lib.pcfa_conv3x3_workspace_bytes(B, K, N, H, W))
    assert wbytes == wg.conv3x3_workspace_bytes(B, K, N, H, W)
    fws = Fenced((max(wbytes // 4, 1),), (1,), NAN_BITS) if (wbytes and workspace) else None
    slope = SLOPE if act == 2 else (mask if mask is not None else 0.0)
    p = lambda f: f.ptr() if f is not None else None  # noqa: E731

    def call():
        if entry == "run":
            return lib.pcfa_conv3x3_run(fx.ptr(), fp.ptr(), p(fb), p(fm), p(fa), fo.ptr(), B, K, N, H, W, act, slope,
                                        mask_channels, p(fws), wbytes if fws is not None else 0, stream())
        if entry == "fwd":
            return lib.pcfa_conv3x3_fwd(fx.ptr(), fp.ptr(), p(fb), fo.ptr(), B, K, N, H, W, act, stream())
        if entry == "act_fwd":
            return lib.pcfa_conv3x3_act_fwd(fx.ptr(), fp.ptr(), p(fb), fo.ptr(), B, K, N, H, W, act, slope, stream())
        if entry == "masked_fwd":
            return lib.pcfa_conv3x3_masked_fwd(fx.ptr(), fp.ptr(), p(fm), fo.ptr(), B, K, N, H, W, stream())
        return lib.pcfa_conv3x3_fused_bwd(fx.ptr(), fp.ptr(), p(fm), p(fa), fo.ptr(), B, K, N, H, W, stream())

    assert call() == 0
    torch.cuda.synchronize()
    out = fo.view().clone()
    for f in (fw, fp, fx, fb, fm, fa):
        assert f is None or _unchanged(f), "an input was written"
    assert fo.fence_intact(), "a store landed outside out"
    assert fws is None or fws.fence_intact(), "a store landed outside the workspace"
    assert bool(torch.isfinite(out).all()), "non-finite output: a sentinel, or a NaN read from a fence"
    # second call: other garbage in the workspace and the output
    if fws is not None:
        fws.view().view(torch.int32).fill_(GARBAGE_BITS)
    fo.view().fill_(-7.0)
    assert call() == 0
    torch.cuda.synchronize()
    assert torch.equal(fo.view().view(torch.int32), out.view(torch.int32)), "not repeatable bit for bit"
    out = out.cpu()

    ref, Pout = epilogue(want, b if bias else None, act, mk, mask if mask is not None else 0.0, ad, mask_channels, P)
    emu_out, _ = epilogue(emu, b if bias else None, act, mk, mask if mask is not None else 0.0, ad, mask_channels)
    n = K + nsplit + (16 if algo == "f43" else 12)
    return gates(out, ref, Pout, n, emu_out, 4 if algo == "f43" else 2, record_property)


# --------------------------------------------------------------------------- 1. the conv3x3 path matrix
PATHS = [  # (shape, label under the default environment)
    ((1, 64, 64, 55, 64), "f23_ks2"),
    ((2, 64, 96, 64, 128), "f23_plain"),
    ((1, 21, 37, 30, 68), "f23_plain_partial"),
    ((1, 8, 256, 52, 520), "f23_xcd"),             # gx = 33 x 7 = 231 tile blocks: the XCD map has dead workgroups
    ((1, 96, 64, 24, 80), "f23_ksliced"),
    ((1, 37, 24, 20, 24), "f23_ksliced"),          # K % 8 != 0: the last slice's last chunk is partial
    ((1, 192, 64, 48, 64), "f43_split"),
    ((1, 192, 64, 50, 64), "f43_split"),           # ragged last tile row
    ((1, 80, 192, 64, 256), "f43_direct"),
    ((1, 1, 1, 1, 1), "f23_plain_partial"),
    ((1, 3, 2, 3, 2), "f23_plain_partial"),
    ((2, 2, 3, 2, 3), "f23_plain_partial"),
    ((1, 16, 3, 3, 1), "f23_ks2"),
]
FALLTHROUGH = [s for s, lab in PATHS if lab.startswith("f43")]
DEFAULT_LABELS = {"f23_ks2", "f23_plain", "f23_plain_partial", "f23_xcd", "f23_ksliced", "f43_split", "f43_direct",
                  "f43_fallthrough"}


def _sid(s):
    return "x".join(map(str, s))


def test_path_table_covers_every_label():
    """The shape table reaches every path of the default policy: a policy change that moves a path's last shape off
    it fails here by name."""
    labels = {wg.conv3x3_path(*s, env={}) for s, _ in PATHS}
    labels |= {wg.conv3x3_path(*s, aligned=False, env={}) for s in FALLTHROUGH}
    for s, lab in PATHS:
        assert wg.conv3x3_path(*s, env={}) == lab, (s, lab)
    assert labels == DEFAULT_LABELS, sorted(DEFAULT_LABELS - labels)


@pytest.mark.parametrize("shape", [s for s, _ in PATHS], ids=_sid)
def test_conv3x3_path_host_rules(shape):
    lib = _lib()
    assert lib.pcfa_conv3x3_algo(*shape) == (43 if wg.use_f43(*shape) else 23)
    assert int(lib.pcfa_conv3x3_workspace_bytes(*shape)) == wg.conv3x3_workspace_bytes(*shape)


@pytest.mark.parametrize("act", [0, 1, 2])
@pytest.mark.parametrize("shape", [s for s, _ in PATHS], ids=_sid)
def test_conv3x3_run_forward(record_property, shape, act):
    """pcfa_conv3x3_run forward with bias and act 0 / 1 / 2 (slope 0.1) on every path."""
    run_conv3x3(record_property, *shape, act=act)


@pytest.mark.parametrize("shape", FALLTHROUGH, ids=_sid)
def test_conv3x3_run_f43_fallthrough(record_property, shape):
    """x one float off 16-B alignment: the F(4x4,3x3) path refuses and the F(2x2,3x3) kernel runs."""
    run_conv3x3(record_property, *shape, act=1, shift=1)


@pytest.mark.parametrize("shape", [s for s, _ in PATHS if s[1] * s[2] <= 64 * 192], ids=_sid)
def test_conv3x3_run_data_gradient(record_property, shape):
    """The data gradient through the backward packing, against conv_transpose2d in float64."""
    run_conv3x3(record_property, *shape, bias=False, backward=True)


EPILOGUES = [(1, 64, 64, 55, 64), (2, 64, 96, 64, 128), (1, 21, 37, 30, 68), (1, 96, 64, 24, 80), (1, 192, 64, 50, 64),
             (1, 80, 192, 64, 256)]


@pytest.mark.parametrize("variant", ["mask0", "mask01", "addend", "mask_then_addend", "addend_then_mask_prefix"])
@pytest.mark.parametrize("shape", EPILOGUES, ids=_sid)
def test_conv3x3_run_epilogues(record_property, shape, variant):
    """Masks (negative, +-0.0, positive subnormals; slope 0 and 0.1), an addend, and mask_channels = m after the addend,
    as data gradients through the backward packing."""
    kw = dict(mask0=dict(mask=0.0), mask01=dict(mask=SLOPE), addend=dict(addend=True),
              mask_then_addend=dict(mask=SLOPE, addend=True),
              addend_then_mask_prefix=dict(mask=0.0, addend=True, mask_channels=max(shape[2] // 2 + 3, 1)))[variant]
    run_conv3x3(record_property, *shape, bias=False, backward=True, **kw)


TAIL_PATHS = {(1, 64, 64, 55, 64): "f23_ks2", (1, 21, 37, 30, 68): "f23_plain_partial", (1, 96, 64, 24, 80): "f23_ksliced",
              (1, 192, 64, 48, 64): "f43_split", (1, 80, 192, 64, 256): "f43_direct"}


@pytest.mark.parametrize("shape", list(TAIL_PATHS), ids=_sid)
def test_conv3x3_tail_nonfinite_under_zero_mask(shape):
    """The tail's select at slope 0 (csrc/conv_tail.hpp), as a data gradient on every place that finishes an output: the
    gradient holds one +inf and one NaN, the mask is non-positive everywhere (negatives, +0.0, -0.0).
    a. mask on every channel, then the addend: the output IS the addend, bit for bit -- the convolution's value, finite or
       not, became an exact zero.  b. mask on a channel prefix after the addend: +0.0 bits in every masked channel.
    c. the same with slope 0.1: a non-zero factor multiplies, so the +inf element's pixel is non-finite in every channel."""
    B, K, N, H, W = shape
    assert wg.conv3x3_path(*shape, env={}) == TAIL_PATHS[shape]
    lib = _lib()
    gen = torch.Generator().manual_seed(K * 131 + N)
    g = torch.randn(B, K, H, W, generator=gen)
    y, x = H // 2, W // 2
    g[0, 1, y, x], g[0, K - 2, H // 3, W // 3] = float("inf"), float("nan")
    wt = torch.randn(K, N, 3, 3, generator=gen) / (9 * K) ** .5
    ad = torch.randn(B, N, H, W, generator=gen)
    sel = torch.randint(0, 3, (B, N, H, W), generator=gen)
    mk = torch.where(sel == 1, torch.zeros(()), -1 - torch.rand(B, N, H, W, generator=gen))
    mk = torch.where(sel == 2, torch.full((), -0.0), mk)
    _, fp = pack_conv3x3(wt, K, N, True)
    fg, fm, fa = (Fenced(t.shape, _dense_stride(t.shape), NAN_BITS).write(t) for t in (g, mk, ad))
    wbytes = int(lib.pcfa_conv3x3_workspace_bytes(*shape))
    fws = Fenced((wbytes // 4,), (1,), NAN_BITS) if wbytes else None

    def run(slope, mask_channels):
        fo = Fenced((B, N, H, W), _dense_stride((B, N, H, W)), SENTINEL)
        assert lib.pcfa_conv3x3_run(fg.ptr(), fp.ptr(), None, fm.ptr(), fa.ptr(), fo.ptr(), B, K, N, H, W, 0, slope,
                                    mask_channels, fws.ptr() if fws else None, wbytes, stream()) == 0
        torch.cuda.synchronize()
        assert fo.fence_intact() and (fws is None or fws.fence_intact()), "a store landed outside its buffer"
        return fo.view().cpu()

    m = N // 2 + 3
    assert torch.equal(run(0.0, 0).view(torch.int32), ad.view(torch.int32)), "a: output != addend"
    assert not bool(run(0.0, m)[:, :m].view(torch.int32).any()), "b: a masked channel holds other bits than +0.0"
    assert not bool(torch.isfinite(run(SLOPE, m)[0, :, y, x]).any()), "c: slope 0.1 selected instead of multiplying"


@pytest.mark.parametrize("entry", ["fwd", "act_fwd", "masked_fwd", "fused_bwd"])
@pytest.mark.parametrize("shape", [(1, 64, 64, 55, 64), (1, 21, 37, 30, 68), (2, 2, 3, 2, 3)], ids=_sid)
def test_conv3x3_older_entries(record_property, shape, entry):
    kw = dict(fwd=dict(act=1), act_fwd=dict(act=2), masked_fwd=dict(bias=False, mask=0.0),
              fused_bwd=dict(bias=False, mask=0.0, addend=True, backward=True))[entry]
    run_conv3x3(record_property, *shape, entry=entry, **kw)


def test_conv3x3_ksliced_null_workspace(record_property):
    """A K-sliced shape with no workspace falls back to the unsliced kernel and still passes the gates."""
    assert wg.conv3x3_path(1, 96, 64, 24, 80, env={}) == "f23_ksliced"
    run_conv3x3(record_property, 1, 96, 64, 24, 80, act=2, workspace=False)


def test_conv3x3_act_fwd_pair(record_property):
    """Two problems in one launch, both outputs in ONE fenced buffer with a fence between them; each passes the gates
    and equals its own pcfa_conv3x3_act_fwd call bit for bit."""
    lib = _lib()
    H, W = 20, 36
    probs = [(24, 64), (40, 32)]   # K % 8 == 0 both (one kernel instance), K % 16 != 0: no in-workgroup split alone
    gap = 4096
    sizes = [N * H * W for _, N in probs]
    fo = Fenced((sizes[0] + gap + sizes[1],), (1,), SENTINEL)
    outs, fins = [], []
    for i, (K, N) in enumerate(probs):
        x, wt, b, want, P, emu = conv3x3_problem(1, K, N, H, W, False, i, "f23", ())
        _, fp = pack_conv3x3(wt, K, N, False)
        fx = Fenced(x.shape, _dense_stride(x.shape), NAN_BITS).write(x)
        fb = Fenced((N,), (1,), NAN_BITS).write(b)
        fins.append((fx, fp, fb, b, want, P, emu))
    o1 = ctypes.c_void_p(fo.ptr().value + 4 * (sizes[0] + gap))
    (x1, p1, b1, *_), (x2, p2, b2, *_) = fins
    assert lib.pcfa_conv3x3_act_fwd_pair(x1.ptr(), p1.ptr(), b1.ptr(), fo.ptr(), probs[0][0], probs[0][1], x2.ptr(),
                                         p2.ptr(), b2.ptr(), o1, probs[1][0], probs[1][1], H, W, 2, SLOPE,
                                         stream()) == 0
    torch.cuda.synchronize()
    allv = fo.view()
    assert fo.fence_intact() and torch.equal(allv[sizes[0]:sizes[0] + gap].view(torch.int32),
                                             torch.full((gap,), SENTINEL, dtype=torch.int32, device=DEV)), \
        "a store landed outside the two outputs"
    for f in fins:
        assert all(_unchanged(g) for g in f[:3])
    outs = [allv[:sizes[0]].clone(), allv[sizes[0] + gap:].clone()]
    for i, ((K, N), out, f) in enumerate(zip(probs, outs, fins)):
        fx, fp, fb, b, want, P, emu = f
        assert wg.f23_launch_path(1, K, N, H, W) != "f23_ks2"
        solo = Fenced((1, N, H, W), _dense_stride((1, N, H, W)), SENTINEL)
        assert lib.pcfa_conv3x3_act_fwd(fx.ptr(), fp.ptr(), fb.ptr(), solo.ptr(), 1, K, N, H, W, 2, SLOPE, stream()) == 0
        torch.cuda.synchronize()
        assert torch.equal(solo.view().flatten().view(torch.int32), out.view(torch.int32)), "pair != two calls"
        ref, Pout = epilogue(want, b, 2, None, 0.0, None, 0, P)
        emu_out, _ = epilogue(emu, b, 2, None, 0.0, None, 0)
        gates(out.view(1, N, H, W).cpu(), ref, Pout, K + 13, emu_out, 2, record_property, prefix="p%d_" % i)


def test_conv3x3_refusals():
    """Refused calls return their documented status and leave out and every fence untouched."""
    lib = _lib()

    def status(shape, act=0, mask=False, mask_channels=0, packed_shift=0, ws="ok"):
        B, K, N, H, W = shape
        gen = torch.Generator().manual_seed(5)
        fx = Fenced((B, K, H, W), _dense_stride((B, K, H, W)), NAN_BITS).write(torch.randn(B, K, H, W, generator=gen))
        n = int(lib.pcfa_conv3x3_packed_floats(K, N))
        fp = Fenced((n,), (1,), NAN_BITS, packed_shift).write(torch.randn(n, generator=gen))
        fm = Fenced((B, N, H, W), _dense_stride((B, N, H, W)), NAN_BITS).write(torch.randn(B, N, H, W, generator=gen)) \
            if mask else None
        fo = Fenced((B, N, H, W), _dense_stride((B, N, H, W)), SENTINEL)
        wbytes = int(lib.pcfa_conv3x3_workspace_bytes(B, K, N, H, W))
        fw = Fenced((max(wbytes // 4, 1),), (1,), NAN_BITS)
        wptr, wlen = {"ok": (fw.ptr(), wbytes), "null": (None, wbytes), "short": (fw.ptr(), wbytes - 16)}[ws]
        st = lib.pcfa_conv3x3_run(fx.ptr(), fp.ptr(), None, fm.ptr() if fm else None, None, fo.ptr(), B, K, N, H, W,
                                  act, SLOPE, mask_channels, wptr, wlen, stream())
        torch.cuda.synchronize()
        assert torch.equal(fo.buf.view(torch.int32), fo.bits0), "a refused call touched out"
        assert all(_unchanged(f) for f in (fx, fp, fw) + ((fm,) if fm else ())), "a refused call wrote an input"
        return st

    f23, f43s = (1, 21, 37, 30, 68), (1, 192, 64, 48, 64)
    assert wg.conv3x3_path(*f43s) == "f43_split"
    for shape in (f23, f43s):
        assert status(shape, act=2, mask=True) == PCFA_ERR_INVALID_ARG
        assert status(shape, mask=True, mask_channels=shape[2] + 1) == PCFA_ERR_INVALID_ARG
        assert status(shape, act=1, mask=True, mask_channels=1) == PCFA_ERR_INVALID_ARG
        assert status(shape, packed_shift=1) == PCFA_ERR_INVALID_ARG
    assert status(f43s, ws="null") == PCFA_ERR_INVALID_ARG
    assert status(f43s, ws="short") == PCFA_ERR_INVALID_ARG


# --------------------------------------------------------------------------- 2. sepconv5
SC5 = [  # (B, Ca, Cb, Cout, H, W, vertical, label with Winograd on)
    (1, 32, 32, 128, 100, 128, 0, "wino_wide"),
    (1, 64, 0, 32, 9, 128, 0, "wino_narrow"),
    (1, 32, 32, 128, 200, 64, 1, "wino_wide"),
    (2, 40, 24, 64, 9, 64, 1, "wino_narrow"),
    (1, 32, 32, 40, 9, 68, 0, "direct_split2"),
    (1, 8, 24, 36, 5, 68, 1, "direct_fast"),
    (2, 5, 7, 9, 7, 13, 0, "direct_slow"),
    (1, 3, 0, 2, 1, 1, 1, "direct_slow"),
]
SC5_LABELS = {"wino_wide", "wino_narrow", "direct_split2", "direct_fast", "direct_slow"}


def test_sepconv5_path_table():
    lib = _lib()
    for B, Ca, Cb, Cout, H, W, v, lab in SC5:
        assert wg.sepconv5_path(B, Ca, Cb, Cout, H, W, v, env={}) == lab
        assert bool(lib.pcfa_sepconv5_uses_winograd(B, Ca, Cb, Cout, H, W, v)) == lab.startswith("wino") or \
            lib.pcfa_sepconv5_algo(-1) == 0
    assert {c[-1] for c in SC5} == SC5_LABELS


@functools.lru_cache(maxsize=4)
def sepconv5_problem(B, Cin, Cout, H, W, vertical, backward, wino, groups):
    gen = torch.Generator().manual_seed(Cin * 31 + Cout + H * W + vertical)
    x = torch.randn(B, Cin, H, W, generator=gen)
    # the Conv2d weight [Cout'][Cin'][5]; the data gradient of a Conv2d Cin' = Cout -> Cout' = Cin: flipped, transposed
    wt = torch.randn(*((Cin, Cout) if backward else (Cout, Cin)), 5, generator=gen) / (5 * Cin) ** .5
    weff = wt.transpose(0, 1).flip(-1) if backward else wt
    w4 = weff.double().unsqueeze(-1 if vertical else -2)
    pad = (2, 0) if vertical else (0, 2)
    want = F.conv2d(x.double(), w4, padding=pad)
    if wino:
        P = wg.winograd_sepconv5(x.double(), weff.double(), vertical, absval=True)
        emu = wg.winograd_sepconv5(x, weff, vertical, dtype=torch.float32,
                                   partials=wg.chunk_partials(Cin, [("interleave", groups)]))
    else:
        P = F.conv2d(x.double().abs(), w4.abs(), padding=pad)
        emu = wg.direct_sepconv5_fp32(x, weff, vertical)
    return x, wt, want, P, emu


def run_sepconv5(record_property, sepconv5_algo, case, algo, backward=False, split=None, acc=(0, 0), masked=0):
    """One sepconv5 call: split = None (pcfa_sepconv5_fwd) or Cout_a (pcfa_sepconv5_fwd_split[_masked], accumulate per
    part `acc`, masked: mask_channels of the b part)."""
    lib = _lib()
    B, Ca, Cb, Cout, H, W, v, _ = case
    if backward:   # the operator of the data gradient: input = grad_out [Cout], output = grad of [a | b]
        Ca, Cb, Cout = Cout, 0, Ca + Cb
    Cin = Ca + Cb
    sepconv5_algo(algo)
    wino = bool(lib.pcfa_sepconv5_uses_winograd(B, Ca, Cb, Cout, H, W, v))
    label = wg.sepconv5_path(B, Ca, Cb, Cout, H, W, v, enabled=algo == "winograd")
    assert wino == label.startswith("wino")
    record_property("path", label)
    groups = wg.sepconv5_wino_groups(B, Cout, H, W, v)
    x, wt, want, P, emu = sepconv5_problem(B, Cin, Cout, H, W, v, backward, wino, groups if wino else 0)
    gen = torch.Generator().manual_seed(Cout + 3)
    Cw_out, Cw_in = wt.shape[:2]
    fw = Fenced(wt.shape, _dense_stride(wt.shape), NAN_BITS).write(wt)
    fpf = Fenced((int(lib.pcfa_sepconv5_packed_floats(Cw_out, Cw_in)),), (1,), NAN_BITS)
    fpb = Fenced((int(lib.pcfa_sepconv5_packed_floats(Cw_in, Cw_out)),), (1,), NAN_BITS)
    assert lib.pcfa_sepconv5_pack_weights(fw.ptr(), fpf.ptr(), fpb.ptr(), Cw_out, Cw_in, stream()) == 0
    torch.cuda.synchronize()
    assert _unchanged(fw) and fpf.fence_intact() and fpb.fence_intact()
    fp = fpb if backward else fpf
    fp.bits0 = fp.buf.view(torch.int32).clone()
    fa = Fenced((B, Ca, H, W), _dense_stride((B, Ca, H, W)), NAN_BITS).write(x[:, :Ca])
    fb = Fenced((B, Cb, H, W), _dense_stride((B, Cb, H, W)), NAN_BITS).write(x[:, Ca:]) if Cb else None
    ca = Cout if split is None else split
    prev = torch.randn(B, Cout, H, W, generator=gen)
    accv = torch.cat([torch.full((ca,), float(acc[0])), torch.full((Cout - ca,), float(acc[1]))]).view(1, -1, 1, 1)
    oa = Fenced((B, ca, H, W), _dense_stride((B, ca, H, W)), SENTINEL)
    ob = Fenced((B, Cout - ca, H, W), _dense_stride((B, Cout - ca, H, W)), SENTINEL) if ca < Cout else None
    mk = _mask_tensor((B, Cout - ca, H, W), gen) if masked else None
    fm = Fenced(mk.shape, _dense_stride(mk.shape), NAN_BITS).write(mk) if masked else None

    def prefill(first):
        """accumulating parts: the previous values; the others: the sentinel (first call) or -7 (second call)"""
        for f, lo, hi, a in ((oa, 0, ca, acc[0]), (ob, ca, Cout, acc[1])):
            if f is None:
                continue
            if a:
                f.view().copy_(prev[:, lo:hi].to(DEV))
            elif first:
                f.view().view(torch.int32).fill_(SENTINEL)
            else:
                f.view().fill_(-7.0)

    def call():
        bp = fb.ptr() if fb else None
        if split is None:
            return lib.pcfa_sepconv5_fwd(fa.ptr(), Ca, bp, Cb, fp.ptr(), oa.ptr(), B, Cout, H, W, v, stream())
        if masked:
            return lib.pcfa_sepconv5_fwd_split_masked(fa.ptr(), Ca, bp, Cb, fp.ptr(), oa.ptr(), ca, acc[0], ob.ptr(),
                                                      acc[1], fm.ptr(), masked, B, Cout, H, W, v, stream())
        return lib.pcfa_sepconv5_fwd_split(fa.ptr(), Ca, bp, Cb, fp.ptr(), oa.ptr(), ca, acc[0],
                                           ob.ptr() if ob else None, acc[1], B, Cout, H, W, v, stream())

    outs = []
    for i in range(2):
        prefill(i == 0)
        assert call() == 0
        torch.cuda.synchronize()
        got = torch.cat([oa.view()] + ([ob.view()] if ob is not None else []), 1).clone()
        outs.append(got)
        assert oa.fence_intact() and (ob is None or ob.fence_intact()), "a store landed outside the output"
        assert all(_unchanged(f) for f in (fa, fb, fp, fm) if f is not None), "an input was written"
        assert bool(torch.isfinite(got).all())
    assert torch.equal(outs[0].view(torch.int32), outs[1].view(torch.int32)), "not repeatable bit for bit"
    ref = want + accv.double() * prev.double()
    Pout = P + accv.double() * prev.double().abs()
    em = emu + accv * prev
    if masked:
        fac = torch.cat([torch.ones(B, ca, H, W), torch.cat([(mk[:, :masked] > 0).float(),
                                                              torch.ones(B, Cout - ca - masked, H, W)], 1)], 1)
        ref, Pout, em = ref * fac.double(), Pout * fac.double(), em * fac
    n = Cin + 10 if wino else 5 * Cin + 2
    gates(outs[0].cpu(), ref, Pout, n, em, 2, record_property)


@pytest.mark.parametrize("algo", ["winograd", "direct"])
@pytest.mark.parametrize("case", SC5, ids=lambda c: "%s-%dx%d+%dx%dx%dx%d-v%d" % ((c[-1],) + c[:-1]))
def test_sepconv5_fwd(record_property, sepconv5_algo, case, algo):
    run_sepconv5(record_property, sepconv5_algo, case, algo)


@pytest.mark.parametrize("algo", ["winograd", "direct"])
@pytest.mark.parametrize("case", [c for c in SC5 if c[3] <= 64 or c[-1] == "wino_wide"],
                         ids=lambda c: "%s-%dx%d+%dx%dx%dx%d-v%d" % ((c[-1],) + c[:-1]))
def test_sepconv5_data_gradient(record_property, sepconv5_algo, case, algo):
    run_sepconv5(record_property, sepconv5_algo, case, algo, backward=True)


SPLITS = [(SC5[0], 64), (SC5[3], 32), (SC5[4], 20), (SC5[6], 4)]


@pytest.mark.parametrize("acc", [(0, 0), (1, 0), (0, 1), (1, 1)])
@pytest.mark.parametrize("case", SPLITS, ids=lambda c: "%s-%d" % (c[0][-1], c[1]))
def test_sepconv5_fwd_split(record_property, sepconv5_algo, case, acc):
    run_sepconv5(record_property, sepconv5_algo, case[0], "winograd", split=case[1], acc=acc)


@pytest.mark.parametrize("acc", [(0, 0), (1, 1)])
@pytest.mark.parametrize("case", SPLITS, ids=lambda c: "%s-%d" % (c[0][-1], c[1]))
def test_sepconv5_fwd_split_masked(record_property, sepconv5_algo, case, acc):
    rest = case[0][3] - case[1]
    run_sepconv5(record_property, sepconv5_algo, case[0], "winograd", split=case[1], acc=acc, masked=max(rest - 3, 1))


# --------------------------------------------------------------------------- 3. the dev A/B switches
DEV_ENVS = [dict(PCFA_CONV3X3_MT="2", PCFA_F43_WAVES="6"),
            dict(PCFA_CONV3X3_RING="3", PCFA_CONV3X3_KS="1", PCFA_XCD_MAP="0", PCFA_CONV3X3_ALGO="r04")]


@pytest.mark.skipif(bool(os.environ.get("PCFA_WINOGRAD_CHILD")), reason="(the child run itself)")
def test_dev_switches():
    """This module once more in a fresh child process per switch set, one after the other; the mirror reads the same
    environment.  A child that ends by a signal or a timeout fails the test before the next one starts."""
    for extra in DEV_ENVS:
        env = dict(os.environ, PCFA_WINOGRAD_CHILD="1", **extra)
        cmd = [sys.executable, "-m", "pytest", os.path.abspath(__file__), "-q", "-x", "-rfE", "-m", "gpu",
               "-p", "no:cacheprovider",
               "-k", "not test_dev_switches"]
        try:
            r = subprocess.run(cmd, env=env, capture_output=True, text=True, timeout=600)
        except subprocess.TimeoutExpired:
            pytest.fail("child %s timed out" % extra)
        assert r.returncode >= 0, "child %s ended by signal %s" % (extra, signal.Signals(-r.returncode).name)
        assert r.returncode == 0, (extra, r.stdout[-4000:])
        assert " passed" in r.stdout and " failed" not in r.stdout, (extra, r.stdout[-2000:])
