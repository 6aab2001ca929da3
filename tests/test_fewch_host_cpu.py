"""The mirror of the few-channel convolutions' host rules (tests/fewch.py), the float64 references and the gates of
tests/test_fewch_f64_gpu.py, on the CPU (no GPU).

The mirror against the library's host-only entry points; what the shape tables must cover (every path, every window
shift, the pixel and channel edges, every named group of the statistical gate with at least 256 elements somewhere);
the float64 data gradients against double autograd; the one-hot property of the references; and torch's own fp32
convolutions on the CPU through both gates on every table shape: the gates are ones a plain fp32 implementation stays
within, so a kernel that misses them is wrong and not merely differently rounded.
"""
import os

import pytest
import torch
import torch.nn.functional as F

from tests import fewch as fc
from tests import winograd as wg
from tests.gates import gates

torch.set_num_threads(min(16, torch.get_num_threads()))


def _lib():
    from pcfa_amd import _hip
    if not os.path.exists(_hip.LIB_PATH):
        import __graft_entry__
        __graft_entry__.build()
    return _hip.load()


def _norecord(*_):
    pass


def _cid(c):
    return "%s-%s" % (c[-1], fc.sid(c[0]))


# --------------------------------------------------------------------------- the mirror
def test_mirror_matches_host():
    bad = fc.host_rule_mismatches(_lib())
    assert not bad, bad[:10]


def test_mirror_invariants():
    assert fc.splits(1, 390, 15) == 6 and fc.kper(390, 6) == 80
    assert fc.splits(1, 1026, 14 * 32) == 16 and fc.kper(1026, 16) == 80
    assert fc.splits(1, 256, 55 * 128) == 1 and fc.splits(1, 255, 16) == 1 and fc.splits(1, 256, 16) == 4
    assert fc.splits(1, 100000, 1) == 64
    assert fc.csplit(1, 15, 64) == 1 and fc.csplit(1, 16, 64) == 2 and fc.csplit(1, 256, 55 * 128) == 8
    assert fc.csplit(1, 16, 128 * 256) == 1
    assert fc.wide(64) and not fc.wide(64, False) and not fc.wide(66)
    assert [sorted(fc.window_shifts(w)) for w in (8, 5, 6, 7)] == [[3], [0, 2, 3], [1, 3], [0, 2, 3]]
    assert {(c, k): fc.fewin_steps(c, k) for c, k in fc.FEWIN} == \
        {(2, 7): (49, 13, 99), (1, 7): (25, 7, 51), (2, 5): (25, 7, 51), (2, 3): (9, 3, 19)}
    assert fc.packed_floats(2, 128, 7) == 4 * 13 * 256 and fc.packed_floats(2, 129, 7) == 8 * 13 * 256
    assert fc.packed_floats(3, 8, 3) == -1 and fc.packed_floats(2, 0, 7) == -1
    assert fc.fewin_passes(2, 128, 7, 128) == (1, 1) and fc.fewin_passes(2, 200, 7, 13) == (2, 1)
    assert fc.fewin_passes(2, 4, 7, 300) == (1, 2)
    assert fc.fewin_supported(2, 256, 7, 128) and not fc.fewin_supported(2, 384, 7, 40) and fc.fewin_supported(2, 384, 7, 8)
    assert not fc.fewin_supported(*[fc.FEWIN_OVER_LDS[i] for i in (1, 2, 3, 5)])
    assert fc.fewin_supported(*[fc.FEWIN_OVER_LDS[i] for i in (1, 2, 3, 5)], packed=True)
    assert not fc.fewin_supported(*[fc.FEWIN_PACKED_OVER_LDS[i] for i in (1, 2, 3, 5)], packed=True)
    assert not fc.fewin_supported(3, 8, 3, 8) and not fc.fewin_supported(2, 8, 9, 8)


@pytest.mark.parametrize("inst", fc.FEWIN, ids=lambda i: "cin%d_k%d" % i)
@pytest.mark.parametrize("N", [1, 33, 129])
def test_packed_layout_holds_every_weight_once(inst, N):
    """Every (row, tap) of the weight appears exactly once among the live floats of the packed layout; the rest is zero."""
    Cin, k = inst
    T = fc.fewin_taps(Cin, k)
    n, tap, live = fc.packed_source(Cin, N, k)
    assert int(live.sum()) == N * T
    assert torch.equal(torch.sort(n[live] * T + tap[live])[0], torch.arange(N * T))
    w = torch.arange(1, N * T + 1, dtype=torch.float32).view(N, Cin, k, k)
    P = fc.pack_reference(w)
    assert P.numel() == fc.packed_floats(Cin, N, k) and bool((P[~live] == 0).all())
    # float q of lane l in group sg of 32-row block nb
    STEPS, SG, _ = fc.fewin_steps(Cin, k)
    nb, sg, lane, q = (N - 1) // 32, SG - 1, ((N - 1) % 32) + 32, 0
    t = 2 * (4 * sg + q) + 1
    assert float(P[((nb * SG + sg) * 64 + lane) * 4 + q]) == (float(w.view(N, T)[N - 1, t]) if t < T else 0.0)


# --------------------------------------------------------------------------- what the tables cover
def test_tables_carry_their_labels():
    for shape, _, sh, lab in fc.CONV3_FWD:
        assert fc.path("conv3_fwd", *shape, x_aligned=sh % 4 == 0) == lab, (shape, lab)
    for shape, _, lab in fc.CONV3_BWD:
        assert fc.path("conv3_bwd", *shape) == lab, (shape, lab)
    for shape, _, lab in fc.DECONV_FWD:
        assert fc.path("deconv_fwd", *shape) == lab, (shape, lab)
    for shape, lab in fc.DECONV_BWD:
        assert fc.path("deconv_bwd", *shape) == lab, (shape, lab)
    for (B, Cin, N, k, H, W), _, _, lab in fc.FEWIN_TABLE:
        assert fc.path("fewin", B, Cin, N, H, W, k) == lab, ((B, Cin, N, k, H, W), lab)
        assert fc.fewin_supported(Cin, N, k, W) and fc.fewin_supported(Cin, N, k, W, True)
    assert {c[-1] for c in fc.CONV3_FWD} == fc.FWD_LABELS
    assert {c[-1] for c in fc.DECONV_FWD} == fc.DECONV_LABELS
    assert {c[-1] for c in fc.FEWIN_TABLE} == {"fewin_w1x1", "fewin_w2x1", "fewin_w1x2"}


def _pixel_edges(shapes):
    """The pixel edges every fewout table holds (shapes: (B, K, N, H, W))."""
    pl = [(s[3] * s[4], s) for s in shapes]
    assert any(p < 64 for p, _ in pl) and any(p == 64 for p, _ in pl) and any(p % 64 == 1 for p, _ in pl)
    for pred in (lambda s: s[4] == 1, lambda s: s[3] == 1, lambda s: s[4] == 2, lambda s: s[4] > 64,
                 lambda s: s[4] == 3 and s[3] * 3 >= 64, lambda s: s[0] == 2):
        assert any(pred(s) for s in shapes)
    assert {s[2] for s in shapes} == {1, 2, 3, 4}


def _split_cases(table):
    """splits == 1 and > 1; a partial last part; an empty trailing part."""
    sk = [(fc.splits(B, K, H * W), K) for (B, K, N, H, W) in table]
    assert any(s == 1 for s, _ in sk) and any(s > 1 for s, _ in sk)
    assert any(s > 1 and (s - 1) * fc.kper(K, s) < K and K % fc.kper(K, s) for s, K in sk), "no partial last split"
    assert any(s > 1 and (s - 1) * fc.kper(K, s) >= K for s, K in sk), "no empty trailing split"


def test_conv3_fwd_table_coverage():
    t = fc.CONV3_FWD
    shapes = [c[0] for c in t]
    _pixel_edges(shapes)
    _split_cases(shapes)
    assert any(lab.startswith("plain") and s[3] * s[4] % 4 == 0 and sh == 1 for s, _, sh, lab in t)
    shifts = set()
    for s, _, _, lab in t:
        if lab == "lds_s1" and s[3] * s[4] > 64:
            shifts |= fc.window_shifts(s[4])
    assert shifts == {0, 1, 2, 3}
    for w4 in range(4):
        assert any(lab.startswith("lds") and s[4] % 4 == w4 and s[3] * s[4] > 64 for s, _, _, lab in t)
    ks = {s[1] for s in shapes}
    assert {1, 15, 17, 65, 129} <= ks
    assert any(lab.startswith("lds") and s[1] == 65 for s, _, _, lab in t)
    assert any(lab.startswith("plain") and s[1] == 129 for s, _, _, lab in t)
    assert {b for _, b, _, _ in t} == {True, False}
    for kernel in ("lds", "plain"):                       # both kernels under a split with an empty trailing part
        assert any(lab == kernel + "_split" and (fc.splits(s[0], s[1], s[3] * s[4]) - 1) * fc.kper(
            s[1], fc.splits(s[0], s[1], s[3] * s[4])) >= s[1] for s, _, _, lab in t)


def test_conv3_bwd_and_deconv_table_coverage():
    for table, flag in ((fc.CONV3_BWD, True), (fc.DECONV_BWD, False)):
        shapes = [c[0] for c in table]
        _pixel_edges(shapes)
        cs = [(fc.csplit(B, K, H * W), (B, K, N, H, W)) for (B, K, N, H, W) in shapes]
        assert any(c == 1 and s[1] < 16 for c, s in cs)
        assert any(c == 1 and s[1] >= 16 and -(-s[3] * s[4] // 64) * s[0] >= 512 for c, s in cs)
        assert any(c >= 4 and s[1] % (8 * c) and s[1] % (32 * c) for c, s in cs)
        if flag:
            assert {a for _, a, _ in table} == {True, False}
    shapes = [c[0] for c in fc.DECONV_FWD]
    _pixel_edges(shapes)
    _split_cases(shapes)
    assert {1, 15, 17, 65, 129} <= {s[1] for s in shapes}
    assert {s[3] % 2 for s in shapes} == {0, 1} and {s[4] % 2 for s in shapes} == {0, 1}
    assert {b for _, b, _ in fc.DECONV_FWD} == {True, False}


def test_fewin_table_coverage():
    t = [c[0] for c in fc.FEWIN_TABLE]
    assert {(s[1], s[3]) for s in t} == set(fc.FEWIN)
    ns = {s[2] for s in t}
    assert {1, 128, 129} <= ns and any(n % 32 for n in ns)
    assert any(fc.fewin_passes(s[1], s[2], s[3], s[5])[0] == 2 and s[2] * fc.fewin_taps(s[1], s[3]) > 16384 for s in t)
    assert any(fc.fewin_passes(s[1], s[2], s[3], s[5])[1] == 2 for s in t)
    assert any(s[2] * fc.fewin_taps(s[1], s[3]) % 4 for s in t)
    assert any(s[5] < s[3] for s in t) and any(s[5] == 1 for s in t) and any(s[4] == 1 for s in t) and any(s[0] == 2 for s in t)
    for px in (fc.FI_PX, fc.FP_PX):
        assert any(s[4] * s[5] > px and s[4] * s[5] % px for s in t)
    assert {(b, r) for _, b, r, _ in fc.FEWIN_TABLE} >= {(True, True), (False, False)}
    assert {b for _, b, _, _ in fc.FEWIN_TABLE} == {True, False} == {r for _, _, r, _ in fc.FEWIN_TABLE}


def test_every_named_region_is_gated_somewhere():
    """The statistical gate skips groups below 256 elements: per entry point every named group has a table shape that
    gives it at least that many."""
    fams = {
        "conv3_fwd": [fc.group_sizes(B, N, H, W) for (B, K, N, H, W), _, _, _ in fc.CONV3_FWD],
        "conv3_bwd": [fc.group_sizes(B, K, H, W) for (B, K, N, H, W), _, _ in fc.CONV3_BWD],
        "deconv_fwd": [fc.group_sizes(B, N, H, W, up=2) for (B, K, N, H, W), _, _ in fc.DECONV_FWD],
        "deconv_bwd": [fc.group_sizes(B, K, H, W) for (B, K, N, H, W), _ in fc.DECONV_BWD],
        "fewin": [fc.group_sizes(B, N, H, W, fc.FI_PX) for (B, Cin, N, k, H, W), _, _, _ in fc.FEWIN_TABLE],
        "fewin_packed": [fc.group_sizes(B, N, H, W, fc.FP_PX) for (B, Cin, N, k, H, W), _, _, _ in fc.FEWIN_TABLE],
    }
    for fam, sizes in fams.items():
        names = {"row0", "rowN", "col0", "colN", "seam", "last_tile"}
        if fam == "deconv_fwd":
            names |= {"class00", "class01", "class10", "class11"}
        for name in names:
            assert max(s[name] for s in sizes) >= 256, (fam, name, max(s[name] for s in sizes))
    for lds in (True, False):    # both forward kernels of the 3x3 see a gated seam and last tile
        sizes = [fc.group_sizes(B, N, H, W) for (B, K, N, H, W), _, _, lab in fc.CONV3_FWD if lab.startswith("lds") == lds]
        assert max(s["seam"] for s in sizes) >= 256 and max(s["last_tile"] for s in sizes) >= 256


# --------------------------------------------------------------------------- the references
@pytest.mark.parametrize("case", fc.CONV3_BWD, ids=_cid)
def test_conv3_f64_gradient_equals_autograd(case):
    (B, K, N, H, W), addend, _ = case
    g, w, a, want, P, emu = fc.conv3_bwd_problem(B, K, N, H, W, addend)
    x = torch.zeros(B, K, H, W, dtype=torch.float64, requires_grad=True)
    (F.conv2d(x, w.double(), padding=1) * g.double()).sum().backward()
    ref = x.grad + (a.double() if addend else 0)
    assert wg.rel_l2_64(want, ref) < 1e-14 and bool((P >= want.abs() * (1 - 1e-12)).all())
    assert wg.rel_l2_64(emu, want) < 1e-5, "the emulation is not this sum"


@pytest.mark.parametrize("case", fc.DECONV_BWD, ids=_cid)
def test_deconv_f64_gradient_equals_autograd(case):
    (B, K, N, H, W), _ = case
    g, w, want, P, emu = fc.deconv_bwd_problem(B, K, N, H, W)
    x = torch.zeros(B, K, H, W, dtype=torch.float64, requires_grad=True)
    (F.conv_transpose2d(x, w.double(), stride=2, padding=1) * g.double()).sum().backward()
    assert wg.rel_l2_64(want, x.grad) < 1e-14 and bool((P >= want.abs() * (1 - 1e-12)).all())
    assert wg.rel_l2_64(emu, want) < 1e-5, "the emulation is not this sum"


def test_one_hot_references_shift_or_scatter_the_input():
    """A weight that is 1.0 at one (o, c, ky, kx): the float64 references return the shifted (the transposed convolution:
    the class-scattered) input exactly, and so do the fp32 emulations."""
    gen = torch.Generator().manual_seed(5)
    B, K, N, H, W = 1, 3, 2, 5, 6
    x = torch.randn(B, K, H, W, generator=gen)
    xp = F.pad(x, (1, 1, 1, 1))
    for ky in range(3):
        for kx in range(3):
            w = fc.one_hot((N, K, 3, 3), (1, 2, ky, kx))
            y = fc.conv3_f64(x.double(), w.double())
            assert torch.equal(y[:, 1].float(), xp[:, 2, ky:ky + H, kx:kx + W]) and not bool(y[:, 0].any())
            assert torch.equal(fc.conv3_fwd_emulation(x, w, None, 1, 16), y.float())
            g = torch.randn(B, N, H, W, generator=gen)
            d = fc.conv3_grad_f64(g.double(), w.double())
            gp = F.pad(g, (1, 1, 1, 1))
            assert torch.equal(d[:, 2].float(), gp[:, 1, 2 - ky:2 - ky + H, 2 - kx:2 - kx + W]) and not bool(d[:, :2].any())
            assert torch.equal(fc.conv3_bwd_emulation(g, w, None), d.float())
    for ky in range(4):
        for kx in range(4):
            w = fc.one_hot((K, N, 4, 4), (2, 1, ky, kx))
            y = fc.deconv_f64(x.double(), w.double())
            exp = torch.zeros(B, 2 * H + 2, 2 * W + 2)
            exp[:, ky:ky + 2 * H:2, kx:kx + 2 * W:2] = x[:, 2]          # Y = 2y - 1 + ky, in a map padded by one
            assert torch.equal(y[:, 1].float(), exp[:, 1:-1, 1:-1]) and not bool(y[:, 0].any())
            assert torch.equal(fc.deconv_fwd_emulation(x, w, None, 1, 16), y.float())
            g = torch.randn(B, N, 2 * H, 2 * W, generator=gen)
            d = fc.deconv_grad_f64(g.double(), w.double())
            gp = F.pad(g, (1, 1, 1, 1))
            assert torch.equal(d[:, 2].float(), gp[:, 1, ky:ky + 2 * H - 1:2, kx:kx + 2 * W - 1:2]) and not bool(d[:, :2].any())
            assert torch.equal(fc.deconv_bwd_emulation(g, w), d.float())
    for Cin, k in ((2, 3), (1, 7)):
        x = torch.randn(1, Cin, 4, 9, generator=gen)
        xp = F.pad(x, (k // 2,) * 4)
        for c in range(Cin):
            for ky in range(k):
                for kx in range(k):
                    w = fc.one_hot((5, Cin, k, k), (3, c, ky, kx))
                    y = F.conv2d(x.double(), w.double(), padding=k // 2)
                    assert torch.equal(y[:, 3].float(), xp[:, c, ky:ky + 4, kx:kx + 9])
                    assert torch.equal(fc.fewin_emulation(x, w), y.float())


# --------------------------------------------------------------------------- torch's fp32 through the gates
def _gate(kind, got, want, P, n, emu, H, W, px=fc.FO_PX, up=1):
    return gates(got, want, P, n, emu, up, _norecord, regions=fc.regions, extra=fc.extra_groups(H, W, px, up))


@pytest.mark.parametrize("case", fc.CONV3_FWD, ids=_cid)
def test_torch_fp32_conv3_fwd_passes_the_gates(case):
    (B, K, N, H, W), bias, _, _ = case
    x, w, b, want, P, emu = fc.conv3_fwd_problem(B, K, N, H, W, bias)
    assert wg.rel_l2_64(emu, want) < 1e-5, "the emulation is not this sum"
    _gate("conv3_fwd", F.conv2d(x, w, b, padding=1), want, P, fc.TERMS["conv3_fwd"](K, N), emu, H, W)


@pytest.mark.parametrize("case", fc.CONV3_BWD, ids=_cid)
def test_torch_fp32_conv3_bwd_passes_the_gates(case):
    (B, K, N, H, W), addend, _ = case
    g, w, a, want, P, emu = fc.conv3_bwd_problem(B, K, N, H, W, addend)
    got = fc.conv3_grad_f64(g, w)
    assert got.dtype == torch.float32
    _gate("conv3_bwd", got + a if addend else got, want, P, fc.TERMS["conv3_bwd"](K, N), emu, H, W)


@pytest.mark.parametrize("case", fc.DECONV_FWD, ids=_cid)
def test_torch_fp32_deconv_fwd_passes_the_gates(case):
    """Under a channel split torch's transposed convolution runs once per split (the mirror's kper channels each) and the
    parts are added in split order, as the kernel does: torch sums the 4 K products of an output in ONE chain (a GEMM over
    the channels, then col2im), which at K = 300 is 3.5-4.7e-7 away from float64 where the kernel's order -- chains of 20
    products per wave, 16 waves, 4 splits -- is 1.0-1.2e-7 away: the single chain misses the statistical gate by 1.2-1.4 x,
    not by a fault but by its length.  Split as the kernel splits, torch's fp32 is 1.6-2.4e-7 away and passes."""
    (B, K, N, H, W), bias, _ = case
    x, w, b, want, P, emu = fc.deconv_fwd_problem(B, K, N, H, W, bias)
    assert wg.rel_l2_64(emu, want) < 1e-5, "the emulation is not this sum"
    s = fc.splits(B, K, H * W)
    kp = fc.kper(K, s)
    got = torch.zeros(B, N, 2 * H, 2 * W)
    for lo in range(0, K, kp):
        got = got + F.conv_transpose2d(x[:, lo:lo + kp], w[lo:lo + kp], None, stride=2, padding=1)
    got = got + b.view(1, -1, 1, 1) if bias else got
    _gate("deconv_fwd", got, want, P, fc.TERMS["deconv_fwd"](K, N), emu, H, W, up=2)


@pytest.mark.parametrize("case", fc.DECONV_BWD, ids=_cid)
def test_torch_fp32_deconv_bwd_passes_the_gates(case):
    (B, K, N, H, W), _ = case
    g, w, want, P, emu = fc.deconv_bwd_problem(B, K, N, H, W)
    got = fc.deconv_grad_f64(g, w)
    assert got.dtype == torch.float32
    _gate("deconv_bwd", got, want, P, fc.TERMS["deconv_bwd"](K, N), emu, H, W)


@pytest.mark.parametrize("case", fc.FEWIN_TABLE, ids=_cid)
def test_torch_fp32_conv_fewin_passes_the_gates(case):
    (B, Cin, N, k, H, W), bias, relu, _ = case
    x, w, b, want, P, emu = fc.fewin_problem(B, Cin, N, k, H, W, bias, relu)
    assert wg.rel_l2_64(emu, want) < 1e-5, "the emulation is not this sum"
    got = F.conv2d(x, w, b, padding=k // 2)
    got = torch.relu(got) if relu else got
    for px in (fc.FI_PX, fc.FP_PX):
        _gate("fewin", got, want, P, fc.fewin_terms(Cin, k), emu, H, W, px)
