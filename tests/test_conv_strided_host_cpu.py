"""The mirror of conv_strided.hip's host rules (tests/strided.py), the float64 references and the gates of
tests/test_conv_strided_f64_gpu.py, on the CPU (no GPU).

The mirror's invariants and its agreement with the library's host-only entry points; the float64 data gradient against
autograd; and torch's own fp32 convolutions on the CPU through both gates on every table shape: the gates are ones a
plain fp32 implementation stays within, so a kernel that misses them is wrong and not merely differently rounded.
"""
import os

import pytest
import torch
import torch.nn.functional as F

from tests import strided as st
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


def test_path_tables_and_labels():
    for table, ds, path, labels in ((st.FWD, False, st.fwd_path, st.FWD_LABELS), (st.DS, True, st.fwd_path, st.DS_LABELS),
                                    (st.BWD, False, st.bwd_path, st.BWD_LABELS),
                                    (st.DS_BWD, True, st.bwd_path, st.DS_BWD_LABELS)):
        for (B, Cin, N, k, H, W), lab in table:
            assert path(Cin, N, k, ds, **({"env": {}} if path is st.fwd_path else {})) == lab, ((B, Cin, N, k, H, W), lab)
            ok = st.bwd_supported if path is st.bwd_path else st.supported
            assert ok(Cin, N, k, H, W), (B, Cin, N, k, H, W)
        assert {lab for _, lab in table} == labels, sorted(labels - {lab for _, lab in table})
    assert st.fwd_path(8, 64, 3, env={"PCFA_S2_WN": "4"}) == "res_wn4" and st.fwd_path(8, 64, 3, True) == "ds_wn2"


def test_chunks_tiles_and_rows_per_workgroup():
    for (B, Cin, N, k, H, W), lab in st.FWD + st.DS + st.BWD + st.DS_BWD:
        n = st.chunks(lab, Cin, N)
        assert lab == "stem" and n == 1 or n % 2 == 0 and n >= 2, (lab, n)
        real = {"stem": 1, "stem_bwd": -(-N // 8)}.get(lab, -(-N // 4) if "bwd" in lab else -(-Cin // 4))
        assert 0 <= n - real <= 1
    assert st.chunks("res_wn1", 10, 24) == 4 and st.chunks("stem_bwd", 3, 20) == 4 and st.chunks("res_bwd_wn1", 5, 10) == 4
    assert [st.pixel_tile(p) for p in ("stem", "res_wn1", "res_wn2", "res_wn3", "res_wn4")] == [128, 128, 64, 32, 32]
    assert [st.pixel_tile(p) for p in ("stem_bwd", "ds_bwd_wn1", "res_bwd_wn2", "res_bwd_wn3", "ds_bwd_wn4")] == \
        [64, 128, 64, 32, 32]
    B, Cin, N, k, H, W = st.RPW_SHAPE
    assert st.fwd_path(Cin, N, k, env={}) == "res_wn4"
    assert st.rows_per_workgroup("res_wn4", B, N, H // 2, W // 2, env={}) == 2
    assert st.rows_per_workgroup("res_wn4", B - 1, N, H // 2, W // 2, env={}) == 1
    assert st.rows_per_workgroup("res_wn4", B, N, H // 2, W // 2, env={"PCFA_S2_RPW": "3"}) == 3
    assert st.rows_per_workgroup("stem", 2, 64, 544, 960, env={}) == 4      # the 1088 x 1920 stem: 8 * 136 * 2 = 2176 at rpw 2
    for (B, Cin, N, k, H, W), lab in st.FWD + st.DS:                          # no table shape is large enough on its own
        assert st.rows_per_workgroup(lab, B, N, *st.out_hw(k, H, W), env={}) == 1
    g = st.regions("res_wn1", 5, 260, rpw=3)
    assert g["last_tile"][1] == slice(256, 260) and g["last_rows"][0] == slice(3, 5) and "class00" not in g
    g = st.regions("stem_bwd", 9, 264)
    assert g["last_tile"][1] == slice(256, 264) and g["last_rows"][0] == slice(8, 9) and g["class11"][0] == slice(1, None, 2)


def test_mirror_matches_host():
    """pcfa_conv_s2_supported, pcfa_conv_s2_bwd_supported and the *_packed_floats entry points against the mirror."""
    bad = st.host_rule_mismatches(_lib())
    assert not bad, bad[:10]


@pytest.mark.parametrize("case", st.BWD + st.DS_BWD, ids=lambda c: "%s-%s" % (c[1], st.sid(c[0])))
def test_f64_data_gradient_equals_autograd(case):
    (B, Cin, N, k, H, W), lab = case
    ds = lab.startswith("ds")
    g, gd, w, wd, want, P, emu = st.bwd_problem(B, Cin, N, k, H, W, ds)
    x = torch.zeros(B, Cin, H, W, dtype=torch.float64, requires_grad=True)
    y = (F.conv2d(x, w.double(), stride=2, padding=k // 2) * g.double()).sum()
    if ds:
        y = y + (F.conv2d(x, wd.double(), stride=2) * gd.double()).sum()
    y.backward()
    assert want.shape == x.grad.shape
    assert wg.rel_l2_64(want, x.grad) < 1e-14
    assert bool((P >= want.abs() * (1 - 1e-12)).all())
    assert wg.rel_l2_64(emu, want) < 1e-5, "the emulation is not this sum"   # a misplaced tap is an error of order 1


@pytest.mark.parametrize("act", [0, 1, 2])
@pytest.mark.parametrize("case", st.FWD + st.DS, ids=lambda c: "%s-%s" % (c[1], st.sid(c[0])))
def test_torch_fp32_forward_passes_the_gates(case, act):
    (B, Cin, N, k, H, W), lab = case
    ds = lab.startswith("ds")
    x, w, wd, b, bd, outs = st.fwd_problem(B, Cin, N, k, H, W, ds)
    bias = act != 0
    rg = lambda h, w_, m: st.regions(lab, h, w_, 3)  # noqa: E731
    want, P, emu = outs[0]
    assert wg.rel_l2_64(emu, want) < 1e-5, "the emulation is not this sum"   # a misplaced tap is an error of order 1
    got = st.activate(F.conv2d(x, w, b if bias else None, stride=2, padding=k // 2), act)
    bb = b.view(1, -1, 1, 1) if bias else torch.zeros(1, N, 1, 1)
    gates(got, st.activate(want + bb.double(), act), P + bb.double().abs(), st.fwd_terms(Cin, k),
          st.activate(emu + bb, act), 0, _norecord, regions=rg)
    if ds:
        want, P, emu = outs[1]
        got = F.conv2d(x, wd, bd if bias else None, stride=2)
        bb = bd.view(1, -1, 1, 1) if bias else torch.zeros(1, N, 1, 1)
        gates(got, want + bb.double(), P + bb.double().abs(), Cin + 1, emu + bb, 0, _norecord, regions=rg)


@pytest.mark.parametrize("case", st.BWD + st.DS_BWD, ids=lambda c: "%s-%s" % (c[1], st.sid(c[0])))
def test_torch_fp32_data_gradient_passes_the_gates(case):
    (B, Cin, N, k, H, W), lab = case
    ds = lab.startswith("ds")
    g, gd, w, wd, want, P, emu = st.bwd_problem(B, Cin, N, k, H, W, ds)
    got = st.grad_f64(g, w, H, W, gd if ds else None, wd if ds else None)
    assert got.dtype == torch.float32
    gates(got, want, P, st.bwd_terms(Cin, N, k, ds), emu, 0, _norecord, regions=lambda h, w_, m: st.regions(lab, h, w_))
