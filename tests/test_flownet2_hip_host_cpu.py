"""Host side of Config.flownet2_ops (no GPU): the switch, its environment variable, the in-flight rule, and the weight
transforms of pcfa_conv_gather (include/pcfa_hip.h) against F.conv2d / F.conv_transpose2d autograd in float64."""
import dataclasses
import os
import subprocess
import sys
from types import SimpleNamespace

import pytest
import torch
import torch.nn.functional as F

from pcfa_amd import attack_PCFA
from pcfa_amd import config as pcfa_config
from pcfa_amd.ops import flownet2 as fn2

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_config_flownet2_ops_validated():
    assert pcfa_config.Config().flownet2_ops == "lib"
    assert pcfa_config.Config(flownet2_ops="hip").flownet2_ops == "hip"
    with pytest.raises(ValueError, match="flownet2_ops"):
        pcfa_config.Config(flownet2_ops="miopen")


@pytest.mark.parametrize("value,expect", [(None, "lib"), ("hip", "hip"), ("lib", "lib")])
def test_pcfa_flownet2_ops_environment(value, expect):
    env = {k: v for k, v in os.environ.items() if k != "PCFA_FLOWNET2_OPS"}
    if value is not None:
        env["PCFA_FLOWNET2_OPS"] = value
    out = subprocess.run([sys.executable, "-c", "from pcfa_amd import config; print(config.DEFAULT.flownet2_ops)"],
                         cwd=ROOT, env=env, capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stderr[-2000:]
    assert out.stdout.strip().splitlines()[-1] == expect


def test_pairs_in_flight_flownet2_rule():
    """FlowNet2 goes in flight only with flownet2_ops='hip'; the refusal names the switch and its variable."""
    rule = attack_PCFA.PairsInFlight._refuse_shared_library_workspaces
    lib = SimpleNamespace(_pcfa_config=dataclasses.replace(pcfa_config.DEFAULT, flownet2_ops="lib"))
    hip = SimpleNamespace(_pcfa_config=dataclasses.replace(pcfa_config.DEFAULT, flownet2_ops="hip"))
    rule(SimpleNamespace(args=SimpleNamespace(net="FlowNet2"), model=hip))
    with pytest.raises(ValueError, match="in flight") as e:
        rule(SimpleNamespace(args=SimpleNamespace(net="FlowNet2"), model=lib))
    assert "flownet2_ops='hip'" in str(e.value) and "PCFA_FLOWNET2_OPS=hip" in str(e.value)


def parity_apply(x, wsub, offs, OH, OW):
    """The parity mode of pcfa_conv_gather restated with F.conv2d: out[.., 2a + ry, 2c + rx] =
    sum_{ci,ty,tx} wsub[2 ry + rx][co][ci][ty][tx] x[.., a + off_ry + ty, c + off_rx + tx] (zero outside x)."""
    B, T = x.shape[0], wsub.shape[-1]
    out = x.new_zeros((B, wsub.shape[1], OH, OW))
    P = 8
    xp = F.pad(x, (P, P + OW, P, P + OH))
    for ry in (0, 1):
        for rx in (0, 1):
            nh, nw = (OH - ry + 1) // 2, (OW - rx + 1) // 2
            if nh == 0 or nw == 0:
                continue
            y0, x0 = P + offs[ry], P + offs[rx]
            out[:, :, ry::2, rx::2] = F.conv2d(xp[:, :, y0:y0 + nh + T - 1, x0:x0 + nw + T - 1], wsub[2 * ry + rx])
    return out


@pytest.mark.parametrize("cin,cout,H,W", [(1024, 8, 2, 3), (6, 5, 7, 16), (9, 16, 5, 4), (3, 2, 1, 1)])
def test_deconv_parity_split_is_conv_transpose(cin, cout, H, W):
    """The four 2x2 parity windows of parity_weights reproduce conv_transpose2d(x, w, stride=2, padding=1)."""
    g = torch.Generator().manual_seed(cin + 10 * H + W)
    w = torch.randn(cin, cout, 4, 4, generator=g, dtype=torch.float64)
    x = torch.randn(2, cin, H, W, generator=g, dtype=torch.float64)
    ref = F.conv_transpose2d(x, w, stride=2, padding=1)
    got = parity_apply(x, fn2.parity_weights(w, 1), fn2.parity_offsets(4, 1), 2 * H, 2 * W)
    assert torch.allclose(got, ref, rtol=1e-12, atol=1e-12)


@pytest.mark.parametrize("k", [3, 5, 7])
@pytest.mark.parametrize("H,W", [(9, 14), (8, 16), (4, 6), (2, 3), (1, 2), (13, 27)])
def test_s2_dgrad_parity_split_is_the_data_gradient(k, H, W):
    """parity_weights(w, k // 2) applied to grad_out is the data gradient of conv2d(., w, stride=2, padding=k // 2),
    odd and even sizes (the shorter parities of an odd k carry zero taps)."""
    g = torch.Generator().manual_seed(100 * k + 10 * H + W)
    w = torch.randn(6, 5, k, k, generator=g, dtype=torch.float64)
    x = torch.randn(2, 5, H, W, generator=g, dtype=torch.float64, requires_grad=True)
    y = F.conv2d(x, w, stride=2, padding=k // 2)
    gy = torch.randn(y.shape, generator=g, dtype=torch.float64)
    (gx,) = torch.autograd.grad(y, x, gy)
    wsub = fn2.parity_weights(w, k // 2)
    assert wsub.shape == (4, 5, 6, (k + 1) // 2, (k + 1) // 2)
    assert int((wsub != 0).sum()) == 5 * 6 * k * k   # every tap in exactly one parity window
    got = parity_apply(gy, wsub, fn2.parity_offsets(k, k // 2), H, W)
    assert torch.allclose(got, gx, rtol=1e-12, atol=1e-12)


@pytest.mark.parametrize("H,W", [(7, 16), (2, 3), (5, 9)])
def test_deconv_dgrad_is_a_stride2_conv_with_the_weight_as_is(H, W):
    """The data gradient of conv_transpose2d(., w, stride=2, padding=1) is conv2d(., w, stride=2, padding=1): the gather
    mode of pcfa_conv_gather with the [Cin, Cout, 4, 4] weight unchanged."""
    g = torch.Generator().manual_seed(H * W)
    w = torch.randn(7, 3, 4, 4, generator=g, dtype=torch.float64)
    x = torch.randn(2, 7, H, W, generator=g, dtype=torch.float64, requires_grad=True)
    y = F.conv_transpose2d(x, w, stride=2, padding=1)
    gy = torch.randn(y.shape, generator=g, dtype=torch.float64)
    (gx,) = torch.autograd.grad(y, x, gy)
    assert torch.allclose(F.conv2d(gy, w, stride=2, padding=1), gx, rtol=1e-12, atol=1e-12)


def test_parity_offsets():
    assert fn2.parity_offsets(4, 1) == (-1, 0)
    assert fn2.parity_offsets(3, 1) == (0, 0)
    assert fn2.parity_offsets(5, 2) == (-1, 0)
    assert fn2.parity_offsets(7, 3) == (-1, -1)


@pytest.mark.parametrize("npar,cin,cout,t", [(1, 3, 64, 7), (1, 12, 70, 5), (1, 5, 16, 4), (4, 6, 32, 2), (4, 9, 12, 3),
                                             (1, 2, 33, 3)])
def test_gather_pack_layout(npar, cin, cout, t):
    """Element (p, co, ci, ty, tx) sits at [p][co/cot][ci/4][(co%cot)/mt][(ci%4)/ks][ty][tx][ci%ks][co%mt]; padding is
    zero."""
    mt, cot = fn2.gather_tile(cout)
    ks = 64 // mt
    shape = (npar, cout, cin, t, t)
    w = torch.arange(1, int(torch.tensor(shape).prod()) + 1, dtype=torch.float32).view(shape)
    p = fn2.gather_pack(w if npar > 1 else w[0])
    nct, nch = -(-cout // cot), -(-cin // 4)
    assert p.numel() == npar * nct * nch * cot * 4 * t * t
    steps = (4 // ks) * t * t
    for par in range(npar):
        for co in range(0, cout, 3):
            for ci in range(cin):
                for ty, tx in ((0, 0), (t - 1, 0), (t // 2, t - 1)):
                    s = ((ci % 4) // ks) * t * t + ty * t + tx
                    lane = (ci % ks) * mt + co % mt
                    idx = ((((par * nct + co // cot) * nch + ci // 4) * (cot // mt) + (co % cot) // mt) * steps + s) * 64 + lane
                    assert float(p[idx]) == float(w[par, co, ci, ty, tx])
    assert int((p != 0).sum()) == w.numel()   # every weight once, zeros elsewhere


def test_gather_tile_rule():
    assert fn2.gather_tile(3) == (16, 16) and fn2.gather_tile(16) == (16, 16)
    assert fn2.gather_tile(32) == (32, 32) and fn2.gather_tile(33) == (32, 64) and fn2.gather_tile(1024) == (32, 64)
