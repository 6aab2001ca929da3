"""Host side of Config.spynet_ops (no GPU): the switch, its environment variable, the in-flight rule and the weight packing
of pcfa_conv7x7 (include/pcfa_hip.h)."""
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
from pcfa_amd.ops import spynet as spy

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_config_spynet_ops_validated():
    assert pcfa_config.Config().spynet_ops == "lib"
    assert pcfa_config.Config(spynet_ops="hip").spynet_ops == "hip"
    with pytest.raises(ValueError, match="spynet_ops"):
        pcfa_config.Config(spynet_ops="miopen")


@pytest.mark.parametrize("value,expect", [(None, "lib"), ("hip", "hip"), ("lib", "lib")])
def test_pcfa_spynet_ops_environment(value, expect):
    env = {k: v for k, v in os.environ.items() if k != "PCFA_SPYNET_OPS"}
    if value is not None:
        env["PCFA_SPYNET_OPS"] = value
    out = subprocess.run([sys.executable, "-c", "from pcfa_amd import config; print(config.DEFAULT.spynet_ops)"],
                         cwd=ROOT, env=env, capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stderr[-2000:]
    assert out.stdout.strip().splitlines()[-1] == expect
    assert pcfa_config.Config.from_env().spynet_ops in ("lib", "hip")


def test_pairs_in_flight_spynet_rule():
    """SpyNet goes in flight only with spynet_ops='hip'; FlowNet2 stays refused."""
    rule = attack_PCFA.PairsInFlight._refuse_shared_library_workspaces
    lib = SimpleNamespace(_pcfa_config=dataclasses.replace(pcfa_config.DEFAULT, spynet_ops="lib"))
    hip = SimpleNamespace(_pcfa_config=dataclasses.replace(pcfa_config.DEFAULT, spynet_ops="hip"))
    rule(SimpleNamespace(args=SimpleNamespace(net="SpyNet"), model=hip))
    with pytest.raises(ValueError, match="in flight") as e:
        rule(SimpleNamespace(args=SimpleNamespace(net="SpyNet"), model=lib))
    assert "spynet_ops='hip'" in str(e.value) and "PCFA_SPYNET_OPS=hip" in str(e.value)
    for model in (lib, hip):
        with pytest.raises(ValueError, match="in flight"):
            rule(SimpleNamespace(args=SimpleNamespace(net="FlowNet2"), model=model))


@pytest.mark.parametrize("cin,cout", [(8, 32), (32, 64), (64, 32), (32, 16), (16, 2), (32, 8), (2, 16), (5, 70)])
def test_dgrad_weight_is_the_data_gradient(cin, cout):
    """conv2d(g, conv7x7_dgrad_weight(w), padding=3) is the data gradient of conv2d(., w, padding=3)."""
    g = torch.Generator().manual_seed(cin * 100 + cout)
    w = torch.randn(cout, cin, 7, 7, generator=g, dtype=torch.float64)
    x = torch.randn(1, cin, 9, 11, generator=g, dtype=torch.float64, requires_grad=True)
    gy = torch.randn(1, cout, 9, 11, generator=g, dtype=torch.float64)
    (gx,) = torch.autograd.grad(F.conv2d(x, w, padding=3), x, gy)
    assert torch.allclose(F.conv2d(gy, spy.conv7x7_dgrad_weight(w), padding=3), gx, rtol=1e-12, atol=1e-12)


@pytest.mark.parametrize("cin,cout", [(8, 32), (32, 64), (64, 32), (32, 16), (16, 2), (32, 8), (2, 16), (5, 70)])
def test_conv7x7_pack_layout(cin, cout):
    """Element (co, ci, ky, kx) sits at [co/cot][ci/4][(co%cot)/mt][(ci%4)/ks][ky][kx][ci%ks][co%mt]; padding is zero."""
    mt, cot = spy.conv7x7_tile(cout)
    ks = 64 // mt
    w = torch.arange(1, cout * cin * 49 + 1, dtype=torch.float32).view(cout, cin, 7, 7)
    p = spy.conv7x7_pack(w)
    nct, nch = -(-cout // cot), -(-cin // 4)
    assert p.numel() == nct * nch * cot * 4 * 49
    steps = (4 // ks) * 49
    seen = torch.zeros_like(p, dtype=torch.bool)
    for co in range(cout):
        for ci in range(cin):
            for ky in (0, 3, 6):
                for kx in (0, 5):
                    s = ((ci % 4) // ks) * 49 + ky * 7 + kx
                    lane = (ci % ks) * mt + co % mt
                    idx = ((((co // cot) * nch + ci // 4) * (cot // mt) + (co % cot) // mt) * steps + s) * 64 + lane
                    assert float(p[idx]) == float(w[co, ci, ky, kx])
                    seen[idx] = True
    assert int((p != 0).sum()) == cout * cin * 49   # every weight once, zeros elsewhere


@pytest.mark.parametrize("cin,cout", [(8, 32), (32, 64), (64, 32), (32, 16), (16, 2)])
def test_conv7x7_pack_is_the_gather_pack(cin, cout):
    """pcfa_conv7x7 is the 7x7 / stride-1 instance of pcfa_conv_gather: for every Basic layer, forward and data gradient,
    the 7x7 packer and tile rule are the gather kernel's."""
    from pcfa_amd.ops import flownet2
    w = torch.randn(cout, cin, 7, 7, generator=torch.Generator().manual_seed(cin * 100 + cout))
    for wk in (w, spy.conv7x7_dgrad_weight(w)):
        assert spy.conv7x7_tile(wk.shape[0]) == flownet2.gather_tile(wk.shape[0])
        assert torch.equal(spy.conv7x7_pack(wk), flownet2.gather_pack(wk))
