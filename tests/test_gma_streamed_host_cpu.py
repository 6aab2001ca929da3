"""Config.gma_attention and its host-side plumbing, without a GPU."""
import dataclasses
import os
import subprocess
import sys
from argparse import Namespace
from types import SimpleNamespace

import pytest
import torch

from pcfa_amd import attack_PCFA, ops
from pcfa_amd import config as pcfa_config
from pcfa_amd.nets import gma
from tests import closure_util

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_config_gma_attention_values():
    assert pcfa_config.Config().gma_attention == "materialised"
    assert pcfa_config.Config(gma_attention="materialised").gma_attention == "materialised"
    assert pcfa_config.Config(gma_attention="streamed").gma_attention == "streamed"
    assert dataclasses.replace(pcfa_config.Config(), gma_attention="streamed").gma_attention == "streamed"
    for bad in ("flash", "", "Streamed", None):
        with pytest.raises(ValueError, match="Config.gma_attention"):
            pcfa_config.Config(gma_attention=bad)


@pytest.mark.parametrize("value,expect", [(None, "materialised"), ("streamed", "streamed"),
                                          ("materialised", "materialised")])
def test_env_sets_default_in_fresh_interpreter(value, expect):
    env = {k: v for k, v in os.environ.items() if k != "PCFA_GMA_ATTENTION"}
    if value is not None:
        env["PCFA_GMA_ATTENTION"] = value
    p = subprocess.run([sys.executable, "-c", "from pcfa_amd import config; print(config.Config.from_env().gma_attention); "
                        "print(config.DEFAULT.gma_attention)"],
                       capture_output=True, text=True, cwd=REPO, env=env, timeout=120)
    assert p.returncode == 0, p.stderr[-2000:]
    assert p.stdout.strip().splitlines()[-2:] == [expect, expect]


def test_env_refuses_unknown_value_in_fresh_interpreter():
    env = dict(os.environ, PCFA_GMA_ATTENTION="flash")
    p = subprocess.run([sys.executable, "-c", "from pcfa_amd import config"], capture_output=True, text=True, cwd=REPO,
                       env=env, timeout=120)
    assert p.returncode != 0 and "Config.gma_attention" in p.stderr


def test_streamed_on_the_cpu_table_is_the_materialised_path_bit_for_bit(oracle_ops):
    """The CPU oracle table has no streamed_attention: the network falls back to the materialised torch path."""
    assert not hasattr(oracle_ops, "streamed_attention")
    torch.set_num_threads(8)
    dev = torch.device("cpu")
    streamed = dataclasses.replace(pcfa_config.DEFAULT, gma_attention="streamed")
    with ops.override_for_testing(oracle_ops):
        a = closure_util.run_closure("GMA", 128, 160, "change_of_variables", False, "neg_flow", "aee", 2, dev,
                                     config=streamed)
        b = closure_util.run_closure("GMA", 128, 160, "change_of_variables", False, "neg_flow", "aee", 2, dev,
                                     config=dataclasses.replace(pcfa_config.DEFAULT, gma_attention="materialised"))
    assert bool(torch.isfinite(a["flow"]).all())
    assert torch.equal(a["flow"], b["flow"]) and a["loss"] == b["loss"]
    for x, y in zip(a["grads"], b["grads"]):
        assert torch.equal(x, y)


@pytest.mark.parametrize("flag", ["position_only", "position_and_content"])
def test_position_flag_with_streamed_raises(oracle_ops, flag):
    att = gma.Attention(args=Namespace(**{flag: True}), dim=128, heads=1, max_pos_size=160, dim_head=128)
    fmap = torch.randn(1, 128, 4, 5)
    with ops.override_for_testing(oracle_ops):
        pcfa_config.attach(att, dataclasses.replace(pcfa_config.DEFAULT, gma_attention="streamed"))
        with pytest.raises(ValueError, match="streamed"):
            att(fmap)
        pcfa_config.attach(att, dataclasses.replace(pcfa_config.DEFAULT, gma_attention="materialised"))
        assert att(fmap).shape == (1, 1, 20, 20)


def test_pairs_in_flight_accepts_streamed_gma():
    rule = attack_PCFA.PairsInFlight._refuse_shared_library_workspaces

    def model(**kw):
        return SimpleNamespace(_pcfa_config=dataclasses.replace(pcfa_config.DEFAULT, **kw))
    for kw, ok in ((dict(gma_attention="streamed", gma_gemm="lib"), True),
                   (dict(gma_attention="streamed", gma_gemm="hip"), True),
                   (dict(gma_attention="materialised", gma_gemm="hip"), True),
                   (dict(gma_attention="materialised", gma_gemm="lib"), False)):
        attack = SimpleNamespace(args=SimpleNamespace(net="GMA"), model=model(**kw))
        if ok:
            rule(attack)
        else:
            with pytest.raises(ValueError, match="in flight"):
                rule(attack)
