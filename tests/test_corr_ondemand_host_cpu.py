"""Config.corr and the on-demand correlation's workspace helper, without a GPU."""
import dataclasses
import os
import subprocess
import sys

import pytest

from pcfa_amd import _hip
from pcfa_amd import config as pcfa_config

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_config_corr_values():
    assert pcfa_config.Config().corr == "all_pairs"
    assert pcfa_config.Config(corr="on_demand").corr == "on_demand"
    assert dataclasses.replace(pcfa_config.Config(), corr="on_demand").corr == "on_demand"
    with pytest.raises(ValueError, match="Config.corr"):
        pcfa_config.Config(corr="alternate")


def test_env_sets_default_in_fresh_interpreter():
    env = dict(os.environ, PCFA_CORR="on_demand")
    p = subprocess.run([sys.executable, "-c", "from pcfa_amd import config; print(config.DEFAULT.corr)"],
                       capture_output=True, text=True, cwd=REPO, env=env, timeout=120)
    assert p.returncode == 0, p.stderr[-2000:]
    assert p.stdout.strip().splitlines()[-1] == "on_demand"


def test_workspace_bytes_linear_in_queries():
    lib = _hip.load()
    sizes = [(55, 128), (110, 256), (220, 512), (440, 1024)]   # Q grows 4x per step
    got = [int(lib.pcfa_corr_ondemand_workspace_bytes(1, 256, h, w, 4)) for h, w in sizes]
    assert all(b > 0 for b in got), got
    for (h0, w0), (h1, w1), b0, b1 in zip(sizes, sizes[1:], got, got[1:]):
        ratio = b1 / b0
        assert 3.5 < ratio < 4.5, (h1, w1, ratio)   # quadratic growth would give 16x
    # 4K: a few GB, where the all-pairs pyramid alone needs ~90 GB
    assert lib.pcfa_corr_ondemand_workspace_bytes(1, 256, 270, 480, 4) < 4 * 2 ** 30
    # twice the pairs, twice the workspace
    b1 = lib.pcfa_corr_ondemand_workspace_bytes(1, 256, 55, 128, 4)
    b2 = lib.pcfa_corr_ondemand_workspace_bytes(2, 256, 55, 128, 4)
    assert 1.9 < b2 / b1 < 2.1


def test_workspace_bytes_refuses_unserved_shapes():
    lib = _hip.load()
    assert lib.pcfa_corr_ondemand_workspace_bytes(1, 255, 55, 128, 4) == 0     # D % 4 != 0
    assert lib.pcfa_corr_ondemand_workspace_bytes(1, 1024, 55, 128, 4) == 0    # D > 512
    assert lib.pcfa_corr_ondemand_workspace_bytes(1, 256, 7, 7, 4) == 0        # level 3 empty
    assert lib.pcfa_corr_ondemand_workspace_bytes(0, 256, 55, 128, 4) == 0
