"""Config.mfma = "bf16x3" through the networks: which kernels a closure launches, parity of loss and gradient with the
mfma = "f32" build of the same weights and inputs, and bit identity of two runs.

The switch has effect where the hand-written GEMM core runs: the all-pairs pyramid forward (always), the attention
products under gma_gemm = "hip", the 1x1 layers under conv1x1 = "hip".  The gates are the closure gates of
tests/test_gpu_parity.py (loss 1e-4 relative, gradient rel-L2 1e-2); the measured distances are recorded as junit
properties."""
import dataclasses

import pytest
import torch

from pcfa_amd.config import DEFAULT
from tests import closure_util
from tests.fenced import DEV
from tests.util import rel_l2

pytestmark = pytest.mark.gpu

HIP_F32 = dataclasses.replace(DEFAULT, gma_gemm="hip", conv1x1="hip", gma_attention="materialised", corr="all_pairs",
                              mfma="f32")
HIP_X3 = dataclasses.replace(HIP_F32, mfma="bf16x3")
LIB = dataclasses.replace(HIP_F32, gma_gemm="lib", conv1x1="lib")
H, W = 128, 160


def _closure(net, config, seed=21):
    return closure_util.run_closure(net, H, W, "change_of_variables", False, "neg_flow", "aee", seed, torch.device(DEV),
                                    config=config)


def _closure_kernel_names(config):
    """The profiler pass of tests/test_gma_streamed_gpu.py: kernel names of one eager GMA closure."""
    import bench
    from torch.autograd import DeviceType
    from torch.profiler import ProfilerActivity, profile
    dev = torch.device(DEV)
    model = bench.load_model("GMA", dev, True, config)
    st = bench.AttackStepper("GMA", H, W, dev, 3, use_graph=False, model=model)
    st.optimizer.zero_grad()
    st.closure_body()
    torch.cuda.synchronize()
    with profile(activities=[ProfilerActivity.CUDA]) as prof:
        st.optimizer.zero_grad()
        st.closure_body()
        torch.cuda.synchronize()
    return [e.name for e in prof.events() if e.device_type == DeviceType.CUDA]


def test_gma_closure_runs_the_bf16x3_kernels():
    """Under gma_gemm = conv1x1 = "hip" every dense product of the GEMM core moves to gemm_bf16x3_mfma_kernel: the pyramid
    forward, the 1 + 2 n + 1 + 2 = 16 attention products of n = 6 iterations and the 1x1 layers; no dense
    gemm_f32_mfma_kernel is left (the pyramid backward's gemm_f32_mfma_sparse_kernel stays fp32, by design), and the
    library (Cijk_) runs no more than under mfma = "f32" and 16 products fewer than in the gma_gemm = "lib" build."""
    n_iter = 6
    x3, f32, lib = (_closure_kernel_names(c) for c in (HIP_X3, HIP_F32, LIB))
    nx3 = sum("gemm_bf16x3_mfma_kernel" in k for k in x3)
    nf32 = sum("gemm_f32_mfma_kernel" in k for k in f32)
    assert nx3 >= 1 + 2 * n_iter + 4, nx3
    assert nx3 == nf32, (nx3, nf32)                        # kernel for kernel the same products
    assert not any("gemm_f32_mfma_kernel" in k for k in x3)
    assert any("gemm_f32_mfma_sparse_kernel" in k for k in x3)
    assert not any("bf16x3" in k for k in f32 + lib)
    cx, cf, cl = (sum(k.startswith("Cijk_") for k in ks) for ks in (x3, f32, lib))
    print("Cijk_ launches per closure: bf16x3 %d, f32/hip %d, lib %d; bf16x3 GEMM launches %d" % (cx, cf, cl, nx3))
    assert cx == cf and cl - cx >= 2 * n_iter + 4, (cx, cf, cl)


@pytest.mark.parametrize("net", ["GMA", "RAFT"])
def test_closure_parity_and_bit_identity(record_property, net):
    """Loss and gradient of the 128x160 closure under mfma = "bf16x3" against mfma = "f32" (same seeded weights, same
    inputs, gma_gemm = conv1x1 = "hip") at the closure gates of tests/test_gpu_parity.py; two bf16x3 runs are
    bit-identical."""
    a, a2, b = _closure(net, HIP_X3), _closure(net, HIP_X3), _closure(net, HIP_F32)
    assert a["loss"] == a2["loss"] and torch.equal(a["flow"], a2["flow"])
    for x, y in zip(a["grads"], a2["grads"]):
        assert torch.equal(x, y), "two runs differ"
    dl = abs(a["loss"] - b["loss"]) / abs(b["loss"])
    dg = max(rel_l2(x, y) for x, y in zip(a["grads"], b["grads"]))
    df = float((a["flow"] - b["flow"]).abs().max()) / float(b["flow"].abs().max())
    record_property("loss_rel", "%.3g" % dl)
    record_property("grad_rel_l2", "%.3g" % dg)
    record_property("flow_rel_max", "%.3g" % df)
    print("%s bf16x3 vs f32: loss rel %.3g, gradient rel-L2 %.3g, flow max-abs / max %.3g" % (net, dl, dg, df))
    assert dl <= 1e-4, dl
    assert dg < 1e-2, dg
    assert not torch.equal(a["grads"][0], b["grads"][0]), "the switch selected nothing"


def test_default_build_ignores_the_switch_where_the_library_runs():
    """mfma = "bf16x3" with the default gma_gemm = conv1x1 = "lib": only the pyramid forward changes kernels."""
    names = _closure_kernel_names(dataclasses.replace(LIB, mfma="bf16x3"))
    assert any("gemm_bf16x3_mfma_kernel" in k for k in names)
    assert not any("gemm_f32_mfma_kernel" in k for k in names)
