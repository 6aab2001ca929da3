"""Config.mfma ("f32" | "bf16x3"): the switch, the three new C-ABI signatures, and the two facts of bf16 arithmetic the
GPU bound of tests/test_gemm_bf16x3_gpu.py rests on -- checked with torch's round-to-nearest bfloat16.  No GPU."""
import dataclasses

import pytest
import torch

U = 2.0 ** -24


# --------------------------------------------------------------------------- Config
def test_config_default_is_f32():
    from pcfa_amd.config import Config
    assert Config().mfma == "f32"
    assert dataclasses.fields(Config)[[f.name for f in dataclasses.fields(Config)].index("mfma")].default == "f32"


def test_config_rejects_other_arithmetics():
    from pcfa_amd.config import Config
    with pytest.raises(ValueError, match="mfma"):
        Config(mfma="tf32")
    assert Config(mfma="bf16x3").mfma == "bf16x3"


def test_config_from_env(monkeypatch):
    from pcfa_amd.config import Config
    monkeypatch.setenv("PCFA_MFMA", "bf16x3")
    assert Config.from_env().mfma == "bf16x3"
    monkeypatch.delenv("PCFA_MFMA")
    assert Config.from_env().mfma == "f32"
    monkeypatch.setenv("PCFA_MFMA", "tf32")
    with pytest.raises(ValueError, match="mfma"):
        Config.from_env()


def test_config_replace():
    from pcfa_amd.config import DEFAULT
    c = dataclasses.replace(DEFAULT, mfma="bf16x3")
    assert c.mfma == "bf16x3" and dataclasses.replace(c, mfma="f32") == dataclasses.replace(DEFAULT, mfma="f32")


def test_operators_take_the_switch_as_a_keyword():
    """Handed down as a keyword with default "f32", like gemm=; no module global."""
    import inspect
    from pcfa_amd.ops import conv, corr, gma
    for fn in (gma.gemm_f32, gma._attn_mm, gma.attention_softmax, gma.AttnGradShare.__init__, corr.CorrBlock.__init__,
               conv.conv1x1):
        assert inspect.signature(fn).parameters["mfma"].default == "f32", fn
    assert gma.gemm_entry("f32") == "pcfa_gemm_f32" and gma.gemm_entry("bf16x3") == "pcfa_gemm_bf16x3"
    with pytest.raises(ValueError):
        gma.gemm_entry("tf32")
    with pytest.raises(ValueError):
        gma.AttnGradShare("hip", "tf32")


# --------------------------------------------------------------------------- signatures
def test_signatures_match_their_fp32_twins():
    from pcfa_amd import _hip
    for new, twin in (("pcfa_gemm_bf16x3_workspace_bytes", "pcfa_gemm_f32_workspace_bytes"),
                      ("pcfa_gemm_bf16x3", "pcfa_gemm_f32"),
                      ("pcfa_corr_pyramid_fwd_bf16x3", "pcfa_corr_pyramid_fwd")):
        assert new in _hip.SIGNATURES, new
        assert _hip.SIGNATURES[new] == _hip.SIGNATURES[twin], new


# --------------------------------------------------------------------------- the split
def _bf(x):
    return x.to(torch.bfloat16).to(torch.float32)   # round to nearest even


def split3(a):
    """a0 = bf16(a), a1 = bf16(a - a0), a2 = bf16(a - a0 - a1), every step in fp32 (as csrc/gemm_bf16x3.hip splits)."""
    a0 = _bf(a)
    r1 = a - a0
    a1 = _bf(r1)
    r2 = r1 - a1
    a2 = _bf(r2)
    return a0, a1, a2


def _mantissas(n, seed):
    g = torch.Generator().manual_seed(seed)
    bits = torch.randint(0, 1 << 23, (n,), generator=g, dtype=torch.int32)
    edge = torch.tensor([0, 1, (1 << 23) - 1, (1 << 23) - 2,                 # 1, 1 + ulp, all ones
                         0x7F, 0x80, 0x81, 0x7FFF, 0x8000, 0x8001,           # around the bf16 half-way points
                         0x17FFF, 0x18000, 0x18001, 0x3F8000, 0x3F7FFF, 0x408000, 0x7F8000, 0x7FFF80, 0x7FFF7F,
                         0x008080, 0x018080, 0x7F7F7F, 0x010101], dtype=torch.int32)
    bits = torch.cat([edge, bits])
    x = ((127 << 23) | bits).view(torch.float32)                              # [1, 2)
    below = torch.tensor([1.0 - 2.0 ** -24, 1.0 - 2.0 ** -23], dtype=torch.float32)   # 1 - ulp
    x = torch.cat([below, x])
    return torch.cat([x, -x])


def test_split_is_exact_and_pieces_shrink():
    a = _mantissas(1 << 20, 1)
    a0, a1, a2 = split3(a)
    a64 = a.double()
    assert torch.equal(a0.double() + a1.double() + a2.double(), a64)          # exact, not merely close
    assert torch.equal((a - a0).double(), a64 - a0.double())                  # both subtractions are exact in fp32
    assert torch.equal(((a - a0) - a1).double(), a64 - a0.double() - a1.double())
    assert bool((a1.abs().double() <= 2.0 ** -8 * a64.abs()).all())
    assert bool((a2.abs().double() <= 2.0 ** -17 * a64.abs()).all())
    # the same over the exponent range the GPU test uses
    for e in (60, -60, 100, -100):
        s = a * 2.0 ** e
        s0, s1, s2 = split3(s)
        assert torch.equal(s0.double() + s1.double() + s2.double(), s.double())


def test_dropped_terms_are_below_one_ulp_of_the_product():
    """a b - sum_{i+j<=2} a_i b_j = a1 b2 + a2 b1 + a2 b2, at most u |a b|: the truncation term of the element bound."""
    a, b = _mantissas(1 << 20, 2), _mantissas(1 << 20, 3)
    b = b[torch.randperm(b.numel(), generator=torch.Generator().manual_seed(4))]
    A, B = [p.double() for p in split3(a)], [p.double() for p in split3(b)]
    six = sum(A[i] * B[j] for i in range(3) for j in range(3) if i + j <= 2)   # each product exact in float64
    exact = a.double() * b.double()
    rel = ((exact - six).abs() / exact.abs()).max().item()
    assert rel <= U, rel
    # and the three-product sum (i + j <= 1) is NOT at fp32 accuracy: the terms of order 2^-16 matter
    three = sum(A[i] * B[j] for i in range(2) for j in range(2) if i + j <= 1)
    assert ((exact - three).abs() / exact.abs()).max().item() > 16 * U


def test_a_bf16_product_is_exact_in_fp32():
    a, b = _mantissas(1 << 16, 5), _mantissas(1 << 16, 6)
    a0, b0 = _bf(a), _bf(b)
    assert torch.equal((a0 * b0).double(), a0.double() * b0.double())
