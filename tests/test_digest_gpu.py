"""pcfa_digest_words / ops.tensor_digest against a numpy uint64 restatement of csrc/digest.hpp: every comparison is exact.

The four values are integer sums mod 2^64, so the reference is the definition itself and the tolerance is zero at every size,
pointer offset and index base; what can go wrong is coverage (a head, tail or grid-stride trip counted twice or not at
all), the 64-bit index path and the launch contract (capture, no allocation, nothing written next to the row)."""
import ctypes

import numpy as np
import pytest
import torch

from tests import fenced
from tests.fenced import DEV, PCFA_ERR_INVALID_ARG

pytestmark = pytest.mark.gpu

C1, C2 = np.uint64(0x9E3779B97F4A7C15), np.uint64(0xD6E8FEB86659FD93)
S32 = np.uint64(32)
SPECIALS = np.array([0x7FC00000, 0xFFC00001, 0x7F800001, 0x7F800000, 0xFF800000, 0x00000000, 0x80000000, 0x00000001,
                     0x807FFFFF, 0x7F7FFFFF, 0xFFFFFFFF], dtype=np.uint32)   # NaNs, +-Inf, +-0, denormals, max, all ones


def h_np(i):
    """digest.hpp's h on a uint64 array (numpy's uint64 arithmetic wraps mod 2^64)."""
    z = i * C1
    z ^= z >> S32
    z *= C2
    z ^= z >> S32
    return z | np.uint64(1)


def digest_np(words, index0=0):
    words = np.ascontiguousarray(words, dtype=np.uint32)
    w = words.astype(np.uint64)
    i = np.uint64(index0) + np.arange(len(words), dtype=np.uint64)
    mag = words & np.uint32(0x7FFFFFFF)
    return np.array([w.sum(dtype=np.uint64), (w * h_np(i)).sum(dtype=np.uint64), (mag > 0x7F800000).sum(),
                     (mag == 0x7F800000).sum()], dtype=np.uint64)


def random_words(n, seed):
    rng = np.random.default_rng(seed)
    w = rng.integers(0, 2 ** 32, size=n, dtype=np.uint64).astype(np.uint32)
    if n:
        at = rng.integers(0, n, size=min(n, 4 * len(SPECIALS)))
        w[at] = SPECIALS[np.arange(len(at)) % len(SPECIALS)]
    return w


def lib():
    from pcfa_amd import _hip
    return _hip.load()


class Buf:
    """n words on the device, `off` words behind a 16-byte boundary."""

    def __init__(self, words, off=0):
        self.n, self.off = len(words), off
        self.store = torch.zeros(self.n + 8, dtype=torch.int32, device=DEV)
        assert self.store.data_ptr() % 16 == 0
        self.words = self.store[off:off + self.n]
        self.words.copy_(torch.from_numpy(np.ascontiguousarray(words).view(np.int32)))

    def ptr(self, skip=0):
        return self.store.data_ptr() + 4 * (self.off + skip)


@pytest.fixture(scope="module")
def scratch():
    out = torch.zeros(4, dtype=torch.int64, device=DEV)
    ws = torch.empty((lib().pcfa_digest_workspace_bytes() + 7) // 8, dtype=torch.int64, device=DEV)
    return out, ws


def run(ptr, n, index0, scratch):
    out, ws = scratch
    out.fill_(-1)
    st = lib().pcfa_digest_words(ctypes.c_void_p(ptr), n, index0, ctypes.c_void_p(out.data_ptr()),
                                 ctypes.c_void_p(ws.data_ptr()), fenced.stream())
    assert st == 0, st
    return out.cpu().numpy().view(np.uint64)


# 2^22 + 2^20 + 11 words: more than the 256 workgroups x 1024 threads x 3 pieces x 4 words one trip of the grid-stride loop
# covers (the grid cap is pcfa_digest_workspace_bytes() / 32 workgroups), so the loop wraps; 2^21 + 1 fills a trip's second
# piece only in part
SIZES = [0, 1, 3, 4, 5, 63, 64, 65, 255, 256, 257, 1023, 1025, 2 ** 20 + 3, 2 ** 21 + 1, 2 ** 22 + 2 ** 20 + 11]


@pytest.mark.parametrize("n", SIZES)
def test_sizes_and_alignment(n, scratch):
    assert lib().pcfa_digest_workspace_bytes() // 32 * 1024 * 3 * 4 < SIZES[-1]     # the last size wraps the loop
    words = random_words(n, seed=n)
    want = digest_np(words)
    if n > 16:
        assert want[2] > 0 and want[3] > 0          # the input holds NaN and Inf patterns
    for off in range(4):
        got = run(Buf(words, off).ptr(), n, 0, scratch)
        assert np.array_equal(got, want), (n, off, got, want)


@pytest.mark.parametrize("index0", [0, 7, 2 ** 32 - 2, 2 ** 40 + 1])
def test_large_indices(index0, scratch):
    words = random_words(64, seed=5)
    for off in (0, 3):
        got = run(Buf(words, off).ptr(), 64, index0, scratch)
        assert np.array_equal(got, digest_np(words, index0)), (index0, off)
    if index0:
        assert digest_np(words, index0)[1] != digest_np(words, 0)[1]


def test_composition(scratch):
    n = 5003
    words = random_words(n, seed=9)
    buf = Buf(words, 2)
    whole = run(buf.ptr(), n, 0, scratch)
    assert np.array_equal(whole, digest_np(words))
    for a in (1, 5, n - 1):
        left = run(buf.ptr(), a, 0, scratch)
        right = run(buf.ptr(a), n - a, a, scratch)
        assert np.array_equal(left + right, whole), a      # uint64 addition wraps mod 2^64


def test_sensitivity(scratch):
    n, off = 4101, 1             # 3 head words, 1024 pieces of four, 2 tail words
    words = random_words(n, seed=3)
    base = run(Buf(words, off).ptr(), n, 0, scratch)
    for k in (0, 2, 2000, 4099, n - 1):      # word 0, a head word, a body word, a tail word, the last word
        for bit in (0, 31):
            w = words.copy()
            w[k] ^= np.uint32(1 << bit)
            got = run(Buf(w, off).ptr(), n, 0, scratch)
            assert got[0] != base[0] and got[1] != base[1], (k, bit)
            assert np.array_equal(got, digest_np(w))
    # two unequal words change places: the plain sum cannot see it, the index-weighted sum does
    for i, j in ((1, 4100), (17, 18), (5, 2049)):
        w = words.copy()
        assert w[i] != w[j]
        w[i], w[j] = words[j], words[i]
        got = run(Buf(w, off).ptr(), n, 0, scratch)
        assert got[0] == base[0] and got[1] != base[1], (i, j)


def test_signed_zero_changes_the_digest():
    from pcfa_amd import ops
    om = ops.get()
    a = torch.zeros(33, device=DEV)
    b = a.clone()
    b[20] = -0.0
    assert torch.equal(a, b)
    rows = torch.zeros((2, 4), dtype=torch.int64, device=DEV).view(torch.uint64)
    ws = torch.empty(om.digest_workspace_words(), dtype=torch.int64, device=DEV)
    om.tensor_digest(a, rows[0], ws)
    om.tensor_digest(b, rows[1], ws)
    got = rows.cpu().numpy()
    assert got[0].tolist() == [0, 0, 0, 0] and got[1][0] == 0x80000000 and got[1][1] != 0


def test_repeatable_and_nothing_else_is_written():
    n = 70001
    words = random_words(n, seed=21)
    x = fenced.Fenced((n,), (1,), fenced.NAN_BITS, shift=3)
    x.buf.view(torch.int32)[x.off:x.off + n] = torch.from_numpy(words.view(np.int32)).to(DEV)
    x.bits0 = x.buf.view(torch.int32).clone()
    row = fenced.Fenced((8,), (1,), fenced.SENTINEL, shift=2)     # four 64-bit values = eight words, 8-byte aligned
    ws = torch.empty((lib().pcfa_digest_workspace_bytes() + 7) // 8, dtype=torch.int64, device=DEV)
    got = []
    for _ in range(2):
        st = lib().pcfa_digest_words(x.ptr(), n, 0, row.ptr(), ctypes.c_void_p(ws.data_ptr()), fenced.stream())
        assert st == 0
        got.append(row.view().view(torch.int64).cpu().numpy().view(np.uint64).copy())
        row.view().view(torch.int32).fill_(fenced.SENTINEL)       # the second call starts from the sentinel again
    assert np.array_equal(got[0], got[1]) and np.array_equal(got[0], digest_np(words))
    # the NaN fence round the input was not read (the NaN count is the input's own), nothing round row or input written
    assert got[0][2] == digest_np(words)[2]
    assert row.fence_intact() and x.fence_intact()
    assert torch.equal(x.buf.view(torch.int32), x.bits0)


def test_capture_and_no_allocation():
    from pcfa_amd import ops
    om = ops.get()
    n = 70001
    x = torch.randn(n, device=DEV)
    rows = torch.zeros((1, 4), dtype=torch.int64, device=DEV).view(torch.uint64)
    ws = torch.empty(om.digest_workspace_words(), dtype=torch.int64, device=DEV)

    def bits(t):
        return t.cpu().numpy().view(np.uint32)
    seen = []

    def spy(name, args, invoke):
        seen.append(name)
        return invoke(name, *args)
    om.tensor_digest(x, rows[0], ws)                      # (first call of the process: module load)
    torch.cuda.synchronize()
    before = torch.cuda.memory_stats()["allocation.all.allocated"]
    ops.core.set_call_spy(spy)
    try:
        om.tensor_digest(x, rows[0], ws)
    finally:
        ops.core.set_call_spy(None)
    torch.cuda.synchronize()
    assert seen == ["pcfa_digest_words"]
    assert torch.cuda.memory_stats()["allocation.all.allocated"] == before
    assert np.array_equal(rows.cpu().numpy()[0], digest_np(bits(x)))

    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        om.tensor_digest(x, rows[0], ws)
    x.mul_(-1.5)
    x[7] = float("inf")
    rows.view(torch.int64).zero_()
    graph.replay()
    torch.cuda.synchronize()
    want = digest_np(bits(x))
    assert np.array_equal(rows.cpu().numpy()[0], want) and want[3] == 1


def test_views_and_other_float_types():
    from pcfa_amd import ops
    om = ops.get()
    rows = torch.zeros((4, 4), dtype=torch.int64, device=DEV).view(torch.uint64)
    ws = torch.empty(om.digest_workspace_words(), dtype=torch.int64, device=DEV)
    x = torch.randn(7, 13, 5, device=DEV)
    om.tensor_digest(x.permute(2, 0, 1), rows[0], ws)                       # through .contiguous()
    om.tensor_digest(x[:, 1:, :][..., 1:4].half(), rows[1], ws)             # through .float()
    om.tensor_digest(x.reshape(-1)[3:], rows[2], ws, index0=3)              # a view 12 bytes behind a 16-byte boundary
    om.tensor_digest(x.reshape(-1)[:3], rows[3], ws)
    got = rows.cpu().numpy()

    def bits(t):
        return t.contiguous().float().cpu().numpy().view(np.uint32).ravel()
    assert np.array_equal(got[0], digest_np(bits(x.permute(2, 0, 1))))
    assert np.array_equal(got[1], digest_np(bits(x[:, 1:, :][..., 1:4].half())))
    assert np.array_equal(got[2] + got[3], digest_np(bits(x)))


def test_argument_errors_launch_nothing():
    words = random_words(64, seed=1)
    buf = Buf(words, 0)
    out = torch.full((6,), -1, dtype=torch.int64, device=DEV)
    ws = torch.empty((lib().pcfa_digest_workspace_bytes() + 7) // 8 + 1, dtype=torch.int64, device=DEV)
    P = ctypes.c_void_p
    good = (P(buf.ptr()), 64, 0, P(out.data_ptr() + 8), P(ws.data_ptr()))
    seen = []
    for k, bad in ((0, P(0)), (0, P(buf.ptr() + 2)), (3, P(0)), (3, P(out.data_ptr() + 12)), (4, P(0)),
                   (4, P(ws.data_ptr() + 4))):
        args = list(good)
        args[k] = bad
        seen.append(lib().pcfa_digest_words(*args, fenced.stream()))
    torch.cuda.synchronize()
    assert seen == [PCFA_ERR_INVALID_ARG] * 6
    assert out.tolist() == [-1] * 6                      # nothing was launched
    # n_words == 0 writes four zeros and reads nothing (no input pointer at all)
    assert lib().pcfa_digest_words(P(0), 0, 5, good[3], good[4], fenced.stream()) == 0
    assert out.tolist() == [-1, 0, 0, 0, 0, -1]
    assert lib().pcfa_digest_words(*good, fenced.stream()) == 0
    assert np.array_equal(out[1:5].cpu().numpy().view(np.uint64), digest_np(words))
    from pcfa_amd import ops
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ops.get().tensor_digest(torch.zeros(4), out[1:5], ws)
    with pytest.raises(TypeError):
        ops.get().tensor_digest(torch.zeros(4, dtype=torch.int32, device=DEV), out[1:5], ws)
