"""pcfa_fgsm_step (pcfa_amd/csrc/attack_math.hip) through the C-ABI on fenced buffers against the torch sequence it
replaces -- fgsm_attack_step(..., clipping=True) + clamp + subtract on the same device -- bit for bit: every size at which
the kernel changes path (below / at / past one float4, one workgroup, several workgroups, a second trip of the grid-stride
loop), aligned and one-float-offset pointers, both modes, crafted gradients and images (tests/fgsm_cases.py)."""
import ctypes

import pytest
import torch

from tests import fenced, fgsm_cases
from tests.fenced import DEV, NAN_BITS, PCFA_ERR_INVALID_ARG, SENTINEL, Fenced

pytestmark = pytest.mark.gpu

SMALL = (1, 3, 4, 5, 255, 256, 257, 1025)


def _lib():
    from pcfa_amd import _hip
    return _hip.load()


def _second_trip(shift):
    """The smallest interesting n at which a thread of the launch runs its loop twice, from the kernel's own bound: a
    launch starts at most pcfa_fgsm_step_max_threads() threads, each takes one float4 (all pointers 16-byte aligned) or one
    float (otherwise) per trip.  A few elements more, so that n is no multiple of 4 either."""
    threads = _lib().pcfa_fgsm_step_max_threads()
    return threads * (4 if shift == 0 else 1) + 5


def _bits(t):
    return t.contiguous().view(torch.int32)


class _Call:
    """Eight fenced operands of n floats, `shifts[i]` floats off 16-byte alignment: x1, x2 (in / out), g1, g2, img1, img2
    (inputs, NaN fill) and d1, d2 (outputs, sentinel fill)."""

    def __init__(self, n, shifts):
        self.n = n
        self.host = fgsm_cases.table(n)
        x1, x2, g1, g2, i1, i2 = self.host
        fills = (NAN_BITS,) * 6 + (SENTINEL, SENTINEL)
        self.ops = [Fenced((n,), (1,), fill, shift=s) for fill, s in zip(fills, shifts)]
        for op, src in zip(self.ops[:6], (x1, x2, g1, g2, i1, i2)):
            op.write(src)
        assert all((op.ptr().value % 16 == 0) == (s % 4 == 0) for op, s in zip(self.ops, shifts))

    def reset(self):
        self.ops[0].write(self.host[0])
        self.ops[1].write(self.host[1])
        for op in self.ops[6:]:
            op.buf.view(torch.int32).fill_(SENTINEL)
            op.bits0 = op.buf.view(torch.int32).clone()

    def run(self, joint, n=None, null=None, epsilon=fgsm_cases.EPSILON):
        ptrs = [op.ptr() for op in self.ops]
        if null is not None:
            ptrs[null] = ctypes.c_void_p(0)
        status = _lib().pcfa_fgsm_step(*ptrs, ctypes.c_float(epsilon), int(joint), self.n if n is None else n,
                                       fenced.stream())
        torch.cuda.synchronize()
        return status

    def outputs(self):
        return [self.ops[i].view().clone() for i in (0, 1, 6, 7)]


def _check(n, shifts, joint):
    c = _Call(n, shifts)
    dev = [t.to(DEV) for t in c.host]
    want = fgsm_cases.torch_reference(*dev, fgsm_cases.EPSILON, joint)
    inputs0 = [op.buf.view(torch.int32).clone() for op in c.ops[2:6]]
    assert c.run(joint) == 0
    got = c.outputs()
    for name, g, w in zip(("x1", "x2", "d1", "d2"), got, want):
        same = _bits(g) == _bits(w)
        assert bool(same.all()), (name, n, shifts, joint, int((~same).sum()), int((~same).nonzero()[0]))
    for op in c.ops:
        assert op.fence_intact(), (n, shifts, joint)
    for op, b0 in zip(c.ops[2:6], inputs0):                     # gradients and clean images are only read
        assert torch.equal(op.buf.view(torch.int32), b0)
    for g in got[2:]:                                           # every output element was written
        assert not bool((_bits(g) == SENTINEL).any())
    c.reset()                                                   # a second call from the same state: the same bits
    assert c.run(joint) == 0
    for g, g2 in zip(got, c.outputs()):
        assert torch.equal(_bits(g), _bits(g2))


@pytest.mark.parametrize("joint", [0, 1])
@pytest.mark.parametrize("shift", [0, 1])
@pytest.mark.parametrize("n", SMALL)
def test_step_equals_torch_bitwise(n, shift, joint):
    _check(n, (shift,) * 8, joint)


@pytest.mark.parametrize("joint", [0, 1])
@pytest.mark.parametrize("shift", [0, 1])
def test_second_trip_of_the_grid_stride_loop(shift, joint):
    n = _second_trip(shift)
    assert n % 4 != 0 and n > _lib().pcfa_fgsm_step_max_threads() * (4 if shift == 0 else 1)
    _check(n, (shift,) * 8, joint)


@pytest.mark.parametrize("odd", range(8))
def test_one_unaligned_pointer_takes_the_scalar_path(odd):
    """Static buffers may be views: a single pointer that is only 4-byte aligned must switch ALL accesses to scalar ones."""
    shifts = tuple(1 if i == odd else 0 for i in range(8))
    _check(1025, shifts, odd % 2)


def test_crafted_block_is_inside_the_sizes():
    """The census of tests/test_fgsm_graph_host_cpu.py speaks about the crafted block: four of the sizes hold all of it."""
    block = len(fgsm_cases.crafted()[0])
    assert sum(n >= block for n in SMALL) >= 4 and min(SMALL) < block
    for joint in (0, 1):
        counts, _ = fgsm_cases.census(joint)
        assert all(counts[c] >= 1 for c in fgsm_cases.CLASSES), (joint, counts)


def test_invalid_arguments_launch_nothing():
    c = _Call(257, (0,) * 8)
    before = [op.buf.view(torch.int32).clone() for op in c.ops]
    assert c.run(0, n=-1) == PCFA_ERR_INVALID_ARG
    for k in range(8):
        assert c.run(1, null=k) == PCFA_ERR_INVALID_ARG, k
    assert c.run(2) == PCFA_ERR_INVALID_ARG
    assert c.run(0, n=0) == 0                                   # nothing to do is not an error -- and writes nothing
    for op, b0 in zip(c.ops, before):
        assert torch.equal(op.buf.view(torch.int32), b0)


def test_operator_checks_its_tensors():
    from pcfa_amd import hip_ops
    x = [torch.zeros(8, device=DEV) for _ in range(8)]
    hip_ops.fgsm_step(*x, 0.01, False)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        hip_ops.fgsm_step(*[t.cpu() for t in x], 0.01, False)
    with pytest.raises(ValueError):
        hip_ops.fgsm_step(*x[:7], torch.zeros(9, device=DEV), 0.01, False)
    with pytest.raises(ValueError):
        hip_ops.fgsm_step(torch.zeros(16, device=DEV)[::2], *x[1:], 0.01, False)
