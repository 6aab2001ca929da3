"""Fenced device buffers and the rounding constants shared by the float64 kernel tests.

A Fenced operand sits inside a larger buffer whose other bits keep a fill pattern (NaN or a sentinel NaN): a kernel that
reads past its operand poisons its result with NaN, one that writes past it breaks the fence.  gamma(n) is the classic
bound on n relative roundings, gamma_n = n u / (1 - n u), u = 2^-24 (Higham, Accuracy and Stability of Numerical
Algorithms, 3.1).
"""
import ctypes

import torch

DEV = "cuda"
U = 2.0 ** -24
FENCE = 128 * 128               # floats of NaN / sentinel on each side of every operand: one 128x128 tile
SENTINEL = 0x7FC0BEEF           # a quiet NaN with a payload: C elements the kernel never wrote stay non-finite
NAN_BITS = 0x7FC00000
TINY = 2.0 ** -126              # results below the fp32 normal range may be flushed to zero
PCFA_ERR_INVALID_ARG, PCFA_ERR_UNSUPPORTED, PCFA_ERR_WORKSPACE = -1, -2, -3


def gamma(n):
    return n * U / (1 - n * U)


def stream():
    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


def _span(size, stride):
    return 1 + sum((s - 1) * st for s, st in zip(size, stride))


class Fenced:
    """A device buffer of `fill` bits with `view` (size, stride) placed `FENCE + shift` floats in: the operand's
    elements are written into it, everything else keeps the fill."""

    def __init__(self, size, stride, fill_bits, shift=0):
        self.size, self.stride, self.off = tuple(size), tuple(stride), FENCE + shift
        n = self.off + _span(size, stride) + FENCE
        self.buf = torch.full((n,), fill_bits, dtype=torch.int32, device=DEV).view(torch.float32)
        self.bits0 = self.buf.view(torch.int32).clone()
        mask = torch.ones(n, dtype=torch.bool, device=DEV)
        mask.as_strided(self.size, self.stride, self.off).fill_(False)
        self.outside = mask

    def view(self):
        return self.buf.as_strided(self.size, self.stride, self.off)

    def write(self, x):
        self.view().copy_(x.to(DEV))
        self.bits0 = self.buf.view(torch.int32).clone()
        return self

    def ptr(self):
        return ctypes.c_void_p(self.buf.data_ptr() + 4 * self.off)

    def fence_intact(self):
        return torch.equal(self.buf.view(torch.int32)[self.outside], self.bits0[self.outside])
