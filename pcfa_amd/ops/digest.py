"""Bit digest of a tensor (include/pcfa_hip.h: pcfa_digest_words): four exact 64-bit sums over the tensor's 32-bit words,
written into a caller's row on torch's current stream -- the record of pcfa_amd.trace.ClosureTrace."""
import torch

from .. import _hip
from .core import _call, _ptr

__all__ = ["tensor_digest", "digest_workspace_words"]


def digest_workspace_words():
    """int64 elements of the workspace one tensor_digest call in flight needs."""
    return (int(_hip.load().pcfa_digest_workspace_bytes()) + 7) // 8


def tensor_digest(t, out_row, workspace, index0=0):
    """out_row[0..3] = (sum of the words, sum of word * h(index0 + position), NaN patterns, +-Inf patterns) of the floating
    tensor t, each mod 2^64 (csrc/digest.hpp): exact, equal for equal bits whatever the launch, and additive over adjacent
    pieces.  t is read as fp32 words in C order: a non-contiguous tensor through .contiguous(), another float type through
    .float().  out_row: four contiguous uint64 (or int64: the same bits) on t's device, overwritten; workspace:
    digest_workspace_words() int64 that no other call in flight uses.  One or two launches on the current stream, no
    allocation for a dense fp32 tensor, no read-back; nothing is returned."""
    for x in (t, out_row, workspace):
        if not x.is_cuda:
            raise RuntimeError("pcfa_amd HIP operator called with a %s tensor: the MI355X path has no CPU fallback"
                               % x.device)
    if not t.is_floating_point():
        raise TypeError("tensor_digest reads floating tensors, got %s" % t.dtype)
    if out_row.dtype not in (torch.uint64, torch.int64) or out_row.numel() != 4 or not out_row.is_contiguous():
        raise ValueError("tensor_digest: out_row is four contiguous uint64, got %s %s" % (out_row.dtype, tuple(out_row.shape)))
    if workspace.dtype != torch.int64 or not workspace.is_contiguous() or workspace.numel() < digest_workspace_words():
        raise ValueError("tensor_digest: workspace is %d contiguous int64" % digest_workspace_words())
    t = t.detach()
    if not t.is_contiguous():
        t = t.contiguous()
    if t.dtype != torch.float32:
        t = t.float()
    _call("pcfa_digest_words", _ptr(t), t.numel(), int(index0), _ptr(out_row), _ptr(workspace))
