"""GMA attention (models/gma/gma.py:34-77,79-115): row softmax in one pass, attention products,
the shared attention gradient; pcfa_gemm_f32.  And the same attention without the [N, N] matrix (Config.gma_attention =
"streamed"): streamed_attention / streamed_attn_times_value on pcfa_attn_stream_*."""
import ctypes
import os
import weakref

import torch

from .. import _hip
from . import core
from .core import _call, _dev, _note_work, _pair, _ptr, _ptr_off, _stream


# --------------------------------------------------------------------------- #
# GMA attention (models/gma/gma.py:34-77,79-115)
# --------------------------------------------------------------------------- #
MFMA_MODES = ("f32", "bf16x3")


def gemm_entry(mfma):
    """The GEMM core's entry point for Config.mfma: "f32" -> pcfa_gemm_f32 (v_mfma_f32_32x32x2_f32), "bf16x3" ->
    pcfa_gemm_bf16x3 (three bf16 pieces per fp32 operand, six v_mfma_f32_32x32x16_bf16 products; same contract)."""
    if mfma not in MFMA_MODES:
        raise ValueError("mfma must be 'f32' or 'bf16x3', got %r" % (mfma,))
    return "pcfa_gemm_f32" if mfma == "f32" else "pcfa_gemm_bf16x3"


def gemm_f32(a, b, a_kmajor, b_kmajor, alpha=1.0, splits=1, out=None, mfma="f32"):
    """C[..., m, n] = alpha * sum_k A(m, k) B(k, n) on the matrix cores, fp32 in and out (pcfa_gemm_f32, or
    pcfa_gemm_bf16x3 under mfma = "bf16x3").  `a` is [.., M, K] (a_kmajor = 0) or [.., K, M] (1); `b` is [.., N, K]
    (b_kmajor = 0) or [.., K, N] (1); leading dims = batch."""
    _dev(a, b)
    entry = gemm_entry(mfma)
    a, b = a.contiguous(), b.contiguous()
    M, K = (a.shape[-1], a.shape[-2]) if a_kmajor else (a.shape[-2], a.shape[-1])
    N = b.shape[-1] if b_kmajor else b.shape[-2]
    if (b.shape[-2] if b_kmajor else b.shape[-1]) != K or a.shape[:-2] != b.shape[:-2]:
        raise ValueError("gemm_f32: operand shapes %s / %s do not match" % (tuple(a.shape), tuple(b.shape)))
    batch = 1
    for d in a.shape[:-2]:
        batch *= d
    if out is None:
        out = torch.empty(a.shape[:-2] + (M, N), device=a.device, dtype=torch.float32)
    lib = _hip.load()
    ws, nbytes = None, 0
    if splits > 1:
        nbytes = int(getattr(lib, entry + "_workspace_bytes")(M, N, batch, splits))
        ws = torch.empty(nbytes // 4, device=a.device, dtype=torch.float32)
    _call(entry, _ptr(a), _ptr(b), _ptr(out), M, N, K, a.shape[-1], b.shape[-1], N, int(a_kmajor),
          int(b_kmajor), batch, M * K, N * K, M * N, float(alpha), int(splits), _ptr(ws), ctypes.c_size_t(nbytes))
    return out


def _attn_mm(a, b, a_kmajor, b_kmajor, alpha=1.0, splits=1, gemm="lib", mfma="f32"):
    """A plain GEMM of the attention block.  gemm = "lib" (Config.gma_gemm's default): the library (rocBLAS through
    torch.matmul) -- these are plain dense products and it runs them at 107-126 TFLOP/s; "hip" routes them through
    pcfa_gemm_f32 (80-105 TFLOP/s, tools/bench_gemm.py), which the parity test exercises either way.  mfma
    (Config.mfma) picks the hand-written core's arithmetic and has no effect on the library product."""
    if gemm == "hip":
        return gemm_f32(a, b, a_kmajor, b_kmajor, alpha=alpha, splits=splits, mfma=mfma)
    gemm_entry(mfma)   # validates
    at = a.transpose(-1, -2) if a_kmajor else a
    bt = b if b_kmajor else b.transpose(-1, -2)
    out = torch.matmul(at, bt)
    return out if alpha == 1.0 else out.mul_(alpha)


class _AttentionSoftmax(torch.autograd.Function):
    """attn = softmax(scale * q k^T) (gma.py:52-74, content-only branch): the similarity product (plain GEMM), then the
    row softmax as ONE read and ONE write of the [N, N] matrix, in place (pcfa_softmax_rows_fwd: a 28 KB row lives in
    the registers of one workgroup; the library makes three passes), and the same in the backward: d sim = attn * (g -
    rowsum(g * attn)) in one pass, dq = scale * dsim k, dk = scale * dsim^T q."""

    @staticmethod
    def forward(ctx, q, k, scale, gemm="lib", mfma="f32"):
        _dev(q, k)
        ctx.gemm, ctx.mfma = gemm, mfma
        q, k = q.contiguous(), k.contiguous()
        sim = _attn_mm(q, k, 0, 0, alpha=scale, gemm=gemm, mfma=mfma)            # [.., N, N]
        n = sim.shape[-1]
        _call("pcfa_softmax_rows_fwd", _ptr(sim), _ptr(sim), sim.numel() // n, n)
        ctx.scale = float(scale)
        ctx.save_for_backward(q, k, sim)
        return sim

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, g):
        q, k, attn = ctx.saved_tensors
        g = g.contiguous()
        n = attn.shape[-1]
        # never in place on `g`: autograd forbids mutating a gradient it hands in (a hook, retain_grad() on the attention
        # matrix or a second consumer would see the overwritten values).  Same traffic either way (one read of attn and
        # g, one write); the price is a 198 MB temporary at 55x128.
        ds = torch.empty_like(g)
        _call("pcfa_softmax_rows_bwd", _ptr(attn), _ptr(g), _ptr(ds), attn.numel() // n, n)
        mm = dict(alpha=ctx.scale, splits=8, gemm=ctx.gemm, mfma=ctx.mfma)
        dq = _attn_mm(ds, k, 0, 1, **mm) if ctx.needs_input_grad[0] else None  # dsim k
        dk = _attn_mm(ds, q, 1, 1, **mm) if ctx.needs_input_grad[1] else None  # dsim^T q
        return dq, dk, None, None, None


def attention_softmax(q, k, scale, gemm="lib", mfma="f32"):
    """softmax(scale * q k^T, dim=-1) for q, k [.., N, d]; gemm: "lib" | "hip" (Config.gma_gemm); mfma: "f32" |
    "bf16x3" (Config.mfma; the arithmetic of the "hip" products)."""
    return _AttentionSoftmax.apply(q, k, scale, gemm, mfma)


class AttnGradShare:
    """One attention matrix multiplied by a different value tensor in every refinement iteration (gma.py:79-115 called
    from update.py:128-130): its gradient is sum_i g_i v_i^T.  The nodes park (g_i, v_i); whichever runs last forms
    ONE product [g_1 | .. | g_n] [v_1 | .. | v_n]^T (K = n * 128) instead of n read-modify-write products over the
    198 MB matrix."""

    def __init__(self, gemm="lib", mfma="f32"):
        self.pending = 0
        self.gs, self.vs = [], []
        self.gemm = gemm   # "lib" | "hip" (Config.gma_gemm): which GEMM the nodes sharing this object run
        self.mfma = mfma   # "f32" | "bf16x3" (Config.mfma): the arithmetic of the "hip" products
        gemm_entry(mfma)


class _AttnTimesValue(torch.autograd.Function):
    @staticmethod
    def forward(ctx, attn, v, shared):
        _dev(attn, v)
        v = v.contiguous()
        ctx.save_for_backward(attn, v)
        ctx.shared = shared
        shared.pending += 1
        return _attn_mm(attn, v, 0, 1, splits=8, gemm=shared.gemm, mfma=shared.mfma)     # [.., N, d]

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, g):
        attn, v = ctx.saved_tensors
        sh = ctx.shared
        g = g.contiguous()
        dv = _attn_mm(attn, g, 1, 1, splits=8, gemm=sh.gemm, mfma=sh.mfma) if ctx.needs_input_grad[1] else None     # attn^T g
        d_attn = None
        if ctx.needs_input_grad[0]:
            if sh.pending <= 0:
                raise RuntimeError("GMA attention gradient: backward re-entered after the shared buffers were released; "
                                   "run a fresh forward (retain_graph is not supported on this path)")
            sh.gs.append(g)
            sh.vs.append(v)
            sh.pending -= 1
            if sh.pending == 0:
                gcat, vcat = torch.cat(sh.gs, dim=-1), torch.cat(sh.vs, dim=-1)
                sh.gs, sh.vs = [], []
                d_attn = _attn_mm(gcat, vcat, 0, 0, gemm=sh.gemm, mfma=sh.mfma)      # [.., N, N], K = n * d
        return d_attn, dv, None


def attn_times_value(attn, v, shared):
    return _AttnTimesValue.apply(attn, v, shared)


# --------------------------------------------------------------------------- #
# The same attention without the [N, N] matrix (Config.gma_attention = "streamed"; csrc/gma_attn_stream.hip)
# --------------------------------------------------------------------------- #
class StreamedAttention:
    """Handle of softmax(scale * q k^T) that never forms the matrix: q, k [.., N, 128], the scale and the row statistics
    lse [.., N], computed once on first use (the attention depends on the context features only, so every refinement
    iteration shares them).  It also carries what AttnGradShare carries: the nodes of the iterations park (g_i, v_i) and
    add their <g_i, out_i> to delta; whichever runs last makes ONE pcfa_attn_stream_dqk pass over all of them."""

    def __init__(self, q, k, scale):
        _dev(q, k)
        if q.shape != k.shape:
            raise ValueError("streamed_attention: q %s and k %s differ in shape" % (tuple(q.shape), tuple(k.shape)))
        self.q, self.k, self.scale = q.contiguous(), k.contiguous(), float(scale)
        self.N, self.d = q.shape[-2], q.shape[-1]
        self.BH = q.numel() // (self.N * self.d)
        self._lse = None
        self.pending = 0
        self.gs, self.vs, self.delta = [], [], None

    def lse(self):
        if self._lse is None:
            q, k = self.q.detach(), self.k.detach()
            lse = torch.empty(q.shape[:-1], device=q.device, dtype=torch.float32)
            _call("pcfa_attn_stream_lse", _ptr(q), _ptr(k), _ptr(lse), self.BH, self.N, self.d, self.scale)
            self._lse = lse
        return self._lse


def streamed_attention(q, k, scale):
    """The handle of softmax(scale * q k^T, dim=-1) for q, k [.., N, 128]; multiply it with streamed_attn_times_value."""
    return StreamedAttention(q, k, scale)


def _stream_fwd(h, q, k, v):
    out = torch.empty_like(v)
    _call("pcfa_attn_stream_fwd", _ptr(q), _ptr(k), _ptr(v), _ptr(h.lse()), _ptr(out), h.BH, h.N, h.d, h.scale)
    return out


class _StreamedAttnTimesValue(torch.autograd.Function):
    """out_i = softmax(scale q k^T) v_i, one node per refinement iteration, inputs (q, k, v_i).  Saves v_i and out_i
    ([N, 128] each).  Backward: dv_i = P^T g_i at once; (g_i, v_i) are parked and delta += <g_i, out_i>; the node that
    runs last returns dq, dk from one pass over dS = P o ([g_1|..|g_n] [v_1|..|v_n]^T - delta), the others None."""

    @staticmethod
    def forward(ctx, q, k, v, h):
        v = v.contiguous()
        out = _stream_fwd(h, q, k, v)
        ctx.save_for_backward(q, k, v, out)
        ctx.h = h
        h.pending += 1
        return out

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, g):
        q, k, v, out = ctx.saved_tensors
        h = ctx.h
        g = g.contiguous()
        dv = None
        if ctx.needs_input_grad[2]:
            dv = torch.empty_like(v)
            _call("pcfa_attn_stream_dv", _ptr(q), _ptr(k), _ptr(g), _ptr(h.lse()), _ptr(dv), h.BH, h.N, h.d, h.scale)
        dq = dk = None
        if ctx.needs_input_grad[0] or ctx.needs_input_grad[1]:
            if h.pending <= 0:
                raise RuntimeError("GMA attention gradient: backward re-entered after the shared buffers were released; "
                                   "run a fresh forward (retain_graph is not supported on this path)")
            first = h.delta is None
            if first:
                h.delta = torch.empty(q.shape[:-1], device=q.device, dtype=torch.float32)
            _call("pcfa_attn_stream_delta", _ptr(g), _ptr(out), _ptr(h.delta), h.BH * h.N, h.d, 0 if first else 1)
            h.gs.append(g)
            h.vs.append(v)
            h.pending -= 1
            if h.pending == 0:
                n = len(h.gs)
                gcat = h.gs[0] if n == 1 else torch.cat(h.gs, dim=-1)
                vcat = h.vs[0] if n == 1 else torch.cat(h.vs, dim=-1)
                delta, h.gs, h.vs, h.delta = h.delta, [], [], None
                dq = torch.empty_like(q) if ctx.needs_input_grad[0] else None
                dk = torch.empty_like(k) if ctx.needs_input_grad[1] else None
                _call("pcfa_attn_stream_dqk", _ptr(q), _ptr(k), _ptr(h.lse()), _ptr(gcat), _ptr(vcat), _ptr(delta),
                      _ptr(dq), _ptr(dk), h.BH, h.N, h.d, n, h.scale)
        return dq, dk, dv, None


def streamed_attn_times_value(handle, v):
    """softmax(scale q k^T) v for the handle's q, k and v [.., N, 128].  Under no_grad, or when nothing requires a
    gradient, the same forward kernels run and nothing is saved."""
    _dev(v)
    if v.shape != handle.q.shape:
        raise ValueError("streamed_attn_times_value: v %s does not match q %s" % (tuple(v.shape), tuple(handle.q.shape)))
    if not (torch.is_grad_enabled() and (handle.q.requires_grad or handle.k.requires_grad or v.requires_grad)):
        return _stream_fwd(handle, handle.q.detach(), handle.k.detach(), v.detach().contiguous())
    return _StreamedAttnTimesValue.apply(handle.q, handle.k, v, handle)
