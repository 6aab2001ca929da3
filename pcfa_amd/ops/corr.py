"""RAFT / GMA all-pairs correlation pyramid and window lookup (models/raft/corr.py:12-60 == models/gma/corr.py:15-63),
also fused with convc1 + ReLU (update.py:79-93); and the same lookup computed on demand from the pooled features
(OnDemandCorrBlock, models/raft/corr.py:63-91)."""
import ctypes
import os

import torch

from .. import _hip
from . import core
from .conv import FEWIN_SHAPES, _conv3x3_cat_fill, _conv3x3_packed, _conv3x3_run, conv_fewin
from .core import _call, _dev, _note_work, _pair, _ptr, _ptr_off, _stream, cached_pack


# --------------------------------------------------------------------------- #
# RAFT / GMA correlation pyramid
# --------------------------------------------------------------------------- #
class _CorrState:
    """Device buffers shared by the build node and its lookup nodes."""
    __slots__ = ("B", "D", "H", "W", "L", "r", "slab", "pyr", "f2ext", "dpyr", "token_grad", "coords_bwd", "bwd_windows", "mfma")


class _CorrBuild(torch.autograd.Function):
    """fmap1, fmap2 -> 1-element token; the pyramid itself lives in `state`.

    The token only carries the autograd dependency: every lookup consumes it, so
    this node's backward runs after ALL lookup backwards have accumulated into
    state.dpyr, and performs the two GEMMs of the volume's backward once.
    """

    @staticmethod
    def forward(ctx, fmap1, fmap2, state):
        lib = _hip.load()
        B, D, H, W = fmap1.shape
        f1 = fmap1.contiguous()
        f2 = fmap2.contiguous()
        slab = state.slab
        state.f2ext = torch.empty((B, D, slab), device=f1.device, dtype=torch.float32)
        state.pyr = torch.empty((B * H * W, slab), device=f1.device, dtype=torch.float32)
        _call("pcfa_corr_f2ext_fwd", _ptr(f2), _ptr(state.f2ext), B, D, H, W, state.L)
        _call("pcfa_corr_pyramid_fwd" if state.mfma == "f32" else "pcfa_corr_pyramid_fwd_bf16x3", _ptr(f1),
              _ptr(state.f2ext), _ptr(state.pyr), B, D, H, W, state.L)
        ctx.state = state
        ctx.save_for_backward(f1)
        return torch.zeros(1, device=f1.device, dtype=torch.float32)

    @staticmethod
    def backward(ctx, grad_token):
        st = ctx.state
        (f1,) = ctx.saved_tensors
        if st.dpyr is None:  # no lookup contributed a gradient
            z = torch.zeros_like(f1)
            st.token_grad = None
            return z, z.clone(), None
        lib = _hip.load()
        B, D, H, W = st.B, st.D, st.H, st.W
        df1 = torch.empty_like(f1)
        df2 = torch.empty_like(f1)
        # the coordinates of every lookup that accumulated into dpyr: the products skip what no window touched
        # (the segment tables of csrc/corr_pyramid.hip are built for up to four levels: more levels -> dense products)
        cs = st.coords_bwd if (st.coords_bwd and len(st.coords_bwd) <= 32 and st.bwd_windows and st.L <= 4) else []
        if cs:
            nbytes = lib.pcfa_corr_pyramid_bwd_windows_workspace_bytes(B, D, H, W, st.L)
            ws = torch.empty((nbytes + 3) // 4, device=f1.device, dtype=torch.float32)
            ptrs = (ctypes.c_void_p * len(cs))(*[c.data_ptr() for c in cs])
            _call("pcfa_corr_pyramid_bwd_windows", _ptr(st.dpyr), _ptr(f1), _ptr(st.f2ext), _ptr(df1), _ptr(df2), _ptr(ws),
                  ctypes.c_size_t(nbytes), ptrs, len(cs), st.r, B, D, H, W, st.L)
            if core.work_recorder() is not None:
                # executed matrix work of the two sparse products: the K segments the kernels walked, read back from the
                # workspace (pcfa_corr_pyramid_bwd_windows_tables: per block {count, widening, hull, (begin, end) x capacity}
                # ints behind the split-K area; segA = blocks of dfmap1's queries, segB = blocks of df2ext's slab columns)
                seg, nbA, _ = window_segment_tables(ws, B, D, H, W, st.L)
                live = torch.arange((seg.shape[1] - 4) // 2)[None, :] < seg[:, :1]
                k = ((seg[:, 5::2] - seg[:, 4::2]) * live).sum(1)
                dense = 2.0 * B * D * (H * W) ** 2
                _note_work("corr_pyramid_gemm_dfmap1", dense, 2.0 * D * 128 * float(k[:B * nbA].sum()))
                _note_work("corr_pyramid_gemm_df2ext", dense, 2.0 * D * 128 * float(k[B * nbA:].sum()))
        else:   # the dense products under their own entry point (and their own launch indices in DispatchTimer's plan)
            nbytes = lib.pcfa_corr_pyramid_bwd_workspace_bytes(B, D, H, W, st.L)
            ws = torch.empty((nbytes + 3) // 4, device=f1.device, dtype=torch.float32)
            _call("pcfa_corr_pyramid_bwd", _ptr(st.dpyr), _ptr(f1), _ptr(st.f2ext), _ptr(df1), _ptr(df2), _ptr(ws),
                  ctypes.c_size_t(nbytes), B, D, H, W, st.L)
        st.dpyr = None
        st.token_grad = None
        st.coords_bwd = None
        return df1, df2, None


def window_segment_tables(ws, B, D, H, W, L):
    """The K-segment records pcfa_corr_pyramid_bwd_windows left in its workspace `ws`, on the host: (int64 records
    [B * (nbA + nbB)][ints per record], table A first, then table B; nbA; pcfa_corr_pyramid_bwd_windows_tables's row)."""
    lib = _hip.load()
    info = (ctypes.c_int * 8)()
    if lib.pcfa_corr_pyramid_bwd_windows_tables(H, W, L, info) != 0:
        raise ValueError("no pyramid layout for %dx%d, %d levels" % (H, W, L))
    rec, nbA, nbB = info[0], info[1], info[2]
    base = (int(lib.pcfa_corr_pyramid_bwd_workspace_bytes(B, D, H, W, L)) + 15) & ~15
    seg = ws.view(torch.int32)[base // 4: base // 4 + rec * B * (nbA + nbB)].cpu().view(-1, rec).long()
    return seg, nbA, list(info)


def _token_grad(st, device):
    """The 1-element token only orders the build node behind every lookup node: ONE lookup per backward pass hands it a
    (zero) gradient, the others return None -- twelve zeros(1) fills and eleven 1-element accumulations per closure
    otherwise (each a kernel launch)."""
    if st.token_grad is None:
        st.token_grad = torch.zeros(1, device=device, dtype=torch.float32)
        return st.token_grad
    return None


class _CorrLookup(torch.autograd.Function):
    @staticmethod
    def forward(ctx, token, coords, state):
        if coords.requires_grad and torch.is_grad_enabled():
            # models/raft/corr.py's bilinear_sampler differentiates w.r.t. coords; RAFT / GMA detach them
            # (raft.py:122-123) and this operator does not implement that gradient: refuse instead of returning zeros
            raise RuntimeError("CorrBlock lookup: coords.requires_grad is not supported (detach the coordinates, as "
                               "models/raft/raft.py:122-123 does)")
        lib = _hip.load()
        st = state
        c = coords.contiguous()
        n1 = 2 * st.r + 1
        out = torch.empty((st.B, st.L * n1 * n1, st.H, st.W), device=c.device, dtype=torch.float32)
        _call("pcfa_corr_lookup_fwd", _ptr(st.pyr), _ptr(c), _ptr(out), st.B, st.H, st.W, st.L, st.r)
        ctx.state = st
        ctx.save_for_backward(c)
        return out

    @staticmethod
    def backward(ctx, grad_out):
        st = ctx.state
        (c,) = ctx.saved_tensors
        lib = _hip.load()
        if st.dpyr is None:
            st.dpyr = torch.zeros_like(st.pyr)
            st.coords_bwd = []
        st.coords_bwd.append(c)
        g = grad_out.contiguous()
        _call("pcfa_corr_lookup_bwd", _ptr(st.dpyr), _ptr(c), _ptr(g), st.B, st.H, st.W, st.L, st.r)
        return _token_grad(st, g.device), None, None


def _convc1_packed(weight):
    """pcfa_lookup_convc1_pack_weights of a frozen [256, 324, 1, 1] weight (both operand orders), cached per version."""
    def make(w):
        cout = w.shape[0]
        w = w.reshape(cout, -1).contiguous()
        packed = torch.empty(int(_hip.load().pcfa_lookup_convc1_packed_floats(cout)), device=w.device, dtype=torch.float32)
        _call("pcfa_lookup_convc1_pack_weights", _ptr(w), _ptr(packed), cout, w.shape[1])
        return packed
    return cached_pack("convc1", (weight,), make)


class _CorrLookupConv(torch.autograd.Function):
    """relu(convc1(lookup(coords))) in one launch per direction (pcfa_lookup_convc1_fwd / _bwd): the lookup node of
    _CorrLookup with the motion encoder's 1x1 convolution (frozen weight) folded in.  Backward accumulates into the
    shared state.dpyr exactly like _CorrLookup."""

    @staticmethod
    def forward(ctx, token, coords, state, weight, bias, relu):
        if coords.requires_grad and torch.is_grad_enabled():
            raise RuntimeError("CorrBlock lookup: coords.requires_grad is not supported (detach the coordinates, as "
                               "models/raft/raft.py:122-123 does)")
        st = state
        c = coords.contiguous()
        packed = _convc1_packed(weight)
        out = torch.empty((st.B, weight.shape[0], st.H, st.W), device=c.device, dtype=torch.float32)
        _call("pcfa_lookup_convc1_fwd", _ptr(st.pyr), _ptr(c), _ptr(packed), _ptr(bias), _ptr(out), st.B, st.H, st.W,
              st.L, st.r, weight.shape[0], int(relu))
        ctx.state, ctx.packed, ctx.relu, ctx.cout = st, packed, int(relu), weight.shape[0]
        ctx.save_for_backward(c, out)
        return out

    @staticmethod
    def backward(ctx, grad_out):
        if ctx.needs_input_grad[3] or ctx.needs_input_grad[4]:
            raise RuntimeError("lookup_conv is the frozen-weight path: no weight / bias gradient")
        st = ctx.state
        c, out = ctx.saved_tensors
        if st.dpyr is None:
            st.dpyr = torch.zeros_like(st.pyr)
            st.coords_bwd = []
        st.coords_bwd.append(c)
        g = grad_out.contiguous()
        _call("pcfa_lookup_convc1_bwd", _ptr(st.dpyr), _ptr(c), _ptr(ctx.packed), _ptr(out), _ptr(g), st.B, st.H, st.W,
              st.L, st.r, ctx.cout, ctx.relu)
        return _token_grad(st, g.device), None, None, None, None, None


# --------------------------------------------------------------------------- #
# RAFT motion encoder with ONE backward for all refinement iterations (Config.motion_bwd = "batched")
# --------------------------------------------------------------------------- #
class _MotionState:
    """Slabs [iters, C, H, W] and bookkeeping shared by the flush node and its step nodes."""
    __slots__ = ("iters", "H", "W", "corr", "w", "cor1", "cf", "rest", "d_rest", "coords", "arrived", "token_grad", "packs")


def _slab_image(slab, i):
    """Image i of a slab [n, C, H, W] as a tensor of its own on the same storage -- NOT a view: autograd tracks in-place
    writes per base tensor, and a later iteration's forward writing ITS image would otherwise invalidate the images that
    earlier nodes saved for their backward."""
    n = slab[0].numel()
    return torch.empty(0, device=slab.device, dtype=slab.dtype).set_(
        slab.untyped_storage(), slab.storage_offset() + i * n, (1,) + tuple(slab.shape[1:]))


class _MotionFlush(torch.autograd.Function):
    """corr token -> alias of it that every step node consumes, so this node's backward runs after ALL of them and before
    _CorrBuild's (the idiom of _CorrBuild / gru._Fanout).  The coordinates and the flow are detached every iteration
    (models/raft/raft.py:122-123), so the motion encoder's backward feeds nothing but the pyramid gradient, which is
    consumed once, after the last iteration's backward: the two 3x3 data gradients (conv, convc2) of all iterations run here
    as one launch each over the slabs (pcfa_conv3x3_run_strided, batch = iters) instead of one small-grid launch per
    iteration, followed by the per-iteration pcfa_lookup_convc1_bwd launches in the order autograd ran them in (last
    iteration first): every sum is formed as before, bit for bit."""

    @staticmethod
    def forward(ctx, token, ms):
        ctx.ms = ms
        return token.view_as(token)

    @staticmethod
    def backward(ctx, grad_token):
        ms = ctx.ms
        st = ms.corr
        live = [i for i in range(ms.iters) if ms.arrived[i]]
        ms.arrived = [False] * ms.iters
        ms.token_grad = None
        if not live:
            return None, None
        H, W, plane = ms.H, ms.W, ms.H * ms.W
        (bwd_c, k_c, n_c), (bwd_c2, k_c2, n_c2) = ms.packs   # conv: cf (k_c) -> n_c ; convc2: cor1 (k_c2) -> n_c2 (< k_c)
        dev = ms.rest.device
        wr = ms.rest.shape[1]
        lib = _hip.load()
        n = ms.iters
        # one launch for all iterations only where it forms every sum as the per-iteration launches do: the direct
        # F(2x2,3x3) kernel both for the batch and for the single-image shapes those launches have (small maps run K slices
        # or F(4x4,3x3) at batch 1: another order of summation) -- pcfa_conv3x3_run_strided refuses the same cases
        direct = lambda b, k, n_: (lib.pcfa_conv3x3_algo(b, k, n_, H, W) == 23   # noqa: E731
                                   and lib.pcfa_conv3x3_workspace_bytes(b, k, n_, H, W) == 0)
        batched = (len(live) == n and all(direct(b, k, n_) for b in (1, n)
                                          for k, n_ in ((n_c, k_c), (n_c, n_c2), (n_c2, k_c2))))
        d_cor1 = torch.empty((n, k_c2, H, W), device=dev, dtype=torch.float32)
        if batched:
            # d cf: only the n_c2 channels convc2 produced are live (the convf2 channels feed the detached flow's branch)
            d_cf = torch.empty((n, n_c2, H, W), device=dev, dtype=torch.float32)
            _call("pcfa_conv3x3_run_strided", _ptr(ms.d_rest), wr * plane, _ptr(bwd_c), None, _ptr(ms.cf), k_c * plane, None, 0,
                  _ptr(d_cf), n_c2 * plane, n, n_c, n_c2, H, W, 0, 0., 0, None, ctypes.c_size_t(0))
            _call("pcfa_conv3x3_run_strided", _ptr(d_cf), n_c2 * plane, _ptr(bwd_c2), None, _ptr(ms.cor1), k_c2 * plane, None, 0,
                  _ptr(d_cor1), k_c2 * plane, n, n_c2, k_c2, H, W, 0, 0., 0, None, ctypes.c_size_t(0))
        if st.dpyr is None:
            st.dpyr = torch.zeros_like(st.pyr)
            st.coords_bwd = []
        packed = _convc1_packed(ms.w["convc1"][0])
        for i in reversed(live):
            if not batched:   # the per-iteration launches of conv3x3_cat's backward
                d_cf = torch.empty((1, k_c, H, W), device=dev, dtype=torch.float32)
                _conv3x3_run(dev, _ptr_off(ms.d_rest, i * wr * plane), bwd_c, None, _ptr_off(ms.cf, i * k_c * plane), None,
                             _ptr(d_cf), 1, n_c, k_c, H, W)
                _conv3x3_run(dev, _ptr(d_cf), bwd_c2, None, _ptr_off(ms.cor1, i * k_c2 * plane), None,
                             _ptr_off(d_cor1, i * k_c2 * plane), 1, n_c2, k_c2, H, W)
            st.coords_bwd.append(ms.coords[i])
            _call("pcfa_lookup_convc1_bwd", _ptr(st.dpyr), _ptr(ms.coords[i]), _ptr(packed), _ptr_off(ms.cor1, i * k_c2 * plane),
                  _ptr_off(d_cor1, i * k_c2 * plane), st.B, st.H, st.W, st.L, st.r, k_c2, 1)
        return grad_token, None


class _MotionStep(torch.autograd.Function):
    """Iteration i of the motion encoder (models/raft/update.py:79-101) as one node: token, coords, flow -> motion features,
    written into slab i by the launches the layer-by-layer path issues (fused lookup + convc1, convf1, convc2 | convf2 as a
    pair, conv, the flow tail).  Its backward launches nothing: it notes that the gradient of slab i has arrived (_GruStep
    writes it in place: gru_step(d_rest_dst=...)) and leaves the work to _MotionFlush."""

    @staticmethod
    def forward(ctx, token, coords, flow, ms, i):
        st = ms.corr
        c = coords.contiguous()
        (wc1, bc1), (wc2, bc2), (wf1, bf1), (wf2, bf2), (wc, bc) = (ms.w[k] for k in ("convc1", "convc2", "convf1", "convf2", "conv"))
        cor1, cf, rest = _slab_image(ms.cor1, i), _slab_image(ms.cf, i), _slab_image(ms.rest, i)
        _call("pcfa_lookup_convc1_fwd", _ptr(st.pyr), _ptr(c), _ptr(_convc1_packed(wc1)), _ptr(bc1), _ptr(cor1), st.B, st.H,
              st.W, st.L, st.r, wc1.shape[0], 1)
        flo1 = conv_fewin(flow, wf1, bf1, True)
        _conv3x3_cat_fill([cor1, flo1.contiguous()], [wc2, wf2], [bc2, bf2], (), cf)
        _conv3x3_cat_fill([cf], [wc], [bc], (flow,), rest)
        ms.coords[i] = c
        ctx.ms, ctx.i = ms, i
        ctx.set_materialize_grads(False)
        return rest

    @staticmethod
    def backward(ctx, g):
        ms, i = ctx.ms, ctx.i
        if g is None:
            return None, None, None, None, None
        dst = _slab_image(ms.d_rest, i)
        if g.data_ptr() != dst.data_ptr() or not g.is_contiguous():   # (the gradient arrived somewhere else)
            dst.copy_(g)
        ms.arrived[i] = True
        tg = None
        if ms.token_grad is None:   # one (zero) gradient per backward pass orders the flush node behind every step node
            tg = ms.token_grad = torch.zeros(1, device=g.device, dtype=torch.float32)
        return tg, None, None, None, None


class MotionSteps:
    """The motion encoder of `iters` refinement iterations with a batched backward; see motion_steps()."""

    def __init__(self, ms, token):
        self._ms, self._token = ms, token

    def step(self, i, coords, flow):
        """relu-deferred motion features [1, C, H, W] of iteration i (a slice of the slab)."""
        _dev(coords, flow)
        if coords.requires_grad and torch.is_grad_enabled():
            raise RuntimeError("motion_steps: coords.requires_grad is not supported (detach the coordinates, as "
                               "models/raft/raft.py:122-123 does)")
        if flow.requires_grad and torch.is_grad_enabled():
            raise RuntimeError("motion_steps: the flow must be detached (models/raft/raft.py:122-123)")
        return _MotionStep.apply(self._token, coords, flow, self._ms, i)

    def d_rest_dst(self, i):
        """Where iteration i's consumer (gru_step) writes the gradient of step(i)'s result."""
        return _slab_image(self._ms.d_rest, i)


def motion_steps(corr_block, iters, convc1, convc2, convf1, convf2, conv):
    """RAFT's motion encoder for `iters` iterations on one image, each layer given as (frozen weight, bias), with its
    backward deferred and batched (_MotionFlush).  Contract: every step's ONLY consumer is gru_step(rest_relu_channels = conv's
    output channels), as with conv3x3_cat(grad_premasked=True, mask_input_grads=True).  Returns None where the fused
    lookup or the slab layout does not apply (the caller then runs the layers one by one)."""
    if not isinstance(corr_block, CorrBlock) or iters < 1:
        return None
    st = corr_block._state
    (wc1, bc1), (wc2, bc2), (wf1, bf1), (wf2, bf2), (wc, bc) = convc1, convc2, convf1, convf2, conv
    if (st.B != 1 or st.L != 4 or st.r != 4 or bc1 is None or tuple(wc1.shape) != (256, 324, 1, 1)
            or not corr_block._token.requires_grad
            or any(t is None or t.requires_grad for t in (wc1, bc1, wc2, bc2, wf1, bf1, wf2, bf2, wc, bc))
            or any(tuple(w.shape[2:]) != (3, 3) for w in (wc2, wf2, wc))
            or (wf1.shape[1], wf1.shape[2]) not in FEWIN_SHAPES or wf1.shape[2] != wf1.shape[3]
            or wc2.shape[1] != wc1.shape[0] or wf2.shape[1] != wf1.shape[0] or wc.shape[1] != wc2.shape[0] + wf2.shape[0]):
        return None
    dev = st.pyr.device
    ms = _MotionState()
    ms.iters, ms.H, ms.W, ms.corr = iters, st.H, st.W, st
    ms.w = {"convc1": convc1, "convc2": convc2, "convf1": convf1, "convf2": convf2, "conv": conv}
    new = lambda c: torch.empty((iters, c, st.H, st.W), device=dev, dtype=torch.float32)  # noqa: E731
    ms.cor1, ms.cf = new(wc1.shape[0]), new(wc.shape[1])
    ms.rest, ms.d_rest = new(wc.shape[0] + 2), new(wc.shape[0] + 2)
    ms.coords, ms.arrived, ms.token_grad = [None] * iters, [False] * iters, None
    # (data-gradient packing, input channels of the gradient, output channels): conv, then convc2
    ms.packs = ((_conv3x3_packed(wc)[1], wc.shape[1], wc.shape[0]), (_conv3x3_packed(wc2)[1], wc2.shape[1], wc2.shape[0]))
    return MotionSteps(ms, _MotionFlush.apply(corr_block._token, ms))


class CorrBlock:
    """Drop-in for models/raft/corr.py:12-50 -- same constructor and __call__."""

    def __init__(self, fmap1, fmap2, num_levels=4, radius=4, bwd_windows=True, mfma="f32"):
        """bwd_windows (Config.pyramid_bwd_windows): the backward products skip what no lookup window touched; False =
        the dense products (A/B, parity tests).  mfma (Config.mfma): "f32" | "bf16x3", the arithmetic of the pyramid's
        FORWARD product (pcfa_corr_pyramid_fwd_bf16x3); the backward products stay on the fp32 matrix cores."""
        _dev(fmap1, fmap2)
        if mfma not in ("f32", "bf16x3"):
            raise ValueError("CorrBlock: mfma must be 'f32' or 'bf16x3', got %r" % (mfma,))
        if fmap1.shape != fmap2.shape or fmap1.dim() != 4:
            raise ValueError("CorrBlock expects two [B,D,H,W] feature maps of equal shape")
        lib = _hip.load()
        self.num_levels = num_levels
        self.radius = radius
        st = _CorrState()
        st.B, st.D, st.H, st.W = fmap1.shape
        st.L, st.r = num_levels, radius
        st.slab = lib.pcfa_corr_slab_floats(st.H, st.W, num_levels)
        if st.slab <= 0 or (st.H >> (num_levels - 1)) < 1 or (st.W >> (num_levels - 1)) < 1:
            raise ValueError("feature map %dx%d too small for %d pyramid levels" % (st.H, st.W, num_levels))
        st.dpyr = None
        st.token_grad = None
        st.coords_bwd = None
        st.bwd_windows = bool(bwd_windows)
        st.mfma = mfma
        self._state = st
        self._token = _CorrBuild.apply(fmap1, fmap2, st)

    def __call__(self, coords):
        _dev(coords)
        return _CorrLookup.apply(self._token, coords, self._state)

    def lookup_conv_relu(self, coords, weight, bias, relu=True):
        """relu(conv1x1(self(coords), weight, bias)) without materialising the lookup (update.py:79-93 convc1);
        None when the shape is not the fused kernel's (4 levels, radius 4, 256 x 324 weight, bias present)."""
        if (self.num_levels != 4 or self.radius != 4 or bias is None or weight.dim() != 4
                or tuple(weight.shape) != (256, 324, 1, 1) or weight.requires_grad or bias.requires_grad):
            return None
        _dev(coords, weight, bias)
        return _CorrLookupConv.apply(self._token, coords, self._state, weight, bias, relu)

    @property
    def corr_pyramid(self):
        """Per-level tensors [B*Q,1,H_l,W_l] gathered out of the tiled slab matrix (for inspection/tests)."""
        st = self._state
        return [st.pyr[:, idx.to(st.pyr.device)].reshape(-1, 1, h, w)
                for (idx, h, w) in tiled_index_maps(st.H, st.W, st.L)]


# --------------------------------------------------------------------------- #
# RAFT / GMA correlation on demand (Config.corr = "on_demand")
# --------------------------------------------------------------------------- #
class _OnDemandState:
    """The build's workspace (include/pcfa_hip.h pcfa_corr_ondemand_*): features, pooled fmap2 pyramid, accumulators."""
    __slots__ = ("B", "D", "H", "W", "L", "r", "ws", "token_grad", "accumulating", "suffix")


class _OnDemandBuild(torch.autograd.Function):
    """fmap1, fmap2 -> 1-element token, as _CorrBuild: every lookup consumes the token, so this node's backward runs after
    ALL lookup backwards have accumulated into the workspace and converts the sums once (pcfa_corr_ondemand_finish)."""

    @staticmethod
    def forward(ctx, fmap1, fmap2, state):
        lib = _hip.load()
        st = state
        f1 = fmap1.contiguous()
        f2 = fmap2.contiguous()
        nbytes = int(lib.pcfa_corr_ondemand_workspace_bytes(st.B, st.D, st.H, st.W, st.L))
        st.ws = torch.empty(nbytes, device=f1.device, dtype=torch.uint8)
        _call("pcfa_corr_ondemand_prepare", _ptr(f1), _ptr(f2), _ptr(st.ws), st.B, st.D, st.H, st.W, st.L)
        ctx.state = st
        ctx.shape = f1.shape
        return torch.zeros(1, device=f1.device, dtype=torch.float32)

    @staticmethod
    def backward(ctx, grad_token):
        st = ctx.state
        if not st.accumulating:   # no lookup contributed a gradient
            z = torch.zeros(ctx.shape, device=st.ws.device, dtype=torch.float32)
            st.token_grad = None
            return z, z.clone(), None
        df1 = torch.empty(ctx.shape, device=st.ws.device, dtype=torch.float32)
        df2 = torch.empty_like(df1)
        _call("pcfa_corr_ondemand_finish", _ptr(st.ws), _ptr(df1), _ptr(df2), st.B, st.D, st.H, st.W, st.L)
        st.accumulating = False
        st.token_grad = None
        return df1, df2, None


class _OnDemandLookup(torch.autograd.Function):
    @staticmethod
    def forward(ctx, token, coords, state):
        st = state
        c = coords.contiguous()
        n1 = 2 * st.r + 1
        out = torch.empty((st.B, st.L * n1 * n1, st.H, st.W), device=c.device, dtype=torch.float32)
        _call("pcfa_corr_ondemand_fwd" + st.suffix, _ptr(st.ws), _ptr(c), _ptr(out), st.B, st.D, st.H, st.W, st.L, st.r)
        ctx.state = st
        ctx.save_for_backward(c)
        return out

    @staticmethod
    def backward(ctx, grad_out):
        st = ctx.state
        (c,) = ctx.saved_tensors
        g = grad_out.contiguous()
        _call("pcfa_corr_ondemand_bwd" + st.suffix, _ptr(st.ws), _ptr(c), _ptr(g), int(st.accumulating), st.B, st.D, st.H, st.W,
              st.L, st.r)
        st.accumulating = True
        return _token_grad(st, g.device), None, None


class OnDemandCorrBlock:
    """CorrBlock's constructor and __call__ without the all-pairs pyramid: every lookup computes its (2r+2)^2 window dot
    products against the pooled fmap2 (the reference's AlternateCorrBlock, models/raft/corr.py:63-91).  Memory O(Q*D)
    per build instead of O(Q^2); same values up to fp32 rounding; deterministic backward.

    lookup (Config.ondemand_lookup): "per_query" | "tiled" (pcfa_corr_ondemand_fwd_tiled / _bwd_tiled: query tiles with a
    small common box on the matrix cores, the rest on the per-query kernels)."""

    def __init__(self, fmap1, fmap2, num_levels=4, radius=4, lookup="per_query"):
        _dev(fmap1, fmap2)
        if lookup not in ("per_query", "tiled"):
            raise ValueError("OnDemandCorrBlock: lookup must be 'per_query' or 'tiled', got %r" % (lookup,))
        if fmap1.shape != fmap2.shape or fmap1.dim() != 4:
            raise ValueError("OnDemandCorrBlock expects two [B,D,H,W] feature maps of equal shape")
        lib = _hip.load()
        self.num_levels = num_levels
        self.radius = radius
        st = _OnDemandState()
        st.B, st.D, st.H, st.W = fmap1.shape
        st.L, st.r = num_levels, radius
        if (st.H >> (num_levels - 1)) < 1 or (st.W >> (num_levels - 1)) < 1:
            raise ValueError("feature map %dx%d too small for %d pyramid levels" % (st.H, st.W, num_levels))
        if lib.pcfa_corr_ondemand_workspace_bytes(st.B, st.D, st.H, st.W, num_levels) == 0 or not 1 <= radius <= 4:
            raise ValueError("OnDemandCorrBlock: D=%d, %d levels, radius %d not served (D %% 4 == 0, D <= 512, radius 1..4)"
                             % (st.D, num_levels, radius))
        st.token_grad = None
        st.accumulating = False
        st.suffix = "_tiled" if lookup == "tiled" else ""
        self._state = st
        self._token = _OnDemandBuild.apply(fmap1, fmap2, st)

    def __call__(self, coords):
        _dev(coords)
        if coords.requires_grad and torch.is_grad_enabled():
            # checked here: inside Function.forward grad mode is off.  RAFT / GMA detach the coordinates
            # (models/raft/raft.py:122-123); this operator has no gradient w.r.t. them
            raise RuntimeError("OnDemandCorrBlock lookup: coords.requires_grad is not supported (detach the coordinates, "
                               "as models/raft/raft.py:122-123 does)")
        return _OnDemandLookup.apply(self._token, coords, self._state)

    def lookup_conv_relu(self, coords, weight, bias, relu=True):
        """No fused on-demand lookup -> convc1 kernel: the caller materialises the lookup."""
        return None


def tiled_index_maps(H, W, num_levels):
    """[(index tensor [H_l*W_l] into a query slab, H_l, W_l)] -- the 4x4-tile layout of include/pcfa_hip.h."""
    out, off, h, w = [], 0, H, W
    for _ in range(num_levels):
        tw = (w + 3) // 4
        ys, xs = torch.meshgrid(torch.arange(h), torch.arange(w), indexing="ij")
        idx = off + ((ys // 4) * tw + xs // 4) * 16 + (ys % 4) * 4 + xs % 4
        out.append((idx.reshape(-1), h, w))
        off += ((h + 3) // 4) * tw * 16
        h, w = h // 2, w // 2
    return out
