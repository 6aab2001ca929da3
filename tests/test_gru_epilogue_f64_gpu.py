"""The four fused SepConvGRU epilogues -- pcfa_sepconv5_gru_gates_fwd / _update_fwd / _gates_bwd / _update_bwd (GruEpi modes
1-4) of the direct implicit GEMM (csrc/sepconv5.hip: predicated, branch-free, branch-free with split-K) and of the 1-D
Winograd F(2,5) (csrc/sepconv5_wino.hip: 64 channels x 2 K-groups, 32 x 4), 1x5 and 5x1 -- through the C-ABI on fenced
buffers, against the float64 statement of tests/gru_epilogue.py on every (entry point, path, orientation).

Each call checks: status 0 and the path label against pcfa_sepconv5_uses_winograd; every fence intact and every input
bit-unchanged; every output element written and finite (outputs hold a sentinel NaN before the first call, -7 before the
second) and the two calls equal bit for bit; the elementwise gate |got - want| <= bound and the statistical gate
rel_l2 <= 3 max(rel_l2(emu), u) of tests/gates.py per output, over its groups plus the columns of the ragged last
64-pixel tile and the saturated elements (addends of +-30, +-100, where the sigmoid must be exactly 1 / 0 and tanh +-1);
for gates_bwd: dh_in a separate buffer, dh_in == dh (the aliasing of pcfa_amd/ops/gru.py: same bits) and NULL, and
accumulate_rest 0 and 1.  The ratios, the worst group and the path are recorded as junit properties.

Fused against un-fused.  Each fused call is compared with the composition it replaces, on the same path setting, and the
number of differing elements is recorded per output.  FUSED_EQUALS_UNFUSED lists the outputs that agree bit for bit on
every case and are asserted equal: z, r, rh, q, dzr, mode 4's dh and both d_rest.  Both sides run the same convolution
kernel to the same accumulators; the activations are calls (expf, the divide, tanhf), products of products and a single
subtraction from 1 leave the compiler nothing to contract.  Four outputs differ, in up to 36 % of their elements
(measured maxima: hnew 590308, mode 3's dh 353507, dz 559458, dqc 498183 elements; dz / dqc agree in the 1x5 Winograd
kernels and differ in all others):
each holds a product that feeds an addition -- hnew = (1 - z) h + z q, dh = drh r + dh_in, dz = g q - g h, dqc's
1 - q q -- and -ffp-contract=fast (hipcc's default) lets the compiler fuse it into an fma per kernel as it sees fit.
gru_math.hip's update-backward kernel is compiled to v_pk_fma_f32 / v_fmamk_f32 for g q - g h and 1 - q q, its
gates-backward kernel to a separate multiply and add (no fma at all: the `+ dh_in` sits in a later block), and the
epilogues, written on scalars inside a 16-row unrolled loop with `c += e4`, are contracted the other way round.  Either
is a correct rounding of the expression (the bound counts every product and addition once), so for these four the
un-fused result must pass the same two float64 gates, and no tolerance between the two results is introduced.

Measured on an MI355X (no kernel changed; c_sigmoid / c_tanh measured 2.43 / 2.36, chosen 5 / 5), the worst ratios over
the cases of a path and the largest number of elements in which fused and un-fused differ:
  entry      path          elementwise (output)   statistical (output, group)   fused != un-fused
  gates_fwd  wino_wide     0.00148 (z)  0.364 (rh last_tile)  0
  gates_fwd  wino_narrow   0.00174 (r)  0.321 (z col0)  0
  gates_fwd  direct_split2 0.00339 (z)  0.322 (z colN)  0
  gates_fwd  direct_fast   0.00282 (z)  0.375 (rh colN)  0
  gates_fwd  direct_slow   0.00767 (z)  0.353 (rh colN)  0
  update_fwd wino_wide     0.00327 (hnew)  0.357 (hnew last_tile)  hnew 590308
  update_fwd wino_narrow   0.00648 (hnew)  0.326 (hnew colN)  hnew 295692
  update_fwd direct_split2 0.0103 (hnew)  0.358 (q last_tile)  hnew 228699
  update_fwd direct_fast   0.0069 (hnew)  0.364 (q last_tile)  hnew 459425
  update_fwd direct_slow   0.0225 (hnew)  0.348 (q row0)  hnew 54717
  gates_bwd  wino_wide     0.959 (dzr)  0.328 (dzr colN)  dh 159833
  gates_bwd  wino_narrow   0.956 (dzr)  0.326 (d_rest_acc last_tile)  dh 353507
  gates_bwd  direct_split2 0.955 (dzr)  0.27 (dh last_tile)  dh 168772
  gates_bwd  direct_fast   0.964 (dzr)  0.367 (d_rest_acc col0)  dh 353253
  gates_bwd  direct_slow   0.879 (dzr)  0.377 (d_rest row0)  dh 1227
  update_bwd wino_wide     0.265 (dz)  0.338 (d_rest last_tile)  dz 279452, dqc 249469
  update_bwd wino_narrow   0.243 (dz)  0.346 (d_rest last_tile)  dz 559458, dqc 498183
  update_bwd direct_split2 0.245 (dz)  0.299 (dqc colN)  dz 276515, dqc 246821
  update_bwd direct_fast   0.27 (dz)  0.351 (dz last_tile)  dz 559384, dqc 498149
  update_bwd direct_slow   0.172 (dz)  0.358 (dh colN)  dz 2010, dqc 1768
The elementwise ratio near 1 of gates_bwd is dzr[:, :C] = dz (1 - z) z, whose bound is gamma(3) |want| alone: three
roundings in a row do come close to 3 u among a million elements.  A read outside an operand shows only where its value
reaches an output (the NaN fences): a prefetch column clamped to W instead of W - 1 loads one float past a row in lanes
that store nothing, and no test here can see it.
"""
import ctypes
import functools
import os

import pytest
import torch

from pcfa_amd import _hip, hip_ops
from pcfa_amd.ops import gru as gru_mod
from tests import gru_epilogue as ge
from tests import winograd as wg
from tests.fenced import DEV, NAN_BITS, PCFA_ERR_INVALID_ARG, SENTINEL, U, Fenced, stream
from tests.gates import dense_stride as _dense_stride, gates, unchanged as _unchanged

pytestmark = pytest.mark.gpu
torch.set_num_threads(min(16, torch.get_num_threads()))

# outputs whose fused and un-fused bits agree on every case (see the module docstring)
FUSED_EQUALS_UNFUSED = {("gates_fwd", "z"), ("gates_fwd", "r"), ("gates_fwd", "rh"), ("update_fwd", "q"), ("gates_bwd", "dzr"),
                        ("gates_bwd", "d_rest"), ("update_bwd", "dh"), ("update_bwd", "d_rest")}


def _lib():
    return _hip.load()


def _fin(t):
    return Fenced(t.shape, _dense_stride(t.shape), NAN_BITS).write(t)


def _fout(*shape):
    return Fenced(shape, _dense_stride(shape), SENTINEL)


def _at(t, *idx):
    """pointer to element idx of a dense device tensor"""
    return ctypes.c_void_p(t[idx].data_ptr())


def _bits(t):
    return t.contiguous().view(torch.int32)


def _pack(wt, backward):
    """pcfa_sepconv5_pack_weights of the Conv2d weight wt [Cout][Cin][5]; the packing the entry point reads"""
    lib = _lib()
    co, ci = wt.shape[:2]
    fw = _fin(wt)
    fpf = Fenced((int(lib.pcfa_sepconv5_packed_floats(co, ci)),), (1,), NAN_BITS)
    fpb = Fenced((int(lib.pcfa_sepconv5_packed_floats(ci, co)),), (1,), NAN_BITS)
    assert lib.pcfa_sepconv5_pack_weights(fw.ptr(), fpf.ptr(), fpb.ptr(), co, ci, stream()) == 0
    torch.cuda.synchronize()
    assert _unchanged(fw) and fpf.fence_intact() and fpb.fence_intact()
    fp = fpb if backward else fpf
    fp.bits0 = fp.buf.view(torch.int32).clone()
    return fp


# entry -> (input tensors of ge.inputs, {output: channels}, argument list from the pointers p)
SPEC = {
    "gates_fwd": (("h", "rest", "add_zr"), dict(z="C", r="C", rh="C"),
                  lambda p, C, Cr, acc: (p["h"], C, p["rest"], Cr, p["w"], p["add_zr"], p["z"], p["r"], p["rh"])),
    "update_fwd": (("rh", "rest", "add_q", "z", "h"), dict(q="C", hnew="C"),
                   lambda p, C, Cr, acc: (p["rh"], C, p["rest"], Cr, p["w"], p["add_q"], p["z"], p["h"], p["q"], p["hnew"])),
    "gates_bwd": (("dqc", "z", "r", "h", "dz", "dh_in"), dict(dzr="2C", dh="C", d_rest="Cr"),
                  lambda p, C, Cr, acc: (p["dqc"], C, Cr, p["w"], p["z"], p["r"], p["h"], p["dz"], p["dh_in"], p["dzr"],
                                         p["dh"], p["d_rest"], acc)),
    "update_bwd": (("dzr", "dh_acc", "z", "q", "h"), dict(dz="C", dqc="C", dh="C", d_rest="Cr"),
                   lambda p, C, Cr, acc: (p["dzr"], C, Cr, p["w"], p["dh_acc"], p["z"], p["q"], p["h"], p["dz"], p["dqc"],
                                          p["dh"], p["d_rest"])),
}
OPTIONAL = {"dh_in"}


class Launch:
    """The fenced operands of one entry point at one shape and the call on them."""

    def __init__(self, entry, shape, v):
        self.entry, self.shape, self.v = entry, shape, v
        B, C, Cr, H, W = shape
        self.d = d = ge.inputs(B, C, Cr, H, W, v)
        names, outs, self.args = SPEC[entry]
        _, wt, backward = ge.operand(d, entry)
        self.ins = {n: _fin(getattr(d, n)) for n in names}
        self.ins["w"] = _pack(wt, backward)
        ch = {"C": C, "2C": 2 * C, "Cr": Cr}
        self.outs = {n: _fout(B, ch[c], H, W) for n, c in outs.items()}
        self.fn = getattr(_lib(), "pcfa_sepconv5_gru_" + entry)

    def fill(self, first, acc_rest):
        """outputs: the sentinel NaN (first call) or -7; an accumulating d_rest: its previous values"""
        for n, f in self.outs.items():
            if n == "d_rest" and acc_rest:
                f.view().copy_(self.d.prev_rest.to(DEV))
            elif first:
                f.view().view(torch.int32).fill_(SENTINEL)
            else:
                f.view().fill_(-7.0)

    def __call__(self, acc=0, C=None, Cr=None, **ptrs):
        B, C0, Cr0, H, W = self.shape
        p = {n: f.ptr() for n, f in list(self.ins.items()) + list(self.outs.items())}
        p.update(ptrs)
        a = self.args(p, C0 if C is None else C, Cr0 if Cr is None else Cr, acc)
        return self.fn(*a, B, H, W, self.v, stream())

    def collect(self):
        """the outputs after a call: fences, inputs, finiteness checked"""
        torch.cuda.synchronize()
        for n, f in self.outs.items():
            assert f.fence_intact(), "a store landed outside " + n
        for n, f in self.ins.items():
            assert _unchanged(f), "input %s was written" % n
        got = {n: f.view().clone() for n, f in self.outs.items()}
        for n, t in got.items():
            assert bool(torch.isfinite(t).all()), "%s: an element was not written, or a NaN was read from a fence" % n
        return got


def unfused(L, acc_rest):
    """The composition the fused call replaces (pcfa_amd/ops/gru.py's other branch), on plain device tensors."""
    lib = _lib()
    B, C, Cr, H, W = L.shape
    v, plane, n = L.v, H * W, C * H * W
    t = {k: f.view() for k, f in L.ins.items()}
    new = lambda c: torch.full((B, c, H, W), float("nan"), device=DEV)  # noqa: E731
    w = L.ins["w"].ptr()
    P = lambda x: ctypes.c_void_p(x.data_ptr())  # noqa: E731
    if L.entry == "gates_fwd":
        zr, z, r, rh = new(2 * C), new(C), new(C), new(C)
        assert lib.pcfa_sepconv5_fwd(P(t["h"]), C, P(t["rest"]), Cr, w, P(zr), B, 2 * C, H, W, v, stream()) == 0
        for b in range(B):
            assert lib.pcfa_gru_gates_fwd(_at(zr, b), _at(zr, b, C), _at(t["h"], b), None, None, _at(t["add_zr"], b),
                                          _at(t["add_zr"], b, C), _at(z, b), _at(r, b), _at(rh, b), n, plane, C, stream()) == 0
        out = dict(z=z, r=r, rh=rh)
    elif L.entry == "update_fwd":
        qc, q, hnew = new(C), new(C), new(C)
        assert lib.pcfa_sepconv5_fwd(P(t["rh"]), C, P(t["rest"]), Cr, w, P(qc), B, C, H, W, v, stream()) == 0
        assert lib.pcfa_gru_update_fwd(P(t["z"]), P(qc), P(t["h"]), None, P(t["add_q"]), P(q), P(hnew), B * n, plane, C,
                                       stream()) == 0
        out = dict(q=q, hnew=hnew)
    elif L.entry == "gates_bwd":
        drh, dzr, dh = new(C), new(2 * C), new(C)
        d_rest = L.d.prev_rest.to(DEV).clone() if acc_rest else new(Cr)
        assert lib.pcfa_sepconv5_fwd_split(P(t["dqc"]), C, None, 0, w, P(drh), C, 0, P(d_rest), acc_rest, B, C + Cr, H, W,
                                           v, stream()) == 0
        for b in range(B):
            assert lib.pcfa_gru_gates_bwd_acc(_at(t["z"], b), _at(t["r"], b), _at(t["h"], b), _at(t["dz"], b), _at(drh, b),
                                              _at(t["dh_in"], b), _at(dzr, b), _at(dzr, b, C), _at(dh, b), n, stream()) == 0
        out = dict(dzr=dzr, dh=dh, d_rest=d_rest)
    else:
        g, dz, dqc, dh = t["dh_acc"].clone(), new(C), new(C), new(C)
        d_rest = L.d.prev_rest.to(DEV).clone()
        assert lib.pcfa_sepconv5_fwd_split(P(t["dzr"]), 2 * C, None, 0, w, P(g), C, 1, P(d_rest), 1, B, C + Cr, H, W, v,
                                           stream()) == 0
        assert lib.pcfa_gru_update_bwd(P(t["z"]), P(t["q"]), P(t["h"]), P(g), P(dz), P(dqc), P(dh), B * n, stream()) == 0
        out = dict(dz=dz, dqc=dqc, dh=dh, d_rest=d_rest)
    torch.cuda.synchronize()
    return out


def check_gates(record, name, got, ref, sat, W, prefix=""):
    want, bound, emu = ref
    extra = {"saturated": sat[name]} if name in sat else None
    return gates(got.cpu(), want, None, 0, emu, 2, record, prefix=prefix + name + "_", bound=bound, regions=ge.groups_of(W),
                 extra=extra)


def sid(s):
    return "x".join(map(str, s))


MATRIX = [(case, v, entry, algo) for case in ge.CASES for v in (0, 1) for entry in ge.ENTRIES
          for algo in ("winograd", "direct")]


@pytest.mark.parametrize("case,v,entry,algo", MATRIX, ids=["%s-v%d-%s-%s" % (sid(c), v, e, a) for c, v, e, a in MATRIX])
def test_fused_epilogue(record_property, sepconv5_algo, case, v, entry, algo):
    lib = _lib()
    shape = ge.run_shape(case, v)
    B, C, Cr, H, W = shape
    Ca, Cb, Cout = ge.op_shape(entry, C, Cr)
    sepconv5_algo(algo)
    wino = bool(lib.pcfa_sepconv5_uses_winograd(B, Ca, Cb, Cout, H, W, v))
    label = ge.path(entry, *shape, v, enabled=algo == "winograd", env=os.environ)
    record_property("path", label)
    assert wino == label.startswith("wino")
    ref, sat = ge.problem(*shape, v, entry, wino, wg.sepconv5_wino_groups(B, Cout, H, W, v) if wino else 0)
    L = Launch(entry, shape, v)
    acc0 = 1 if entry == "update_bwd" else 0      # mode 4 always accumulates into d_rest

    runs = []
    for first in (True, False):
        L.fill(first, acc0)
        assert L(acc=acc0) == 0
        runs.append(L.collect())
    got = runs[0]
    for n in got:
        assert torch.equal(_bits(runs[0][n]), _bits(runs[1][n])), n + ": not repeatable bit for bit"
    for n in got:
        check_gates(record_property, n, got[n], ref[n], sat, W)
    for n in sat:   # the saturated tails, exactly
        if n in ("z", "r", "q"):
            add = L.d.add_q if n == "q" else L.d.add_zr[:, :C] if n == "z" else L.d.add_zr[:, C:]
            hard, value = ge.saturated_exact(add, n != "q")
            assert torch.equal(got[n].cpu()[hard], value[hard]), n + ": a saturated activation is not exactly 0 / 1 / +-1"

    if entry == "gates_bwd":
        # dh_in == dh, accumulate_rest = 1: the wrapper's call.  Same bits as the separate buffer; d_rest accumulated.
        L.fill(True, 1)
        L.outs["dh"].view().copy_(L.d.dh_in.to(DEV))
        assert L(acc=1, dh_in=L.outs["dh"].ptr()) == 0
        alias = L.collect()
        assert torch.equal(_bits(alias["dzr"]), _bits(got["dzr"])) and torch.equal(_bits(alias["dh"]), _bits(got["dh"])), \
            "dh_in == dh differs from dh_in in a buffer of its own"
        check_gates(record_property, "d_rest_acc", alias["d_rest"], ref["d_rest_acc"], sat, W)
        # dh_in = NULL
        L.fill(True, 0)
        assert L(acc=0, dh_in=None) == 0
        null = L.collect()
        assert torch.equal(_bits(null["dzr"]), _bits(got["dzr"])) and torch.equal(_bits(null["d_rest"]), _bits(got["d_rest"]))
        check_gates(record_property, "dh_null", null["dh"], ref["dh_null"], sat, W)

    # fused against the composition it replaces
    un = unfused(L, acc0)
    for n in got:
        diff = int((_bits(got[n]) != _bits(un[n])).sum())
        record_property("unfused_differs_" + n, diff)
        if (entry, n) in FUSED_EQUALS_UNFUSED:
            assert diff == 0, "%s: fused != un-fused in %d elements" % (n, diff)
        else:
            check_gates(record_property, n, un[n], ref[n], sat, W, prefix="unfused_")


# --------------------------------------------------------------------------- the operator
STEP_SHAPES = [(2, 32, 32, 9, 128), (2, 32, 12, 7, 13)]


@functools.lru_cache(maxsize=2)
def step_problem(shape, relu, winograd):
    B, C, Cr, H, W = shape
    gen = torch.Generator().manual_seed(11 + C + W + relu)
    rnd = lambda *s: torch.randn(*s, generator=gen)  # noqa: E731
    h, rest = torch.tanh(rnd(B, C, H, W)), rnd(B, Cr, H, W)
    rest = torch.cat([torch.relu(rest[:, :relu]), rest[:, relu:]], 1)   # rest[:, :relu] are ReLU outputs
    sc = (5 * (C + Cr)) ** -.5
    halves = tuple((rnd(2 * C, C + Cr, 5) * sc, rnd(B, 2 * C, H, W), rnd(C, C + Cr, 5) * sc, rnd(B, C, H, W)) for _ in range(2))
    go = rnd(B, C, H, W)
    f8 = lambda t: t.double()  # noqa: E731
    want = ge.step(ge.step_conv_f64, f8(h), f8(rest), tuple(tuple(map(f8, hf)) for hf in halves), f8(go), relu)
    emu = ge.step(ge.step_conv_fp32(winograd), h, rest, halves, go, relu)
    return h, rest, halves, go, want, emu


@pytest.mark.parametrize("fused", [True, False], ids=["fused", "unfused"])
@pytest.mark.parametrize("algo", ["winograd", "direct"])
@pytest.mark.parametrize("relu", [0, 5])
@pytest.mark.parametrize("shape", STEP_SHAPES, ids=sid)
def test_gru_step_operator(record_property, monkeypatch, sepconv5_algo, shape, relu, algo, fused):
    """hip_ops.gru_step with the epilogues on and off: the output and all six gradients against the float64 reference of
    the whole step, each tensor scaled by the fp32 emulation's own error: rel_l2 <= 3 max(rel_l2(emu), u)."""
    sepconv5_algo(algo)
    monkeypatch.setattr(gru_mod, "_GRU_EPILOGUES", fused)
    h, rest, halves, go, want, emu = step_problem(shape, relu, algo == "winograd")
    leaf = lambda t, g: t.detach().clone().to(DEV).requires_grad_(g)  # noqa: E731
    hh, rr = leaf(h, True), leaf(rest, True)
    k4 = lambda w, v: w.unsqueeze(-1) if v else w.unsqueeze(-2)  # noqa: E731
    hv = [(leaf(k4(w_zr, v), False), leaf(p_zr, True), leaf(k4(w_q, v), False), leaf(p_q, True))
          for v, (w_zr, p_zr, w_q, p_q) in enumerate(halves)]
    out = hip_ops.gru_step(hh, rr, tuple(hv), rest_relu_channels=relu)
    out.backward(go.to(DEV))
    got = [out, hh.grad, rr.grad] + [hf[i].grad for hf in hv for i in (1, 3)]
    for name, g_, w_, e_ in zip(("out", "dh", "d_rest", "dp_zr1", "dp_q1", "dp_zr2", "dp_q2"), got, want, emu):
        assert g_.shape == w_.shape and bool(torch.isfinite(g_).all())
        ratio = wg.rel_l2_64(g_.detach().cpu(), w_) / (3 * max(wg.rel_l2_64(e_, w_), U))
        record_property(name + "_stat_ratio", "%.3g" % ratio)
        assert ratio <= 1, (name, ratio)


# --------------------------------------------------------------------------- refusals, constants
def _refused(L, **kw):
    L.fill(True, 0)
    before = {n: f.buf.view(torch.int32).clone() for n, f in L.outs.items()}
    st = L(**kw)
    torch.cuda.synchronize()
    for n, f in L.outs.items():
        assert torch.equal(f.buf.view(torch.int32), before[n]), "a refused call touched " + n
    assert all(_unchanged(f) for f in L.ins.values())
    return st


@pytest.mark.parametrize("entry", ge.ENTRIES)
def test_refusals(entry):
    """C = 16, C = 40, Cr = 0 (backward) and a NULL for each required pointer in turn: PCFA_ERR_INVALID_ARG, outputs
    bit-unchanged."""
    for C in (16, 40):
        assert _refused(Launch(entry, (1, C, 12, 7, 13), 0)) == PCFA_ERR_INVALID_ARG, C
    L = Launch(entry, (1, 32, 12, 7, 13), 1)
    if entry.endswith("bwd"):
        assert _refused(L, Cr=0) == PCFA_ERR_INVALID_ARG
    for n in list(L.ins) + list(L.outs):
        if n not in OPTIONAL:
            assert _refused(L, **{n: None}) == PCFA_ERR_INVALID_ARG, n
    acc = int(entry == "update_bwd")   # (mode 4 adds to what d_rest holds)
    L.fill(True, acc)   # and the operands are fine: the same call goes through
    assert L(acc=acc) == 0
    L.collect()


def test_activation_constants(record_property):
    """c_sigmoid / c_tanh of tests/gru_epilogue.py, measured again from the un-fused kernels of gru_math.hip: the chosen
    constants are at least twice the maximum on the grid."""
    lib = _lib()
    x = ge.activation_grid().to(DEV)
    n = x.numel()
    one, z, r, rh, q, hn = (torch.ones_like(x) for _ in range(6))
    P = lambda t: ctypes.c_void_p(t.data_ptr())  # noqa: E731
    assert lib.pcfa_gru_gates_fwd(P(x), P(x), P(one), None, None, None, None, P(z), P(r), P(rh), n, n, 1, stream()) == 0
    assert lib.pcfa_gru_update_fwd(P(one), P(x), P(one), None, None, P(q), P(hn), n, n, 1, stream()) == 0
    torch.cuda.synchronize()
    x64 = x.cpu().double()
    ms = ge.units_of_u(z.cpu(), 1 / (1 + torch.exp(-x64)))
    mt = ge.units_of_u(q.cpu(), torch.tanh(x64))
    record_property("measured_sigmoid", "%.3f" % ms)
    record_property("measured_tanh", "%.3f" % mt)
    assert torch.equal(z, r)
    assert 2 * ms <= ge.C_SIGMOID and 2 * mt <= ge.C_TANH, (ms, mt)
    assert ms <= ge.MEASURED_SIGMOID and mt <= ge.MEASURED_TANH, (ms, mt)
