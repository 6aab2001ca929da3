"""The float64 reference, the bounds and the case table of tests/test_gru_epilogue_f64_gpu.py (tests/gru_epilogue.py), on
the CPU (no GPU).

The reference of a whole SepConvGRU step -- forward modes 1 -> 2 per half-step, the un-fused update backward, then modes
3 -> 4 -> 3 -- equals float64 autograd of the formula (models/raft/update.py:45-60), which proves the four statements and
the [B][2C] channel layout of dzr; the case table reaches every (entry point, path, orientation); and two plain fp32
implementations pass both gates on every output of every case: the emulation in the kernel's order of summation, and
torch's own fp32 convolution followed by torch.sigmoid / torch.tanh, which shares nothing with the emulation but the
formula.  So a kernel that misses a gate is wrong and not merely differently rounded.
"""
import pytest
import torch
import torch.nn.functional as F

from tests import gru_epilogue as ge
from tests import winograd as wg
from tests.gates import gates

torch.set_num_threads(min(16, torch.get_num_threads()))


def _formula(h, rest, halves):
    """models/raft/update.py:45-60 with the context's share of the pre-activations (bias included) as p_zr / p_q"""
    C = h.shape[1]
    for v, (w_zr, p_zr, w_q, p_q) in enumerate(halves):
        k = (lambda w: w.unsqueeze(-1)) if v else (lambda w: w.unsqueeze(-2))
        pad = (2, 0) if v else (0, 2)
        hx = torch.cat([h, rest], 1)
        zr = F.conv2d(hx, k(w_zr), padding=pad) + p_zr
        z, r = torch.sigmoid(zr[:, :C]), torch.sigmoid(zr[:, C:])
        q = torch.tanh(F.conv2d(torch.cat([r * h, rest], 1), k(w_q), padding=pad) + p_q)
        h = (1 - z) * h + z * q
    return h


@pytest.mark.parametrize("rest_relu", [0, 3])
@pytest.mark.parametrize("shape", [(2, 8, 5, 6, 7), (1, 32, 12, 7, 13)], ids=lambda s: "x".join(map(str, s)))
def test_reference_equals_autograd(shape, rest_relu):
    B, C, Cr, H, W = shape
    gen = torch.Generator().manual_seed(C + W)
    rnd = lambda *s: torch.randn(*s, generator=gen, dtype=torch.float64)  # noqa: E731
    h, rest_pre = torch.tanh(rnd(B, C, H, W)), rnd(B, Cr, H, W)
    halves = [(rnd(2 * C, C + Cr, 5) / (5 * (C + Cr)) ** .5, rnd(B, 2 * C, H, W), rnd(C, C + Cr, 5) / (5 * (C + Cr)) ** .5,
               rnd(B, C, H, W)) for _ in range(2)]
    go = rnd(B, C, H, W)
    leaves = [h, rest_pre] + [hf[i] for hf in halves for i in (1, 3)]
    for t in leaves:
        t.requires_grad_(True)
    # rest[:, :rest_relu] are ReLU outputs: the step returns their gradient already multiplied by [rest > 0]
    rest = torch.cat([torch.relu(rest_pre[:, :rest_relu]), rest_pre[:, rest_relu:]], 1)
    out = _formula(h, rest, halves)
    grads = torch.autograd.grad(out, leaves, go)
    with torch.no_grad():
        got = ge.step(ge.step_conv_f64, h, rest, halves, go, rest_relu)
    for name, g_, w_ in zip(("out", "dh", "d_rest", "dp_zr1", "dp_q1", "dp_zr2", "dp_q2"), got, (out,) + tuple(grads)):
        assert g_.shape == w_.shape
        assert wg.rel_l2_64(g_, w_.detach()) < 1e-12, (name, wg.rel_l2_64(g_, w_.detach()))


def test_problem_is_the_step():
    """problem()'s `want` of each entry point is what `step` computes at that place: the same epilogue functions on the
    same convolution, with the operands problem() draws (so the entry-level reference inherits the proof above)."""
    B, C, Cr, H, W = 2, 32, 12, 7, 13
    d = ge.inputs(B, C, Cr, H, W, 0)
    f8 = lambda t: t.double()  # noqa: E731
    o, _ = ge.problem(B, C, Cr, H, W, 0, "gates_fwd", False, 0)
    z, r, rh = ge.epi_gates_fwd(ge.conv_f64(torch.cat([d.h, d.rest], 1), d.w_zr, 0) + f8(d.add_zr), f8(d.h))
    assert torch.equal(o["z"][0], z) and torch.equal(o["r"][0], r) and torch.equal(o["rh"][0], rh)
    o, _ = ge.problem(B, C, Cr, H, W, 0, "gates_bwd", False, 0)
    y = ge.conv_f64(d.dqc, ge.bwd_weight(d.w_q), 0)
    dzr, dh = ge.epi_gates_bwd(y[:, :C], f8(d.z), f8(d.r), f8(d.h), f8(d.dz), f8(d.dh_in))
    assert torch.equal(o["dzr"][0], dzr) and torch.equal(o["dh"][0], dh) and torch.equal(o["d_rest"][0], y[:, C:])
    assert torch.equal(o["d_rest_acc"][0], y[:, C:] + f8(d.prev_rest))
    o, _ = ge.problem(B, C, Cr, H, W, 0, "update_bwd", False, 0)
    y = ge.conv_f64(d.dzr, ge.bwd_weight(d.w_zr), 0)
    dz, dqc, dh = ge.epi_update_bwd(f8(d.dh_acc) + y[:, :C], f8(d.z), f8(d.q), f8(d.h))
    assert torch.equal(o["dz"][0], dz) and torch.equal(o["dqc"][0], dqc) and torch.equal(o["dh"][0], dh)


def test_case_table_reaches_every_path():
    """4 entry points x 5 path labels x 2 orientations = 40 triples, each reached by a case under one of the two algo
    settings; the 5x1 runs of the first two cases do take H = 101."""
    seen = {}
    for case in ge.CASES:
        for v in (0, 1):
            shape = ge.run_shape(case, v)
            for entry in ge.ENTRIES:
                for on in (True, False):
                    seen.setdefault((entry, ge.path(entry, *shape, v, on), v), shape)
    want = {(e, lab, v) for e in ge.ENTRIES for lab in ge.LABELS for v in (0, 1)}
    assert len(want) == 40 and set(seen) == want, sorted(want - set(seen))
    assert ge.run_shape(ge.CASES[0], 1)[3] == 101 and ge.run_shape(ge.CASES[1], 1)[3] == 101
    assert ge.run_shape(ge.CASES[0], 0)[3] == 100
    B, C, Cr, H, W = ge.CASES[0]   # pairs that test_gru_step_vs_oracle's shapes never ran
    assert ge.path("update_fwd", B, C, Cr, H, W, 0) == "wino_wide" and ge.path("update_fwd", B, C, Cr, H, W, 0, False) == "direct_fast"
    assert all(ge.path(e, *ge.CASES[6], 0) == "direct_slow" for e in ge.ENTRIES)


def problems():
    """(case, vertical, entry, wino) of every distinct problem of the GPU module, in its order"""
    out = []
    for case in ge.CASES:
        for v in (0, 1):
            shape = ge.run_shape(case, v)
            for entry in ge.ENTRIES:
                for wino in sorted({ge.path(entry, *shape, v, on).startswith("wino") for on in (True, False)}, reverse=True):
                    out.append((shape, v, entry, wino))
    return out


@pytest.mark.parametrize("shape,v,entry,wino", problems(),
                         ids=lambda p: "x".join(map(str, p)) if isinstance(p, tuple) else str(int(p)) if isinstance(p, bool) else str(p))
def test_fp32_implementations_pass_the_gates(record_property, shape, v, entry, wino):
    B, C, Cr, H, W = shape
    Ca, Cb, Cout = ge.op_shape(entry, C, Cr)
    outs, sat = ge.problem(*shape, v, entry, wino, wg.sepconv5_wino_groups(B, Cout, H, W, v) if wino else 0)
    d = ge.inputs(*shape, v)
    x, wt, backward = ge.operand(d, entry)
    weff = ge.bwd_weight(wt) if backward else wt
    y = F.conv2d(x, weff.unsqueeze(-1 if v else -2).contiguous(), padding=(2, 0) if v else (0, 2))
    assert y.dtype == torch.float32
    if entry == "gates_fwd":
        zr = torch.sigmoid(y + d.add_zr)
        plain = {"z": zr[:, :C], "r": zr[:, C:], "rh": zr[:, C:] * d.h}
    elif entry == "update_fwd":
        q = torch.tanh(y + d.add_q)
        plain = {"q": q, "hnew": torch.addcmul((1 - d.z) * d.h, d.z, q)}
    elif entry == "gates_bwd":
        dzr, dh = ge.epi_gates_bwd(y[:, :C], d.z, d.r, d.h, d.dz, d.dh_in)
        plain = {"dzr": dzr, "dh": dh, "dh_null": y[:, :C] * d.r, "d_rest": y[:, C:], "d_rest_acc": d.prev_rest + y[:, C:]}
    else:
        dz, dqc, dh = ge.epi_update_bwd(d.dh_acc + y[:, :C], d.z, d.q, d.h)
        plain = {"dz": dz, "dqc": dqc, "dh": dh, "d_rest": d.prev_rest + y[:, C:]}
    assert set(plain) == set(outs)
    for name, (want, bound, emu) in outs.items():
        assert wg.rel_l2_64(emu, want) < 1e-5, "the emulation is not this expression"   # a misplaced term is of order 1
        assert bool((bound > 0).all()) and bool(torch.isfinite(bound).all())
        extra = {"saturated": sat[name]} if name in sat else None
        kw = dict(bound=bound, regions=ge.groups_of(W), extra=extra)
        e1, _ = gates(emu, want, None, 0, emu, 2, record_property, prefix=name + "_emu_", **kw)
        e2, s2 = gates(plain[name], want, None, 0, emu, 2, record_property, prefix=name + "_torch_", **kw)
        assert max(e1, e2) < 1 and s2 < 1
    for name in sat:   # the saturated tails: finite everywhere, exactly 0 / 1 / +-1 where float64 rounds to that
        e = outs[name][2]
        assert bool(torch.isfinite(e).all())
        if name in ("z", "r", "q"):
            add = d.add_q if name == "q" else d.add_zr[:, :C] if name == "z" else d.add_zr[:, C:]
            hard, value = ge.saturated_exact(add, name != "q")
            assert int(hard.sum()) > 0 and torch.equal(e[hard], value[hard]), name
            assert float((outs[name][0][hard] - value[hard].double()).abs().max()) < 1e-10
