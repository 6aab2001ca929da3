"""The L-BFGS kernels through the C-ABI on fenced buffers (tests/fenced.py) against float64: pcfa_lbfgs_gram_reset / _update /
_direction (pcfa_amd/csrc/lbfgs_gram.hip), pcfa_lbfgs_direction and pcfa_lbfgs_pair (pcfa_amd/csrc/lbfgs.hip).  The references, the fp32
emulations, the case tables, the census and the derivation of every bound are in tests/optim.py; tests/test_optim_host_cpu.py
shows on the CPU that the cases reach their classes, that the emulations pass every gate and that one-line faults fail one.

Inputs sit between NaN; outputs, the state and the workspaces are exactly *_bytes() / *_floats() long and pre-filled with a
sentinel NaN.  After each call: the status (hip_ops._call raises on any but 0); every input and every fence bit-unchanged; no
sentinel where the contract says the kernel writes; a second call from the same initial state gives identical bits (none of
these kernels uses atomics).  The worst ratios of each case are junit properties (--junitxml=FILE -o junit_family=xunit1).

Kernel by kernel:
  gram_pass_kernel, gram_direction_kernel -- every Gram case: ld4 = 1 (smallest_n4), one full workgroup (block_edges_2048),
    a workgroup whose second half is past the end (block_edges_3072, and the last of n = 4099 / 1031), 293 workgroups
    (many_blocks); count 0 .. 128 and the candidate on every slot of the ring (rows_to_128).
  gram_reduce_kernel -- second trip of its lane loop: many_blocks (293 > 64 workgroups).
  gram_coeff_kernel -- m = 0 .. 128 one by one (rows_to_128: the second lane-row from m = 65, the i >= 64 pivots, every
    remainder of the prefetch, 16 staged elements, 135,168 B of LDS), rejections on an empty and a part-filled ring
    (rows_to_128) and on a full wrapped one (reject_on_full), first != 0 (every case that wraps), m = 64 / 65 on a full ring
    (second_row_edge), the attack's capacity wrapped 30 times (workload_cap).
  gram_direction_final_kernel -- second trip: many_blocks (293 > 256).
  lbfgs_step_kernel<FIRST, LOOP1, TURN, LOOP2, LAST> -- grid_stride (second trip, n % 4 = 3), tail_only (no float4 group at
    all; m = 1: FIRST, TURN, LAST alone), one_pair, full_ring (count == capacity, first = 4).
  lbfgs_pair_kernel, lbfgs_pair_final_kernel -- the same sizes, update_prev 0 and 1, and one-hot vectors at 0, 3, 4,
    1048575, 1048576, n - 1.
"""
import ctypes

import numpy as np
import pytest
import torch

from pcfa_amd import _hip, hip_ops
from tests import optim as op
from tests.fenced import NAN_BITS, PCFA_ERR_INVALID_ARG, PCFA_ERR_UNSUPPORTED, SENTINEL, Fenced, gamma, stream
from tests.gates import dense_stride, unchanged

pytestmark = pytest.mark.gpu
torch.set_num_threads(min(16, torch.get_num_threads()))
_call = hip_ops._call


def _lib():
    return _hip.load()


def _buf(shape, fill):
    shape = tuple(shape)
    return Fenced(shape, dense_stride(shape), fill)


def _in(t):
    return _buf(t.shape, NAN_BITS).write(t)


def _out(shape):
    return _buf(shape, SENTINEL)


def _bits(t):
    return t.contiguous().view(torch.int32)


def _words(f):
    """the operand's bits on the CPU"""
    return f.view().contiguous().view(torch.int32).cpu()


def _no_sentinel(t):
    return not bool((_bits(t) == SENTINEL).any())


def _restore(fs, snaps):
    for f, s in zip(fs, snaps):
        f.buf.view(torch.int32).copy_(s)


# --------------------------------------------------------------------------- Gram form
def _header(state_words):
    i = state_words[:4].tolist()
    f = state_words[4:10].view(torch.float32).tolist()
    return tuple(i), dict(zip(("H", "cg", "ys", "yy", "gtd", "dmax"), f))


@pytest.mark.parametrize("kind", op.KINDS)
@pytest.mark.parametrize("case", op.GRAM_CASES, ids=lambda c: c.name)
def test_gram(record_property, case, kind):
    lib = _lib()
    cap, n, rows = case.cap, case.n, case.cap + 1
    ld = (n + 3) // 4 * 4
    steps, _ = op.gram_trajectory(case, kind)
    feeds = op.feed_inputs(case, kind)
    nstate, nws = int(lib.pcfa_lbfgs_gram_state_bytes(cap)), int(lib.pcfa_lbfgs_gram_workspace_bytes(cap, ld))
    nblk = op.gram_blocks(ld)
    assert nws == (rows * 4 * nblk + 2 * nblk) * 4 and nstate % 4 == 0
    state, ws = _out((nstate // 4,)), _out((nws // 4,))
    S, Y, out2 = _out((rows, ld)), _out((rows, ld)), _out((2,))
    fg, fprev, fd = _in(feeds[0][0]), _in(feeds[0][1]), _in(feeds[0][2])
    mutable = [fprev, S, Y, state, ws, fd, out2]
    P = lambda f: f.ptr()   # noqa: E731

    _call("pcfa_lbfgs_gram_reset", P(state), cap)
    torch.cuda.synchronize()
    hdr, fl = _header(_words(state))
    assert hdr == (0, 0, 0, rows) and fl == dict(H=1.0, cg=-1.0, ys=0.0, yy=0.0, gtd=0.0, dmax=0.0)
    assert state.fence_intact() and bool((_words(state)[10:] == SENTINEL).all()), "the reset wrote more than the header"

    def run():
        _call("pcfa_lbfgs_gram_update", P(fg), P(fprev), P(fd), op.T_STEP, P(S), P(Y), P(state), P(ws), cap, ld)
        _call("pcfa_lbfgs_gram_direction", P(fg), P(S), P(Y), P(state), P(fd), P(out2), P(ws), cap, ld)
        torch.cuda.synchronize()

    worst = dict(elem=0.0, stat=0.0, gtd=0.0, ys=0.0)
    per_m = {}
    H_bits = _words(state)[4].item()
    for st, (grad, g_prev, d) in zip(steps, feeds):
        fg.write(grad)
        fd.write(d)
        assert torch.equal(_words(fprev), _bits(g_prev)), "g_prev is not the previous gradient"
        snaps = [f.buf.view(torch.int32).clone() for f in mutable]
        S0, Y0 = _words(S), _words(Y)
        run()
        assert unchanged(fg), "the gradient was written"
        assert all(f.fence_intact() for f in mutable), "a store landed outside a buffer"
        first_bits = [f.buf.view(torch.int32).clone() for f in mutable]
        sw = _words(state)
        hdr, fl = _header(sw)
        # bookkeeping and the scalars of the pair
        assert hdr == st.header, (st.feed, hdr, st.header)
        assert abs(fl["ys"] - st.ys64) <= gamma(op.DOT_DEPTH) * st.ys_abs and abs(fl["yy"] - st.yy64) <= gamma(op.DOT_DEPTH) * st.yy_abs
        op.fold(worst, "ys", abs(fl["ys"] - st.ys64) / (gamma(op.DOT_DEPTH) * st.ys_abs))
        if st.accepted:
            assert np.float32(fl["H"]) == np.float32(fl["ys"]) / np.float32(fl["yy"])
            H_bits = sw[4].item()
        assert sw[4].item() == H_bits and fl["cg"] == -fl["H"]
        # the pair, g_prev, the untouched rows
        assert torch.equal(_words(fprev), _bits(grad))
        Sw, Yw = _words(S), _words(Y)
        assert torch.equal(Sw[st.crow, :n], _bits(st.s32)) and torch.equal(Yw[st.crow, :n], _bits(st.y32))
        assert not bool(Sw[st.crow, n:].any()) and not bool(Yw[st.crow, n:].any())
        others = torch.arange(rows) != st.crow
        assert torch.equal(Sw[others], S0[others]) and torch.equal(Yw[others], Y0[others]), "a row other than the candidate's changed"
        # what the contract says is written holds no sentinel
        live = [(hdr[0] + k) % rows for k in range(hdr[1])]
        o_cS, o_cY, o_red = 12, 12 + (rows + 3) // 4 * 4, 12 + 2 * ((rows + 3) // 4 * 4)
        assert _no_sentinel(sw[:10]) and _no_sentinel(sw[o_red:o_red + rows * 8])
        assert _no_sentinel(sw[o_cS:o_cS + rows][live]) and _no_sentinel(sw[o_cY:o_cY + rows][live])
        dk = fd.view().cpu()
        assert bool(torch.isfinite(dk).all()) and not bool(dk[n:].abs().sum())
        gtd, dmax = out2.view().cpu().tolist()
        assert gtd == fl["gtd"] and dmax == fl["dmax"] == float(dk.abs().max())
        g64, d64k = grad[:n].double(), dk[:n].double()
        b_gtd = gamma(op.DOT_DEPTH) * float((g64 * d64k).abs().sum())
        assert abs(gtd - float(g64 @ d64k)) <= b_gtd
        op.fold(worst, "gtd", abs(gtd - float(g64 @ d64k)) / b_gtd)
        # the two gates of d
        e, s_ = op.elem_ratio(dk[:n], st.d64, st.bound), op.stat_ratio(dk[:n], st.d64, st.dE)
        worst["elem"], worst["stat"] = max(worst["elem"], e), max(worst["stat"], s_)
        per_m[st.m] = max(per_m.get(st.m, (0.0, 0.0)), (op.rel_l2(dk[:n], st.d64), op.rel_l2(st.dE, st.d64)))
        assert e <= 1 and s_ <= 1, (st.feed, st.m, e, s_, op.rel_l2(dk[:n], st.d64), op.rel_l2(st.dE, st.d64))
        # the same call from the same state
        _restore(mutable, snaps)
        run()
        assert all(torch.equal(f.buf.view(torch.int32), b) for f, b in zip(mutable, first_bits)), "not repeatable bit for bit"
    for k, v in worst.items():
        record_property(k + "_ratio", "%.3g" % v)
    for m in sorted(set(per_m) & {1, 6, 63, 64, 65, 100, 128, max(per_m)}):
        record_property("rel_l2_m%d" % m, "kernel %.3g emulation %.3g" % per_m[m])


def test_gram_refusals():
    """Each returns its status before any launch: no buffer is touched"""
    lib = _lib()
    cap, ld = 5, 1032
    rows = cap + 1
    assert int(lib.pcfa_lbfgs_gram_state_bytes(0)) == 0 and int(lib.pcfa_lbfgs_gram_state_bytes(129)) == 0
    assert int(lib.pcfa_lbfgs_gram_state_bytes(128)) > 2 * 129 * 129 * 8
    for c, l in ((0, ld), (129, ld), (cap, ld + 2), (cap, 0)):
        assert int(lib.pcfa_lbfgs_gram_workspace_bytes(c, l)) == 0
    state, ws = _out((int(lib.pcfa_lbfgs_gram_state_bytes(cap)) // 4,)), _out((int(lib.pcfa_lbfgs_gram_workspace_bytes(cap, ld)) // 4,))
    big = _out((int(lib.pcfa_lbfgs_gram_state_bytes(128)) // 4,))
    S, Y, out2 = _out((rows, ld)), _out((rows, ld)), _out((2,))
    fg, fprev, fd = (_in(torch.randn(ld)) for _ in range(3))
    every = [state, ws, big, S, Y, out2, fg, fprev, fd]
    P = lambda f: f.ptr()   # noqa: E731
    off = lambda f: ctypes.c_void_p(f.ptr().value + 4)   # noqa: E731
    s = stream()

    def refused(status, want):
        torch.cuda.synchronize()
        assert status == want, (status, want)
        assert all(unchanged(f) for f in every), "a refused call touched a buffer"

    def update(g=P(fg), gp=P(fprev), d=P(fd), S_=P(S), Y_=P(Y), st=P(state), c=cap, l=ld):
        return lib.pcfa_lbfgs_gram_update(g, gp, d, op.T_STEP, S_, Y_, st, P(ws), c, l, s)

    def direction(g=P(fg), S_=P(S), Y_=P(Y), st=P(state), d=P(fd), c=cap, l=ld):
        return lib.pcfa_lbfgs_gram_direction(g, S_, Y_, st, d, P(out2), P(ws), c, l, s)

    for fn in (update, direction):
        refused(fn(l=ld + 2), PCFA_ERR_INVALID_ARG)
        refused(fn(l=0), PCFA_ERR_INVALID_ARG)
        refused(fn(c=0), PCFA_ERR_INVALID_ARG)
        refused(fn(c=129, st=P(big)), PCFA_ERR_UNSUPPORTED)
        for name in ("g", "S_", "Y_", "st", "d"):
            refused(fn(**{name: off({"g": fg, "S_": S, "Y_": Y, "st": state, "d": fd}[name])}), PCFA_ERR_INVALID_ARG)
        refused(fn(g=None), PCFA_ERR_INVALID_ARG)
    refused(update(gp=off(fprev)), PCFA_ERR_INVALID_ARG)
    refused(lib.pcfa_lbfgs_gram_reset(P(state), 0, s), PCFA_ERR_INVALID_ARG)
    refused(lib.pcfa_lbfgs_gram_reset(P(big), 129, s), PCFA_ERR_INVALID_ARG)
    refused(lib.pcfa_lbfgs_gram_reset(None, cap, s), PCFA_ERR_INVALID_ARG)


# --------------------------------------------------------------------------- two-loop form
def _ring(case, pairs, ro):
    """S, Y [capacity][ld] and ro [capacity] with the live pairs on their slots, NaN everywhere else (pads included)"""
    ld = (case.n + 3) // 4 * 4
    S = torch.full((case.capacity, ld), float("nan"))
    Y, r = S.clone(), torch.full((case.capacity,), float("nan"))
    for k, (s, y) in enumerate(pairs):
        slot = (case.first + k) % case.capacity
        S[slot, :case.n], Y[slot, :case.n], r[slot] = s, y, float(ro[k])
    return S, Y, r, ld


@pytest.mark.parametrize("case", op.LOOP_CASES, ids=lambda c: c.name)
def test_two_loop_direction(record_property, case):
    lib = _lib()
    d64, dE, bound, (g, pairs, ro, H) = op.loop_reference(case)
    S, Y, r, ld = _ring(case, pairs, ro)
    ins = [_in(g), _in(S), _in(Y), _in(r), _in(torch.tensor([float(H)]))]
    al, d, ws = _out((case.count,)), _out((case.n,)), _out((int(lib.pcfa_lbfgs_workspace_floats()),))
    outs = [al, d, ws]
    res = []
    for _ in range(2):
        for f in outs:
            f.buf.view(torch.int32).copy_(f.bits0)
        _call("pcfa_lbfgs_direction", *[f.ptr() for f in ins], al.ptr(), d.ptr(), ws.ptr(), case.first, case.count, case.capacity,
              ld, case.n)
        torch.cuda.synchronize()
        assert all(unchanged(f) for f in ins), "an input was written"
        assert all(f.fence_intact() for f in outs), "a store landed outside an output or the workspace"
        res.append([_words(f) for f in outs])
    assert all(torch.equal(a, b) for a, b in zip(*res)), "not repeatable bit for bit"
    got, alk = d.view().cpu(), al.view().cpu()
    assert bool(torch.isfinite(got).all()) and bool(torch.isfinite(alk).all()), "a sentinel, or a NaN read from a dead slot or a pad"
    e, s_ = op.elem_ratio(got, d64, bound), op.stat_ratio(got, d64, dE)
    record_property("elem_ratio", "%.3g" % e)
    record_property("stat_ratio", "%.3g" % s_)
    record_property("rel_l2", "kernel %.3g emulation %.3g" % (op.rel_l2(got, d64), op.rel_l2(dE, d64)))
    assert e <= 1 and s_ <= 1, (e, s_)


def _pair_call(lib, n, g, g_prev, d, update_prev):
    """One checked pcfa_lbfgs_pair: (y, s, g_prev after, scal4)"""
    fg, fd, fprev = _in(g), _in(d), _in(g_prev)
    y, s, scal, ws = _out((n,)), _out((n,)), _out((4,)), _out((int(lib.pcfa_lbfgs_workspace_floats()),))
    outs = [y, s, scal, ws, fprev]
    res = []
    for _ in range(2):
        for f in outs:
            f.buf.view(torch.int32).copy_(f.bits0)
        _call("pcfa_lbfgs_pair", fg.ptr(), fprev.ptr(), fd.ptr(), op.T_STEP, y.ptr(), s.ptr(), scal.ptr(), ws.ptr(), update_prev, n)
        torch.cuda.synchronize()
        assert unchanged(fg) and unchanged(fd), "an input was written"
        assert all(f.fence_intact() for f in outs), "a store landed outside an output or the workspace"
        res.append([_words(f) for f in outs])
    assert all(torch.equal(a, b) for a, b in zip(*res)), "not repeatable bit for bit"
    assert _no_sentinel(res[0][3]), "a partial sum was never written"
    return y.view().cpu(), s.view().cpu(), fprev.view().cpu(), scal.view().cpu()


@pytest.mark.parametrize("update_prev", (0, 1))
@pytest.mark.parametrize("n", op.PAIR_NS)
def test_pair(record_property, n, update_prev):
    g, g_prev, d = op.pair_inputs(n)
    y, s, prev, scal = _pair_call(_lib(), n, g, g_prev, d, update_prev)
    yw, sw = g - g_prev, d * np.float32(op.T_STEP)
    assert torch.equal(_bits(y), _bits(yw)) and torch.equal(_bits(s), _bits(sw))
    assert torch.equal(_bits(prev), _bits(g if update_prev else g_prev))
    worst = {}
    for key, got, a, b in (("ys", scal[0], yw, sw), ("yy", scal[1], yw, yw)):
        want, mag = float(a.double() @ b.double()), float((a.double() * b.double()).abs().sum())
        op.fold(worst, key, abs(float(got) - want) / (gamma(op.pair_depth(n)) * mag))
    record_property("sum_ratio", "%.3g" % max(worst.values()))
    ys, yy = np.float32(scal[0].item()), np.float32(scal[1].item())
    assert np.float32(scal[2].item()) == np.float32(1) / ys and np.float32(scal[3].item()) == ys / yy


@pytest.mark.parametrize("at", op.ONE_HOT_AT)
def test_pair_one_hot_is_exact(at):
    """One element of 2.7 M missing from a sum is far below any value gate; here it is the whole sum"""
    n = 1049779
    g, d, z = torch.zeros(n), torch.zeros(n), torch.zeros(n)
    g[at], d[at] = 2.0 ** 5, 2.0 ** -3
    y, s, _, scal = _pair_call(_lib(), n, g, z, d, 1)
    assert scal.tolist()[:2] == [2.0 ** 5 * 0.75 * 2.0 ** -3, 2.0 ** 10]
    assert float(y[at]) == 2.0 ** 5 and float(s[at]) == 0.75 * 2.0 ** -3 and int((y != 0).sum()) == int((s != 0).sum()) == 1


def test_two_loop_refusals():
    lib = _lib()
    case = op.LOOP_CASES[-1]
    d64, dE, bound, (g, pairs, ro, H) = op.loop_reference(case)
    S, Y, r, ld = _ring(case, pairs, ro)
    fg, fS, fY, fr, fH = _in(g), _in(S), _in(Y), _in(r), _in(torch.tensor([float(H)]))
    al, d, ws = _out((case.count,)), _out((case.n,)), _out((int(lib.pcfa_lbfgs_workspace_floats()),))
    y, s_, scal = _out((case.n,)), _out((case.n,)), _out((4,))
    every = [fg, fS, fY, fr, fH, al, d, ws, y, s_, scal]
    P = lambda f: f.ptr()   # noqa: E731
    off = lambda f: ctypes.c_void_p(f.ptr().value + 4)   # noqa: E731
    st = stream()
    assert int(lib.pcfa_lbfgs_workspace_floats()) == 2048

    def refused(status):
        torch.cuda.synchronize()
        assert status == PCFA_ERR_INVALID_ARG, status
        assert all(unchanged(f) for f in every), "a refused call touched a buffer"

    def direction(g_=P(fg), S_=P(fS), Y_=P(fY), d_=P(d), first=case.first, count=case.count, cap=case.capacity, l=ld, n=case.n):
        return lib.pcfa_lbfgs_direction(g_, S_, Y_, P(fr), P(fH), P(al), d_, P(ws), first, count, cap, l, n, st)

    refused(direction(count=0))
    refused(direction(cap=case.count - 1))
    refused(direction(first=case.capacity))
    refused(direction(first=-1))
    refused(direction(l=case.n - 3))
    refused(direction(l=ld + 2))
    refused(direction(n=0))
    for kw in (dict(g_=off(fg)), dict(S_=off(fS)), dict(Y_=off(fY)), dict(d_=off(d)), dict(g_=None)):
        refused(direction(**kw))

    def pair(g_=P(fg), p_=P(fS), d_=P(fY), y_=P(y), s2=P(s_), n=case.n):
        return lib.pcfa_lbfgs_pair(g_, p_, d_, op.T_STEP, y_, s2, P(scal), P(ws), 1, n, st)

    refused(pair(n=0))
    for kw in (dict(g_=off(fg)), dict(p_=off(fS)), dict(d_=off(fY)), dict(y_=off(y)), dict(s2=off(s_)), dict(y_=None)):
        refused(pair(**kw))
