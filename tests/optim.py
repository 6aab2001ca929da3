"""References, emulations, case tables, census and bounds of tests/test_lbfgs_f64_gpu.py and tests/test_attack_math_f64_gpu.py:
the optimiser side of the attack (pcfa_amd/csrc/lbfgs_gram.hip, lbfgs.hip and attack_math.hip).  Not a test; no GPU.
tests/test_optim_host_cpu.py shows on the CPU that every case reaches its classes, that the fp32 emulations pass every gate
against float64 and that seven one-line faults (MUTANTS) each fail one.

u = 2^-24, gamma(k) = k u / (1 - k u) (tests/fenced.py).  Every reference is float64 arithmetic on the same fp32 inputs.

L-BFGS, Gram form (GramEmu mirrors gram_pass / gram_reduce / gram_coeff / gram_direction, ring bookkeeping included)
  Reference: the textbook two-loop recursion in float64 on the pairs RefBook kept (two_loop_f64).
  Inner products: per lane a chain of 8 fused multiply-adds, the wave (the DPP steps of wave_sum_lane63 add up to the
    balanced tree in lane order: quads, rows of 16, the four rows), the 4 waves in turn (fp32), the workgroups in float64:
    depth 8 + 6 + 3 = 17 fp32 roundings, one more for the cast where a value leaves as fp32.  DOT_DEPTH = 20 bounds g.d, y.s
    and y.y:  |x - x64| <= gamma(20) sum|a_i b_i|.  The emulation follows this order exactly, fusing included: with few pairs
    the error of d is the error of H = ys / yy, one number and no statistic, and an emulation that rounds the products gets
    another one (block_edges_2048-corr, m = 1: 6.2e-8 unfused, 2.27e-7 fused, and 2.27e-7 is what the kernel gives).
  d = cg g + sum_k (cY_k y_k + cS_k s_k), newest pair first, one multiply and 2m FMAs per element.  With exact coefficients
    the assembly is off by at most gamma(2m + 1) P_i, P_i = |cg g_i| + sum|cY_k y_ki| + sum|cS_k s_ki|; two more roundings
    (the fp32 casts of the coefficients, H = ys / yy) give gamma(2m + 3).  The coefficients themselves come
    from fp32 inner products with heavy cancellation (s.g of two unrelated vectors of length n keeps sqrt(n) of n), so their
    error is not a few u: it is MEASURED, on the emulation, against the float64 coefficients c64 (the same substitutions on
    float64 inner products; substitutions_equal_two_loop pins them to the two-loop recursion).  One realisation of one
    coefficient can be small by chance, so eps_k = max(|cE_k - c64_k| over two realisations of the inner products (kernel
    order; torch's matrix-vector product), their root mean square over the 2m + 1 coefficients of the solve, u |c64_k|), and
        |d_i - d64_i| <= gamma(2m + 3) P_i + 3 (eps_g |g_i| + sum_k eps_Yk |y_ki| + eps_Sk |s_ki|) + (2m + 3) 2^-126.
  Statistical: rel_l2(d, d64) <= 3 max(rel_l2(E, d64), u), E the emulation's d; as in tests/gates.py a vector of fewer than
    256 elements (smallest, tail_only) is no statistic and is left to the elementwise gate.
  Measured on the CPU (n = 4099, both kinds, every m up to 128): E within 4.2e-7 of float64 (a numpy emulation with rounded
  products: 5.1e-7), a plain fp32 two-loop recursion within 4.0e-7, so the statistical gate sits near 1.3e-6 at m = 128 and
  near 9e-7 at m = 64; the test of 6 pairs that came before asked 2e-5.  KERNEL_MEASURED holds the kernel's own error.

L-BFGS, two-loop form (two_loop_f32: the recursion of lbfgs_step_kernel in torch fp32)
  The same two gates; the coefficients are cg = -H, cY_k = -H al_k, cS_k = al_k - be_k, the second realisation sums every
  dot product in float64 and rounds it once.  pcfa_lbfgs_pair: y and s are one rounding each (bit-equal to torch), ys and yy
  a chain over the trips of the grid-stride loop (ceil(n / 4 / 262144)) of 4 products each, one more term in threads
  0 .. n % 4 - 1 of block 0 (the scalar tail, added after the trips), the block (6 + 4), the 4 partials per thread of the
  final kernel, its block (6 + 4): pair_depth(n) = 4 trips + [n % 4 != 0] + 24, + 1 for the product (34 at n = 1,049,779).

Reductions of attack_math.hip (loss_partial_kernel / loss_final_kernel; strided_sum32 is their order)
  1024 x 256 threads: thread i adds elements i, i + 262144, ... (ceil(N / 262144) additions), 6 shuffle levels, 4 wave
  partials, 4 block partials per thread of the final kernel, 6 levels, 4 waves:  D(N) = ceil(N / 262144) + 24 additions at
  most on the path of any element.  A term carries r roundings of its own (TERM_R: the end-point error sqrt(du^2 + dv^2) 3,
  its square 4, a product sum of two channels 2, a square 1) and the scalar leaves through at most two more operations, so
        |S - S64| <= gamma(D + 2 + r) sum|t_i|.
  The loss is gated term by term (loss_bounds): the similarity term (cosim: the three sums propagated through
  1 - pt / sqrt(pp) sqrt(tt)), the mean square, and the total within B_sim + mu (B_msq + u |msq - bound^2|) + 2 u |loss|.
  bound^2 is float(delta_bound^2) as in the kernel and in the reference project (torch.tensor(delta_bound ** 2)).
  Outside the tie case the inputs are built so that |msq64 - bound^2| >= 1000 B_msq (asserted in loss_case): the regime of
  the penalty is a property of the case, not of the rounding.

Loss gradient (flow_grad_bound / the delta gradient)
  aee: g = gl / npix, gs = g / (2 sqrt(sq)), gu = gs (2 du): 1 + 3 + 1 + 1 + 1 roundings -> gamma(8) |gu64|; NaN exactly
  where pred == target (inf 0), as float64 autograd.  mse: gamma(4).  cosim: a = -gl stt / spp, c = gl stt pt / (2 pp spp)
  from the forward sums: |da| <= |a| (e_tt / 2 + e_pp / 2 + 5u), |dc| <= |c| (e_tt / 2 + 3 e_pp / 2 + 7u) + |c / pt| E_pt,
  |dgu| <= |da tu| + |dc 2 pu| + 3u (|a tu| + |c 2 pu|), e_* the relative and E_pt the absolute reduction bounds.
  Deltas: gl mu sel / ndelta (2 d) mult: gamma(4) |g64|; exactly 0 below the bound; sel = 1/2 at the exact tie.

Element-wise kernels
  Clipping and joint: inputs are multiples of 1/64 (gradients of 1/256), every sum and product is exact: bit-equal to
  float64 rounded, forward and backward, the mask inclusive at exactly 0 and 1.
  Change of variables: e_t = max |tanh32 - tanh64| of the CPU emulation over the case's inputs, the kernel's tanhf is allowed
  3 e_t.  Forward: the project's 2e-7 (x scale), absolute.  Gradient g k (1 - t^2): the error of t enters 1 - t^2 as
  2 |t| dt + dt^2, absolute (the cancellation leaves no relative accuracy), the square and the difference add 2u:
        |dg| <= |g k| (6 e_t |t| + 9 e_t^2 + 2u) + gamma(3) |g64| + 2^-126    (x B for the batch sum of grad_delta, + gamma(B) sum|g64|).
  Exactly 0 at |x| >= 12 and +-inf: tanhf is 1 there (1 - tanh 12 = 7.5e-11 < u / 2).
  pm1_pair: the torch fp32 expression on the GPU is the reference, bit for bit.

Which case reaches what (census() returns it, the CPU module asserts it)
  gram_pass_kernel / gram_direction_kernel: ld4 = 1 (every lane but one clamped to ld4 - 1 = 0; smallest), 512 (no clamped
    lane) and 768 (ok1 false for a whole workgroup; block_edges), 3 workgroups with a ragged end (n = 4099, 1031), 293
    (many_blocks); count = 0 .. 128 (rows_to_128), the candidate row on every ring slot, wrapped.
  gram_reduce_kernel: second trip of the lane loop (> 64 workgroups) -- many_blocks.
  gram_coeff_kernel: m = 0 .. 128: rows_to_128 (m = 63 / 64 / 65 and 127 / 128: the second lane-row r1 / a1 / g1 / k1 and the
    i >= 64 pivots; all four remainders of the 4-step prefetch; up to 16 staged elements per thread, 135,168 B of LDS),
    rejections on an empty (feed 0) and a part-filled ring (5, 64, and 130 at m = 127); on a full, wrapped ring:
    reject_on_full; first != 0: every wrapped case;
    second_row_edge: a full ring whose last row is lane 63 of the first / lane 0 of the second lane-row; workload_cap:
    cap 100 wrapped 30 times.
  gram_direction_final_kernel: second trip (> 256 workgroups) -- many_blocks.
  lbfgs_step_kernel<FIRST .. LAST>, lbfgs_pair_kernel: second trip of the grid-stride loop and the n % 4 = 3 tail --
    grid_stride; tail only (n4 = 0) and n4 = 1 with tails 0 / 1 / 3 -- tail_only; m = 1 (FIRST, TURN, LAST only) -- one_pair,
    tail_only; count == capacity with first = 4 (the ring wraps inside both loops) -- full_ring.
  loss_partial_kernel: second trip over pixels (crop: 446,464 pixels) and over deltas (n2 = 300,007); strided, channels-last,
    zero-stride and 3-D views; one-hot at 0, 255, 256, 262143, 262144, N - 1.  loss_bwd_delta_kernel: second trip (more than
    524,288 elements) -- big_delta.  loss_bwd_flow_kernel: second trip (more than 524,288 pixels) -- bwd_second_trip
    (525,312 pixels).
  box_fwd_kernel, deltas_*_kernel, pm1_pair_*_kernel: second trip at (2,3,300,301) = 541,800; box_bwd_kernel: at
    (2,3,420,420), 529,200 per sample.
"""
import functools
import math
from collections import namedtuple

import numpy as np
import torch

from tests.fenced import TINY, U, gamma
from tests.gates import dense_stride

F32, F64 = torch.float32, torch.float64
RED_THREADS_TOTAL = 1024 * 256       # threads of loss_partial_kernel, of lbfgs_pair_kernel and lbfgs_step_kernel
EW_THREADS_TOTAL = 2048 * 256        # the cap of ew_blocks
DOT_DEPTH = 20
MUTANTS = ("drop_rows_ge_64", "lower_triangle", "ring_off_by_one", "drop_tail", "drop_second_trip", "sel_one_at_tie",
           "exclusive_mask")

# The kernel's own error against float64 on an MI355X, next to the emulation's (rel_l2 of d, n = 4099, worst of both kinds;
# filled from the junit properties of tests/test_lbfgs_f64_gpu.py::test_gram[rows_to_128-*] and [workload_cap-*]).
KERNEL_MEASURED = {
    # m: (kernel, emulation) -- equal to every printed digit: the emulation follows the kernel's order rounding for rounding
    1: (7.91e-08, 7.91e-08),
    6: (1.43e-07, 1.43e-07),
    63: (2.89e-07, 2.89e-07),
    64: (2.98e-07, 2.98e-07),
    65: (3.02e-07, 3.02e-07),
    100: (3.71e-07, 3.71e-07),
    128: (4.20e-07, 4.20e-07),
}


def rel_l2(a, b):
    a, b = torch.as_tensor(a).double(), torch.as_tensor(b).double()
    n = float(b.norm())
    return float((a - b).norm()) / n if n > 0 else float((a - b).norm())


# =========================================================================== L-BFGS
GramCase = namedtuple("GramCase", "name cap n feeds rejects")
GRAM_CASES = [
    GramCase("rows_to_128", 128, 4099, 140, (0, 5, 64, 130)),
    GramCase("workload_cap", 100, 4099, 130, ()),
    GramCase("second_row_edge_64", 64, 1031, 80, ()),
    GramCase("second_row_edge_65", 65, 1031, 80, ()),
    GramCase("smallest_n4", 1, 4, 4, ()),
    GramCase("smallest_n5", 1, 5, 4, ()),
    GramCase("smallest_n8", 1, 8, 4, ()),
    GramCase("block_edges_2048", 5, 2048, 8, ()),
    GramCase("block_edges_3072", 5, 3072, 8, ()),
    GramCase("many_blocks", 3, 600001, 6, ()),
    # rows_to_128 has kept 127 pairs when its feed 130 is rejected (three earlier rejections), one short of a full ring:
    GramCase("reject_on_full", 5, 1031, 10, (7,)),
]
KINDS = ("indep", "corr")
T_STEP = 0.75


def gram_blocks(ld):
    return (ld // 4 + 511) // 512


def history(kind, n, feeds, rejects=(), seed=13):
    """The candidates [(s, y)] in fp32; a rejected one has y negated (y.s < 0)."""
    gen = torch.Generator().manual_seed(seed + n)
    out, s = [], None
    A = torch.linspace(1, 100, n)
    for k in range(feeds):
        z = torch.randn(n, generator=gen)
        if kind == "indep":
            s = z
            y = s + 0.3 * torch.randn(n, generator=gen)
        else:
            s = z if s is None else 0.8 * s + 0.6 * z
            y = A * s
        if float(y.double() @ s.double()) <= 0:     # a tiny n can draw a pair with negative curvature: mirror it
            y = -y
        out.append((s.clone(), -y if k in rejects else y))
    return out


def feed_inputs(case, kind):
    """[(grad, g_prev, d)] of every update, each [ld] fp32 with zero pads, and grad0: what the test hands the kernel.  The
    kernel forms y = grad - g_prev and s = t d itself; g_prev of a feed is the grad of the one before."""
    ld = (case.n + 3) // 4 * 4
    gen = torch.Generator().manual_seed(7 + case.n)
    g_prev = torch.zeros(ld)
    g_prev[:case.n] = torch.randn(case.n, generator=gen)
    out = []
    for s, y in history(kind, case.n, case.feeds, case.rejects):
        d, grad = torch.zeros(ld), torch.zeros(ld)
        d[:case.n] = s / T_STEP
        grad[:case.n] = g_prev[:case.n] + y
        out.append((grad, g_prev, d))
        g_prev = grad
    return out


def two_loop_f64(g, kept, H):
    """torch.optim.LBFGS's direction on the kept pairs [(s, y)] oldest first, float64; also (al, be) oldest first."""
    kept = [(s_i.numpy(), y_i.numpy()) for s_i, y_i in kept]          # (numpy: a quarter of torch's cost per small vector)
    q = -g.numpy()
    al = []
    for s_i, y_i in reversed(kept):
        a = (s_i @ q) / (y_i @ s_i)
        al.append(a)
        q = q - a * y_i
    al = al[::-1]
    r = q * H
    be = []
    for (s_i, y_i), a in zip(kept, al):
        b = (y_i @ r) / (y_i @ s_i)
        be.append(b)
        r = r + (a - b) * s_i
    return torch.from_numpy(r), np.array(al, dtype=np.float64), np.array(be, dtype=np.float64)


def substitute(SYl, YYl, Sg, Yg, H, drop_ge_64=False):
    """gram_coeff_kernel's two substitutions in float64 on the live-ordered matrices: (cg, cS[m], cY[m]) in float64.
    R = upper triangle of SYl.  drop_ge_64: the mutant that never updates the second lane-row (rows 64 .. 127)."""
    m = len(Sg)
    G = np.triu(SYl)
    r = -np.array(Sg, dtype=np.float64)
    al = np.zeros(m)
    for i in range(m - 1, -1, -1):
        al[i] = r[i] * (1.0 / G[i, i])
        upd = G[:i, i] * al[i]
        if drop_ge_64:
            upd[64:] = 0
        r[:i] -= upd
    a = H * (-np.array(Yg, dtype=np.float64) - YYl @ al)
    de = np.zeros(m)
    for i in range(m):
        de[i] = al[i] - a[i] * (1.0 / G[i, i])
        upd = G[i, i + 1:] * de[i]
        if drop_ge_64:
            upd[max(0, 64 - (i + 1)):] = 0
        a[i + 1:] += upd
    return -H, de, -H * al


def fma32(c, a, x):
    """fp32 fma(c, a, x) for an fp32 scalar c: the product of two fp32 numbers is exact in float64"""
    return (float(c) * a.double() + x.double()).float()


class GramEmu:
    """lbfgs_gram.hip on the CPU: fp32 inner products in the kernel's order, the ring and the matrices of gram_coeff_kernel,
    float64 substitutions, fp32 FMA assembly newest pair first.  mutant: one of MUTANTS or None.  dots: "kernel" or "matvec"
    (torch's own fp32 matrix-vector product: a second realisation of the same roundings)."""

    def __init__(self, cap, n, mutant=None, dots="kernel"):
        self.cap, self.rows, self.n = cap, cap + 1, n
        self.ld = (n + 3) // 4 * 4
        self.nblk = gram_blocks(self.ld)
        self.L = self.nblk * 2048
        self.S, self.Y = torch.zeros(self.rows, self.L), torch.zeros(self.rows, self.L)
        self.SY, self.YY = np.zeros((self.rows, self.rows)), np.zeros((self.rows, self.rows))
        self.first = self.count = self.accepted = 0
        self.H = np.float32(1.0)
        self.ys = self.yy = np.float32(0.0)
        self.mutant, self.dots = mutant, dots
        self.seen = set()

    def ring(self, k):
        r = self.first + k
        if r >= self.rows:
            r -= self.rows
            self.seen.add("wrap")
            if self.mutant == "ring_off_by_one":
                r += 1
        return r

    def _dot(self, A, b):
        """[k] float64: the inner products of the rows of A [k][L] with b [L]"""
        if self.dots == "matvec":
            cols = [A[:, i * 2048:(i + 1) * 2048] @ b[i * 2048:(i + 1) * 2048] for i in range(self.nblk)]
            return torch.stack(cols, 1).double().sum(1).numpy()
        k = A.shape[0]
        A5, b5 = A.view(k, self.nblk, 2, 256, 4), b.view(self.nblk, 2, 256, 4)        # float64 already (update)
        acc = torch.zeros(k, self.nblk, 256, dtype=F64)
        for h in (0, 1):                # dot4(second group, dot4(first group, 0)): a chain of 8 fused multiply-adds; the
            for j in range(4):          # product of two fp32 numbers is exact in float64, the sum is rounded to fp32
                acc = (A5[:, :, h, :, j] * b5[:, h, :, j] + acc).float().double()
        acc = acc.float()
        w = acc.view(k, self.nblk, 4, 64)
        while w.shape[-1] > 1:
            w = w[..., 0::2] + w[..., 1::2]
        w = w[..., 0]
        v = ((w[..., 0] + w[..., 1]) + w[..., 2]) + w[..., 3]          # [k][nblk]
        if self.nblk > 64:
            self.seen.add("reduce_second_trip")
            if self.mutant == "drop_second_trip":
                v = v[:, :64]
        return v.double().sum(1).numpy()

    def update(self, g, g_prev, d, t=T_STEP):
        pad = lambda x: torch.cat([x, torch.zeros(self.L - x.numel())])   # noqa: E731
        g, y, s = pad(g), pad(g - g_prev), pad(d * np.float32(t))
        c = (self.first + self.count) % self.rows
        self.S[c], self.Y[c] = s, y
        live = [self.ring(k) for k in range(self.count)] + [c]
        Sl, Yl = self.S[live], self.Y[live]
        if self.dots == "kernel":
            Sl, Yl, g, y = Sl.double(), Yl.double(), g.double(), y.double()
        red = np.zeros((self.rows, 4))
        red[live, 0], red[live, 1] = self._dot(Sl, g), self._dot(Sl, y)
        red[live, 2], red[live, 3] = self._dot(Yl, g), self._dot(Yl, y)
        ys, yy = red[c, 1], red[c, 3]
        self.accepted = int(float(np.float32(ys)) > 1e-10)
        if self.accepted:
            for r in live[:-1]:
                self.SY[r, c] = red[r, 1]
                self.YY[r, c] = self.YY[c, r] = red[r, 3]
            self.SY[c, c], self.YY[c, c] = ys, yy
            if self.count == self.cap:
                self.first = (self.first + 1) % self.rows
            else:
                self.count += 1
            self.H = np.float32(ys) / np.float32(yy)
        self.ys, self.yy = np.float32(ys), np.float32(yy)
        self.red = red
        self.seen.add("m%d" % self.count)
        self.seen.add("accepted" if self.accepted else "rejected_at_%s" % ("empty" if self.count == 0 else
                                                                            "full" if self.count == self.cap else "partial"))
        if self.first:
            self.seen.add("first_nonzero")
        return c

    def coefficients(self):
        """(cg, cS, cY) as the kernel stores them: fp32, cS / cY in live order (oldest first)"""
        m = self.count
        if m == 0:
            return -self.H, np.zeros(0, np.float32), np.zeros(0, np.float32)
        idx = [self.ring(k) for k in range(m)]
        SYl = self.SY[np.ix_(idx, idx)]
        if self.mutant == "lower_triangle":
            SYl = SYl.T
        if m > 64:
            self.seen.add("second_lane_row")
        self.seen.add("prefetch_rem%d" % (m % 4))
        self.seen.add("staged%d" % ((m * m + 1023) // 1024))
        cg, cS, cY = substitute(SYl, self.YY[np.ix_(idx, idx)], self.red[idx, 0], self.red[idx, 2], float(self.H),
                                self.mutant == "drop_rows_ge_64")
        return np.float32(cg), cS.astype(np.float32), cY.astype(np.float32)

    def direction(self, g):
        cg, cS, cY = self.coefficients()
        x = (g * cg)[:self.ld]
        for k in range(self.count - 1, -1, -1):
            r = self.ring(k)
            x = fma32(cY[k], self.Y[r, :self.ld], x)
            x = fma32(cS[k], self.S[r, :self.ld], x)
        return x, (cg, cS, cY)


class RefBook:
    """The reference's bookkeeping: the pairs torch.optim.LBFGS would keep, in float64"""

    def __init__(self, cap):
        self.cap, self.kept, self.H, self.first = cap, [], 1.0, 0

    def update(self, s, y):
        ys = float(y @ s)
        accepted = ys > 1e-10
        if accepted:
            if len(self.kept) == self.cap:
                self.first = (self.first + 1) % (self.cap + 1)
            self.kept = (self.kept + [(s, y)])[-self.cap:]
            self.H = float(np.float32(ys) / np.float32(float(y @ y)))   # H as fp32(ys) / fp32(yy) of exact sums: within 3u
        return accepted, ys, float(y @ y)


def coefficient_eps(c64, realisations):
    """eps_k of the docstring for the concatenated coefficients (cg, cS.., cY..)"""
    errs = np.stack([np.abs(np.asarray(c, dtype=np.float64) - c64) for c in realisations])
    worst = errs.max(0)
    rms = math.sqrt(float((errs ** 2).mean()))
    return np.maximum(np.maximum(worst, rms), U * np.abs(c64))


def elem_bound(m, g, Sm, Ym, c64, eps):
    """The elementwise bound of d from the float64 coefficients c64 = (cg, cS[m], cY[m]) and eps; g [n], Sm / Ym [m][n]"""
    cg, cS, cY = c64[0], c64[1:1 + m], c64[1 + m:]
    P = abs(cg) * g.abs()
    E = eps[0] * g.abs()
    if m:
        aS, aY = Sm.abs().T, Ym.abs().T
        P = P + aS @ torch.from_numpy(np.abs(cS)) + aY @ torch.from_numpy(np.abs(cY))
        E = E + aS @ torch.from_numpy(eps[1:1 + m]) + aY @ torch.from_numpy(eps[1 + m:])
    return gamma(2 * m + 3) * P + 3 * E + (2 * m + 3) * TINY


GramStep = namedtuple("GramStep", "feed crow header H accepted ys64 yy64 ys_abs yy_abs s32 y32 m d64 dE bound c64 cE emu")


@functools.lru_cache(maxsize=None)
def gram_trajectory(case, kind, mutant=None):
    """Per feed: the reference's header and H, the candidate pair as torch forms it, d64, the emulation's d and the
    elementwise bound.  With a mutant only the emulation changes.  Returns (steps, classes the emulation reached)."""
    n = case.n
    emu, emu2, book = GramEmu(case.cap, n, mutant), GramEmu(case.cap, n, None, "matvec"), RefBook(case.cap)
    steps = []
    for feed, (grad, g_prev, d) in enumerate(feed_inputs(case, kind)):
        s32, y32 = (d * np.float32(T_STEP))[:n], (grad - g_prev)[:n]
        accepted, ys64, yy64 = book.update(s32.double(), y32.double())
        crow = emu.update(grad, g_prev, d)
        emu2.update(grad, g_prev, d)
        dE, cE = emu.direction(torch.cat([grad, torch.zeros(emu.L - grad.numel())]))
        cE2 = emu2.coefficients()
        g64 = grad[:n].double()
        d64, _, _ = two_loop_f64(g64, book.kept, book.H)
        m = len(book.kept)
        if m:
            Sm, Ym = torch.stack([p[0] for p in book.kept]), torch.stack([p[1] for p in book.kept])
            SY, YY = (Sm @ Ym.T).numpy(), (Ym @ Ym.T).numpy()
            c64 = np.concatenate([np.ravel(x) for x in substitute(SY, YY, (Sm @ g64).numpy(), (Ym @ g64).numpy(), book.H)])
        else:
            Sm = Ym = None
            c64 = np.array([-book.H])
        eps = coefficient_eps(c64, [np.concatenate([np.ravel(x) for x in c]) for c in (cE, cE2)]) if mutant is None else None
        bound = elem_bound(m, g64, Sm, Ym, c64, eps) if mutant is None else None
        steps.append(GramStep(feed, crow, (book.first, m, int(accepted), case.cap + 1), book.H, accepted, ys64, yy64,
                              float((y32.double() * s32.double()).abs().sum()), float((y32.double() ** 2).sum()),
                              s32, y32, m, d64, dE[:n], bound, c64, cE,
                              ((emu.first, emu.count, emu.accepted, emu.rows), float(emu.H), float(emu.ys), float(emu.yy))))
    return steps, frozenset(emu.seen)


def gram_census(case):
    """Classes of gram_pass_kernel / gram_direction_kernel that the sizes alone decide"""
    ld4 = (case.n + 3) // 4
    nblk = gram_blocks(ld4 * 4)
    seen = {"nblk%d" % nblk}
    last = ld4 - (nblk - 1) * 512       # float4 groups of the last workgroup
    seen.add("last_block_full" if last == 512 else "last_block_ok1_false" if last <= 256 else "last_block_ragged")
    if ld4 == 1:
        seen.add("ld4_is_1")
    if ld4 * 4 != case.n:
        seen.add("padded")
    if nblk > 64:
        seen.add("reduce_second_trip")
    if nblk > 256:
        seen.add("final_second_trip")
    return seen


def stat_ratio(got, want, emu):
    """the statistical gate's ratio; as in tests/gates.py, fewer than 256 elements are no statistic and are left to the
    elementwise gate (8 elements with a typical error of u each miss 3 u in the norm one time in ten)"""
    if torch.as_tensor(want).numel() < 256:
        return 0.0
    return rel_l2(got, want) / (3 * max(rel_l2(emu, want), U))


def worst_ratio(got, want, bound):
    """max |got - want| / bound over every element.  A NaN -- in got, or of inf - inf -- counts as infinite: Python's
    max(0.0, nan) is 0.0 and nan.max() depends on the position, so a gate folded with max() would pass on one."""
    r = (torch.as_tensor(got).double() - want).abs() / bound
    return float(torch.nan_to_num(r, nan=float("inf")).max())


def fold(worst, key, value):
    """asserts the ratio where it is computed (NaN <= 1 is false), then keeps the larger one for the record"""
    assert value <= 1, (key, value)
    worst[key] = max(worst.get(key, 0.0), value)


def elem_ratio(got, want, bound):
    return worst_ratio(got, want, bound)


# --------------------------------------------------------------------------- two-loop form
LoopCase = namedtuple("LoopCase", "name n count capacity first")
LOOP_CASES = [LoopCase("grid_stride", 1049779, 3, 4, 2)] + \
    [LoopCase("tail_only_n%d_m%d" % (n, m), n, m, 3, 2) for n in (1, 2, 3) for m in (1, 2)] + \
    [LoopCase("tail_only_n%d" % n, n, 2, 3, 2) for n in (4, 5, 7)] + \
    [LoopCase("one_pair", 4099, 1, 3, 1), LoopCase("full_ring", 4099, 9, 9, 4)]
PAIR_NS = (1049779, 1, 2, 3, 4, 5, 7, 4099)


def loop_inputs(case):
    """g [n], the pairs oldest first [(s, y)], ro (fp32 1 / y.s as pcfa_lbfgs_pair forms it) and H, all fp32"""
    gen = torch.Generator().manual_seed(3 + case.n)
    g = torch.randn(case.n, generator=gen)
    pairs = history("indep", case.n, case.count, seed=29)
    ro = [np.float32(1.0) / np.float32(float(y.double() @ s.double())) for s, y in pairs]
    s, y = pairs[-1]
    H = np.float32(float(y.double() @ s.double())) / np.float32(float(y.double() @ y.double()))
    return g, pairs, ro, H


def two_loop_f32(g, pairs, ro, H, mutant=None, exact_dots=False):
    """lbfgs_step_kernel's sequence in torch fp32: (d, al, be).  exact_dots: every dot product summed in float64 and
    rounded once (the second realisation)."""
    n = g.numel()
    n_eff = n
    if mutant == "drop_tail":
        n_eff = n - n % 4
    if mutant == "drop_second_trip":
        n_eff = min(n, 4 * RED_THREADS_TOTAL)
    a_ = slice(0, n_eff)

    def dot(a, b):
        if exact_dots:
            return np.float32(float(a[a_].double() @ b[a_].double()))
        return np.float32(float((a[a_] * b[a_]).sum()))          # fp32 products, torch's cascaded fp32 sum
    x = torch.zeros(n)
    x[a_] = -g[a_]
    m = len(pairs)
    al, be = [None] * m, [None] * m
    for i in range(m - 1, -1, -1):
        s_i, y_i = pairs[i]
        al[i] = dot(s_i, x) * ro[i]
        x[a_] = fma32(-al[i], y_i[a_], x[a_])
    x[a_] = x[a_] * H
    for i in range(m):
        s_i, y_i = pairs[i]
        be[i] = dot(y_i, x) * ro[i]
        x[a_] = fma32(al[i] - be[i], s_i[a_], x[a_])
    return x, np.array(al, dtype=np.float32), np.array(be, dtype=np.float32)


def loop_coefficients(al, be, H):
    al, be = np.asarray(al, dtype=np.float64), np.asarray(be, dtype=np.float64)
    return np.concatenate([[-float(H)], al - be, -float(H) * al])


@functools.lru_cache(maxsize=4)
def loop_reference(case, mutant=None):
    """(d64, dE, bound, inputs)"""
    g, pairs, ro, H = loop_inputs(case)
    kept = [(s.double(), y.double()) for s, y in pairs]
    g64 = g.double()
    # the reference takes the kernel's own ro and H (inputs of pcfa_lbfgs_direction), not 1 / y.s of the exact sums
    q, al64 = -g64, [None] * len(kept)
    for i in range(len(kept) - 1, -1, -1):
        al64[i] = float(kept[i][0] @ q) * float(ro[i])
        q = q - al64[i] * kept[i][1]
    r, be64 = q * float(H), [None] * len(kept)
    for i in range(len(kept)):
        be64[i] = float(kept[i][1] @ r) * float(ro[i])
        r = r + (al64[i] - be64[i]) * kept[i][0]
    dE, alE, beE = two_loop_f32(g, pairs, ro, H, mutant)
    _, al2, be2 = two_loop_f32(g, pairs, ro, H, None, True)
    c64 = loop_coefficients(al64, be64, H)
    eps = coefficient_eps(c64, [loop_coefficients(alE, beE, H), loop_coefficients(al2, be2, H)])
    Sm, Ym = torch.stack([p[0] for p in kept]), torch.stack([p[1] for p in kept])
    return r, dE, elem_bound(len(kept), g64, Sm, Ym, c64, eps), (g, pairs, ro, H)


def loop_census(case):
    seen = set()
    n4 = case.n // 4
    seen.add("n4_%s" % ("zero" if n4 == 0 else "second_trip" if n4 > RED_THREADS_TOTAL else "one_trip"))
    seen.add("tail%d" % (case.n % 4))
    seen.add("m1" if case.count == 1 else "m_many")
    if case.count == case.capacity:
        seen.add("full_ring")
    if case.first + case.count > case.capacity:
        seen.add("ring_wraps")
    return seen


def pair_depth(n):
    """the longest chain of additions of y.s / y.y: 4 products per trip of the grid-stride loop, the scalar tail term that
    threads 0 .. n % 4 - 1 of block 0 add after their trips, the two blocks' 6 + 4 each, the final kernel's 4 partials per
    thread, and the product's own rounding"""
    return 4 * max(1, -(-(n // 4) // RED_THREADS_TOTAL)) + (1 if n % 4 else 0) + 25


def pair_inputs(n, seed=5):
    gen = torch.Generator().manual_seed(seed + n)
    g, g_prev, d = (torch.randn(n, generator=gen) for _ in range(3))
    return g, g_prev, d


ONE_HOT_AT = (0, 3, 4, 1048575, 1048576, -1)


# =========================================================================== reductions of attack_math.hip
TERM_R = {"epe": 3, "sq": 4, "pt": 2, "pp": 2, "tt": 2, "d": 1}


def red_depth(N):
    return -(-N // RED_THREADS_TOTAL) + 24


def strided_sum32(terms, mutant=None):
    """loss_partial_kernel + loss_final_kernel on one sum: fp32, in the kernel's order"""
    t = terms.reshape(-1).float()
    N = t.numel()
    T = max(1, -(-N // RED_THREADS_TOTAL))
    t = torch.cat([t, torch.zeros(T * RED_THREADS_TOTAL - N)]).view(T, 1024, 4, 64)
    if mutant == "drop_second_trip":
        T = 1
    acc = torch.zeros(1024, 4, 64)
    for k in range(T):
        acc = acc + t[k]

    def block(w):                       # [.., 4, 64] -> [..]
        while w.shape[-1] > 1:
            h = w.shape[-1] // 2
            w = w[..., :h] + w[..., h:]     # __shfl_down by h
        w = w[..., 0]
        return ((w[..., 0] + w[..., 1]) + w[..., 2]) + w[..., 3]
    part = block(acc)                   # [1024]
    p = part.view(4, 4, 64)             # partial[t + k * 256]
    v = torch.zeros(4, 64)
    for k in range(4):
        v = v + p[k]
    return np.float32(float(block(v)))


class Operand:
    """A flow operand as the kernel sees it: base (1-D fp32, NaN where the view does not reach), size [B,2,H,W], stride, offset"""

    def __init__(self, x, layout="dense"):
        x4 = x if x.dim() == 4 else x.unsqueeze(0)
        B, C, H, W = x4.shape
        self.dims3 = x.dim() == 3
        if layout == "dense":
            base_shape, stride, off = (B, C, H, W), dense_stride((B, C, H, W)), 0
        elif layout == "crop":           # rows 2 .. H + 2 of a map with 4 more rows
            base_shape, stride, off = (B, C, H + 4, W), dense_stride((B, C, H + 4, W)), 2 * W
        elif layout == "channels_last":
            base_shape, stride, off = (B, H, W, C), (H * W * C, 1, W * C, C), 0
        elif layout == "expanded":       # x is [1,2,H,W], seen B = 3 times through a zero stride
            base_shape, stride, off = (1, C, H, W), (0,) + dense_stride((C, H, W)), 0
            B = 3
        else:
            raise ValueError(layout)
        self.layout = layout
        self.base = torch.full((int(np.prod(base_shape)),), float("nan"))
        if layout == "expanded":
            self.base.view(C, H, W).copy_(x4[0])
        else:
            self.base.as_strided(tuple(x4.shape), stride, off).copy_(x4)
        self.size, self.stride, self.off = (B, C, H, W), tuple(stride), off

    def view(self):
        v = self.base.as_strided(self.size, self.stride, self.off)
        return v[0] if self.dims3 else v


LossCase = namedtuple("LossCase", "name shape pred_layout target_layout n1 n2 regime equal_pixels")
LOSS_CASES = [
    LossCase("one_pixel", (1, 2, 1, 1), "dense", "dense", 7, 9, "above", 0),
    LossCase("small", (2, 2, 3, 5), "dense", "dense", 30, 30, "above", 3),
    LossCase("small_below", (2, 2, 3, 5), "dense", "dense", 30, 30, "below", 0),
    LossCase("flow3d", (2, 7, 9), "dense", "dense", 64, 32, "above", 2),
    LossCase("crop_436", (1, 2, 436, 1024), "crop", "dense", 1000, 1000, "above", 5),
    LossCase("channels_last", (3, 2, 300, 301), "channels_last", "channels_last", 513, 255, "above", 0),
    LossCase("expanded_target", (3, 2, 17, 19), "dense", "expanded", 100, 28, "below", 0),
    LossCase("long_delta2", (2, 2, 3, 5), "dense", "dense", 3, 300007, "above", 0),
    LossCase("big_delta", (2, 2, 3, 5), "dense", "dense", EW_THREADS_TOTAL + 5, 3, "above", 0),
    LossCase("tie", (2, 2, 3, 5), "dense", "dense", 512, 1536, "tie", 0),
    # no shape above has more than 524,288 pixels: the second trip of loss_bwd_flow_kernel's loop
    LossCase("bwd_second_trip", (1, 2, 513, 1024), "dense", "dense", 16, 16, "above", 1),
]
F_TYPES = ("aee", "mse", "cosim")
MU = 5e5
GRAD_LOSSES = (1.0, 0.37)
DELTA_BOUND = {"above": 0.005, "below": 0.05, "tie": 0.5}


def msq_bound(n1, n2, sum_sq):
    """B_msq: the bound of the mean square (v5 + v6) / ndelta"""
    return gamma(red_depth(max(n1, n2)) + 2 + TERM_R["d"]) * sum_sq / (n1 + n2)


@functools.lru_cache(maxsize=None)
def loss_case(name):
    """(pred Operand, target Operand, d1, d2, delta_bound) of the case"""
    case = next(c for c in LOSS_CASES if c.name == name)
    gen = torch.Generator().manual_seed(len(name) * 131 + case.n2)
    shape = case.shape
    pred = 3 * torch.randn(*shape, generator=gen)
    tshape = (1,) + shape[1:] if case.target_layout == "expanded" else shape
    target = 3 * torch.randn(*tshape, generator=gen)
    if case.equal_pixels:            # pred == target in both channels: |du| = |dv| = 0, the NaN of the AEE gradient
        flat_p = pred.view(-1, 2, shape[-2] * shape[-1]) if len(shape) == 4 else pred.view(1, 2, -1)
        flat_t = target.view(-1, 2, shape[-2] * shape[-1]) if len(shape) == 4 else target.view(1, 2, -1)
        idx = torch.randperm(flat_p.shape[-1], generator=gen)[:case.equal_pixels]
        flat_p[0, :, idx] = flat_t[0, :, idx]
        flat_p[0, :, 0] = flat_t[0, :, 0]
    if case.regime == "tie":
        d1, d2 = torch.full((case.n1,), 0.5), torch.full((case.n2,), 0.5)
        d2[::2] = -0.5
    else:
        d1, d2 = 0.02 * torch.randn(case.n1, generator=gen), 0.02 * torch.randn(case.n2, generator=gen)
    bound = DELTA_BOUND[case.regime]
    ssq = float((d1.double() ** 2).sum() + (d2.double() ** 2).sum())
    msq64, b2 = ssq / (case.n1 + case.n2), float(np.float32(bound * bound))
    if case.regime == "tie":
        assert msq64 == b2 == 0.25
    else:        # a condition on the inputs, not a measurement: the case decides the regime, the rounding cannot
        assert abs(msq64 - b2) >= 1000 * msq_bound(case.n1, case.n2, ssq), (name, msq64, b2)
        assert (msq64 > b2) == (case.regime == "above")
    return Operand(pred, case.pred_layout), Operand(target, case.target_layout), d1, d2, bound


def loss_terms(p, t, dtype):
    """The five per-pixel terms of loss_partial_kernel from the operand views, in `dtype`, pixel-major"""
    p, t = p.to(dtype), t.to(dtype)
    cd = p.dim() - 3
    pu, pv, tu, tv = p.select(cd, 0), p.select(cd, 1), t.select(cd, 0), t.select(cd, 1)
    du, dv = pu - tu, pv - tv
    sq = du * du + dv * dv
    return {"epe": sq.sqrt(), "sq": sq, "pt": pu * tu + pv * tv, "pp": pu * pu + pv * pv, "tt": tu * tu + tv * tv}


def loss_ref64(oracle_ops, name, f_type, grad_loss=1.0):
    """float64: oracle.ops on double inputs.  (scalars dict, grad_pred, grad_d1, grad_d2)"""
    po, to, d1, d2, bound = loss_case(name)
    p = po.view().double().requires_grad_(True)
    t = to.view().double()
    a, b = d1.double().requires_grad_(True), d2.double().requires_grad_(True)
    loss = oracle_ops.loss_delta_constraint(p, t, a, b, None, bound, MU, f_type)
    gp, ga, gb = torch.autograd.grad(loss, (p, a, b), torch.tensor(float(np.float32(grad_loss)), dtype=F64), allow_unused=True)
    with torch.no_grad():
        sim = float(oracle_ops.get_loss(f_type, p, t))
        msq = float(oracle_ops.two_norm_avg_delta_squared(a, b))
    return {"loss": float(loss.detach()), "sim": sim, "msq": msq, "arg": msq - float(np.float32(bound * bound))}, gp, ga, gb


def loss_bounds(name, f_type):
    """B_sim, B_msq, the relative bounds of pp and tt and the absolute one of pt, and the float64 sums"""
    po, to, d1, d2, bound = loss_case(name)
    T = {k: v.reshape(-1) for k, v in loss_terms(po.view(), to.view(), F64).items()}
    npix = T["epe"].numel()
    D = red_depth(npix)
    S = {k: float(v.sum()) for k, v in T.items()}
    A = {k: float(v.abs().sum()) for k, v in T.items()}
    E = {k: gamma(D + 2 + TERM_R[k]) * A[k] for k in T}
    if f_type == "aee":
        b_sim = E["epe"] / npix
    elif f_type == "mse":
        b_sim = E["sq"] / (2 * npix)
    else:
        val = abs(S["pt"]) / math.sqrt(S["pp"]) * math.sqrt(S["tt"])
        b_sim = math.sqrt(S["tt"] / S["pp"]) * E["pt"] + val * (E["pp"] / S["pp"] / 2 + E["tt"] / S["tt"] / 2 + 5 * U) + \
            U * abs(1 - S["pt"] / math.sqrt(S["pp"]) * math.sqrt(S["tt"]))
    ssq = float((d1.double() ** 2).sum() + (d2.double() ** 2).sum())
    return {"sim": b_sim, "msq": msq_bound(d1.numel(), d2.numel(), ssq), "e_pp": E["pp"] / S["pp"], "e_tt": E["tt"] / S["tt"],
            "E_pt": E["pt"], "sums": S, "abs": A, "npix": npix, "D": D}


def loss_total_bound(bounds, ref, mu=MU):
    return bounds["sim"] + mu * (bounds["msq"] + U * abs(ref["arg"])) + 2 * U * abs(ref["loss"]) + TINY


def loss_fwd_emu(name, f_type, mutant=None):
    """loss_partial_kernel + loss_final_kernel in fp32: the 7 scalars of out_scalars"""
    po, to, d1, d2, bound = loss_case(name)
    T = loss_terms(po.view(), to.view(), F32)
    v = {k: strided_sum32(x, mutant) for k, x in T.items()}
    v5, v6 = strided_sum32(d1 * d1, mutant), strided_sum32(d2 * d2, mutant)
    npix = np.float32(T["epe"].numel())
    if f_type == "aee":
        sim = v["epe"] / npix
    elif f_type == "mse":
        sim = v["sq"] / (np.float32(2) * npix)
    else:
        sim = np.float32(1) - v["pt"] / np.sqrt(v["pp"]) * np.sqrt(v["tt"])
    msq = (v5 + v6) / np.float32(d1.numel() + d2.numel())
    arg = msq - np.float32(bound * bound)
    pen = max(np.float32(0), arg)
    return np.array([sim + np.float32(MU) * pen, sim, msq, v["pt"], v["pp"], v["tt"], arg], dtype=np.float32)


def loss_bwd_emu(name, f_type, grad_loss, scal, mutant=None):
    """loss_bwd_flow_kernel and loss_bwd_delta_kernel in torch fp32 from the forward scalars: (grad_pred [B,2,H,W], gd1, gd2)"""
    po, to, d1, d2, _ = loss_case(name)
    p, t = po.base.as_strided(po.size, po.stride, po.off), to.base.as_strided(to.size, to.stride, to.off)
    pu, pv, tu, tv = p[:, 0], p[:, 1], t[:, 0], t[:, 1]
    npix = pu.numel()
    gl = np.float32(grad_loss)
    f = lambda x: torch.tensor(x, dtype=F32)   # noqa: E731
    if f_type == "aee":
        du, dv = pu - tu, pv - tv
        gs = f(gl / np.float32(npix)) / (2 * (du * du + dv * dv).sqrt())
        gu, gv = gs * (2 * du), gs * (2 * dv)
    elif f_type == "mse":
        g = f(gl / np.float32(2 * npix))
        gu, gv = g * (2 * (pu - tu)), g * (2 * (pv - tv))
    else:
        pt, pp, tt = (np.float32(x) for x in scal[3:6])
        spp, stt = np.sqrt(pp), np.sqrt(tt)
        a, c = f(-gl * stt / spp), f(gl * stt * pt / (np.float32(2) * pp * spp))
        gu, gv = a * tu + c * (2 * pu), a * tv + c * (2 * pv)
    arg = np.float32(scal[6])
    sel = np.float32(1 if arg > 0 else (0.5 if arg == 0 else 0))
    if mutant == "sel_one_at_tie" and arg == 0:
        sel = np.float32(1)
    g = f(gl * np.float32(MU) * sel / np.float32(d1.numel() + d2.numel()))
    return torch.stack([gu, gv], 1), g * (2 * d1), g * (2 * d2)


def flow_grad_bound(name, f_type, gp64, grad_loss):
    """The elementwise bound of grad_pred ([B,2,H,W] or [2,H,W] like gp64); NaN where gp64 is NaN"""
    if f_type == "aee":
        return gamma(8) * gp64.abs() + TINY
    if f_type == "mse":
        return gamma(4) * gp64.abs() + TINY
    po, to, _, _, _ = loss_case(name)
    b = loss_bounds(name, f_type)
    S = b["sums"]
    gl = abs(float(np.float32(grad_loss)))
    a = gl * math.sqrt(S["tt"] / S["pp"])
    c = gl * math.sqrt(S["tt"]) * abs(S["pt"]) / (2 * S["pp"] ** 1.5)
    da = a * (b["e_tt"] / 2 + b["e_pp"] / 2 + 5 * U)
    dc = c * (b["e_tt"] / 2 + 1.5 * b["e_pp"] + 7 * U) + gl * math.sqrt(S["tt"]) / (2 * S["pp"] ** 1.5) * b["E_pt"]
    p, t = po.view().double().abs(), to.view().double().abs()
    return da * t + dc * 2 * p + 3 * U * (a * t + c * 2 * p) + TINY


def loss_census(case):
    seen = set()
    B, H, W = (case.shape[0] if len(case.shape) == 4 else 1), case.shape[-2], case.shape[-1]
    npix = B * H * W
    seen.add("pix_second_trip" if npix > RED_THREADS_TOTAL else "pix_one_trip")
    if npix > EW_THREADS_TOTAL:
        seen.add("bwd_flow_second_trip")
    if max(case.n1, case.n2) > RED_THREADS_TOTAL:
        seen.add("delta_second_trip")
    if max(case.n1, case.n2) > EW_THREADS_TOTAL:
        seen.add("bwd_delta_second_trip")
    if case.n1 != case.n2:
        seen.add("n1_ne_n2")
    seen.update({"pred_" + case.pred_layout, "target_" + case.target_layout, "regime_" + case.regime})
    if len(case.shape) == 3:
        seen.add("flow3d")
    if case.equal_pixels:
        seen.add("aee_nan")
    return seen


RED_ONE_HOT_AT = (0, 255, 256, 262143, 262144, -1)
ONE_HOT_FLOW = (1, 2, 436, 1024)        # 446,464 pixels
ONE_HOT_N = 300007


# =========================================================================== element-wise kernels
EW_SHAPES = ((2, 3, 300, 301), (2, 3, 420, 420), (3, 3, 1, 1), (1, 1, 1, 5))


def ew_census(shape):
    B = shape[0]
    n = int(np.prod(shape[1:]))
    seen = set()
    seen.add("total_second_trip" if B * n > EW_THREADS_TOTAL else "total_one_trip")
    seen.add("sample_second_trip" if n > EW_THREADS_TOTAL else "sample_one_trip")
    return seen


def _grid(gen, shape, lo, hi, den):
    """multiples of 1 / den in [lo, hi]"""
    return torch.randint(int(lo * den), int(hi * den) + 1, shape, generator=gen).float() / den


def _plant(x, values):
    """the first elements of x take `values` in turn (the tiny shapes cannot leave the edges to chance)"""
    f = x.view(-1)
    k = min(f.numel(), len(values))
    f[:k] = torch.tensor(values[:k])
    return x


@functools.lru_cache(maxsize=2)
def clip_inputs(shape, with_delta):
    """image, delta (or None), grad_out: image + delta is a multiple of 1/64 in [-0.5, 1.5], grad_out of 1/256 in [-4, 4]"""
    gen = torch.Generator().manual_seed(shape[-1] + 17 * with_delta)
    if with_delta:
        image, delta = _grid(gen, shape, 0, 1, 64), _grid(gen, (1,) + shape[1:], -0.5, 0.5, 64)
        _plant(delta, [0.0] * 5)
        _plant(image, [0.0, 1.0, 0.5, 1.0, 0.0])
    else:
        image, delta = _plant(_grid(gen, shape, -0.5, 1.5, 64), [0.0, 1.0, -1 / 64, 65 / 64, 0.5]), None
    return image, delta, _grid(gen, shape, -4, 4, 256)


@functools.lru_cache(maxsize=2)
def joint_inputs(shape):
    """nw_delta, images_max, images_min, grad: multiples of 1/64; images_min == images_max on a third of the elements"""
    gen = torch.Generator().manual_seed(shape[-1] + 5)
    imax, imin = _grid(gen, shape, 0, 1, 64), _grid(gen, shape, 0, 1, 64)
    imin = torch.minimum(imin, imax)
    same = torch.randint(0, 3, shape, generator=gen) == 0
    imin[same] = imax[same]
    nd = _grid(gen, shape, -1.5, 1.5, 64)
    _plant(imax, [0.5, 0.5, 0.25, 0.25, 1.0])
    _plant(imin, [0.5, 0.5, 0.25, 0.25, 0.0])
    _plant(nd, [-0.5, 0.5, -0.25, 0.75, 0.5])     # a = 0, 1, 0, 1, 1.5; b = 0, 1, 0, 1, 0
    return nd, imax, imin, _grid(gen, shape, -4, 4, 256)


@functools.lru_cache(maxsize=2)
def cov_inputs(shape, with_delta):
    """image, delta, grad_out with image + delta interior (|x| <= 4), saturated (|x| >= 12) or +-inf; and the class map"""
    gen = torch.Generator().manual_seed(shape[-1] + 3 * with_delta)
    cls = torch.randint(0, 8, shape, generator=gen)          # 0..4 interior, 5..6 saturated, 7 infinite
    sign = torch.randint(0, 2, shape, generator=gen).float() * 2 - 1
    _plant(cls, [0, 5, 7, 6, 7])
    _plant(sign, [1.0, 1.0, 1.0, -1.0, -1.0])
    image = (torch.rand(shape, generator=gen) * 6 - 3)
    image = torch.where(cls >= 5, sign * (14 + 6 * torch.rand(shape, generator=gen)), image)
    image = torch.where(cls == 7, sign * float("inf"), image)
    delta = (torch.rand((1,) + shape[1:], generator=gen) * 2 - 1) if with_delta else None
    return image, delta, torch.randn(shape, generator=gen), cls


def box_k_c(eps, dtype):
    k, c = (1. / 2.) * 1. / (1. - eps), 1. - eps
    return (float(np.float32(k)), float(np.float32(c))) if dtype == F32 else (k, c)


def box_fwd(image, delta, cov, eps, scale, dtype):
    """box_fwd_kernel's formula in `dtype` (float64: the reference, with Python's double constants)"""
    x = image.to(dtype)
    if delta is not None:
        x = x + delta.to(dtype)
    if cov:
        k, c = box_k_c(eps, dtype)
        x = k * (torch.tanh(x) + c)
    x = x.clamp(0., 1.)
    return scale * x if scale != 1. else x


def box_bwd(image, delta, gout, cov, eps, scale, dtype, mutant=None):
    """box_bwd_kernel in `dtype`: (grad_image, grad_delta summed over the batch in index order)"""
    x = image.to(dtype)
    if delta is not None:
        x = x + delta.to(dtype)
    g = gout.to(dtype)
    if scale != 1.:
        g = g * scale
    y, t = x, None
    if cov:
        k, c = box_k_c(eps, dtype)
        t = torch.tanh(x)
        y = k * (t + c)
    inside = (y > 0) & (y < 1) if mutant == "exclusive_mask" else (y >= 0) & (y <= 1)
    g = torch.where(inside, g, torch.zeros_like(g))
    if cov:
        g = (g * k) * (1 - t * t)
    gd = torch.zeros_like(g[0])
    for b in range(g.shape[0]):
        gd = gd + g[b]
    return g, gd.unsqueeze(0)


def deltas_fwd(w, image, cov, eps, dtype):
    x = w.to(dtype)
    if cov:
        k, c = box_k_c(eps, dtype)
        return k * (torch.tanh(x) + c) - image.to(dtype)
    return x.clamp(0., 1.) - image.to(dtype)


def deltas_bwd(w, gd, cov, eps, dtype, mutant=None):
    x, g = w.to(dtype), gd.to(dtype)
    if cov:
        k, _ = box_k_c(eps, dtype)
        t = torch.tanh(x)
        return (g * k) * (1 - t * t)
    inside = (x > 0) & (x < 1) if mutant == "exclusive_mask" else (x >= 0) & (x <= 1)
    return torch.where(inside, g, torch.zeros_like(g))


def joint_fwd(nd, imax, imin, dtype):
    nd, imax, imin = nd.to(dtype), imax.to(dtype), imin.to(dtype)
    up = (nd + imax).clamp(0., 1.) - imax
    return (up + imin).clamp(0., 1.) - imin


def joint_bwd(nd, imax, imin, gd, dtype, mutant=None):
    nd, imax, imin, g = nd.to(dtype), imax.to(dtype), imin.to(dtype), gd.to(dtype)
    a = nd + imax
    b = a.clamp(0., 1.) - imax + imin
    if mutant == "exclusive_mask":
        inside = (a > 0) & (a < 1) & (b > 0) & (b < 1)
    else:
        inside = (a >= 0) & (a <= 1) & (b >= 0) & (b <= 1)
    return torch.where(inside, g, torch.zeros_like(g))


def tanh_error(x):
    """e_t: the largest |tanh32 - tanh64| over the finite inputs x (fp32)"""
    x = x[torch.isfinite(x)]
    return float((torch.tanh(x).double() - torch.tanh(x.double())).abs().max())


def cov_grad_bound(x, g_in, k, g64, e_t):
    """The absolute bound of g k (1 - t^2); g_in = the incoming gradient (x scale), x the fp32 argument of tanh, g64 the
    float64 result.  grad_delta: the sum of the samples' bounds + gamma(B) sum |g64_b| for the B additions."""
    t = torch.tanh(x.double()).abs()
    return (g_in.double().abs() * k) * (6 * e_t * t + 9 * e_t * e_t + 2 * U) + gamma(3) * g64.abs() + TINY


def edge_census(values):
    """how many elements sit exactly on 0 and on 1"""
    return int((values == 0).sum()), int((values == 1).sum())
