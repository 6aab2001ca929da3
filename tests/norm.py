"""Instance norm (csrc/norm_ops.hip: pcfa_instnorm_fwd / _bwd on their three code paths) and the exact streaming kernels
(pcfa_add_relu_fwd, pcfa_relu_bwd, pcfa_relu_bwd2) for the float64 tests: a mirror of the host's plan, the float64
reference, the kernel's own arithmetic on the CPU (`emu`), the inputs with nothing undecided at the ReLU, the case table and
the gates of tests/test_norm_f64_gpu.py and tests/test_norm_host_cpu.py.  No GPU, no ctypes.

Plan.  plan(planes, plane, vec, fused) restates norm_plan and plane_kernel_threads: label `plane256` / `plane1024` (one
launch, one workgroup of 256 / 1024 threads x 7 float4 pieces per plane: vec, planes >= 96, plane <= 7168 / 28672),
`two_vec` / `two_scalar` (stats + apply over (chunks, planes) workgroups of 256 threads); vec = plane % 4 == 0 and every
operand 16-B aligned.  The workspace is planes * chunks * 16 bytes on every path.

Reference (float64, from the fp32 input): mu = mean(x), var = mean((x - mu)^2) (two passes, biased), r = 1 / sqrt(var + eps),
xhat = (x - mu) r, y = relu?(xhat); g = dy [xhat > 0] under ReLU, else dy; m1 = mean(g), m2 = mean(g xhat),
dx = r (g - m1 - xhat m2).

Emulation.  The kernel's arithmetic in the kernel's order: the sums of x and x x (forward) or g and fp32(g xhat) (backward)
in fp64 -- per thread over its pieces in index order, the 64 lanes by the shuffle tree, the waves, then the chunks in index
order (kernel_sum) --, mu = S1 / n, var = max(S2 / n - mu^2, 0), mean, rstd = 1 / sqrt(var + eps), m1, m2 rounded to
fp32, then xh = (x - mean) rstd, y = max(xh, 0) and dx = rstd ((g - m1) - xh m2) in fp32.

Bounds (u = 2^-24, e = 2^-53, gamma(k) = k u / (1 - k u), g64(k) = k e / (1 - k e), TINY = 2^-126; A1 = mean |x|,
A2 = mean x^2 = mu^2 + var, so A1 <= sqrt(A2) and |mu| A1 <= A2).  d = the number of additions an addend passes through:
pieces per thread + 6 (lanes) + waves + chunks (plan.depth); any summation order of that depth errs by at most
g64(d) sum |addend| (Higham 4.2).
  mean      S1 / n: |mu_k - mu| <= g64(d + 1) A1 =: dmu.  Stored in fp32: |mean - mu| <= u |mu| + dmu.
  rstd      x x is exact in fp64 (48 bits).  |S2 / n - A2| <= g64(d + 1) A2; mu_k^2: 2 |mu| dmu + e A2; the subtraction: e A2.
            |var_k - var| <= 3 g64(d + 2) A2 =: dvar (the clamp at 0 moves var_k towards var).  var + eps, sqrt, the
            division: 3 e.  rho64 = dvar / (2 (var + eps)) + 4 e is rstd's relative error before its rounding to fp32 (u):
            the fp64 cancellation term, 2^-53 (mu^2 + var) / (var + eps) times the summation depth.  The inputs are asserted
            to have dvar / (var + eps) <= 2^-16 on every plane: second-order terms (3 u rho64, 3 u^2, ..) stay below the
            2^-14 spare on the first-order ones.
  forward   xh = fl(fl(x - mean) rstd).  The subtraction: |mean - mu| + u |x - mean|; the product: u; rstd: u + rho64.
            |xh - xhat| <= (1 + 2^-14) [r (u |mu| + dmu) + (3 u + rho64) |xhat|] + TINY =: fb.
            max(., 0) is a contraction: the same bound with or without ReLU.
  m1        g is exact once the mask is decided (below).  |m1_k - m1| <= u |m1| + g64(d + 1) mean |g| =: dm1.
  m2        each term fl(g xh): |g| fb + u |g xhat| (+ TINY, flushed products); the fp64 sum g64(d + 1) mean |g xhat|; its
            rounding u |m2|:  dm2 = (1 + 2^-14) [mean(|g| fb) + (u + g64(d + 1)) mean |g xhat| + u |m2|] + TINY.
  backward  dx = fl(rstd fl(fl(g - m1) - fl(xh m2))) (or the last two fused): with P = |g| + |m1| + |xhat m2| >= |g - m1 -
            xhat m2|, the three inner operations gamma(3) P, rstd and the outer product (2 u + rho64) P, the operands
            dm1 + |m2| fb + (|xhat| + fb) dm2:
            |dx_k - dx| <= (1 + 2^-14) r [dm1 + |m2| fb + (|xhat| + fb) dm2 + (gamma(5) + rho64) P] + 4 TINY =: bb.
The statistical gate is that of tests/gates.py against `emu`: overall, per 32 planes and per data class.

Nothing undecided at the ReLU.  [xhat > 0] is discontinuous, and an element that flips moves m1 and m2 for the whole plane.
inputs() therefore moves every element with |xhat64| < THRESHOLD fb (THRESHOLD = 4: the kernel's xh and xhat64 differ by at
most fb, so both have the sign of xhat64 beyond 1 fb; 4 leaves room for the move itself changing mu and var) to
mu + sign 4 THRESHOLD fb / r, repeats until none is left and asserts that none is left -- a condition on the inputs, not a
measurement.  Exact zeros are kept on purpose where kernel and reference agree on them: constant planes (every partial sum
k c is exact in fp64: 24 + 18 bits, so mu = c = mean exactly and xh = xhat = 0) and the symmetric planes of +a / -a pairs and
zeros (partial sums are multiples of a: mu = 0 exactly, and xh = xhat = 0 at the zeros).  Both mask them.

Data classes, one per plane and mixed inside a tensor (neighbours must not influence one another): `normal` N(0.4, 1.7);
`bigmean` |mu| / sigma = 10^3 (what the fp64 accumulation is for); `smallsigma` sigma = 10^-4 << sqrt(eps); `constant`;
`symmetric`; `outlier` one element at 10^4 sigma; `huge` magnitude 10^18 (x x overflows fp32, not fp64).  With eps = 0 the
constant planes (class constant, symmetric planes of fewer than 3 elements, one-element planes) are left out: they are drawn
`normal`, and the one-element case is not run.

Kernel by kernel: instnorm_plane_kernel<256,7,.> -- 96x1x4, 96x2x6 (n4 = 1, 3), 97x1x7164, 96x56x128 (7168, full);
instnorm_plane_kernel<1024,7,.> -- 96x1x7172, 96x7x1028, 96x112x256 (28672, full); instnorm_stats_kernel<false/true> and
instnorm_apply_kernel<false/true>, vec -- 96x67x428 (28676: 8 chunks, last 3560), 95x4x8, 2x7x1756, 2x1x262148 (64 chunks),
and the two PCFA_INSTNORM_FUSED=0 cases; scalar -- 2x5x2459, 3x1x4097, 1x1x262147, 3x1x1, 5x7x9 and the misaligned
cases; add_relu_kernel, relu_bwd_kernel, relu_bwd2_kernel -- exact_operands(n) for n in EXACT_N, aligned and with each
operand misaligned in turn; the last n makes the grid-stride loops of relu_bwd_kernel, relu_bwd2_kernel (2048 blocks) and of
add_relu_kernel's scalar form wrap -- its float4 loop (8192 blocks) would need more than 8.4 M floats and wraps in no test.
"""
import functools
import math
import types

import torch
import torch.nn.functional as Fn

from tests.fenced import TINY, U, gamma
from tests.gates import gates as _gates

F32, F64 = torch.float32, torch.float64
E64 = 2.0 ** -53
SPARE = 1 + 2.0 ** -14
THRESHOLD = 4.0
EPS = 1e-5
CLASSES = ("normal", "bigmean", "smallsigma", "constant", "symmetric", "outlier", "huge")
GOUTS = ("random", "zero", "onehot")


def g64(k):
    return k * E64 / (1 - k * E64)


# --------------------------------------------------------------------------- the host's plan
def plan(planes, plane, vec=None, fused=True):
    """norm_plan + plane_kernel_threads: label, chunks, chunk_len, last (chunk's length), nt, w (floats per piece), iters
    (pieces per thread), depth."""
    vec = plane % 4 == 0 if vec is None else (vec and plane % 4 == 0)
    want = max(1, min((2048 + planes - 1) // planes, (plane + 4095) // 4096, 64))
    ln = (-(-plane // want) + 3) & ~3
    chunks = -(-plane // ln)
    p = types.SimpleNamespace(planes=planes, plane=plane, vec=vec, ws_chunks=chunks, ws_bytes=planes * chunks * 16)
    if fused and vec and planes >= 96 and plane <= 4 * 1024 * 7:
        p.nt = 256 if plane <= 4 * 256 * 7 else 1024
        p.label, p.chunks, p.chunk_len, p.last, p.w, p.iters = "plane%d" % p.nt, 1, plane, plane, 4, 7
    else:
        p.label, p.nt, p.chunks, p.chunk_len, p.last = "two_vec" if vec else "two_scalar", 256, chunks, ln, plane - (chunks - 1) * ln
        p.w = 4 if vec else 1
        p.iters = -(-ln // (256 * p.w))
    p.depth = p.iters * p.w + 6 + p.nt // 64 + p.chunks
    return p


def kernel_sum(v, p, mut=None):
    """The fp64 sum of the addends v [planes][plane] in the kernels' order."""
    P, n = v.shape
    v = Fn.pad(v, (0, p.chunks * p.chunk_len - n)).view(P, p.chunks, p.chunk_len)
    stride = p.nt * p.w
    v = Fn.pad(v, (0, p.iters * stride - p.chunk_len)).view(P, p.chunks, p.iters, p.nt, p.w).clone()
    if mut == "drop_tail":                      # the last chunk's last, partial, round of pieces
        full = p.last // stride
        assert p.last % stride, "no ragged tail in this case"
        v[:, p.chunks - 1, full:] = 0
    acc = torch.zeros(P, p.chunks, p.nt, dtype=F64)
    for it in range(p.iters):
        for k in range(p.w):
            acc = acc + v[:, :, it, :, k]
    acc = acc.view(P, p.chunks, p.nt // 64, 64)
    h = 32
    while h:
        acc = acc[..., :h] + acc[..., h:2 * h]
        h //= 2
    acc = acc[..., 0]
    tot = torch.zeros(P, p.chunks, dtype=F64)
    for w in range(p.nt // 64):
        tot = tot + acc[:, :, w]
    res = torch.zeros(P, dtype=F64)
    for c in range(p.chunks):
        res = res + tot[:, c]
    if mut == "surplus_twice":                  # a clamped surplus lane's re-read of the last piece, summed
        assert p.label.startswith("plane")
        res = res + v.reshape(P, -1)[:, :n][:, -4:].sum(1)
    return res


# --------------------------------------------------------------------------- reference and bounds
def stats64(x, eps, p):
    """Per plane [planes][1]: mu, var, r, the bound's constants."""
    x64 = x.double()
    n = x.shape[1]
    mu = x64.mean(1, keepdim=True)
    var = ((x64 - mu) ** 2).mean(1, keepdim=True)
    s = types.SimpleNamespace(mu=mu, var=var, r=1.0 / torch.sqrt(var + float(torch.tensor(eps, dtype=F32))), n=n)
    A1, A2 = x64.abs().mean(1, keepdim=True), (x64 * x64).mean(1, keepdim=True)
    s.dmu = g64(p.depth + 1) * A1
    s.dvar = 3 * g64(p.depth + 2) * A2
    s.rel = s.dvar / (var + eps)
    s.rho = s.rel / 2 + 4 * E64
    s.xh = (x64 - mu) * s.r
    s.fb = SPARE * (s.r * (U * mu.abs() + s.dmu) + (3 * U + s.rho) * s.xh.abs()) + TINY
    return s


def ref_fwd(x, eps, relu, p):
    """(y64, bound, stats)."""
    s = stats64(x, eps, p)
    return (s.xh.clamp_min(0) if relu else s.xh), s.fb, s


def ref_bwd(x, dy, eps, relu, p, mut=None):
    """(dx64, bound)."""
    s = stats64(x, eps, p)
    g = dy.double()
    if relu:
        g = torch.where(s.xh > 0, g, torch.zeros((), dtype=F64))
    m1, m2 = g.mean(1, keepdim=True), (g * s.xh).mean(1, keepdim=True)
    dx = s.r * (g - m1 - s.xh * m2)
    gx = (g * s.xh).abs().mean(1, keepdim=True)
    dm1 = U * m1.abs() + g64(p.depth + 1) * g.abs().mean(1, keepdim=True)
    dm2 = SPARE * ((g.abs() * s.fb).mean(1, keepdim=True) + (U + g64(p.depth + 1)) * gx + U * m2.abs()) + TINY
    P = g.abs() + m1.abs() + (s.xh * m2).abs()
    bb = SPARE * s.r * (dm1 + m2.abs() * s.fb + (s.xh.abs() + s.fb) * dm2 + (gamma(5) + s.rho) * P) + 4 * TINY
    return dx, bb


# --------------------------------------------------------------------------- the kernel's arithmetic
def emu_stats(x, eps, p, mut=None):
    """(mean, rstd) [planes][1] fp32."""
    x64 = x.double()
    n = x.shape[1]
    S1 = kernel_sum(x64, p, mut)
    if mut == "fp32_sumsq":
        sq = (x * x)
        S2 = sq.cumsum(1, dtype=F32)[:, -1].double()       # one fp32 accumulator
    else:
        S2 = kernel_sum(x64 * x64, p, mut)
    mu = S1 / n
    var = S2 / n - mu * mu
    if mut == "unbiased":
        var = var * n / max(n - 1, 1)
    var = var.clamp_min(0)
    e = float(torch.tensor(eps, dtype=F32))
    rstd = 1.0 / (torch.sqrt(var) + e) if mut == "eps_outside" else 1.0 / torch.sqrt(var + e)
    return mu.float().unsqueeze(1), rstd.float().unsqueeze(1)


def emu_fwd(x, eps, relu, p, mut=None):
    """(y, mean_rstd [planes][2]) fp32."""
    mean, rstd = emu_stats(x, eps, p, mut)
    xh = (x - mean) * rstd
    return (torch.where(xh > 0, xh, torch.zeros(())) if relu else xh), torch.cat([mean, rstd], 1)


def emu_bwd(x, mean_rstd, dy, relu, p, mut=None):
    mean, rstd = mean_rstd[:, :1], mean_rstd[:, 1:]
    n = x.shape[1]
    xh = (x - mean) * rstd
    zero = torch.zeros(())
    g = dy
    if relu:
        g = torch.where((xh >= 0) if mut == "mask_ge" else (xh > 0), dy, zero)
    g2 = dy if mut == "m2_nomask" else g
    m1 = (kernel_sum(g.double(), p) / n).float().unsqueeze(1)
    m2 = (kernel_sum((g2 * xh).double(), p) / n).float().unsqueeze(1)
    return rstd * ((g - m1) - xh * m2)


# --------------------------------------------------------------------------- the case table
def _case(planes, H, W, label, classes=None, need=None):
    return types.SimpleNamespace(planes=planes, H=H, W=W, plane=H * W, label=label, classes=classes, need=need or {},
                                 name="%dx%dx%d" % (planes, H, W))


TABLE = [
    _case(96, 1, 4, "plane256", need={"n4": 1}),
    _case(96, 2, 6, "plane256", need={"n4": 3}),
    _case(97, 1, 7164, "plane256", need={"n4": 1791}),
    _case(96, 56, 128, "plane256", need={"n4": 1792}),
    _case(96, 1, 7172, "plane1024", need={"n4": 1793}),
    _case(96, 7, 1028, "plane1024"),
    _case(96, 112, 256, "plane1024", need={"n4": 7168}),
    _case(96, 67, 428, "two_vec", need={"chunks": 8, "chunk_len": 3588, "last": 3560}),
    _case(95, 4, 8, "two_vec", need={"chunks": 1}),
    _case(2, 7, 1756, "two_vec", ("bigmean", "outlier"), {"chunks": 4, "last": 3064}),
    _case(2, 5, 2459, "two_scalar", ("bigmean", "symmetric"), {"chunks": 4, "ragged": 1}),
    _case(3, 1, 4097, "two_scalar", ("normal", "bigmean", "huge"), {"chunks": 2, "ragged": 1}),
    _case(2, 1, 262148, "two_vec", ("bigmean", "normal"), {"chunks": 64, "ragged": 1}),
    _case(1, 1, 262147, "two_scalar", ("bigmean",), {"chunks": 64, "ragged": 1}),
    _case(3, 1, 1, "two_scalar", ("normal", "bigmean", "huge")),
    _case(5, 7, 9, "two_scalar"),
]
CASES = {c.name: c for c in TABLE}
FUSED_OFF = ("96x56x128", "96x7x1028")          # one per one-launch kernel, re-run on the two-launch form
MISALIGNED = ("96x2x6", "96x7x1028", "2x7x1756")    # plane % 4 == 0: a 4-byte shift sends them down the scalar path
WILD = "96x7x1028"


def plan_facts(p):
    return {"n4": p.plane // 4, "chunks": p.chunks, "chunk_len": p.chunk_len, "last": p.last,
            "ragged": int(p.last != p.chunk_len)}


def case_plan(case, vec=None, fused=True):
    return plan(case.planes, case.plane, vec, fused)


def plane_classes(case, eps0=False):
    """The data class of every plane."""
    out = []
    for i in range(case.planes):
        c = case.classes[i % len(case.classes)] if case.classes else CLASSES[i % len(CLASSES)]
        if case.plane == 1:
            c = "constant"
        elif c == "symmetric" and case.plane < 3:
            c = "constant"
        if eps0 and c == "constant":
            c = "normal"
        out.append(c)
    return out


def _draw(cls, n, i, g):
    z = torch.randn(n, generator=g)
    if cls == "normal":
        return 0.4 + 1.7 * z
    if cls == "bigmean":
        return (1000.0 if i % 2 else -1000.0) + z
    if cls == "smallsigma":
        return 0.3 + 1e-4 * z
    if cls == "constant":
        return torch.full((n,), (0.7 + 0.01 * i) * (-1) ** i)
    if cls == "symmetric":
        a, k = float(0.5 + torch.rand((), generator=g)), n // 3
        v = torch.cat([torch.full((k,), a), torch.full((k,), -a), torch.zeros(n - 2 * k)])
        return v[torch.randperm(n, generator=g)]
    if cls == "outlier":
        z[n // 2] = 1.0e4
        return z
    if cls == "huge":
        return 1.0e18 * z
    raise KeyError(cls)


def undecided(x, eps, p, exact):
    """Elements whose ReLU mask the fp32 kernel and float64 may decide differently; exact [planes][1]: planes whose
    x == mu elements are exact zeros for both."""
    s = stats64(x, eps, p)
    zero = (x.double() == s.mu) & exact
    return (s.xh.abs() < THRESHOLD * s.fb) & ~zero, s


@functools.lru_cache(maxsize=None)
def _inputs(name, eps0, wild):
    case = CASES[name]
    g = torch.Generator().manual_seed(1000 * case.planes + case.plane)
    cls = plane_classes(case, eps0)
    x = torch.stack([_draw(c, case.plane, i, g) for i, c in enumerate(cls)]).float().contiguous()
    exact = torch.tensor([c in ("constant", "symmetric") for c in cls]).view(-1, 1)
    # every form the case may run on: the worst depth decides
    plans = [case_plan(case), case_plan(case, vec=False), case_plan(case, fused=False)]
    p = max(plans, key=lambda q: q.depth)
    eps = 0.0 if eps0 else EPS
    for _ in range(40):
        low, s = undecided(x, eps, p, exact)
        if not bool(low.any()):
            break
        sign = torch.where(s.xh < 0, -1.0, 1.0)
        x = torch.where(low, (s.mu + sign * 4 * THRESHOLD * s.fb / s.r).float(), x)
    low, s = undecided(x, eps, p, exact)
    assert not bool(low.any()), "an element within THRESHOLD bounds of the ReLU's edge"
    assert float(s.rel.max()) <= 2.0 ** -16, "var + eps too small against the fp64 cancellation"
    if eps0:
        assert float(s.var.min()) > 0
    if wild:
        x = x.clone()
        for i, v in zip(wild_planes(case), (math.nan, math.inf, -math.inf)):
            x[i, (7 * i) % case.plane] = v
    return x


def inputs(case, eps=EPS, wild=False):
    return _inputs(case.name, eps == 0.0, wild)


def wild_planes(case):
    return (1, case.planes // 2, case.planes - 2)


@functools.lru_cache(maxsize=None)
def _gout(name, variant, eps0):
    case = CASES[name]
    g = torch.Generator().manual_seed(77 + case.planes + case.plane)
    dy = torch.randn(case.planes, case.plane, generator=g)
    if variant == "zero":
        dy = torch.zeros_like(dy)
    elif variant == "onehot":                       # at the plane's largest element: never masked unless all are
        x = _inputs(name, eps0, False)
        dy = torch.zeros_like(dy).scatter_(1, x.argmax(1, keepdim=True), 1.0)
    return dy


def gout(case, variant="random", eps=EPS):
    return _gout(case.name, variant, eps == 0.0)


def runs(case):
    """(eps, relu) of the forward and (eps, relu, variant) of the backward calls of one case."""
    eps_all = (EPS,) if case.plane == 1 else (EPS, 0.0)
    fwd = [(e, r) for e in eps_all for r in (0, 1)]
    return fwd, [(e, r, "random") for e, r in fwd] + [(EPS, r, v) for r in (1, 0) for v in ("zero", "onehot")]


# --------------------------------------------------------------------------- gates
def _none(H, W, m):
    return {}


def _groups(case, eps):
    cls = plane_classes(case, eps == 0.0)
    out = {}
    for c in set(cls):
        out["class/" + c] = torch.tensor([k == c for k in cls]).view(1, -1, 1, 1).expand(1, case.planes, 1, case.plane)
    return out


def _as4(t):
    return t.reshape(1, t.shape[0], 1, t.shape[1])


def gate(case, eps, got, want, bound, emu, record, prefix, keep=None):
    """Both gates on [planes][plane] results; keep [planes] leaves planes out (the wild case)."""
    if keep is not None:
        k = keep.view(-1, 1)
        got, emu = torch.where(k, got, want.float()), torch.where(k, emu, want.float())
    record(prefix + "bits_of_fp32_model", "%.4f" % float((got.contiguous().view(torch.int32) == emu.contiguous().view(torch.int32)).double().mean()))
    return _gates(_as4(got), _as4(want), None, 0, _as4(emu), 0, record, prefix, regions=_none, bound=_as4(bound),
                  extra=_groups(case, eps))


def check_fwd(case, eps, relu, got_y, got_mr, p, record, prefix="fwd_", keep=None):
    clean = inputs(case, eps)
    want, bound, s = ref_fwd(clean, eps, relu, p)
    ey, emr = emu_fwd(clean, eps, relu, p)
    mr = got_mr if keep is None else torch.where(keep.view(-1, 1), got_mr, emr)
    dm = float(((mr[:, :1].double() - s.mu).abs() / (SPARE * (U * s.mu.abs() + s.dmu) + TINY)).max())
    dr = float(((mr[:, 1:].double() - s.r).abs() / (SPARE * s.r * (U + s.rho))).max())
    record(prefix + "mean_ratio", "%.3g" % dm)
    record(prefix + "rstd_ratio", "%.3g" % dr)
    assert dm <= 1 and dr <= 1, (dm, dr)
    return gate(case, eps, got_y, want, bound, ey, record, prefix, keep)


def check_bwd(case, eps, relu, variant, got, p, record, prefix="bwd_", keep=None):
    x, dy = inputs(case, eps), gout(case, variant, eps)
    want, bound = ref_bwd(x, dy, eps, relu, p)
    emu = emu_bwd(x, emu_fwd(x, eps, relu, p)[1], dy, relu, p)
    if variant == "zero":
        assert bool((got == 0).all()), "zero grad_out must give exact zeros"
    return gate(case, eps, got, want, bound, emu, record, prefix, keep)


# --------------------------------------------------------------------------- the exact kernels
EXACT_N = (1, 3, 4, 5, 1023, 1024 * 4 + 3, 2048 * 256 * 4 + 7)
SUB = 2.0 ** -149


def exact_operands(n):
    """a, b (a + b cancels to exactly 0 on a fifth of the elements; +-0 and the smallest subnormal among the values),
    out, out2 in {> 0, 0, -0}, grad_out."""
    g = torch.Generator().manual_seed(n)
    special = torch.tensor([0.0, -0.0, SUB, -SUB, 1.0, -1.0, 3.0e38, -3.0e38])
    a = torch.randn(n, generator=g)
    i = torch.arange(n)
    a = torch.where(i % 3 == 0, special[i % 8], a)
    b = torch.where(i % 5 == 0, -a, torch.where(i % 7 == 0, special[(i // 7) % 8], torch.randn(n, generator=g)))
    both = i % 11 == 2                                           # a = b = -0: the sum is -0
    a, b = torch.where(both, torch.tensor(-0.0), a), torch.where(both, torch.tensor(-0.0), b)
    pick = torch.tensor([1.5, 0.0, -0.0, SUB])
    out, out2 = pick[i % 4], pick[(i // 4 + i) % 4]
    return a, b, out, out2, torch.randn(n, generator=g)


def add_relu_ref(a, b):
    return torch.relu(a + b)


def relu_bwd_ref(out, gout_):
    return torch.where(out > 0, gout_, torch.zeros(()))


def relu_bwd2_ref(out, out2, gout_):
    gx = torch.where(out > 0, gout_, torch.zeros(()))
    return gx, torch.where(out2 > 0, gx, torch.zeros(()))
