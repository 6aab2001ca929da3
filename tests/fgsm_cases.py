"""Inputs, torch reference and census of tests/test_fgsm_step_gpu.py (pcfa_fgsm_step, pcfa_amd/csrc/attack_math.hip).
Not a test; no GPU.  tests/test_fgsm_graph_host_cpu.py asserts the census on the CPU.

The reference is the torch sequence the kernel replaces -- attack_FGSM.fgsm_attack_step(..., clipping=True) followed by
torch.clamp(nw, 0., 1.) - image -- run on the device of its inputs; the kernel has to reproduce it bit for bit.

A case of n elements is the first n entries of ONE table: the CRAFTED block, every gradient pair below against every start
value, then seeded random entries.  n = 1, 3, 4, 5 see only the head of the block; every n >= len(CRAFTED block) sees all
of it, and the census is taken over exactly that block."""
import numpy as np
import torch

EPSILON = 0.00025                       # the CLI default (parsing_file.py)
EPS32 = np.float32(EPSILON)
SUB = np.float32(2.0 ** -149)           # the smallest subnormal
BIG = np.float32(3.0e38)                # BIG + BIG overflows
INF, NAN = np.float32(np.inf), np.float32(np.nan)

# (g1, g2): what the disjoint signs see element by element and what the joint sign sees in 0.5f * (g1 + g2)
GRAD_PAIRS = [
    (0.0, -0.0), (-0.0, 0.0),            # +-0: sign 0 in both modes
    (SUB, -SUB),                         # the smallest subnormal and its negative: +-1 disjoint, the sum is 0
    (SUB, 0.0), (0.0, -SUB),             # the sum is the smallest subnormal: its half rounds to 0 (joint: no move)
    (INF, 1.0), (-INF, 1.0),             # +-inf: +-1
    (INF, -INF), (-INF, INF),            # joint: inf - inf = NaN -> sign 0 -> no move
    (NAN, 1.0), (1.0, NAN), (NAN, NAN),  # NaN: sign 0
    (BIG, BIG), (-BIG, -BIG),            # the sum overflows to +-inf: still +-1
    (1.0, 2.0), (-1.0, -2.0), (1.0, -3.0), (0.5, -0.5), (-2.0, 0.25),
]
# start values of x: both clamps are reached (0 - eps, 1 + eps), eps / 2 and 1 - eps / 2 clamp one way and move the other,
# 0.5 always moves freely, and a NaN pixel stays NaN
X_VALUES = [0.0, 1.0, float(EPS32 / np.float32(2)), float(np.float32(1) - EPS32 / np.float32(2)), 0.5, float("nan")]

CLASSES = ("moved by +eps", "moved by -eps", "unmoved by sign 0", "clamped at 0", "clamped at 1", "NaN kept")


def crafted():
    """(x1, x2, g1, g2, img1, img2) of the crafted block as float32 numpy arrays."""
    x1, x2, g1, g2 = [], [], [], []
    for (a, b) in GRAD_PAIRS:
        for k, v in enumerate(X_VALUES):
            x1.append(v)
            x2.append(X_VALUES[(k + 1) % len(X_VALUES)])     # the two images never start from the same value
            g1.append(a)
            g2.append(b)
    x1, x2 = np.array(x1, np.float32), np.array(x2, np.float32)
    # the clean images: where the entry index is even the start value itself (delta is exactly the move), else another value
    idx = np.arange(len(x1))
    img1 = np.where(idx % 2 == 0, x1, np.float32(0.25)).astype(np.float32)
    img2 = np.where(idx % 2 == 1, x2, np.float32(0.75)).astype(np.float32)
    return x1, x2, np.array(g1, np.float32), np.array(g2, np.float32), img1, img2


_TABLE = {}


def table(n):
    """The first n entries of the case table: six float32 CPU tensors (x1, x2, g1, g2, img1, img2)."""
    if "t" not in _TABLE or _TABLE["t"][0].numel() < n:
        block = crafted()
        m = max(n, 4096) - len(block[0])
        rng = np.random.RandomState(20240611)
        rand = [rng.uniform(0, 1, m), rng.uniform(0, 1, m), rng.standard_normal(m), rng.standard_normal(m),
                rng.uniform(0, 1, m), rng.uniform(0, 1, m)]
        # a tenth of the random start values sit within eps of an end of the box, so the clamps stay busy past the block
        for x in rand[:2]:
            edge = rng.uniform(0, 1, m) < 0.1
            x[edge] = np.where(rng.uniform(0, 1, m) < 0.5, 0.0, 1.0)[edge]
        _TABLE["t"] = [torch.from_numpy(np.concatenate([b, r.astype(np.float32)])) for b, r in zip(block, rand)]
    return [t[:n].clone() for t in _TABLE["t"]]


def torch_reference(x1, x2, g1, g2, img1, img2, epsilon, joint):
    """(x1', x2', d1, d2): attack_FGSM.py:205-209 as the package's eager loop ran it before the kernel existed."""
    from pcfa_amd.attack_FGSM import fgsm_attack_step
    p1, p2 = fgsm_attack_step(x1, x2, epsilon, g1, g2, clipping=True, common_perturb=bool(joint))
    return p1, p2, torch.clamp(p1, 0., 1.) - img1, torch.clamp(p2, 0., 1.) - img2


def census(joint):
    """class -> number of elements (both images counted) of the crafted block that fall into it, from float64 arithmetic on
    the CPU: the sign the mode uses, the unclamped move, which clamp (if any) catches it."""
    x1, x2, g1, g2, _, _ = (a.astype(np.float64) for a in crafted())
    f1, f2 = crafted()[2], crafted()[3]
    with np.errstate(invalid="ignore", over="ignore"):
        if joint:
            s = np.sign(np.nan_to_num((np.float32(0.5) * (f1 + f2)).astype(np.float32), nan=0.0))   # fp32 sum, then the half
            s1 = s2 = s
        else:
            s1, s2 = np.sign(np.nan_to_num(f1, nan=0.0)), np.sign(np.nan_to_num(f2, nan=0.0))
    masks = {}
    for which, (x, s) in enumerate(((x1, s1), (x2, s2))):
        p = x - float(EPS32) * s
        nan = np.isnan(x)
        masks[which] = {"NaN kept": nan, "unmoved by sign 0": (s == 0) & ~nan, "clamped at 0": (p < 0) & ~nan,
                        "clamped at 1": (p > 1) & ~nan, "moved by +eps": (s < 0) & (p <= 1) & ~nan,
                        "moved by -eps": (s > 0) & (p >= 0) & ~nan}
    counts = {c: int(masks[0][c].sum() + masks[1][c].sum()) for c in CLASSES}
    return counts, masks
