"""Helpers shared by the test modules."""
import os

import numpy as np
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(REPO, "tests", "golden")


def load_golden(name):
    z = np.load(os.path.join(GOLDEN, name + ".npz"))
    return {k: z[k] for k in z.files}


def pattern(shape, salt):
    """Deterministic pseudo-random float32 array, exact on every host (integer hash -> multiples of 1/512 in [-2, 2)):
    a gradient that a fixture does not need to store."""
    i = np.arange(int(np.prod(shape)), dtype=np.uint64) + np.uint64(salt) * np.uint64(1000003)
    h = (i * np.uint64(2654435761)) % np.uint64(4294967291)
    return (((h % np.uint64(2048)).astype(np.float32) - 1024) / 512).reshape(shape)


def t(a, device="cpu"):
    """numpy -> float32 torch tensor"""
    return torch.from_numpy(np.ascontiguousarray(a)).float().to(device)


def rel_l2(a, b):
    a, b = a.detach().double().flatten().cpu(), b.detach().double().flatten().cpu()
    return float((a - b).norm() / (b.norm() + 1e-30))


def max_abs(a, b):
    return float((a.detach().double().cpu() - b.detach().double().cpu()).abs().max())
