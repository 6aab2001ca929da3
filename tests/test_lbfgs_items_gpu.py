"""pcfa_amd.lbfgs.BatchedLBFGS against a solo pcfa_amd.lbfgs.LBFGS per item, BIT FOR BIT (pcfa_lbfgs_gram_*_items in
pcfa_amd/csrc/lbfgs_gram.hip: the solo kernels with the item on the grid's y axis).

B = 4 items of n = 1003 variables in two parameters (500 + 503: ld = 1004 has a pad), history_size = 5 (the ring wraps),
three step() calls of max_iter = 10.  The closures are item-separable and evaluate f_b with ATen ops on a fresh copy of the
item's own vector, so the solo optimiser on that item sees identical loss and gradient bits:
  item 0  well-conditioned quadratic: stops early on a tolerance rule and is frozen while its batch-mates go on
  item 1  ill-conditioned quadratic (1 .. 1e3): runs every iteration; |g|_1 > 1, so the first t < 1
  item 2  linear: y = 0, every pair is rejected, H stays 1
  item 3  starts at the exact minimiser: gradient 0, returns at the initial test in every step()"""
import pytest
import torch

from pcfa_amd.lbfgs import LBFGS, BatchedLBFGS

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
B, N1, N2 = 4, 500, 503
N = N1 + N2
STEPS, MAX_ITER, HISTORY = 3, 10, 5


class Problem:
    def __init__(self):
        g = torch.Generator().manual_seed(7)
        self.c = torch.randn(B, N, generator=g).to(DEV)
        self.a0 = (1.0 + 0.05 * torch.rand(N, generator=g)).to(DEV)
        self.a1 = torch.logspace(0, 3, N).to(DEV)
        self.w = (torch.randn(N, generator=g) * 0.01).to(DEV)

    def f(self, b, x):
        """(loss, gradient) of item b at the fresh, dense vector x."""
        if b == 2:
            return (self.w * x).sum(), self.w.clone()
        r = x - self.c[b]
        gr = (self.a0, self.a1, None, 1.0)[b] * r
        return 0.5 * (gr * r).sum(), gr

    def start(self, b):
        return self.c[3].clone() if b == 3 else torch.zeros(N, device=DEV)


def _solo(prob, b):
    x = prob.start(b)
    ps = [x[:N1].clone().view(20, 25).requires_grad_(), x[N1:].clone().requires_grad_()]
    opt = LBFGS(ps, max_iter=MAX_ITER, history_size=HISTORY)

    def closure():
        loss, gr = prob.f(b, torch.cat([p.detach().reshape(-1) for p in ps]))
        ps[0].grad, ps[1].grad = gr[:N1].clone().view(20, 25), gr[N1:].clone()
        return loss
    return opt, ps, closure


def _batched(prob, items):
    x = torch.stack([prob.start(b) for b in items])
    ps = [x[:, :N1].clone().view(len(items), 20, 25).requires_grad_(), x[:, N1:].clone().requires_grad_()]
    opt = BatchedLBFGS(ps, items=len(items), max_iter=MAX_ITER, history_size=HISTORY)
    losses = torch.zeros(len(items), device=DEV)       # a static buffer, as a captured closure hands back
    seen = []                                          # the variables at every evaluation

    def closure():
        seen.append([p.detach().clone() for p in ps])
        ps[0].grad, ps[1].grad = torch.empty_like(ps[0]), torch.empty_like(ps[1])
        for k, b in enumerate(items):
            loss, gr = prob.f(b, torch.cat([p.detach()[k].reshape(-1) for p in ps]))
            losses[k] = loss
            ps[0].grad[k], ps[1].grad[k] = gr[:N1].view(20, 25), gr[N1:]
        return losses
    return opt, ps, closure, seen


def _compare(prob, items):
    bat, bps, bclosure, seen = _batched(prob, items)
    solos = [_solo(prob, b) for b in items]
    evals = []
    for step in range(STEPS):
        del seen[:]
        got = bat.step(bclosure)
        row = []
        for k, (b, (opt, ps, closure)) in enumerate(zip(items, solos)):
            before = opt.state[ps[0]].get("func_evals", 0)
            want = opt.step(closure)
            st = opt.state[ps[0]]
            what = "item %d, step() %d" % (b, step)
            assert torch.equal(bps[0][k], ps[0]) and torch.equal(bps[1][k], ps[1]), what
            assert torch.equal(got[k], want.reshape(())), what
            assert bat.state[k]["func_evals"] == st["func_evals"], what
            assert bat.state[k]["n_iter"] == st["n_iter"], what
            assert bat.history_count(k) == opt.history_count(), what
            row.append(st["func_evals"] - before)
            # frozen once it stopped: from its last evaluation on, the item's variables never move in this step() unless
            # it ran to max_iter with everybody else (then the last update follows the last evaluation)
            if row[-1] < MAX_ITER:
                for later in seen[row[-1] - 1:]:
                    assert torch.equal(later[0][k], ps[0]) and torch.equal(later[1][k], ps[1]), what
        assert len(seen) == max(row)                   # one evaluation for everybody, as many as the longest item needs
        evals.append(row)
    return bat, solos, evals


def test_items_match_solo_optimisers():
    prob = Problem()
    bat, solos, evals = _compare(prob, [0, 1, 2, 3])
    # the four items are the cases the docstring names
    assert all(row[0] < MAX_ITER for row in evals) and evals[0][0] > 1            # item 0 stops early ...
    assert all(row[1] == MAX_ITER and row[2] == MAX_ITER for row in evals)         # ... while items 1 and 2 continue
    assert all(row[3] == 1 for row in evals) and bat.state[3]["n_iter"] == 0       # item 3 returns at the initial test
    assert solos[1][0].history_count() == HISTORY and bat.history_count(1) == HISTORY   # the ring wrapped
    assert bat.history_count(2) == 0                                               # every pair of the linear item rejected
    assert bat.state[1]["n_iter"] == STEPS * MAX_ITER
    # two host reads per trip for all items together: as many as the longest solo run, not B times that
    assert bat.host_syncs == solos[1][0].host_syncs


def test_one_item_equals_solo():
    bat, solos, _ = _compare(Problem(), [1])
    assert bat.host_syncs == solos[0][0].host_syncs


def test_item_count_is_checked():
    x = torch.zeros(17, 8, device=DEV, requires_grad=True)
    with pytest.raises(ValueError):
        BatchedLBFGS([x], items=17)
    with pytest.raises(ValueError):
        BatchedLBFGS([x[:4].detach().requires_grad_()], items=3)
