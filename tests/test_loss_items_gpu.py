"""The per-item loss and metric entry points (pcfa_flow_loss_items_fwd / _bwd, pcfa_avg_epe_items, pcfa_sum_squares_items
in pcfa_amd/csrc/attack_math.hip) against the single calls on each item's slices, BIT FOR BIT: item b rides on the grid's y
axis and runs the blocks, threads and summation order of the single call with B = 1.  The float64 accuracy of the single
calls is pinned by tests/test_attack_math_f64_gpu.py; bit equality carries it over.

Cases: B = 3 at 5x7 (less than one workgroup) and at 33x70 read as the un-padded view of a 40x72 buffer; aee, mse, cosim;
disjoint and joint perturbations; item 0 with an active penalty, item 1 with an inactive one, item 2 in between (active);
one run with delta_bound = 0 on zero deltas (the relu tie: half the gradient, per item)."""
import pytest
import torch

from pcfa_amd import _hip, hip_ops

pytestmark = pytest.mark.gpu
_call, _ptr, _s4 = hip_ops._call, hip_ops._ptr, _hip.strides4
DEV = "cuda:0"
B = 3
SIZES = {"5x7": (5, 7, 5, 7), "33x70_of_40x72": (33, 70, 40, 72)}
BOUND, MU = 0.02, 100.0


def _case(size, joint, tie=False, seed=0):
    H, W, HP, WP = SIZES[size]
    g = torch.Generator().manual_seed(seed)
    pred = (torch.randn(B, 2, HP, WP, generator=g) * 3).to(DEV)[:, :, :H, :W]
    target = (torch.randn(B, 2, HP, WP, generator=g) * 3).to(DEV)[:, :, :H, :W]
    # mean square of item 0 above BOUND^2 (penalty active), of item 1 far below (inactive), of item 2 above
    scale = torch.tensor([0.05, 0.001, 0.03]).view(B, 1, 1, 1)
    d1 = (torch.randn(B, 3, H, W, generator=g) * scale).to(DEV)
    d2 = d1 if joint else (torch.randn(B, 3, H, W, generator=g) * scale).to(DEV)
    if tie:
        d1 = torch.zeros_like(d1)
        d2 = d1 if joint else torch.zeros_like(d1)
    return pred, target, d1, d2


def _ws(items):
    return torch.empty(items * _hip.load().pcfa_flow_loss_workspace_bytes() // 4, device=DEV)


def _single(pred, target, d1, d2, bound, f_type, gl, b):
    """pcfa_flow_loss_fwd / _bwd with B = 1 on item b's slices."""
    p, t, a, c = pred[b:b + 1], target[b:b + 1], d1[b], d2[b]
    _, _, H, W = p.shape
    n = a.numel()
    ft = _hip.PCFA_LOSS[f_type]
    scal = torch.full((8,), float("nan"), device=DEV)
    _call("pcfa_flow_loss_fwd", _ptr(p), _s4(p), _ptr(t), _s4(t), 1, H, W, _ptr(a), n, _ptr(c), n, bound, MU, ft,
          _ptr(scal), _ptr(_ws(1)))
    gp, ga, gc = torch.empty(1, 2, H, W, device=DEV), torch.empty_like(a), torch.empty_like(c)
    _call("pcfa_flow_loss_bwd", _ptr(p), _s4(p), _ptr(t), _s4(t), 1, H, W, _ptr(a), n, _ptr(c), n, MU, ft, 0,
          _ptr(scal), _ptr(gl), _ptr(gp), _ptr(ga), _ptr(gc))
    return scal, gp[0], ga, gc


def _items(pred, target, d1, d2, bound, f_type, gl, items=B):
    _, _, H, W = pred.shape
    n = d1[0].numel()
    ft = _hip.PCFA_LOSS[f_type]
    scal = torch.full((items, 8), float("nan"), device=DEV)
    total = torch.full((1,), float("nan"), device=DEV)
    _call("pcfa_flow_loss_items_fwd", _ptr(pred), _s4(pred), _ptr(target), _s4(target), items, H, W, _ptr(d1), n,
          _ptr(d2), n, bound, MU, ft, _ptr(scal), _ptr(total), _ptr(_ws(items)))
    gp, ga, gc = torch.empty(items, 2, H, W, device=DEV), torch.empty_like(d1), torch.empty_like(d2)
    _call("pcfa_flow_loss_items_bwd", _ptr(pred), _s4(pred), _ptr(target), _s4(target), items, H, W, _ptr(d1), n,
          _ptr(d2), n, MU, ft, 0, _ptr(scal), _ptr(gl), _ptr(gp), _ptr(ga), _ptr(gc))
    return scal, total, gp, ga, gc


def _check(pred, target, d1, d2, bound, f_type):
    gl = torch.tensor([0.37], device=DEV)
    scal, total, gp, ga, gc = _items(pred, target, d1, d2, bound, f_type, gl)
    for b in range(B):
        s1, gp1, ga1, gc1 = _single(pred, target, d1, d2, bound, f_type, gl, b)
        assert torch.equal(scal[b, :7], s1[:7]), (b, scal[b], s1)
        assert torch.equal(gp[b], gp1), b
        assert torch.equal(ga[b], ga1), b
        assert torch.equal(gc[b], gc1), b
    want = scal[0, 0]
    for b in range(1, B):
        want = want + scal[b, 0]                  # the in-order fp32 sum
    assert torch.equal(total[0], want)
    return scal, ga


@pytest.mark.parametrize("joint", [False, True], ids=["disjoint", "joint"])
@pytest.mark.parametrize("f_type", ["aee", "mse", "cosim"])
@pytest.mark.parametrize("size", list(SIZES))
def test_items_equal_single_calls(size, f_type, joint):
    pred, target, d1, d2 = _case(size, joint)
    scal, ga = _check(pred, target, d1, d2, BOUND, f_type)
    arg = scal[:, 6].tolist()                      # mean square - bound^2 per item
    assert arg[0] > 0 and arg[1] < 0 and arg[2] > 0
    assert ga[0].abs().max() > 0 and ga[1].abs().max() == 0 and ga[2].abs().max() > 0


@pytest.mark.parametrize("joint", [False, True], ids=["disjoint", "joint"])
def test_relu_tie_per_item(joint):
    pred, target, d1, d2 = _case("5x7", joint, tie=True)
    d1[1] = 0.5                                    # item 1 leaves the tie; items 0 and 2 sit exactly on it
    scal, ga = _check(pred, target, d1, d2, 0.0, "aee")
    assert scal[0, 6] == 0 and scal[2, 6] == 0 and scal[1, 6] > 0
    assert ga[0].abs().max() == 0 and ga[1].abs().max() > 0      # 2 * 0 at the tie; the half shows in the equality above


@pytest.mark.parametrize("size", list(SIZES))
def test_metrics_equal_single_calls(size):
    pred, target, d1, _ = _case(size, False, seed=3)
    epe, ssq = hip_ops.avg_epe_items(pred, target), hip_ops.sum_squares_items(d1)
    assert epe.shape == (B,) and ssq.shape == (B,)
    for b in range(B):
        assert torch.equal(epe[b], hip_ops.avg_epe(pred[b:b + 1], target[b:b + 1]))
        assert torch.equal(ssq[b], hip_ops.sum_squares(d1[b]))


@pytest.mark.parametrize("joint", [False, True], ids=["disjoint", "joint"])
@pytest.mark.parametrize("f_type", ["aee", "cosim"])
def test_operator_is_one_node_with_per_item_bits(f_type, joint):
    """ops.loss_delta_constraint_items: total and [B] losses, backward of the total = the per-item gradients of
    ops.loss_delta_constraint on the item's slices (joint: the two slots added by autograd, as there)."""
    pred, target, d1, d2 = _case("33x70_of_40x72", joint, seed=5)
    leaves = [pred.clone().requires_grad_(), d1.clone().requires_grad_()]
    leaves.append(leaves[1] if joint else d2.clone().requires_grad_())
    total, losses = hip_ops.loss_delta_constraint_items(leaves[0], target, leaves[1], leaves[2], BOUND, MU, f_type)
    assert not losses.requires_grad and losses.shape == (B,)
    total.backward()
    want = losses[0]
    for b in range(1, B):
        want = want + losses[b]
    assert torch.equal(total, want)
    for b in range(B):
        p, a = pred[b:b + 1].clone().requires_grad_(), d1[b].clone().requires_grad_()
        c = a if joint else d2[b].clone().requires_grad_()
        one = hip_ops.loss_delta_constraint(p, target[b:b + 1], a, c, None, BOUND, MU, f_type)
        one.backward()
        assert torch.equal(one, losses[b])
        assert torch.equal(p.grad[0], leaves[0].grad[b])
        assert torch.equal(a.grad, leaves[1].grad[b])
        assert torch.equal(c.grad, leaves[2].grad[b])


def test_more_than_sixteen_items_raises():
    n = _hip.MAX_ITEMS + 1
    pred, d = torch.zeros(n, 2, 5, 7, device=DEV), torch.zeros(n, 3, 5, 7, device=DEV)
    gl = torch.ones(1, device=DEV)
    with pytest.raises(RuntimeError):
        _items(pred, pred, d, d, BOUND, "aee", gl, items=n)
    with pytest.raises(RuntimeError):
        _items(pred, pred, d, d, BOUND, "aee", gl, items=0)
    with pytest.raises(ValueError):
        hip_ops.loss_delta_constraint_items(pred, pred, d, d, BOUND, MU, "aee")
    with pytest.raises(ValueError):
        hip_ops.avg_epe_items(pred, pred)
    with pytest.raises(ValueError):
        hip_ops.sum_squares_items(d)
