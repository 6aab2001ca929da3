"""Tier A of tests/net_modules.py: the networks' glue in float64 on the CPU operator table, and the negative controls.

Every case: (1) its committed seed is the first whose float64 restatement keeps the kink margins; (2) the frozen fast path
of pcfa_amd/nets, in float64 under ops.override_for_testing(oracle), agrees with the restatement to rel-L2 <= 1e-11 and
max-abs <= 1e-11 max|ref| on every output and every input gradient, each tensor on its own; (3) the unfrozen fallback
(norm(conv(x)), SepConvGRU.forward, head(net), the library modules of PWC-Net) agrees to 1e-12.  The CPU table ignores
the mask flags, so this pins what is value glue: the BatchNorm fold, the biases cancelled under instance norm, _split /
precompute / fanout, mask_logits, _regrid and the layout hand-over, _s2_pad, the BGR fold, the alias of skip_first, the
detach placement in the refinement loop and flow_step.  The flags and the kernels' dispatch are the GPU tier's.

The negative controls put one fault each into the code under test and assert that the comparator reports it on the
tensor named: the gates above are tight enough to see what the closure gates (rel-L2 < 1e-2) let through.
"""
import pytest
import torch

from oracle import ops as oracle
from pcfa_amd import ops
from tests import net_modules as nm

torch.set_num_threads(min(16, torch.get_num_threads()))

_REF = {}


def ref(case):
    """The float64 restatement of a case, computed once and shared (never modified)."""
    if case.name not in _REF:
        _REF[case.name] = nm.reference(case, case.seed)
    return _REF[case.name]


def fast_path(case, table=oracle, frozen=True, config=None):
    module, x = nm.materialise(case, case.seed)
    module = nm.prepare(module, config, torch.float64, "cpu", frozen)
    with ops.override_for_testing(table):
        return nm.evaluate(lambda leaves: case.run(module, leaves), x, case.diff, case.seed, torch.float64)


@pytest.mark.parametrize("case", nm.CASES, ids=repr)
def test_seed_is_the_first_margin_clean_one(case):
    assert case.seed is not None and nm.first_clean_seed(case) == case.seed
    _, tape = ref(case)
    act, coord = tape.worst()
    assert act >= nm.RELU_MARGIN and coord >= nm.COORD_MARGIN


@pytest.mark.parametrize("case", nm.CASES, ids=repr)
def test_frozen_fast_path_matches_restatement_in_float64(case):
    want, tape = ref(case)
    assert tape.clean()
    got = fast_path(case)
    assert list(got) == list(want)
    bad = nm.failures(got, want, 1e-11, 1e-11)
    assert not bad, {k: nm.distances(got, want)[k] for k in bad}


@pytest.mark.parametrize("case", nm.CASES, ids=repr)
def test_unfrozen_fallback_matches_restatement_in_float64(case):
    want, _ = ref(case)
    got = fast_path(case, frozen=False)
    bad = nm.failures(got, want, 1e-12, 1e-12)
    assert not bad, {k: nm.distances(got, want)[k] for k in bad}


# --------------------------------------------------------------------------- negative controls
class Patched:
    """The CPU table with some entries replaced."""

    def __init__(self, base, **over):
        self._base, self._over = base, over

    def __getattr__(self, name):
        over = self.__dict__["_over"]
        return over[name] if name in over else getattr(self.__dict__["_base"], name)


def control(case, named, table=oracle):
    """The comparator must fail on `named` (and the unpatched code must not fail at all: the other tests)."""
    want, _ = ref(case)
    bad = nm.failures(fast_path(case, table), want, 1e-11, 1e-11)
    assert named in bad, "the fault went unnoticed on %s (failing: %s)" % (named, bad)
    return bad


def test_control_fold_batchnorm_dropping_running_mean(monkeypatch):
    from pcfa_amd.nets import raft
    orig = raft._fold_batchnorm

    def fold(conv, bn, cache, tag):
        w, b = orig(conv, bn, cache, tag)
        return w, b + bn.running_mean * bn.weight * torch.rsqrt(bn.running_var + bn.eps)   # = (b - 0) * s + beta

    monkeypatch.setattr(raft, "_fold_batchnorm", fold)
    control(nm.BY_NAME["resblock-batch-s1-2x12x16"], "out")
    control(nm.BY_NAME["resblock-batch-s2-2x12x16"], "d_x")


def test_control_gru_split_taking_the_context_weights_for_rest(monkeypatch):
    from pcfa_amd.nets import raft

    def split(self, tag, convs):
        hd, cd = self.hidden_dim, self.const_dim
        with torch.no_grad():
            w = torch.cat([c.weight for c in convs], dim=0)
            b = torch.cat([c.bias for c in convs], dim=0).contiguous()
            w_dyn = torch.cat([w[:, :hd], w[:, hd:-cd]], dim=1).contiguous()   # w[:, hd:] instead of w[:, hd + cd:]
            w_const = w[:, hd:hd + cd].contiguous()
        return w_dyn, w_const, b

    monkeypatch.setattr(raft.SepConvGRU, "_split", split)
    control(nm.BY_NAME["update-b1-mask-8x12"], "net")
    control(nm.BY_NAME["update-b2-nomask-8x12"], "d_flow")


def test_control_regrid_with_sub_grid_indices_swapped(monkeypatch):
    from pcfa_amd.nets import pwcnet
    orig = pwcnet._regrid

    def regrid(x, d_from, d_to, batch):
        y = orig(x, d_from, d_to, batch)
        if d_to == 1 or d_from == d_to:
            return y
        return y.reshape((batch, d_to, d_to) + tuple(y.shape[1:])).transpose(1, 2).reshape(y.shape)   # (gy, gx) -> (gx, gy)

    monkeypatch.setattr(pwcnet, "_regrid", regrid)
    case = nm.BY_NAME["pwcctx-16x32"]
    assert case.hw[0] != case.hw[1]
    control(case, "flow")


def test_control_bgr_weight_unflipped(monkeypatch):
    from pcfa_amd.nets import pwcnet
    monkeypatch.setattr(pwcnet._ConvLeaky, "_bgr_weight", lambda self: self[0].weight)
    control(nm.BY_NAME["pwcpyr-l1-20x32"], "out")


def test_control_fanout_returning_the_last_alias_gradient_only():
    table = Patched(oracle, fanout=lambda x, n: tuple(x.detach() for _ in range(n - 1)) + (x,))
    bad = control(nm.BY_NAME["raftloop-train-8x12"], "d_cnet_out", table)
    assert not any(k.startswith("flow_up") for k in bad)   # a gradient-only fault


def test_control_lookup_coordinates_not_detached(monkeypatch):
    """Stand-in for `coords1 = coords1.detach()` removed from the loop: flow_step's live coordinates reach a
    differentiable lookup (the CPU table's grid_sample) through a patched LookupRef."""
    from pcfa_amd.nets import raft
    live = {}

    def flow_step(coords1, delta, coords0):
        live["coords"], flow = oracle.flow_step(coords1, delta, coords0)
        return live["coords"], flow

    class Leaky(raft.LookupRef):
        def __init__(self, corr_fn, coords):
            super().__init__(corr_fn, live.get("coords", coords))

    monkeypatch.setattr(raft, "LookupRef", Leaky)
    bad = control(nm.BY_NAME["raftloop-test-8x12"], "d_cnet_out", Patched(oracle, flow_step=flow_step))
    assert "flow_up" not in bad   # the values are those of the detached coordinates


def test_control_mask_logits_folding_one_half(monkeypatch):
    from pcfa_amd.nets import raft
    orig = raft.mask_logits
    monkeypatch.setattr(raft, "mask_logits", lambda head, net, cache: 2 * orig(head, net, cache))
    control(nm.BY_NAME["update-b1-mask-8x12"], "mask")


def test_control_s2_pad_slicing_one_column_late():
    """Stand-in for `y[..., 1:w_out + 1]` after the padded stride-2 layer: the table hands back the padded result moved
    one column to the left, so the layer's own `[..., :w_out]` cuts those columns."""
    case = nm.BY_NAME["pwcpyr-l3-20x36"]
    seen = []

    def conv_s2(x, *args, **kw):
        y = oracle.conv_s2(x, *args, **kw)
        seen.append(x.shape[-1])
        return torch.nn.functional.pad(y[..., 1:], (0, 1)) if x.shape[-1] != case.hw[1] else y

    control(case, "out", Patched(oracle, conv_s2=conv_s2))
    assert seen == [40]   # the layer did pad 36 -> 40 (a multiple of 8 for its own data gradient)
