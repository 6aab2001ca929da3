"""pcfa_amd.graph_sets on the host (stub owners, no GPU): the one LRU of the three attacks' graph-set caches, its cap per
lane, and -- on the CPU port -- that attack_PCFA's fresh and adopted construction wire the same state."""
import pytest
import torch

from pcfa_amd import attack_PCFA, graph_sets, ops
from pcfa_amd.helper_functions import logging, ownutilities
from tests import closure_util


class _Owner:
    retired = False
    graphed = "a graph"

    def _retire(self):
        self.retired = True


# the three attacks' keys: the lane is not where the cap looks for it -- the set carries it
KEYS = {"pair": lambda shape, lane: ("RAFT", shape, "change_of_variables", False, "aee", 5e5, 0.005, 1e-7, "cuda:0", lane),
        "pair_batch": lambda shape, lane: ("RAFT", shape, "change_of_variables", False, "aee", 5e5, 0.005, 1e-7, "cuda:0",
                                           lane, 2),
        "fgsm": lambda shape, lane: ("RAFT", shape, shape, "aee", False, 0.00025, "zero", "cuda:0", lane)}


class _Cache:
    def __init__(self, kind, cap):
        self.sets, self.owners, self.kind, self.cap = {}, {}, kind, cap

    def put(self, shape, lane):
        key = KEYS[self.kind](shape, lane)
        self.owners[key] = _Owner()
        graph_sets.put(self.sets, key, graph_sets.GraphSet(self.owners[key], lane, ("graphed",)), self.cap, "test-graph")
        return key

    def retired(self):
        return [k for k, o in self.owners.items() if o.retired]


@pytest.mark.parametrize("kind", list(KEYS))
def test_graph_cache_is_lru_per_lane(kind):
    c = _Cache(kind, 2)
    keys = [c.put(shape, lane) for shape in ("A", "B") for lane in range(5)]
    assert len(c.sets) == 10 and not c.retired()                               # cap 2 PER LANE: nothing evicted
    oldest = c.sets[KEYS[kind]("A", 3)]
    third = c.put("C", 3)
    gone = KEYS[kind]("A", 3)
    assert gone not in c.sets and c.owners[gone].retired                       # the oldest shape of lane 3 ...
    assert oldest.graphed is None                                              # (its graphs let go)
    assert third in c.sets and len(c.sets) == 10
    assert all(k in c.sets and not c.owners[k].retired for k in keys if k != gone)   # ... and nothing of another lane
    # a hit makes a set the most recently used one of its lane
    hit = KEYS[kind]("B", 3)
    newcomer = _Owner()
    assert graph_sets.adopt(c.sets, hit, newcomer) is c.sets[hit] and list(c.sets)[-1] == hit
    assert c.owners[hit].retired and c.sets[hit].owner() is newcomer and c.sets[hit].pairs == 2
    assert newcomer.graphed is c.sets[hit].graphed                             # the kept attributes are the new owner's
    c.put("D", 3)
    assert third not in c.sets and c.owners[third].retired and hit in c.sets and not newcomer.retired
    assert graph_sets.adopt(c.sets, KEYS[kind]("E", 3), _Owner()) is None


@pytest.mark.parametrize("kind", list(KEYS))
def test_five_lanes_of_one_shape_retire_nobody(kind):
    """More lanes than Config.max_cached_shapes (PairsInFlight builds them one after the other): building lane 4 must not
    retire lane 0's live attack."""
    c = _Cache(kind, 4)
    keys = [c.put("A", lane) for lane in range(5)]
    assert list(c.sets) == keys and not c.retired()


@pytest.mark.parametrize("cap", [2, 4])
@pytest.mark.parametrize("kind", list(KEYS))
def test_four_lanes_of_two_shapes_keep_all_eight(kind, cap):
    """... and a lane's further shapes evict that lane's oldest set only, once the lane holds more than the cap: the third
    shape at cap 2, the fifth at cap 4 (with the cap counted over all lanes, cap 4 kept four of the eight)."""
    c = _Cache(kind, cap)
    keys = [c.put(shape, lane) for shape in ("A", "B") for lane in range(4)]
    assert list(c.sets) == keys and not c.retired()
    for shape in "CDE"[:cap - 2]:
        c.put(shape, 2)
    assert len(c.sets) == 8 + cap - 2 and not c.retired()                      # lane 2 holds `cap` sets: all kept
    c.put("Z", 2)
    assert c.retired() == [KEYS[kind]("A", 2)] and len(c.sets) == 8 + cap - 2


# ---- attack_PCFA: the fresh and the adopted construction wire the same state -------------------------------------------
@pytest.fixture
def _cpu_port(oracle_ops):
    torch.set_num_threads(8)
    with ops.override_for_testing(oracle_ops):
        yield


def _check_wiring(st, images, box, joint, eps):
    """`st` right after construction on the preprocessed `images`: variables, static buffers, the network's operands and
    the 12-tuple of the initial state."""
    image1, image2 = images
    assert torch.equal(st.image1, image1) and torch.equal(st.image2, image2)
    assert torch.equal(st.images_max, torch.max(image1, image2)) and torch.equal(st.images_min, torch.min(image1, image2))
    if joint:
        assert len(st.params) == 1 and torch.equal(st.params[0], torch.zeros_like(image1))
        assert st.nw_delta is st.params[0] and st.nw_input1 is st.image1 and st.nw_input2 is st.image2
        assert list(st.fwd_kwargs) == ["delta1"] and st.fwd_kwargs["delta1"] is st.params[0]
    else:
        want = [torch.atanh(2. * (1. - eps) * x - (1 - eps)) for x in images] if box == "change_of_variables" else images
        assert len(st.params) == 2 and torch.equal(st.params[0], want[0]) and torch.equal(st.params[1], want[1])
        assert st.nw_delta is None and st.nw_input1 is st.params[0] and st.nw_input2 is st.params[1]
        assert st.fwd_kwargs == {}
    assert all(p.requires_grad and p.grad is None and p.is_leaf for p in st.params)
    assert not st.target.requires_grad and torch.equal(st.target, torch.zeros_like(st.flow_pred_init))
    assert st.flow_pred is st.flow_pred_init and st.steps_done == 0 and st.closures == 0
    assert not st.delta1.any() and not st.delta2.any() and st.delta1_min is None
    inf = float("inf")
    assert st.result() == (None, logging.calc_metrics_const(st.target, st.flow_pred_init), None, 0., 0., 0., 0., 0., 0., inf,
                           0., inf)
    assert st.aee_tgt == st.result()[1] > 0 and st.aee_adv_tgt_min_val == inf


@pytest.mark.parametrize("box,joint", [("clipping", False), ("change_of_variables", False), ("clipping", True)],
                         ids=["clipping", "change_of_variables", "joint_perturbation"])
def test_fresh_and_adopted_construction_wire_the_same_state(_cpu_port, box, joint):
    dev, eps = torch.device("cpu"), attack_PCFA.EPS_BOX
    model = closure_util.load_model("RAFT", box == "change_of_variables", dev)
    args = closure_util.cli_args(net="RAFT", boxconstraint=box, joint_perturbation=joint, steps=1)
    sets = graph_sets.cache(model, "pair-graph")
    assert sets is model._pcfa_pair_graphs
    sets.clear()

    def build(seed, **kw):
        raw = closure_util.test_images(seed, 128, 160)
        _, images = ownutilities.preprocess_img("RAFT", raw[0] / 255., raw[1] / 255.)
        st = attack_PCFA.PairAttack(model, raw[0], raw[1], None, seed, eps, dev, False, attack_PCFA.default_mu(args), args,
                                    **kw)
        return st, images
    try:
        fresh, images = build(1, use_graph=False)
        assert not fresh.graphs_reused and fresh.graphed is None and not sets
        _check_wiring(fresh, images, box, joint, eps)
        # what a capture would leave behind (the CPU port captures nothing and its optimiser is torch's, without reset())
        fresh.optimizer.reset = fresh.optimizer.state.clear
        graph_sets.put(sets, fresh.graph_key, graph_sets.GraphSet(fresh, fresh.lane, fresh.KEPT), 4, "pair-graph")
        adopted, images2 = build(2, use_graph=True, reuse_graphs=True)
        assert adopted.graphs_reused and fresh.retired and list(sets) == [adopted.graph_key] == [fresh.graph_key]
        assert not torch.equal(images2[0], images[0])
        for name in fresh.KEPT:
            mine, theirs = getattr(adopted, name), getattr(sets[fresh.graph_key], name)
            assert mine is theirs or (name == "params" and all(a is b for a, b in zip(mine, theirs)))
        assert adopted.image1 is fresh.image1 and adopted.optimizer is fresh.optimizer
        _check_wiring(adopted, images2, box, joint, eps)
        with pytest.raises(RuntimeError, match="retired"):
            fresh.step()
    finally:
        sets.clear()
