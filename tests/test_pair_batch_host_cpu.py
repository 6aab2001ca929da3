"""Host logic of --pairs_per_closure (attack_PCFA.attack_l2, group_pairs): how a rank's pair stream is grouped and flushed,
that every row reaches gather_rows under its pair's own index whatever the grouping, rank sharding, the refused flag
combinations and the parser flag.  The attacks themselves are replaced by recorders: no GPU, no network."""
from argparse import Namespace

import pytest
import torch

from pcfa_amd import attack_PCFA, sharding
from pcfa_amd.helper_functions import parsing_file


def test_groups_fill_in_arrival_order_and_flush_oldest_first():
    stream = [(0, "a"), (1, "b"), (2, "a"), (3, "a"), (4, "c"), (5, "b"), (6, "a"), (7, "a"), (8, "b")]
    groups = list(attack_PCFA.group_pairs(iter(stream), 3, lambda p: p[1]))
    assert groups == [[(0, "a"), (2, "a"), (3, "a")],            # full: attacked at once
                      [(1, "b"), (5, "b"), (8, "b")],
                      [(4, "c")], [(6, "a"), (7, "a")]]          # flushed at the end, oldest open group first
    assert list(attack_PCFA.group_pairs(iter(stream), 1, lambda p: p[1])) == [[p] for p in stream]
    assert list(attack_PCFA.group_pairs(iter([]), 4, lambda p: p)) == []


def _args(**kw):
    base = dict(net="RAFT", steps=2, joint_perturbation=False, universal_perturbation=False,
                boxconstraint="change_of_variables", delta_bound=0.005, mu=-1., target="zero", custom_target_path="",
                loss="aee", save_frequency=1, small_save=False, no_save=True, output_folder="experiment_data",
                pairs_in_flight=1, pairs_per_closure=1)
    base.update(kw)
    return Namespace(**base)


def _loader(shapes):
    return [(torch.zeros(1, 3, h, w), torch.zeros(1, 3, h, w), None, None) for h, w in shapes]


class _Recorder:
    """Stands in for the model, pcfa_attack and PairBatch: remembers who attacked what, answers with the pair's index."""

    def __init__(self, monkeypatch, rank=0, world=1, device="cuda"):
        self.solo, self.batches, self.rows = [], [], None
        rec = self

        class FakeBatch:
            def __init__(self, model, pairs, eps_box, device, has_gt, optim_mu, args, use_graph=None):
                assert len({tuple(p[1].shape) for p in pairs}) == 1
                self.pairs, self.steps = pairs, 0
                rec.batches.append([p[0] for p in pairs])

            def step(self):
                self.steps += 1

            def result(self, b):
                return (None,) + tuple(100.0 * self.pairs[b][0] + k + 0.5 * self.steps for k in range(11))

        def fake_attack(model, image1, image2, flow, batch, folder, eps_box, device, has_gt, optim_mu, args):
            rec.solo.append(batch)
            return (None,) + tuple(100.0 * batch + k + 0.5 * args.steps for k in range(11))

        def fake_gather(rows, width, device):
            rec.rows = list(rows)
            return [tuple(r) for r in rows]

        monkeypatch.setattr(attack_PCFA, "PairBatch", FakeBatch)
        monkeypatch.setattr(attack_PCFA, "pcfa_attack", fake_attack)
        monkeypatch.setattr(attack_PCFA, "_load_model", lambda args, device, variable_change: object())
        monkeypatch.setattr(attack_PCFA, "select_device", lambda: torch.device(device))
        monkeypatch.setattr(sharding, "gather_rows", fake_gather)
        monkeypatch.setattr(sharding, "rank", lambda: rank)
        monkeypatch.setattr(sharding, "world_size", lambda: world)


SHAPES = [(64, 96), (64, 96), (72, 96), (64, 96), (64, 96), (72, 96), (64, 96)]     # indices 0 .. 6


def test_rows_keep_pair_indices_whatever_the_grouping(monkeypatch):
    rec = _Recorder(monkeypatch)
    res3 = attack_PCFA.attack_l2(_args(pairs_per_closure=3), _loader(SHAPES), False)
    assert rec.batches == [[0, 1, 3], [2, 5], [4, 6]] and rec.solo == []      # one full group, two flushed ones
    rows3 = {r[0]: r for r in rec.rows}
    rec.batches[:] = []
    res2 = attack_PCFA.attack_l2(_args(pairs_per_closure=2), _loader(SHAPES), False)
    assert rec.batches == [[0, 1], [3, 4], [2, 5]] and rec.solo == [6]          # a flushed group of one goes to pcfa_attack
    rows2 = {r[0]: r for r in rec.rows}
    rec.batches[:], rec.solo[:] = [], []
    res1 = attack_PCFA.attack_l2(_args(pairs_per_closure=1), _loader(SHAPES), False)
    assert rec.batches == [] and rec.solo == list(range(7))
    rows1 = {r[0]: r for r in rec.rows}
    assert sorted(rows1) == list(range(7))
    for rows in (rows2, rows3):
        assert sorted(rows) == list(range(7))
        for i in range(7):
            assert rows[i][2:] == rows1[i][2:] and rows[i][1] != rows[i][1]    # the pair's own values; None -> NaN
    assert res1 == res2 == res3 and res1["pairs"] == 7                         # the averages do not depend on the grouping


def test_every_batch_steps_args_steps_times(monkeypatch):
    rec = _Recorder(monkeypatch)
    attack_PCFA.attack_l2(_args(pairs_per_closure=2, steps=3), _loader(SHAPES[:2]), False)
    assert rec.rows[0][2] == 0 * 100.0 + 0 + 0.5 * 3 and rec.rows[1][2] == 100.0 + 0.5 * 3


@pytest.mark.parametrize("rank", [0, 1])
def test_rank_takes_every_world_th_pair(monkeypatch, rank):
    rec = _Recorder(monkeypatch, rank=rank, world=2)
    attack_PCFA.attack_l2(_args(pairs_per_closure=2), _loader(SHAPES), False)
    mine = [i for i in range(7) if i % 2 == rank]
    assert sorted(r[0] for r in rec.rows) == mine
    assert sorted([i for g in rec.batches for i in g] + rec.solo) == mine
    for group in rec.batches:
        assert len({SHAPES[i] for i in group}) == 1 and len(group) == 2


def test_refuses_lanes_and_batches_together(monkeypatch):
    _Recorder(monkeypatch)
    with pytest.raises(ValueError, match="pairs_per_closure"):
        attack_PCFA.attack_l2(_args(pairs_per_closure=2, pairs_in_flight=2), _loader(SHAPES), False)


def test_refuses_a_cpu_device(monkeypatch):
    _Recorder(monkeypatch, device="cpu")
    with pytest.raises(ValueError, match="--pairs_per_closure needs a GPU"):
        attack_PCFA.attack_l2(_args(pairs_per_closure=2), _loader(SHAPES), False)
    rec = _Recorder(monkeypatch, device="cpu")
    attack_PCFA.attack_l2(_args(pairs_per_closure=1), _loader(SHAPES[:2]), False)      # the default is not affected
    assert rec.solo == [0, 1]


def test_refuses_more_items_than_the_kernels_take(monkeypatch):
    _Recorder(monkeypatch)
    with pytest.raises(ValueError, match="at most 16"):
        attack_PCFA.attack_l2(_args(pairs_per_closure=17), _loader(SHAPES), False)


def test_parser_has_pairs_per_closure():
    parser = parsing_file.create_parser(stage='training', attack_type='pcfa')
    assert parser.parse_args([]).pairs_per_closure == 1
    assert parser.parse_args(["--pairs_per_closure", "4"]).pairs_per_closure == 4


def test_best_iterate_rule_is_the_reference_rule():
    """attack_PCFA.py:226-243 written out, against best_iterate_rule on every combination of a small grid."""
    vals, bound = (0.001, 0.005, 0.009), 0.005
    for below in (False, True):
        for l2 in vals:
            for l2_min in vals + (float("inf"),):
                for aee in (1.0, 2.0):
                    for aee_min in (1.0, 2.0, float("inf")):
                        update, now_below = False, below
                        if not below:
                            if l2 < l2_min or (l2 == l2_min and aee < aee_min):
                                update = True
                                if l2 <= bound:
                                    now_below = True
                        elif l2 <= bound and aee < aee_min:
                            update = True
                        assert attack_PCFA.best_iterate_rule(below, l2, aee, l2_min, aee_min, bound) == (update, now_below)
