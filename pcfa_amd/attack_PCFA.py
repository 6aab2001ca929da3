"""Perturbation-Constrained Flow Attack driver -- the hot loop of the reference's attack_PCFA.py.

    extract_deltas / extract_deltas_joint   attack_PCFA.py:20-37   (fused HIP, pcfa_amd.ops)
    pcfa_attack                             attack_PCFA.py:40-294
    attack_l2_universal                     attack_PCFA.py:297-566
    attack_l2                               attack_PCFA.py:570-701

Schedule: the averaged-L2 bound is an exact penalty minimised by
L-BFGS(max_iter=10, no line search: pcfa_amd.lbfgs.LBFGS = torch.optim.LBFGS semantics on HIP kernels); one `--steps` iteration = one LBFGS.step = 10
closure evaluations (forward + loss + backward) followed by one re-prediction forward, and the
reported result is the best iterate with ||delta|| <= bound.  Kept: the optimiser's algorithm and host
decisions, the closure arithmetic and the best-iterate rule.  Dropped because they cannot change a result:
  * the `loss.backward()` before every LBFGS.step (attack_PCFA.py:173) -- the closure's
    zero_grad() discards its gradient before anything reads it;
  * the autograd graph of the re-prediction forward (only metrics read it) -> torch.no_grad();
  * torch.autograd.set_detect_anomaly, the per-forward `.cpu()` round trip, mlflow.

Multi-GPU (one process per GPU, torch.distributed over RCCL): independent pairs are sharded
round-robin over ranks with no collective in the data path (`attack_l2`); the universal attack
is data parallel over the batch with ONE all-reduce of d(loss)/d(delta) per closure
(`attack_l2_universal`), see pcfa_amd/sharding.py.
"""
import contextlib
import os
import time

import numpy as np
import torch

from . import _hip, config, graph_sets, ops, sharding
from .graph_sets import _log_eviction
from .helper_functions import datasets, logging, losses, ownutilities, parsing_file, pictures, targets
from .helper_functions.config_paths import Conf

EPS_BOX = 1e-7  # attack_PCFA.py:608


def extract_deltas(nw_input1, nw_input2, image1, image2, boxconstraint, eps_box=0.):
    """delta_i = box(nw_input_i) - image_i (attack_PCFA.py:20-29)."""
    return ops.get().extract_deltas(nw_input1, nw_input2, image1, image2, boxconstraint, eps_box=eps_box)


def extract_deltas_joint(nw_delta, images_max, images_min):
    """Two-sided clamp of a shared perturbation against both frames (attack_PCFA.py:32-37)."""
    return ops.get().extract_deltas_joint(nw_delta, images_max, images_min)


def default_mu(args):
    """attack_PCFA.py:578-584."""
    optim_mu = args.mu
    if optim_mu == -1.:
        optim_mu = 2500. / args.delta_bound
        if args.target not in ['zero']:
            optim_mu = 1.5 * optim_mu
    return optim_mu


def select_device():
    """attack_PCFA.py:631-634."""
    if Conf.config('useCPU') or not torch.cuda.is_available():
        return torch.device("cpu")
    if torch.distributed.is_available() and torch.distributed.is_initialized():
        return torch.device("cuda", sharding.local_rank())
    return torch.device("cuda")


def _should_save(batch, args):
    return ((batch % args.save_frequency == 0 and not args.small_save) or (args.small_save and batch < 32)) \
        and not args.no_save


def best_iterate_rule(below_threshold, l2_delta12, aee_adv_tgt, delta12_min, aee_adv_tgt_min, delta_bound):
    """The best-iterate rule (attack_PCFA.py:226-243): until an iterate has met the bound the smallest perturbation wins
    (ties: the smaller AEE to the target); from then on the smallest AEE to the target among the iterates inside the bound.
    Returns (record this iterate, an iterate has met the bound)."""
    if below_threshold:
        return l2_delta12 <= delta_bound and aee_adv_tgt < aee_adv_tgt_min, True
    if l2_delta12 < delta12_min or (l2_delta12 == delta12_min and aee_adv_tgt < aee_adv_tgt_min):
        return True, l2_delta12 <= delta_bound
    return False, False


def _graphs_enabled(device, args):
    return torch.device(device).type == "cuda" and os.environ.get("PCFA_HIP_GRAPH", "1") == "1" and args.steps > 0


def _max_cached_shapes(model):
    """Graph sets kept per model and lane (graph_sets.put) and batch states per universal attack, from the model's Config
    (default 4; KITTI under /8 padding alone has three padded shapes)."""
    return config.cfg(model).max_cached_shapes


class _ItemRecord:
    """What an attack keeps per pair besides the variables: the pair's dataset index, the constant metrics, the last step's
    metrics and the best iterate."""

    def __init__(self, batch):
        self.batch = batch
        self.aee_gt = self.aee_tgt = self.aee_gt_tgt = None
        self.delta_below_threshold = False
        self.delta12_min_val = float('inf')
        self.aee_adv_tgt_min_val = float('inf')
        self.aee_adv_pred_min_val = 0.
        self.delta1_min = self.delta2_min = self.flow_pred_min = None
        self.aee_adv_gt = 0.
        self.aee_adv_tgt = self.aee_adv_pred = 0.
        self.l2_delta1 = self.l2_delta2 = self.l2_delta12 = 0.

    def record(self, curr_step, delta_bound, aee_adv_tgt, aee_adv_pred, aee_adv_gt, l2_delta1, l2_delta2, l2_delta12,
               delta1, delta2, flow_pred):
        """One step's metrics (host floats) of this pair and the tensors they were computed from: logged under the
        reference's names, and kept as the best iterate where the rule says so (attack_PCFA.py:199-243).  Returns the
        step's (aee_adv_tgt, aee_adv_pred, l2_delta12)."""
        self.aee_adv_tgt, self.aee_adv_pred, self.aee_adv_gt = aee_adv_tgt, aee_adv_pred, aee_adv_gt
        self.l2_delta1, self.l2_delta2, self.l2_delta12 = l2_delta1, l2_delta2, l2_delta12
        logging.log_metrics(curr_step, ("aee_predadv-tgt", aee_adv_tgt), ("aee_pred-predadv", aee_adv_pred),
                            ("aee_predadv-gt", aee_adv_gt))
        logging.log_metrics(curr_step, ("l2_delta1", l2_delta1), ("l2_delta2", l2_delta2),
                            ("l2_delta-avg", l2_delta12))
        update_minima, self.delta_below_threshold = best_iterate_rule(
            self.delta_below_threshold, l2_delta12, aee_adv_tgt, self.delta12_min_val, self.aee_adv_tgt_min_val,
            delta_bound)
        if update_minima:
            self.delta12_min_val = l2_delta12
            self.aee_adv_tgt_min_val = aee_adv_tgt
            self.aee_adv_pred_min_val = aee_adv_pred
            self.delta1_min = delta1.detach().clone()
            self.delta2_min = delta2.detach().clone()
            self.flow_pred_min = flow_pred.detach().clone()
        logging.log_metrics(curr_step, ("aee_pred-tgt_min", self.aee_adv_tgt_min_val),
                            ("l2_delta-avg_min", self.delta12_min_val),
                            ("aee_pred-predadv_min", self.aee_adv_pred_min_val))
        return aee_adv_tgt, aee_adv_pred, l2_delta12

    def as_tuple(self):
        """The reference's 12-tuple (attack_PCFA.py:294)."""
        return (self.aee_gt, self.aee_tgt, self.aee_gt_tgt, self.aee_adv_gt, self.aee_adv_tgt, self.aee_adv_pred,
                self.l2_delta1, self.l2_delta2, self.l2_delta12, self.aee_adv_tgt_min_val,
                self.aee_adv_pred_min_val, self.delta12_min_val)


class _AttackState:
    """What PairAttack and PairBatch share: the variables of `len(self.rec)` image pairs stacked along the batch dimension,
    the static buffers their closure reads, the target(s), the closure and its capture, and the graph set the next pair(s)
    of the same key adopt (graph_sets).  A class adds its record(s) `rec`, `closure_body`, its optimiser, the constant
    metrics and `step()`.

    On the GPU the closure (static shapes, variables updated in place by L-BFGS) and the re-prediction forward are captured
    once per key into hipGraphs and replayed (`use_graph=None`: on for CUDA devices unless PCFA_HIP_GRAPH=0; if capture
    fails the eager closure -- the same kernels in the same order -- is used and a warning is logged).  A pair of the same
    shape and flags as an earlier one copies its images / initial variables / target into that pair's buffers and resets
    the optimiser -- no warm-up, no re-capture (`reuse_graphs`, default Config.reuse_pair_graphs; results equal a fresh
    capture: tests/test_gpu_parity.py::test_pair_graph_reuse_equals_fresh_capture)."""

    CACHE = None      # the key of graph_sets.CACHES under which this class keeps its graph sets
    KEPT = ("image1", "image2", "images_max", "images_min", "params", "target", "optimizer", "graphed", "repredict")

    def __init__(self, model, image1, image2, flow, eps_box, device, has_gt, optim_mu, args, use_graph, reuse_graphs,
                 key_tail=(), adopt=True, trace=None):
        self.model, self.args, self.device = model, args, device
        self.trace = trace   # a pcfa_amd.trace.ClosureTrace: every closure evaluation leaves its operators' digests there
        if trace is not None:
            adopt = False    # a traced closure's graphs hold digest launches: it neither adopts a graph set nor leaves one
        self.has_gt, self.optim_mu, self.eps_box = has_gt, optim_mu, eps_box
        if reuse_graphs is None:   # pairs of one shape share static buffers + hipGraphs unless the model's config says no
            reuse_graphs = config.cfg(model).reuse_pair_graphs
        self.reuse_graphs = reuse_graphs
        items = len(self.rec)

        image1, image2 = image1.to(device), image2.to(device)
        self.flow_gt = flow.to(device) if flow is not None else None
        if not ownutilities.model_takes_unit_input(args.net):
            image1 = image1 / 255.
            image2 = image2 / 255.
        self.padder, [image1, image2] = ownutilities.preprocess_img(args.net, image1, image2)
        cov = args.boxconstraint in ['change_of_variables']
        joint = bool(args.joint_perturbation)
        if joint and cov:
            raise ValueError("Training a --joint_perturbation with --boxconstraint=change_of_variables is not "
                             "defined. Please use --boxconstraint=clipping.")
        if use_graph is None:
            use_graph = _graphs_enabled(device, args)
        self.lane = ops.core.current_lane()
        self.graph_key = (args.net, (image1.shape[0] // items,) + tuple(image1.shape[1:]), args.boxconstraint, joint,
                          args.loss, float(optim_mu), float(args.delta_bound), float(eps_box), str(device),
                          self.lane) + key_tail
        self.retired = False

        # the static buffers: an earlier pair's of the same key (with its graphs and optimiser; that pair is retired), or new
        kept = graph_sets.adopt(self._graph_sets(), self.graph_key, self) if (use_graph and reuse_graphs and adopt) else None
        self.graphs_reused = kept is not None
        if kept is not None:
            self.optimizer.reset()
        else:
            self.image1, self.image2 = torch.empty_like(image1), torch.empty_like(image2)
            self.images_max, self.images_min = torch.empty_like(image1), torch.empty_like(image1)
            self.params = [torch.zeros_like(image1).requires_grad_() for _ in range(1 if joint else 2)]
            self.target = None
            self.optimizer = self._make_optimizer()
            self.graphed = self.repredict = None
        with torch.no_grad():
            self.image1.copy_(image1)
            self.image2.copy_(image2)
            self.images_max.copy_(torch.max(image1, image2))
            self.images_min.copy_(torch.min(image1, image2))
            if joint:
                self.params[0].zero_()
            elif cov:
                self.params[0].copy_(torch.atanh(2. * (1. - eps_box) * image1 - (1 - eps_box)))
                self.params[1].copy_(torch.atanh(2. * (1. - eps_box) * image2 - (1 - eps_box)))
            else:
                self.params[0].copy_(image1)
                self.params[1].copy_(image2)
        for p_ in self.params:
            p_.grad = None
        if joint:
            self.nw_delta = self.params[0]
            self.nw_input1, self.nw_input2 = self.image1, self.image2
            self.fwd_kwargs = {"delta1": self.nw_delta}
        else:
            self.nw_delta = None
            self.nw_input1, self.nw_input2 = self.params
            self.fwd_kwargs = {}

        # the unattacked flow (the forward at the initial variables) and, from it, every pair's own target
        if self.repredict is not None:
            _, flow0 = self.repredict()
        else:
            with torch.no_grad():
                flow0 = self.predict()
        self.flow_pred_init = flow0.detach().clone()
        target = [targets.get_target(args.target, self._item(self.flow_pred_init, b),
                                     custom_target_path=args.custom_target_path, device=device).to(device)
                  for b in range(items)]
        target = target[0] if items == 1 else torch.cat(target)
        if self.target is None:
            self.target = target
        else:
            self.target.copy_(target)
        self.target.requires_grad = False

        for r, const in zip(self.rec, self._constant_metrics()):
            r.aee_tgt = const[0]
            if has_gt:
                r.aee_gt_tgt, r.aee_gt = const[1:]
            curr_step = r.batch * args.steps
            logging.log_metrics(curr_step, ("aee_pred-tgt", r.aee_tgt), ("aee_gt-tgt", r.aee_gt_tgt),
                                ("aee_pred-gt", r.aee_gt))
            logging.log_metric(key="optim_mu", value=optim_mu, step=curr_step)
        model.zero_grad()

        self.flow_pred = self.flow_pred_init
        self.delta1, self.delta2 = torch.zeros_like(self.image1), torch.zeros_like(self.image2)
        self.steps_done = 0
        self.closures = 0          # evaluations of the closure (each one is a closure evaluation of every item)
        self._pictured = set()     # items whose pictures --save_png has written
        if use_graph and kept is None:
            self.enable_graph()

    def _graph_sets(self):
        return graph_sets.cache(self.model, self.CACHE)

    def _item(self, tens, b):
        """Pair b's rows of a tensor stacked over the pairs."""
        n = tens.shape[0] // len(self.rec)
        return tens[b * n:(b + 1) * n]

    # ---- pieces of the closure (attack_PCFA.py:175-192) ---------------------------------------------------------
    def predict(self):
        out = ownutilities.compute_flow(self.model, "scaled_input_model", self.nw_input1, self.nw_input2,
                                        test_mode=True, **self.fwd_kwargs)
        [out] = ownutilities.postprocess_flow(self.args.net, self.padder, out)
        return out

    def current_deltas(self):
        if self.args.joint_perturbation:
            return extract_deltas_joint(self.nw_delta, self.images_max, self.images_min)
        return extract_deltas(self.nw_input1, self.nw_input2, self.image1, self.image2, self.args.boxconstraint,
                              eps_box=self.eps_box)

    def _repredict_body(self):
        return self.current_deltas(), self.predict()

    def enable_graph(self, **how):
        try:
            self._capture(**how)
        except Exception as e:  # noqa: BLE001 -- the eager closure launches the same kernels in the same order
            import logging as pylog
            pylog.warning("hipGraph capture of the closure failed (%r): launching eagerly", e)
            self.graphed = self.repredict = None

    def _capture(self):
        from .graphed import GraphedClosure, GraphedForward
        sink = getattr(self.optimizer, "flat_grad_views", None)
        self.graphed = GraphedClosure(self.closure_body, self.params, grad_sink=sink() if sink else None)
        self.repredict = GraphedForward(self._repredict_body, self.device)
        if self.reuse_graphs and self.trace is None and hasattr(self.optimizer, "reset"):   # the next pair of this key adopts them
            graph_sets.put(self._graph_sets(), self.graph_key, graph_sets.GraphSet(self, self.lane, self.KEPT),
                           _max_cached_shapes(self.model), self.CACHE)

    def _retire(self):
        """A later pair of the same key took over this one's static buffers, graphs and optimiser (or the set was evicted
        from the per-model cache): results recorded so far stay readable, further evaluation raises."""
        self.retired = True
        self.graphed = self.repredict = None

    def _check_live(self):
        if self.retired:
            raise RuntimeError("this %s was retired: a later one of the same shape adopted its static buffers, graphs and "
                               "optimiser (one live attack per shape, model and lane; reuse_graphs=False keeps pairs "
                               "independent)" % type(self).__name__)

    def closure(self):
        self._check_live()
        self.closures += 1
        if self.graphed is not None:
            loss = self.graphed()
        else:
            for p_ in self.params:
                p_.grad = None
            loss = self.closure_body()
        if self.trace is not None:   # (the warm-up and capture evaluations do not come through here)
            self.trace.keep(self.closures - 1, step=self.steps_done)
        return loss

    # ---- one `--steps` iteration (attack_PCFA.py:155-247) -------------------------------------------------------
    def _optimise(self):
        """The optimiser's step (10 closure evaluations) and the re-prediction at the new variables; returns the number of
        steps done before and the new (delta1, delta2, flow_pred).  The class's `step()` adds the metrics."""
        self._check_live()
        steps = self.steps_done
        for r in self.rec:
            logging.log_metrics(r.batch * self.args.steps + steps, ("batch", r.batch), ("steps", steps), ("epoch", 0))

        self.optimizer.step(self.closure)

        if self.repredict is not None:
            (delta1, delta2), flow_pred = self.repredict()
        else:
            with torch.no_grad():
                (delta1, delta2), flow_pred = self._repredict_body()
        self.delta1, self.delta2, self.flow_pred = delta1, delta2, flow_pred
        return steps, delta1, delta2, flow_pred

    def save(self, distortion_folder, b=0):
        r = self.rec[b]
        for tens, name in ((self._item(self.delta1, b), "delta1_final"), (self._item(self.delta2, b), "delta2_final"),
                           (r.delta1_min, "delta1_best"), (r.delta2_min, "delta2_best"),
                           (self._item(self.image1, b), "image1"), (self._item(self.image2, b), "image2"),
                           (self._item(self.target, b), "target"), (self._item(self.flow_pred, b), "flow_pred_final"),
                           (r.flow_pred_min, "flow_pred_best"), (self._item(self.flow_pred_init, b), "flow_pred_init")):
            logging.save_tensor(tens, name, r.batch, distortion_folder)
        if self.has_gt:
            logging.save_tensor(self._item(self.flow_gt, b), "flow_gt", r.batch, distortion_folder)
        if getattr(self.args, "save_png", False):
            self._save_pictures(distortion_folder, b)

    def _save_pictures(self, distortion_folder, b):
        """`--save_png`: the pictures of attack_PCFA.py:267-292, for ALL pairs of this state at the first pair saved: every
        conversion is one launch over the items.  Launches and device-to-host copies are queued on the current stream
        inside save() -- the stream the pair ran on; under --pairs_in_flight the driver makes the lane's stream current
        (PairsInFlight.on_lane) -- so stream order keeps them ahead of the uploads of the next pair(s) that adopt the static
        buffers."""
        if b in self._pictured:
            return
        items = [i for i in range(len(self.rec)) if _should_save(self.rec[i].batch, self.args)]
        self._pictured.update(items)
        everyone = len(items) == len(self.rec)

        def pick(t):   # the rows of the pairs that are saved
            if t is None:
                return None
            return t.detach() if everyone else torch.cat([self._item(t, i).detach() for i in items])

        def best(name, last):   # the best iterate; a pair that never took a step has only its last (= initial) state
            return torch.cat([self._item(last, i).detach() if getattr(self.rec[i], name) is None
                              else getattr(self.rec[i], name) for i in items])

        d1, d2 = best("delta1_min", self.delta1), best("delta2_min", self.delta2)
        flow_best = best("flow_pred_min", self.flow_pred)
        image1, image2 = pick(self.image1), pick(self.image2)
        flow_init, flow_gt = pick(self.flow_pred_init), pick(self.flow_gt) if self.has_gt else None
        joint = bool(self.args.joint_perturbation)
        ps = pictures.PictureSet()
        logging.save_attack_pictures(
            ps, [self.rec[i].batch for i in items], distortion_folder,
            images=(("image1", image1, None), ("image2", image2, None), ("image1_delta_best", image1, d1),
                    ("image2_delta_best", image2, d2)),
            deltas=(("delta1_best", d1), (None if joint else "delta2_best", d2)),
            flows=(("flow_pred_best", flow_best), ("flow_pred_init", flow_init), ("flow_target", pick(self.target)),
                   ("flow_gt", flow_gt)),
            flow_scale=logging.flow_picture_scale(getattr(self.args, "png_flow_scale", "own"),
                                                  (flow_gt, flow_init, flow_best)))
        ps.write()

    def result(self, b=0):
        """Pair b's 12-tuple (attack_PCFA.py:294)."""
        return self.rec[b].as_tuple()


class PairAttack(_AttackState, _ItemRecord):
    """Everything pcfa_attack holds for ONE image pair (attack_PCFA.py:40-247): the optimisation variables,
    the optimiser, the target, the best-iterate bookkeeping (the pair is its own record) -- and `step()`, the body of the
    `--steps` loop.

    `pcfa_attack` is `PairAttack(...)` + `args.steps` x `step()`; bench.py times `step()` of this class, so the
    measured loop IS the product loop.  Capture and graph-set reuse: _AttackState."""

    CACHE = "pair-graph"
    rec = property(lambda self: (self,))

    def __init__(self, model, image1, image2, flow, batch, eps_box, device, has_gt, optim_mu, args, use_graph=None,
                 reuse_graphs=None, trace=None):
        _ItemRecord.__init__(self, batch)
        _AttackState.__init__(self, model, image1, image2, flow, eps_box, device, has_gt, optim_mu, args, use_graph,
                              reuse_graphs, adopt=os.environ.get("PCFA_SHARED_FORWARD", "0") != "1", trace=trace)

    def _make_optimizer(self):
        return ops.get().LBFGS(self.params, max_iter=10)

    def _constant_metrics(self):
        const = (logging.calc_metrics_const(self.target, self.flow_pred_init),)
        if self.has_gt:
            const += logging.calc_metrics_const_gt(self.target, self.flow_pred_init, self.flow_gt)
        return [const]

    def _forward_with_loss(self):
        """closure_body without the backward: (loss, ((delta1, delta2), flow)) -- see graphed.SplitGraphedClosure."""
        flow = self.predict()
        d1, d2 = self.current_deltas()
        loss = losses.loss_delta_constraint(flow, self.target, d1, d2, self.device, delta_bound=self.args.delta_bound,
                                            mu=self.optim_mu, f_type=self.args.loss)
        return loss, ((d1, d2), flow)

    def closure_body(self):
        if self.trace is not None:
            return self._traced_closure_body()
        loss_closure, _ = self._forward_with_loss()
        loss_closure.backward()
        return loss_closure

    def _traced_closure_body(self):
        """closure_body inside one pass of the trace -- warm-up, capture and eager evaluation alike, so the digest launches
        are captured with the closure -- closed by the digests of the loss and of the variables' gradients."""
        with self.trace.recording() as tr:
            loss_closure, _ = self._forward_with_loss()
            loss_closure.backward()
            tr.record("closure loss", loss_closure.detach().reshape(1))
            for i, p_ in enumerate(self.params):
                tr.record("closure grad of variable %d %s" % (i, tuple(p_.shape)), p_.grad)
        return loss_closure

    def _capture(self, share_forward=None):
        """share_forward (default: PCFA_SHARED_FORWARD=1, off otherwise): capture the closure as forward + backward graphs
        and let the re-prediction after a step double as the forward of the next step's first closure evaluation (such a
        pair never enters the graph-set cache)."""
        if share_forward is None:
            share_forward = os.environ.get("PCFA_SHARED_FORWARD", "0") == "1"
        if not share_forward:
            return super()._capture()
        if self.trace is not None:
            raise ValueError("a traced PairAttack captures its closure as one graph: not with PCFA_SHARED_FORWARD=1")
        from .graphed import SplitGraphedClosure
        split = SplitGraphedClosure(self._forward_with_loss, self.params)
        self.graphed = split

        def repredict():
            _, ((d1, d2), flow) = split.forward()
            return (d1.detach(), d2.detach()), flow.detach()
        self.repredict = repredict

    def step(self):
        steps, delta1, delta2, flow_pred = self._optimise()
        aee_adv_tgt, aee_adv_pred = logging.calc_metrics_adv(flow_pred, self.target, self.flow_pred_init)
        aee_adv_gt = logging.calc_metrics_adv_gt(flow_pred, self.flow_gt) if self.has_gt else None
        curr_step = self.batch * self.args.steps + steps
        l2_delta1, l2_delta2, l2_delta12 = logging.calc_delta_metrics(delta1, delta2, curr_step)
        out = self.record(curr_step, self.args.delta_bound, aee_adv_tgt, aee_adv_pred, aee_adv_gt, l2_delta1, l2_delta2,
                          l2_delta12, delta1, delta2, flow_pred)
        self.steps_done += 1
        return out


def _trace_folder(args):
    """--trace_digests DIR (pcfa_amd.trace), refused where no per-pair closure exists to trace."""
    folder = getattr(args, "trace_digests", "") or ""
    if folder and max(1, int(getattr(args, "pairs_per_closure", 1))) > 1:
        raise ValueError("--trace_digests records one pair's closure: not with --pairs_per_closure > 1")
    if folder and getattr(args, "universal_perturbation", False):
        raise ValueError("--trace_digests records one pair's closure: not with --universal_perturbation")
    return folder


def _new_trace(model, device, args):
    """The recorder of one pair under --trace_digests (None without the flag): room for every closure evaluation that
    `--steps` L-BFGS steps can ask for."""
    if not _trace_folder(args):
        return None
    from .trace import ClosureTrace
    return ClosureTrace(model, device, max_closures=max(1, args.steps) * 10 * 5 // 4)


def _save_trace(st, args):
    if st.trace is not None:
        st.trace.save(os.path.join(_trace_folder(args), "%05d_trace.npz" % st.batch))
        st.trace.close()


def pcfa_attack(model, image1, image2, flow, batch, distortion_folder, eps_box, device, has_gt, optim_mu, args,
                statistics_in_every_step=True):
    """Attack one image pair; returns the reference's 12-tuple (attack_PCFA.py:40-294; with `--steps 0` its initial zeros
    for the adversarial statistics)."""
    st = PairAttack(model, image1, image2, flow, batch, eps_box, device, has_gt, optim_mu, args,
                    trace=_new_trace(model, device, args))
    for _ in range(args.steps):
        st.step()
    _save_trace(st, args)
    if distortion_folder is not None and _should_save(batch, args):
        st.save(distortion_folder)
    return st.result()


class PairBatch(_AttackState):
    """B independent PairAttacks whose closure evaluations are ONE forward and backward at batch B, on one stream, in one
    graph: per item its own variables, target (from its own unattacked flow), L-BFGS state (lbfgs.BatchedLBFGS) and
    best-iterate record.  Pair b's variables enter only pair b's loss term, so the gradient of the summed loss with respect
    to them is exactly that pair's own gradient (ops.loss_delta_constraint_items); what differs from attacking the pair
    alone is the rounding of the network's kernels at batch B (and, under the fixed-point scatters, a shift shared by the
    batch).  With B = 1 every bit equals PairAttack's.

    pairs: B x (batch, image1 [1,3,H,W], image2, flow or None), all of one shape.  `step()` = BatchedLBFGS.step, one
    re-prediction at batch B, the per-item metrics from one launch each and one read-back.  Item b's metrics are logged
    under its own `batch * steps + step`; `result(b)` is its 12-tuple, `save(folder, b)` writes its artefacts.  The graph
    sets live in a cache of their own on the model, keyed by PairAttack's key + (B,)."""

    CACHE = "pair-batch-graph"

    def __init__(self, model, pairs, eps_box, device, has_gt, optim_mu, args, use_graph=None):
        self.items = B = len(pairs)
        self.rec = [_ItemRecord(batch) for batch, _, _, _ in pairs]
        shapes = {tuple(p[1].shape) for p in pairs} | {tuple(p[2].shape) for p in pairs}
        if len(shapes) != 1 or next(iter(shapes))[0] != 1:
            raise ValueError("PairBatch: every pair is two [1,3,H,W] images of one shape, got %s" % sorted(shapes))
        super().__init__(model, torch.cat([p[1] for p in pairs]), torch.cat([p[2] for p in pairs]),
                         torch.cat([p[3] for p in pairs]) if has_gt else None, eps_box, device, has_gt, optim_mu, args,
                         use_graph, None, key_tail=(B,))

    def _make_optimizer(self):
        return ops.get().BatchedLBFGS(self.params, items=self.items, max_iter=10)

    def _constant_metrics(self):
        om = ops.get()
        const = [om.avg_epe_items(self.target, self.flow_pred_init)]
        if self.has_gt:
            const += [om.avg_epe_items(self.target, self.flow_gt), om.avg_epe_items(self.flow_pred_init, self.flow_gt)]
        return zip(*torch.stack(const).tolist())

    def closure_body(self):
        """Forward at batch B, the per-item losses, ONE backward of their sum; returns the B losses."""
        flow = self.predict()
        d1, d2 = self.current_deltas()
        total, item_losses = ops.get().loss_delta_constraint_items(flow, self.target, d1, d2,
                                                                   delta_bound=self.args.delta_bound, mu=self.optim_mu,
                                                                   f_type=self.args.loss)
        total.backward()
        return item_losses

    def step(self):
        """One `--steps` iteration for every item; returns B x (aee_adv_tgt, aee_adv_pred, l2_delta12)."""
        steps, delta1, delta2, flow_pred = self._optimise()
        args, om = self.args, ops.get()
        # the metrics of PairAttack.step per item (logging.calc_metrics_adv, calc_delta_metrics: the same fp32 operations
        # on B values at once), one read-back for all of them
        n1, n2 = delta1[0].numel(), delta2[0].numel()
        ss1 = om.sum_squares_items(delta1)
        ss2 = ss1 if delta2 is delta1 else om.sum_squares_items(delta2)
        rows = [om.avg_epe_items(flow_pred, self.target), om.avg_epe_items(flow_pred, self.flow_pred_init),
                torch.sqrt(ss1) / (n1 ** 0.5), torch.sqrt(ss2) / (n2 ** 0.5), torch.sqrt(ss1 + ss2) / ((n1 + n2) ** 0.5)]
        if self.has_gt:
            rows.append(om.avg_epe_items(flow_pred, self.flow_gt))
        rows = torch.stack(rows).tolist()
        out = [r.record(r.batch * args.steps + steps, args.delta_bound, rows[0][b], rows[1][b],
                        rows[5][b] if self.has_gt else None, rows[2][b], rows[3][b], rows[4][b],
                        delta1[b:b + 1], delta2[b:b + 1], flow_pred[b:b + 1]) for b, r in enumerate(self.rec)]
        self.steps_done += 1
        return out


def group_pairs(stream, per_closure, shape_of):
    """Collect a stream of pairs, in arrival order, into groups of equal `shape_of(pair)` with up to `per_closure` members:
    yields a group as soon as it is full and the incomplete ones, oldest first, at the end.  (attack_l2 groups by the
    image shape: the members of a PairBatch share one padder, so equal padded shapes alone would not do.)"""
    open_groups = {}
    for pair in stream:
        key = shape_of(pair)
        group = open_groups.setdefault(key, [])
        group.append(pair)
        if len(group) == per_closure:
            yield open_groups.pop(key)
    for group in open_groups.values():
        yield group


def _load_model(args, device, variable_change):
    model_takes_unit_input = ownutilities.model_takes_unit_input(args.net)
    kwargs = {"weights": getattr(args, "weights", "pretrained")}
    if variable_change:
        kwargs["eps_box"] = EPS_BOX
    model = ownutilities.import_and_load(args.net, make_unit_input=not model_takes_unit_input,
                                         variable_change=variable_change, make_scaled_input_model=True,
                                         device=device, **kwargs)
    model.eval()
    for param in model.parameters():
        param.requires_grad = False
    return model


def _output_folder(args, tag):
    if args.no_save:
        return None
    stamp = time.strftime("%Y-%m-%d_%H:%M:%S")
    kind = "%s_PCFA_%s_%s" % (args.net, "cd" if args.joint_perturbation else "dd",
                              "u" if args.universal_perturbation else "-")
    folder = os.path.join(args.output_folder, kind, stamp + tag)
    return logging.create_subfolder(folder, "patches")


class PairsInFlight:
    """Several independent image pairs attacked SIDE BY SIDE on one GPU (attack_PCFA.py:668-670 loops over pairs one after
    the other; the pairs share nothing but the frozen weights).

    (The lane travels with the STREAM, not with the host thread: autograd runs backward nodes on a thread of its own.)
    At one pair per GPU every launch of the 55 x 128 feature maps is 1-2 workgroups per CU and ends in a tail; a second
    pair's launches fill the idle CUs.  Lane k = one host thread + one HIP stream + one set of static buffers, hipGraphs
    and L-BFGS state (`ops.core.lane(k)` keys every shared scratch buffer and the per-model graph cache), so the lanes
    never touch each other's memory and each pair's arithmetic is exactly the solo run's: results are bit-identical to
    attacking the pairs one after the other (tests/test_gpu_parity.py::test_pairs_in_flight_bit_identical_to_solo).

    make_attack(k) -> PairAttack is called in the caller's thread, one lane after the other (weight packs and graph
    captures are built sequentially); `run(steps)` then drives every lane's `step()` from its own thread."""

    def __init__(self, make_attack, n, device):
        self.device = torch.device(device)
        if self.device.index is None:      # "cuda": the caller's current device (a new host thread starts on device 0)
            self.device = torch.device("cuda", torch.cuda.current_device())
        self.streams = ops.core.lane_run_streams(self.device, n)   # (not torch.cuda.Stream(): a pool of 32 shared objects)
        self.attacks = []
        for k in range(n):
            with ops.core.lane(k), torch.cuda.stream(self.streams[k]):
                self.attacks.append(make_attack(k))
            torch.cuda.synchronize(self.device)
            if k == 0 and n > 1:
                self._refuse_shared_library_workspaces(self.attacks[0])

    @staticmethod
    def _refuse_shared_library_workspaces(attack):
        """GMA's attention products run on rocBLAS by default (Config.gma_gemm = "lib").  Every graph of this
        process is captured by ONE host thread, i.e. with one rocBLAS handle, and a handle owns ONE device workspace that
        all its launches share in stream order -- replayed side by side, two lanes' products use it at the same time.
        Observed (r05, tools/dev/flight_scaling.py GMA 436x1024, two lanes): the first step never returns.  The package's own
        products take their split-K scratch from the caller, so the build with gma_gemm = "hip" is safe in flight, and so is
        gma_attention = "streamed" (own kernels, no scratch at all) whatever gma_gemm says; likewise
        SpyNet with spynet_ops = "hip" (own 7x7 convolutions and warp, no scratch shared between lanes) and FlowNet2 with
        flownet2_ops = "hip" (own strided / transposed convolutions, no library kernel in the closure)."""
        net = getattr(getattr(attack, "args", None), "net", None)
        if net == "FlowNet2" and config.cfg(attack.model).flownet2_ops != "hip":
            # the default build keeps library convolutions (the strided and transposed ones): never validated in flight --
            # refused rather than left to chance
            raise ValueError("FlowNet2 with Config.flownet2_ops='lib' keeps library convolutions inside its captured closure "
                             "and cannot run several pairs in flight: build the model with flownet2_ops='hip' "
                             "(PCFA_FLOWNET2_OPS=hip) or use --pairs_in_flight 1")
        if net == "SpyNet" and config.cfg(attack.model).spynet_ops != "hip":
            # the default build runs Basic's 7x7 layers on MIOpen; the spynet_ops = "hip" build holds no library kernel
            raise ValueError("SpyNet with Config.spynet_ops='lib' keeps library convolutions inside its captured closure and "
                             "cannot run several pairs in flight: build the model with spynet_ops='hip' "
                             "(PCFA_SPYNET_OPS=hip) or use --pairs_in_flight 1")
        if net == "GMA" and config.cfg(attack.model).gma_attention == "streamed":
            return   # no attention product goes to rocBLAS, and the streamed kernels take no scratch shared between lanes
        if net == "GMA" and config.cfg(attack.model).gma_gemm != "hip":
            raise ValueError("GMA with Config.gma_gemm='lib' cannot run several pairs in flight (the lanes' captured rocBLAS "
                             "products would share one handle's workspace): build the model with gma_gemm='hip' "
                             "(PCFA_GMA_GEMM=hip) or use --pairs_in_flight 1")

    @contextlib.contextmanager
    def on_lane(self, k):
        """The caller's thread as lane k: its scratch keys and its stream current.  What touches a lane's static buffers
        after run() -- save() with its picture conversions and copies -- is queued here, so that stream order keeps it ahead
        of the uploads of the next pair that adopts those buffers on the same stream."""
        with ops.core.lane(k), torch.cuda.stream(self.streams[k]):
            yield self.attacks[k]

    def run(self, steps):
        """`steps` attack steps on every lane, concurrently; returns each lane's last (aee_adv_tgt, aee_adv_pred, l2)."""
        import threading
        last, errors = [None] * len(self.attacks), []
        start = threading.Barrier(len(self.attacks))

        def drive(k):
            try:
                torch.cuda.set_device(self.device)       # the current device is per host thread
                with ops.core.lane(k), torch.cuda.stream(self.streams[k]):
                    start.wait()
                    for _ in range(steps):
                        last[k] = self.attacks[k].step()
                    self.streams[k].synchronize()
            except BaseException as e:  # noqa: BLE001 -- re-raised in the caller's thread
                errors.append(e)
                start.abort()
        threads = [threading.Thread(target=drive, args=(k,), name="pcfa-lane-%d" % k) for k in range(len(self.attacks))]
        for t in threads:
            t.start()
        for t in threads:
            t.join()
        if errors:
            raise errors[0]
        return last


def _hardware_queues_for(nflight):
    """Kernels of two lanes overlap only if their streams sit on different hardware queues, and the HIP runtime makes four
    per device unless GPU_MAX_HW_QUEUES says otherwise when it initialises.  Up to three pairs in flight that is enough; the
    fourth lane shares a queue (RAFT, four pairs: 9.65 pair-steps/s with 4 queues, 10.73 with 8;
    profiles/r05/pairs_in_flight_scaling.txt).  So ask for 8 -- which only works before the process first touches the GPU."""
    if nflight < 4 or "GPU_MAX_HW_QUEUES" in os.environ:
        return
    if torch.cuda.is_initialized():
        print("--pairs_in_flight %d: the GPU runtime is already initialised with its default of 4 hardware queues; export "
              "GPU_MAX_HW_QUEUES=8 before starting for the fourth lane to overlap" % nflight)
        return
    os.environ["GPU_MAX_HW_QUEUES"] = "8"


def _result_row(batch, result):
    """The 13-wide row attack_l2 gathers for one pair: its index and its 12-tuple, what does not exist (no ground truth) as
    NaN."""
    return (batch,) + tuple(float('nan') if v is None else float(v) for v in result)


def attack_l2(args, data_loader=None, has_gt=None):
    """PCFA on every pair of a dataset, one perturbation (pair) per image pair (attack_PCFA.py:570-701).

    With torch.distributed initialised, pair i is attacked on rank i % world_size and rank 0
    receives every pair's result tuple; there is no collective inside the attack.
    Returns the dict of averaged metrics (also logged under the reference's metric names).
    """
    _trace_folder(args)
    optim_mu = default_mu(args)
    rank, world = sharding.rank(), sharding.world_size()
    distortion_folder = _output_folder(args, "_r%d" % rank if world > 1 else "")
    if data_loader is None:
        data_loader, has_gt = datasets.prepare_dataloader(args, batch_size=1, shuffle=False)
    _hardware_queues_for(max(1, int(getattr(args, "pairs_in_flight", 1))))
    device = select_device()
    cov = args.boxconstraint in ['change_of_variables']
    model = _load_model(args, device, variable_change=cov)

    local = []
    nflight = max(1, int(getattr(args, "pairs_in_flight", 1)))
    if nflight > 1 and torch.device(device).type != "cuda":
        raise ValueError("--pairs_in_flight needs a GPU (lanes are HIP streams)")
    per_closure = max(1, int(getattr(args, "pairs_per_closure", 1)))
    if per_closure > 1 and nflight > 1:
        raise ValueError("--pairs_per_closure and --pairs_in_flight are two ways to put several pairs on one GPU: "
                         "use one of them")
    if per_closure > 1 and torch.device(device).type != "cuda":
        raise ValueError("--pairs_per_closure needs a GPU (the batched optimiser has no CPU path)")
    if per_closure > _hip.MAX_ITEMS:
        raise ValueError("--pairs_per_closure: at most %d pairs per closure" % _hip.MAX_ITEMS)
    pending = []   # (batch, image1, image2, flow) of this rank, attacked `nflight` at a time

    def attack_group(group):
        if len(group) == 1 or nflight == 1:
            for batch, image1, image2, flow in group:
                res = pcfa_attack(model, image1, image2, flow, batch, distortion_folder, EPS_BOX, device, has_gt, optim_mu,
                                  args)
                local.append(_result_row(batch, res))
            return
        # the pairs of a dataset are independent (attack_PCFA.py:668-670): lane k = stream + graph set + scratch of its own,
        # every pair's result bit-identical to attacking it alone (PairsInFlight)
        flight = PairsInFlight(lambda k: PairAttack(model, group[k][1], group[k][2], group[k][3], group[k][0], EPS_BOX, device,
                                                    has_gt, optim_mu, args, trace=_new_trace(model, device, args)),
                               len(group), device)
        if args.steps > 0:
            flight.run(args.steps)
        for k, ((batch, _, _, _), st) in enumerate(zip(group, flight.attacks)):
            _save_trace(st, args)
            if distortion_folder is not None and _should_save(batch, args):
                with flight.on_lane(k):     # on the lane's own stream: the next group adopts its buffers there
                    st.save(distortion_folder)
            local.append(_result_row(batch, st.result()))

    def attack_batch(group):
        # one closure for the whole group (PairBatch): every pair keeps its own variables, target, optimiser state and
        # best-iterate record, and its row goes out under its own index
        if len(group) == 1:
            return attack_group(group)
        pb = PairBatch(model, group, EPS_BOX, device, has_gt, optim_mu, args)
        for _ in range(args.steps):
            pb.step()
        for b, (batch, _, _, _) in enumerate(group):
            if distortion_folder is not None and _should_save(batch, args):
                pb.save(distortion_folder, b)
            local.append(_result_row(batch, pb.result(b)))

    mine = ((batch, image1, image2, flow) for batch, (image1, image2, flow, _) in enumerate(data_loader)
            if batch % world == rank)
    # --save_png: a pair's pictures are deflated and written by one worker thread while the next pair is attacked; leaving
    # the block joins it and re-raises its error
    with pictures.background_writes() if getattr(args, "save_png", False) else contextlib.nullcontext():
        if per_closure > 1:
            for group in group_pairs(mine, per_closure, lambda pair: tuple(pair[1].shape)):
                attack_batch(group)
        else:
            for pair in mine:
                pending.append(pair)
                if len(pending) == nflight:
                    attack_group(pending)
                    pending = []
            if pending:
                attack_group(pending)

    rows = sharding.gather_rows(local, width=13, device=device)
    if rank != 0:
        return None
    rows = sorted(rows, key=lambda r: r[0])
    tests = len(rows)
    names = ("aee_avg_pred-gt", "aee_avg_pred-tgt", "aee_avg_gt-tgt", "aee_avg_predadv-gt", "aee_avg_predadv-tgt",
             "aee_avg_pred-predadv", "l2_avg_delta1", "l2_avg_delta2", "l2_avg_delta12", "aee_avg_predadv-tgt_min",
             "aee_avg_pred-predadv_min", "l2_avg_delta12_min")
    sums = {n: float(np.nansum([r[i + 1] for r in rows])) for i, n in enumerate(names)}
    logging.calc_log_averages(tests, *sums.items())
    result = {n: (v / tests if tests else float('nan')) for n, v in sums.items()}
    result["pairs"] = tests
    print("\nFinished attacking with PCFA. The best achieved values are")
    print("\tAEE(f_adv, f_init)=%f" % result["aee_avg_pred-predadv_min"])
    print("\tAEE(f_adv, f_targ)=%f" % result["aee_avg_predadv-tgt_min"])
    print("\tL2(perturbation)  =%f" % result["l2_avg_delta12_min"])
    return result


class _UniversalBatchState:
    """Static device buffers + captured hipGraphs of the universal closure for ONE batch shape."""

    def __init__(self, image1, image2, padder):
        self.image1 = image1.clone()
        self.image2 = image2.clone()
        self.padder = padder
        self.target = None
        self.graphed = None
        self.repredict = None
        self.tried_graph = False


class UniversalAttack:
    """State of attack_l2_universal (attack_PCFA.py:297-566): ONE perturbation (pair) `[3,Hp,Wp]` shared by every
    image, ONE L-BFGS optimiser for the whole run, data parallel over the batch.

    Every rank holds batch_size/world_size pairs of each global batch, a replica of delta and of the L-BFGS
    state.  Per closure: local forward/backward, then ONE all-reduce of a flat buffer holding d(loss)/d(delta) of
    both perturbations and the scalar loss (sharding.FlatReducer).  The penalty depends on delta only, so it is
    identical on every rank and its average is itself; the similarity term is a mean over the batch, so the
    average of the local means equals the reference's single-process mean over the global batch
    (attack_PCFA.py:469-490).

    On the GPU forward + loss + backward (+ the packing of gradients and loss for the all-reduce) is captured ONCE
    per batch shape into a hipGraph: delta is updated in place by L-BFGS and the images / target of a new batch
    are copied into the same static buffers, so every closure evaluation of every batch replays the same graph;
    the collective runs between replays, outside the graph (PCFA_HIP_GRAPH=0 disables capture)."""

    def __init__(self, model, delta_like1, delta_like2, device, optim_mu, args, use_graph=None):
        self.model, self.args, self.device, self.optim_mu = model, args, device, optim_mu
        self.world = sharding.world_size()
        # cosim is a ratio of sums over the global batch: its three sums are all-reduced between the forward and the
        # backward pass of every closure (sharding.BatchSums); that collective cannot sit inside a captured graph
        self.batch_sums = sharding.BatchSums() if (self.world > 1 and args.loss == "cosim") else None
        self.unit_input = ownutilities.model_takes_unit_input(args.net)
        self.nw_delta1 = torch.zeros_like(delta_like1).to(device)
        self.nw_delta2 = torch.zeros_like(delta_like2).to(device)
        self.nw_delta1.requires_grad = True
        if args.joint_perturbation:
            self.params = [self.nw_delta1]
        else:
            self.nw_delta2.requires_grad = True
            self.params = [self.nw_delta1, self.nw_delta2]
        self.optimizer = ops.get().LBFGS(self.params, max_iter=10)
        self.reducer = sharding.FlatReducer(self.params) if self.world > 1 else None
        self.use_graph = _graphs_enabled(device, args) if use_graph is None else use_graph
        if self.batch_sums is not None:
            self.use_graph = False
        self.states = {}   # batch shape -> _UniversalBatchState
        self.st = None
        self.flow_pred_init = None
        self.flow_pred = None      # the attacked prediction of the last step (--save_png)
        self.closures = 0

    def deltas(self):
        if self.args.joint_perturbation:
            return self.nw_delta1, self.nw_delta1
        return self.nw_delta1, self.nw_delta2

    def predict(self, perturbed=True):
        st, kw = self.st, {}
        if perturbed:
            kw = {"delta1": self.nw_delta1} if self.args.joint_perturbation else {"delta1": self.nw_delta1,
                                                                                   "delta2": self.nw_delta2}
        out = ownutilities.compute_flow(self.model, "scaled_input_model", st.image1, st.image2, test_mode=True, **kw)
        [out] = ownutilities.postprocess_flow(self.args.net, st.padder, out)
        return out

    def closure_body(self):
        d1, d2 = self.deltas()
        loss_closure = losses.loss_delta_constraint(self.predict(), self.st.target, d1, d2, self.device,
                                                    delta_bound=self.args.delta_bound, mu=self.optim_mu,
                                                    f_type=self.args.loss, batch_sums=self.batch_sums)
        loss_closure.backward()
        if self.reducer is not None:
            self.reducer.pack(loss_closure)
        return loss_closure

    def closure(self):
        self.closures += 1
        if self.st.graphed is not None:
            loss_closure = self.st.graphed()
        else:
            self.optimizer.zero_grad()
            loss_closure = self.closure_body()
        return self.reducer.reduce() if self.reducer is not None else loss_closure

    def begin_batch(self, image1, image2):
        """Upload a batch (this rank's slice), predict the unattacked flow, set the target (attack_PCFA.py:404-452).
        Returns AEE(target, unattacked flow) averaged over ranks."""
        device = self.device
        image1, image2 = image1.to(device), image2.to(device)
        if not self.unit_input:
            image1 = image1 / 255.
            image2 = image2 / 255.
        padder, [image1, image2] = ownutilities.preprocess_img(self.args.net, image1, image2)
        key = tuple(image1.shape)
        st = self.states.pop(key, None)
        if st is None:
            st = _UniversalBatchState(image1, image2, padder)
        else:
            st.image1.copy_(image1)
            st.image2.copy_(image2)
        self.states[key] = st                              # most recently used last
        while len(self.states) > _max_cached_shapes(self.model):   # every state pins a closure graph pool: keep the newest
            old_key = next(iter(self.states))
            self.states.pop(old_key)
            _log_eviction("universal batch-state", old_key)
        self.st = st
        with torch.no_grad():
            self.flow_pred_init = self.predict(perturbed=False).detach().clone()
        self.flow_pred = None
        target = targets.get_target(self.args.target, self.flow_pred_init,
                                    custom_target_path=self.args.custom_target_path, device=device).to(device)
        if st.target is None:
            st.target = target.clone()
        else:
            st.target.copy_(target)
        self.model.zero_grad()
        self.optimizer.zero_grad()
        if self.use_graph and not st.tried_graph:
            st.tried_graph = True
            try:
                from .graphed import GraphedClosure, GraphedForward
                st.graphed = GraphedClosure(self.closure_body, self.params)
                st.repredict = GraphedForward(self.predict, device)
            except Exception as e:  # noqa: BLE001 -- the eager closure computes the same thing
                import logging as pylog
                pylog.warning("hipGraph capture of the universal closure failed (%r): launching eagerly", e)
                st.graphed = st.repredict = None
        return sharding.mean_scalar(logging.calc_metrics_const(st.target, self.flow_pred_init), device)

    def step(self):
        """One `--steps` iteration on the current batch (attack_PCFA.py:455-517): L-BFGS step (10 closures, each
        followed by the all-reduce), re-prediction, metrics (averaged over ranks)."""
        st = self.st
        self.optimizer.step(self.closure)
        if st.repredict is not None:
            flow_pred = st.repredict()
        else:
            with torch.no_grad():
                flow_pred = self.predict()
        self.flow_pred = flow_pred
        d1, d2 = self.deltas()
        aee_adv_tgt, aee_adv_pred = logging.calc_metrics_adv(flow_pred, st.target, self.flow_pred_init)
        if self.world > 1:
            aee_adv_tgt, aee_adv_pred = sharding.mean_scalars((aee_adv_tgt, aee_adv_pred), self.device)
        l2_delta1, l2_delta2, l2_delta12 = logging.calc_delta_metrics(d1.detach(), d2.detach())
        return {"aee_predadv-tgt": aee_adv_tgt, "aee_pred-predadv": aee_adv_pred, "l2_delta1": l2_delta1,
                "l2_delta2": l2_delta2, "l2_delta-avg": l2_delta12}

    def save_pictures(self, distortion_folder, batch_ctr, epoch, flow_gt=None):
        """`--save_png`: the per-epoch pictures of attack_PCFA.py:526-541 from the last batch's tensors: the perturbations
        normalised to their common maximum, the attacked frames and the attacked prediction (item i of the batch under the
        reference's rule: `<name>.png`, then `<name>.png_i.png`)."""
        st, e = self.st, str(epoch)
        d1, d2 = (d.detach().unsqueeze(0) for d in self.deltas())
        joint = bool(self.args.joint_perturbation)
        flow_pred = self.flow_pred if self.flow_pred is not None else self.flow_pred_init
        ps = pictures.PictureSet()
        m = torch.maximum(ops.get().absmax(d1), ops.get().absmax(d2))
        logging.save_image(d1, batch_ctr, distortion_folder, image_name="delta1_e" + e, normalize_max=m, pictures=ps)
        if not joint:
            logging.save_image(d2, batch_ctr, distortion_folder, image_name="delta2_e" + e, normalize_max=m, pictures=ps)
        logging.save_image(st.image1, batch_ctr, distortion_folder, image_name="image1_delta_e" + e, add=d1, pictures=ps)
        logging.save_image(st.image2, batch_ctr, distortion_folder, image_name="image2_delta_e" + e, add=d2, pictures=ps)
        scale = logging.flow_picture_scale(getattr(self.args, "png_flow_scale", "own"),
                                           (flow_gt, self.flow_pred_init, flow_pred))
        logging.save_flow(flow_pred, batch_ctr, distortion_folder, flow_name="flow_pred_e" + e, auto_scale=False,
                          max_scale=scale, honour_scale=scale is not None, pictures=ps)
        ps.write()

    @property
    def graphed(self):
        return any(s_.graphed is not None for s_ in self.states.values())


def attack_l2_universal(args, data_loader=None, has_gt=None):
    """One perturbation for a whole dataset (attack_PCFA.py:297-566), data parallel over the batch: see
    `UniversalAttack`.  Returns the final perturbations, the per-step metric history and how many collectives ran."""
    _trace_folder(args)
    optim_mu = default_mu(args)
    rank, world = sharding.rank(), sharding.world_size()
    distortion_folder = _output_folder(args, "") if rank == 0 else None
    device = select_device()
    if data_loader is None:
        if args.batch_size % world != 0:
            raise ValueError("--batch_size %d must be divisible by the %d ranks" % (args.batch_size, world))
        data_loader, has_gt = datasets.prepare_dataloader(args, batch_size=args.batch_size // world, shuffle=True,
                                                          shard=(rank, world))
    model = _load_model(args, device, variable_change=False)  # universal = clipping only (attack_PCFA.py:365)

    image1_init, image2_init, _, _ = next(iter(data_loader))
    _, [image1_init, image2_init] = ownutilities.preprocess_img(args.net, image1_init, image2_init)
    ua = UniversalAttack(model, image1_init[0, :, :, :], image2_init[0, :, :, :], device, optim_mu, args)

    history = []
    batches = []
    batch_ctr = -1
    for epoch in range(args.epochs):
        for batch, (image1, image2, flow, _) in enumerate(data_loader):
            batch_ctr += 1
            curr_step = batch_ctr * args.steps
            aee_tgt = ua.begin_batch(image1, image2)
            logging.log_metrics(curr_step, ("aee_pred-tgt", aee_tgt))
            batches.append({"epoch": epoch, "batch": batch, "aee_pred-tgt": aee_tgt})
            for steps in range(args.steps):
                curr_step = batch_ctr * args.steps + steps
                logging.log_metrics(curr_step, ("steps", steps), ("batch", batch), ("epoch", epoch))
                m = ua.step()
                logging.log_metrics(curr_step, *m.items())
                history.append(dict(m, epoch=epoch, batch=batch, step=steps))
            if distortion_folder is not None and _should_save(batch_ctr, args):
                logging.save_tensor(ua.nw_delta1, "delta1_b" + str(batch_ctr), batch_ctr, distortion_folder)
                logging.save_tensor(ua.deltas()[1], "delta2_b" + str(batch_ctr), batch_ctr, distortion_folder)
        if distortion_folder is not None:
            # `NNNNN_delta1_e{E}.npy`: the pattern evaluate_PCFA.py:42-43 looks for
            logging.save_tensor(ua.nw_delta1, "delta1_e" + str(epoch), batch_ctr, distortion_folder)
            if not args.joint_perturbation:
                logging.save_tensor(ua.nw_delta2, "delta2_e" + str(epoch), batch_ctr, distortion_folder)
            if getattr(args, "save_png", False):
                ua.save_pictures(distortion_folder, batch_ctr, epoch, flow.to(device) if has_gt else None)
    return {"delta1": ua.nw_delta1.detach(), "delta2": ua.deltas()[1].detach(), "history": history,
            "batches": batches, "collectives": ua.reducer.collectives if ua.reducer is not None else 0,
            "batch_sum_collectives": ua.batch_sums.collectives if ua.batch_sums is not None else 0,
            "graphed": ua.graphed}


def main(argv=None):
    parser = parsing_file.create_parser(stage='training', attack_type='pcfa')
    args = parser.parse_args(argv)
    print(args)
    sharding.init_from_env()
    try:
        if args.universal_perturbation:
            return attack_l2_universal(args)
        return attack_l2(args)
    finally:
        sharding.shutdown()


if __name__ == '__main__':
    main()
