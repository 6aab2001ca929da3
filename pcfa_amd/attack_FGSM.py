"""Iterated FGSM baseline on the same adapter and kernels (reference attack_FGSM.py:21-56,59-308).

One iteration = 1 backward + a signed-gradient step of size --epsilon with the images clipped to [0,1] + 1 forward at the
moved images; `--joint_perturbation` averages the two image gradients before taking the sign.

    fgsm_attack_step     attack_FGSM.py:21-56     (torch; the CPU port and the arithmetic the kernel is tested against)
    pgd_l2_attack_step   (no counterpart)         `--step_norm l2`: a step of averaged L2 length --epsilon, then the
                                                  projection onto two_norm_avg_delta <= --delta_bound (torch; the CPU port)
    FgsmAttack           attack_FGSM.py:150-254   one pair: static buffers, captured forward / backward, `step()`
    fgsm_attack          FgsmAttack + args.steps x step()
    attack               attack_FGSM.py:59-308    every pair of a dataset, `--pairs_in_flight`, artefacts, rank sharding

On the GPU the loop runs like PCFA's (attack_PCFA.PairAttack): the network forward and the loss + backward are captured once
per shape into two hipGraphs (graphed.SplitGraphedStep), the signed step and the perturbations are ONE kernel
(ops.fgsm_step, in place on the static images), the six per-iteration metrics of the reference (attack_FGSM.py:199-241) are
computed inside the forward graph and collected in a device buffer that is read back once after the last iteration.  Nothing
in `step()` allocates or waits for the GPU, so several pairs can be in flight (attack_PCFA.PairsInFlight)."""
import math
import os
import time

import numpy as np
import torch

from . import config, graph_sets, ops, sharding
from .attack_PCFA import PairsInFlight, _graphs_enabled, _hardware_queues_for, _load_model, _should_save, select_device
from .helper_functions import datasets, logging, losses, ownutilities, parsing_file, pictures, targets

# columns of the per-iteration history, under the reference's metric names (attack_FGSM.py:234-241)
HISTORY_KEYS = ("aee_predadv-tgt", "aee_pred-predadv", "aee_predadv-gt", "l2_delta1", "l2_delta2", "l2_delta-avg")


def fgsm_attack_step(image1, image2, epsilon, image1_grad, image2_grad, image_min=0., image_max=1., clipping=True,
                     common_perturb=False):
    """attack_FGSM.py:21-56."""
    if not common_perturb:
        s1, s2 = image1_grad.sign(), image2_grad.sign()
    else:
        s1 = s2 = (0.5 * (image1_grad + image2_grad)).sign()
    p1 = image1 - epsilon * s1
    p2 = image2 - epsilon * s2
    if clipping:
        p1 = torch.clamp(p1, image_min, image_max)
        p2 = torch.clamp(p2, image_min, image_max)
    return p1, p2


def _f32(v):
    """The fp32 value nearest to the Python float v, as a Python float (inf past the range)."""
    with np.errstate(over="ignore"):
        return float(np.float32(v))


def _sum_squares_f64(a, b):
    return float(a.double().square().sum() + b.double().square().sum())


def pgd_l2_attack_step(x1, x2, image1_grad, image2_grad, image1, image2, epsilon, delta_bound, common_perturb=False):
    """One projected-gradient iteration under PCFA's budget (`--step_norm l2`; the reference has no projection).
    This is the arithmetic ops.pgd_l2_step implements (include/pcfa_hip.h) and the CPU port's path.  n floats per image,
    N = 2n; epsilon and delta_bound enter as their fp32 values, as the kernel receives them:

        joint        g1 = g2 = 0.5f * (g1 + g2), the fp32 sum rounded first as in fgsm_attack_step
        G            sum g1^2 + sum g2^2 in double (here in torch's order, in the kernel in the order the header states)
        a            fp32(epsilon * sqrt(N / G)), evaluated in double and rounded once: the move a * g has averaged L2
                     length epsilon, what a signed step of size epsilon has.  a = 0 where G is 0, NaN or Inf (or the
                     rounded a is not finite): then nothing moves -- the product a * g is not formed -- and nothing turns NaN
        y_i, e_i     clamp(x_i - a * g_i, 0, 1), product rounded, then the difference;  e_i = y_i - image_i
        E, r         sum e1^2 + sum e2^2 in double;  r = sqrt(E / N) = two_norm_avg_delta(e1, e2)
        r > b        s = fp32(b / r);  x_i <- clamp(image_i + s * e_i, 0, 1), product rounded, then the sum;
                     d_i = x_i - image_i from the updated x_i
        otherwise    (also: E not finite, or a quotient that rounds to 1)  s = 1, x_i <- y_i, d_i = e_i as they are

    Returns (x1', x2', d1, d2, (G, a, E, s)).  Reads its scalars on the host: not for a captured loop."""
    eps, bound = _f32(epsilon), _f32(delta_bound)
    g1, g2 = image1_grad, image2_grad
    if common_perturb:
        g1 = g2 = 0.5 * (g1 + g2)
    n_total = float(g1.numel() + g2.numel())
    G = _sum_squares_f64(g1, g2)
    a = _f32(eps * math.sqrt(n_total / G)) if 0. < G < math.inf else 0.
    if not math.isfinite(a):
        a = 0.
    if a == 0.:
        y1, y2 = torch.clamp(x1, 0., 1.), torch.clamp(x2, 0., 1.)
    else:
        y1, y2 = torch.clamp(x1 - a * g1, 0., 1.), torch.clamp(x2 - a * g2, 0., 1.)
    e1, e2 = y1 - image1, y2 - image2
    E = _sum_squares_f64(e1, e2)
    s = 1.
    if E < math.inf:
        r = math.sqrt(E / n_total)
        if r > bound:
            s = _f32(bound / r)
    if s == 1.:
        return y1, y2, e1, e2, (G, a, E, s)
    p1, p2 = torch.clamp(image1 + s * e1, 0., 1.), torch.clamp(image2 + s * e2, 0., 1.)
    return p1, p2, p1 - image1, p2 - image2, (G, a, E, s)


class FgsmAttack:
    """Everything the reference's loop holds for ONE image pair (attack_FGSM.py:150-254) and `step()`, one iteration:
    backward at x_i, signed step, forward at x_{i+1}, metrics.  `fgsm_attack` is `FgsmAttack(...)` + args.steps x `step()`.

    On the GPU (`use_graph=None`: CUDA device, PCFA_HIP_GRAPH != 0, steps > 0 -- PairAttack's rule -- and an operator table
    that has the step kernel) forward and loss + backward are replayed from hipGraphs captured once per key and kept per model
    for the next pair of that key (`reuse_graphs`, default Config.reuse_pair_graphs), the step is one launch of ops.fgsm_step,
    and the metrics go to a device buffer: `step()` neither allocates nor synchronises.  If capture fails a warning is logged
    and the eager loop -- the same kernels in the same order -- runs.  With `args.step_norm == "l2"` the step is
    ops.pgd_l2_step instead (pgd_l2_attack_step: three launches, outside the graphs like the signed step, no host read) and
    every iterate satisfies two_norm_avg_delta <= args.delta_bound; nothing else in the loop differs.  `history` (one dict
    per iteration, the reference's names) and `result()` read the buffer back, once.  Since `step()` does not wait, a caller
    that moves a lane to another stream reads a result (or synchronises) first: a lane's scratch buffers belong to one
    stream-ordered sequence of launches (ops.core); `fgsm_attack` and PairsInFlight.run both end with such a wait."""

    def __init__(self, model, image1, image2, flow, batch, device, has_gt, args, use_graph=None, reuse_graphs=None):
        self.model, self.args, self.device, self.batch, self.has_gt = model, args, device, batch, has_gt
        if reuse_graphs is None:
            reuse_graphs = config.cfg(model).reuse_pair_graphs
        self.reuse_graphs = reuse_graphs
        self.joint = bool(args.joint_perturbation)
        self.step_norm = getattr(args, "step_norm", "sign")
        if self.step_norm not in ("sign", "l2"):
            raise ValueError("--step_norm is 'sign' or 'l2', got %r" % (self.step_norm,))
        self._take_step = self._l2_step if self.step_norm == "l2" else self._signed_step
        # the CPU port's table has neither step kernel: torch fallback
        self.has_step_kernel = hasattr(ops.get(), "pgd_l2_step" if self.step_norm == "l2" else "fgsm_step")
        self.delta_bound = None    # the budget of the l2 step; the signed step has none
        if self.step_norm == "l2":
            self.delta_bound = float(args.delta_bound)
            if not (0 < self.delta_bound < math.inf and 0 < args.epsilon < math.inf):
                raise ValueError("--step_norm l2 needs a positive, finite --epsilon and --delta_bound, got %r and %r"
                                 % (args.epsilon, args.delta_bound))
            logging.log_param("delta_bound", self.delta_bound)
        image1, image2 = image1.to(device), image2.to(device)
        self.flow_gt = flow.to(device) if (flow is not None and has_gt) else None
        if not ownutilities.model_takes_unit_input(args.net):
            image1, image2 = image1 / 255., image2 / 255.
        raw_shape = tuple(image1.shape)
        self.padder, [image1, image2] = ownutilities.preprocess_img(args.net, image1, image2)
        image1, image2 = image1.contiguous(), image2.contiguous()
        if use_graph is None:
            use_graph = _graphs_enabled(device, args)
        use_graph = bool(use_graph) and self.has_step_kernel and torch.device(device).type == "cuda"
        # (the un-padded shape is part of the key: it is the shape of the flow, the target and the metrics' operands)
        self.graph_key = (args.net, tuple(image1.shape), raw_shape, args.loss, self.joint, float(args.epsilon), args.target,
                          self.step_norm, self.delta_bound, str(device), ops.core.current_lane())
        self.graphed = None
        self.retired = False
        self.steps_done = 0
        self.step_launches = 0
        self._hist = None          # device buffer [steps][6]: one row of metrics per iteration
        self._history = []         # the rows read back so far, as dicts
        # same key as an earlier pair: its static buffers and graphs (KEPT), refilled.  The earlier FgsmAttack (if still alive)
        # is retired first -- it keeps copies of its results.
        kept = graph_sets.adopt(self._graph_sets(), self.graph_key, self) if (use_graph and reuse_graphs) else None
        self.graphs_reused = kept is not None

        if kept is not None:
            with torch.no_grad():
                self.image1.copy_(image1)
                self.image2.copy_(image2)
                self.x1.copy_(image1)
                self.x2.copy_(image2)
                self.delta1.zero_()
                self.delta2.zero_()
                if self.flow_gt is not None:
                    self._flow_gt_buf.copy_(self.flow_gt)
                else:
                    self._flow_gt_buf.zero_()
            self._begin_graphed()
        else:
            self.image1, self.image2 = image1.detach(), image2.detach()
            self.x1 = image1.clone().detach().requires_grad_(True)
            self.x2 = image2.clone().detach().requires_grad_(True)
            self.delta1, self.delta2 = torch.zeros_like(image1), torch.zeros_like(image2)
            self._flow_gt_buf = None
            if use_graph:
                self.enable_graph()
            if self.graphed is None:
                self.flow_pred = self.predict()     # keeps its autograd graph: the first iteration's backward runs through it
                self.flow_pred_init = self.flow_pred.detach().clone()
                self.target = targets.get_target(args.target, self.flow_pred_init,
                                                 custom_target_path=args.custom_target_path, device=device).to(device)
                self._flow_gt_buf = self.flow_gt if self.flow_gt is not None else torch.zeros_like(self.flow_pred_init)
        self.target.requires_grad = False
        self.aee_tgt = logging.calc_metrics_const(self.target, self.flow_pred_init)
        logging.log_metrics(batch * args.steps, ("aee_pred-tgt", self.aee_tgt))
        self._hist = torch.empty((max(1, int(args.steps)), len(HISTORY_KEYS)), device=device, dtype=torch.float32)

    # what one pair leaves to the next pair of the same key: the static buffers the two graphs read and write, and the graphs
    # (there is no optimiser state in I-FGSM).  A cache of its own: PCFA's (`_pcfa_pair_graphs`) is not touched by this attack
    KEPT = ("x1", "x2", "image1", "image2", "delta1", "delta2", "target", "flow_pred_init", "_flow_gt_buf", "graphed")

    def _graph_sets(self):
        return graph_sets.cache(self.model, "fgsm-graph")

    # ---- pieces of one iteration --------------------------------------------------------------------------------
    def predict(self):
        out = ownutilities.compute_flow(self.model, "scaled_input_model", self.x1, self.x2, test_mode=True)
        [out] = ownutilities.postprocess_flow(self.args.net, self.padder, out)
        return out

    def _forward_with_metrics(self):
        """The forward half of an iteration (the forward graph, or the eager loop's forward): the prediction (autograd
        recording on) and, from it and the perturbations the step left, the six metrics of attack_FGSM.py:199-241 -- the
        launches of logging.calc_metrics_adv(_gt) and calc_delta_metrics without their host reads (without ground truth
        the third column is computed against zeros and dropped from `history`)."""
        flow = self.predict()
        with torch.no_grad():
            f = flow.detach()
            row = torch.stack([losses.avg_epe(f, self.target), losses.avg_epe(f, self.flow_pred_init),
                               losses.avg_epe(f, self._flow_gt_buf), losses.two_norm_avg(self.delta1),
                               losses.two_norm_avg(self.delta2), losses.two_norm_avg_delta(self.delta1, self.delta2)])
        return flow, row

    def _loss(self, flow):
        return losses.get_loss(self.args.loss, flow, self.target)

    def enable_graph(self):
        try:
            from .graphed import SplitGraphedStep
            with torch.no_grad():     # the shape of the flow (and the first-call work of every kernel) before any capture
                flow0 = self.predict().detach()
            self.flow_pred_init = flow0.clone()
            self.target = torch.zeros_like(flow0)
            self._flow_gt_buf = self.flow_gt.clone() if self.flow_gt is not None else torch.zeros_like(flow0)
            # the step kernel is launched OUTSIDE the captured graphs: warm-up and capture leave the images where they are
            self.graphed = SplitGraphedStep(self._forward_with_metrics, self._loss, [self.x1, self.x2])
            if self.reuse_graphs:   # the next pair of this key adopts them
                graph_sets.put(self._graph_sets(), self.graph_key, graph_sets.GraphSet(self, self.graph_key[-1], self.KEPT),
                               config.cfg(self.model).max_cached_shapes, "fgsm-graph")
            self._begin_graphed()
        except Exception as e:  # noqa: BLE001 -- the eager loop launches the same kernels in the same order
            import logging as pylog
            pylog.warning("hipGraph capture of the I-FGSM iteration failed (%r): launching eagerly", e)
            self._graph_sets().pop(self.graph_key, None)
            self.graphed = None
            self.x1.grad = self.x2.grad = None

    def _begin_graphed(self):
        """Forward at the clean images = the unattacked flow; the target chosen from it goes into its static buffer."""
        flow, _ = self.graphed.forward()
        self.flow_pred = flow.detach()
        with torch.no_grad():
            self.flow_pred_init.copy_(self.flow_pred)
            target = targets.get_target(self.args.target, self.flow_pred_init,
                                        custom_target_path=self.args.custom_target_path, device=self.device).to(self.device)
            self.target.copy_(target)

    def _retire(self):
        """A later pair of the same key took over this pair's static buffers and graphs (or the set was evicted): the
        results are copied out first and stay readable, further iterations raise."""
        if self.retired:
            return
        self._finish()
        if self.graphed is not None:
            for name in ("delta1", "delta2", "image1", "image2", "target", "flow_pred", "flow_pred_init"):
                setattr(self, name, getattr(self, name).detach().clone())
        self.retired = True
        self.graphed = None

    def _check_live(self):
        if self.retired:
            raise RuntimeError("this FgsmAttack was retired: a later pair of the same shape adopted its static buffers and "
                               "graphs (one live FgsmAttack per shape, model and lane; reuse_graphs=False keeps pairs "
                               "independent)")

    def _signed_step(self, g1, g2):
        if self.has_step_kernel:
            ops.get().fgsm_step(self.x1, self.x2, g1.contiguous(), g2.contiguous(), self.image1, self.image2, self.delta1,
                                self.delta2, self.args.epsilon, self.joint)
            self.step_launches += 1
            return
        with torch.no_grad():    # operator tables without the kernel (the CPU port): attack_FGSM.py:205-209 in torch
            p1, p2 = fgsm_attack_step(self.x1, self.x2, self.args.epsilon, g1, g2, clipping=True, common_perturb=self.joint)
            self.delta1 = torch.clamp(p1, 0., 1.) - self.image1
            self.delta2 = torch.clamp(p2, 0., 1.) - self.image2
            self.x1.copy_(p1)
            self.x2.copy_(p2)

    def _l2_step(self, g1, g2):
        if self.has_step_kernel:
            ops.get().pgd_l2_step(self.x1, self.x2, g1.contiguous(), g2.contiguous(), self.image1, self.image2, self.delta1,
                                  self.delta2, self.args.epsilon, self.delta_bound, self.joint)
            self.step_launches += 1
            return
        with torch.no_grad():    # operator tables without the kernel (the CPU port)
            p1, p2, d1, d2, _ = pgd_l2_attack_step(self.x1, self.x2, g1, g2, self.image1, self.image2, self.args.epsilon,
                                                   self.delta_bound, common_perturb=self.joint)
            self.delta1, self.delta2 = d1, d2
            self.x1.copy_(p1)
            self.x2.copy_(p2)

    # ---- one iteration (attack_FGSM.py:199-241) -----------------------------------------------------------------
    def step(self):
        self._check_live()
        k = self.steps_done
        if k >= self._hist.shape[0]:     # more iterations than --steps announced: grow (not on the product loop)
            self._hist = torch.cat([self._hist, torch.empty_like(self._hist)])
        if self.graphed is not None:
            g1, g2 = self.graphed.backward()
            self._take_step(g1, g2)
            _, row = self.graphed.forward()
        else:
            loss = self._loss(self.flow_pred)
            self.model.zero_grad()
            self.x1.grad = self.x2.grad = None
            loss.backward()
            self._take_step(self.x1.grad.data, self.x2.grad.data)
            self.flow_pred, row = self._forward_with_metrics()
        self._hist[k].copy_(row)
        self.steps_done = k + 1

    def _finish(self):
        """Bring `history` up to the iterations done -- for the graph loop ONE read of the device buffer -- and log the
        new rows under the reference's names."""
        n = self.steps_done
        if len(self._history) == n:
            return
        rows = self._hist[:n].tolist()
        for i in range(len(self._history), n):
            row = dict(zip(HISTORY_KEYS, rows[i]))
            if self.flow_gt is None:
                del row["aee_predadv-gt"]
            self._history.append(row)
            logging.log_metrics(self.batch * self.args.steps + i, *row.items())

    @property
    def history(self):
        """One dict per iteration done: the metrics the reference logs at every step (attack_FGSM.py:234-241)."""
        self._finish()
        return self._history

    def result(self):
        """The final metrics as a dict (the keys and values `fgsm_attack` has always returned)."""
        res = {"aee_pred-tgt": self.aee_tgt}
        if self.steps_done == 0:       # no iteration: the metrics of the clean prediction and a zero perturbation
            flow = self.flow_pred.detach()
            aee_adv_tgt, aee_adv_pred = logging.calc_metrics_adv(flow, self.target, self.flow_pred_init)
            l2_1, l2_2, l2_12 = logging.calc_delta_metrics(self.delta1.detach(), self.delta2.detach())
            res.update({"aee_predadv-tgt": aee_adv_tgt, "aee_pred-predadv": aee_adv_pred, "l2_delta1": l2_1,
                        "l2_delta2": l2_2, "l2_delta-avg": l2_12})
            if self.flow_gt is not None:
                res["aee_predadv-gt"] = logging.calc_metrics_adv_gt(flow, self.flow_gt)
            return res
        last = self.history[-1]
        res.update({key: last[key] for key in ("aee_predadv-tgt", "aee_pred-predadv", "l2_delta1", "l2_delta2",
                                               "l2_delta-avg")})
        if self.flow_gt is not None:
            res["aee_predadv-gt"] = last["aee_predadv-gt"]
        return res

    def save(self, distortion_folder):
        """attack_FGSM.py:246-254."""
        batch = self.batch
        for tens, name in ((self.delta1, "delta1_final"), (self.delta2, "delta2_final"), (self.image1, "image1"),
                           (self.image2, "image2"), (self.target, "target"), (self.flow_pred, "flow_pred_final"),
                           (self.flow_pred_init, "flow_pred_init")):
            logging.save_tensor(tens, name, batch, distortion_folder)
        if self.flow_gt is not None:
            logging.save_tensor(self.flow_gt, "flow_gt", batch, distortion_folder)
        if getattr(self.args, "save_png", False):
            self._save_pictures(distortion_folder)

    def _save_pictures(self, distortion_folder):
        """`--save_png`: the pictures of attack_FGSM.py:256-278, queued on the current stream like PairAttack's.  The
        perturbations are normalised to their common max |delta| as in attack_PCFA.py (the reference's FGSM script takes
        max(delta) without the absolute value, which is not positive for a perturbation that only darkens)."""
        joint = bool(self.args.joint_perturbation)
        ps = pictures.PictureSet()
        logging.save_attack_pictures(
            ps, [self.batch], distortion_folder,
            images=(("image1", self.image1, None), ("image2", self.image2, None)),
            deltas=(("delta1", self.delta1), (None if joint else "delta2", self.delta2)),
            flows=(("flow_pred_final", self.flow_pred), ("flow_pred_init", self.flow_pred_init),
                   ("flow_target", self.target), ("flow_gt", self.flow_gt)),
            flow_scale=logging.flow_picture_scale(getattr(self.args, "png_flow_scale", "own"),
                                                  (self.flow_gt, self.flow_pred_init, self.flow_pred)))
        ps.write()


def fgsm_attack(model, image1, image2, flow, device, has_gt, args, batch=0, distortion_folder=None):
    """The per-pair loop of attack_FGSM.py:150-254; returns the final metrics as a dict, with the per-iteration metrics
    under "history"."""
    st = FgsmAttack(model, image1, image2, flow, batch, device, has_gt, args)
    for _ in range(args.steps):
        st.step()
    return _finish_pair(st, distortion_folder)


def _finish_pair(st, distortion_folder):
    res = st.result()
    res["history"] = st.history
    if distortion_folder is not None and _should_save(st.batch, st.args):
        st.save(distortion_folder)
    return res


def _output_folder(args, tag):
    if getattr(args, "no_save", True):
        return None
    stamp = time.strftime("%Y-%m-%d_%H:%M:%S")
    kind = "%s_FGSM_%s_-" % (args.net, "cd" if args.joint_perturbation else "dd")
    return logging.create_subfolder(os.path.join(args.output_folder, kind, stamp + tag), "patches")


def attack(args, data_loader=None, has_gt=None):
    """attack_FGSM.py:59-308: every pair of the dataset, pairs sharded over ranks like attack_PCFA.attack_l2 and, with
    `--pairs_in_flight N`, attacked N at a time on every GPU (each pair's result is that of attacking it alone)."""
    rank, world = sharding.rank(), sharding.world_size()
    distortion_folder = _output_folder(args, "_r%d" % rank if world > 1 else "")
    if data_loader is None:
        data_loader, has_gt = datasets.prepare_dataloader(args, batch_size=1, shuffle=False)
    nflight = max(1, int(getattr(args, "pairs_in_flight", 1)))
    _hardware_queues_for(nflight)
    device = select_device()
    model = _load_model(args, device, variable_change=False)
    if nflight > 1 and torch.device(device).type != "cuda":
        raise ValueError("--pairs_in_flight needs a GPU (lanes are HIP streams)")
    keys = ("aee_pred-tgt", "aee_predadv-tgt", "aee_pred-predadv", "l2_delta1", "l2_delta2", "l2_delta-avg")
    rows = []
    pending = []   # (batch, image1, image2, flow) of this rank, attacked `nflight` at a time

    def attack_group(group):
        if len(group) == 1 or nflight == 1:
            for batch, image1, image2, flow in group:
                r = fgsm_attack(model, image1, image2, flow, device, has_gt, args, batch=batch,
                                distortion_folder=distortion_folder)
                rows.append((batch,) + tuple(r[k] for k in keys))
            return
        flight = PairsInFlight(lambda k: FgsmAttack(model, group[k][1], group[k][2], group[k][3], group[k][0], device, has_gt,
                                                    args), len(group), device)
        if args.steps > 0:
            flight.run(args.steps)
        for k, st in enumerate(flight.attacks):
            with flight.on_lane(k):     # save() queues its conversions and copies on the lane's own stream
                r = _finish_pair(st, distortion_folder)
            rows.append((st.batch,) + tuple(r[k] for k in keys))

    for batch, (image1, image2, flow, _) in enumerate(data_loader):
        if batch % world != rank:
            continue
        pending.append((batch, image1, image2, flow))
        if len(pending) == nflight:
            attack_group(pending)
            pending = []
    if pending:
        attack_group(pending)
    rows = sharding.gather_rows(rows, width=len(keys) + 1, device=device)
    if rank != 0:
        return None
    n = len(rows)
    out = {k: sum(r[i + 1] for r in rows) / max(n, 1) for i, k in enumerate(keys)}
    out["pairs"] = n
    logging.calc_log_averages(1, *[("avg_" + k, v) for k, v in out.items()])
    return out


def main(argv=None):
    args = parsing_file.create_parser(stage='training', attack_type='fgsm').parse_args(argv)
    sharding.init_from_env()
    try:
        return attack(args)
    finally:
        sharding.shutdown()


if __name__ == '__main__':
    main()
