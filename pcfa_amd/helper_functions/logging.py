"""Metric helpers + a light metric sink for the attack loop.

The metric *math* mirrors the reference's helper_functions/logging.py:165-262 (thin wrappers
over losses.avg_epe / two_norm_avg); the mlflow sink (logging.py:67-111,343-354) is replaced by
an in-process recorder that can be dumped as JSON lines -- mlflow is out of scope
and its ~15 synchronous log_metric calls per step do not belong in a GPU hot loop.
Metric names are the reference's.
"""
import json
import os

import numpy as np
import torch

from . import losses, ownutilities
from . import pictures as _pictures


class MetricSink:
    """Collects (key, value, step) triples; `dump(path)` writes them as JSON lines."""

    def __init__(self):
        self.records = []
        self.params = {}

    def log_metric(self, key, value, step=None):
        if value is not None:
            self.records.append((key, float(value), step))

    def log_param(self, key, value):
        self.params[key] = value

    def dump(self, path):
        with open(path, "w") as f:
            f.write(json.dumps({"params": {k: str(v) for k, v in self.params.items()}}) + "\n")
            for k, v, s in self.records:
                f.write(json.dumps({"key": k, "value": v, "step": s}) + "\n")


SINK = MetricSink()


def log_metric(key, value, step=None):
    SINK.log_metric(key, value, step)


def log_param(key, value):
    SINK.log_param(key, value)


def log_metrics(step, *key_value_pairs):
    """logging.py:343-354."""
    for key, value in key_value_pairs:
        if value is not None:
            SINK.log_metric(key, value, step)


def calc_log_averages(numsteps, *key_value_pairs):
    """logging.py:357-372: log value/numsteps under `key`."""
    for key, value in key_value_pairs:
        SINK.log_metric(key, value / numsteps if numsteps else float("nan"))


def calc_metrics_adv(flow_pred, target, flow_pred_init):
    """AEE(adv, target), AEE(adv, init) -- logging.py:165-185."""
    return float(losses.avg_epe(flow_pred, target)), float(losses.avg_epe(flow_pred, flow_pred_init))


def calc_metrics_adv_gt(flow_pred, flow_gt):
    """logging.py:188-203."""
    return float(losses.avg_epe(flow_pred, flow_gt))


def calc_metrics_const(target, flow_pred_init):
    """logging.py:206-221."""
    return float(losses.avg_epe(target, flow_pred_init))


def calc_metrics_const_gt(target, flow_pred_init, flow_gt):
    """logging.py:224-246."""
    return float(losses.avg_epe(target, flow_gt)), float(losses.avg_epe(flow_pred_init, flow_gt))


def calc_delta_metrics(delta1, delta2, step=None):
    """logging.py:249-262."""
    l2_delta1 = ownutilities.torchfloat_to_float64(losses.two_norm_avg(delta1))
    l2_delta2 = ownutilities.torchfloat_to_float64(losses.two_norm_avg(delta2))
    l2_delta12 = ownutilities.torchfloat_to_float64(losses.two_norm_avg_delta(delta1, delta2))
    return l2_delta1, l2_delta2, l2_delta12


def create_subfolder(folder_path, name):
    path = os.path.join(folder_path, name)
    os.makedirs(path, exist_ok=True)
    return path


def save_tensor(tens, tensor_name, batch, output_folder, unregistered_artifacts=True):
    """`{batch:05d}_{name}.npy`, fp32 -- the artefact format evaluate_PCFA.py consumes (logging.py:265-286)."""
    if tens is None or output_folder is None:
        return None
    path = os.path.join(output_folder, "%05d_%s.npy" % (batch, tensor_name))
    np.save(path, tens.detach().cpu().numpy().astype(np.float32))
    return path


def _picture_path(batch, name, output_folder):
    return os.path.join(output_folder, "%05d_%s.png" % (batch, name))


def save_image(image_data, batch, output_folder, image_name='image', unit_input=True, normalize_max=None,
               unregistered_artifacts=True, add=None, pictures=None):
    """`{batch:05d}_{name}.png` (logging.py:289-317): the image times 255 (unit_input), or with normalize_max = m
    (a number or a device tensor) image / m / 2 + 0.5, times 255 -- the perturbation picture.  Converted on the GPU
    (ops.image_to_rgb8: out-of-range values saturate).  Extra keywords of this build: `add`, a perturbation added in the
    same launch (the reference's save_image(image + delta, ...)); `pictures`, a pictures.PictureSet that collects the
    picture for one common write()."""
    if image_data is None or output_folder is None:
        return None
    path = _picture_path(batch, image_name, output_folder)
    ps = _pictures.PictureSet() if pictures is None else pictures
    t = image_data.detach()
    items = t.shape[0] if t.dim() == 4 else 1
    if normalize_max is not None:
        normalize_max = _pictures.on_device(normalize_max, t.device)
    ps.add_image(_pictures.item_paths(path, items), t, add=add, normalize_max=normalize_max, unit_input=unit_input)
    if pictures is None:
        ps.write()
    return path


def save_flow(flow, batch, output_folder, flow_name='flowgt', auto_scale=True, max_scale=-1, unregistered_artifacts=True,
              honour_scale=False, pictures=None):
    """`{batch:05d}_{name}.png` in the Middlebury colour code (logging.py:320-339).  As in the reference the picture is
    scaled to its own longest vector WHATEVER auto_scale / max_scale say (ownutilities.quickvisualization_flow drops
    them there); honour_scale=True passes them on."""
    if flow is None or output_folder is None:
        return None
    path = _picture_path(batch, flow_name, output_folder)
    ownutilities.quickvisualization_flow(flow.detach(), path, auto_scale=auto_scale, max_scale=max_scale,
                                         honour_scale=honour_scale, pictures=pictures)
    return path


def flow_picture_scale(mode, flows):
    """The scale of a pair's flow pictures under `--png_flow_scale`: None for 'own' (every picture to its own longest
    vector, what the reference writes), for 'shared' the per-item maximum over `flows` (ground truth if any, initial and
    attacked prediction) of ops.flow_maxlen -- a device tensor; nothing is read back (what attack_PCFA.py:281-292 means
    to do)."""
    if mode != "shared":
        return None
    from .. import ops
    scale = None
    for f in flows:
        if f is not None:
            m = ops.get().flow_maxlen(f)
            scale = m if scale is None else torch.maximum(scale, m)
    return scale


def save_attack_pictures(pictures, batches, output_folder, images=(), deltas=(), flows=(), flow_scale=None):
    """Queue one attack's pictures on `pictures` for the pairs numbered `batches` (one per item of the tensors).
    images: (name, tensor, add or None); deltas: (name, tensor) normalised to their common per-item maximum (the
    reference's max_delta); flows: (name, tensor), scaled by flow_scale (flow_picture_scale; None: own maximum)."""
    from .. import ops

    def paths(name):
        return [_picture_path(b, name, output_folder) for b in batches]

    for name, tens, add in images:
        pictures.add_image(paths(name), tens, add=add)
    if deltas:
        max_delta = None
        for _, d in deltas:
            m = ops.get().absmax(d.detach().reshape(len(batches), -1))
            max_delta = m if max_delta is None else torch.maximum(max_delta, m)
        for name, d in deltas:
            if name is not None:
                pictures.add_image(paths(name), d, normalize_max=max_delta)
    for name, f in flows:
        if f is not None:
            pictures.add_flow(paths(name), f, ops.get().flow_maxlen(f) if flow_scale is None else flow_scale)
