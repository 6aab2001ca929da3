"""The picture-artefact kernels (pcfa_amd/csrc/artefact_ops.hip) against the float64 restatement of tests/artefacts.py, and
`--save_png` end to end.  The gates are those the plain fp32 arithmetic passes on the CPU
(tests/test_artefacts_host_cpu.py)."""
import os

import numpy as np
import pytest
import torch

from tests import artefacts as A
from tests import closure_util

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda")


def _ops():
    from pcfa_amd import hip_ops
    return hip_ops


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def _view(a):
    """The array as a non-contiguous [B,C,H,W] device view of a wider tensor."""
    wide, index = A.strided_view(a, *a.shape)
    v = _dev(wide)[index]
    assert not v.is_contiguous() and tuple(v.shape) == a.shape
    return v


def _colour(flow, scale, forced, normal, view=False):
    got = _ops().flow_to_rgb8(_view(flow) if view else _dev(flow), _dev(np.asarray(scale, np.float32)))
    assert got.dtype == torch.uint8 and got.is_contiguous() and tuple(got.shape) == (flow.shape[0],) + flow.shape[2:] + (3,)
    worst, share = A.check_colour(got.cpu().numpy(), flow, scale, forced, random_normal=normal)
    print("colour %s forced=%s: max level difference %d, %.3f %% of the pixels differ" % (flow.shape, forced, worst,
                                                                                        100 * share))


@pytest.mark.parametrize("shape", A.SHAPES)
def test_maxima_equal_numpy(shape):
    B, H, W = shape
    flow = A.normal_flow(B, H, W, seed=1)
    assert np.array_equal(_ops().flow_maxlen(_dev(flow)).cpu().numpy(), A.flow_maxlen_f32(flow))
    assert np.array_equal(_ops().flow_maxlen(_view(flow)).cpu().numpy(), A.flow_maxlen_f32(flow))
    holes = A.with_nans(flow, seed=1)
    assert np.array_equal(_ops().flow_maxlen(_dev(holes)).cpu().numpy(), A.flow_maxlen_f32(holes))
    x = (A.unit_images(B, H, W, seed=1)[0] - np.float32(0.5)).astype(np.float32)
    assert np.array_equal(_ops().absmax(_dev(x)).cpu().numpy(), A.absmax_f32(x))
    # two calls, equal bits: a maximum does not depend on the order of reduction
    assert torch.equal(_ops().flow_maxlen(_dev(flow)), _ops().flow_maxlen(_dev(flow)))


def test_maxima_of_zero_and_single_flows():
    z = np.zeros((2, 2, 5, 7), np.float32)
    assert np.array_equal(_ops().flow_maxlen(_dev(z)).cpu().numpy(), np.zeros(2, np.float32))
    assert np.array_equal(_ops().flow_maxlen(_dev(z[0])).cpu().numpy(), np.zeros(1, np.float32))     # [2,H,W]
    assert np.array_equal(_ops().absmax(_dev(np.full((1, 3, 1, 1), -2.5, np.float32))).cpu().numpy(), [2.5])


@pytest.mark.parametrize("shape", A.SHAPES)
def test_colour_of_random_flows(shape):
    """Three items with very different maxima: each to its own maximum (read from device memory, straight from
    flow_maxlen), then to half of it, where the rad > 1 branch is taken."""
    B, H, W = shape
    flow = A.normal_flow(B, H, W)
    own = _ops().flow_maxlen(_dev(flow)).cpu().numpy()
    _colour(flow, own, False, True)
    _colour(flow, own / 2, True, True)
    _colour(flow, own, False, True, view=True)


@pytest.mark.parametrize("shape", A.SHAPES)
def test_colour_of_nan_pixels(shape):
    B, H, W = shape
    holes = A.with_nans(A.normal_flow(B, H, W))
    _colour(holes, A.flow_maxlen_f32(holes), False, False)
    _colour(holes, A.flow_maxlen_f32(holes), False, False, view=True)


def test_colour_of_a_zero_flow_is_white():
    z = np.zeros((2, 2, 5, 7), np.float32)
    _colour(z, A.flow_maxlen_f32(z), False, False)
    assert (_ops().flow_to_rgb8(_dev(z), _ops().flow_maxlen(_dev(z))) == 255).all()


@pytest.mark.parametrize("case", ["grid", "centres"])
def test_colour_at_the_seam_and_on_bin_centres(case):
    """Integer vectors with v = +-0.0 and u of either sign (atan2's seam, k0 = 54 -> k1 = 0), and vectors exactly on the
    wheel's entries (fk an integer)."""
    flow = A.integer_grid() if case == "grid" else A.bin_centres()
    own = A.flow_maxlen_f32(flow)
    _colour(flow, own, False, False)
    _colour(flow, own / 2, True, False)


def test_one_scale_for_all_items():
    flow = A.normal_flow(3, 5, 7)
    shared = A.flow_maxlen_f32(flow).max(keepdims=True)
    got = _ops().flow_to_rgb8(_dev(flow), _dev(shared)).cpu().numpy()
    A.check_colour(got, flow, np.repeat(shared, 3), False)


@pytest.mark.parametrize("shape", A.SHAPES)
def test_images_equal_fp32_numpy(shape):
    """image_to_rgb8(x) and image_to_rgb8(x, add=d) are numpy fp32 x * 255 and (x + d) * 255, truncated, exactly."""
    B, H, W = shape
    x, d = A.unit_images(B, H, W)
    want = (x * np.float32(255)).astype(np.uint8).transpose(0, 2, 3, 1)
    want_add = ((x + d) * np.float32(255)).astype(np.uint8).transpose(0, 2, 3, 1)
    assert ((x + d) >= 0).all() and ((x + d) <= 1).all()
    for up in (_dev, _view):
        got = _ops().image_to_rgb8(up(x))
        assert got.dtype == torch.uint8 and got.is_contiguous() and np.array_equal(got.cpu().numpy(), want)
        assert np.array_equal(_ops().image_to_rgb8(up(x), add=up(d)).cpu().numpy(), want_add)
    # one perturbation for every item (the universal attack): the item stride of `add` is 0
    assert np.array_equal(_ops().image_to_rgb8(_dev(x), add=_dev(d[:1])).cpu().numpy(),
                          A.image_f32(x, add=np.broadcast_to(d[:1], x.shape)))
    # input in levels already
    levels = (x * np.float32(255)).astype(np.float32)
    assert np.array_equal(_ops().image_to_rgb8(_dev(levels), unit_input=False).cpu().numpy(), want)


def test_images_saturate():
    """NaN and negative values give 0, values above 255 give 255 (the reference's astype(np.uint8) would wrap)."""
    n = len(A.OUT_OF_RANGE)
    x = np.ascontiguousarray(np.broadcast_to(A.OUT_OF_RANGE.reshape(1, 1, 1, n), (1, 3, 1, n)))
    got = _ops().image_to_rgb8(_dev(x)).cpu().numpy()
    for c in range(3):
        assert np.array_equal(got[0, 0, :, c], A.OUT_OF_RANGE_LEVELS)


@pytest.mark.parametrize("shape", A.SHAPES)
def test_normalised_perturbations(shape):
    """With normalize_max every pixel is within one level of float64, and the elements equal to +m and -m give exactly 255
    and 0 -- with one m for all items and with one per item."""
    B, H, W = shape
    delta = ((A.unit_images(B, H, W, seed=2)[0] - np.float32(0.5)) * np.float32(0.02)).astype(np.float32)
    m = A.absmax_f32(delta)
    for b in range(B):       # plant +m and -m in every item, in different channels
        delta[b].reshape(-1)[0] = m[b]
        delta[b].reshape(-1)[-1] = -m[b]
    per_item = _ops().absmax(_dev(delta))
    assert np.array_equal(per_item.cpu().numpy(), m)
    got = _ops().image_to_rgb8(_dev(delta), normalize_max=per_item).cpu().numpy()
    want = A.image_f64(delta, m=m)
    assert np.abs(got.astype(int) - want.astype(int)).max() <= 1
    for b in range(B):
        assert got[b].transpose(2, 0, 1).reshape(-1)[0] == 255 and got[b].transpose(2, 0, 1).reshape(-1)[-1] == 0
    common = per_item.max().reshape(1)
    got = _ops().image_to_rgb8(_view(delta), normalize_max=common).cpu().numpy()
    want = A.image_f64(delta, m=np.repeat(m.max(), B))
    assert np.abs(got.astype(int) - want.astype(int)).max() <= 1


def test_ops_refuse_bad_arguments():
    with pytest.raises(ValueError):
        _ops().flow_to_rgb8(torch.zeros(2, 2, 4, 4, device=DEV), torch.ones(3, device=DEV))
    with pytest.raises(ValueError):
        _ops().image_to_rgb8(torch.zeros(1, 2, 4, 4, device=DEV))
    with pytest.raises(ValueError):
        _ops().image_to_rgb8(torch.zeros(2, 3, 4, 4, device=DEV), add=torch.zeros(2, 3, 4, 5, device=DEV))


# ---------------------------------------------------------------------------------------------- end to end
def _files(folder):
    return {f: os.path.join(d, f) for d, _, files in os.walk(str(folder)) for f in files}


def _check_pair_pictures(files, batch, names):
    """image1.png is trunc(image1.npy * 255) exactly; flow_pred_init.png is within the colour gate of the restatement
    applied to flow_pred_init.npy at its own fp32 maximum."""
    for n in names:
        pic = A.read_png_file(files["%05d_%s.png" % (batch, n)])
        assert pic.ndim == 3 and pic.shape[2] == 3
    image1 = np.load(files["%05d_image1.npy" % batch])
    assert np.array_equal(A.read_png_file(files["%05d_image1.png" % batch]),
                          (image1 * np.float32(255)).astype(np.uint8)[0].transpose(1, 2, 0))
    flow = np.load(files["%05d_flow_pred_init.npy" % batch])
    scale = A.flow_maxlen_f32(flow)
    print("pair %d: longest unattacked flow vector %.6g" % (batch, scale[0]))
    A.check_colour(A.read_png_file(files["%05d_flow_pred_init.png" % batch])[None], flow, scale, False)


PCFA_PICTURES = ("image1", "image2", "image1_delta_best", "image2_delta_best", "delta1_best", "delta2_best",
                 "flow_pred_best", "flow_pred_init", "flow_target", "flow_gt")
PCFA_TENSORS = ("delta1_final", "delta2_final", "delta1_best", "delta2_best", "image1", "image2", "target",
                "flow_pred_final", "flow_pred_best", "flow_pred_init", "flow_gt")


@pytest.mark.parametrize("per_closure", [1, 2])
def test_attack_l2_writes_the_pictures(tmp_path, per_closure):
    from pcfa_amd import attack_PCFA
    attack_PCFA.attack_l2(closure_util.cli_args(steps=1, no_save=False, output_folder=str(tmp_path / "png"), save_png=True,
                                                pairs_per_closure=per_closure, pairs_in_flight=1))
    files = _files(tmp_path / "png")
    want = ["%05d_%s.npy" % (b, n) for b in (0, 1) for n in PCFA_TENSORS]
    want += ["%05d_%s.png" % (b, n) for b in (0, 1) for n in PCFA_PICTURES]
    assert sorted(files) == sorted(want)
    for b in (0, 1):
        _check_pair_pictures(files, b, PCFA_PICTURES)
    # the perturbation pictures share one maximum: the largest |delta| of either frame sits at level 255 or 0
    d1, d2 = (np.load(files["00000_delta%d_best.npy" % i]) for i in (1, 2))
    m = max(np.abs(d1).max(), np.abs(d2).max())
    levels = np.concatenate([A.read_png_file(files["00000_delta%d_best.png" % i]).reshape(-1) for i in (1, 2)])
    assert m > 0 and (levels.max() == 255 or levels.min() == 0)
    want = np.concatenate([A.image_f64(d, m=[m])[0].reshape(-1) for d in (d1, d2)])
    assert np.abs(levels.astype(int) - want.astype(int)).max() <= 1


def test_attack_l2_without_the_flag_writes_no_picture(tmp_path):
    """The same run without --save_png: the .npy files as ever (the inputs bit for bit; SpyNet's attacked tensors are not
    reproducible from run to run) and no picture."""
    from pcfa_amd import attack_PCFA
    attack_PCFA.attack_l2(closure_util.cli_args(steps=1, no_save=False, output_folder=str(tmp_path), synthetic_pairs=1,
                                                pairs_per_closure=1, pairs_in_flight=1))
    files = _files(tmp_path)
    assert sorted(files) == sorted("00000_%s.npy" % n for n in PCFA_TENSORS)


def test_shared_flow_scale_and_joint_run(tmp_path):
    """--png_flow_scale shared: one scale for a pair's flow pictures, the longest vector of ground truth, initial and best
    prediction; a --joint_perturbation run writes no delta2 picture."""
    from pcfa_amd import attack_PCFA
    attack_PCFA.attack_l2(closure_util.cli_args(steps=1, no_save=False, output_folder=str(tmp_path), save_png=True,
                                                png_flow_scale="shared", joint_perturbation=True, boxconstraint="clipping",
                                                synthetic_pairs=1, pairs_per_closure=1, pairs_in_flight=1))
    files = _files(tmp_path)
    assert sorted(f for f in files if f.endswith(".png")) == sorted("00000_%s.png" % n for n in PCFA_PICTURES
                                                                    if n != "delta2_best")
    flows = {n: np.load(files["00000_%s.npy" % n]) for n in ("flow_gt", "flow_pred_init", "flow_pred_best")}
    scale = np.max([A.flow_maxlen_f32(f) for f in flows.values()], axis=0)
    # the synthetic ground truth, (3, -2) everywhere, is longer than anything the randomly weighted SpyNet predicts: the
    # unattacked prediction is drawn at a scale well above its own maximum, so its picture tells the two modes apart
    own = A.flow_maxlen_f32(flows["flow_pred_init"])
    print("shared scale %.6g, the unattacked prediction's own %.6g" % (scale[0], own[0]))
    assert own[0] < 0.9 * scale[0]
    A.check_colour(A.read_png_file(files["00000_flow_pred_init.png"])[None], flows["flow_pred_init"], scale, True)
    A.check_colour(A.read_png_file(files["00000_flow_target.png"])[None], np.load(files["00000_target.npy"]), scale, True)


def test_pairs_in_flight_write_the_pictures_of_a_sequential_run(tmp_path):
    """--pairs_in_flight 2 on four pairs: the second group adopts the first group's static buffers lane by lane while the
    worker thread may still be writing, so every save() has to queue its conversions on its lane's own stream.  A pair's
    results do not depend on the lanes, so every picture must have the bytes of the sequential run's, and image1.png must
    be the pair's own image1.npy."""
    from pcfa_amd import attack_PCFA
    runs = []
    for nflight in (1, 2):
        folder = tmp_path / ("flight%d" % nflight)
        attack_PCFA.attack_l2(closure_util.cli_args(net="RAFT", synthetic_size="128x160", synthetic_pairs=4, steps=1,
                                                    no_save=False, output_folder=str(folder), save_png=True,
                                                    pairs_per_closure=1, pairs_in_flight=nflight))
        runs.append(_files(folder))
    solo, flight = runs
    pngs = sorted(f for f in solo if f.endswith(".png"))
    assert len(pngs) == 4 * len(PCFA_PICTURES) and sorted(flight) == sorted(solo)
    for f in pngs:
        with open(solo[f], "rb") as a, open(flight[f], "rb") as b:
            assert a.read() == b.read(), f
    for batch in range(4):
        image1 = np.load(flight["%05d_image1.npy" % batch])
        assert np.array_equal(A.read_png_file(flight["%05d_image1.png" % batch]),
                              (image1 * np.float32(255)).astype(np.uint8)[0].transpose(1, 2, 0))


def test_fgsm_attack_writes_the_pictures(tmp_path):
    from pcfa_amd import attack_FGSM
    attack_FGSM.attack(closure_util.cli_args(steps=1, synthetic_pairs=1, no_save=False, epsilon=0.00025,
                                             output_folder=str(tmp_path), save_png=True, pairs_in_flight=1))
    files = _files(tmp_path)
    names = ("image1", "image2", "delta1", "delta2", "flow_pred_final", "flow_pred_init", "flow_target", "flow_gt")
    assert sorted(f for f in files if f.endswith(".png")) == sorted("00000_%s.png" % n for n in names)
    assert len([f for f in files if f.endswith(".npy")]) == 8
    _check_pair_pictures(files, 0, names)


def test_universal_attack_writes_the_pictures(tmp_path):
    from pcfa_amd import attack_PCFA
    attack_PCFA.attack_l2_universal(closure_util.cli_args(universal_perturbation=True, boxconstraint="clipping", steps=1,
                                                          no_save=False, output_folder=str(tmp_path), save_png=True))
    files = _files(tmp_path)
    want = ["00000_delta1_e0.png", "00000_delta2_e0.png"]
    for n in ("image1_delta_e0", "image2_delta_e0", "flow_pred_e0"):
        want += ["00000_%s.png" % n, "00000_%s.png_1.png" % n]
    assert sorted(f for f in files if ".png" in f) == sorted(want)
    delta = np.load(files["00000_delta1_e0.npy"])
    assert A.read_png_file(files["00000_delta1_e0.png"]).shape == delta.shape[1:] + (3,)
    assert A.read_png_file(files["00000_image1_delta_e0.png_1.png"]).shape == delta.shape[1:] + (3,)
