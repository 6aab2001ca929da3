"""Host side of `--save_png` (no GPU): the float64 restatement against the reference's pictures, the fp32 arithmetic
against the GPU gates, the PNG writer, the flags and the file names."""
import os
import types
from argparse import Namespace

import numpy as np
import pytest
import torch

from tests import artefacts as A
from tests.util import load_golden


def _golden_flows():
    g = load_golden("flow_colour")
    i = 0
    while "flow_%d" % i in g:
        yield i, np.transpose(g["flow_%d" % i], (2, 0, 1))[None], g
        i += 1


def _own_scale_f64(flow):
    w = flow.astype(np.float64)
    with np.errstate(invalid="ignore"):
        length = np.sqrt(np.square(w[:, 0]) + np.square(w[:, 1]))
    return np.nan_to_num(length, nan=0.0).reshape(len(flow), -1).max(axis=1)


def test_restatement_equals_the_reference_pictures():
    """flow_colour_f64 reproduces colorplot_light bit for bit, auto-scaled and at a forced scale."""
    n = 0
    for i, flow, g in _golden_flows():
        auto, _ = A.flow_colour_f64(flow, _own_scale_f64(flow))
        forced, _ = A.flow_colour_f64(flow, [g["forced_scale_%d" % i]])
        assert np.array_equal(auto[0], g["rgb_auto_%d" % i]), i
        assert np.array_equal(forced[0], g["rgb_forced_%d" % i]), i
        n += 1
    assert n >= 5
    assert os.path.getsize(os.path.join(os.path.dirname(__file__), "golden", "flow_colour.npz")) < 100 * 1024


def test_wheel_is_the_middlebury_wheel():
    w = A.wheel()
    assert w.shape == (55, 3) and w.min() == 0 and w.max() == 255
    assert list(w[0]) == [255, 0, 0] and list(w[15]) == [255, 255, 0] and list(w[21]) == [0, 255, 0]
    assert list(w[25]) == [0, 255, 255] and list(w[36]) == [0, 0, 255] and list(w[49]) == [255, 0, 255]
    assert list(w[54]) == [255, 0, 43]


def _colour_cases():
    """(name, flow, scale, forced, random_normal): the inputs of the GPU colour tests."""
    for B, H, W in A.SHAPES:
        f = A.normal_flow(B, H, W)
        own = A.flow_maxlen_f32(f)
        yield "normal %dx%dx%d own" % (B, H, W), f, own, False, True
        yield "normal %dx%dx%d half" % (B, H, W), f, own / 2, True, True
        h = A.with_nans(f)
        yield "nan %dx%dx%d" % (B, H, W), h, A.flow_maxlen_f32(h), False, False
    z = np.zeros((2, 2, 5, 7), np.float32)
    yield "zero", z, A.flow_maxlen_f32(z), False, False
    for name, f in (("grid", A.integer_grid()), ("centres", A.bin_centres())):
        own = A.flow_maxlen_f32(f)
        yield name + " own", f, own, False, False
        yield name + " half", f, own / 2, True, False


def test_fp32_arithmetic_passes_the_colour_gates():
    """The reference arithmetic in plain fp32 stays inside the gates the kernel has to meet, on every case."""
    for name, flow, scale, forced, normal in _colour_cases():
        A.check_colour(A.flow_colour_f32(flow, scale), flow, scale, forced, random_normal=normal)
    white, _ = A.flow_colour_f64(np.zeros((1, 2, 2, 2), np.float32), [0.0])
    assert (white == 255).all()


def test_fp32_arithmetic_passes_the_image_gates():
    x, d = A.unit_images(2, 33, 66)
    assert np.array_equal(A.image_f32(x), A.image_f64(x))          # x * 255 is exact in float64: the cast is the same
    delta = (x - 0.5).astype(np.float32)
    m = np.maximum(A.absmax_f32(delta), A.absmax_f32(d))
    diff = np.abs(A.image_f32(delta, m=m).astype(int) - A.image_f64(delta, m=m).astype(int))
    assert diff.max() <= 1
    sat = A.image_f32(np.broadcast_to(A.OUT_OF_RANGE.reshape(1, 1, 1, -1), (1, 3, 1, len(A.OUT_OF_RANGE))))
    assert np.array_equal(sat[0, 0, :, 0], A.OUT_OF_RANGE_LEVELS)


@pytest.mark.parametrize("shape", [(1, 1), (5, 7), (33, 66)])
def test_png_round_trip(shape):
    from pcfa_amd.helper_functions import png
    rng = np.random.RandomState(shape[0])
    pix = rng.randint(0, 256, shape + (3,)).astype(np.uint8)
    if shape == (33, 66):
        pix[:16] = np.arange(66, dtype=np.uint8).reshape(1, 66, 1)      # smooth rows as well as noise
    data = png.encode_rgb8(pix)
    assert np.array_equal(A.read_png(data), pix)
    assert png.encode_rgb8(pix.copy()) == data                            # the bytes depend on the pixels only
    kinds = [data[i:i + 4] for i in range(12, len(data)) if data[i:i + 4] in (b"IHDR", b"IDAT", b"IEND", b"tEXt", b"tIME")]
    assert kinds[0] == b"IHDR" and b"tEXt" not in kinds and b"tIME" not in kinds


def test_png_round_trip_through_pillow(tmp_path):
    Image = pytest.importorskip("PIL.Image")
    from pcfa_amd.helper_functions import png
    for shape in ((1, 1), (5, 7), (33, 66)):
        pix = np.random.RandomState(7).randint(0, 256, shape + (3,)).astype(np.uint8)
        path = png.write_rgb8(str(tmp_path / ("p%d.png" % shape[0])), pix)
        with Image.open(path) as im:
            assert im.mode == "RGB" and np.array_equal(np.asarray(im), pix)


def test_png_refuses_what_it_cannot_write():
    from pcfa_amd.helper_functions import png
    with pytest.raises(ValueError):
        png.encode_rgb8(np.zeros((4, 4), np.uint8))
    with pytest.raises(TypeError):
        png.encode_rgb8(np.zeros((4, 4, 3), np.float32))


def test_package_does_not_import_pillow():
    import subprocess
    import sys
    code = ("import sys; import pcfa_amd.attack_PCFA, pcfa_amd.attack_FGSM, pcfa_amd.helper_functions.png; "
            "sys.exit(int(any(m == 'PIL' or m.startswith('PIL.') for m in sys.modules)))")
    from tests.util import REPO
    assert subprocess.run([sys.executable, "-c", code], cwd=REPO).returncode == 0


def test_save_png_parses():
    from pcfa_amd.helper_functions import parsing_file
    for attack in ("pcfa", "fgsm"):
        parser = parsing_file.create_parser(stage="training", attack_type=attack)
        off = parser.parse_args([])
        assert off.save_png is False and off.png_flow_scale == "own"
        on = parser.parse_args(["--save_png", "--png_flow_scale", "shared"])
        assert on.save_png is True and on.png_flow_scale == "shared"
        with pytest.raises(SystemExit):
            parser.parse_args(["--png_flow_scale", "global"])


def test_ops_refuse_cpu_tensors():
    from pcfa_amd import hip_ops
    f, x = torch.zeros(1, 2, 4, 4), torch.zeros(1, 3, 4, 4)
    for call in (lambda: hip_ops.flow_maxlen(f), lambda: hip_ops.absmax(x), lambda: hip_ops.flow_to_rgb8(f, torch.ones(1)),
                 lambda: hip_ops.image_to_rgb8(x)):
        with pytest.raises(RuntimeError, match="no CPU fallback"):
            call()


def test_entry_points_validate_before_any_launch():
    from pcfa_amd import _hip
    lib = _hip.load()
    assert lib.pcfa_flow_maxlen_items(None, None, 1, 4, 4, None, None) == -1
    assert lib.pcfa_absmax_items(None, 1, 16, None, None) == -1
    assert lib.pcfa_flow_colour_u8(None, None, None, 1, 4, 4, None, None) == -1
    assert lib.pcfa_image_u8(None, None, None, None, None, 0, 1, 1, 4, 4, None, None) == -1


# ---------------------------------------------------------------------------------------------- file names
class _Recorder:
    """Stands in for pictures.PictureSet: keeps the file names, converts nothing."""
    names = []

    def add_image(self, paths, x, add=None, normalize_max=None, unit_input=True):
        _Recorder.names += [os.path.basename(p) for p in paths]

    def add_flow(self, paths, flow, scale):
        _Recorder.names += [os.path.basename(p) for p in paths]

    def write(self):
        return []


_STUB_OPS = types.SimpleNamespace(absmax=lambda x: torch.ones(x.shape[0]), flow_maxlen=lambda f: torch.ones(f.shape[0]))


@pytest.fixture
def recorded(monkeypatch):
    from pcfa_amd import ops
    from pcfa_amd.helper_functions import pictures
    _Recorder.names = []
    monkeypatch.setattr(pictures, "PictureSet", _Recorder)
    with ops.override_for_testing(_STUB_OPS):
        yield _Recorder


def _args(**kw):
    base = dict(save_png=True, png_flow_scale="own", joint_perturbation=False, save_frequency=1, small_save=False,
                no_save=False)
    base.update(kw)
    return Namespace(**base)


_IMG, _FLOW = torch.zeros(1, 3, 4, 6), torch.zeros(1, 2, 4, 6)
# attack_PCFA.py:267-292 of the reference, in its order
PCFA_NAMES = ["image1", "image2", "image1_delta_best", "image2_delta_best", "delta1_best", "delta2_best", "flow_pred_best",
              "flow_pred_init", "flow_target", "flow_gt"]
# attack_FGSM.py:256-278
FGSM_NAMES = ["image1", "image2", "delta1", "delta2", "flow_pred_final", "flow_pred_init", "flow_target", "flow_gt"]


def _pcfa_state(joint, has_gt, scale="own"):
    rec = types.SimpleNamespace(batch=7, delta1_min=_IMG, delta2_min=_IMG, flow_pred_min=_FLOW)
    return types.SimpleNamespace(rec=(rec,), args=_args(joint_perturbation=joint, png_flow_scale=scale), device="cpu",
                                 _pictured=set(), has_gt=has_gt, image1=_IMG, image2=_IMG, delta1=_IMG, delta2=_IMG,
                                 flow_pred=_FLOW, flow_pred_init=_FLOW, target=_FLOW, flow_gt=_FLOW if has_gt else None,
                                 _item=lambda t, b: t)


@pytest.mark.parametrize("scale", ["own", "shared"])
def test_pcfa_file_names(recorded, scale):
    from pcfa_amd.attack_PCFA import _AttackState
    _AttackState._save_pictures(_pcfa_state(False, True, scale), "out", 0)
    assert recorded.names == ["00007_%s.png" % n for n in PCFA_NAMES]


def test_pcfa_file_names_without_ground_truth_and_joint(recorded):
    from pcfa_amd.attack_PCFA import _AttackState
    _AttackState._save_pictures(_pcfa_state(False, False), "out", 0)
    assert recorded.names == ["00007_%s.png" % n for n in PCFA_NAMES if n != "flow_gt"]
    recorded.names = []
    _AttackState._save_pictures(_pcfa_state(True, True), "out", 0)      # a joint run writes no delta2 picture
    assert recorded.names == ["00007_%s.png" % n for n in PCFA_NAMES if n != "delta2_best"]


def test_fgsm_file_names(recorded):
    from pcfa_amd.attack_FGSM import FgsmAttack
    for joint, has_gt in ((False, True), (True, False)):
        recorded.names = []
        st = types.SimpleNamespace(args=_args(joint_perturbation=joint), batch=3, image1=_IMG, image2=_IMG, delta1=_IMG,
                                   delta2=_IMG, flow_pred=_FLOW, flow_pred_init=_FLOW, target=_FLOW,
                                   flow_gt=_FLOW if has_gt else None)
        FgsmAttack._save_pictures(st, "out")
        want = [n for n in FGSM_NAMES if not (joint and n == "delta2") and not (n == "flow_gt" and not has_gt)]
        assert recorded.names == ["00003_%s.png" % n for n in want]


def test_universal_file_names(recorded):
    """attack_PCFA.py:526-541 for a batch of two: item 0 under the name, item 1 under name + "_1.png"."""
    from pcfa_amd.attack_PCFA import UniversalAttack
    img2, flow2 = torch.zeros(2, 3, 4, 6), torch.zeros(2, 2, 4, 6)
    for joint in (False, True):
        recorded.names = []
        delta = torch.zeros(3, 4, 6)
        ua = types.SimpleNamespace(st=types.SimpleNamespace(image1=img2, image2=img2), deltas=lambda: (delta, delta),
                                   args=_args(joint_perturbation=joint), flow_pred=flow2, flow_pred_init=flow2)
        UniversalAttack.save_pictures(ua, "out", 5, 2)
        want = ["00005_delta1_e2.png"] + ([] if joint else ["00005_delta2_e2.png"])
        for n in ("image1_delta_e2", "image2_delta_e2", "flow_pred_e2"):
            want += ["00005_%s.png" % n, "00005_%s.png_1.png" % n]
        assert recorded.names == want


def test_attack_saves_no_picture_without_the_flag(recorded):
    from pcfa_amd.attack_PCFA import _AttackState
    st = _pcfa_state(False, True)
    st.args.save_png = False
    st.delta1 = st.delta2 = st.flow_pred = None      # save() hands None tensors to save_tensor, which skips them
    st.rec[0].delta1_min = st.rec[0].delta2_min = st.rec[0].flow_pred_min = None
    st.image1 = st.image2 = st.target = st.flow_pred_init = st.flow_gt = None
    _AttackState.save(st, None)
    assert recorded.names == []
