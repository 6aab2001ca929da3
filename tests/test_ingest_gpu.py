"""The dataset-ingest kernels (pcfa_amd/csrc/ingest_ops.hip) bit for bit against their host statements -- the data are
integers -- the readers on the GPU against the CPU path, and `--dataset Sintel` end to end against the same arrays handed
over as a DataLoader.  Every output lives inside a larger buffer filled with a guard value that must survive."""
import numpy as np
import pytest
import torch

from pcfa_amd.helper_functions import datasets, frame_utils, png
from tests import closure_util
from tests import png_cases as P

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda")
GUARD_BYTE, GUARD_FLOAT, MARGIN = 0xA5, -7.0, 64

# a single row, a single column, W > H, a wave boundary (64 / 65 rows), both sides of the 1024-row band boundary, three bands
UNFILTER_SHAPES = [(1, 1), (1, 7), (2, 1), (3, 2), (64, 3), (65, 5), (5, 70), (1024, 2), (1025, 2), (2049, 1)]


def _ops():
    from pcfa_amd import hip_ops
    return hip_ops


def _dev(a):
    return torch.from_numpy(np.array(a)).to(DEV)     # (a copy: arrays over bytes objects are read-only)


# ---------------------------------------------------------------------------------------------- 6. png_unfilter
@pytest.mark.parametrize("shape", UNFILTER_SHAPES, ids=lambda s: "%dx%d" % s)
def test_png_unfilter_equals_the_reference_loop(shape):
    h, w = shape
    n = 0
    for bpp in ((3, 6) if h >= 1024 else (1, 3, 4, 6)):
        row_bytes = w * bpp
        for name, scanlines, raw in P.unfilter_cases(h, w, bpp):
            want = png.unfilter_reference(scanlines, h, row_bytes, bpp)
            assert want == raw.tobytes(), (bpp, name)                   # (the loop inverts the encoder: also a CPU test)
            for lead in (MARGIN, MARGIN + 1):                           # the output at an even and an odd address
                buf = torch.full((lead + h * row_bytes + MARGIN,), GUARD_BYTE, dtype=torch.uint8, device=DEV)
                out = buf[lead:lead + h * row_bytes]
                got = _ops().png_unfilter(_dev(np.frombuffer(scanlines, np.uint8)), h, row_bytes, bpp, out=out)
                assert got.data_ptr() == out.data_ptr()
                host = buf.cpu().numpy()
                assert host[lead:lead + h * row_bytes].tobytes() == want, (bpp, name, lead)
                assert (host[:lead] == GUARD_BYTE).all() and (host[lead + h * row_bytes:] == GUARD_BYTE).all(), (bpp, name)
            n += 1
    assert n == 14 * (2 if h >= 1024 else 4)


def test_png_unfilter_allocates_and_checks():
    name, scanlines, raw = next(P.unfilter_cases(7, 5, 3))
    got = _ops().png_unfilter(_dev(np.frombuffer(scanlines, np.uint8)), 7, 15, 3)
    assert got.dtype == torch.uint8 and got.shape == (105,) and got.cpu().numpy().tobytes() == raw.tobytes()
    with pytest.raises(ValueError):
        _ops().png_unfilter(_dev(np.frombuffer(scanlines, np.uint8)), 7, 14, 3)
    with pytest.raises(RuntimeError, match="status -1"):
        _ops().png_unfilter(_dev(np.zeros(7 * 15, np.uint8)), 7, 14, 5)
    with pytest.raises(TypeError):
        _ops().png_unfilter(torch.zeros(7 * 16, device=DEV), 7, 15, 3)


# ---------------------------------------------------------------------------------------------- 7. samples_to_planar
def _targets(h, w):
    """equal, larger in both, smaller in both (crop), and mixed"""
    return [(h, w), (h + 3, w + 5), (max(h - 1, 1), max(w - 2, 1)), (h + 2, max(w - 1, 1)), (max(h - 1, 1), w + 4)]


def _planar(samples, fmt, kind, hp, wp, lead):
    h, w = samples.shape[:2]
    want = torch.nn.functional.pad(torch.from_numpy(P.planes_of(samples, fmt)), (0, wp - w, 0, hp - h), "constant", 0)
    buf = torch.full((lead + 3 * hp * wp + MARGIN,), GUARD_FLOAT, device=DEV)
    out = buf[lead:lead + 3 * hp * wp].view(3, hp, wp)
    got = _ops().samples_to_planar(_dev(P.sample_bytes(samples).reshape(-1)), h, w, kind, hp, wp, out=out)
    assert got.data_ptr() == out.data_ptr()
    host = buf.cpu()
    assert torch.equal(host[lead:lead + 3 * hp * wp].view(3, hp, wp), want), (fmt, samples.shape, hp, wp, lead)
    assert bool((host[:lead] == GUARD_FLOAT).all()) and bool((host[lead + 3 * hp * wp:] == GUARD_FLOAT).all())
    return want


@pytest.mark.parametrize("fmt", ["rgb8", "grey8", "rgba8"])
def test_samples_to_planar_8bit(fmt):
    rng = np.random.RandomState(11)
    for h, w in [(1, 1), (1, 5), (3, 4), (5, 7), (2, 33)]:
        samples = P.random_samples(fmt, h, w, rng)
        samples.reshape(-1)[:3] = (0, 255, 128)[:samples.reshape(-1)[:3].size]
        for hp, wp in _targets(h, w):
            for lead in (MARGIN, MARGIN + 1, MARGIN + 2, MARGIN + 3):    # rows at and off 16-byte alignment
                _planar(samples, fmt, fmt, hp, wp, lead)


def test_samples_to_planar_kitti_flow16():
    edge = np.array([0, 1, 32767, 32768, 32769, 65535], np.uint16)
    rng = np.random.RandomState(12)
    for h, w in [(1, 1), (1, 6), (3, 4), (5, 7), (2, 33)]:
        samples = edge[rng.randint(0, 6, (h, w, 3))]
        samples.reshape(-1)[:6] = edge[:samples.size][:6]
        for hp, wp in _targets(h, w):
            for lead in (MARGIN, MARGIN + 1):
                want = _planar(samples, "rgb16", "kitti_flow16", hp, wp, lead)
        # u and v are exact, valid is the third sample
        s = samples.astype(np.float64)
        hh, ww = min(h, hp), min(w, wp)
        assert np.array_equal(want[0, :hh, :ww].numpy().astype(np.float64), ((s[..., 0] - 32768) / 64)[:hh, :ww])
        assert np.array_equal(want[2, :hh, :ww].numpy().astype(np.float64), s[:hh, :ww, 2])
    out = _ops().samples_to_planar(_dev(P.sample_bytes(samples).reshape(-1)), 2, 33, "kitti_flow16")
    assert out.shape == (3, 2, 33) and out.dtype == torch.float32
    with pytest.raises(ValueError):
        _ops().samples_to_planar(_dev(np.zeros(12, np.uint8)), 2, 2, "rgb8", 0, 2)
    with pytest.raises(ValueError):
        _ops().samples_to_planar(_dev(np.zeros(12, np.uint8)), 2, 2, "bgr8")


# ---------------------------------------------------------------------------------------------- 8. readers
def test_readers_on_the_gpu_equal_the_cpu_path(tmp_path):
    rng = np.random.RandomState(21)
    for fmt in ("rgb8", "grey8", "rgba8"):
        samples = P.random_samples(fmt, 37, 29, rng)
        path = P.write(str(tmp_path / (fmt + ".png")), samples, fmt, list(rng.randint(0, 5, 37)), idat_chunks=3)
        for pad_to in (None, (40, 32), (30, 31)):
            got, cpu = frame_utils.read_image(path, DEV, pad_to), frame_utils.read_image(path, "cpu", pad_to)
            assert got.is_cuda and got.dtype == torch.float32 and torch.equal(got.cpu(), cpu), (fmt, pad_to)
        assert np.array_equal(cpu[:, :30, :29].numpy(), P.planes_of(samples, fmt)[:, :30])
    fl = P.random_samples("rgb16", 37, 29, rng)
    path = P.write(str(tmp_path / "flow.png"), fl, "rgb16", list(rng.randint(0, 5, 37)), idat_chunks=2)
    for pad_to in (None, (40, 32)):
        (flow, valid), (cflow, cvalid) = frame_utils.read_flow_kitti(path, DEV, pad_to), frame_utils.read_flow_kitti(path, "cpu", pad_to)
        assert flow.is_cuda and torch.equal(flow.cpu(), cflow) and torch.equal(valid.cpu(), cvalid)


def test_kitti_sample_is_375_by_1242_with_a_zero_pad(tmp_path):
    """A full-size KITTI-15 pair through the dataset on the GPU: 370 x 1224 sources, every filter type in the files."""
    made = P.kitti_tree(str(tmp_path), [(370, 1224)])
    ds = datasets.KITTI(split="training", root=str(tmp_path), has_gt=True, device=DEV)
    image1, image2, flow, valid = ds[0]
    f1, f2, fl = made[0]
    for t, planes in ((image1, P.planes_of(f1, "rgb8")), (image2, P.planes_of(f2, "rgb8")),
                      (torch.cat([flow, valid[None]]), P.planes_of(fl, "rgb16"))):
        assert t.is_cuda and tuple(t.shape) == (3, 375, 1242)
        host = t.cpu()
        assert np.array_equal(host[:, :370, :1224].numpy(), planes)
        assert float(host[:, 370:].abs().sum()) == 0.0 and float(host[:, :, 1224:].abs().sum()) == 0.0


# ---------------------------------------------------------------------------------------------- 9. end to end
class _Arrays(torch.utils.data.Dataset):
    """The pairs the test encoded, as host tensors: what the files hold, without the files."""

    def __init__(self, made, scenes):
        self.items = []
        for scene in scenes:
            frames, flows = made[scene]
            for i in range(len(frames) - 1):
                flow = torch.from_numpy(np.ascontiguousarray(np.transpose(flows[i], (2, 0, 1))))
                self.items.append((torch.from_numpy(P.planes_of(frames[i], "rgb8")),
                                   torch.from_numpy(P.planes_of(frames[i + 1], "rgb8")), flow,
                                   (flow[0].abs() < 1000) & (flow[1].abs() < 1000)))

    def __len__(self):
        return len(self.items)

    def __getitem__(self, i):
        return self.items[i]


def test_attack_from_sintel_files_equals_the_arrays(tmp_path, monkeypatch):
    """attack_l2 --dataset Sintel --dataset_root ... on two 64 x 96 pairs gives the result rows, bit for bit, of the same
    call handed a DataLoader over the arrays; and with --pairs_in_flight 2, where both pairs are decoded on the loader's
    stream and attacked on two other streams, each pair still has its solo row (the stream-order contract of datasets.py)."""
    from pcfa_amd import attack_PCFA, sharding
    made = P.sintel_tree(str(tmp_path), {"temple": 2, "alley": 2}, 64, 96)
    seen = []
    gather = sharding.gather_rows
    monkeypatch.setattr(sharding, "gather_rows", lambda rows, **kw: seen.append(sorted(rows)) or gather(rows, **kw))
    base = dict(net="PWCNet", weights="random:1234", steps=1, no_save=True, dataset="Sintel", dataset_stage="training",
                dataset_root=str(tmp_path))
    arrays = torch.utils.data.DataLoader(_Arrays(made, ["alley", "temple"]), batch_size=1, shuffle=False)
    attack_PCFA.attack_l2(closure_util.cli_args(pairs_in_flight=1, **base), data_loader=arrays, has_gt=True)
    attack_PCFA.attack_l2(closure_util.cli_args(pairs_in_flight=1, **base))
    attack_PCFA.attack_l2(closure_util.cli_args(pairs_in_flight=2, **base))
    from_arrays, from_files, in_flight = seen
    assert len(from_arrays) == 2 and [r[0] for r in from_arrays] == [0, 1] and all(len(r) == 13 for r in from_arrays)
    assert all(v == v for r in from_arrays for v in r)                 # ground truth is there: no NaN column
    assert from_files == from_arrays
    assert in_flight == from_arrays
    assert from_arrays[0] != from_arrays[1]
