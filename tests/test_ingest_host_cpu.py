"""Host side of the dataset readers (no GPU): the PNG container checks, the reconstruction loop against the test encoder
(tests/png_cases.py) and Pillow, the dataset logic on small trees, the flag and the two entry points' validation."""
import os
import struct
import zlib
from argparse import Namespace

import numpy as np
import pytest
import torch

from pcfa_amd.helper_functions import datasets, frame_utils, png
from tests import png_cases as P

SHAPES = [(1, 1), (2, 3), (7, 5), (9, 17)]


def _args(**kw):
    base = dict(dataset="Sintel", dataset_stage="training", dstype="final", small_run=False, dataset_root="",
                synthetic_size="64x96", synthetic_pairs=2)
    base.update(kw)
    return Namespace(**base)


@pytest.fixture
def cpu_device(monkeypatch):
    monkeypatch.setenv("PCFA_USE_CPU", "1")


# ---------------------------------------------------------------------------------------------- 1. the missing feature
def test_prepare_dataloader_reads_sintel_and_kitti(tmp_path, cpu_device):
    """`--dataset Sintel` / `Kitti15` give pairs (before the readers existed: NotImplementedError)."""
    made = P.sintel_tree(str(tmp_path / "sintel"), {"alley": 3}, 6, 9)
    loader, has_gt = datasets.prepare_dataloader(_args(dataset="Sintel", dataset_root=str(tmp_path / "sintel")))
    assert has_gt and len(loader) == 2
    frames, flows = made["alley"]
    for i, (image1, image2, flow, valid) in enumerate(loader):
        assert image1.shape == (1, 3, 6, 9) and image1.dtype == torch.float32 and flow.shape == (1, 2, 6, 9)
        assert np.array_equal(image1[0].numpy(), P.planes_of(frames[i], "rgb8"))
        assert np.array_equal(image2[0].numpy(), P.planes_of(frames[i + 1], "rgb8"))
        assert np.array_equal(flow[0].numpy(), np.transpose(flows[i], (2, 0, 1)))
        assert valid.shape == (1, 6, 9) and valid.dtype == torch.bool and bool(valid.all())
    kitti = P.kitti_tree(str(tmp_path / "kitti"), [(5, 8), (4, 7)])
    loader, has_gt = datasets.prepare_dataloader(_args(dataset="Kitti15", dataset_root=str(tmp_path / "kitti")))
    assert has_gt and len(loader) == 2
    for (f1, f2, fl), (image1, image2, flow, valid) in zip(kitti, loader):
        h, w = f1.shape[:2]
        assert image1.shape == (1, 3, 375, 1242) and flow.shape == (1, 2, 375, 1242) and valid.shape == (1, 375, 1242)
        assert np.array_equal(image1[0, :, :h, :w].numpy(), P.planes_of(f1, "rgb8"))
        assert np.array_equal(image2[0, :, :h, :w].numpy(), P.planes_of(f2, "rgb8"))
        want = P.planes_of(fl, "rgb16")
        assert np.array_equal(flow[0, :, :h, :w].numpy(), want[:2]) and np.array_equal(valid[0, :h, :w].numpy(), want[2])
        for t in (image1, image2, flow, valid.unsqueeze(1)):
            assert float(t[0, :, h:].abs().sum()) == 0.0 and float(t[0, :, :, w:].abs().sum()) == 0.0


# ---------------------------------------------------------------------------------------------- 2. reconstruction
@pytest.mark.parametrize("fmt", sorted(P.FORMATS))
@pytest.mark.parametrize("shape", SHAPES)
def test_unfilter_reference_inverts_the_encoder(fmt, shape):
    h, w = shape
    bpp = P.FORMATS[fmt][3]
    n = 0
    for name, scanlines, raw in P.unfilter_cases(h, w, bpp):
        assert png.unfilter_reference(scanlines, h, w * bpp, bpp) == raw.tobytes(), name
        n += 1
    assert n == 14


@pytest.mark.parametrize("fmt", sorted(P.FORMATS))
def test_decode_round_trip_with_several_idat_chunks(fmt):
    ctype, depth, _, bpp = P.FORMATS[fmt]
    for h, w in SHAPES:
        rng = np.random.RandomState(h * 31 + w)
        samples = P.random_samples(fmt, h, w, rng)
        data = P.encode(samples, fmt, [y % 5 for y in range(h)], idat_chunks=3)
        assert data.count(b"IDAT") >= 3
        got = png.decode_header_and_scanlines(data)
        assert got[:4] == (w, h, depth, ctype) and len(got[4]) == h * (1 + w * bpp)
        assert png.unfilter_reference(got[4], h, w * bpp, bpp) == P.sample_bytes(samples).tobytes()


@pytest.mark.parametrize("fmt,mode", [("rgb8", "RGB"), ("grey8", "L"), ("rgba8", "RGBA")])
def test_pillow_decodes_the_test_files_to_the_same_samples(fmt, mode, tmp_path):
    Image = pytest.importorskip("PIL.Image")
    for h, w in SHAPES:
        rng = np.random.RandomState(h + 7 * w)
        for name, plan in P.plans(h, rng):
            samples = P.EDGE_BYTES[rng.randint(0, 7, (h, w, P.FORMATS[fmt][2]))]
            path = P.write(str(tmp_path / ("%s_%d_%d_%s.png" % (fmt, h, w, name))), samples, fmt, plan, idat_chunks=3)
            with Image.open(path) as im:
                assert im.mode == mode
                assert np.array_equal(np.asarray(im).reshape(samples.shape), samples), (h, w, name)
            assert np.array_equal(frame_utils.read_image(path).numpy(), P.planes_of(samples, fmt)), (h, w, name)


def test_readers_on_the_cpu(tmp_path):
    rng = np.random.RandomState(3)
    for fmt in ("rgb8", "grey8", "rgba8"):
        samples = P.random_samples(fmt, 7, 5, rng)
        path = P.write(str(tmp_path / (fmt + ".png")), samples, fmt)
        want = P.planes_of(samples, fmt)
        assert np.array_equal(frame_utils.read_image(path).numpy(), want)
        for hp, wp in ((9, 8), (4, 3), (9, 2), (3, 11)):
            padded = torch.nn.functional.pad(torch.from_numpy(want), (0, wp - 5, 0, hp - 7), "constant", 0)
            assert torch.equal(frame_utils.read_image(path, pad_to=(hp, wp)), padded), (fmt, hp, wp)
    fl = np.array([0, 1, 32767, 32768, 32769, 65535], np.uint16)[rng.randint(0, 6, (4, 6, 3))]
    path = P.write(str(tmp_path / "flow.png"), fl, "rgb16")
    flow, valid = frame_utils.read_flow_kitti(path)
    assert np.array_equal(flow.numpy(), P.planes_of(fl, "rgb16")[:2]) and np.array_equal(valid.numpy(), fl[..., 2])
    with pytest.raises(ValueError, match="16-bit"):
        frame_utils.read_image(path)
    with pytest.raises(ValueError, match="8-bit"):
        frame_utils.read_flow_kitti(str(tmp_path / "rgb8.png"))
    uv = rng.randn(3, 4, 2).astype(np.float32)
    assert np.array_equal(frame_utils.read_flo(P.write_flo(str(tmp_path / "a" / "x.flo"), uv)), uv)
    with open(str(tmp_path / "bad.flo"), "wb") as f:
        f.write(b"\0" * 20)
    with pytest.raises(ValueError, match="magic"):
        frame_utils.read_flo(str(tmp_path / "bad.flo"))


# ---------------------------------------------------------------------------------------------- 3. container
def _good():
    samples = P.random_samples("rgb8", 4, 5, np.random.RandomState(0))
    return samples, P.encode(samples, "rgb8", [0, 1, 3, 4])


def _with_scanlines(scanlines, h=4, w=5):
    return P.encode(np.zeros((h, w, 3), np.uint8), "rgb8", None, scanlines=scanlines)


def test_container_accepts_the_good_file():
    samples, data = _good()
    w, h, depth, ctype, scan = png.decode_header_and_scanlines(data)
    assert (w, h, depth, ctype) == (5, 4, 8, 2)
    assert png.unfilter_reference(scan, 4, 15, 3) == samples.tobytes()


def test_container_refuses_broken_files():
    samples, data = _good()
    scan = P.filter_rows(P.sample_bytes(samples), 3, [0, 1, 3, 4])
    with pytest.raises(ValueError, match="signature"):
        png.decode_header_and_scanlines(b"\x89PNX" + data[4:])
    flipped = bytearray(data)
    flipped[data.index(b"IDAT") + 6] ^= 1
    with pytest.raises(ValueError, match="CRC"):
        png.decode_header_and_scanlines(bytes(flipped))
    with pytest.raises(ValueError, match="truncated"):
        png.decode_header_and_scanlines(data[:data.index(b"IDAT") + 9])
    # an IDAT chunk that is whole but whose deflate stream stops early
    z = zlib.compress(scan, 6)
    short = P.SIGNATURE + P.chunk(b"IHDR", struct.pack(">IIBBBBB", 5, 4, 8, 2, 0, 0, 0)) + P.chunk(b"IDAT", z[:-6]) \
        + P.chunk(b"IEND", b"")
    with pytest.raises(ValueError, match="inflate|inflated length"):
        png.decode_header_and_scanlines(short)
    for off_by_one in (scan[:-1], scan + b"\0"):
        with pytest.raises(ValueError, match="inflated length"):
            png.decode_header_and_scanlines(_with_scanlines(off_by_one))
    five = bytearray(scan)
    five[2 * 16] = 5
    with pytest.raises(ValueError, match="filter type"):
        png.decode_header_and_scanlines(_with_scanlines(bytes(five)))
    with pytest.raises(ValueError, match="IHDR"):
        png.decode_header_and_scanlines(P.SIGNATURE + P.chunk(b"IDAT", z) + P.chunk(b"IEND", b""))
    with pytest.raises(ValueError, match="IEND"):
        png.decode_header_and_scanlines(data[:-12])


@pytest.mark.parametrize("what,ihdr", [("interlace", (5, 4, 8, 2, 0, 0, 1)), ("format", (5, 4, 8, 3, 0, 0, 0)),
                                       ("format", (5, 4, 4, 0, 0, 0, 0)), ("format", (5, 4, 16, 0, 0, 0, 0)),
                                       ("compression", (5, 4, 8, 2, 1, 0, 0)), ("filter method", (5, 4, 8, 2, 0, 1, 0))])
def test_container_refuses_what_is_not_served(what, ihdr):
    """Adam7 interlace, palette images, depth 4, 16-bit grey; unknown compression and filter methods."""
    data = P.encode(np.zeros((4, 5, 3), np.uint8), "rgb8", [0] * 4, ihdr_override=struct.pack(">IIBBBBB", *ihdr))
    with pytest.raises(ValueError, match=what):
        png.decode_header_and_scanlines(data)


def test_unfilter_reference_checks_its_input():
    with pytest.raises(ValueError):
        png.unfilter_reference(b"\0" * 9, 2, 4, 1)
    with pytest.raises(ValueError, match="filter type"):
        png.unfilter_reference(b"\5abc", 1, 3, 3)


# ---------------------------------------------------------------------------------------------- 4. dataset logic
def test_sintel_pairing_order_and_flow_alignment(tmp_path, cpu_device):
    root = str(tmp_path)
    # created out of order; a scene with one frame yields nothing
    made = P.sintel_tree(root, {"market": 3, "alley": 2, "single": 1, "bamboo": 4}, 4, 6)
    ds = datasets.MpiSintel(split="training", root=root, dstype="final", has_gt=True)
    assert [info for info in ds.extra_info] == [("alley", 0), ("bamboo", 0), ("bamboo", 1), ("bamboo", 2), ("market", 0),
                                                ("market", 1)]
    assert len(ds) == 6 and len(ds.flow_list) == 6
    for (scene, i), (p1, p2), fl in zip(ds.extra_info, ds.image_list, ds.flow_list):
        assert p1.endswith(os.path.join(scene, "frame_%04d.png" % (i + 1)))
        assert p2.endswith(os.path.join(scene, "frame_%04d.png" % (i + 2)))
        assert fl.endswith(os.path.join("flow", scene, "frame_%04d.flo" % (i + 1)))
    image1, image2, flow, valid = ds[3]
    assert np.array_equal(image2.numpy(), P.planes_of(made["bamboo"][0][3], "rgb8"))
    assert np.array_equal(flow.numpy(), np.transpose(made["bamboo"][1][2], (2, 0, 1)))
    # valid = |u| < 1000 & |v| < 1000
    big = made["alley"][1][0].copy()
    big[0, 0, 0], big[1, 2, 1], big[2, 3, 0] = 1000.0, -1500.0, 999.0
    P.write_flo(ds.flow_list[0], big)
    valid = ds[0][3].numpy()
    assert not valid[0, 0] and not valid[1, 2] and valid[2, 3] and valid.sum() == valid.size - 2
    # a scene whose flow files do not match its pairs is named
    os.remove(ds.flow_list[-1])
    with pytest.raises(ValueError, match="market"):
        datasets.MpiSintel(split="training", root=root, dstype="final", has_gt=True)


def test_evaluation_stage_has_no_ground_truth(tmp_path, cpu_device):
    P.sintel_tree(str(tmp_path / "s"), {"a": 2}, 4, 6, split="test", with_flow=False)
    loader, has_gt = datasets.prepare_dataloader(_args(dataset_stage="evaluation", dataset_root=str(tmp_path / "s")))
    assert has_gt is False and len(loader) == 1
    image1, image2, flow, valid = next(iter(loader))
    assert flow.shape == (1, 2, 4, 6) and float(flow.abs().sum()) == 0.0 and not bool(valid.any())
    P.kitti_tree(str(tmp_path / "k"), [(3, 5)], split="testing", with_flow=False)
    loader, has_gt = datasets.prepare_dataloader(_args(dataset="Kitti15", dataset_stage="evaluation",
                                                       dataset_root=str(tmp_path / "k")))
    assert has_gt is False
    image1, image2, flow, valid = next(iter(loader))
    assert image1.shape == (1, 3, 375, 1242) and flow.shape == (1, 2, 375, 1242)
    assert float(flow.abs().sum()) == 0.0 and not bool(valid.any())
    # the training split is not there
    with pytest.raises(FileNotFoundError):
        datasets.prepare_dataloader(_args(dataset="Kitti15", dataset_stage="training", dataset_root=str(tmp_path / "k")))


def test_kitti_sizes_come_out_375_by_1242(tmp_path, cpu_device, monkeypatch):
    """370 x 1224 is zero-padded, 376 x 1241 is cropped in H and padded in W.  The files use filter type 0 only and the
    byte loop is replaced by its type-0 case (strip the filter bytes): this test is about the dataset's padding, and
    seconds of interpreter time per frame would buy nothing (the full-size decode runs on the GPU: test_ingest_gpu.py)."""
    def strip(scanlines, h, row_bytes, bpp):
        rows = np.frombuffer(scanlines, np.uint8).reshape(h, 1 + row_bytes)
        assert not rows[:, 0].any()
        return rows[:, 1:].tobytes()
    monkeypatch.setattr(png, "unfilter_reference", strip)
    rng = np.random.RandomState(5)
    sizes = [(370, 1224), (376, 1241)]
    made = []
    for i, (h, w) in enumerate(sizes):
        f1, fl = P.random_samples("rgb8", h, w, rng), P.random_samples("rgb16", h, w, rng)
        P.write(str(tmp_path / "training" / "image_2" / ("%06d_10.png" % i)), f1, "rgb8", [0] * h)
        P.write(str(tmp_path / "training" / "image_2" / ("%06d_11.png" % i)), f1[::-1].copy(), "rgb8", [0] * h)
        P.write(str(tmp_path / "training" / "flow_occ" / ("%06d_10.png" % i)), fl, "rgb16", [0] * h)
        made.append((f1, fl))
    ds = datasets.KITTI(split="training", root=str(tmp_path), has_gt=True)
    for (h, w), (f1, fl), (image1, image2, flow, valid) in zip(sizes, made, ds):
        assert image1.shape == (3, 375, 1242) and image2.shape == (3, 375, 1242)
        assert flow.shape == (2, 375, 1242) and valid.shape == (375, 1242)
        hh = min(h, 375)
        assert np.array_equal(image1[:, :hh, :w].numpy(), P.planes_of(f1, "rgb8")[:, :hh])
        assert np.array_equal(image2[:, :hh, :w].numpy(), P.planes_of(f1[::-1], "rgb8")[:, :hh])
        want = P.planes_of(fl, "rgb16")[:, :hh]
        assert np.array_equal(flow[:, :hh, :w].numpy(), want[:2]) and np.array_equal(valid[:hh, :w].numpy(), want[2])
        for t in (image1, image2, flow, valid[None]):
            assert float(t[:, hh:].abs().sum()) == 0.0 and float(t[:, :, w:].abs().sum()) == 0.0
    assert image1.shape[1] < 376   # the second source lost its last row


def test_small_run_takes_the_first_32_pairs(tmp_path, cpu_device):
    P.sintel_tree(str(tmp_path), {"b": 20, "a": 16}, 2, 3)
    loader, _ = datasets.prepare_dataloader(_args(small_run=True, dataset_root=str(tmp_path)))
    assert len(loader) == 32
    full, _ = datasets.prepare_dataloader(_args(dataset_root=str(tmp_path)))
    assert len(full) == 34
    assert loader.dataset.dataset.extra_info[:32] == [("a", i) for i in range(15)] + [("b", i) for i in range(17)]


def test_empty_root_names_the_variable(tmp_path, cpu_device, monkeypatch):
    monkeypatch.delenv("PCFA_SINTEL_DIR", raising=False)
    monkeypatch.delenv("PCFA_KITTI15_DIR", raising=False)
    with pytest.raises(FileNotFoundError, match="PCFA_SINTEL_DIR") as e:
        datasets.prepare_dataloader(_args(dataset_root=str(tmp_path)))
    assert str(tmp_path) in str(e.value)
    with pytest.raises(FileNotFoundError, match="PCFA_KITTI15_DIR"):
        datasets.prepare_dataloader(_args(dataset="Kitti15", dataset_root=str(tmp_path / "missing")))
    with pytest.raises(FileNotFoundError, match="PCFA_KITTI15_DIR"):
        datasets.prepare_dataloader(_args(dataset="Kitti15"))
    # the environment variable is the root when the flag is empty
    P.sintel_tree(str(tmp_path / "env"), {"a": 2}, 2, 3)
    monkeypatch.setenv("PCFA_SINTEL_DIR", str(tmp_path / "env"))
    assert len(datasets.prepare_dataloader(_args())[0]) == 1


def test_dataset_root_parses():
    from pcfa_amd.helper_functions import parsing_file
    for stage, attack in (("training", "pcfa"), ("evaluation", "pcfa"), ("training", "fgsm")):
        parser = parsing_file.create_parser(stage=stage, attack_type=attack)
        assert parser.parse_args([]).dataset_root == ""
        assert parser.parse_args(["--dataset", "Sintel", "--dataset_root", "/data/sintel"]).dataset_root == "/data/sintel"


def test_synthetic_loader_is_unchanged():
    loader, has_gt = datasets.prepare_dataloader(_args(dataset="Synthetic"))
    assert has_gt and len(loader) == 2 and loader.collate_fn is torch.utils.data.dataloader.default_collate
    image1, _, flow, valid = next(iter(loader))
    want = datasets.synthetic_pair(0, 64, 96)
    assert torch.equal(image1[0], want[0]) and torch.equal(flow[0], want[2]) and valid.shape == (1, 64, 96)


# ---------------------------------------------------------------------------------------------- 5. entry points
def test_entry_points_validate_before_any_launch():
    from pcfa_amd import _hip
    lib = _hip.load()
    assert lib.pcfa_png_unfilter(None, None, 4, 12, 3, None) == -1
    assert lib.pcfa_samples_to_planar(None, 4, 4, 0, None, 4, 4, None) == -1
    one = 0x1000   # never dereferenced: every call below is refused before a launch
    for h, row_bytes, bpp in ((0, 12, 3), (4, 0, 3), (4, 12, 2), (4, 12, 5), (4, 13, 3), (4, 12, 0), (-1, 12, 3)):
        assert lib.pcfa_png_unfilter(one, one, h, row_bytes, bpp, None) == -1, (h, row_bytes, bpp)
    for h, w, kind, hp, wp in ((0, 4, 0, 4, 4), (4, 0, 0, 4, 4), (4, 4, -1, 4, 4), (4, 4, 4, 4, 4), (4, 4, 0, 0, 4),
                               (4, 4, 0, 4, 0)):
        assert lib.pcfa_samples_to_planar(one, h, w, kind, one, hp, wp, None) == -1, (h, w, kind, hp, wp)
    assert lib.pcfa_samples_to_planar(one, 4, 4, 0, one + 2, 4, 4, None) == -1     # out is not 4-byte aligned


def test_ops_refuse_cpu_tensors():
    from pcfa_amd import hip_ops
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        hip_ops.png_unfilter(torch.zeros(8, dtype=torch.uint8), 2, 3, 3)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        hip_ops.samples_to_planar(torch.zeros(12, dtype=torch.uint8), 2, 2, "rgb8")
