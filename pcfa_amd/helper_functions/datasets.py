"""Image-pair sources for the attack loop.

What the attack needs is a DataLoader yielding (image1 [B,3,H,W] in [0,255], image2, flow_gt [B,2,H,W], valid).

`MpiSintel` and `KITTI` read the benchmark data from disk with the reference's file layout, padding rule and tuple
contract (helper_functions/datasets.py:51-190, ownutilities.prepare_dataloader:172-238), through the package's own
readers (frame_utils.py: inflate on the host, PNG filters and unpacking on the device):

  Sintel    root/<split>/<dstype>/<scene>/*.png, consecutive frames of a scene paired; root/<split>/flow/<scene>/*.flo;
            valid = |u| < 1000 & |v| < 1000
  KITTI-15  root/<split>/image_2/*_10.png paired with *_11.png; root/<split>/flow_occ/*_10.png (16-bit PNG: flow and
            valid); frames, flow and valid zero-padded or cropped to 375 x 1242

`--dataset_stage training` reads the split with ground truth; `evaluation` reads Sintel `test` / KITTI `testing`
(Paths.splits), where flow is all zeros, valid is False and has_gt is False.  The root is `--dataset_root`, else
PCFA_SINTEL_DIR / PCFA_KITTI15_DIR (Paths.config).  Scenes are walked in SORTED order: the reference walks them in
os.listdir order, which depends on the file system, so its pair indices are not reproducible from one machine to the next.

A sample is decoded on the device the attack runs on (attack_PCFA.select_device) and is COMPLETE when __getitem__ returns
it -- one synchronise of the decoding stream per sample: the lanes of --pairs_in_flight run on streams that do not order
with the stream the loader works on.  For the same reason the loader's collate launches nothing for a batch of one (the
batch dimension is a view) and synchronises after stacking a larger one.

`SyntheticPairs` needs no files: a low-pass filtered random image and a copy shifted by (3,-2) px
with additive noise from a seed, so the unattacked flow is non-degenerate.
"""
import glob
import os

import torch
import torch.nn.functional as F
from torch.utils.data import DataLoader, Dataset, Subset
from torch.utils.data.dataloader import default_collate

from . import frame_utils
from .config_paths import Paths

SHIFT_X, SHIFT_Y = 3, -2
KITTI_SIZE = (375, 1242)   # every KITTI-15 sample is padded or cropped to this (datasets.py:184-186 of the reference)


def synthetic_pair(seed, height, width):
    g = torch.Generator().manual_seed(int(seed))
    raw = torch.randint(0, 256, (1, 3, height + 16, width + 16), generator=g).float()
    smooth = F.avg_pool2d(F.pad(raw, (4, 4, 4, 4), mode='reflect'), kernel_size=9, stride=1)
    # stretch the blurred image back to a useful dynamic range
    smooth = (smooth - smooth.mean()) * 6.0 + 127.5
    image1 = smooth[0, :, 8:8 + height, 8:8 + width]
    image2 = smooth[0, :, 8 - SHIFT_Y:8 - SHIFT_Y + height, 8 - SHIFT_X:8 - SHIFT_X + width]
    image2 = image2 + 2.0 * torch.randn(image2.shape, generator=g)
    flow = torch.empty(2, height, width)
    flow[0].fill_(float(SHIFT_X))
    flow[1].fill_(float(SHIFT_Y))
    return image1.clamp(0, 255).contiguous(), image2.clamp(0, 255).contiguous(), flow


class SyntheticPairs(Dataset):
    def __init__(self, pairs, height, width, seed0=0):
        self.pairs, self.height, self.width, self.seed0 = pairs, height, width, seed0

    def __len__(self):
        return self.pairs

    def has_groundtruth(self):
        return True

    def __getitem__(self, i):
        image1, image2, flow = synthetic_pair(self.seed0 + i, self.height, self.width)
        return image1, image2, flow, torch.ones(self.height, self.width)


class _Shard(Dataset):
    """Every world-th sample starting at rank (the universal attack's local slice of each global batch)."""

    def __init__(self, base, rank, world):
        self.base, self.rank, self.world = base, rank, world

    def __len__(self):
        return len(self.base) // self.world

    def __getitem__(self, i):
        return self.base[i * self.world + self.rank]


class _FilePairs(Dataset):
    """Pairs read from disk: `image_list` of (frame 1, frame 2) paths and, with ground truth, `flow_list` aligned with it.
    Samples are decoded on `device` and complete when returned (module docstring)."""

    def __init__(self, has_gt, device):
        self.has_gt, self.device = bool(has_gt), torch.device(device)
        self.image_list, self.flow_list, self.extra_info = [], [], []
        self.pad_to = None   # (H, W): the reference's enforce_dimensions

    def __len__(self):
        return len(self.image_list)

    def has_groundtruth(self):
        return self.has_gt

    def read_flow(self, path):
        """(flow [2,H,W], valid [H,W]) on self.device, padded like the frames."""
        raise NotImplementedError

    def __getitem__(self, i):
        path1, path2 = self.image_list[i]
        image1 = frame_utils.read_image(path1, self.device, self.pad_to)
        image2 = frame_utils.read_image(path2, self.device, self.pad_to)
        if self.has_gt:
            flow, valid = self.read_flow(self.flow_list[i])
        else:   # no ground truth: a zero flow of the frames' size and valid = False, as the reference yields them
            flow, valid = torch.zeros((2,) + tuple(image1.shape[1:]), device=self.device), False
        if self.device.type == "cuda":
            torch.cuda.current_stream(self.device).synchronize()   # the sample is complete for ANY stream from here on
        return image1, image2, flow, valid

    def _refuse_empty(self, what, root, variable):
        if not self.image_list:
            raise FileNotFoundError(
                "No %s image pairs found under dataset root %r: pass --dataset_root DIR or set the environment variable "
                "%s to the directory that holds the dataset's split folders." % (what, root, variable))


class MpiSintel(_FilePairs):
    """MPI Sintel: root/<split>/<dstype>/<scene>/*.png, consecutive frames of a scene paired, scenes in sorted order (the
    reference: os.listdir order, which is not reproducible); flow from root/<split>/flow/<scene>/*.flo."""

    def __init__(self, split="training", root=None, dstype="clean", has_gt=False, device="cpu"):
        super().__init__(has_gt, device)
        root = Paths.config("sintel_mpi") if root is None else root
        image_root, flow_root = os.path.join(root, split, dstype), os.path.join(root, split, "flow")
        scenes = sorted(os.listdir(image_root)) if os.path.isdir(image_root) else []
        for scene in scenes:
            frames = sorted(glob.glob(os.path.join(image_root, scene, "*.png")))
            for i in range(len(frames) - 1):
                self.image_list.append((frames[i], frames[i + 1]))
                self.extra_info.append((scene, i))
            if self.has_gt:
                flows = sorted(glob.glob(os.path.join(flow_root, scene, "*.flo")))
                if len(flows) != max(len(frames) - 1, 0):
                    raise ValueError("Sintel scene %r: %d frames make %d pairs, but %d flow files in %s"
                                     % (scene, len(frames), max(len(frames) - 1, 0), len(flows),
                                        os.path.join(flow_root, scene)))
                self.flow_list += flows
        self._refuse_empty("MPI Sintel", root, "PCFA_SINTEL_DIR")

    def read_flow(self, path):
        return frame_utils.read_flow_sintel(path, self.device)


class KITTI(_FilePairs):
    """KITTI-15: root/<split>/image_2/*_10.png paired with *_11.png, flow and valid from root/<split>/flow_occ/*_10.png;
    everything zero-padded or cropped to 375 x 1242."""

    def __init__(self, split="training", root=None, has_gt=False, device="cpu"):
        super().__init__(has_gt, device)
        root = Paths.config("kitti15") if root is None else root
        base = os.path.join(root, split)
        first = sorted(glob.glob(os.path.join(base, "image_2", "*_10.png")))
        second = sorted(glob.glob(os.path.join(base, "image_2", "*_11.png")))
        for path1, path2 in zip(first, second):
            self.image_list.append((path1, path2))
            self.extra_info.append((os.path.basename(path1),))
        if self.has_gt:
            self.flow_list = sorted(glob.glob(os.path.join(base, "flow_occ", "*_10.png")))
            if len(self.flow_list) != len(self.image_list):
                raise ValueError("KITTI: %d image pairs but %d flow files in %s"
                                 % (len(self.image_list), len(self.flow_list), os.path.join(base, "flow_occ")))
        self.pad_to = KITTI_SIZE
        self._refuse_empty("KITTI-15", root, "PCFA_KITTI15_DIR")

    def read_flow(self, path):
        return frame_utils.read_flow_kitti(path, self.device, self.pad_to)


def _collate_complete(samples):
    """default_collate for samples that live on the GPU already, keeping them complete for every stream: a batch of one gets
    its batch dimension as a view (no launch); a larger one is stacked on the current stream, which is then synchronised."""
    fields, stacked = [], False
    for column in zip(*samples):
        if isinstance(column[0], torch.Tensor) and column[0].is_cuda:
            if len(column) == 1:
                fields.append(column[0].unsqueeze(0))
            else:
                fields.append(torch.stack(column))
                stacked = True
        else:
            fields.append(default_collate(list(column)))
    if stacked:
        torch.cuda.current_stream().synchronize()
    return fields


def _file_dataset(args):
    """The MpiSintel / KITTI dataset of args.dataset, args.dataset_stage, args.dstype and args.dataset_root, decoding on the
    device the attack runs on."""
    from ..attack_PCFA import select_device   # (attack_PCFA imports this module)
    root = getattr(args, "dataset_root", "") or None
    stage = getattr(args, "dataset_stage", "evaluation")
    if stage not in ("training", "evaluation"):
        raise ValueError("The specified mode: %s is unknown." % stage)
    train = stage == "training"
    device = select_device()
    if args.dataset == "Sintel":
        return MpiSintel(split=Paths.splits("sintel_train" if train else "sintel_eval"), root=root,
                         dstype=getattr(args, "dstype", "final"), has_gt=train, device=device)
    return KITTI(split=Paths.splits("kitti_train" if train else "kitti_eval"), root=root, has_gt=train, device=device)


def prepare_dataloader(args, batch_size=1, shuffle=False, shard=None):
    """(DataLoader, has_gt) for args.dataset (ownutilities.py:172-238): 'Sintel' and 'Kitti15' from disk (module
    docstring), 'Synthetic' from a seed.  --small_run keeps the first 32 pairs.

    `shuffle=True` uses a generator seeded identically on every rank, so all ranks walk the same
    global batch order (the reference's unseeded shuffle, attack_PCFA.py:347, is not reproducible).
    """
    collate = None
    if args.dataset in ('Sintel', 'Kitti15'):
        ds = _file_dataset(args)
        has_gt = ds.has_groundtruth()
        collate = _collate_complete
        if args.small_run:
            ds = Subset(ds, range(min(32, len(ds))))
    elif args.dataset == 'Synthetic':
        h, w = (int(v) for v in args.synthetic_size.lower().split("x"))
        n = 32 if args.small_run else args.synthetic_pairs
        ds = SyntheticPairs(n, h, w)
        has_gt = ds.has_groundtruth()
    else:
        raise ValueError("Unknown dataset %r, use 'Sintel', 'Kitti15' or 'Synthetic'." % args.dataset)
    if shard is not None and shard[1] > 1:
        ds = _Shard(ds, shard[0], shard[1])
    gen = torch.Generator().manual_seed(1234) if shuffle else None
    return DataLoader(ds, batch_size=batch_size, shuffle=shuffle, generator=gen, collate_fn=collate), has_gt
