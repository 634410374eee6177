"""Datasets on the input side of the hot path.

``RENIDatasetHDR`` / ``RENIDatasetLDR`` / ``get_dataset`` mirror src/data/datasets.py:18-175: a directory of .exr (HDR) or
ordinary image files, naturally sorted, ``dataset[i] -> (img[3,H,W] float32, i)`` after the configured transforms.  The
EXR files are read by reni_amd/exr.py (imageio is not installed).  The reference's ``download=True`` branch fetches a
Google-Drive archive; there is no network here, so it raises.

``ResidentDataset`` wraps either of them and keeps every resolution level of every image on the GPU: a file is read and
decoded once (not once per epoch), resampled and normalised by libreni_hip.so (reni_tu_resample.hip, reni_tu_image.hip),
and a training batch is one device gather.

``SyntheticEnvMapDataset`` is the stand-in bench.py and the tests use when no dataset is on disk: values distributed like
minmax-normalised log-HDR pixels (custom_transforms.py:8-12, minmax from configs/experiment.yaml:88).
"""
import os
import re

import numpy as np
import torch
from torch.utils.data import Dataset

from . import _lib, exr
from .custom_transforms import MinMaxNormalise, Normalize, Resize, ToTensor, UnMinMaxNormlise, UnNormalise


def natsorted(names):
    """natural order ("img2" before "img10"), as natsort.natsorted gives for the dataset's file names (datasets.py:47)"""
    return sorted(names, key=lambda s: [int(t) if t.isdigit() else t for t in re.split(r"(\d+)", s)])


class RENIDatasetHDR(Dataset):
    """src/data/datasets.py:18-101"""

    def __init__(self, dataset_path, transforms=None, download=False):
        super().__init__()
        self.dataset_path = dataset_path
        self.transforms = transforms
        if download:
            raise NotImplementedError("download=True fetches the RENI_HDR archive from Google Drive (datasets.py:31-38); "
                                      "there is no network here: unpack the archive under DATASET.RENI_HDR.PATH")
        files = [f for f in os.listdir(self.dataset_path) if f.endswith(".exr")]
        self.img_names = natsorted(files)
        self.unnormalise = None
        # the dataset's min / max in the log domain, for MinMaxNormalise and its inverse (datasets.py:49-64)
        if self.transforms is not None:
            for t in self.transforms.transforms:
                if isinstance(t, MinMaxNormalise):
                    if len(t.minmax) == 0:
                        t.minmax = self.calculate_minmax()
                    self.unnormalise = UnMinMaxNormlise(t.minmax)

    def __len__(self):
        return len(self.img_names)

    def __getitem__(self, idx):
        img = self.get_image(idx)
        img = self.transforms(img)
        img = torch.nan_to_num(img)
        return img, idx

    def get_image(self, idx):
        img = exr.read_exr(os.path.join(self.dataset_path, self.img_names[idx]))
        return ToTensor()(img[:, :, :3] if img.ndim == 3 else img)

    def double_resolution(self):
        if self.transforms is not None:
            for t in self.transforms.transforms:
                if isinstance(t, Resize):
                    t.size = (t.size[0] * 2, t.size[1] * 2)

    def calculate_minmax(self):
        lo, hi = float("inf"), float("-inf")
        for idx in range(len(self)):
            img = self.get_image(idx)
            img = torch.clip(img, img[img > 0.0].min(), img[img < torch.inf].max()).log()
            lo, hi = min(lo, float(img.min())), max(hi, float(img.max()))
        return [lo, hi]


class RENIDatasetLDR(Dataset):
    """src/data/datasets.py:104-156"""

    def __init__(self, dataset_path, transforms=None, download=False):
        super().__init__()
        self.dataset_path = dataset_path
        self.transforms = transforms
        if download:
            raise NotImplementedError("download=True fetches the RENI_LDR archive from Google Drive (datasets.py:117-124); "
                                      "there is no network here: unpack the archive under DATASET.RENI_LDR.PATH")
        self.unnormalise = None
        if self.transforms is not None:
            for t in self.transforms.transforms:
                if isinstance(t, Normalize):
                    self.unnormalise = UnNormalise(t.mean, t.std)
        self.img_names = natsorted(os.listdir(self.dataset_path))

    def __len__(self):
        return len(self.img_names)

    def __getitem__(self, idx):
        img = self.get_image(idx)[:3, :, :]  # no alpha channel
        return self.transforms(img), idx

    def double_resolution(self):
        if self.transforms is not None:
            for t in self.transforms.transforms:
                if isinstance(t, Resize):
                    t.size = (t.size[0] * 2, t.size[1] * 2)

    def get_image(self, idx):
        from PIL import Image
        return ToTensor()(np.asarray(Image.open(os.path.join(self.dataset_path, self.img_names[idx]))))


def get_dataset(dataset_name, dataset_path, transform, is_hdr):
    """src/data/datasets.py:166-170"""
    if dataset_name == "RENI_HDR" or (dataset_name == "CUSTOM" and is_hdr):
        return RENIDatasetHDR(dataset_path, transform, False)
    if dataset_name == "RENI_LDR" or (dataset_name == "CUSTOM" and not is_hdr):
        return RENIDatasetLDR(dataset_path, transform, False)
    raise ValueError(f"unknown DATASET.NAME {dataset_name!r}")


class ResidentDataset(Dataset):
    """A constructed RENIDatasetHDR / RENIDatasetLDR kept on the GPU at ``levels + 1`` resolutions.

    The wrapped dataset's transform list must be ``Resize`` followed by any of ``ToTensor`` (a no-op here), ``MinMaxNormalise``
    and ``Normalize``; anything else raises ValueError.  Level j holds the images at ``Resize.size * 2^j`` in one device tensor
    [len, 3, H_j, W_j].  The first touch of image i calls ``dataset.get_image(i)`` once (the only file read), uploads it,
    resamples it FROM THE SOURCE to every level (the reference resizes the file again after ``double_resolution``; it never
    resizes a level), normalises each level on the device, and drops the source.  The wrapped ``__getitem__`` is never called.
    Files of different sizes are fine.  Filling is lazy, so a data-parallel rank decodes only the images it is given; the
    missing files of one ``batch`` are decoded by up to ``workers`` (<= 16) threads.

    ``dataset[i] -> (img [3, H, W] on the device, i)``; ``batch(idx) -> [B, 3, H, W]``: one index_select, no host work for
    cached images.  ``double_resolution()`` moves to the next level and rebuilds from the files only beyond ``levels``.

    Rotation augmentation (not in the reference; conventions in reni_amd/rotation.py).  ``batch(idx, rotations=R)`` with R
    [B, 3, 3] on the device returns the images turned by R: ONE reni_rotate_envmap launch that gathers from the level tensor
    and rotates (no index_select in front of it).  ``rotate="SO2"`` (yaw) or ``"SO3"`` makes every ``batch`` call without
    explicit rotations take a fresh one per image from the dataset's own device generator, seeded with ``rotate_seed`` and
    the data-parallel rank (``rotate_rank``, default: the process's torch.distributed rank) so that ranks draw different
    streams.  The matrices are drawn ``ROTATION_POOL`` at a time and handed out in order (a draw is some thirty small
    launches, a step one slice), so the sequence depends on the seed, the rank and the batch sizes asked for, nothing else.
    The rotation interpolates the STORED level bilinearly, i.e. normalised log radiance for an HDR dataset: that is the
    tensor the loss sees, and a sun does not bleed across four pixels as it would in linear radiance.  ``dataset[i]`` is
    never rotated (FIT_LATENT, FIT_INVERSE and the ground-truth renders use it), and with ``rotate=None`` and no
    ``rotations`` ``batch`` is the plain gather."""

    MAX_WORKERS = 16
    ROTATION_POOL = 4096

    def __init__(self, dataset, levels=0, device=None, workers=8, rotate=None, rotate_seed=0, rotate_rank=None):
        super().__init__()
        if not torch.cuda.is_available():
            raise _lib.RENILibraryError("ResidentDataset keeps the images on a GPU device and none is available; "
                                        "there is no CPU fallback")
        device = torch.device("cuda", torch.cuda.current_device()) if device is None else torch.device(device)
        if device.type != "cuda":
            raise _lib.RENILibraryError(f"ResidentDataset needs a GPU device, got {device}; there is no CPU fallback")
        if device.index is None:
            device = torch.device("cuda", torch.cuda.current_device())
        if not isinstance(dataset, (RENIDatasetHDR, RENIDatasetLDR)):
            raise ValueError(f"ResidentDataset wraps a RENIDatasetHDR or RENIDatasetLDR, got {type(dataset).__name__}")
        ts = list(dataset.transforms.transforms) if dataset.transforms is not None else []
        if not ts or not isinstance(ts[0], Resize):
            raise ValueError("ResidentDataset: the wrapped dataset's first transform must be Resize, got "
                             + (type(ts[0]).__name__ if ts else "no transforms"))
        for t in ts[1:]:
            if not isinstance(t, (ToTensor, MinMaxNormalise, Normalize)):
                raise ValueError(f"ResidentDataset: transform {type(t).__name__} is not supported on the device "
                                 "(Resize, then ToTensor / MinMaxNormalise / Normalize)")
        if int(levels) < 0:
            raise ValueError(f"levels must be >= 0, got {levels}")
        self.dataset, self.device = dataset, device
        self.workers = max(1, min(int(workers), self.MAX_WORKERS))
        self._resize = ts[0]
        self._post = [t for t in ts[1:] if not isinstance(t, ToTensor)]
        self._hdr = isinstance(dataset, RENIDatasetHDR)
        if rotate not in (None, "SO2", "SO3"):
            raise ValueError(f"rotate must be None, 'SO2' or 'SO3', got {rotate!r}")
        self.rotate = rotate
        if rotate is not None:
            if rotate_rank is None:
                import torch.distributed as dist
                rotate_rank = dist.get_rank() if dist.is_available() and dist.is_initialized() else 0
            self._rotate_gen = torch.Generator(device=device)
            self._rotate_gen.manual_seed((int(rotate_seed) * 1000003 + int(rotate_rank)) % (1 << 63))
            self._rotate_pool, self._rotate_next = None, 0
        self._allocate([(self._resize.size[0] << j, self._resize.size[1] << j) for j in range(int(levels) + 1)])

    def _allocate(self, sizes):
        self.sizes, self.level = list(sizes), 0
        self._store = [torch.empty(len(self.dataset), 3, h, w, dtype=torch.float32, device=self.device) for h, w in self.sizes]
        self._filled = np.zeros(len(self.dataset), bool)
        self._missing = len(self.dataset)

    # ------------------------------------------------------------------ pass-through surface
    @property
    def transforms(self):
        return self.dataset.transforms

    @property
    def unnormalise(self):
        return self.dataset.unnormalise

    @property
    def img_names(self):
        return self.dataset.img_names

    @property
    def size(self):
        """(H, W) of the current level"""
        return self.sizes[self.level]

    def level_tensor(self, level=None):
        """The device tensor [len, 3, H, W] of a level (rows of images not touched yet are uninitialised)."""
        return self._store[self.level if level is None else level]

    def __len__(self):
        return len(self.dataset)

    # ------------------------------------------------------------------ fill
    def _source(self, i):
        img = self.dataset.get_image(int(i))
        return img if self._hdr else img[:3, :, :]  # LDR: no alpha channel (datasets.py:146)

    def _finish(self, x):
        """the transforms after Resize (and the HDR loader's nan_to_num) of one level [1, 3, H, W] on the device"""
        from . import ops
        clean = not self._hdr
        for k, t in enumerate(self._post):
            if isinstance(t, MinMaxNormalise):
                last = self._hdr and k == len(self._post) - 1
                x = ops.minmax_normalise_batch(x, t.minmax, nan_to_num=last)
                clean = clean or last
            else:
                x = t(x)
        return x if clean else torch.nan_to_num(x)

    def _build(self, i, img):
        from . import ops
        src = img.to(self.device, torch.float32, non_blocking=False)[None]  # [1, 3, Hs, Ws]
        for j, (h, w) in enumerate(self.sizes):
            x = src if tuple(src.shape[-2:]) == (h, w) else ops.resample(src, (h, w), "bilinear")  # Resize keeps an equal size as it is
            self._store[j][i].copy_(self._finish(x)[0])
        self._filled[i] = True
        self._missing -= 1

    def fill(self, idx=None):
        """Decode, upload and build the levels of the images in ``idx`` (default: all) that are not on the device yet."""
        todo = [int(i) for i in (range(len(self)) if idx is None else idx)]
        todo = [i for i in dict.fromkeys(todo) if not self._filled[i]]
        if not todo:
            return
        if len(todo) == 1 or self.workers == 1:
            for i in todo:
                self._build(i, self._source(i))
            return
        from concurrent.futures import ThreadPoolExecutor
        with ThreadPoolExecutor(max_workers=min(self.workers, len(todo))) as pool:
            # at most `workers` decoded sources wait on the host; one at a time is on the device
            for k in range(0, len(todo), self.workers):
                chunk = todo[k:k + self.workers]
                for i, img in zip(chunk, pool.map(self._source, chunk)):
                    self._build(i, img)

    def __getitem__(self, i):
        i = int(i)
        if i < 0 or i >= len(self):
            raise IndexError(i)
        if not self._filled[i]:
            self.fill([i])
        return self._store[self.level][i].clone(), i  # a copy: UnNormalise works in place on what it is given

    def batch(self, idx, rotations=None):
        """[B, 3, H, W] of the images ``idx`` (a list or an integer tensor) at the current level; turned by ``rotations``
        [B, 3, 3] when given, else by a fresh draw per image when the dataset was built with ``rotate``."""
        if self._missing:
            self.fill(idx.tolist() if isinstance(idx, torch.Tensor) else idx)
        sel = torch.as_tensor(idx, dtype=torch.long).to(self.device)
        if rotations is None and self.rotate is None:
            return self._store[self.level].index_select(0, sel)
        from . import ops
        if rotations is None:
            rotations = self._next_rotations(sel.numel())
        return ops.rotate_envmap(self._store[self.level], rotations.to(self.device), "bilinear", "chw", index=sel)

    def _next_rotations(self, n):
        """the next n matrices [n, 3, 3] of the dataset's stream (what is left of a pool that is too short is dropped)"""
        if self._rotate_pool is None or self._rotate_next + n > self._rotate_pool.shape[0]:
            from .rotation import random_rotations
            self._rotate_pool = random_rotations(max(n, self.ROTATION_POOL), self.rotate, self._rotate_gen)
            self._rotate_next = 0
        self._rotate_next += n
        return self._rotate_pool[self._rotate_next - n:self._rotate_next]

    def double_resolution(self):
        """Multi-resolution curriculum hook (src/lightning/callbacks.py:27): the next level; beyond the last one the cache is
        rebuilt from the files at twice the size (one level)."""
        self.dataset.double_resolution()  # keeps ``transforms`` (Resize.size) telling the truth
        if self.level + 1 < len(self.sizes):
            self.level += 1
        else:
            h, w = self.sizes[self.level]
            self._store = None  # release before the larger tensor is allocated
            self._allocate([(2 * h, 2 * w)])


MINMAX = (-18.0536, 11.4633)


class SyntheticEnvMapDataset(Dataset):
    def __init__(self, n_images, height, width, seed_base=1234):
        self.n, self.h, self.w, self.seed_base = n_images, height, width, seed_base
        self.unnormalise = UnMinMaxNormlise(MINMAX)  # datasets.py:80-86: inverse of the minmax-log transform

    def __len__(self):
        return self.n

    def make(self, i, height=None, width=None):
        g = torch.Generator().manual_seed(self.seed_base + int(i))
        h, w = height or self.h, width or self.w
        logx = torch.randn(3, h, w, generator=g) * 2.0 - 3.0
        return 2.0 * (logx - MINMAX[0]) / (MINMAX[1] - MINMAX[0]) - 1.0

    def __getitem__(self, i):
        return self.make(i), i

    def double_resolution(self):
        """Multi-resolution curriculum hook (src/lightning/callbacks.py:27)."""
        self.h, self.w = 2 * self.h, 2 * self.w
