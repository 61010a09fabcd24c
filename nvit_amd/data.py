"""The device-resident dataset: the first link of the input chain.  Which images form a step's batch is drawn on the
device and the uint8 batch and its labels are gathered there, so a captured train step needs nothing from the host.

    ds = DeviceDataset(images_u8, labels).to(device)        # uint8 [N,H,W,C], int64 [N]
    ld = ds.loader(batch_size=512, shuffle=True, seed=0, world_size=1, rank=0, repeats=1)
    xb = mix.batch(erase.batch(ra.batch(rrc.batch(ld.batch()))))     # ld.batch() where a uint8 tensor stood
    train_step(model, opt, xb, None)                                  # the labels come from the loader

What a `DataLoader(shuffle=True, drop_last=True)` with a `DistributedSampler` does on the host (reference train.py:256-354),
as a function of (seed, step) alone ("The device-resident dataset"; tests/loader_ref.py restates it in
numpy).  With s the device step counter, G = batch_size * world_size and S = (N * repeats) // G steps per epoch:
epoch = s // S, row i of rank r sits at position q = (s % S) * G + r * batch_size + i of the epoch and shows image
perm_{seed,epoch}(q // repeats), or q // repeats itself without shuffle.  perm is a stateless bijection of [0, N), evaluated
per element (a 4-round Feistel network on Philox words, cycle-walked), so N = 1.28 M costs what N = 50 000 costs.  Two
launches per step: nvit_loader_draw (one workgroup, advances the counter itself) and nvit_loader_gather.
"""
from __future__ import annotations

from typing import Iterator, Optional, Tuple

import torch

from . import _lib
from ._lib import call
from .crop import ResizeCenterCrop
from .ops import _s, normalize_images
from .stages import DeviceStepCounter, StagedBatch

Tensor = torch.Tensor

MAX_IMAGES = _lib.const("LOADER_MAX_IMAGES")
MAX_BATCH = _lib.const("LOADER_MAX_BATCH")
MAX_REPEATS = _lib.const("LOADER_MAX_REPEATS")
RECORD = _lib.const("LOADER_RECORD")   # int64s of the device record: epoch, step in the epoch


def _check_int(what: str, v, lo: int, hi: Optional[int] = None) -> int:
    if isinstance(v, bool) or not isinstance(v, int):
        raise TypeError(f"{what} must be an int (got {v!r})")
    if v < lo or (hi is not None and v > hi):
        raise ValueError(f"{what} must be {'>= ' + str(lo) if hi is None else 'in ' + str(lo) + '..' + str(hi)} (got {v})")
    return v


class LoaderBatch(StagedBatch):
    """A loader together with its dataset's own uint8 [N,H,W,C] tensor: what `ld.batch()` returns and
    `RandomResizedCrop.batch`, `AutoAugment.batch` and `RandAugment.batch` accept in place of a uint8 tensor.  The innermost
    stage of a chain; `.shape` is that of the gathered batch, [B,H,W,C].  Its launches yield the batch AND its labels, so
    the step around it takes y=None."""

    key, word, accepts, names = "data", "DeviceDataset loader", (), ("loader", "images")

    def __init__(self, loader: "DeviceLoader", images: Optional[Tensor] = None):
        own = loader.dataset.images
        if images is not None and images is not own:
            same = (isinstance(images, Tensor) and images.data_ptr() == own.data_ptr() and images.shape == own.shape
                    and images.dtype == own.dtype and images.device == own.device)
            if not same:
                raise ValueError("DeviceLoader.batch: a loader batch stands on its dataset's own tensor, no other")
        super().__init__(loader, own, (loader.batch_size, *own.shape[1:]))

    def rebind(self, tensor: Tensor) -> "LoaderBatch":
        return LoaderBatch(self.loader, tensor)

    def labels(self) -> Tensor:
        return self.loader.dataset.labels[:self.loader.batch_size]

    def check_step(self) -> None:
        raise TypeError("a DeviceDataset loader's batch is uint8: wrap it in AutoAugment.batch / RandAugment.batch, or in "
                        "RandomResizedCrop.batch and one of those or RandomErasing.batch")

    def _run(self, x: Tensor, y, inplace: bool):
        if y is not None:
            raise ValueError("the labels of a loader batch come from the dataset: pass y=None")
        if x is not self.loader.dataset.images:
            raise ValueError("the dataset's tensor was replaced (DeviceDataset.to) after this batch object was made")
        return self.loader()


class DeviceLoader(DeviceStepCounter):
    """`ds.loader(batch_size, shuffle=True, seed=0, world_size=1, rank=0, repeats=1)`: the shuffled, epoch-wise,
    rank-partitioned sequence of batches of a DeviceDataset, as a counter-based draw (module docstring).  drop_last: the
    (N * repeats) % G last positions of every epoch's permutation are left out.  repeats = 3 is DeiT's repeated
    augmentation: `repeats` consecutive positions show the same image (the stages behind draw per (global row index, step),
    so the copies differ).  One rank with batch G and world_size ranks with batch G / world_size see the same global batch,
    rank r rows [r * B, (r + 1) * B) of it.  The loader does not reach into the stages behind it: for their draws to be
    invariant to the split as well, rank r gives each of them `first_index = r * B` itself (a Mixup r * ((B + 1) // 2), and
    its pairs stay inside the rank's rows), as on a host-fed run.

    `ld()` draws and gathers the next batch: (uint8 [B,H,W,C], int64 [B]); `draw` and `gather` are its halves;
    `ld.batch()` is what the chain takes.  The counter lives on the device and the draw kernel advances it, one per step
    whatever accumulation_steps is; `record` is a device int64 [2] that the draw fills with (epoch, step in the epoch), for
    logging without a synchronisation.  `state_dict()` is (seed, step) and the parameters that fix the sequence;
    `load_state_dict` works in place and refuses other parameters."""

    def __init__(self, dataset: "DeviceDataset", batch_size: int, shuffle: bool = True, seed: int = 0, world_size: int = 1,
                 rank: int = 0, repeats: int = 1):
        if not isinstance(dataset, DeviceDataset):
            raise TypeError("DeviceLoader takes a DeviceDataset")
        if not isinstance(shuffle, bool):
            raise TypeError(f"shuffle must be a bool (got {shuffle!r})")
        B = _check_int("batch_size", batch_size, 1, MAX_BATCH)
        world = _check_int("world_size", world_size, 1)
        rank = _check_int("rank", rank, 0, world - 1)
        repeats = _check_int("repeats", repeats, 1, MAX_REPEATS)
        super().__init__(seed, rank * B)   # first_index: this rank's first row of the global batch
        self.dataset, self.batch_size, self.shuffle = dataset, B, shuffle
        self.world_size, self.rank, self.repeats = world, rank, repeats
        self.global_batch = B * world
        self.steps_per_epoch = (dataset.N * repeats) // self.global_batch
        if self.steps_per_epoch == 0:
            raise ValueError(f"a global batch of {self.global_batch} images is more than the dataset's {dataset.N} x "
                             f"{repeats}: no whole step per epoch (drop_last)")
        self.record: Optional[Tensor] = None
        if dataset.images.is_cuda:
            self.to(dataset.images.device)

    def to(self, device) -> "DeviceLoader":
        device = self._step_to(device)
        self.record = torch.zeros(RECORD, dtype=torch.int64).to(device)
        return self

    # ------------------------------------------------------------------ host views
    @property
    def epoch(self) -> int:
        """The epoch of the next step (reads the device counter: synchronises)."""
        return self.step // self.steps_per_epoch

    def _sequence(self) -> dict:
        return {"N": self.dataset.N, "batch_size": self.batch_size, "world_size": self.world_size, "rank": self.rank,
                "repeats": self.repeats, "shuffle": self.shuffle}

    def state_dict(self) -> dict:
        return {"seed": self.seed, "step": self.step, **self._sequence()}

    def load_state_dict(self, state: dict) -> None:
        mine = self._sequence()
        wrong = [f"{k}: {state.get(k)!r} (this loader: {mine[k]!r})" for k in mine
                 if k not in state or type(state[k]) is not type(mine[k]) or state[k] != mine[k]]
        if wrong:
            raise ValueError("DeviceLoader.load_state_dict: the state belongs to another sequence - " + "; ".join(wrong))
        super().load_state_dict(state)

    # ------------------------------------------------------------------ the launches
    def _images(self) -> Tensor:
        self._need_device()
        images = self.dataset.images
        if images.device != self.device or self.dataset.labels.device != self.device:
            raise RuntimeError("DeviceLoader: the dataset and the loader's counter live on different devices; call "
                               "DeviceDataset.to(device) and DeviceLoader.to(device)")
        return images

    def draw(self) -> Tensor:
        """int64 [B]: the dataset indices of this rank's next batch (nvit_loader_draw); advances the step counter."""
        self._images()
        idx = torch.empty(self.batch_size, device=self.device, dtype=torch.int64)
        call("nvit_loader_draw", self.seed, self._step, self.dataset.N, self.steps_per_epoch, self.global_batch,
             self.first_index, self.repeats, int(self.shuffle), idx, self.record, self.batch_size, _s())
        return idx

    def gather(self, idx: Tensor) -> Tuple[Tensor, Tensor]:
        """(images[idx] uint8 [B,H,W,C], labels[idx] int64 [B]) (nvit_loader_gather)."""
        self._images()
        return self.dataset.take(idx)

    def __call__(self) -> Tuple[Tensor, Tensor]:
        return self.gather(self.draw())

    def batch(self, images: Optional[Tensor] = None) -> LoaderBatch:
        """What `RandomResizedCrop.batch`, `AutoAugment.batch` and `RandAugment.batch` take in place of a uint8 tensor: the
        draw and the gather then run inside the step (and inside its captured graph).  images: nothing, or the dataset's own
        tensor (what `rebind` hands back)."""
        return LoaderBatch(self, images)


class DeviceDataset:
    """DeviceDataset(images, labels): a whole dataset as two tensors, uint8 [N,H,W,C] (C 1 or 3, one size per dataset) and
    int64 [N].  CIFAR is 154 MB, ImageNet at 64 px 15.7 GB: it is held in device memory, `.to(device)` if it is not there
    yet, and never copied again.  `loader(...)` is the training side, `eval_batches(...)` the evaluation side."""

    def __init__(self, images: Tensor, labels: Tensor):
        if not isinstance(images, Tensor) or images.dtype != torch.uint8:
            raise TypeError("DeviceDataset takes uint8 [N,H,W,C] images")
        if not isinstance(labels, Tensor) or labels.dtype != torch.int64:
            raise TypeError("DeviceDataset takes int64 [N] labels")
        if images.dim() != 4 or images.shape[3] not in (1, 3) or min(images.shape) < 1:
            raise ValueError(f"DeviceDataset takes uint8 [N,H,W,C] images, C 1 or 3 (got shape {tuple(images.shape)})")
        if labels.dim() != 1 or labels.shape[0] != images.shape[0]:
            raise ValueError(f"DeviceDataset takes int64 [N] labels, one per image (got shape {tuple(labels.shape)} for "
                             f"{images.shape[0]} images)")
        if images.shape[0] > MAX_IMAGES:
            raise ValueError(f"DeviceDataset holds at most {MAX_IMAGES} images")
        if images.device != labels.device:
            raise ValueError("DeviceDataset: images and labels must live on one device")
        if not images.is_contiguous() or not labels.is_contiguous():
            raise ValueError("DeviceDataset takes contiguous tensors (it keeps them, it makes no copy)")
        self.images, self.labels = images, labels

    @property
    def N(self) -> int:
        return self.images.shape[0]

    def __len__(self) -> int:
        return self.N

    @property
    def device(self):
        return self.images.device

    def to(self, device) -> "DeviceDataset":
        """Moves the two tensors (in this object; a tensor already there is kept as it is)."""
        self.images, self.labels = self.images.to(device), self.labels.to(device)
        return self

    def take(self, idx: Tensor) -> Tuple[Tensor, Tensor]:
        """(images[idx], labels[idx]) for a device int64 [B] (nvit_loader_gather): rows of H*W*C bytes, 16 bytes per lane
        where the row size and both addresses allow it."""
        if not self.images.is_cuda:
            raise RuntimeError("DeviceDataset.take runs on the HIP device (no CPU path)")
        if not isinstance(idx, Tensor) or idx.dtype != torch.int64 or idx.dim() != 1 or not 1 <= idx.shape[0] <= MAX_BATCH:
            raise ValueError(f"DeviceDataset.take: idx must be int64 [B], B in 1..{MAX_BATCH}")
        if idx.device != self.images.device or self.labels.device != self.images.device:
            raise RuntimeError("DeviceDataset.take: idx, images and labels must live on one device")
        B = idx.shape[0]
        _, H, W, C = self.images.shape
        out = torch.empty((B, H, W, C), device=self.images.device, dtype=torch.uint8)
        y = torch.empty(B, device=self.images.device, dtype=torch.int64)
        call("nvit_loader_gather", self.images, self.labels, idx.contiguous(), out, y, self.N, H * W * C, B, _s())
        return out, y

    def loader(self, batch_size: int, shuffle: bool = True, seed: int = 0, world_size: int = 1, rank: int = 0,
               repeats: int = 1) -> DeviceLoader:
        return DeviceLoader(self, batch_size, shuffle, seed, world_size, rank, repeats)

    def eval_batches(self, batch_size: int, transform: Optional[ResizeCenterCrop] = None, mean: float = 0.5,
                     std: float = 0.5) -> Iterator[tuple]:
        """(X, y) over contiguous slices of the dataset in order, the short last one included: what `validate` and
        `estimate_loss` take.  X is `transform.batch(u8[a:b])` for a ResizeCenterCrop (it then runs in front of the forward)
        and `normalize_images(u8[a:b], mean, std)` without one.  A plain Python iterator: no kernel of its own."""
        _check_int("batch_size", batch_size, 1)
        if transform is not None and not isinstance(transform, ResizeCenterCrop):
            raise TypeError("eval_batches: transform is a ResizeCenterCrop or None")
        return self._eval_batches(batch_size, transform, mean, std)

    def _eval_batches(self, B, transform, mean, std):
        for a in range(0, self.N, B):
            u8, y = self.images[a:a + B], self.labels[a:a + B]
            yield (transform.batch(u8) if transform is not None else normalize_images(u8, mean, std)), y
