"""Device-resident training set: the batch that upstream's `CardiacACDCDataset` + `DataLoader` assemble on the host, gathered and paired
on the device from volumes that are uploaded once.

What is reproduced (medseg/dataset_loader/base_segmentation_dataset.py:69-202, cardiac_ACDC_dataset.py:117-161, transform.py:46-97,
train_adv_supervised_segmentation_triplet.py:33-60, 110-116):
  per slice    `formulate_labels` (a 256-entry table), `PadNumpy(pad_size)` (torchsample's; defined here as: an axis shorter than pad_size
               gets ceil(d / 2) zeros in front and floor(d / 2) behind, a longer one is left alone), then the augmentation chain
               (`augment.BatchAugmenter`, which ends with MySpecialCrop and the min-max normalisation)
  the pair     `keep_orig_image_label_pair`: the raw slice and its remapped label placed on crop_size by the crop_or_pad rule (pad-before
               ceil(d / 2), crop start (h - Hc) // 2), concatenated behind the augmented half as `get_batch` does
  empty slices a slice whose raw label sums to 0 is replaced by a non-empty slice of its volume, uniformly
  epoch order  `DataLoader(shuffle, drop_last, generator)`: the same slice indices in the same batches for the same generator state

    train = DeviceSliceSet(volumes, pad_size=(224, 224), crop_size=(192, 192), label_map={0: 0, 1: 1, 2: 2, 3: 3})
    loader = DeviceBatchLoader(train, batch_size=16, augmenter=BatchAugmenter("ACDC_affine_elastic_intensity", (192, 192)))
    image, label = loader.next_batch()        # [16,1,192,192] float32, [16,192,192] int64 on the device: 8 augmented + their 8 originals

Per batch the host draws the augmentation parameters and copies `n` indices; the voxels never leave the device.  `gather_host`,
`resolve_empty_slices` and `epoch_order` are the host statements: the definitions the device path is tested against, and the whole path
for numpy volumes with device=None.  Deviations from upstream are listed in DESIGN.md ("Device-resident training set")."""
from __future__ import annotations

import random

import numpy as np
import torch

from . import ops
from .augment import BatchAugmenter


# ------------------------------------------------------------------------------------------------ host statements
def placement(a: int, target: int):
    """upstream's crop_or_pad rule on one axis (base_segmentation_dataset.py:150-181; PadNumpy is the same split): a source axis of size
    `a` on a target of size `target` -> (first target index, first source index, length)."""
    a, target = int(a), int(target)
    if a < target:
        return (target - a + 1) // 2, 0, a
    return 0, (a - target) // 2, target


def place_host(plane: np.ndarray, shape) -> np.ndarray:
    """A 2-D array on a zero canvas of `shape` by `placement` on each axis (dtype kept)."""
    out = np.zeros((int(shape[0]), int(shape[1])), dtype=plane.dtype)
    ty, sy, ly = placement(plane.shape[0], shape[0])
    tx, sx, lx = placement(plane.shape[1], shape[1])
    out[ty:ty + ly, tx:tx + lx] = plane[sy:sy + ly, sx:sx + lx]
    return out


def label_lut(label_map=None) -> np.ndarray:
    """`formulate_labels` (base_segmentation_dataset.py:190-202) as a uint8 table [256]: {old value: new value}; a value without an
    entry maps to 0, as upstream's zeros_like start does.  None: the identity."""
    if label_map is None:
        return np.arange(256, dtype=np.uint8)
    lut = np.zeros(256, dtype=np.uint8)
    for old, new in label_map.items():
        if not (0 <= int(old) <= 255 and 0 <= int(new) <= 255):
            raise ValueError(f"label_map: {old} -> {new} is outside 0..255")
        lut[int(old)] = int(new)
    return lut


def gather_host(slices, index, lut, canvas, crop=None):
    """The definition of ops.batch_gather in numpy.  slices: a sequence of (image [h,w] float32, label [h,w] uint8); index: the slices
    of the batch; lut: uint8 [256].  -> image float32 [n,1,H,W], label int64 [n,H,W] on the canvas, and with crop = (Hc, Wc) also
    orig_image [n,1,Hc,Wc], orig_label [n,Hc,Wc]: the raw slice and the remapped label placed on the crop size."""
    lut = np.asarray(lut, dtype=np.uint8)
    index = [int(i) for i in index]
    if any(i < 0 or i >= len(slices) for i in index):
        raise IndexError(f"gather_host: index outside [0, {len(slices)})")
    H, W = int(canvas[0]), int(canvas[1])
    image = np.zeros((len(index), 1, H, W), dtype=np.float32)
    label = np.zeros((len(index), H, W), dtype=np.int64)
    if crop is not None:
        orig_image = np.zeros((len(index), 1, int(crop[0]), int(crop[1])), dtype=np.float32)
        orig_label = np.zeros((len(index), int(crop[0]), int(crop[1])), dtype=np.int64)
    for b, i in enumerate(index):
        im, la = slices[i]
        im = np.asarray(im, dtype=np.float32)
        new = lut[np.asarray(la, dtype=np.uint8)]                 # remap first, pad after: the padding is 0 whatever lut[0] is
        image[b, 0] = place_host(im, (H, W))
        label[b] = place_host(new, (H, W))
        if crop is not None:
            orig_image[b, 0] = place_host(im, crop)
            orig_label[b] = place_host(new, crop)
    return (image, label) if crop is None else (image, label, orig_image, orig_label)


def resolve_empty_slices(counts, volume_of, seed: int = 0, names=None) -> np.ndarray:
    """int64 [S]: every slice's stand-in.  A slice with counts[s] != 0 stands for itself; an empty one gets a slice drawn uniformly from
    the non-empty slices of its volume with random.Random(seed), empty slices taken in index order (cardiac_ACDC_dataset.py:141-149: the
    first non-empty hit of upstream's remove / shuffle / take-first loop is uniform over them).  A volume without a non-empty slice
    raises ValueError naming it (upstream crashes there)."""
    counts = np.asarray(counts).reshape(-1)
    volume_of = np.asarray(volume_of).reshape(-1)
    if counts.shape != volume_of.shape:
        raise ValueError("resolve_empty_slices: one count and one volume id per slice")
    rng = random.Random(seed)
    resolved = np.arange(counts.size, dtype=np.int64)
    candidates = {}
    for s in range(counts.size):
        v = int(volume_of[s])
        if v not in candidates:
            candidates[v] = [int(t) for t in np.nonzero((volume_of == v) & (counts != 0))[0]]
            if not candidates[v]:
                name = names[v] if names is not None else v
                raise ValueError(f"resolve_empty_slices: volume {name!r} has no slice with a non-zero label")
        if counts[s] == 0:
            resolved[s] = candidates[v][rng.randrange(len(candidates[v]))]
    return resolved


def train_batch_size(batch_size: int, keep_orig: bool) -> int:
    """train_adv_supervised_segmentation_triplet.py:101-108: half the batch is drawn when each sample brings its original along."""
    batch_size = int(batch_size)
    if batch_size < 1:
        raise ValueError(f"batch size must be >= 1, got {batch_size}")
    return max(1, batch_size // 2) if keep_orig else batch_size


def epoch_order(size: int, batch_size: int, shuffle: bool, drop_last: bool, generator: torch.Generator):
    """The index batches of one pass over `DataLoader(range(size), batch_size, shuffle, drop_last, generator=generator)`, consuming
    `generator` as one DataLoader iterator does: the iterator's base seed (one int64 .random_()), then with shuffle the permutation
    (torch.randperm) and the second randperm that RandomSampler draws for its empty remainder when the pass ends."""
    size, batch_size = int(size), int(batch_size)
    torch.empty((), dtype=torch.int64).random_(generator=generator)
    if shuffle:
        order = torch.randperm(size, generator=generator).tolist()
        torch.randperm(size, generator=generator)
    else:
        order = list(range(size))
    batches = [order[i:i + batch_size] for i in range(0, size, batch_size)]
    if drop_last and batches and len(batches[-1]) < batch_size:
        batches.pop()
    return batches


# ------------------------------------------------------------------------------------------------ the set
def _is_device(a) -> bool:
    return torch.is_tensor(a) and a.is_cuda


def _host_array(a) -> np.ndarray:
    return a.numpy() if torch.is_tensor(a) else np.asarray(a)


class DeviceSliceSet:
    """The slices of a list of volumes, packed once.

    volumes    [(image [s,h,w] float32, label [s,h,w] uint8 / int64, ...)]: numpy arrays, host tensors or device tensors (the output of
               prepare.load_volume as it is; entries after the second are ignored).  In-plane sizes may differ between volumes; label
               values lie in 0..255.
    pad_size   PadNumpy's size; crop_size: the size of the batch (MySpecialCrop, and the target of the original pair)
    label_map  {old value: new value} (formulate_labels), None = identity
    canvas     None: the element-wise max of pad_size and the largest slice, so no slice is cropped before the augmentation; (H, W): forced
               (larger slices are then centre-cropped by the crop_or_pad rule)
    seed       of the replacement draw for empty slices (resolve_empty_slices), done once here
    device     None with any device tensor among the volumes: that tensor's device; None with host volumes only: everything stays on the
               host and runs the host statements; a device: host volumes are uploaded there through pinned memory, one copy per arena

    len(set) = number of slices (upstream's datasize).  image_arena / label_arena / table / lut: what ops.batch_gather reads;
    counts: raw foreground voxels per slice; resolved: int64 [S], the slice each index stands for."""

    def __init__(self, volumes, pad_size, crop_size, label_map=None, canvas=None, seed: int = 0, device=None, names=None):
        if not len(volumes):
            raise ValueError("DeviceSliceSet: no volumes")
        pairs = [(v[0], v[1]) for v in volumes]
        for k, (im, la) in enumerate(pairs):
            if len(im.shape) != 3 or tuple(im.shape) != tuple(la.shape) or min(im.shape) < 1:
                raise ValueError(f"DeviceSliceSet: volume {k}: expected an [s,h,w] image and a label of its shape, got {tuple(im.shape)} and "
                                 f"{tuple(la.shape)}")
        on_device = [_is_device(im) or _is_device(la) for im, la in pairs]
        if device is None and any(on_device):
            device = next(t.device for p in pairs for t in p if _is_device(t))
        self.device = None if device is None else torch.device(device)
        self.pad_size = (int(pad_size[0]), int(pad_size[1]))
        self.crop_size = (int(crop_size[0]), int(crop_size[1]))
        self.names = list(names) if names is not None else list(range(len(pairs)))
        self.lut_host = label_lut(label_map)
        shapes = [tuple(int(v) for v in im.shape) for im, _ in pairs]
        self.canvas = (max(self.pad_size[0], max(s[1] for s in shapes)), max(self.pad_size[1], max(s[2] for s in shapes))) \
            if canvas is None else (int(canvas[0]), int(canvas[1]))
        if self.crop_size[0] > self.canvas[0] or self.crop_size[1] > self.canvas[1]:
            raise ValueError(f"DeviceSliceSet: crop {self.crop_size} is larger than the canvas {self.canvas}")
        # arena layout: the host volumes first (one staging buffer, one upload), then the device volumes; the table is in slice order
        order = [k for k, d in enumerate(on_device) if not d] + [k for k, d in enumerate(on_device) if d]
        start, total = {}, 0
        for k in order:
            start[k] = total
            total += shapes[k][0] * shapes[k][1] * shapes[k][2]
        host_elems = sum(shapes[k][0] * shapes[k][1] * shapes[k][2] for k, d in enumerate(on_device) if not d)
        rows, volume_of = [], []
        for k, (s, h, w) in enumerate(shapes):
            rows += [(start[k] + i * h * w, h, w) for i in range(s)]
            volume_of += [k] * s
        self.table_host = np.asarray(rows, dtype=np.int64).reshape(-1, 3)
        self.volume_of = np.asarray(volume_of, dtype=np.int64)
        image_h, label_h = np.empty(host_elems, dtype=np.float32), np.empty(host_elems, dtype=np.uint8)
        for k, (im, la) in enumerate(pairs):
            if on_device[k]:
                continue
            n = im.shape[0] * im.shape[1] * im.shape[2]
            image_h[start[k]:start[k] + n] = _host_array(im).astype(np.float32, copy=False).reshape(-1)
            label_h[start[k]:start[k] + n] = self._label_bytes(_host_array(la), k).reshape(-1)
        if self.device is None:
            self.image_arena, self.label_arena, self.table, self.lut = image_h, label_h, self.table_host, self.lut_host
            self.slices = [(image_h[o:o + h * w].reshape(h, w), label_h[o:o + h * w].reshape(h, w)) for o, h, w in rows]
            self.counts = np.asarray([int(np.count_nonzero(la)) for _, la in self.slices], dtype=np.int32)
        else:
            self.slices = None
            self.image_arena = torch.empty(total, dtype=torch.float32, device=self.device)
            self.label_arena = torch.empty(total, dtype=torch.uint8, device=self.device)
            if host_elems:
                self.image_arena[:host_elems].copy_(torch.from_numpy(image_h).pin_memory(), non_blocking=True)
                self.label_arena[:host_elems].copy_(torch.from_numpy(label_h).pin_memory(), non_blocking=True)
            for k, (im, la) in enumerate(pairs):
                if not on_device[k]:
                    continue
                n = shapes[k][0] * shapes[k][1] * shapes[k][2]
                self.image_arena[start[k]:start[k] + n].copy_(torch.as_tensor(im).reshape(-1))
                la = torch.as_tensor(la)
                if la.dtype != torch.uint8:
                    lo, hi = (int(v) for v in torch.stack([la.min(), la.max()]).cpu())
                    if lo < 0 or hi > 255:
                        raise ValueError(f"DeviceSliceSet: volume {self.names[k]!r}: label values {lo}..{hi} are outside 0..255")
                self.label_arena[start[k]:start[k] + n].copy_(la.reshape(-1))
            self.table = torch.from_numpy(self.table_host).to(self.device)
            self.lut = torch.from_numpy(self.lut_host).to(self.device)
            self.counts = ops.slice_foreground(self.label_arena, self.table).cpu().numpy()
        self.resolved = resolve_empty_slices(self.counts, self.volume_of, seed=seed, names=self.names)

    def _label_bytes(self, la: np.ndarray, k: int) -> np.ndarray:
        if la.dtype == np.uint8:
            return la
        if la.dtype.kind not in "iu":
            raise TypeError(f"DeviceSliceSet: volume {self.names[k]!r}: labels are integers, got {la.dtype}")
        if la.min() < 0 or la.max() > 255:
            raise ValueError(f"DeviceSliceSet: volume {self.names[k]!r}: label values {la.min()}..{la.max()} are outside 0..255")
        return la.astype(np.uint8)

    def __len__(self) -> int:
        return int(self.table_host.shape[0])

    def gather(self, index, with_orig: bool = True, out=None, orig_out=None):
        """ops.batch_gather (device) or gather_host (host set) of the slices `index` names, as they are: no replacement of empty slices."""
        crop = self.crop_size if with_orig else None
        if self.device is None:
            return gather_host(self.slices, index, self.lut_host, self.canvas, crop)
        return ops.batch_gather(self.image_arena, self.label_arena, self.table, index, self.lut, self.canvas, crop, out=out, orig_out=orig_out)


# ------------------------------------------------------------------------------------------------ the loader
class DeviceBatchLoader:
    """`DataLoader(slice_set, train_batch_size, shuffle, drop_last, generator=generator)` followed by `get_batch`
    (train_adv_supervised_segmentation_triplet.py:48-60, 101-116), on the device.

    batch_size   the size of the batch the solver sees; with keep_orig max(1, batch_size // 2) slices are drawn per batch and each brings its
                 original along: [augmented ; original]
    augmenter    default BatchAugmenter("no_aug", crop_size): upstream's validate transform
    generator    a torch.Generator consumed as the DataLoader consumes it (None: a fresh one seeded from torch's global generator)

    len(loader), iteration and next_batch() (= sample_batch: wraps around into a new pass) follow the DataLoader with the same arguments
    and generator state.  A batch is (image [2n or n,1,Hc,Wc] float32, label [...,Hc,Wc] int64), device tensors for a device set, numpy
    arrays for a host set.  last_index / last_params: the resolved slice indices and the drawn parameters of the latest batch.
    assemble(index_dev, params_dev, out) is the device-only body: gather, then the augmenter into the first half, the original pair
    gathered straight into the second; no host synchronisation, capturable in a graph (index and parameters are read on the device)."""

    def __init__(self, slice_set: DeviceSliceSet, batch_size: int, augmenter: BatchAugmenter = None, keep_orig: bool = True,
                 shuffle: bool = True, drop_last: bool = False, generator: torch.Generator = None):
        self.set = slice_set
        self.keep_orig, self.shuffle, self.drop_last = bool(keep_orig), bool(shuffle), bool(drop_last)
        self.batch_size = int(batch_size)
        self.train_batch_size = train_batch_size(batch_size, keep_orig)
        self.augmenter = augmenter if augmenter is not None else BatchAugmenter("no_aug", slice_set.crop_size)
        if tuple(self.augmenter.crop_size) != tuple(slice_set.crop_size):
            raise ValueError(f"DeviceBatchLoader: the augmenter crops to {self.augmenter.crop_size}, the set to {slice_set.crop_size}")
        if generator is None:
            generator = torch.Generator()
            generator.manual_seed(int(torch.empty((), dtype=torch.int64).random_().item()))
        self.generator = generator
        self._pending = None
        self._canvas = {}
        self.last_index = self.last_params = None

    def __len__(self) -> int:
        s, b = len(self.set), self.train_batch_size
        return s // b if self.drop_last else -(-s // b)

    def _new_pass(self):
        return iter(epoch_order(len(self.set), self.train_batch_size, self.shuffle, self.drop_last, self.generator))

    def __iter__(self):
        for batch in self._new_pass():
            yield self.load(batch)

    def next_batch(self):
        if self._pending is None:
            self._pending = self._new_pass()
        batch = next(self._pending, None)
        if batch is None:
            self._pending = self._new_pass()
            batch = next(self._pending)
        return self.load(batch)

    def canvas_buffers(self, n: int):
        """The [n] canvas batch the gather writes and the augmenter reads (kept per n: a captured graph needs fixed addresses)."""
        if n not in self._canvas:
            H, W = self.set.canvas
            self._canvas[n] = (torch.empty((n, 1, H, W), dtype=torch.float32, device=self.set.device),
                               torch.empty((n, H, W), dtype=torch.int64, device=self.set.device))
        return self._canvas[n]

    def empty_batch(self, n: int):
        rows, (hc, wc) = (2 * n if self.keep_orig else n), self.set.crop_size
        return (torch.empty((rows, 1, hc, wc), dtype=torch.float32, device=self.set.device),
                torch.empty((rows, hc, wc), dtype=torch.int64, device=self.set.device))

    def assemble(self, index_dev: torch.Tensor, params_dev: dict, out):
        n = int(index_dev.shape[0])
        image, label = out
        canvas = self.canvas_buffers(n)
        s = self.set
        if self.keep_orig:
            ops.batch_gather(s.image_arena, s.label_arena, s.table, index_dev, s.lut, s.canvas, s.crop_size, out=canvas,
                             orig_out=(image[n:], label[n:]))
        else:
            ops.batch_gather(s.image_arena, s.label_arena, s.table, index_dev, s.lut, s.canvas, None, out=canvas)
        self.augmenter.apply(canvas[0], canvas[1], params_dev, out=(image[:n], label[:n]))
        return out

    def load(self, indices):
        """The batch of the slice indices `indices` (empty ones replaced by their stand-ins)."""
        index = self.set.resolved[np.asarray(indices, dtype=np.int64)]
        n = int(index.size)
        params = self.augmenter.draw(n, *self.set.canvas)
        self.last_index, self.last_params = index, params
        if self.set.device is None:
            got = self.set.gather(index, with_orig=self.keep_orig)
            image, label = self.augmenter.apply(got[0], got[1], params)
            if self.keep_orig:
                image, label = np.concatenate([image, got[2]], axis=0), np.concatenate([label, got[3]], axis=0)
            return image, label
        index_dev = torch.from_numpy(index.astype(np.int32)).pin_memory().to(self.set.device, non_blocking=True)
        return self.assemble(index_dev, BatchAugmenter.upload(params, self.set.device), self.empty_batch(n))
