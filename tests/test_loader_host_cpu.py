"""The host statements of the device-resident training set (loader.py) against literal restatements of upstream's arithmetic, without a
GPU: placement (PadNumpy's ceil / floor split, the pad-then-slice lines of base_segmentation_dataset.py:150-181), the relation between
the common canvas and upstream's ragged planes, the replacement of empty slices, and the epoch order against a real DataLoader."""
import itertools
import math

import numpy as np
import pytest
import torch
from torch.utils.data import DataLoader

from cooperative_training_and_latent_space_data_augmentation_amd import loader as L
from cooperative_training_and_latent_space_data_augmentation_amd.augment import BatchAugmenter, crop_offsets

import loader_cases as F


def pad_numpy(a, size):
    """PadNumpy(size) by its definition: an axis shorter than size gets ceil(d / 2) zeros in front and floor(d / 2) behind."""
    d = [max(int(size[k]) - a.shape[k], 0) for k in (0, 1)]
    return np.pad(a, [(int(math.ceil(d[0] / 2)), int(math.floor(d[0] / 2))), (int(math.ceil(d[1] / 2)), int(math.floor(d[1] / 2)))])


def upstream_pair(orig_image, orig_label, new_h, new_w):
    """base_segmentation_dataset.py:150-181 for a 2-D slice, line for line"""
    h, w = orig_image.shape[0], orig_image.shape[1]
    h_s = (h - new_h) // 2
    w_s = (w - new_w) // 2
    if h < new_h:
        pad_result = np.zeros((new_h, orig_image.shape[1]), dtype=orig_image.dtype)
        pad_result[-h_s:-h_s + h] = orig_image
        orig_image = pad_result
        pad_result = np.zeros((new_h, orig_image.shape[1]), dtype=orig_label.dtype)
        pad_result[-h_s:-h_s + h] = orig_label
        orig_label = pad_result
    if w < new_w:
        pad_result = np.zeros((orig_image.shape[0], new_w), dtype=orig_image.dtype)
        pad_result[:, -w_s:-w_s + w] = orig_image
        orig_image = pad_result
        pad_result = np.zeros((orig_image.shape[0], new_w), dtype=orig_label.dtype)
        pad_result[:, -w_s:-w_s + w] = orig_label
        orig_label = pad_result
    h, w = orig_image.shape[0], orig_image.shape[1]
    h_s = (h - new_h) // 2
    w_s = (w - new_w) // 2
    assert h_s >= 0 and w_s >= 0
    # (upstream guards the next two lines with `if h_s > 0 or w_s > 0`: an axis exactly one pixel longer than the target, both starts 0,
    #  then keeps its size and the sample no longer collates.  The slice itself is the rule; it is applied always.)
    orig_image = orig_image[h_s:h_s + new_h, w_s:w_s + new_w]
    orig_label = orig_label[h_s:h_s + new_h, w_s:w_s + new_w]
    return orig_image, orig_label


def formulate_labels(label, label_map):
    new = np.zeros_like(label, dtype=np.uint8)
    for old, value in label_map.items():
        new[label == old] = value
    return new


# ------------------------------------------------------------------------------------------------ placement
@pytest.mark.parametrize("crop", F.CROPS)
def test_gather_host_is_upstreams_arithmetic(crop):
    volumes = F.make_volumes()
    slices = F.slice_list(volumes)
    lut = L.label_lut(F.LABEL_MAP)
    assert lut[7] == 0 and lut[0] == 0 and lut[1] == 3
    index = list(range(len(slices)))
    image, label, oi, ol = L.gather_host(slices, index, lut, F.DEFAULT_CANVAS, crop)
    assert image.dtype == np.float32 and label.dtype == np.int64 and oi.dtype == np.float32 and ol.dtype == np.int64
    for i, (im, la) in enumerate(slices):
        new = formulate_labels(la, F.LABEL_MAP)
        # the default canvas crops nothing: PadNumpy to the canvas size
        assert np.array_equal(image[i, 0], pad_numpy(im, F.DEFAULT_CANVAS)) and np.array_equal(label[i], pad_numpy(new, F.DEFAULT_CANVAS))
        ui, ul = upstream_pair(im, new, *crop)
        assert np.array_equal(oi[i, 0], ui) and np.array_equal(ol[i], ul)
    # a forced canvas crops the larger slices by the same rule
    for canvas in ((32, 32), (40, 40)):
        image, label = L.gather_host(slices, index, lut, canvas)
        for i, (im, la) in enumerate(slices):
            ui, ul = upstream_pair(im, formulate_labels(la, F.LABEL_MAP), *canvas)
            assert np.array_equal(image[i, 0], ui) and np.array_equal(label[i], ul)
    with pytest.raises(IndexError):
        L.gather_host(slices, [len(slices)], lut, F.DEFAULT_CANVAS)


def test_padding_is_zero_whatever_the_table_holds_at_zero():
    slices = [(np.ones((3, 3), dtype=np.float32), np.zeros((3, 3), dtype=np.uint8))]
    _, label = L.gather_host(slices, [0], L.label_lut({0: 5}), (5, 5))
    assert label[0, 1:4, 1:4].min() == 5 and label.sum() == 45


def test_placement_brute_force_and_canvas_relation():
    """Every size up to 18 on one axis.  placement is upstream's pad-then-slice; and a slice padded onto the common canvas H and then
    centre-cropped (MySpecialCrop, first row ceil((H - Hc) / 2)) lands where upstream's pad to max(h, Hp) and crop puts it exactly when
    H - max(h, Hp) is even or Hc - h is even, and one pixel away otherwise."""
    n_max, checked = 18, 0
    for h, target in itertools.product(range(1, n_max + 1), repeat=2):
        a = np.arange(1, h + 1, dtype=np.float32)[:, None]
        ui, _ = upstream_pair(a, a.astype(np.uint8), target, 1)
        assert np.array_equal(L.place_host(a, (target, 1)), ui)
    for h, hp, hc, H in itertools.product(range(1, n_max + 1), repeat=4):
        P = max(h, hp)
        if hc > P or H < P:
            continue
        checked += 1
        upstream = (P - h + 1) // 2 - crop_offsets(P, 1, hc, 1)[0]          # crop row of slice row 0
        ours = L.placement(h, H)[0] - crop_offsets(H, 1, hc, 1)[0]
        if (H - P) % 2 == 0 or (hc - h) % 2 == 0:
            assert ours == upstream, (h, hp, hc, H)
        else:
            assert abs(ours - upstream) == 1, (h, hp, hc, H)
    assert checked == 20520


# ------------------------------------------------------------------------------------------------ empty slices
def test_resolve_empty_slices():
    counts = np.array([5, 0, 3, 9, 0, 0, 4, 1, 0, 2])
    volume_of = np.array([0, 0, 0, 1, 1, 1, 1, 1, 2, 2])
    for seed in range(50):
        r = L.resolve_empty_slices(counts, volume_of, seed=seed)
        assert np.all(counts[r] != 0) and np.all(volume_of[r] == volume_of)
        assert np.array_equal(r[counts != 0], np.nonzero(counts != 0)[0])
        assert np.array_equal(r, L.resolve_empty_slices(counts, volume_of, seed=seed))
    assert len({tuple(L.resolve_empty_slices(counts, volume_of, seed=s)) for s in range(50)}) > 1
    with pytest.raises(ValueError, match="patient_b"):
        L.resolve_empty_slices(np.array([1, 0, 0]), np.array([0, 1, 1]), names=["patient_a", "patient_b"])


def test_replacement_is_uniform():
    """One empty slice, three non-empty candidates, 2,000 seeds: each candidate's count within 4 sigma of the binomial(2000, 1/3)."""
    counts, volume_of = np.array([0, 2, 2, 2]), np.zeros(4, dtype=np.int64)
    n = 2000
    hits = np.bincount([int(L.resolve_empty_slices(counts, volume_of, seed=s)[0]) for s in range(n)], minlength=4)
    assert hits[0] == 0 and hits.sum() == n
    bound = 4.0 * math.sqrt(n * (1 / 3) * (2 / 3))
    assert np.all(np.abs(hits[1:] - n / 3) <= bound), hits


def test_slice_set_on_the_host():
    volumes = F.make_volumes()
    s = L.DeviceSliceSet(volumes, F.PAD, (24, 24), label_map=F.LABEL_MAP, seed=3)
    assert s.device is None and len(s) == 12 and s.canvas == F.DEFAULT_CANVAS
    assert np.array_equal(s.counts, [np.count_nonzero(la) for _, la in F.slice_list(volumes)])
    empty = [1, 8]                                                          # (volume 0, slice 1), (volume 3, slice 2)
    assert np.array_equal(np.nonzero(s.counts == 0)[0], empty)
    assert s.resolved[1] in (0, 2) and s.resolved[8] in (6, 7, 9)
    zero = [(im, np.zeros_like(la)) if k == 2 else (im, la) for k, (im, la) in enumerate(volumes)]
    with pytest.raises(ValueError, match="'p2'"):
        L.DeviceSliceSet(zero, F.PAD, (24, 24), names=[f"p{k}" for k in range(5)])
    with pytest.raises(ValueError, match="larger than the canvas"):
        L.DeviceSliceSet(volumes, F.PAD, (24, 24), canvas=(20, 20))


def test_host_loader_batches():
    """numpy volumes, device=None: the whole path on the host statements."""
    volumes = F.make_volumes()
    s = L.DeviceSliceSet(volumes, F.PAD, (24, 24), label_map=F.LABEL_MAP, seed=3)
    g = torch.Generator()
    g.manual_seed(5)
    loader = L.DeviceBatchLoader(s, 10, augmenter=BatchAugmenter("ACDC_affine", (24, 24), seed=1), generator=g)
    twin = BatchAugmenter("ACDC_affine", (24, 24), seed=1)
    seen = []
    for image, label in loader:
        n = image.shape[0] // 2
        assert isinstance(image, np.ndarray) and image.shape == (2 * n, 1, 24, 24) and label.shape == (2 * n, 24, 24)
        assert image.dtype == np.float32 and label.dtype == np.int64
        got = L.gather_host(s.slices, loader.last_index, s.lut_host, s.canvas, s.crop_size)
        ai, al = twin.apply(got[0], got[1], twin.draw(n, *s.canvas))
        assert np.array_equal(image[:n], ai) and np.array_equal(label[:n], al)
        assert np.array_equal(image[n:], got[2]) and np.array_equal(label[n:], got[3])
        seen += [int(i) for i in loader.last_index]
    assert sorted(seen) == sorted(int(i) for i in s.resolved)


# ------------------------------------------------------------------------------------------------ epoch order
@pytest.mark.parametrize("size", [23, 24])
@pytest.mark.parametrize("drop_last", [False, True])
@pytest.mark.parametrize("shuffle", [True, False])
def test_epoch_order_is_the_dataloaders(size, drop_last, shuffle):
    g, g_ref = torch.Generator(), torch.Generator()
    g.manual_seed(11)
    g_ref.manual_seed(11)
    ref = DataLoader(range(size), batch_size=5, shuffle=shuffle, drop_last=drop_last, generator=g_ref)
    for _ in range(3):
        want = [b.tolist() for b in ref]
        got = L.epoch_order(size, 5, shuffle, drop_last, g)
        assert got == want and len(got) == len(ref)
    assert torch.equal(g.get_state(), g_ref.get_state())


@pytest.mark.parametrize("batch_size,train,val", [(1, 1, 1), (2, 1, 2), (5, 2, 5), (20, 10, 20)])
def test_batch_size_rule(batch_size, train, val):
    """train_adv_supervised_segmentation_triplet.py:101-116: batch_size // 2 (at least 1) slices per training batch with the original
    pair, the full batch size for validation."""
    assert L.train_batch_size(batch_size, True) == train and L.train_batch_size(batch_size, False) == val
    s = L.DeviceSliceSet(F.make_volumes(), F.PAD, (24, 24), label_map=F.LABEL_MAP)
    g, g_ref = torch.Generator(), torch.Generator()
    g.manual_seed(2)
    g_ref.manual_seed(2)
    loader = L.DeviceBatchLoader(s, batch_size, generator=g)
    ref = DataLoader(range(len(s)), batch_size=train, shuffle=True, drop_last=False, generator=g_ref)
    assert loader.train_batch_size == train and len(loader) == len(ref)
    assert len(L.DeviceBatchLoader(s, batch_size, keep_orig=False, shuffle=False)) == -(-len(s) // val)
    # next_batch wraps around as sample_batch does: two passes of the DataLoader, the same slices in the same batches
    want = [b.tolist() for _ in range(2) for b in ref]
    for batch in want:
        image, _ = loader.next_batch()
        assert image.shape[0] == 2 * len(batch) and np.array_equal(loader.last_index, s.resolved[batch])
