"""The device-resident training set on the GPU: ctl_slice_foreground and ctl_batch_gather against the numpy statements of loader.py, bit
for bit (the gather is a copy: images are compared as int32 views, labels exactly), in guard-banded buffers, as views into the second
half of a batch, and run twice; the loader's batches against the augmenter on the uploaded host canvas; a captured `assemble`."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from oracle.guarded import Guarded, GuardedCall  # noqa: E402
from cooperative_training_and_latent_space_data_augmentation_amd import augment, ops  # noqa: E402
from cooperative_training_and_latent_space_data_augmentation_amd import loader as L  # noqa: E402
from cooperative_training_and_latent_space_data_augmentation_amd.augment import BatchAugmenter  # noqa: E402

import loader_cases as F  # noqa: E402

DEV = "cuda"
_cache = {}


def world():
    """volumes, their slices, and one device set per (canvas, crop); host references are computed once and never changed"""
    if not _cache:
        volumes = F.make_volumes()
        _cache["volumes"], _cache["slices"], _cache["lut"] = volumes, F.slice_list(volumes), L.label_lut(F.LABEL_MAP)
        _cache["sets"], _cache["ref"] = {}, {}
    return _cache


def device_set(ci, cri):
    w = world()
    if (ci, cri) not in w["sets"]:
        w["sets"][ci, cri] = L.DeviceSliceSet(w["volumes"], F.PAD, F.CROPS[cri], label_map=F.LABEL_MAP, canvas=F.CANVASES[ci], seed=3, device=DEV)
    return w["sets"][ci, cri]


def reference(ci, cri, n):
    w = world()
    if (ci, cri, n) not in w["ref"]:
        canvas = F.CANVASES[ci] or F.DEFAULT_CANVAS
        ref = L.gather_host(w["slices"], F.INDEX[n], w["lut"], canvas, F.CROPS[cri])
        for a in ref:
            a.setflags(write=False)
        w["ref"][ci, cri, n] = ref
    return w["ref"][ci, cri, n]


def same_bits(got: torch.Tensor, want: np.ndarray):
    got = got.cpu().numpy()
    assert got.shape == want.shape and got.dtype == want.dtype, (got.shape, want.shape, got.dtype, want.dtype)
    if want.dtype == np.float32:
        got, want = got.view(np.int32), want.view(np.int32)
    bad = np.nonzero(got != want)
    assert bad[0].size == 0, f"{bad[0].size} element(s) differ, first at {tuple(int(b[0]) for b in bad)}"


def index_dev(n):
    return torch.tensor(F.INDEX[n], dtype=torch.int32, device=DEV)


# ------------------------------------------------------------------------------------------------ kernels
def test_slice_foreground_is_exact():
    s = device_set(0, 0)
    want = np.asarray([np.count_nonzero(la) for _, la in world()["slices"]], dtype=np.int32)
    assert s.canvas == F.DEFAULT_CANVAS and len(s) == 12 and np.array_equal(s.counts, want) and (want == 0).sum() == 2
    g = Guarded(len(s), torch.int32, DEV, name="counts")
    for _ in range(2):
        ops.slice_foreground(s.label_arena, s.table, out=g.view((len(s),)))
        g.check_guards()
        g.check_written()
        assert np.array_equal(g.flat().cpu().numpy(), want)
        g.repoison()
    assert np.array_equal(s.resolved, L.resolve_empty_slices(want, s.volume_of, seed=3))


@pytest.mark.parametrize("ci,cri,n", F.combos())
def test_batch_gather_bit_for_bit(ci, cri, n):
    s = device_set(ci, cri)
    ref = reference(ci, cri, n)
    got = s.gather(index_dev(n), with_orig=True)
    for g, r in zip(got, ref):
        same_bits(g, r)
    again = s.gather(index_dev(n), with_orig=True)
    assert all(torch.equal(a.view(torch.int32) if a.dtype == torch.float32 else a, b.view(torch.int32) if b.dtype == torch.float32 else b)
               for a, b in zip(got, again))
    alone = s.gather(index_dev(n), with_orig=False)                        # without the pair: a launch of two planes per sample
    assert len(alone) == 2
    same_bits(alone[0], ref[0])
    same_bits(alone[1], ref[1])
    host = s.gather(np.asarray(F.INDEX[n]), with_orig=True)                # a host index: checked, uploaded, the same launch
    for g, r in zip(host, ref):
        same_bits(g, r)


@pytest.mark.parametrize("ci,cri,n", F.combos())
def test_batch_gather_in_guarded_buffers(ci, cri, n):
    s = device_set(ci, cri)
    ref = reference(ci, cri, n)
    (H, W), (hc, wc) = s.canvas, s.crop_size
    gc = GuardedCall(DEV)
    shapes = {"image": ((n, 1, H, W), torch.float32), "label": ((n, H, W), torch.int64), "orig_image": ((n, 1, hc, wc), torch.float32),
              "orig_label": ((n, hc, wc), torch.int64)}
    bufs = {k: gc.out(k, int(np.prod(shape)), dtype) for k, (shape, dtype) in shapes.items()}
    views = {k: bufs[k].view(shapes[k][0]) for k in shapes}
    idx = index_dev(n)

    def launch():
        s.gather(idx, with_orig=True, out=(views["image"], views["label"]), orig_out=(views["orig_image"], views["orig_label"]))

    gc.run(launch)                                                         # guards intact, no element left unwritten
    for k, r in zip(shapes, ref):
        same_bits(views[k], r)
    gc.rerun(launch)                                                       # and identical bits the second time


@pytest.mark.parametrize("ci,cri,n", F.combos())
def test_original_pair_as_views_into_the_second_half(ci, cri, n):
    """orig_* = batch[n:] of a [2n,...] tensor, as the loader passes them: at n * Hc * Wc elements the rows start at every alignment.
    The first half keeps its poison, the guards hold."""
    s = device_set(ci, cri)
    ref = reference(ci, cri, n)
    hc, wc = s.crop_size
    gi = Guarded(2 * n * hc * wc, torch.float32, DEV, name="batch image")
    gl = Guarded(2 * n * hc * wc, torch.int64, DEV, name="batch label")
    image, label = gi.view((2 * n, 1, hc, wc)), gl.view((2 * n, hc, wc))
    got = s.gather(index_dev(n), with_orig=True, orig_out=(image[n:], label[n:]))
    assert got[2].data_ptr() == image[n:].data_ptr() and got[3].data_ptr() == label[n:].data_ptr()
    gi.check_guards()
    gl.check_guards()
    half = n * hc * wc
    assert gi.unwritten().numel() == half and int(gi.unwritten().max()) == half - 1
    assert gl.unwritten().numel() == half and int(gl.unwritten().max()) == half - 1
    same_bits(got[0], ref[0])
    same_bits(got[1], ref[1])
    same_bits(image[n:], ref[2])
    same_bits(label[n:], ref[3])


def test_device_and_host_volumes_pack_alike():
    """device tensors (float32 / int64 and uint8, as prepare.load_volume returns them) mixed with numpy volumes: device copies for the
    former, one upload for the latter, the same batches"""
    w = world()
    mixed = []
    for k, (im, la) in enumerate(w["volumes"]):
        mixed.append((torch.from_numpy(im).to(DEV), torch.from_numpy(la).to(DEV), (1.0, 1.0, 1.0)) if k % 2 else (im, la))
    s = L.DeviceSliceSet(mixed, F.PAD, F.CROPS[1], label_map=F.LABEL_MAP, seed=3)
    assert s.device.type == "cuda" and np.array_equal(s.counts, device_set(0, 1).counts) and np.array_equal(s.resolved, device_set(0, 1).resolved)
    for g, r in zip(s.gather(index_dev(16)), reference(0, 1, 16)):
        same_bits(g, r)
    zero = [(im, np.zeros_like(la)) if k == 4 else (im, la) for k, (im, la) in enumerate(w["volumes"])]
    with pytest.raises(ValueError, match="'p4'"):
        L.DeviceSliceSet(zero, F.PAD, F.CROPS[0], device=DEV, names=[f"p{k}" for k in range(5)])


# ------------------------------------------------------------------------------------------------ loader
@pytest.mark.parametrize("policy", [None, "ACDC_affine_elastic_intensity"])
@pytest.mark.parametrize("ci,cri", [(0, 1), (2, 0)])
def test_loader_batches(policy, ci, cri):
    s = device_set(ci, cri)
    w = world()
    g = torch.Generator()
    g.manual_seed(9)
    aug = None if policy is None else BatchAugmenter(policy, s.crop_size, seed=4)
    twin = BatchAugmenter(policy or "no_aug", s.crop_size, seed=4)
    loader = L.DeviceBatchLoader(s, 10, augmenter=aug, generator=g)
    assert loader.train_batch_size == 5 and len(loader) == 3
    seen = []
    for image, label in loader:
        n = image.shape[0] // 2
        assert image.is_cuda and tuple(image.shape) == (2 * n, 1) + s.crop_size and tuple(label.shape) == (2 * n,) + s.crop_size
        assert image.dtype == torch.float32 and label.dtype == torch.int64
        ref = L.gather_host(w["slices"], loader.last_index, w["lut"], s.canvas, s.crop_size)
        params = BatchAugmenter.upload(loader.last_params, DEV)
        want = twin.apply(torch.from_numpy(ref[0]).to(DEV), torch.from_numpy(ref[1]).to(DEV), params)
        assert torch.equal(image[:n].view(torch.int32), want[0].view(torch.int32)) and torch.equal(label[:n], want[1])
        same_bits(image[n:], ref[2])
        same_bits(label[n:], ref[3])
        seen += [int(i) for i in loader.last_index]
    assert sorted(seen) == sorted(int(i) for i in s.resolved) and not set(seen) & {1, 8}          # one pass: every resolved slice once
    plain = L.DeviceBatchLoader(s, 4, keep_orig=False, shuffle=False)
    image, label = plain.next_batch()
    assert tuple(image.shape) == (4, 1) + s.crop_size and np.array_equal(plain.last_index, s.resolved[:4])


def test_captured_assemble_replays_with_refreshed_inputs():
    s = device_set(0, 0)
    n = 5
    aug = BatchAugmenter("ACDC_affine_elastic_intensity", s.crop_size, seed=6)
    loader = L.DeviceBatchLoader(s, 2 * n, augmenter=aug)
    eager = L.DeviceBatchLoader(s, 2 * n, augmenter=BatchAugmenter("ACDC_affine_elastic_intensity", s.crop_size, seed=6))
    s_index = index_dev(5).clone()
    s_p = BatchAugmenter.upload(aug.draw(n, *s.canvas), DEV)
    out = loader.empty_batch(n)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        loader.assemble(s_index, s_p, out)                                 # warm up outside the capture
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        loader.assemble(s_index, s_p, out)
    for index in ([3, 3, 9, 0, 10], [7, 2, 11, 6, 4]):
        fresh = torch.tensor(index, dtype=torch.int32, device=DEV)
        p = BatchAugmenter.upload(aug.draw(n, *s.canvas), DEV)
        s_index.copy_(fresh)
        for k in augment.DEVICE_KEYS:
            s_p[k].copy_(p[k])
        graph.replay()
        torch.cuda.synchronize()
        want = eager.assemble(fresh, p, eager.empty_batch(n))
        assert torch.equal(out[0].view(torch.int32), want[0].view(torch.int32)) and torch.equal(out[1], want[1])


def test_slice_beyond_two_to_the_31_elements():
    """An arena may pass 2^31 elements: a slice whose element offset needs 64 bits is counted and gathered like any other.  The arenas
    are allocated, not filled; only the two slices are written."""
    rng = np.random.default_rng(5)
    far = 2 ** 31 + 7
    shapes, offsets = [(9, 13), (21, 18)], [3, far]
    total = far + 21 * 18
    image_arena = torch.empty(total, dtype=torch.float32, device=DEV)
    label_arena = torch.empty(total, dtype=torch.uint8, device=DEV)
    slices = []
    for (h, w), o in zip(shapes, offsets):
        im, la = rng.normal(0, 9, (h, w)).astype(np.float32), rng.integers(0, 4, (h, w)).astype(np.uint8)
        image_arena[o:o + h * w] = torch.from_numpy(im).to(DEV).reshape(-1)
        label_arena[o:o + h * w] = torch.from_numpy(la).to(DEV).reshape(-1)
        slices.append((im, la))
    table = torch.tensor([[o, h, w] for (h, w), o in zip(shapes, offsets)], dtype=torch.int64, device=DEV)
    lut_host = L.label_lut(F.LABEL_MAP)
    counts = ops.slice_foreground(label_arena, table)
    assert np.array_equal(counts.cpu().numpy(), [np.count_nonzero(la) for _, la in slices])
    index = [1, 0, 1]
    got = ops.batch_gather(image_arena, label_arena, table, torch.tensor(index, dtype=torch.int32, device=DEV),
                           torch.from_numpy(lut_host).to(DEV), (16, 16), (20, 15))
    for g, r in zip(got, L.gather_host(slices, index, lut_host, (16, 16), (20, 15))):
        same_bits(g, r)
    del image_arena, label_arena
