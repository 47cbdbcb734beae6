"""Raw array + spacing in, scored patient out: prepare.load_volume / prepare.prepare_patient on the device against
prepare.prepare_patient_host, and TestSegmentationNetwork.evaluate on a pack whose tensors already live on the device.

The resampled image is within one float32 ulp of the host statement (tests/test_prep_resample_gpu.py); the normalisation, the crop and
the per-slice rescale then do the same operations on both sides.  The chain is compared bit for bit: with identical resampled bits
(the distance measured there is 0 ulp) everything after is identical too.  Labels are exact."""
import numpy as np
import pytest
import torch

from cooperative_training_and_latent_space_data_augmentation_amd import prepare

pytestmark = pytest.mark.gpu
F32 = np.float32
SPACING, NEW_SPACING = (1.5625, 1.5625, 10.0), [1.36719, 1.36719, -1]


def patient(seed, shape=(6, 40, 36)):
    rng = np.random.default_rng(seed)
    d, h, w = shape
    y, x = np.mgrid[0:h, 0:w]
    r = np.hypot((y - h / 2) / h, (x - w / 2) / w)
    label = np.zeros(shape, dtype=np.uint8)
    for c, rad in ((3, 0.42), (2, 0.3), (1, 0.18)):
        label[:, r < rad] = c
    image = (label * 150.0 + rng.gamma(2.0, 40.0, size=shape)).astype(F32)
    image[rng.random(shape) < 0.2] = 0
    return image, label


def test_prepare_patient_matches_the_host_statement():
    image, label = patient(0)
    kw = dict(spacing=SPACING, new_spacing=NEW_SPACING, normalize=True, crop_size=[32, 32])
    want = prepare.prepare_patient_host(image, label, **kw)
    for im, lb in ((image, label), (torch.from_numpy(image).cuda(), torch.from_numpy(label).cuda()), (image, label.astype(np.int64))):
        got = prepare.prepare_patient(im, lb, **kw)
        assert got["image"].is_cuda and got["label"].is_cuda and got["image"].dtype == torch.float32 and got["label"].dtype == torch.int64
        assert tuple(got["image"].shape) == (6, 1, 32, 32) and tuple(got["label"].shape) == (6, 32, 32)
        assert np.array_equal(got["label"].cpu().numpy(), want["label"])
        g = got["image"].cpu().numpy()
        print("  max |device - host| = %.3g" % float(np.abs(g - want["image"]).max()))
        assert np.array_equal(g.view(np.uint32), want["image"].view(np.uint32))
    assert want["image"].min() == 0 and want["image"].max() == 1 and len(np.unique(want["label"])) == 4


def test_load_volume_steps():
    image, label = patient(1)
    img, lab, sp = prepare.load_volume(image, label)                                     # nothing asked: an upload and a cast
    assert sp is None and lab.dtype == torch.uint8 and np.array_equal(img.cpu().numpy(), image) and np.array_equal(lab.cpu().numpy(), label)
    img, lab, sp = prepare.load_volume(image, label, spacing=SPACING, new_spacing=NEW_SPACING)
    wi, wl, wsp = prepare.resample_inplane_host(image, SPACING, NEW_SPACING, label=label)
    assert sp == wsp and tuple(img.shape) == (6, 46, 41) and np.array_equal(lab.cpu().numpy(), wl)
    assert np.array_equal(img.cpu().numpy().view(np.uint32), wi.view(np.uint32))
    img, lab, _ = prepare.load_volume(image, None, normalize=True)
    assert lab is None and np.array_equal(img.cpu().numpy().view(np.uint32), prepare.percentile_normalize_host(image, (2, 98)).view(np.uint32))
    with pytest.raises(ValueError):
        prepare.load_volume(image, label, new_spacing=NEW_SPACING)
    with pytest.raises(NotImplementedError):
        prepare.load_volume(image, label, spacing=SPACING, new_spacing=[1.36719, 1.36719, 10.0])
    padded = prepare.prepare_patient(image, label, crop_size=[44, 30], normalize_2D=False)
    want = prepare.prepare_patient_host(image, label, crop_size=[44, 30], normalize_2D=False)
    assert np.array_equal(padded["image"].cpu().numpy(), want["image"]) and np.array_equal(padded["label"].cpu().numpy(), want["label"])


class _Packs:
    """The slice of the reference dataset interface the patient-wise tester reads (the stub of tests/test_engine_gpu.py), serving
    ready packs."""
    formalized_label_dict = {0: "BG", 1: "LV", 2: "MYO", 3: "RV"}

    def __init__(self, packs):
        self.packs, self.patient_number, self._cur = packs, len(packs), None

    def get_patient_data_for_testing(self, i, crop_size=None):
        self._cur = i
        return self.packs[i]

    def get_id(self):
        return "patient%03d" % self._cur

    def get_voxel_spacing(self):
        return [10.0, 1.36719, 1.36719]


def test_tester_scores_a_device_pack_like_the_host_pack():
    from cooperative_training_and_latent_space_data_augmentation_amd.solver import AdvancedTripletReconSegmentationModel
    from cooperative_training_and_latent_space_data_augmentation_amd.tester import TestSegmentationNetwork
    torch.manual_seed(0)
    solver = AdvancedTripletReconSegmentationModel(network_type="FCN_16_standard", image_ch=1, num_classes=4, use_gpu=True)
    solver.eval()
    kw = dict(spacing=SPACING, new_spacing=NEW_SPACING, normalize=True, crop_size=[32, 32])
    device_packs = [prepare.prepare_patient(*patient(s), **kw) for s in (3, 4)]
    host_packs = [{k: v.cpu() for k, v in p.items()} for p in device_packs]
    assert all(p["image"].is_cuda and p["label"].is_cuda for p in device_packs)

    def run(packs, **opts):
        t = TestSegmentationNetwork(_Packs(packs), crop_size=None, segmentation_model=solver, metrics_list=("Dice",), **opts)
        t.run()
        return t

    on_device, on_host = run(device_packs), run(host_packs)
    rows_d, rows_h = on_device.segmentation_metric.tables, on_host.segmentation_metric.tables
    assert len(rows_d) == len(rows_h) == 2
    for a, b in zip(rows_d, rows_h):
        assert a[0] == b[0] and len(a) == len(b)
        assert all(x == y or (np.isnan(x) and np.isnan(y)) for x, y in zip(a[1:], b[1:])), (a, b)
    for pid, res in on_device.result_dict.items():                                        # keep_results: host arrays, the same ones
        for key in ("image", "label", "pred", "soft_pred"):
            assert isinstance(res[key], np.ndarray) and np.array_equal(res[key], on_host.result_dict[pid][key]), (pid, key)
    lean = run(device_packs, keep_results=False)
    assert lean.result_dict == {} and len(lean.segmentation_metric.tables) == 2
