"""TestSegmentationNetwork(native_grid=True): the logits of a prepared patient are put back on the native grid on the device, and
post-processing and the score table are those of the native volume; with native_grid=False nothing changes.

The native prediction is compared with prepare.restore_scores_host of the kept logits wherever the host's top-two margin exceeds
1e-9 * max |v|; at most 1 % of the voxels may fall under that bound (measured on an MI355X: 0 of 8640 per patient, both modes)."""
import numpy as np
import pytest
import torch

from cooperative_training_and_latent_space_data_augmentation_amd import ops, prepare
from cooperative_training_and_latent_space_data_augmentation_amd.metrics import runningMySegmentationScore

import restore_cases as R

pytestmark = pytest.mark.gpu
F32 = np.float32
SHAPE, SPACING, NEW_SPACING, WINDOW = (6, 40, 36), (1.5625, 1.5625, 10.0), [1.36719, 1.36719, -1], [32, 32]
METRICS = ("Dice", "VolError")


def patient(seed, shape=SHAPE):
    """the phantom of tests/test_prepare_gpu.py: three nested discs under gamma noise with holes"""
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


class _Packs:
    """The slice of the reference dataset interface the patient-wise tester reads, serving ready packs; the labels it serves for
    scoring are native, so the spacing it reports is the native one."""
    formalized_label_dict = {0: "BG", 1: "LV", 2: "MYO", 3: "RV"}

    def __init__(self, packs):
        self.packs, self.patient_number, self._cur = packs, len(packs), None

    def get_patient_data_for_testing(self, i, crop_size=None):
        self._cur = i
        return self.packs[i]

    def get_id(self):
        return "patient%03d" % self._cur

    def get_voxel_spacing(self):
        return [10.0, 1.5625, 1.5625]


@pytest.fixture(scope="module")
def solver():
    from cooperative_training_and_latent_space_data_augmentation_amd.solver import AdvancedTripletReconSegmentationModel
    torch.manual_seed(0)
    s = AdvancedTripletReconSegmentationModel(network_type="FCN_16_standard", image_ch=1, num_classes=4, use_gpu=True)
    s.eval()
    return s


@pytest.fixture(scope="module")
def packs():
    kw = dict(spacing=SPACING, new_spacing=NEW_SPACING, normalize=True, crop_size=WINDOW)
    return [prepare.prepare_patient(*patient(s), want_geometry=True, **kw) for s in (3, 4)]


def run(solver, packs, **opts):
    from cooperative_training_and_latent_space_data_augmentation_amd.tester import TestSegmentationNetwork
    t = TestSegmentationNetwork(_Packs(packs), crop_size=None, segmentation_model=solver, metrics_list=METRICS, **opts)
    t.run()
    return t


def same_rows(a, b):
    assert len(a) == len(b)
    for x, y in zip(a, b):
        assert x[0] == y[0] and len(x) == len(y)
        assert all(p == q or (np.isnan(p) and np.isnan(q)) for p, q in zip(x[1:], y[1:])), (x, y)


def test_the_pack_carries_the_geometry(packs):
    plain = prepare.prepare_patient(*patient(3), spacing=SPACING, new_spacing=NEW_SPACING, normalize=True, crop_size=WINDOW)
    assert sorted(plain) == ["image", "label"]                                    # without the flag: today's dict
    p = packs[0]
    assert sorted(p) == ["geometry", "image", "label", "native_label"]
    assert torch.equal(p["image"], plain["image"]) and torch.equal(p["label"], plain["label"])
    geo = p["geometry"]
    assert geo == prepare.geometry(*SHAPE, spacing=SPACING, new_spacing=NEW_SPACING, crop_size=WINDOW)
    assert geo.native_hw == (40, 36) and geo.resampled_hw == (46, 41) and geo.window_hw == (32, 32) and geo.offset == (7, 4)
    assert p["native_label"].is_cuda and p["native_label"].dtype == torch.uint8 and np.array_equal(p["native_label"].cpu().numpy(), patient(3)[1])


@pytest.mark.parametrize("mode", R.MODES)
def test_native_grid_scores_the_restored_volume(solver, packs, mode):
    t = run(solver, packs, native_grid=True, restore_mode=mode)
    fresh = runningMySegmentationScore(n_classes=4, idx2cls_dict=_Packs.formalized_label_dict, metrics_list=METRICS)
    assert len(t.result_dict) == 2
    for i, (pid, res) in enumerate(t.result_dict.items()):
        geo = packs[i]["geometry"]
        assert sorted(res) == ["image", "label", "native_label", "native_pred", "pred", "soft_pred"]
        assert res["native_pred"].shape == SHAPE and res["native_pred"].dtype == np.uint8
        assert res["pred"].shape == (6, 32, 32) and res["soft_pred"].shape == (6, 4, 32, 32) and res["image"].shape == (6, 32, 32)
        assert np.array_equal(res["native_label"], patient(3 + i)[1]) and np.array_equal(res["label"], packs[i]["label"].cpu().numpy())
        assert np.array_equal(res["pred"], res["soft_pred"].argmax(axis=1))         # the window keys keep their meaning
        v, inside = prepare.restore_values_host(res["soft_pred"], geo, mode=mode)
        want = prepare.restore_scores_host(res["soft_pred"], geo, mode=mode)
        decided = R.decided(v, inside)
        under = int((~decided).sum())
        print("  %s %s: %d of %d voxels under the near-tie bound, %d outside" % (pid, mode, under, decided.size, int((~inside).sum()) * 6))
        assert under <= 0.01 * decided.size
        assert np.array_equal(res["native_pred"][decided], want[decided])
        assert len(np.unique(res["native_pred"])) > 1
        fresh.update(pid=pid, preds=res["native_pred"], gts=res["native_label"], voxel_spacing=[10.0, 1.5625, 1.5625])
    same_rows(t.segmentation_metric.tables, fresh.tables)
    lean = run(solver, packs, native_grid=True, restore_mode=mode, keep_results=False)       # no kept result: no window arg-max either
    assert lean.result_dict == {}
    same_rows(lean.segmentation_metric.tables, fresh.tables)


def test_post_process_acts_on_the_native_volume(solver, packs):
    raw = run(solver, packs, native_grid=True)
    cc = run(solver, packs, native_grid=True, post_process="largest_cc")
    fresh = runningMySegmentationScore(n_classes=4, idx2cls_dict=_Packs.formalized_label_dict, metrics_list=METRICS)
    changed = 0
    for pid, res in cc.result_dict.items():
        before = torch.from_numpy(raw.result_dict[pid]["native_pred"]).cuda()
        want = ops.keep_largest_components(before, 4, per_slice=False).cpu().numpy()
        assert np.array_equal(res["native_pred"], want)
        window = ops.keep_largest_components(torch.from_numpy(raw.result_dict[pid]["pred"]).cuda(), 4, per_slice=False).cpu().numpy()
        assert np.array_equal(res["pred"], window)
        changed += int((want != raw.result_dict[pid]["native_pred"]).sum())
        fresh.update(pid=pid, preds=res["native_pred"], gts=res["native_label"], voxel_spacing=[10.0, 1.5625, 1.5625])
    print("  largest_cc changed %d native voxels" % changed)
    assert changed > 0
    same_rows(cc.segmentation_metric.tables, fresh.tables)


def test_without_native_grid_nothing_changes(solver, packs):
    plain_packs = [{k: p[k] for k in ("image", "label")} for p in packs]
    from cooperative_training_and_latent_space_data_augmentation_amd import _ffi
    before = _ffi.lib.ctl_launch_count()
    old = run(solver, plain_packs)
    mid = _ffi.lib.ctl_launch_count()
    new = run(solver, packs, native_grid=False, restore_mode="logit")
    after = _ffi.lib.ctl_launch_count()
    assert after - mid == mid - before                                             # the same launches
    same_rows(new.segmentation_metric.tables, old.segmentation_metric.tables)
    for pid, res in old.result_dict.items():
        assert sorted(new.result_dict[pid]) == sorted(res) == ["image", "label", "pred", "soft_pred"]
        for key in res:
            assert np.array_equal(new.result_dict[pid][key], res[key]), (pid, key)


def test_refusals(solver, packs):
    from cooperative_training_and_latent_space_data_augmentation_amd.tester import TestSegmentationNetwork
    for drop in ("geometry", "native_label"):
        broken = [{k: v for k, v in p.items() if k != drop} for p in packs]
        with pytest.raises(ValueError, match="geometry"):
            run(solver, broken, native_grid=True)
    with pytest.raises(ValueError, match="restore_mode"):
        TestSegmentationNetwork(_Packs(packs), crop_size=None, segmentation_model=solver, native_grid=True, restore_mode="softmax")
