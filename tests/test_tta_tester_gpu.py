"""Test-time augmentation in the patient-wise tester (tester.TestSegmentationNetwork(tta=, tta_mode=), tester.predict_volume(tta=)):
tta=None is today's tester; the identity view in "logit" mode changes no bit; a W-flipped volume under (0, 4) gives the W-flipped result;
"d4" in "prob" mode against the per-view composition written with torch.flip / transpose and a float64 softmax mean, within the bounds
tests/test_uncertainty_gpu.py derives (PB on the mean probability, cal_bounds of tests/test_uncertainty_metrics_gpu.py on the columns);
chunks concatenate; native_grid restores the merged scores; uncertainty_maps returns the mutual information."""
import numpy as np
import pytest
import torch

from cooperative_training_and_latent_space_data_augmentation_amd import ops, prepare, tta, uncertainty as U
from cooperative_training_and_latent_space_data_augmentation_amd.tester import TestSegmentationNetwork, predict_volume

from test_uncertainty_gpu import HB, MB, PB
from test_uncertainty_metrics_gpu import CAL, NAMES, _Patients, cal_bounds

pytestmark = pytest.mark.gpu
F32 = np.float32


@pytest.fixture(scope="module")
def solver():
    from cooperative_training_and_latent_space_data_augmentation_amd.solver import AdvancedTripletReconSegmentationModel
    torch.manual_seed(0)
    s = AdvancedTripletReconSegmentationModel(network_type="FCN_16_standard", image_ch=1, num_classes=4, use_gpu=True)
    s.eval()
    return s


class _Flipped(_Patients):
    """the same patients, image and label flipped along W"""

    def get_patient_data_for_testing(self, i, crop_size=None):
        pack = super().get_patient_data_for_testing(i, crop_size)
        return {k: torch.flip(v, dims=(-1,)).contiguous() for k, v in pack.items()}


class _Oblong(_Patients):
    def __init__(self):
        super().__init__(n=1, shape=(6, 32, 48))


def run(solver, dataset, metrics=("Dice",) + CAL, **opts):
    t = TestSegmentationNetwork(dataset, crop_size=None, segmentation_model=solver, metrics_list=metrics, **opts)
    t.run()
    return t


def same_results(a, b, keys=("image", "label", "pred", "soft_pred")):
    assert list(a.result_dict) == list(b.result_dict)
    for pid in a.result_dict:
        assert sorted(a.result_dict[pid]) == sorted(b.result_dict[pid])
        for k in keys:
            x, y = a.result_dict[pid][k], b.result_dict[pid][k]
            assert x.dtype == y.dtype and np.array_equal(x.view(np.int32) if x.dtype == F32 else x, y.view(np.int32) if y.dtype == F32 else y), (pid, k)


def view_torch(x, v):
    a = x.transpose(-1, -2) if v & 1 else x
    a = torch.flip(a, dims=(-2,)) if v & 2 else a
    return torch.flip(a, dims=(-1,)) if v & 4 else a


def unview_torch(y, v):
    a = torch.flip(y, dims=(-1,)) if v & 4 else y
    a = torch.flip(a, dims=(-2,)) if v & 2 else a
    return a.transpose(-1, -2) if v & 1 else a


def test_tta_none_is_todays_tester(solver):
    plain = run(solver, _Patients())
    none = run(solver, _Patients(), tta=None, tta_mode="prob")
    assert plain.segmentation_metric.tables == none.segmentation_metric.tables
    same_results(plain, none)
    image = _Patients().get_patient_data_for_testing(0)["image"].cuda()
    assert torch.equal(predict_volume(solver, image), predict_volume(solver, image, tta=None))
    assert np.array_equal(predict_volume(solver, image).cpu().numpy(), plain.result_dict["patient000"]["pred"])


def test_the_identity_view_in_logit_mode_changes_no_bit(solver):
    plain = run(solver, _Patients())
    ident = run(solver, _Patients(), tta=(0,), tta_mode="logit")
    assert plain.segmentation_metric.tables == ident.segmentation_metric.tables          # the calibration columns included
    same_results(plain, ident)
    image = _Patients().get_patient_data_for_testing(1)["image"].cuda()
    assert torch.equal(predict_volume(solver, image), predict_volume(solver, image, tta=(0,), tta_mode="logit"))


def test_a_flipped_volume_gives_the_flipped_result(solver):
    """(0, 4) in "logit" mode: on the W-flipped volume the two members swap, and a two-term fp32 sum commutes"""
    a = run(solver, _Patients(), metrics=("Dice", "VolError"), tta=(0, 4), tta_mode="logit")
    b = run(solver, _Flipped(), metrics=("Dice", "VolError"), tta=(0, 4), tta_mode="logit")
    assert a.segmentation_metric.tables == b.segmentation_metric.tables
    for pid in a.result_dict:
        for k in ("image", "label", "pred", "soft_pred"):
            x, y = a.result_dict[pid][k], np.flip(b.result_dict[pid][k], axis=-1)
            assert np.array_equal(x.view(np.int32) if x.dtype == F32 else x, y.view(np.int32) if y.dtype == F32 else y), (pid, k)
    plain = run(solver, _Patients(), metrics=("Dice", "VolError"))
    assert any(not np.array_equal(a.result_dict[p]["soft_pred"], plain.result_dict[p]["soft_pred"]) for p in a.result_dict)      # TTA did something


def test_d4_prob_against_the_per_view_composition(solver):
    t = run(solver, _Patients(), tta="d4", tta_mode="prob", uncertainty_maps=True)
    T, c = 8, 4
    for i, (pid, res) in enumerate(t.result_dict.items()):
        assert sorted(res) == ["conf", "entropy", "image", "label", "mi", "pred", "soft_pred"]
        pack = _Patients().get_patient_data_for_testing(i)
        image, label = pack["image"].cuda(), pack["label"]
        members = [unview_torch(solver.predict(view_torch(image, v).contiguous(), softmax=False), v) for v in range(T)]
        stack = torch.cat([m.float() for m in members], dim=0).cpu()
        want = torch.softmax(stack.double().view(T, 6, c, 32, 32), dim=2).mean(dim=0).numpy()
        err = np.abs(res["soft_pred"].astype(np.float64) - want).max()
        top2 = np.sort(want, axis=1)[:, -2:]
        tie = (top2[:, 1] - top2[:, 0]) < 2 * PB(c, T)
        print(f"  {pid}: soft_pred max |diff| {err:.3e} bound {PB(c, T):.3e}; {int(tie.sum())} of {tie.size} pixels within 2 PB of a tie")
        assert err <= PB(c, T) and tie.sum() <= 0.005 * tie.size
        assert np.array_equal(res["pred"][~tie], want.argmax(axis=1)[~tie])
        # the one T * n pass gives the members the per-view passes give (batching is bitwise neutral), so the stack is the ensemble's
        assert torch.equal(U.tta_members(solver, image, "d4").cpu(), stack)
        ref = U.predictive_stats_host(stack.double().numpy(), label.numpy(), members=T)
        host = U.calibration_from_tables(ref.stats, ref.bins, pixels=label.numel())
        bounds = cal_bounds(stack, label, T)
        row = t.segmentation_metric.tables[i]
        for k, got in zip(CAL, row[-4:]):
            print(f"  {pid} {k}: {got:.9f} (host {host[k]:.9f}, |diff| {abs(got - host[k]):.3e}, bound {bounds[k]:.3e})")
            assert np.isfinite(got) and abs(got - host[k]) <= bounds[k], (pid, k, got, host[k], bounds[k])
        assert np.abs(res["entropy"] - ref.entropy).max() <= HB(c, T) and np.abs(res["conf"] - ref.conf).max() <= PB(c, T)
        assert np.abs(res["mi"] - ref.mi).max() <= MB(c, T) and res["mi"].max() > 0 and res["mi"].shape == (6, 32, 32)


def test_chunked_and_whole_volume_runs_give_identical_rows(solver):
    whole = run(solver, _Patients(), tta="flips", keep_results=False)
    assert whole.result_dict == {}
    loop = TestSegmentationNetwork(_Patients(), crop_size=None, segmentation_model=solver, metrics_list=("Dice",) + CAL, keep_results=False, tta="flips")
    ds = loop.test_dataset
    for i in range(2):
        pid, result = loop.evaluate(i, ds.get_patient_data_for_testing(i), 2, maximum_batch_size=2, coalesce=False)
        assert result is None
    assert loop.segmentation_metric.tables == whole.segmentation_metric.tables
    image = _Patients().get_patient_data_for_testing(0)["image"].cuda()
    assert torch.equal(predict_volume(solver, image, tta="flips"), predict_volume(solver, image, chunk=2, coalesce=False, tta="flips"))
    assert torch.equal(predict_volume(solver, image, tta="flips"), tta.predict_tta(solver, image, "flips", want="pred").pred)


def test_uncertainty_maps_return_the_mutual_information(solver):
    maps = run(solver, _Patients(), keep_results=False, uncertainty_maps=True, tta=(0, 4))
    for pid, res in maps.result_dict.items():
        assert sorted(res) == ["conf", "entropy", "mi"] and res["mi"].shape == (6, 32, 32) and res["mi"].dtype == F32
        assert res["mi"].max() > 0 and res["mi"].min() >= -MB(4, 2)
    plain = run(solver, _Patients(), keep_results=False, uncertainty_maps=True)
    assert all(sorted(res) == ["conf", "entropy"] for res in plain.result_dict.values())      # without tta: today's keys


# ---------------------------------------------------------------------------------------------- native grid
SHAPE, NATIVE_SPACING, NEW_SPACING, WINDOW = (6, 40, 36), (1.5625, 1.5625, 10.0), [1.36719, 1.36719, -1], [32, 32]


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
    formalized_label_dict = NAMES

    def __init__(self, packs):
        self.packs, self.patient_number, self._cur = packs, len(packs), None

    def get_patient_data_for_testing(self, i, crop_size=None):
        self._cur = i
        return self.packs[i]

    def get_id(self):
        return "patient%03d" % self._cur

    def get_voxel_spacing(self):
        return [10.0, 1.5625, 1.5625]


@pytest.mark.parametrize("mode", ["prob", "logit"])
def test_native_grid_restores_the_merged_scores(solver, mode):
    packs = [prepare.prepare_patient(*patient(3), spacing=NATIVE_SPACING, new_spacing=NEW_SPACING, normalize=True, crop_size=WINDOW,
                                     want_geometry=True)]
    t = run(solver, _Packs(packs), metrics=("Dice", "VolError"), native_grid=True, tta="flips", tta_mode=mode)
    res = t.result_dict["patient000"]
    merged = tta.predict_tta(solver, packs[0]["image"].cuda().float(), "flips", mode=mode, want=("merged", "pred"))
    assert np.array_equal(res["soft_pred"].view(np.int32), merged.merged.cpu().numpy().view(np.int32))
    assert np.array_equal(res["pred"], merged.pred.cpu().numpy())
    by_hand = ops.restore_scores(torch.from_numpy(res["soft_pred"]).cuda(), packs[0]["geometry"], mode="logit")
    assert res["native_pred"].shape == SHAPE and np.array_equal(res["native_pred"], by_hand.cpu().numpy())
    assert len(np.unique(res["native_pred"])) > 1
    if mode == "prob":
        assert np.abs(res["soft_pred"].sum(axis=1) - 1.0).max() <= 4 * PB(4, 4)      # probabilities, not logits
    with pytest.raises(ValueError, match="native_grid"):                          # the existing refusal stands with tta
        TestSegmentationNetwork(_Packs(packs), crop_size=None, segmentation_model=solver, metrics_list=("Dice", "ECE"), native_grid=True, tta="flips")
    with pytest.raises(ValueError, match="native_grid"):
        TestSegmentationNetwork(_Packs(packs), crop_size=None, segmentation_model=solver, native_grid=True, tta="flips", uncertainty_maps=True)


# ---------------------------------------------------------------------------------------------- refusals
def test_refusals(solver):
    with pytest.raises(ValueError, match="duplicate view code 4"):
        TestSegmentationNetwork(_Patients(), crop_size=None, segmentation_model=solver, tta=(0, 4, 4))
    with pytest.raises(ValueError, match="unknown view set"):
        TestSegmentationNetwork(_Patients(), crop_size=None, segmentation_model=solver, tta="rot90")
    with pytest.raises(ValueError, match="tta_mode"):
        TestSegmentationNetwork(_Patients(), crop_size=None, segmentation_model=solver, tta="flips", tta_mode="mean")
    with pytest.raises(ValueError, match="view code 1 transposes"):
        run(solver, _Oblong(), metrics=("Dice",), tta="d4")
    oblong = _Oblong().get_patient_data_for_testing(0)["image"].cuda()
    with pytest.raises(ValueError, match="view code 3 transposes"):
        predict_volume(solver, oblong, tta=(0, 3))
    with pytest.raises(ValueError, match="duplicate"):
        predict_volume(solver, oblong, tta=(2, 2))
    flips = run(solver, _Oblong(), metrics=("Dice",), tta="flips")                   # non-transposing views work on any window
    assert flips.result_dict["patient000"]["pred"].shape == (6, 32, 48)
    assert np.array_equal(flips.result_dict["patient000"]["pred"], predict_volume(solver, oblong, tta="flips").cpu().numpy())
