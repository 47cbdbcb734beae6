"""`trainer.train_network` from a DeviceBatchLoader on the GPU: two epochs of four steps on three small synthetic volumes.  Losses are
finite, the best checkpoint exists and loads into a fresh solver, a second run from the same seeds ends with identical weights, and a
loop driven by hand over the same loader and solver calls (train_adv_supervised_segmentation_triplet.py:171-237, 63-78) gives the same
weights bit for bit."""
import glob
import math
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from cooperative_training_and_latent_space_data_augmentation_amd import basic_operations, loader as L, trainer  # noqa: E402
from cooperative_training_and_latent_space_data_augmentation_amd.augment import BatchAugmenter  # noqa: E402
from cooperative_training_and_latent_space_data_augmentation_amd.solver import AdvancedTripletReconSegmentationModel  # noqa: E402

PAD, CROP, BATCH = (80, 80), (64, 64), 4
IMG_CFG = {"loss_name": "mse", "mask_type": "channel", "max_threshold": 0.5, "random_threshold": False, "if_soft": False}
SEG_CFG = {"loss_name": "ce", "mask_type": "spatial", "max_threshold": 0.5, "random_threshold": False, "if_soft": False}
OPT = {"learning": {"n_epochs": 2, "max_iteration": 1000, "latent_DA": True, "separate_training": False, "batch_size": BATCH},
       "latent_DA": {"mask_scope": ["image code", "shape code"], "image code": IMG_CFG, "shape code": SEG_CFG},
       "data": {"keep_orig_image_label_pair_for_training": True},
       "output": {"save_epoch_every_num_epochs": 2}, "segmentation_model": {"network_type": "FCN_16_standard"}}


def blob_volume(s, h, w, seed):
    """smooth image in [0, 1] with three nested blobs labelled 1..3"""
    rng = np.random.default_rng(seed)
    yy, xx = np.meshgrid(np.arange(h), np.arange(w), indexing="ij")
    image, label = np.zeros((s, h, w), dtype=np.float32), np.zeros((s, h, w), dtype=np.uint8)
    for i in range(s):
        cy, cx = h / 2 + rng.uniform(-4, 4), w / 2 + rng.uniform(-4, 4)
        r = np.sqrt((yy - cy) ** 2 + (xx - cx) ** 2)
        for k, radius in ((1, 18.0), (2, 12.0), (3, 6.0)):
            label[i][r < radius + rng.uniform(-1, 1)] = k
        image[i] = (0.2 + 0.2 * label[i] + 0.1 * np.sin(yy / 7.0) * np.cos(xx / 9.0)).astype(np.float32)
    return image, label


def loaders():
    train = L.DeviceSliceSet([blob_volume(3, 70, 60, 1), blob_volume(2, 64, 64, 2), blob_volume(3, 58, 72, 3)], PAD, CROP, seed=0, device="cuda")
    val = L.DeviceSliceSet([blob_volume(3, 66, 62, 4)], PAD, CROP, seed=0, device="cuda")
    g, gv = torch.Generator(), torch.Generator()
    g.manual_seed(21)
    gv.manual_seed(22)
    train_loader = L.DeviceBatchLoader(train, BATCH, augmenter=BatchAugmenter("ACDC_affine_elastic_intensity", CROP, seed=5), keep_orig=True,
                                       generator=g)
    val_loader = L.DeviceBatchLoader(val, BATCH, keep_orig=False, shuffle=False, generator=gv)
    assert len(train) == 8 and train_loader.train_batch_size == 2 and len(train_loader) == 4 and len(val_loader) == 1
    return train_loader, val_loader


def solver(golden_sd):
    torch.manual_seed(17)
    s = AdvancedTripletReconSegmentationModel(use_gpu=True)
    for k, m in s.model.items():
        m.load_state_dict(golden_sd[k])
    return s


def weights(s):
    torch.cuda.synchronize()
    return {f"{k}/{n}": v.detach().cpu().clone() for k, m in s.model.items() for n, v in m.state_dict().items()}


def same(a, b):
    assert a.keys() == b.keys()
    for k in a:
        assert torch.equal(a[k], b[k]), k


def hand_driven(s, train_loader, val_loader):
    """the loop of train_network written out over the loader and the solver's stock calls"""
    s.reset_all_optimizers()
    s.train()
    scores = []
    for _ in range(OPT["learning"]["n_epochs"]):
        for _ in range(len(train_loader)):
            s.train()
            s.reset_all_optimizers()
            clean, label = train_loader.next_batch()
            noisy = basic_operations.add_input_noise(clean, sigma=0.05, seed=int(torch.randint(0, 2 ** 62, (1,)).item()))
            std = s.standard_training(clean, label, perturbed_image=noisy, separate_training=False)
            standard_loss = std[0] + std[1] + std[3] + std[2]
            s.reset_all_optimizers()
            xh, yh = s.hard_example_generation(clean.detach().clone(), label.detach().clone(), gen_corrupted_seg=True, gen_corrupted_image=True,
                                               corrupted_image_DA_config=IMG_CFG, corrupted_seg_DA_config=SEG_CFG)
            hard = s.hard_example_training(perturbed_image=xh, perturbed_seg=yh, clean_image_l=clean, label_l=label, separate_training=False)
            loss = standard_loss + (hard[0] + hard[1] + hard[2] + hard[3])
            s.reset_all_optimizers()
            loss.backward()
            s.optimize_all_params()
        s.eval()
        s.running_metric.reset()
        for _ in range(len(val_loader)):
            image, target = val_loader.next_batch()
            s.evaluate(input=image, targets_npy=target, n_iter=2)
        scores.append(s.running_metric.get_scores()[0]['Mean IoU : \t'])
    return scores


def test_train_network_from_the_device_loader(golden_sd, tmp_path):
    runs = []
    for name in ("a", "b"):
        s = solver(golden_sd)
        networks = list(s.model)
        rec = trainer.train_network(s, *loaders(), OPT, str(tmp_path / name), verbose=False)
        runs.append((rec, weights(s)))
    rec, w_a = runs[0]
    assert rec["iterations"] == 8 and len(rec["losses"]) == 2 and len(rec["score_list"]) == 2
    for epoch in rec["losses"]:
        assert set(epoch) == set(trainer.LOSS_KEYS) | {"loss/total"} and all(math.isfinite(v) for v in epoch.values()), epoch
        assert abs(epoch["loss/total"] - epoch["loss/standard/total"] - epoch["loss/hard/total"]) < 1e-4 * max(1.0, abs(epoch["loss/total"]))
    assert all(math.isfinite(v) and 0.0 <= v <= 1.0 for v in rec["score_list"]) and rec["best_score"] == max(rec["score_list"])
    same(w_a, runs[1][1])                                                   # the same seeds: the same weights
    assert rec["losses"] == runs[1][0]["losses"] and rec["score_list"] == runs[1][0]["score_list"]
    # checkpoints: best, epoch 0 and the periodic save of epoch 1; 'best' loads into a fresh solver
    best = str(tmp_path / "a" / "best" / "checkpoints")
    files = sorted(os.path.basename(p) for p in glob.glob(os.path.join(best, "*.pth")))
    assert files == sorted(f"{k}.pth" for k in networks)
    for epoch in ("0", "1"):
        assert len(glob.glob(str(tmp_path / "a" / epoch / "checkpoints" / "*.pth"))) == len(files)
    fresh = AdvancedTripletReconSegmentationModel(use_gpu=True, checkpoint_dir=best)
    w_best = weights(fresh)
    if rec["score_list"][1] > rec["score_list"][0]:
        same(w_best, w_a)                                                   # the last epoch was the best one: its weights
    last = AdvancedTripletReconSegmentationModel(use_gpu=True, checkpoint_dir=str(tmp_path / "a" / "1" / "checkpoints"))
    same(weights(last), w_a)
    # the loop written out by hand over the same loader and solver calls
    s = solver(golden_sd)
    scores = hand_driven(s, *loaders())
    same(weights(s), w_a)
    assert scores == rec["score_list"]


def test_cooperative_flag_and_iteration_cap(golden_sd, tmp_path):
    s = solver(golden_sd)
    opt = dict(OPT, learning=dict(OPT["learning"], n_epochs=3, max_iteration=2))
    rec = trainer.train_network(s, *loaders(), opt, str(tmp_path / "c"), cooperative=True, verbose=False)
    assert rec["iterations"] == 3 and len(rec["losses"]) == 1                # upstream's counter: the flag is raised after step max_iteration + 1
    assert all(math.isfinite(v) for v in rec["losses"][0].values())
    assert len(glob.glob(str(tmp_path / "c" / "best" / "checkpoints" / "*.pth"))) == len(s.model)
