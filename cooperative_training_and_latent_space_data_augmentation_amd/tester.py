"""Patient-wise evaluation harness: volume in -> per-class Dice out.

Mirror of `TestSegmentationNetwork` (medseg/test_basic_segmentation_solver.py:29-172) for the part that sits on the accelerated
path: the volume is uploaded once, predicted in chunks of <= `maximum_batch_size` slices (`predict`, model.py:375-394), the arg-max
and the per-patient voxel counts are taken on the device, and one 2*n^2-word readback per patient replaces the reference's two
full-volume `.cpu().numpy()` copies per chunk.  The dataset only has to offer what the reference's tester reads from it:
`patient_number`, `get_patient_data_for_testing(i, crop_size=)` -> {'image': [n,1,H,W], 'label': [n,H,W]}, `get_id()`,
`get_voxel_spacing()` and `formalized_label_dict`.  The tensors of a pack may live on the host (uploaded once here) or already on the
device (prepare.prepare_patient: no upload at all).  Writing nrrd files (SimpleITK) is outside the path and not offered.
With native_grid=True (a project addition, off by default) the logits are put back on the patient's native grid on the device
(ops.restore_scores) and post-processing and the metrics run there; the packs then carry 'geometry' and 'native_label'
(prepare.prepare_patient(want_geometry=True)).
With 'ECE' / 'NLL' / 'Brier' / 'Entropy' in metrics_list (project additions, metrics.runningMySegmentationScore) every chunk's logits go through
ops.predictive_stats while they are on the device and only its small per-slice tables are kept; uncertainty_maps=True adds the 'entropy' and
'conf' maps of the volume to the patient's result.
With tta="flips" / "d4" / a tuple of view codes (a project addition, off by default: tta.py) every chunk is predicted as T flipped / rotated
views in one pass and the members are merged on the device (ops.tta_views, ops.tta_merge: two more launches per chunk); the merged scores
take the place of the logits everywhere and the calibration columns become those of the T-member ensemble."""
import os

import numpy as np
import torch

from . import ops, tta as tta_mod
from .metrics import runningMySegmentationScore


PASS_FLOATS_PER_PIXEL = 512      # generous bound of what one slice of a `predict` pass keeps on the device, in floats per input pixel (FTN + STN
                                 # encoder / decoder workspaces: a bs16 256^2 decoder pass holds 289 MB = 69 floats per pixel and slice)


def max_slices_per_pass(h: int, w: int, widest_channels: int = 16, device=None) -> int:
    """The kernels address a tensor with 32-bit byte offsets (< 2 GiB, include/ctl_hip.h); the widest tensor of a pass is the
    full-resolution 16-channel fp32 feature map: 64 bytes per pixel.  With `device` the pass is also bounded by HALF of the device memory
    that is free right now (`maximum_batch_size` exists upstream to bound GPU memory: a coalesced pass must not defeat that -- ADVICE r4)."""
    limit = max(1, (2 ** 31 - 1) // (h * w * widest_channels * 4))
    if device is not None:
        free, _ = torch.cuda.mem_get_info(device)
        limit = max(1, min(limit, int(free // 2) // (h * w * 4 * PASS_FLOATS_PER_PIXEL)))
    return limit


COALESCE_CHUNKS = True      # run consecutive <= `maximum_batch_size`-slice chunks of a volume as one pass (see predict_volume)


def predict_volume(segmentation_model, image_d: torch.Tensor, n_iter=None, chunk=None, out: torch.Tensor = None, coalesce=None, tta=None,
                   tta_mode="prob") -> torch.Tensor:
    """uint8 label volume [n,H,W] of a device volume [n,1,H,W]: `predict` (model.py:375-394) + arg-max on the device.
    chunk = 10 is the reference's loop (test_basic_segmentation_solver.py:85-114): a GPU-MEMORY workaround, not part of the computation --
    `predict` puts every network in eval mode (running BatchNorm statistics), so slices are independent and batching changes nothing but
    the number of launches (bitwise equal logits and labels, tests/test_engine_gpu.py::test_whole_volume_pass_is_bitwise_the_chunked_loop).
    With `coalesce` (default: tester.COALESCE_CHUNKS = True) consecutive chunks therefore run as ONE pass, as many as the 2 GiB
    addressing limit of a tensor AND half of the currently free device memory allow (max_slices_per_pass); coalesce=False is the
    reference's literal loop.  chunk = None:
    the whole volume per pass either way.
    tta (None: today's path, no extra launch): a view set of tta.parse_views; a chunk then holds limit // T slices, so that the T * n pass
    respects max_slices_per_pass, and the labels are the arg-max of the merged scores (tta.predict_tta, mode `tta_mode`)."""
    n, _, h, w = image_d.shape
    limit = max_slices_per_pass(h, w, device=image_d.device)
    codes = None if tta is None else tta_mod.parse_views(tta, (h, w))
    if codes is not None:
        limit = max(1, limit // len(codes))
    coalesce = COALESCE_CHUNKS if coalesce is None else bool(coalesce)
    if chunk is not None and int(chunk) < 1:
        raise ValueError("chunk must be positive")
    chunk = limit if (chunk is None or coalesce) else min(int(chunk), limit)
    pred = out if out is not None else torch.empty((n, h, w), dtype=torch.uint8, device=image_d.device)
    for lo in range(0, n, chunk):
        hi = min(n, lo + chunk)
        if codes is None:
            pred[lo:hi] = ops.argmax_c(segmentation_model.predict(input=image_d[lo:hi], softmax=False, n_iter=n_iter))
        else:
            pred[lo:hi] = tta_mod.predict_tta(segmentation_model, image_d[lo:hi], codes, mode=tta_mode, n_iter=n_iter, want=("pred",)).pred
    return pred


# `post_process` of TestSegmentationNetwork -> per_slice of ops.keep_largest_components (None: the prediction is scored as it is)
POST_PROCESS = {None: None, "largest_cc": False, "largest_cc_2d": True}


class TestSegmentationNetwork(object):
    __test__ = False                     # not a pytest class

    def __init__(self, test_dataset, crop_size, segmentation_model, use_gpu=True, save_path="", summary_report_file_name="result.csv",
                 detailed_report_file_name="details.csv", patient_wise=True, metrics_list=("Dice", "HD"), foreground_only=False,
                 save_soft_prediction=False, keep_results=True, post_process=None, native_grid=False, restore_mode="logit",
                 uncertainty_maps=False, tta=None, tta_mode="prob"):
        if not use_gpu:
            raise ValueError("this build has no CPU path")
        if post_process not in POST_PROCESS:
            raise ValueError("post_process {!r}: one of {}".format(post_process, sorted(POST_PROCESS, key=str)))
        if restore_mode not in ops.RESTORE_MODES:
            raise ValueError("restore_mode {!r}: one of {}".format(restore_mode, sorted(ops.RESTORE_MODES)))
        self.post_process, self.native_grid, self.restore_mode = post_process, bool(native_grid), restore_mode
        self.tta = None if tta is None else tta_mod.parse_views(tta)      # (duplicate or unknown codes: ValueError here)
        if tta_mode not in ops.TTA_MODES:
            raise ValueError("tta_mode {!r}: one of {}".format(tta_mode, sorted(ops.TTA_MODES)))
        self.tta_mode = tta_mode
        self.calibration = any(m in runningMySegmentationScore.PATIENT_LEVEL for m in metrics_list)
        self.uncertainty_maps = bool(uncertainty_maps)
        if self.native_grid and (self.calibration or self.uncertainty_maps):
            raise ValueError("native_grid=True with {} or uncertainty_maps: the logits live on the window grid, calibration on the native grid "
                             "is not offered".format(list(runningMySegmentationScore.PATIENT_LEVEL)))
        self.test_dataset, self.crop_size, self.segmentation_model = test_dataset, crop_size, segmentation_model
        self.num_classes = segmentation_model.num_classes
        self.segmentation_metric = runningMySegmentationScore(n_classes=self.num_classes,
                                                              idx2cls_dict=getattr(test_dataset, "formalized_label_dict", None),
                                                              metrics_list=metrics_list, foreground_only=foreground_only)
        self.save_path, self.patient_wise = save_path, patient_wise
        self.summary_report_file_name, self.detailed_report_file_name = summary_report_file_name, detailed_report_file_name
        self.save_soft_prediction, self.keep_results = save_soft_prediction, keep_results
        if save_path and not os.path.exists(save_path):
            os.makedirs(save_path)
        self.df, self.result_dict = None, {}

    def run(self):
        n = self.test_dataset.patient_number if self.patient_wise else len(self.test_dataset)
        for i in range(n):
            pack = self.test_dataset.get_patient_data_for_testing(i, crop_size=self.crop_size) if self.patient_wise else self.test_dataset[i]
            pid, result = self.evaluate(i, pack, n)
            if self.keep_results or self.uncertainty_maps:
                self.result_dict[pid] = result
        join = os.path.join
        self.segmentation_metric.get_scores(save_path=join(self.save_path, self.summary_report_file_name) if self.save_path else None)
        self.df = self.segmentation_metric.save_patient_wise_result_to_csv(
            save_path=join(self.save_path, self.detailed_report_file_name) if self.save_path else None)
        return self.df

    def evaluate(self, i, data_tensor_pack, total_number, maximum_batch_size=10, coalesce=None):
        """One patient: `predict` over the volume, device arg-max into one uint8 volume, metric update from the device tensors.
        maximum_batch_size = 10 is upstream's default argument (a GPU-memory workaround); the chunks it asks for are run as one pass
        (tester.COALESCE_CHUNKS, exact: see predict_volume; 2x the slices/s on a 40-slice volume); coalesce=False: the literal loop.
        The metric update reads back only small tables (voxel counts, and for 'HD' / 'ASD' the per-slice / per-class surface statistics
        of ops.surface_stats), so with keep_results=False and save_soft_prediction=False a patient is scored without any full-volume
        device-to-host copy.  That also holds with `post_process` ("largest_cc": the volume as one 3-D object, "largest_cc_2d": every slice
        on its own), which is applied on the device between the arg-max and the metric update; 'pred' of the result is then the
        post-processed volume.
        native_grid: the pack carries 'geometry' (prepare.Geometry) and 'native_label' [n,h,w]; every chunk's logits are restored into one
        native uint8 volume (ops.restore_scores, mode `restore_mode`: one more launch per chunk), `post_process` and the metric update
        take that volume and the native label, and get_voxel_spacing() is then the native spacing.  The four keys of the result keep
        their meaning (window grid); 'native_pred' and 'native_label' are added.
        Calibration columns: one ops.predictive_stats call per chunk on the logits `predict` just returned (2 launches); the per-slice
        tables join the metric's one readback, no logits are kept for it.  uncertainty_maps: the same call also writes the chunk's
        'entropy' and 'conf' maps, which are added to the result (the only keys when nothing else is kept).
        tta (TestSegmentationNetwork(tta=, tta_mode=)): a chunk holds limit // T slices and is predicted as its T views in one pass
        (tta.predict_tta).  The merged scores take the place of the logits for the arg-max, for restore_scores and for 'soft_pred': with
        tta_mode="prob" (the default) 'soft_pred' holds the mean PROBABILITIES of the members, not logits, and
        restore_scores(mode="logit") is then the bilinear interpolation of those probabilities; with "logit" it holds the mean logits.
        The calibration columns and uncertainty_maps read the members put back on the native grid (predictive_stats(members=T)) and
        are those of the ensemble's mean probability in either mode; uncertainty_maps then also returns 'mi', the mutual information.
        native_grid works with tta as long as no calibration column is asked for (the refusal above stands)."""
        dev = torch.device("cuda", torch.cuda.current_device())
        image = data_tensor_pack["image"]
        if image.dim() == 5:                              # DataLoader(batch_size=1) adds a leading axis upstream
            image = image[0]
        limit = max_slices_per_pass(image.shape[-2], image.shape[-1], device=dev)
        codes = None if self.tta is None else tta_mod.parse_views(self.tta, image.shape[-2:])      # a transposing view: square windows only
        if codes is not None:
            limit = max(1, limit // len(codes))
        assert maximum_batch_size is None or int(maximum_batch_size) > 0
        if maximum_batch_size is None or (COALESCE_CHUNKS if coalesce is None else coalesce):
            maximum_batch_size = min(int(image.shape[0]), limit)
        else:
            maximum_batch_size = min(int(maximum_batch_size), limit)
        label = torch.as_tensor(data_tensor_pack["label"]).reshape(-1, image.shape[-2], image.shape[-1])
        assert image.size(1) == 1, "currently only support gray images, found: {}".format(image.size(1))
        image_d = image.to(dev, dtype=torch.float32, non_blocking=True)
        label_d = label.to(dev, dtype=torch.int64, non_blocking=True)
        pid = self.test_dataset.get_id()
        total = image_d.size(0)
        geo = native_d = native_label_d = None
        if self.native_grid:
            if "geometry" not in data_tensor_pack or "native_label" not in data_tensor_pack:
                raise ValueError("native_grid=True needs a pack with 'geometry' and 'native_label' (prepare.prepare_patient(want_geometry=True))")
            geo = data_tensor_pack["geometry"]
            native_label_d = torch.as_tensor(data_tensor_pack["native_label"]).reshape(-1, *geo.native_hw).to(dev, dtype=torch.int64, non_blocking=True)
            if native_label_d.size(0) != total:
                raise ValueError("native_grid=True: 'native_label' has {} slices, the image {}".format(native_label_d.size(0), total))
            native_d = torch.empty((total,) + tuple(geo.native_hw), dtype=torch.uint8, device=dev)
        pred_d = torch.empty((total, image_d.shape[-2], image_d.shape[-1]), dtype=torch.uint8, device=dev)
        soft = [] if (self.save_soft_prediction or self.keep_results) else None
        uncert = [] if (self.calibration or self.uncertainty_maps) else None
        want_pred = native_d is None or soft is not None          # native grid: the window arg-max is only a kept result
        for lo in range(0, total, maximum_batch_size):
            hi = min(total, lo + maximum_batch_size)
            if codes is None:
                logit = members = self.segmentation_model.predict(input=image_d[lo:hi], softmax=False)
                if want_pred:
                    pred_d[lo:hi] = ops.argmax_c(logit)
            else:                                                 # `logit`: the merged scores; `members`: the T aligned members
                want = (("merged",) if (native_d is not None or soft is not None) else ()) + (("pred",) if want_pred else ()) + \
                       (("aligned",) if uncert is not None else ())
                merge = tta_mod.predict_tta(self.segmentation_model, image_d[lo:hi], codes, mode=self.tta_mode, want=want)
                logit, members = merge.merged, merge.aligned
                if want_pred:
                    pred_d[lo:hi] = merge.pred
            if native_d is not None:
                ops.restore_scores(logit, geo, mode=self.restore_mode, out=native_d[lo:hi])
            if soft is not None:
                soft.append(logit)
            if uncert is not None:
                maps = ("entropy", "conf") + (("mi",) if codes is not None else ())
                uncert.append(ops.predictive_stats(members, label_d[lo:hi], members=1 if codes is None else len(codes),
                                                   n_bins=self.segmentation_metric.calibration_bins,
                                                   want=maps if self.uncertainty_maps else ()))
        scored_d, scored_label_d = (pred_d, label_d) if native_d is None else (native_d, native_label_d)
        if self.post_process is not None:                 # largest component of every class (post_process.py:5-22), in place on the device
            per_slice = POST_PROCESS[self.post_process]
            ops.keep_largest_components(scored_d, self.num_classes, per_slice=per_slice, out=scored_d)
            if native_d is not None and soft is not None:
                ops.keep_largest_components(pred_d, self.num_classes, per_slice=per_slice, out=pred_d)
        spacing = self.test_dataset.get_voxel_spacing() if hasattr(self.test_dataset, "get_voxel_spacing") else None
        self.segmentation_metric.update(pid=pid, preds=scored_d, gts=scored_label_d, voxel_spacing=spacing,
                                        logits=uncert if self.calibration else None)
        result = None
        if soft is not None:
            soft_np = torch.cat(soft, 0).float().cpu().numpy()
            # a pack prepared on the device (prepare.prepare_patient) is copied back here, and only here: keep_results asks for host arrays
            result = {"image": image.cpu().numpy().reshape(-1, image.shape[-2], image.shape[-1]), "label": label.cpu().numpy(),
                      "pred": pred_d.cpu().numpy(), "soft_pred": soft_np}
            if native_d is not None:
                result["native_pred"], result["native_label"] = native_d.cpu().numpy(), native_label_d.cpu().numpy()
        if self.uncertainty_maps:
            result = {} if result is None else result
            result["entropy"] = torch.cat([u.entropy for u in uncert], 0).cpu().numpy()
            result["conf"] = torch.cat([u.conf for u in uncert], 0).cpu().numpy()
            if self.tta is not None:
                result["mi"] = torch.cat([u.mi for u in uncert], 0).cpu().numpy()
        if result is not None and total == 1:
            result = {k: v[0] for k, v in result.items()}
        if self.save_soft_prediction and self.save_path:
            out = os.path.join(self.save_path, "pred_npy")
            os.makedirs(out, exist_ok=True)
            tag = str(pid).replace("/", "_")
            for name, key in (("soft_pred", "soft_pred"), ("gt", "label"), ("image", "image")):
                np.save(os.path.join(out, "{}_{}.npy".format(tag, name)), result[key])
        return pid, result

    def get_top_k_results(self, topk=5, attribute="MYO_Dice", order=0):
        assert self.df is not None, "please run evaluation before saving"
        if order == 0:
            return self.df.nlargest(topk, attribute)
        if order == 1:
            return self.df.nsmallest(topk, attribute)
        raise ValueError(order)
