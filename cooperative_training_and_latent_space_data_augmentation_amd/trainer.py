"""`train_network` of medseg/train_adv_supervised_segmentation_triplet.py:63-78, 144-288 driven from `loader.DeviceBatchLoader`: volumes
plus config in, best checkpoint out, with no per-step host work on voxels.

Where the solver is concerned the loop is upstream's, statement for statement: `train()`, `reset_all_optimizers()`, the input noise
(:185-187, `basic_operations.add_input_noise`), `standard_training`, `hard_example_generation`, `hard_example_training`, the summed loss,
`backward`, `optimize_all_params`, then `eval_model` (`evaluate(..., n_iter=2)`, mean IoU for model selection), `save_model(..., 'best')`
and the periodic save.  `cooperative=True` runs the same iteration through `solver.cooperative_step` (the engine's fused form).

What differs: the epoch loss sums stay on the device and are read once per epoch (upstream reads ten `.item()`s per step); the
validation targets stay on the device; an exception saves the snapshot as upstream does and is then raised again, not swallowed.
Left out: tensorboard logging, `save_testing_images_results`, the command line and the config files."""
from __future__ import annotations

import gc

import torch

from . import basic_operations

LOSS_KEYS = ['loss/standard/total', 'loss/standard/seg', 'loss/standard/image', 'loss/standard/shape', 'loss/standard/gt_shape',
             'loss/hard/total', 'loss/hard/seg', 'loss/hard/image', 'loss/hard/shape']


def get_batch(loader):
    """:48-60: the next batch, wrapping around into a new pass; with the loader's keep_orig it is already [augmented ; original], on the
    device, float32 / int64."""
    return loader.next_batch()


def eval_model(segmentation_model, validate_loader):
    """:63-78: one pass over the validation loader through `evaluate(..., n_iter=2)` -> (mean IoU, mean accuracy).  The targets are
    device tensors: the confusion matrix is accumulated on the device and read once, by get_scores."""
    segmentation_model.eval()
    segmentation_model.running_metric.reset()
    for _ in range(len(validate_loader)):
        clean_image_l, label_l = get_batch(validate_loader)
        segmentation_model.evaluate(input=clean_image_l, targets_npy=label_l, n_iter=2)
    score, _ = segmentation_model.running_metric.get_scores()
    return score['Mean IoU : \t'], score['Mean Acc : \t']


def latent_da_configs(experiment_opt):
    """:125-142 -> (latent_DA, separate_training, image code config or None, shape code config or None)"""
    latent_DA = experiment_opt['learning']['latent_DA']
    separate_training = experiment_opt['learning']['separate_training']
    image_cfg = seg_cfg = None
    if latent_DA:
        scope = experiment_opt['latent_DA']['mask_scope']
        if 'image code' in scope:
            image_cfg = experiment_opt['latent_DA']['image code']
        if 'shape code' in scope:
            seg_cfg = experiment_opt['latent_DA']['shape code']
    return latent_DA, separate_training, image_cfg, seg_cfg


def noise_seed() -> int:
    """The seed of one step's input noise, from torch's host generator (as every device-side counter hash of the engine is seeded)."""
    return int(torch.randint(0, 2 ** 62, (1,)).item())


def train_step(segmentation_solver, clean_image_l, label_l, latent_DA, separate_training, image_cfg, seg_cfg, cooperative=False):
    """:176-233 for one batch -> the 8 losses as detached device scalars: standard (seg, image, gt_shape, shape), hard (seg, image,
    shape, perturbed shape)."""
    segmentation_solver.train()
    segmentation_solver.reset_all_optimizers()
    image_l = basic_operations.add_input_noise(clean_image_l, sigma=0.05, seed=noise_seed())
    if cooperative:
        return segmentation_solver.cooperative_step(clean_image_l, label_l, image_l, image_cfg, seg_cfg, latent_DA=latent_DA,
                                                    separate_training=separate_training)
    seg_loss, image_recon_loss, gt_recon_loss, shape_recon_loss = segmentation_solver.standard_training(
        clean_image_l, label_l, perturbed_image=image_l, separate_training=separate_training)
    standard_loss = seg_loss + image_recon_loss + shape_recon_loss + gt_recon_loss
    if latent_DA:
        segmentation_solver.reset_all_optimizers()
        perturbed_image_0, perturbed_y_0 = segmentation_solver.hard_example_generation(
            clean_image_l.detach().clone(), label_l.detach().clone(), gen_corrupted_seg=seg_cfg is not None,
            gen_corrupted_image=image_cfg is not None, corrupted_image_DA_config=image_cfg, corrupted_seg_DA_config=seg_cfg)
        hard = segmentation_solver.hard_example_training(perturbed_image=perturbed_image_0, perturbed_seg=perturbed_y_0,
                                                         clean_image_l=clean_image_l, label_l=label_l, separate_training=separate_training)
        hard_loss = hard[0] + hard[1] + hard[2] + hard[3]
    else:
        zero = torch.zeros((), device=clean_image_l.device)
        hard, hard_loss = (zero, zero, zero, zero), zero
    loss = standard_loss + hard_loss
    segmentation_solver.reset_all_optimizers()
    loss.backward()
    segmentation_solver.optimize_all_params()
    return tuple(v.detach() for v in (seg_loss, image_recon_loss, gt_recon_loss, shape_recon_loss) + tuple(hard))


TAIL_KEYS = ('lr_policy', 'lr_decay_iters', 'max_grad_norm', 'skip_nonfinite', 'use_ema', 'ema_decay')


def configure_optim_tail(segmentation_solver, learning) -> bool:
    """The optional optimizer-tail keys of experiment_opt['learning'] onto the solver -> is any feature on?  Keys that are absent leave
    what the solver was built with."""
    given = {k: learning[k] for k in TAIL_KEYS if k in learning}
    s = segmentation_solver
    if given:
        s.max_grad_norm = given.get('max_grad_norm', s.max_grad_norm)
        s.skip_nonfinite = bool(given.get('skip_nonfinite', s.skip_nonfinite))
        s.use_ema = bool(given.get('use_ema', s.use_ema))
        s.ema_decay = float(given.get('ema_decay', s.ema_decay))
        if 'lr_policy' in given and given['lr_policy'] != s.lr_policy:
            s.lr_policy, s.schedulers = given['lr_policy'], None
        if 'lr_decay_iters' in given and given['lr_decay_iters'] != s._sched_kw['lr_decay_iters']:
            s._sched_kw['lr_decay_iters'], s.schedulers = given['lr_decay_iters'], None      # (a new schedule starts from the current rates)
        if s.max_grad_norm is not None or s.skip_nonfinite or s.use_ema or s.lr_policy is not None:
            s._enable_tail()
    return bool(getattr(s, '_tail_on', False))


def train_network(segmentation_solver, train_loader, validate_loader, experiment_opt, model_dir, start_epoch=0, cooperative=False,
                  experiment_name='experiment', verbose=True):
    """:144-288.  experiment_opt: upstream's dict -- ['learning'] (n_epochs, max_iteration, latent_DA, separate_training), ['latent_DA']
    (mask_scope, 'image code', 'shape code'), ['output']['save_epoch_every_num_epochs'], ['segmentation_model']['network_type'].  The
    batch size and keep_orig_image_label_pair_for_training are the loaders' (DeviceBatchLoader(train_set, batch_size, keep_orig=True);
    validation: DeviceBatchLoader(val_set, batch_size, keep_orig=False, shuffle=False), each with a generator of its own).
    -> {'score_list', 'best_score', 'losses': one {key: mean over the epoch's steps} per epoch, 'iterations'}.
    Optional keys of ['learning'] switch the solver's optimizer tail on (absent: nothing changes): lr_policy, lr_decay_iters,
    max_grad_norm, skip_nonfinite, use_ema, ema_decay.  The schedule advances once per epoch after validation (the plateau policies get
    the epoch's mean total loss); validation and the 'best' checkpoint then use the EMA weights; the result gains 'lr' and
    'skipped_steps', one entry per epoch, read with the epoch's losses."""
    latent_DA, separate_training, image_cfg, seg_cfg = latent_da_configs(experiment_opt)
    prefix = experiment_opt['segmentation_model']['network_type']
    tail_on = configure_optim_tail(segmentation_solver, experiment_opt['learning'])
    lrs, skipped = [], []
    best_score = -10000
    stop_flag = False
    score_list, losses, iterations = [], [], 0
    segmentation_solver.reset_all_optimizers()
    segmentation_solver.train()
    device = segmentation_solver.device
    i_epoch = start_epoch
    try:
        for i_epoch in range(start_epoch, experiment_opt['learning']['n_epochs']):
            gc.collect()
            g_count = 0
            sums = torch.zeros(len(LOSS_KEYS) + 1, device=device)           # LOSS_KEYS, then the total loss: read once, below
            for i_iter in range(len(train_loader)):
                if stop_flag:
                    break
                clean_image_l, label_l = get_batch(train_loader)
                l = train_step(segmentation_solver, clean_image_l, label_l, latent_DA, separate_training, image_cfg, seg_cfg, cooperative)
                standard, hard = l[0] + l[1] + l[3] + l[2], l[4] + l[5] + l[6] + l[7]
                sums += torch.stack([standard, l[0], l[1], l[3], l[2], hard, l[4], l[5], l[6] + l[7], standard + hard])
                g_count += 1
                iterations += 1
                i_iter += 1
                if i_iter > experiment_opt['learning']['max_iteration']:
                    stop_flag = True
            means = (sums / max(g_count, 1)).tolist()                       # the epoch's one readback of losses
            losses.append(dict(zip(LOSS_KEYS + ['loss/total'], means)))
            if tail_on:
                skipped.append(segmentation_solver.optim_report()['skipped_steps'])      # (joins the epoch's readback)
                lrs.append(next(iter(segmentation_solver.optimizers.values())).param_groups[0]['lr'])
            if verbose:
                print('{} network: {} epoch {} training loss iter: {}, total  loss: {}'.format(experiment_name, prefix, i_epoch, g_count, means[-1]))
            curr_score, _ = eval_model(segmentation_solver, validate_loader)
            score_list.append(curr_score)
            if best_score < curr_score:
                best_score = curr_score
                segmentation_solver.save_model(model_dir, epoch_iter='best', model_prefix=prefix)
            if (i_epoch + 1) % experiment_opt['output']['save_epoch_every_num_epochs'] == 0 or i_epoch == 0:
                segmentation_solver.save_model(model_dir, epoch_iter=i_epoch, model_prefix=prefix)
            if tail_on:
                segmentation_solver.scheduler_step(means[-1])
            if stop_flag:
                break
    except Exception:
        if i_epoch > 0:
            segmentation_solver.save_snapshots(model_dir, epoch=i_epoch)
        raise
    result = {'score_list': score_list, 'best_score': best_score, 'losses': losses, 'iterations': iterations}
    if tail_on:
        result.update(lr=lrs, skipped_steps=skipped)
    return result
