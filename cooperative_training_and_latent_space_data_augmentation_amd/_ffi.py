"""ctypes binding of libctl_hip.so (include/ctl_hip.h).  There is NO fallback: if the HIP library is missing or a call
fails, the product path raises -- it never routes through PyTorch ops or the CPU oracle."""
from __future__ import annotations

import ctypes as C
import os
from collections import namedtuple

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(_HERE, "csrc", "libctl_hip.so")
ABI_VERSION = 11                     # CTL_ABI_VERSION of include/ctl_hip.h this binding was written against
RED_BLOCKS = 512                     # CTL_RED_BLOCKS of ctl_hip.h; checked against the library's compiled value (ctl_red_blocks) at load

# enums of ctl_hip.h
IN_PLAIN, IN_UP2, IN_ZINS2, IN_C4 = 0, 1, 2, 3
ACT_NONE, ACT_LEAKY, ACT_SIGMOID = 0, 1, 2
EPI_BIAS, EPI_ACCUM, EPI_RES, EPI_STATS, EPI_BNBWD, EPI_TAILBWD = 1, 2, 4, 8, 16, 32
(OP_CONV, OP_WGRAD, OP_WGRAD_REDUCE, OP_PACK, OP_BN_FINALIZE, OP_BN_EVAL, OP_BN_ACT, OP_BWD_REDUCE, OP_BN_BWD_FINALIZE,
 OP_BWD_APPLY, OP_CHAN_SUM_FINALIZE, OP_SUMPOOL2, OP_SIGMOID_BWD, OP_ZERO, OP_COPY, OP_PACK_BATCH, OP_WGRAD_REDUCE_BATCH, OP_DROPOUT2D, OP_BN_REPLAY,
 OP_WGRAD_GROUP) = range(1, 21)
WGRAD_GROUP_MAX = 8                  # members of one grouped weight-gradient launch (CTL_OP_WGRAD_GROUP)
OP_MAX_T = 14

CONV_DTYPE = np.dtype([
    ("n", "<i4"), ("hin", "<i4"), ("win", "<i4"), ("cin", "<i4"), ("hout", "<i4"), ("wout", "<i4"), ("cout", "<i4"),
    ("ks", "<i4"), ("stride", "<i4"), ("pad", "<i4"), ("in_mode", "<i4"), ("pro_affine", "<i4"), ("pro_slope", "<f4"),
    ("epi_flags", "<i4"), ("epi_act", "<i4"), ("epi_slope", "<f4"), ("out_h", "<i4"), ("out_w", "<i4"),
    ("out_sy", "<i4"), ("out_sx", "<i4"), ("nsub", "<i4"), ("out_sub", "<i4"), ("groups", "<i4"), ("dt", "<i4")])
DT_BF16, DT_X16, DT_Y16, DT_RES16, DT_X3 = 1, 2, 4, 8, 16
PACK_X3 = 16                         # or-ed into the mode word of a pack record (CTL_PACK_X3)
LOSS_WCE, LOSS_FOCAL, LOSS_DICE, LOSS_FG_DICE = 0, 1, 2, 3      # CTL_LOSS_* kinds of ctl_seg_loss_fwd / ctl_seg_loss_bwd
DLOSS_BOUNDARY, DLOSS_HAUSDORFF_DT = 0, 1                       # CTL_DLOSS_* kinds of ctl_dist_loss_fwd / ctl_dist_loss_bwd
CONS_KL, CONS_CE, CONS_WCE, CONS_MSE, CONS_DICE, CONS_CONTOUR = 1, 2, 4, 8, 16, 32    # CTL_CONS_* bits of ctl_consistency_fwd / _bwd (bit t = kind t)
RECON_MSE, RECON_L1, RECON_SMOOTH_L1, RECON_NCC, RECON_LNCC = 1, 2, 4, 8, 16                 # CTL_RECON_* bits of ctl_recon_loss_fwd / _bwd (bit k = kind k)
ADV_L2, ADV_RMS, ADV_LINF = 0, 1, 2                             # CTL_ADV_* norms of ctl_adv_unit_scale
FIELD_D2, FIELD_SIGNED, FIELD_SQUARED = 0, 1, 2                 # CTL_FIELD_* forms of ctl_class_fields
LABEL_U8, LABEL_I64 = 0, 1                                      # CTL_LABEL_* of ctl_class_fields
TTA_LOGIT, TTA_PROB, TTA_MAX_VIEWS = 0, 1, 8                    # CTL_TTA_* of ctl_tta_merge
# the optimizer tail's control record (CTL_OPTIM_* of ctl_hip.h): word indices of a double[OPTIM_CTRL_DOUBLES], and the pass-1 chunk
OPTIM_CTRL_DOUBLES, OPTIM_MAX_NETS, GRAD_NORM_CHUNK = 32, 8, 16384
OPTIM_LR, OPTIM_MAX_NORM, OPTIM_GUARD, OPTIM_EMA_OMD = 0, 8, 9, 10
OPTIM_SUMSQ, OPTIM_NORM, OPTIM_CLIP, OPTIM_FINITE, OPTIM_SKIPPED = 16, 17, 18, 19, 20
OP_DTYPE = np.dtype([("kind", "<i4"), ("i", "<i4", (27,)), ("f", "<f4", (4,)), ("slot", "<i4", (OP_MAX_T,)),
                     ("off", "<i8", (OP_MAX_T,)), ("l", "<i8", (4,))], align=True)

# Where ctl_plan_run (csrc/ctl_plan.cpp) reads each operand of a record, per kind -- the lines of the "plan record layout" table of
# include/ctl_hip.h, word for word (tests/test_plan_layout_cpu.py compares the two).  `KIND -> entry`: the entry the fields are handed to
# under these, its parameter names.  Banks: i (int32 words: in order from 0, or `k=name` at word k; `conv` = a ctl_conv in i[0..23]),
# l (int64), f (float), t (tensor slots: (slot, byte offset) pairs, slot -1 = NULL).  For READERS and hand-built records (tests, tools):
# the emitters of nets.PlanBuilder still write these positions by hand.
_OP_LAYOUT = """
CONV -> ctl_conv_forward_ex | i: conv | t: x wpack bias pro_scale pro_shift res res_scale res_shift y stats_partial res2 x2 pool xout
WGRAD -> ctl_conv_wgrad_ex | i: conv 24=group_splits | t: x pro_scale pro_shift dy w_partial b_partial dy2 dy_coef
WGRAD_GROUP | i: members
WGRAD_REDUCE -> ctl_wgrad_reduce | i: conv 24=accumulate | l: s_co s_ci s_kh s_kw | t: w_partial b_partial dw dbias
PACK -> ctl_pack_weights | i: cout cin ks flip | l: s_co s_ci s_kh s_kw | t: src dst
BN_FINALIZE -> ctl_bn_finalize_ex | i: blocks c update_running groups | l: count | f: eps momentum | t: partial gamma beta running_mean running_var num_batches_tracked scale shift save_mean save_invstd save_uvar
BN_REPLAY -> ctl_bn_replay_running | i: n_rec | f: momentum | t: act buffers num_batches_tracked table
BN_EVAL -> ctl_bn_eval_coeffs | i: c groups | f: eps | t: gamma beta running_mean running_var scale shift
BN_ACT -> ctl_bn_act_dt | i: c groups 25=bf16_mask | l: pixels | f: slope | t: x scale shift y
BWD_REDUCE -> ctl_bwd_reduce_dt | i: mode c groups 25=bf16_mask | l: pixels | f: slope | t: dy act_src bn_src scale shift partial ds
BN_BWD_FINALIZE -> ctl_bn_bwd_finalize_ex | i: c accumulate groups blocks affine_groups | l: count | t: partial gamma save_mean save_invstd coef dgamma dbeta
BWD_APPLY -> ctl_bwd_apply_dt | i: mode c groups 25=bf16_mask | l: pixels | f: slope | t: dy act_src bn_src scale shift coef ds dx
CHAN_SUM_FINALIZE -> ctl_chan_sum_finalize | i: c accumulate | t: partial out
SUMPOOL2 -> ctl_sumpool2_dt | i: n h w c accumulate 25=bf16_mask | t: dup dx
SIGMOID_BWD -> ctl_sigmoid_bwd | l: count | t: dy y dx
ZERO | l: nbytes | t: dst
COPY | l: nbytes | t: src dst
PACK_BATCH -> ctl_pack_weights_batched | i: n_rec form | l: max_total | t: params wpack table
WGRAD_REDUCE_BATCH -> ctl_wgrad_reduce_batched | i: n_rec | l: max_blocks | t: scratch grad table
DROPOUT2D -> ctl_dropout2d_dt | i: n hw c 25=bf16_mask | l: seed_or_salt | f: p | t: z keep state out keep_out
"""
OpLayout = namedtuple("OpLayout", "name entry conv fields")      # fields: {name: (bank, index)} in the line's order


def _parse_op_layout(text: str) -> dict:
    table = {}
    for ln in text.strip().splitlines():
        head, *banks = [s.strip() for s in ln.split("|")]
        name, _, entry = [s.strip() for s in head.partition("->")]
        fields, conv = {}, False
        for bank, _, names in (b.partition(":") for b in banks):
            k = 0
            for tok in names.split():
                if tok == "conv":
                    conv = True
                elif "=" in tok:
                    fields[tok.split("=")[1]] = (bank, int(tok.split("=")[0]))
                else:
                    fields[tok] = (bank, k)
                    k += 1
        table[globals()["OP_" + name]] = OpLayout(name, entry or None, conv, fields)
    return table


OP_LAYOUT = _parse_op_layout(_OP_LAYOUT)


def op_field(record, name: str):
    """The field `name` of one plan record by OP_LAYOUT: an int (i, l), a float (f), the (slot, byte offset) of a tensor -- slot -1 = NULL --
    or, for `conv`, the ctl_conv record at the head of i."""
    lay = OP_LAYOUT[int(record["kind"])]
    if name == "conv" and lay.conv:
        return np.frombuffer(np.ascontiguousarray(record["i"]).tobytes()[:CONV_DTYPE.itemsize], dtype=CONV_DTYPE)[0]
    if name not in lay.fields:
        raise KeyError(f"a {lay.name} record has no field {name!r} (it has: {' '.join(lay.fields)})")
    bank, k = lay.fields[name]
    if bank == "t":
        return int(record["slot"][k]), int(record["off"][k])
    return float(record["f"][k]) if bank == "f" else int(record[bank][k])


def new_op(kind: int, conv=None, **fields) -> np.ndarray:
    """One plan record of `kind` from named fields (OP_LAYOUT): conv = a ctl_conv record, a tensor field = a (slot, byte offset) pair or
    None; what is not named stays 0 / NULL.  A name the kind does not have raises."""
    lay = OP_LAYOUT[kind]
    unknown = [n for n in fields if n not in lay.fields]
    if unknown or (conv is not None and not lay.conv):
        raise KeyError(f"a {lay.name} record has no field {' '.join(unknown) or 'conv'!r} (it has: {' '.join(lay.fields)})")
    r = np.zeros((), dtype=OP_DTYPE)
    r["kind"] = kind
    r["slot"][:] = -1
    if conv is not None:
        words = np.frombuffer(conv.tobytes(), dtype="<i4")
        r["i"][:len(words)] = words
    for name, v in fields.items():
        bank, k = lay.fields[name]
        if bank != "t":
            r[bank][k] = v
        elif v is not None:
            r["slot"][k], r["off"][k] = v
    return r


# One row of the int64 table behind WGRAD_REDUCE_BATCH, columns in the word order ctl_hip.h documents ("reduce record")
ReduceRow = namedtuple("ReduceRow", "w_off b_off dw_off db_off splits taps_ks cin cout cin_p cout_p s_co s_ci s_kh s_kw accumulate reserved")


class CtlError(RuntimeError):
    pass


def _signatures() -> dict:
    """Every entry of include/ctl_hip.h, in the header's order: name -> (return type, argument types).  The one place a ctl_* name is
    spelled as a definition: load() applies it, EXPORTED is its keys, tests/test_cabi.py compares it with the header's prototypes."""
    p, cstr, int_, i32, i64, u32, u64, f32, f64, sz = (C.c_void_p, C.c_char_p, C.c_int, C.c_int32, C.c_int64, C.c_uint32, C.c_uint64,
                                                       C.c_float, C.c_double, C.c_size_t)
    return {
        "ctl_version": (int_, []),
        "ctl_last_error": (cstr, []),
        "ctl_conv_wpack_floats": (sz, [i32, i32, i32]),
        "ctl_conv_stats_floats": (sz, [p]),
        "ctl_conv_stats_blocks": (int_, [p]),
        "ctl_pack_weights": (int_, [p, p, i32, i32, i32] + [i64] * 4 + [i32, p]),
        "ctl_conv_forward": (int_, [p] * 12),
        "ctl_conv_forward_ex": (int_, [p] * 16),
        "ctl_conv_pool_ok": (int_, [p]),
        "ctl_wgrad_splits": (int_, [p]),
        "ctl_wgrad_partial_floats": (sz, [p]),
        "ctl_wgrad_bias_partial_floats": (sz, [p]),
        "ctl_conv_wgrad": (int_, [p] * 8),
        "ctl_conv_wgrad_ex": (int_, [p] * 10),
        "ctl_wgrad_group_class": (int_, [p, i32]),
        "ctl_wgrad_group_plan": (int_, [p, i32, p]),
        "ctl_conv_wgrad_group": (int_, [i32] + [p] * 11),
        "ctl_wgrad_reduce": (int_, [p] * 4 + [i64] * 4 + [p, i32, p]),
        "ctl_pack_weights_batched": (int_, [p, p, p, i32, i64, p]),
        "ctl_wgrad_reduce_batched": (int_, [p, p, p, i32, i64, p]),
        "ctl_pack_weights_bf16_batched": (int_, [p, p, p, i32, i64, p]),
        "ctl_conv_wpack_floats_x3": (sz, [i32, i32, i32]),
        "ctl_pack_weights_x3_batched": (int_, [p, p, p, i32, i64, p]),
        "ctl_bn_finalize": (int_, [p, i32, i32, i64, p, p, f32, f32, i32] + [p] * 7 + [i32, p]),
        "ctl_bn_finalize_ex": (int_, [p, i32, i32, i64, p, p, f32, f32, i32] + [p] * 8 + [i32, p]),
        "ctl_bn_replay_running": (int_, [p] * 4 + [i32, f32, p]),
        "ctl_bn_eval_coeffs": (int_, [i32] + [p] * 4 + [f32, p, p, i32, p]),
        "ctl_bn_act": (int_, [p, p, p, f32, p, i64, i32, i32, p]),
        "ctl_bwd_reduce": (int_, [i32] + [p] * 5 + [f32, i64, i32, p, i32, p]),
        "ctl_bwd_reduce_rows": (int_, [i32, i64, i32]),
        "ctl_red_blocks": (int_, []),
        "ctl_bn_bwd_finalize": (int_, [p, i32, i64] + [p] * 6 + [i32, i32, i32, p]),
        "ctl_bn_bwd_finalize_ex": (int_, [p, i32, i64] + [p] * 6 + [i32, i32, i32, u32, p]),
        "ctl_bwd_apply": (int_, [i32] + [p] * 5 + [f32, p, i64, i32, p, p, i32, p]),
        "ctl_chan_sum_finalize": (int_, [p, i32, p, i32, p]),
        "ctl_sumpool2": (int_, [p, p] + [i32] * 5 + [p]),
        "ctl_sigmoid_bwd": (int_, [p, p, p, i64, p]),
        "ctl_softmax_t_fwd": (int_, [p, f32, p, i64, i32, p]),
        "ctl_softmax_t_bwd": (int_, [p, p, f32, p, i64, i32, p]),
        "ctl_onehot": (int_, [p, p, i64, i32, p]),
        "ctl_ce2d_fwd": (int_, [p, p, i64, i32, p, p, p]),
        "ctl_ce2d_bwd": (int_, [p, p, p, i64, i32, p, p]),
        "ctl_seg_loss_blocks": (int_, [i32, i64]),
        "ctl_seg_loss_ws_doubles": (sz, [i32, i32, i64, i32]),
        "ctl_seg_loss_fwd": (int_, [i32, p, p, p, f32, i32, i64, i32, p, p, p]),
        "ctl_seg_loss_bwd": (int_, [i32, p, p, p, f32, p, p, i32, i64, i32, p, p]),
        "ctl_class_fields_ws_bytes": (sz, [i32] * 4),
        "ctl_class_fields": (int_, [p] + [i32] * 6 + [p, p, sz, p]),
        "ctl_confident_label": (int_, [p, p, i64, i32, p]),
        "ctl_dist_loss_ws_doubles": (sz, [i32, i32, i64, i32]),
        "ctl_dist_loss_fwd": (int_, [i32, p, p, p, p, i32, i64, i32, p, p, p]),
        "ctl_dist_loss_bwd": (int_, [i32, p, p, p, p, p, i32, i64, i32, p, p]),
        "ctl_consistency_ws_doubles": (sz, [i32] * 5),
        "ctl_consistency_fwd": (int_, [i32] + [p] * 5 + [i32] * 5 + [p, p, p]),
        "ctl_consistency_bwd": (int_, [i32] + [p] * 5 + [i32, p, p] + [i32] * 4 + [p, p]),
        "ctl_avgpool_fwd": (int_, [p] + [i32] * 5 + [p, p]),
        "ctl_avgpool_bwd": (int_, [p] + [i32] * 5 + [p, p]),
        "ctl_recon_ws_doubles": (sz, [i32] * 6),
        "ctl_recon_loss_fwd": (int_, [i32] + [p] * 4 + [i32] * 5 + [f64] + [i32] * 3 + [p, p, p]),
        "ctl_recon_loss_bwd": (int_, [i32] + [p] * 4 + [i32, p, p] + [i32] * 4 + [f64] + [i32] * 3 + [p, p]),
        "ctl_adv_bias_ws_bytes": (sz, [i32] * 4),
        "ctl_adv_bias_fwd": (int_, [p, p] + [i32] * 7 + [p, p, p]),
        "ctl_adv_bias_bwd": (int_, [p, p, p] + [i32] * 7 + [p, sz, p, p, p]),
        "ctl_adv_unit_scale_ws_bytes": (sz, [i32, i64]),
        "ctl_adv_unit_scale": (int_, [p, i32, i64, i32, f64, p, sz, p, p]),
        "ctl_mse_fwd": (int_, [p, p, i64, f32, p, p, p]),
        "ctl_mse_bwd": (int_, [p, p, p, i64, f32, p, p]),
        "ctl_argmax_c": (int_, [p, p, i64, i32, p]),
        "ctl_bn_act_dt": (int_, [p, p, p, f32, p, i64, i32, i32, u32, p]),
        "ctl_bwd_reduce_dt": (int_, [i32] + [p] * 5 + [f32, i64, i32, p, i32, u32, p, p]),
        "ctl_bwd_apply_dt": (int_, [i32] + [p] * 5 + [f32, p, i64, i32, p, p, i32, u32, p]),
        "ctl_sumpool2_dt": (int_, [p, p] + [i32] * 5 + [u32, p]),
        "ctl_latent_score_ws_floats": (sz, [i32] * 4),
        "ctl_latent_score": (int_, [i32, p, p, p, i32, i32, i32, p]),
        "ctl_latent_mask_apply_ws_floats": (sz, [i32] * 4),
        "ctl_latent_mask_apply": (int_, [i32, p, p, p, i32] + [p] * 4 + [i32, i32, i32, p]),
        "ctl_latent_mask_fused_ws_floats": (sz, [i32] * 4),
        "ctl_latent_mask_fused": (int_, [i32, p, p, p, i32] + [p] * 5 + [i32, i32, i32, p]),
        "ctl_dropout2d": (int_, [p, p, u64, f32, p, p, i32, i32, i32, p]),
        "ctl_uniform": (int_, [p, i64, u64, p]),
        "ctl_step_tick": (int_, [p, p]),
        "ctl_spin": (int_, [i32, p]),
        "ctl_dropout2d_ex": (int_, [p, p, u64, p, f32, p, p, p, i32, i32, i32, p]),
        "ctl_uniform_dev": (int_, [p, i64, u64, p, p]),
        "ctl_dropout2d_dt": (int_, [p, p, u64, p, f32, p, p, i32, i32, i32, u32, p]),
        "ctl_confusion_hist": (int_, [p, p, i64, i32, p, p]),
        "ctl_rescale_intensity_ws_floats": (sz, [i32]),
        "ctl_rescale_intensity": (int_, [p, p, p, i32, i64, f32, f32, f32, p]),
        "ctl_noise_clamp": (int_, [p, p, u64, f32, f32, f32, p, i64, p]),
        "ctl_crop_or_pad": (int_, [p, p] + [i32] * 6 + [p]),
        "ctl_surface_stats_rows": (int_, [i32] * 4),
        "ctl_surface_stats_ws_bytes": (sz, [i32] * 6),
        "ctl_surface_stats": (int_, [p, p] + [i32] * 7 + [p, p, p, sz, p]),
        "ctl_surface_quantiles_ws_bytes": (sz, [i32] * 7),
        "ctl_surface_quantiles": (int_, [p, p] + [i32] * 7 + [p, p, i32, p, p, p, sz, p]),
        "ctl_surface_map_ws_bytes": (sz, [i32] * 4),
        "ctl_surface_map": (int_, [p] + [i32] * 5 + [p] * 4 + [sz, p]),
        "ctl_cc_ws_bytes": (sz, [i32] * 5),
        "ctl_cc_label": (int_, [p] + [i32] * 6 + [p, p]),
        "ctl_cc_keep_largest": (int_, [p] + [i32] * 6 + [p, p, p, sz, p]),
        "ctl_predictive_stats_ws_bytes": (sz, [i32, i32, i64, i32, i32]),
        "ctl_predictive_stats": (int_, [p, p, i32, i32, i64, i32, i32, f32, i32] + [p] * 9),
        "ctl_tta_views": (int_, [p, i32, i32, i32, i32, p, i32, p, p]),
        "ctl_tta_merge": (int_, [p] + [i32] * 5 + [p, i32, p, p, p, p]),
        "ctl_aug_ws_bytes": (sz, [i32, i32, i32]),
        "ctl_aug_warp_ws_bytes": (sz, [i32] * 5),
        "ctl_aug_field": (int_, [p] * 4 + [i32, i32, i32, p, p, sz, p]),
        "ctl_aug_warp": (int_, [p] * 5 + [i32] * 5 + [p, p, p, sz, p]),
        "ctl_aug_spline_ws_bytes": (sz, [i32] * 4),
        "ctl_aug_warp_cubic_ws_bytes": (sz, [i32] * 6),
        "ctl_aug_spline_coeffs": (int_, [p, p, p] + [i32] * 4 + [p, p, sz, p]),
        "ctl_aug_warp_cubic": (int_, [p] * 5 + [i32] * 6 + [p, p, p, sz, p]),
        "ctl_aug_bias_ws_bytes": (sz, [i32, i32, i32]),
        "ctl_aug_bias": (int_, [p] * 4 + [i32, i32, i32, p, p, sz, p]),
        "ctl_aug_coarse_field": (int_, [p, i32, i32, i32, p, p]),
        "ctl_order_stats_ws_bytes": (sz, [i32, i32]),
        "ctl_order_stats": (int_, [p, i32, i64, p, i32, p, p, sz, p]),
        "ctl_percentile_apply": (int_, [p, p, i32, i64, f64, f64, i32, f32, f32, p, p, p]),
        "ctl_resample_inplane": (int_, [p, p] + [i32] * 6 + [f64, f64, p, p, p]),
        "ctl_restore_scores": (int_, [p] + [i32] * 10 + [f64, f64, i32, p, p, p]),
        "ctl_restore_labels": (int_, [p] + [i32] * 9 + [f64, f64, p, p]),
        "ctl_corrupt_bias": (int_, [p, p, i32, i32, i32, p, p]),
        "ctl_corrupt_spike_ws_bytes": (sz, [i32] * 4),
        "ctl_corrupt_spike": (int_, [p, i32, i32, i32, p, p, i32, f64, p, p, sz, p]),
        "ctl_corrupt_rigid3d": (int_, [p, i32, i32, i32, p, i32, p, p]),
        "ctl_axis_operator": (int_, [p, p] + [i32] * 5 + [p, p, p]),
        "ctl_slice_foreground": (int_, [p, p, i32, i64, p, p]),
        "ctl_batch_gather": (int_, [p, p, p, i32, i64, p, i32, p, i32, i32, p, p, i32, i32, p, p, p]),
        "ctl_adam": (int_, [p] * 4 + [i64] + [f32] * 4 + [i32, f32, p]),
        "ctl_accumulate": (int_, [p, p, i32, i64, p]),
        "ctl_adam_dev": (int_, [p] * 4 + [i64] + [f32] * 4 + [p, f32, p]),
        "ctl_optim_control": (int_, [p, i32, p, f32, i32, f32, p]),
        "ctl_grad_norm_work": (sz, [p, i32]),
        "ctl_grad_norm": (int_, [p, p, i32, f32, p, p, p]),
        "ctl_adam_tail": (int_, [p] * 5 + [i64] + [f32] * 3 + [p, i32, f32, p, i32, p]),
        "ctl_plan_run": (int_, [p, i32, p, i32, p]),
        "ctl_prof_start": (int_, [cstr]),
        "ctl_prof_start_sampled": (int_, [cstr, i32]),
        "ctl_prof_stop": (int_, [p, sz]),
        "ctl_launch_count": (C.c_ulonglong, []),
        "ctl_sizeof_op": (sz, []),
        "ctl_sizeof_conv": (sz, []),
    }


SIGNATURES = _signatures()
EXPORTED = list(SIGNATURES)


class _Lib:
    def __init__(self):
        self._lib = None

    def load(self):
        if self._lib is not None:
            return self._lib
        if not os.path.exists(LIB_PATH):
            raise CtlError(f"HIP extension not built: {LIB_PATH} is missing. Run `python -c 'import __graft_entry__ as g; "
                           "g.build()'` (or `make -C <package>/csrc`). There is no fallback path.")
        # PyTorch first: its wheel carries its own libamdhip64.so, and the extension must bind to THAT runtime (the one that owns the
        # device, the streams and the memory).  Loaded before torch, the extension pulled in /opt/rocm's copy instead and every launch
        # failed with "no ROCm-capable device is detected" (build() followed by smoke() in one process).
        import torch  # noqa: F401
        lib = C.CDLL(LIB_PATH)
        for name, (restype, argtypes) in SIGNATURES.items():
            fn = getattr(lib, name)
            fn.restype, fn.argtypes = restype, argtypes
        if lib.ctl_version() != ABI_VERSION or lib.ctl_sizeof_op() != OP_DTYPE.itemsize or lib.ctl_sizeof_conv() != CONV_DTYPE.itemsize:
            raise CtlError(f"ABI mismatch: library version {lib.ctl_version()} vs binding {ABI_VERSION}, sizeof(ctl_op)={lib.ctl_sizeof_op()} "
                           f"vs {OP_DTYPE.itemsize}, sizeof(ctl_conv)={lib.ctl_sizeof_conv()} vs {CONV_DTYPE.itemsize}")
        if lib.ctl_red_blocks() != RED_BLOCKS:
            raise CtlError(f"ABI mismatch: the library was built with CTL_RED_BLOCKS={lib.ctl_red_blocks()}, this binding sizes scratch for {RED_BLOCKS}")
        self._lib = lib
        return lib

    def __getattr__(self, name):
        return getattr(self.load(), name)


lib = _Lib()


def prof_start(kernel_filter: str = "", every: int = 1) -> None:
    """Bracket the launches whose id contains `kernel_filter` with HIP events on their own stream (every `every`-th one)."""
    call("ctl_prof_start_sampled", kernel_filter.encode(), int(every))


def prof_stop() -> dict:
    """{kernel id: dict(launches, ms, flops, bytes)} for the launches bracketed since prof_start."""
    buf = C.create_string_buffer(1 << 18)
    call("ctl_prof_stop", buf, len(buf))
    out = {}
    for line in buf.value.decode().splitlines():
        parts = line.split()
        out[parts[0]] = {k: float(v) for k, v in (kv.split("=") for kv in parts[1:])}
    return out


def check(rc: int, what: str = "") -> None:
    if rc != 0:
        msg = lib.ctl_last_error()
        raise CtlError(f"{what} failed (rc={rc}): {msg.decode() if msg else ''}")


def call(name: str, *args) -> None:
    """Call the status-returning entry `name`; a non-zero status raises CtlError naming that entry."""
    check(getattr(lib, name)(*args), name)


def conv_desc(**kw) -> np.ndarray:
    """Build a ctl_conv record (numpy scalar array of CONV_DTYPE) with defaults for the plain, non-scattered case."""
    d = np.zeros((), dtype=CONV_DTYPE)
    d["pad"] = 1 if kw.get("ks", 3) in (3, 4) else 0
    d["stride"] = 1
    d["nsub"] = 1
    d["groups"] = 1
    d["out_sy"] = d["out_sx"] = 1
    for k, v in kw.items():
        d[k] = v
    if "out_h" not in kw:
        d["out_h"] = d["hout"]
    if "out_w" not in kw:
        d["out_w"] = d["wout"]
    return d


def desc_ptr(d: np.ndarray) -> int:
    return d.ctypes.data
