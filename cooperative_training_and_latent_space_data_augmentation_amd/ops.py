"""Thin tensor-level wrappers over the C-ABI (one call = one kernel enqueue on torch's current stream).

PyTorch is used here only for device memory and the stream handle.  4-D activations are logical NCHW tensors in
``torch.channels_last`` memory format, i.e. NHWC in HBM, which is what every kernel expects.
"""
from __future__ import annotations

import ctypes as C
from collections import namedtuple
from typing import Optional

import numpy as np
import torch

from . import _ffi
from ._ffi import lib, call
# the loss families own their name -> kind tables and their argument rules (losses.py, consistency.py, recon.py); the wrappers below call them
from .consistency import CONSISTENCY_KINDS, check_kinds as check_consistency_kinds, check_plane
from .losses import (DIST_LOSS_FORM, DIST_LOSS_KINDS, LOSS_KINDS, MAX_CLASSES, check_mask, check_names, check_two_classes, class_weight_tuple,
                     mask_u8)      # MAX_CLASSES = 16: channel rows of the loss / statistics kernels
from .recon import RECON_KINDS, check_image, check_params as check_recon_params


def stream_ptr() -> int:
    return torch.cuda.current_stream().cuda_stream


def ptr(t: Optional[torch.Tensor]) -> Optional[int]:
    return None if t is None else t.data_ptr()


def require_gpu(*ts: torch.Tensor) -> None:
    for t in ts:
        if t is not None and not t.is_cuda:
            raise _ffi.CtlError("the HIP path needs device tensors (got a CPU tensor); there is no CPU fallback")


def as_nhwc(x: torch.Tensor) -> torch.Tensor:
    """Logical NCHW tensor whose memory is NHWC (no copy if it already is)."""
    if x.dim() != 4:
        raise ValueError("expected a 4-D NCHW tensor")
    return x.float().contiguous(memory_format=torch.channels_last)


def empty_nhwc(n: int, c: int, h: int, w: int, device, dtype=torch.float32) -> torch.Tensor:
    return torch.empty((n, c, h, w), dtype=dtype, device=device, memory_format=torch.channels_last)


def as_nhwc_any(x: torch.Tensor) -> torch.Tensor:
    """NHWC memory, dtype kept (fp32 or bf16): the bf16 kernel family reads either (ctl_conv.dt)."""
    if x.dim() != 4 or x.dtype not in (torch.float32, torch.bfloat16):
        raise ValueError("expected a 4-D fp32 / bf16 NCHW tensor")
    return x.contiguous(memory_format=torch.channels_last)


def _arg(t: torch.Tensor, dtype, shape, who: str, name: str, dense: bool = False, on_device: bool = False) -> None:
    """ValueError unless the tensor argument `name` of `who` has `dtype` (one, or a tuple to choose from) and `shape` (None: any size on
    that axis), is contiguous (dense) and sits on the device (on_device)."""
    dtypes = dtype if isinstance(dtype, tuple) else (dtype,)
    fits = t.dim() == len(shape) and all(want is None or want == got for want, got in zip(shape, t.shape))
    if t.dtype not in dtypes or not fits or (dense and not t.is_contiguous()) or (on_device and not t.is_cuda):
        kind = ("a contiguous " if dense else "a ") + " or ".join(str(v).replace("torch.", "") for v in dtypes) + (" device" if on_device else "")
        dims = ",".join("*" if v is None else str(int(v)) for v in shape)
        raise ValueError(f"{who}: {name} must be {kind} tensor [{dims}], got {t.dtype} {tuple(t.shape)}"
                         f"{'' if t.is_contiguous() else ' (strided)'}{'' if t.is_cuda else ' on the host'}")


def _out(out: Optional[torch.Tensor], dtype, shape, device, who: str, name: str = "out", on_device: bool = True, not_input=None) -> torch.Tensor:
    """A caller-supplied output: a new tensor when None, else it must be a contiguous `dtype` tensor of `shape` (ValueError), on the device
    unless the wrapper leaves that to require_gpu (on_device=False), and not the tensor `not_input`."""
    if out is None:
        return torch.empty(tuple(shape), dtype=dtype, device=device)
    _arg(out, dtype, tuple(shape), who, f"`{name}`", dense=True, on_device=on_device)
    if not_input is not None and out.data_ptr() == not_input.data_ptr():
        raise ValueError(f"{who}: `{name}` must not be the input")
    return out


def _workspace(query: str, *dims, device, dtype=torch.uint8, floor: int = 1):
    """(tensor, size) for the library's size query `query(*dims)`: a `dtype` device tensor of max(size, floor) elements."""
    size = getattr(lib, query)(*dims)
    return torch.empty(max(size, floor), dtype=dtype, device=device), size


def _nhwc_f32(who: str, text: str, *tensors, also: bool = True) -> None:
    """ValueError(f"{who}: {text}") unless every tensor is 4-D fp32 and NHWC in memory (and `also` holds)."""
    if not (all(t.dim() == 4 and t.dtype == torch.float32 and t.permute(0, 2, 3, 1).is_contiguous() for t in tensors) and also):
        raise ValueError(f"{who}: {text}")


def _kind_bits(kinds, table):
    """(bits, c_double array of len(table)) of a checked {name: weight} mapping over the {name: bit} `table`; bit t is kind t, the order of the weights."""
    bits, weights = 0, [0.0] * len(table)
    for name, weight in kinds.items():
        bits |= table[name]
        weights[table[name].bit_length() - 1] = float(weight)
    return bits, (C.c_double * len(weights))(*weights)


def _class_weight_array(class_weights, c: int):
    """One double per class of a host sequence (the library normalises it in fp64)."""
    return (C.c_double * c)(*class_weight_tuple(class_weights, c))


def _kinds_scratch(query: str, dims, table, device):
    """(ws, loss) of a fused forward over the kinds of `table`: its fp64 scratch of `query(*dims)` doubles and the fp32 vector [total, one
    term per kind] it writes."""
    return _workspace(query, *dims, device=device, dtype=torch.float64)[0], torch.empty(1 + len(table), dtype=torch.float32, device=device)


def _scratch_given(ws, gout, query: str, dims, who: str, fwd: str) -> None:
    """ValueError unless `ws` can be the scratch that the forward `fwd` returned for these sizes."""
    require_gpu(gout, ws)
    _arg(ws, torch.float64, (None,), who, "ws", dense=True)
    if ws.numel() < getattr(lib, query)(*dims):
        raise ValueError(f"{who}: `ws` is not the scratch of {fwd} for these arguments")


def _logits_and_label(logit, label, who: str, *fields):
    """(n, c, h, w) of fp32 NHWC logits [B,C,H,W], their contiguous int64 label map [B,H,W] and the fp32 NHWC `fields` of the logits' shape"""
    if logit.dim() != 4 or logit.dtype != torch.float32 or label.dtype != torch.int64 or \
            tuple(label.shape) != (logit.shape[0], logit.shape[2], logit.shape[3]):
        raise ValueError(f"{who}: expected fp32 logits [B,C,H,W] and an int64 label map [B,H,W]")
    for f in fields:
        _arg(f, torch.float32, tuple(logit.shape), who, "a field")
    _nhwc_f32(who, "the logits" + (" and the fields" if fields else "") + " must be NHWC in memory (channels_last) and the label map contiguous",
              logit, *fields, also=label.is_contiguous())
    return tuple(int(v) for v in logit.shape)


# ---------------------------------------------------------------------------------------------- conv (unit-level API)
def pack_weights(src: torch.Tensor, cout: int, cin: int, ks: int, strides, flip: bool, src_offset: int = 0) -> torch.Tensor:
    require_gpu(src)
    n = lib.ctl_conv_wpack_floats(cin, cout, ks)
    dst = torch.empty(n, dtype=torch.float32, device=src.device)
    call("ctl_pack_weights", src.data_ptr() + 4 * src_offset, dst.data_ptr(), cout, cin, ks, *[int(s) for s in strides], int(flip), stream_ptr())
    return dst


def pack_oihw_fwd(w: torch.Tensor) -> torch.Tensor:
    co, ci, ks, _ = w.shape
    return pack_weights(w.contiguous(), co, ci, ks, (ci * ks * ks, ks * ks, ks, 1), False)


def pack_oihw_dgrad(w: torch.Tensor) -> torch.Tensor:
    co, ci, ks, _ = w.shape
    return pack_weights(w.contiguous(), ci, co, ks, (ks * ks, ci * ks * ks, ks, 1), True)


def pack_weights_bf16(w: torch.Tensor, cout: int, cin: int, ks: int, strides, flip=0, mode: int = 0) -> torch.Tensor:
    """bf16 MFMA fragments (tap pairs x 16-channel chunks, see ctl_conv_bf16.hip) of one effective conv through the table-driven pack
    kernel; `strides`/`flip`/`mode` as in ctl_pack_weights_batched records."""
    require_gpu(w)
    total = lib.ctl_conv_wpack_floats(cin, cout, ks)
    table = torch.tensor([[0, 0, cout, cin, ks, int(flip), *[int(v) for v in strides], total, mode]], dtype=torch.int64, device=w.device)
    dst = torch.zeros(total, dtype=torch.float32, device=w.device)
    src = w.contiguous().float()
    call("ctl_pack_weights_bf16_batched", src.data_ptr(), dst.data_ptr(), table.data_ptr(), 1, total, stream_ptr())
    return dst


def pack_weights_x3(w: torch.Tensor, cout: int, cin: int, ks: int, strides, flip=0, mode: int = 0) -> torch.Tensor:
    """Three-plane bf16 fragments for CTL_DT_X3 launches (hi | mid | lo planes summing exactly to the fp32 weight, ctl_conv_x3.hip) of
    one effective conv; `strides` / `flip` / `mode` as in ctl_pack_weights_batched records."""
    require_gpu(w)
    total = lib.ctl_conv_wpack_floats_x3(cin, cout, ks)
    table = torch.tensor([[0, 0, cout, cin, ks, int(flip), *[int(v) for v in strides], total, mode | _ffi.PACK_X3]], dtype=torch.int64, device=w.device)
    dst = torch.zeros(total, dtype=torch.float32, device=w.device)
    src = w.contiguous().float()
    call("ctl_pack_weights_x3_batched", src.data_ptr(), dst.data_ptr(), table.data_ptr(), 1, total, stream_ptr())
    return dst


def pack_oihw_fwd_x3(w: torch.Tensor) -> torch.Tensor:
    co, ci, ks, _ = w.shape
    return pack_weights_x3(w, co, ci, ks, (ci * ks * ks, ks * ks, ks, 1), 0)


def pack_oihw_dgrad_x3(w: torch.Tensor) -> torch.Tensor:
    co, ci, ks, _ = w.shape
    return pack_weights_x3(w, ci, co, ks, (ks * ks, ci * ks * ks, ks, 1), 1)


def pack_oihw_fwd_bf16(w: torch.Tensor) -> torch.Tensor:
    co, ci, ks, _ = w.shape
    return pack_weights_bf16(w, co, ci, ks, (ci * ks * ks, ks * ks, ks, 1), 0)


def pack_oihw_dgrad_bf16(w: torch.Tensor) -> torch.Tensor:
    co, ci, ks, _ = w.shape
    return pack_weights_bf16(w, ci, co, ks, (ks * ks, ci * ks * ks, ks, 1), 1)


def conv_forward(d: np.ndarray, x, wpack, bias=None, pro_scale=None, pro_shift=None, res=None, res_scale=None,
                 res_shift=None, y=None, want_stats=False, x2=None, res2=None, pool=None, xout=None):
    """Run one conv problem described by the ctl_conv record `d`.  Returns (y, stats_partial or None).  With d["dt"] & DT_BF16 the
    storage dtypes of x / res / y must agree with the DT_X16 / DT_RES16 / DT_Y16 flags (y is allocated accordingly).
    x2 (d["pro_affine"] == 2): the BatchNorm-backward prologue, input = A*x + B*x2 + C with pro_scale = [groups][3][cin] coefficients.
    res2 (CTL_EPI_TAILBWD): res = the block output, res2 = the BatchNorm input of the residual tail; pool: that epilogue also writes the
    2x2 sum-pool of its result into this [n, h/2, w/2, cout] tensor (lib.ctl_conv_pool_ok(desc) says whether the problem can);
    xout (with x2): the virtual input the conv stages is also written to this tensor of x's shape and dtype."""
    require_gpu(x, wpack)
    if (x2 is not None) != (int(d["pro_affine"]) == 2) or (x2 is not None and (x2.dtype != x.dtype or x2.shape != x.shape)):
        raise _ffi.CtlError("conv_forward: x2 goes with ctl_conv.pro_affine == 2 and has the dtype and shape of x")
    n, cout, oh, ow = int(d["n"]), int(d["cout"]), int(d["out_h"]), int(d["out_w"])
    dt = int(d["dt"])
    for t, flag, what in ((x, _ffi.DT_X16, "x"), (res, _ffi.DT_RES16, "res"), (res2, _ffi.DT_RES16, "res2"), (y, _ffi.DT_Y16, "y")):
        if t is not None and (t.dtype == torch.bfloat16) != bool(dt & flag):
            raise _ffi.CtlError(f"conv_forward: dtype of {what} ({t.dtype}) disagrees with ctl_conv.dt = {dt}")
    if y is None:
        y = empty_nhwc(n, cout, oh, ow, x.device, torch.bfloat16 if dt & _ffi.DT_Y16 else torch.float32)
    stats = None
    if want_stats:
        stats = torch.empty(lib.ctl_conv_stats_floats(_ffi.desc_ptr(d)), dtype=torch.float32, device=x.device)
    call("ctl_conv_forward_ex", _ffi.desc_ptr(d), ptr(x), ptr(wpack), ptr(bias), ptr(pro_scale), ptr(pro_shift), ptr(res),
         ptr(res_scale), ptr(res_shift), ptr(res2), ptr(x2), ptr(y), ptr(stats), ptr(pool), ptr(xout), stream_ptr())
    return y, stats


def conv_wgrad(d: np.ndarray, x, dy, dw: torch.Tensor, strides, dbias: Optional[torch.Tensor] = None, pro_scale=None,
               pro_shift=None, accumulate=False, dy2=None, dy_coef=None):
    """dy2 / dy_coef: the output gradient is the virtual BatchNorm-backward result A*dy + B*dy2 + C (ctl_conv_wgrad_ex)."""
    require_gpu(x, dy, dw)
    if dy2 is not None and (dy_coef is None or dy2.dtype != dy.dtype or dy2.shape != dy.shape):
        raise _ffi.CtlError("conv_wgrad: dy2 needs dy_coef and the dtype and shape of dy")
    dt = int(d["dt"])
    if (x.dtype == torch.bfloat16) != bool(dt & _ffi.DT_X16) or (dy.dtype == torch.bfloat16) != bool(dt & _ffi.DT_Y16):
        raise _ffi.CtlError(f"conv_wgrad: dtypes of x / dy ({x.dtype}, {dy.dtype}) disagree with ctl_conv.dt = {dt}")
    dp = _ffi.desc_ptr(d)
    wpart = torch.empty(lib.ctl_wgrad_partial_floats(dp), dtype=torch.float32, device=x.device)
    bpart = torch.empty(lib.ctl_wgrad_bias_partial_floats(dp), dtype=torch.float32, device=x.device) if dbias is not None else None
    call("ctl_conv_wgrad_ex", dp, ptr(x), ptr(pro_scale), ptr(pro_shift), ptr(dy), ptr(dy2), ptr(dy_coef), ptr(wpart), ptr(bpart), stream_ptr())
    call("ctl_wgrad_reduce", dp, ptr(wpart), ptr(bpart), ptr(dw), *[int(s) for s in strides], ptr(dbias), int(accumulate), stream_ptr())
    return dw, dbias


# ---------------------------------------------------------------------------------------------- BN pieces
def bn_finalize(partial, c, count, gamma, beta, eps=1e-5, momentum=0.1, running_mean=None, running_var=None, nbt=None, groups=1):
    """partial: [groups][blocks][2][c]; `count` = pixels of one group.  Returns scale, shift, mean, invstd, each [groups*c]."""
    dev = partial.device
    scale, shift, mean, invstd = (torch.empty(groups * c, dtype=torch.float32, device=dev) for _ in range(4))
    blocks = partial.numel() // (2 * c * groups)
    call("ctl_bn_finalize", ptr(partial), blocks, c, count, ptr(gamma), ptr(beta), eps, momentum,
         int(running_mean is not None), ptr(running_mean), ptr(running_var), ptr(nbt), ptr(scale),
         ptr(shift), ptr(mean), ptr(invstd), groups, stream_ptr())
    return scale, shift, mean, invstd


def bn_act(x, scale, shift, slope, groups=1):
    y = torch.empty_like(x)
    n, c, h, w = x.shape
    call("ctl_bn_act", ptr(x), ptr(scale), ptr(shift), slope, ptr(y), n * h * w, c, groups, stream_ptr())
    return y


# ---------------------------------------------------------------------------------------------- STN input / losses
def softmax_t_fwd(x: torch.Tensor, temperature: float = 2.0) -> torch.Tensor:
    require_gpu(x)
    n, c, h, w = x.shape
    p = torch.empty_like(x)
    call("ctl_softmax_t_fwd", ptr(x), 1.0 / temperature, ptr(p), n * h * w, c, stream_ptr())
    return p


def softmax_t_bwd(p, dp, temperature: float = 2.0):
    n, c, h, w = p.shape
    dx = torch.empty_like(p)
    call("ctl_softmax_t_bwd", ptr(p), ptr(dp), 1.0 / temperature, ptr(dx), n * h * w, c, stream_ptr())
    return dx


def onehot(label: torch.Tensor, c: int) -> torch.Tensor:
    require_gpu(label)
    label = label.long().contiguous()
    n, h, w = label.shape
    y = empty_nhwc(n, c, h, w, label.device)
    call("ctl_onehot", ptr(label), ptr(y), n * h * w, c, stream_ptr())
    return y


def ce2d_fwd(logit, label):
    n, c, h, w = logit.shape
    partial = torch.empty(_ffi.RED_BLOCKS, dtype=torch.float64, device=logit.device)
    loss = torch.empty((), dtype=torch.float32, device=logit.device)
    call("ctl_ce2d_fwd", ptr(logit), ptr(label), n * h * w, c, ptr(partial), ptr(loss), stream_ptr())
    return loss


def ce2d_bwd(logit, label, gout):
    n, c, h, w = logit.shape
    d = torch.empty_like(logit)
    call("ctl_ce2d_bwd", ptr(logit), ptr(label), ptr(gout), n * h * w, c, ptr(d), stream_ptr())
    return d


def _loss_args(logit, label, kind, class_weights):
    """The kinds of losses.LOSS_KINDS; the name is checked before the tensors are looked at."""
    check_names((kind,), LOSS_KINDS, "segmentation loss")
    require_gpu(logit, label)
    n, c, h, w = _logits_and_label(logit, label, "segmentation loss")
    wts = _class_weight_array(class_weights, c) if class_weights is not None and LOSS_KINDS[kind] == _ffi.LOSS_WCE else None
    return LOSS_KINDS[kind], n, h * w, c, wts


def seg_loss_fwd(logit, label, kind, class_weights=None, gamma=2.0):
    """(loss, ws): `ws` holds the block sums and, for the Dice kinds, the coefficient table seg_loss_bwd reads."""
    k, n, hw, c, wts = _loss_args(logit, label, kind, class_weights)
    ws = torch.empty(max(1, lib.ctl_seg_loss_ws_doubles(k, n, hw, c)), dtype=torch.float64, device=logit.device)
    loss = torch.empty((), dtype=torch.float32, device=logit.device)
    call("ctl_seg_loss_fwd", k, ptr(logit), ptr(label), wts, gamma, n, hw, c, ptr(ws), ptr(loss), stream_ptr())
    return loss, ws


def seg_loss_bwd(logit, label, kind, gout, ws=None, class_weights=None, gamma=2.0):
    """gout: 0-d fp32 device tensor; ws: what seg_loss_fwd returned (the Dice kinds need it)."""
    k, n, hw, c, wts = _loss_args(logit, label, kind, class_weights)
    require_gpu(gout, ws)
    d = torch.empty_like(logit)
    call("ctl_seg_loss_bwd", k, ptr(logit), ptr(label), wts, gamma, ptr(gout), ptr(ws), n, hw, c, ptr(d), stream_ptr())
    return d


# ---------------------------------------------------------------------------------------------- distance-map losses
FIELD_FORMS = {"d2": _ffi.FIELD_D2, "signed": _ffi.FIELD_SIGNED, "squared": _ffi.FIELD_SQUARED}


def class_fields(label: torch.Tensor, n_class: int, form: str = "d2") -> torch.Tensor:
    """Class fields of a uint8 / int64 label map [B,H,W] (losses.class_fields_host): 'd2' = the exact squared fields, fp64 [B,C,H,W]; the
    training forms 'signed' (Kervadec's signed map) and 'squared', fp32 logical [B,C,H,W] in NHWC memory like the logits they meet."""
    if form not in FIELD_FORMS:
        raise ValueError(f"class_fields: form {form!r} (one of {', '.join(FIELD_FORMS)})")
    n_class = int(n_class)
    if not 1 <= n_class <= MAX_CLASSES:
        raise ValueError(f"class_fields: {n_class} classes (1 .. {MAX_CLASSES})")
    require_gpu(label)
    _arg(label, (torch.uint8, torch.int64), (None, None, None), "class_fields", "label", dense=True)
    b, h, w = (int(v) for v in label.shape)
    if form == "d2":
        out = torch.empty((b, n_class, h, w), dtype=torch.float64, device=label.device)
    else:
        out = empty_nhwc(b, n_class, h, w, label.device)
    ws, nbytes = _workspace("ctl_class_fields_ws_bytes", b, h, w, n_class, device=label.device)
    call("ctl_class_fields", ptr(label), _ffi.LABEL_U8 if label.dtype == torch.uint8 else _ffi.LABEL_I64, b, h, w, n_class, FIELD_FORMS[form],
         ptr(out), ptr(ws), nbytes, stream_ptr())
    return out


def confident_label(logit: torch.Tensor) -> torch.Tensor:
    """uint8 [B,H,W]: the class whose softmax probability exceeds 1/2, 255 where none does (losses.confident_label_host)."""
    require_gpu(logit)
    logit = as_nhwc(logit)
    n, c, h, w = logit.shape
    out = torch.empty((n, h, w), dtype=torch.uint8, device=logit.device)
    call("ctl_confident_label", ptr(logit), ptr(out), n * h * w, c, stream_ptr())
    return out


def _dist_loss_args(logit, label, kind, field_a, field_b):
    check_names((kind,), DIST_LOSS_KINDS, "distance-map loss")
    two = kind == "hausdorff dt"
    fields = (field_a, field_b) if two else (field_a,)
    if any(f is None for f in fields):
        raise ValueError(f"{kind!r} needs {'two field tensors (label, prediction)' if two else 'the signed map of the label'}")
    require_gpu(logit, label, *fields)
    n, c, h, w = _logits_and_label(logit, label, "distance-map loss", *fields)
    check_two_classes(kind, c)
    return DIST_LOSS_KINDS[kind], n, h * w, c


def dist_loss_fwd(logit, label, kind, field_a, field_b=None):
    """0-d fp32 device loss of 'boundary' (field_a = the signed map of the label) or 'hausdorff dt' (field_a / field_b = the squared fields of
    the label / of confident_label(logit))."""
    k, n, hw, c = _dist_loss_args(logit, label, kind, field_a, field_b)
    ws = torch.empty(max(1, lib.ctl_dist_loss_ws_doubles(k, n, hw, c)), dtype=torch.float64, device=logit.device)
    loss = torch.empty((), dtype=torch.float32, device=logit.device)
    call("ctl_dist_loss_fwd", k, ptr(logit), ptr(label), ptr(field_a), ptr(field_b), n, hw, c, ptr(ws), ptr(loss), stream_ptr())
    return loss


def dist_loss_bwd(logit, label, kind, gout, field_a, field_b=None):
    """gout (0-d fp32 device tensor) * dloss/dlogit; the prediction field of 'hausdorff dt' is a constant."""
    k, n, hw, c = _dist_loss_args(logit, label, kind, field_a, field_b)
    require_gpu(gout)
    d = torch.empty_like(logit)
    call("ctl_dist_loss_bwd", k, ptr(logit), ptr(label), ptr(field_a), ptr(field_b), ptr(gout), n, hw, c, ptr(d), stream_ptr())
    return d


# ---------------------------------------------------------------------------------------------- consistency losses
def _consistency_args(output, reference, kinds, class_weights, mask, who):
    """(kind bits, weights, class weights, mask as uint8, n, h, w, c) of a {name: weight} mapping `kinds`; names and weights are checked
    before the tensors are looked at."""
    check_consistency_kinds(kinds, class_weights)
    bits, weights = _kind_bits(kinds, CONSISTENCY_KINDS)
    require_gpu(output, reference, mask)
    if output.dim() != 4 or output.dtype != torch.float32 or reference.dtype != torch.float32 or tuple(reference.shape) != tuple(output.shape):
        raise ValueError(f"{who}: expected fp32 output and reference logits of one shape [B,C,H,W]")
    _nhwc_f32(who, "output and reference must be NHWC in memory (channels_last)", output, reference)
    n, c, h, w = (int(v) for v in output.shape)
    if "contour" in kinds:
        check_two_classes("contour", c)
    wts = _class_weight_array(class_weights, c) if class_weights is not None and "weighted ce" in kinds else None
    check_mask(mask, output.shape)
    return bits, weights, wts, mask_u8(mask), n, h, w, c


def consistency_fwd(output, reference, kinds, class_weights=None, mask=None, is_gt=False):
    """(loss, terms, ws) of the {name: weight} mapping `kinds` (CONSISTENCY_KINDS): the 0-d weighted total, fp32 terms[6] in the order of
    CONSISTENCY_KINDS (0 for a name that is not in `kinds`), and the scratch consistency_bwd reads.  `mask`: [B,1,H,W] or [B,H,W], any
    dtype, nonzero = 1 (a contiguous uint8 mask is used as it is)."""
    bits, weights, wts, mask, n, h, w, c = _consistency_args(output, reference, kinds, class_weights, mask, "consistency_fwd")
    ws, loss = _kinds_scratch("ctl_consistency_ws_doubles", (bits, n, h, w, c), CONSISTENCY_KINDS, output.device)
    call("ctl_consistency_fwd", bits, weights, wts, ptr(output), ptr(reference), ptr(mask), int(bool(is_gt)), n, h, w, c, ptr(ws), ptr(loss),
         stream_ptr())
    return loss[0], loss[1:], ws


def consistency_bwd(output, reference, kinds, gout, ws, class_weights=None, mask=None, is_gt=False):
    """gout (0-d fp32 device tensor) * d total / d output; `ws` is what consistency_fwd returned for the same arguments."""
    bits, weights, wts, mask, n, h, w, c = _consistency_args(output, reference, kinds, class_weights, mask, "consistency_bwd")
    _scratch_given(ws, gout, "ctl_consistency_ws_doubles", (bits, n, h, w, c), "consistency_bwd", "consistency_fwd")
    d = torch.empty_like(output)
    call("ctl_consistency_bwd", bits, weights, wts, ptr(output), ptr(reference), ptr(mask), int(bool(is_gt)), ptr(gout), ptr(ws), n, h, w, c,
         ptr(d), stream_ptr())
    return d


def _pool_args(x, scale, who):
    require_gpu(x)
    scale = int(scale)
    _nhwc_f32(who, "expected an fp32 [B,C,H,W] tensor that is NHWC in memory (channels_last)", x)
    if not 1 <= scale <= 4:
        raise ValueError(f"{who}: scale {scale} (1 .. 4)")
    return scale, tuple(int(v) for v in x.shape)


def avgpool_fwd(x: torch.Tensor, scale: int) -> torch.Tensor:
    """AvgPool2d(2^scale) (window = stride, floor sizes) of fp32 NHWC logits: the fp64 window mean, rounded once."""
    scale, (n, c, h, w) = _pool_args(x, scale, "avgpool_fwd")
    check_plane(h, w, scale)
    y = empty_nhwc(n, c, h >> scale, w >> scale, x.device)
    call("ctl_avgpool_fwd", ptr(x), n, h, w, c, scale, ptr(y), stream_ptr())
    return y


def avgpool_bwd(gy: torch.Tensor, scale: int, hw) -> torch.Tensor:
    """The transpose of avgpool_fwd for an input plane hw = (H, W): gy * 4^-scale on every pixel of a window, zero where the floor drops."""
    scale, (n, c, ho, wo) = _pool_args(gy, scale, "avgpool_bwd")
    h, w = (int(v) for v in hw)
    if (h >> scale, w >> scale) != (ho, wo):
        raise ValueError(f"avgpool_bwd: a {h}x{w} plane pools to {h >> scale}x{w >> scale} at scale {scale}, the gradient is {ho}x{wo}")
    gx = empty_nhwc(n, c, h, w, gy.device)
    call("ctl_avgpool_bwd", ptr(gy), n, h, w, c, scale, ptr(gx), stream_ptr())
    return gx


# ---------------------------------------------------------------------------------------------- image-similarity (reconstruction) losses
def _recon_args(x, t, kinds, mask, beta, win, reduction, who):
    """(kind bits, weights, mask as uint8, t's batch, n, h, w, c, reduce_sum) of a {name: weight} mapping `kinds`; names, weights and
    parameters are checked before the tensors are looked at."""
    check_names(kinds, RECON_KINDS, "image-similarity loss")
    check_recon_params(kinds, beta, win, reduction, device=True)
    bits, weights = _kind_bits(kinds, RECON_KINDS)
    require_gpu(x, t, mask)
    if x.dim() != 4 or t.dim() != 4 or x.dtype != torch.float32 or t.dtype != torch.float32 or tuple(t.shape[1:]) != tuple(x.shape[1:]) \
            or t.shape[0] not in (1, x.shape[0]):
        raise ValueError(f"{who}: expected an fp32 prediction [B,C,H,W] and an fp32 target of that shape or [1,C,H,W]")
    _nhwc_f32(who, "prediction and target must be NHWC in memory (channels_last)", x, t)
    n, c, h, w = (int(v) for v in x.shape)
    check_image(kinds, x.shape, win)
    check_mask(mask, x.shape)
    return bits, weights, mask_u8(mask), int(t.shape[0]), n, h, w, c, int(reduction == "sum")


def recon_loss_fwd(x, t, kinds, mask=None, beta=1.0 / 9, win=9, zero_mean=True, reduction="mean"):
    """(loss, terms, ws) of the {name: weight} mapping `kinds` (RECON_KINDS) between the prediction x and the constant target t ([B,C,H,W]
    or [1,C,H,W]): the 0-d weighted total, fp32 terms[5] in the order of RECON_KINDS (0 for a name that is not in `kinds`), and the
    scratch recon_loss_bwd reads.  `mask`: [B,1,H,W] or [B,H,W], any dtype, nonzero = 1 (a contiguous uint8 mask is used as it is)."""
    bits, weights, mask, tb, n, h, w, c, rsum = _recon_args(x, t, kinds, mask, beta, win, reduction, "recon_loss_fwd")
    ws, loss = _kinds_scratch("ctl_recon_ws_doubles", (bits, n, h, w, c, int(win)), RECON_KINDS, x.device)
    call("ctl_recon_loss_fwd", bits, weights, ptr(x), ptr(t), ptr(mask), tb, n, h, w, c, float(beta), int(win), int(bool(zero_mean)), rsum,
         ptr(ws), ptr(loss), stream_ptr())
    return loss[0], loss[1:], ws


def recon_loss_bwd(x, t, kinds, gout, ws, mask=None, beta=1.0 / 9, win=9, zero_mean=True, reduction="mean"):
    """gout (0-d fp32 device tensor) * d total / d x; `ws` is what recon_loss_fwd returned for the same arguments."""
    bits, weights, mask, tb, n, h, w, c, rsum = _recon_args(x, t, kinds, mask, beta, win, reduction, "recon_loss_bwd")
    _scratch_given(ws, gout, "ctl_recon_ws_doubles", (bits, n, h, w, c, int(win)), "recon_loss_bwd", "recon_loss_fwd")
    d = torch.empty_like(x)
    call("ctl_recon_loss_bwd", bits, weights, ptr(x), ptr(t), ptr(mask), tb, ptr(gout), ptr(ws), n, h, w, c, float(beta), int(win),
         int(bool(zero_mean)), rsum, ptr(d), stream_ptr())
    return d


# ---------------------------------------------------------------------------------------------- adversarial input augmentation
ADV_NORMS = {"l2": _ffi.ADV_L2, "rms": _ffi.ADV_RMS, "linf": _ffi.ADV_LINF}      # names of adversarial.unit_scale_host -> CTL_ADV_*


def adv_bias_grid(h: int, w: int, spacing: int):
    """(gh, gw) of the control grid of an h x w plane at integer spacing >= 2: (h - 1) // s + 4, (w - 1) // s + 4."""
    from .adversarial import bias_grid
    return bias_grid(h, w, spacing)


def _adv_bias_args(x, theta, spacing, who):
    """(n, h, w, c, s, gh, gw) of an fp32 image [N,C,H,W] (NHWC in memory) and its fp32 control grid [N,gh,gw]"""
    adv_bias_grid(1, 1, spacing)                     # the spacing is checked before the tensors are looked at
    require_gpu(x, theta)
    if x.dim() != 4 or x.dtype != torch.float32 or not x.permute(0, 2, 3, 1).is_contiguous():
        raise ValueError(f"{who}: expected an fp32 image [N,C,H,W] that is NHWC in memory (channels_last)")
    n, c, h, w = (int(v) for v in x.shape)
    gh, gw = adv_bias_grid(h, w, spacing)
    _arg(theta, torch.float32, (n, gh, gw), who, "theta", dense=True)
    return n, h, w, c, int(spacing), gh, gw


def adv_bias_fwd(x, theta, spacing, with_field=False):
    """x * exp(S(theta)) with S the cubic B-spline field of the control grid `theta` [N,gh,gw] (log space, adv_bias_grid); one launch.
    with_field: (x', f) with the field f [N,H,W] as well."""
    n, h, w, c, s, gh, gw = _adv_bias_args(x, theta, spacing, "adv_bias_fwd")
    y = torch.empty_like(x)
    f = torch.empty((n, h, w), dtype=torch.float32, device=x.device) if with_field else None
    call("ctl_adv_bias_fwd", ptr(x), ptr(theta), n, h, w, c, s, gh, gw, ptr(y), ptr(f), stream_ptr())
    return (y, f) if with_field else y


def adv_bias_bwd(g, x, theta, spacing, need_dx=True):
    """(dtheta [N,gh,gw], dx or None) of adv_bias_fwd for the gradient g at its output; two launches."""
    n, h, w, c, s, gh, gw = _adv_bias_args(x, theta, spacing, "adv_bias_bwd")
    require_gpu(g)
    if g.dtype != torch.float32 or tuple(g.shape) != tuple(x.shape) or not g.permute(0, 2, 3, 1).is_contiguous():
        raise ValueError("adv_bias_bwd: the gradient must be an fp32 tensor of the image's shape, NHWC in memory")
    ws, _ = _workspace("ctl_adv_bias_ws_bytes", n, h, w, s, device=x.device)
    dtheta = torch.empty_like(theta)
    dx = torch.empty_like(x) if need_dx else None
    call("ctl_adv_bias_bwd", ptr(g), ptr(x), ptr(theta), n, h, w, c, s, gh, gw, ptr(ws), ws.numel(), ptr(dtheta), ptr(dx), stream_ptr())
    return dtheta, dx


def adv_unit_scale(g, scale, norm="l2"):
    """Per sample (the first axis) scale * g / norm(g), norm one of ADV_NORMS; a sample whose norm is 0 or not finite gives zeros.  Two
    launches; the result keeps g's shape and memory format."""
    if norm not in ADV_NORMS:
        raise ValueError(f"adv_unit_scale: norm {norm!r} (one of {', '.join(ADV_NORMS)})")
    require_gpu(g)
    dense = g.is_contiguous() or (g.dim() == 4 and g.is_contiguous(memory_format=torch.channels_last))
    if g.dtype != torch.float32 or g.dim() < 1 or g.numel() == 0 or not dense:
        raise ValueError(f"adv_unit_scale: expected a dense, non-empty fp32 tensor with the samples on the first axis, got {g.dtype} {tuple(g.shape)}")
    n = int(g.shape[0])
    m = g.numel() // n
    ws, _ = _workspace("ctl_adv_unit_scale_ws_bytes", n, m, device=g.device)
    out = torch.empty_like(g)
    call("ctl_adv_unit_scale", ptr(g), n, m, ADV_NORMS[norm], float(scale), ptr(ws), ws.numel(), ptr(out), stream_ptr())
    return out


def mse_fwd(a, b, scale):
    partial = torch.empty(_ffi.RED_BLOCKS, dtype=torch.float64, device=a.device)
    loss = torch.empty((), dtype=torch.float32, device=a.device)
    call("ctl_mse_fwd", ptr(a), ptr(b), a.numel(), scale, ptr(partial), ptr(loss), stream_ptr())
    return loss


def mse_bwd(a, b, gout, scale):
    d = torch.empty_like(a)
    call("ctl_mse_bwd", ptr(a), ptr(b), ptr(gout), a.numel(), scale, ptr(d), stream_ptr())
    return d


def argmax_c(logit: torch.Tensor) -> torch.Tensor:
    require_gpu(logit)
    logit = as_nhwc(logit)
    n, c, h, w = logit.shape
    out = torch.empty((n, h, w), dtype=torch.uint8, device=logit.device)
    call("ctl_argmax_c", ptr(logit), ptr(out), n * h * w, c, stream_ptr())
    return out


# ---------------------------------------------------------------------------------------------- predictive uncertainty
PredictiveStats = namedtuple("PredictiveStats", "entropy mi conf pred mean_prob stats bins")      # maps that were not asked for are None
UNCERT_MAPS = PredictiveStats._fields[:5]


def predictive_stats(logits: torch.Tensor, label: Optional[torch.Tensor] = None, members: int = 1, n_bins: int = 15, eps: float = 1e-7,
                     is_prob: bool = False, want=("entropy",)) -> PredictiveStats:
    """Uncertainty maps and calibration tables of an ensemble of `members` predictions (include/ctl_hip.h "predictive uncertainty"; the
    float64 statement is uncertainty.predictive_stats_host).  logits: fp32 device tensor [members * n, C, H, W], member-major, C <= 16
    (is_prob: probabilities, the softmax is skipped); label: int64 device tensor [n, H, W] or None, a value outside 0..C-1 = unlabelled.
    want: which of 'entropy', 'mi', 'conf' (fp32 [n,H,W]; entropies in bits), 'pred' (uint8 [n,H,W]) and 'mean_prob' (fp32 [n,C,H,W],
    channels_last) to write.  Always returned: stats, fp64 [n,6] = per slice (labelled pixels, correct, sum H, sum MI, sum nll, sum brier)
    and bins, int64 [n,n_bins,3] = per slice and reliability bin (labelled pixels, correct, sum of conf * 2^32); uncertainty.
    calibration_from_tables finishes ECE / NLL / Brier from them on the host.  2 launches, no readback, the same bits on every call."""
    who = "predictive_stats"
    want = (want,) if isinstance(want, str) else tuple(want)
    unknown = [m for m in want if m not in UNCERT_MAPS]
    if unknown:
        raise ValueError(f"{who}: unknown map {unknown[0]!r} (one of {', '.join(UNCERT_MAPS)})")
    require_gpu(logits, label)
    _arg(logits, torch.float32, (None, None, None, None), who, "logits")
    tn, c, h, w = (int(v) for v in logits.shape)
    t = int(members)
    if t < 1 or tn % t:
        raise ValueError(f"{who}: {tn} logit slices do not divide into {members} members")
    n = tn // t
    if label is not None:
        _arg(label, torch.int64, (n, h, w), who, "label", dense=True)
    x, dev = as_nhwc(logits), logits.device
    outs = {m: None for m in UNCERT_MAPS}
    for m in want:
        outs[m] = (empty_nhwc(n, c, h, w, dev) if m == "mean_prob" else
                   torch.empty((n, h, w), dtype=torch.uint8 if m == "pred" else torch.float32, device=dev))
    stats = torch.empty((n, 6), dtype=torch.float64, device=dev)
    bins = torch.empty((n, max(int(n_bins), 1), 3), dtype=torch.int64, device=dev)
    ws, _ = _workspace("ctl_predictive_stats_ws_bytes", t, n, h * w, c, int(n_bins), device=dev, floor=8)      # 0 bytes: the call names the reason
    call("ctl_predictive_stats", ptr(x), ptr(label), t, n, h * w, c, int(n_bins), float(eps), int(bool(is_prob)), *[ptr(outs[m]) for m in UNCERT_MAPS],
         ptr(stats), ptr(bins), ptr(ws), stream_ptr())
    return PredictiveStats(stats=stats, bins=bins, **outs)


# ---------------------------------------------------------------------------------------------- test-time augmentation
TtaMerge = namedtuple("TtaMerge", "aligned merged pred")      # outputs that were not asked for are None
TTA_MODES = {"logit": _ffi.TTA_LOGIT, "prob": _ffi.TTA_PROB}


def _tta_codes(views, h: int, w: int):
    """(codes, the int32 host array ctl_tta_* reads) of a view set for an h x w plane (tta.parse_views: ValueError)"""
    from .tta import parse_views
    codes = parse_views(views, (h, w))
    return codes, (C.c_int32 * len(codes))(*codes)


def tta_views(image: torch.Tensor, views) -> torch.Tensor:
    """The D4 views of a device batch (include/ctl_hip.h "test-time augmentation"; the numpy statement is tta.views_host).  image: fp32
    [n, c, H, W], c <= 4; views: "flips", "d4" or a tuple of distinct codes 0..7 (bit 0 transpose, bit 1 flip H, bit 2 flip W, in that
    order) -> fp32 [T * n, c, H, W] (channels_last), member-major: rows t * n .. t * n + n - 1 are view views[t] of every slice.  A
    transposing code needs H == W (ValueError), so every member has the input's extent.  One launch, no readback."""
    who = "tta_views"
    require_gpu(image)
    _arg(image, torch.float32, (None, None, None, None), who, "image")
    n, c, h, w = (int(v) for v in image.shape)
    codes, arr = _tta_codes(views, h, w)
    x = as_nhwc(image)
    out = empty_nhwc(len(codes) * n, c, h, w, image.device)
    call("ctl_tta_views", ptr(x), n, h, w, c, arr, len(codes), ptr(out), stream_ptr())
    return out


def tta_merge(logits: torch.Tensor, views, hw, mode: str = "prob", want=("merged",)) -> TtaMerge:
    """The network's logits on the views of tta_views, back on the native grid (the numpy statement is tta.merge_host).  logits: fp32
    [T * n, C, H, W], member-major, C <= 16; views as in tta_views; hw: the native (H, W).  want: any of
      'aligned'  fp32 [T * n, C, H, W] (channels_last): every member on the native grid, what predictive_stats(members=T) reads;
      'merged'   fp32 [n, C, H, W] (channels_last): mode "logit" -> the fp32 mean of the members' logits, added in member order;
                 mode "prob" -> the mean of the members' softmax, the arithmetic of predictive_stats' mean_prob;
      'pred'     uint8 [n, H, W]: the arg-max of merged, first maximum.
    -> TtaMerge(aligned, merged, pred), None for what was not asked for.  One launch, no readback, the same bits on every call."""
    who = "tta_merge"
    want = (want,) if isinstance(want, str) else tuple(want)
    unknown = [m for m in want if m not in TtaMerge._fields]
    if unknown or not want:
        raise ValueError(f"{who}: want {want!r}: at least one of {', '.join(TtaMerge._fields)}")
    if mode not in TTA_MODES:
        raise ValueError(f"{who}: mode {mode!r}, one of {sorted(TTA_MODES)}")
    require_gpu(logits)
    h, w = (int(v) for v in hw)
    _arg(logits, torch.float32, (None, None, h, w), who, "logits")
    tn, c = int(logits.shape[0]), int(logits.shape[1])
    codes, arr = _tta_codes(views, h, w)
    t = len(codes)
    if tn % t:
        raise ValueError(f"{who}: {tn} logit slices do not divide into {t} views")
    n, dev = tn // t, logits.device
    x = as_nhwc(logits)
    outs = {"aligned": empty_nhwc(tn, c, h, w, dev) if "aligned" in want else None,
            "merged": empty_nhwc(n, c, h, w, dev) if "merged" in want else None,
            "pred": torch.empty((n, h, w), dtype=torch.uint8, device=dev) if "pred" in want else None}
    call("ctl_tta_merge", ptr(x), t, n, h, w, c, arr, TTA_MODES[mode], ptr(outs["aligned"]), ptr(outs["merged"]), ptr(outs["pred"]), stream_ptr())
    return TtaMerge(**outs)


# ---------------------------------------------------------------------------------------------- latent masking
def latent_score(grad: torch.Tensor, mode: int) -> torch.Tensor:
    """mode 0: [N,C] signed mean over H*W; mode 1: [N,H*W] signed mean over C (model_util.py:224-225 / 285-286)."""
    require_gpu(grad)
    grad = as_nhwc(grad)
    n, c, h, w = grad.shape
    L = c if mode == 0 else h * w
    score = torch.empty((n, L), dtype=torch.float32, device=grad.device)
    scratch, _ = _workspace("ctl_latent_score_ws_floats", mode, n, h * w, c, device=grad.device, dtype=torch.float32)
    call("ctl_latent_score", mode, ptr(grad), ptr(score), ptr(scratch), n, h * w, c, stream_ptr())
    return score


def latent_mask_apply(code: torch.Tensor, score: torch.Tensor, mode: int, k, soft_noise: Optional[torch.Tensor] = None):
    """Returns (masked code [N,C,H,W], mask [N,C,1,1] or [N,1,H,W]).  `k` is an int or a 1-element int32 device tensor."""
    require_gpu(code, score)
    code = as_nhwc(code)
    n, c, h, w = code.shape
    masked = torch.empty_like(code)
    L = c if mode == 0 else h * w
    mask = torch.empty((n, L), dtype=torch.float32, device=code.device)
    k_dev = k if isinstance(k, torch.Tensor) else None
    k_host = 0 if k_dev is not None else int(k)
    if soft_noise is not None:
        soft_noise = soft_noise.reshape(n, L).float().contiguous()
    ws = lib.ctl_latent_mask_apply_ws_floats(mode, n, h * w, c)
    scratch = torch.empty(ws, dtype=torch.float32, device=code.device) if ws else None
    call("ctl_latent_mask_apply", mode, ptr(code), ptr(score), ptr(soft_noise), k_host, ptr(k_dev), ptr(masked), ptr(mask),
         ptr(scratch), n, h * w, c, stream_ptr())
    return masked, (mask.view(n, c, 1, 1) if mode == 0 else mask.view(n, 1, h, w))


def latent_mask(grad: torch.Tensor, code: torch.Tensor, mode: int, k, soft_noise: Optional[torch.Tensor] = None, want_score: bool = False):
    """The generator tail behind one call (`ctl_latent_mask_fused`): signed-mean score of `grad`, rank-select of the top-k entries
    (strict '>', exact under ties), masked = code * mask; ONE launch at latent-code sizes.  Returns (masked, mask[, score]); mask is
    [N,C,1,1] (mode 0) or [N,1,H,W] (mode 1).  `k`: int or 1-element int32 device tensor (graph replay)."""
    require_gpu(grad, code)
    grad, code = as_nhwc(grad), as_nhwc(code)
    n, c, h, w = code.shape
    if grad.shape != code.shape:
        raise ValueError("latent_mask: grad and code must have the same shape")
    L = c if mode == 0 else h * w
    masked = torch.empty_like(code)
    mask = torch.empty((n, L), dtype=torch.float32, device=code.device)
    score = torch.empty((n, L), dtype=torch.float32, device=code.device) if want_score else None
    k_dev = k if isinstance(k, torch.Tensor) else None
    k_host = 0 if k_dev is not None else int(k)
    if soft_noise is not None:
        soft_noise = soft_noise.reshape(n, L).float().contiguous()
    need = lib.ctl_latent_mask_fused_ws_floats(mode, n, h * w, c)
    ws = torch.empty(need, dtype=torch.float32, device=code.device) if need else None
    call("ctl_latent_mask_fused", mode, ptr(grad), ptr(code), ptr(soft_noise), k_host, ptr(k_dev), ptr(masked), ptr(mask), ptr(score),
         ptr(ws), n, h * w, c, stream_ptr())
    mask = mask.view(n, c, 1, 1) if mode == 0 else mask.view(n, 1, h, w)
    return (masked, mask, score) if want_score else (masked, mask)


def dropout2d(z: torch.Tensor, p: float, keep: Optional[torch.Tensor] = None, seed: int = 0, state: Optional[torch.Tensor] = None,
              want_mask: bool = False):
    """Returns (out, keep[N,C]) or, with want_mask, (out, keep, mask) where mask is upstream's full-size equality mask
    (model.py:334-336).  keep=None draws the Bernoulli pattern on device from `seed`; with `state` (device int64[3], see
    ctl_step_tick) `seed` is a call-site salt and nothing step-dependent is baked into the launch (HIP-graph replay)."""
    require_gpu(z)
    z = as_nhwc(z)
    n, c, h, w = z.shape
    out = torch.empty_like(z)
    keep_out = torch.empty((n, c), dtype=torch.float32, device=z.device)
    mask = torch.empty_like(z) if want_mask else None
    if keep is not None:
        keep = keep.reshape(n, c).float().contiguous()
    call("ctl_dropout2d_ex", ptr(z), ptr(keep), seed & (2 ** 64 - 1), ptr(state), p, ptr(out), ptr(keep_out), ptr(mask), n, h * w, c, stream_ptr())
    return (out, keep_out, mask) if want_mask else (out, keep_out)


def uniform(shape, device, seed: int, state: Optional[torch.Tensor] = None) -> torch.Tensor:
    out = torch.empty(shape, dtype=torch.float32, device=device)
    if state is not None:
        call("ctl_uniform_dev", ptr(out), out.numel(), seed & (2 ** 64 - 1), ptr(state), stream_ptr())
    else:
        call("ctl_uniform", ptr(out), out.numel(), seed & (2 ** 64 - 1), stream_ptr())
    return out


def step_tick(state: torch.Tensor) -> None:
    """Advance the device-resident step state (RNG counter, Adam step): one launch at the head of a graph-replayed step."""
    require_gpu(state)
    assert state.dtype == torch.int64 and state.numel() >= 3
    call("ctl_step_tick", ptr(state), stream_ptr())


def adam_step(p, g, m, v, lr, beta1, beta2, eps, step, grad_scale=1.0, state: Optional[torch.Tensor] = None):
    require_gpu(p, g, m, v)
    if state is not None:       # step count read from state[2] on the device
        call("ctl_adam_dev", ptr(p), ptr(g), ptr(m), ptr(v), p.numel(), lr, beta1, beta2, eps, ptr(state), grad_scale, stream_ptr())
    else:
        call("ctl_adam", ptr(p), ptr(g), ptr(m), ptr(v), p.numel(), lr, beta1, beta2, eps, step, grad_scale, stream_ptr())


# ---------------------------------------------------------------------------------------------- optimizer tail (ctl_optim.hip)
def _ctrl_arg(ctrl: torch.Tensor, who: str) -> None:
    _arg(ctrl, torch.float64, (_ffi.OPTIM_CTRL_DOUBLES,), who, "ctrl", dense=True, on_device=True)


def optim_ctrl(device) -> torch.Tensor:
    """A zeroed control record (ctl_hip.h, "optimizer tail") with clip = finite = 1: neutral until optim_control / grad_norm write it."""
    ctrl = torch.zeros(_ffi.OPTIM_CTRL_DOUBLES, dtype=torch.float64, device=device)
    ctrl[_ffi.OPTIM_CLIP:_ffi.OPTIM_FINITE + 1] = 1.0
    return ctrl


def optim_control(ctrl: torch.Tensor, lrs, max_norm: float = 0.0, skip_nonfinite: bool = False, ema_omd: float = 0.0) -> None:
    """Write the host fields of the control record: ONE launch, the values travel as launch arguments (graph.py: a replay may be
    queued far ahead of the device, so they must not sit in host memory that the next step overwrites)."""
    _ctrl_arg(ctrl, "optim_control")
    lrs = [float(v) for v in lrs]
    if not 1 <= len(lrs) <= _ffi.OPTIM_MAX_NETS:
        raise ValueError(f"optim_control: 1 to {_ffi.OPTIM_MAX_NETS} learning rates, got {len(lrs)}")
    arr = (C.c_float * len(lrs))(*lrs)
    call("ctl_optim_control", ptr(ctrl), len(lrs), C.cast(arr, C.c_void_p), float(max_norm), int(bool(skip_nonfinite)), float(ema_omd), stream_ptr())


def grad_norm_work(counts) -> int:
    """Doubles of workspace grad_norm needs for flat buffers of these sizes."""
    arr = (C.c_int64 * len(counts))(*[int(c) for c in counts])
    size = lib.ctl_grad_norm_work(C.cast(arr, C.c_void_p), len(counts))
    if size == 0:
        raise ValueError(f"grad_norm_work: 1 to {_ffi.OPTIM_MAX_NETS} positive counts, got {list(counts)}")
    return size


def grad_norm(grads, grad_scale: float, ctrl: torch.Tensor, work: Optional[torch.Tensor] = None) -> torch.Tensor:
    """Global norm of the flat fp32 gradient buffers `grads` (1 to 8) into the control record: sumsq, norm, clip, finite, skipped.
    Two launches, no readback.  Returns the workspace (pass it back in to reuse it)."""
    _ctrl_arg(ctrl, "grad_norm")
    grads = list(grads)
    if not 1 <= len(grads) <= _ffi.OPTIM_MAX_NETS:
        raise ValueError(f"grad_norm: 1 to {_ffi.OPTIM_MAX_NETS} gradient buffers, got {len(grads)}")
    for j, g in enumerate(grads):
        _arg(g, torch.float32, (None,), "grad_norm", f"grads[{j}]", dense=True, on_device=True)
    counts = [g.numel() for g in grads]
    need = grad_norm_work(counts)
    if work is None:
        work = torch.empty(need, dtype=torch.float64, device=ctrl.device)
    else:
        _arg(work, torch.float64, (None,), "grad_norm", "work", dense=True, on_device=True)
        if work.numel() < need:
            raise ValueError(f"grad_norm: work holds {work.numel()} doubles, {need} needed")
    ptrs = (C.c_void_p * len(grads))(*[g.data_ptr() for g in grads])
    cnts = (C.c_int64 * len(grads))(*counts)
    call("ctl_grad_norm", C.cast(ptrs, C.c_void_p), C.cast(cnts, C.c_void_p), len(grads), float(grad_scale), ptr(work), ptr(ctrl), stream_ptr())
    return work


def adam_tail(p, g, m, v, ema: Optional[torch.Tensor], beta1, beta2, eps, step, grad_scale, ctrl: torch.Tensor, net: int,
              state: Optional[torch.Tensor] = None) -> None:
    """ctl_adam / ctl_adam_dev with lr, clip factor and skip decision read from the control record, and the EMA shadow `ema` (or None)
    updated in the same pass."""
    _ctrl_arg(ctrl, "adam_tail")
    for name, t in (("p", p), ("g", g), ("m", m), ("v", v)) + ((("ema", ema),) if ema is not None else ()):
        _arg(t, torch.float32, (p.numel(),), "adam_tail", name, dense=True, on_device=True)
    if not 0 <= int(net) < _ffi.OPTIM_MAX_NETS:
        raise ValueError(f"adam_tail: net must lie in 0..{_ffi.OPTIM_MAX_NETS - 1}, got {net}")
    call("ctl_adam_tail", ptr(p), ptr(g), ptr(m), ptr(v), ptr(ema), p.numel(), beta1, beta2, eps, ptr(state), int(step), grad_scale,
         ptr(ctrl), int(net), stream_ptr())


# ---------------------------------------------------------------------------------------------- metrics + input pipeline
def confusion_hist(label_true: torch.Tensor, label_pred: torch.Tensor, n_class: int, hist: Optional[torch.Tensor] = None) -> torch.Tensor:
    """Accumulate `runningScore._fast_hist` (metrics.py:18-23) into `hist` (int64 [n_class, n_class], created zeroed if None)."""
    require_gpu(label_true, label_pred)
    lt = label_true.long().contiguous()
    lp = label_pred.to(torch.uint8).contiguous()
    if lt.numel() != lp.numel():
        raise ValueError("confusion_hist: label_true and label_pred differ in size")
    if hist is None:
        hist = torch.zeros((n_class, n_class), dtype=torch.int64, device=lt.device)
    call("ctl_confusion_hist", ptr(lt), ptr(lp), lt.numel(), n_class, ptr(hist), stream_ptr())
    return hist


def _surface_mode(mode) -> int:
    m = {2: 2, 3: 3, "2d": 2, "3d": 3, "2D": 2, "3D": 3}.get(mode)
    if m is None:
        raise ValueError(f"surface mode {mode!r}: '2d' (every slice on its own) or '3d' (the whole volume)")
    return m


def _surface_sampling(sampling, ndim: int):
    """None, a scalar or `ndim` values in array-axis order -> a host array of `ndim` doubles (or None = unit sampling)."""
    if sampling is None:
        return None
    s = np.ascontiguousarray(np.broadcast_to(np.asarray(sampling, dtype=np.float64), (ndim,)))
    return (C.c_double * ndim)(*s.tolist())


def surface_stats(pred: torch.Tensor, gt: torch.Tensor, n_class: int, sampling=None, connectivity: int = 1, mode="3d",
                  foreground_only: bool = False) -> torch.Tensor:
    """Surface-distance statistics of every foreground class and both directions of one patient (measure.py:333-548, 1096-1128 on
    device): pred / gt are [D,H,W] label volumes.  -> fp64 device table [classes, 2, D if mode == '2d' else 1, 4]; entry [c - 1, side]
    takes the exact Euclidean distance map of the surface of side's mask (0 = pred, 1 = gt) and samples it at the surface voxels of the
    other side's mask: (max d^2, sum of d, number of sampled voxels, 1.0 if either mask is empty).  4 ('2d') or 5 ('3d') launches."""
    require_gpu(pred, gt)
    mode = _surface_mode(mode)
    if pred.dim() != 3 or tuple(pred.shape) != tuple(gt.shape):
        raise ValueError(f"surface_stats: expected two [D,H,W] volumes of one shape, got {tuple(pred.shape)} and {tuple(gt.shape)}")
    p, g = pred.to(torch.uint8).contiguous(), gt.long().contiguous()
    d, h, w = (int(v) for v in p.shape)
    samp = _surface_sampling(sampling, mode)
    rows = lib.ctl_surface_stats_rows(d, n_class, int(foreground_only), mode)
    if rows < 0:
        _ffi.check(rows, "ctl_surface_stats_rows")
    table = torch.empty((rows, 4), dtype=torch.float64, device=p.device)
    ws, nbytes = _workspace("ctl_surface_stats_ws_bytes", d, h, w, n_class, int(foreground_only), mode, device=p.device)
    call("ctl_surface_stats", ptr(p), ptr(g), d, h, w, n_class, int(foreground_only), mode, int(connectivity), samp, ptr(table), ptr(ws),
         nbytes, stream_ptr())
    return table.view(-1, 2, d if mode == 2 else 1, 4)


def surface_quantiles(pred: torch.Tensor, gt: torch.Tensor, n_class: int, q=(95.0,), sampling=None, connectivity: int = 1, mode="3d",
                      foreground_only: bool = False, want_stats: bool = False):
    """Order statistics of the pooled surface distances (both directions in one list) of every foreground class of one patient: what
    `metrics.hd95` / `surface_distance_percentile` need.  `q`: 1 to 4 percentages in [0, 100].  -> fp64 device table
    [classes, D if mode == '2d' else 1, len(q), 4]; with n pooled distances and k = floor((n - 1) * q / 100) an entry is (d^2 of rank k,
    d^2 of rank min(k + 1, n - 1), n, 1.0 if either mask is empty); an entry with the flag set is (inf, inf, 0, 1).
    `metrics._percentile_from_ranks` finishes numpy's percentile from it.  want_stats: -> (that table, the table `surface_stats` returns
    for the same arguments, same bits) from the same launches.  3 launches more than `surface_stats`."""
    require_gpu(pred, gt)
    mode = _surface_mode(mode)
    if pred.dim() != 3 or tuple(pred.shape) != tuple(gt.shape):
        raise ValueError(f"surface_quantiles: expected two [D,H,W] volumes of one shape, got {tuple(pred.shape)} and {tuple(gt.shape)}")
    qs = [float(v) for v in np.atleast_1d(np.asarray(q, dtype=np.float64))]
    p, g = pred.to(torch.uint8).contiguous(), gt.long().contiguous()
    d, h, w = (int(v) for v in p.shape)
    samp = _surface_sampling(sampling, mode)
    ws, nbytes = _workspace("ctl_surface_quantiles_ws_bytes", d, h, w, n_class, int(foreground_only), mode, len(qs), device=p.device)
    rows = lib.ctl_surface_stats_rows(d, n_class, int(foreground_only), mode) if nbytes else 0
    groups = max(rows, 0) // 2
    q_table = torch.empty((groups, max(len(qs), 1), 4), dtype=torch.float64, device=p.device)
    stats = torch.empty((max(rows, 0), 4), dtype=torch.float64, device=p.device) if want_stats else None
    call("ctl_surface_quantiles", ptr(p), ptr(g), d, h, w, n_class, int(foreground_only), mode, int(connectivity), samp,
         (C.c_double * max(len(qs), 1))(*qs), len(qs), ptr(stats) if want_stats else None, ptr(q_table), ptr(ws),
         nbytes, stream_ptr())
    gpm = d if mode == 2 else 1
    q_table = q_table.view(-1, gpm, len(qs), 4)
    return (q_table, stats.view(-1, 2, gpm, 4)) if want_stats else q_table


def _surface_map(mask: torch.Tensor, sampling, connectivity: int, per_slice: bool, want_d2: bool):
    require_gpu(mask)
    if mask.dim() not in (2, 3) or (per_slice and mask.dim() != 3):
        raise ValueError(f"expected a [H,W] or [D,H,W] mask ([D,H,W] with per_slice), got {tuple(mask.shape)}")
    mode = 2 if (mask.dim() == 2 or per_slice) else 3
    m = (mask != 0).to(torch.uint8).reshape((-1,) + tuple(mask.shape[-2:])).contiguous()
    d, h, w = (int(v) for v in m.shape)
    samp = _surface_sampling(sampling, mode)
    if want_d2:
        out = torch.empty((d, h, w), dtype=torch.float64, device=m.device)
        ws, nbytes = _workspace("ctl_surface_map_ws_bytes", d, h, w, mode, device=m.device)
        call("ctl_surface_map", ptr(m), d, h, w, mode, int(connectivity), samp, ptr(out), None, ptr(ws), nbytes, stream_ptr())
    else:
        out = torch.empty((d, h, w), dtype=torch.uint8, device=m.device)
        call("ctl_surface_map", ptr(m), d, h, w, mode, int(connectivity), samp, None, ptr(out), None, 0, stream_ptr())
        out = out.bool()
    return out.reshape(mask.shape)


def surface_of(mask: torch.Tensor, connectivity: int = 1, per_slice: bool = False) -> torch.Tensor:
    """`metrics._border` on device: mask XOR binary_erosion(mask, generate_binary_structure(ndim, connectivity)) as a bool tensor of
    mask's shape ([H,W] or [D,H,W]; per_slice: every [H,W] slice of a volume on its own)."""
    return _surface_map(mask, None, connectivity, per_slice, False)


def edt_sq(mask: torch.Tensor, sampling=None, connectivity: int = 1, per_slice: bool = False) -> torch.Tensor:
    """fp64 map of the SQUARED exact Euclidean distance of every voxel to the nearest voxel of `surface_of(mask, connectivity)`, i.e.
    distance_transform_edt(~_border(mask), sampling) ** 2 (measure.py:1096-1128); +inf where the mask (of the slice) is empty."""
    return _surface_map(mask, sampling, connectivity, per_slice, True)


def _cc_volume(labelmap: torch.Tensor, per_slice: bool, who: str):
    """A [H,W] or [D,H,W] uint8 device label map -> (contiguous [D,H,W] view, D, H, W, mode)."""
    require_gpu(labelmap)
    if labelmap.dtype != torch.uint8:
        raise TypeError(f"{who}: expected a uint8 label map (what ops.argmax_c writes), got {labelmap.dtype}")
    if labelmap.dim() not in (2, 3):
        raise ValueError(f"{who}: expected a [H,W] or [D,H,W] label map, got {tuple(labelmap.shape)}")
    mode = 2 if (labelmap.dim() == 2 or per_slice) else 3
    m = labelmap.reshape((-1,) + tuple(labelmap.shape[-2:])).contiguous()
    d, h, w = (int(v) for v in m.shape)
    return m, d, h, w, mode


def connected_components(labelmap: torch.Tensor, n_class: int, connectivity: int = 1, per_slice: bool = False) -> torch.Tensor:
    """Connected components of every foreground class of a uint8 label map ([H,W] or [D,H,W]; per_slice: every [H,W] slice of a volume
    on its own) -> int32 tensor of the same shape: for a voxel of class 1 <= c < n_class the smallest C-order linear index (within the
    array, or within its slice with per_slice) of any voxel of its component, -1 elsewhere.  connectivity as
    scipy.ndimage.generate_binary_structure(ndim, connectivity).  3 launches, no readback."""
    m, d, h, w, mode = _cc_volume(labelmap, per_slice, "connected_components")
    labels = torch.empty((d, h, w), dtype=torch.int32, device=m.device)
    call("ctl_cc_label", ptr(m), d, h, w, int(n_class), mode, int(connectivity), ptr(labels), stream_ptr())
    return labels.reshape(labelmap.shape)


def keep_largest_components(labelmap: torch.Tensor, n_class: int, connectivity: int = 1, per_slice: bool = False,
                            out: Optional[torch.Tensor] = None, want_table: bool = False):
    """`keep_largest_connected_components` (post_process.py:5-22) on device: the uint8 label map with every voxel set to 0 that is not in
    the largest component of its class (of its slice with per_slice); among components of equal size the one that starts first in C
    order is kept.  `out` (uint8, labelmap's shape, contiguous) may be labelmap itself.  want_table: also the int64 device table
    [groups, n_class - 1, 3] = (components, voxels of the kept one, its label or -1), groups = slices with per_slice else 1.
    5 launches, no readback."""
    m, d, h, w, mode = _cc_volume(labelmap, per_slice, "keep_largest_components")
    out = _out(out, torch.uint8, labelmap.shape, m.device, "keep_largest_components")
    table = torch.empty((d if mode == 2 else 1, int(n_class) - 1, 3), dtype=torch.int64, device=m.device) if want_table else None
    ws, nbytes = _workspace("ctl_cc_ws_bytes", d, h, w, int(n_class), mode, device=m.device)
    call("ctl_cc_keep_largest", ptr(m), d, h, w, int(n_class), mode, int(connectivity), ptr(out), ptr(table), ptr(ws), nbytes, stream_ptr())
    return (out, table) if want_table else out


def _aug_vec(v, n: int, dtype, device, who: str, name: str) -> torch.Tensor:
    """A per-sample parameter: a scalar (broadcast) or n values -> contiguous device tensor [n] of dtype."""
    if not isinstance(v, torch.Tensor):
        v = torch.as_tensor(v)
    if v.dim() == 0:
        v = v.expand(n)
    if v.numel() != n:
        raise ValueError(f"{who}: {name} must be a scalar or hold one value per sample ({n}), got {tuple(v.shape)}")
    return v.reshape(n).to(device=device, dtype=dtype).contiguous()


def _aug_ws(nbytes: int, n: int, hp: int, wp: int, hc: int, wc: int, device, who: str):
    """The workspace of an augmentation entry: (uint8 device tensor, bytes).  Refused shapes (a size query of 0) raise."""
    if nbytes == 0:
        raise ValueError(f"{who}: n={n}, {hp}x{wp} -> {hc}x{wc} is refused: sizes must be positive, planes at most 512x512 and the crop "
                         "no larger than the input")
    return torch.empty(nbytes, dtype=torch.uint8, device=device), nbytes


def aug_elastic_field(n: int, hp: int, wp: int, alpha, sigma, seed, noise: Optional[torch.Tensor] = None, device=None,
                      out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """Elastic displacement of `MyElasticTransform` (elastic_transform.py:41-58) for a batch -> float32 device tensor [n,2,hp,wp]
    (rows, cols) = alpha * gaussian_filter(u, sigma, mode='constant', truncate=4) with u uniform in [-1, 1): `noise` ([n,2,hp,wp]) when
    given, else the counter hash of (seed, sample, axis, pixel).  alpha, sigma, seed: a scalar or one value per sample (host values or
    device tensors; device tensors are read by the kernels, nothing returns to the host).  alpha == 0 gives a zero field.  2 launches."""
    n, hp, wp = int(n), int(hp), int(wp)
    if noise is not None:
        require_gpu(noise)
        _arg(noise, torch.float32, (n, 2, hp, wp), "aug_elastic_field", "noise")
        noise = noise.contiguous()
        device = noise.device
    elif device is None:
        device = next((v.device for v in (alpha, sigma, seed) if isinstance(v, torch.Tensor) and v.is_cuda), torch.device("cuda"))
    ws, nbytes = _aug_ws(lib.ctl_aug_ws_bytes(n, hp, wp), n, hp, wp, 1, 1, device, "aug_elastic_field")
    a = _aug_vec(alpha, n, torch.float32, device, "aug_elastic_field", "alpha")
    s = _aug_vec(sigma, n, torch.float32, device, "aug_elastic_field", "sigma")
    sd = _aug_vec(seed, n, torch.int64, device, "aug_elastic_field", "seed")
    out = _out(out, torch.float32, (n, 2, hp, wp), device, "aug_elastic_field")
    call("ctl_aug_field", ptr(noise), ptr(sd), ptr(a), ptr(s), n, hp, wp, ptr(out), ptr(ws), nbytes, stream_ptr())
    return out


BIAS_FLOATS = 192                    # floats of one sample's record of ctl_aug_bias / ctl_aug_coarse_field (include/ctl_hip.h)
COARSE_FLOATS = 24


def aug_bias_field(image: torch.Tensor, bias: torch.Tensor, seed=None, noise: Optional[torch.Tensor] = None,
                   out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """Bias-field pre-pass of `MyRandomPurtarbationV2` (intensity_transform.py:373-546) for a batch: image float32 [n,1,hp,hp] -> a new
    float32 [n,1,hp,hp] = the image times the clipped bicubic field of each sample's record, min-max normalised, plus eps * N(0, 1) clipped
    to [0, 1] when the record's eps is positive.  bias: float32 device tensor [n,192], the record of include/ctl_hip.h
    (augment.bias_record); N: `noise` (float32 [n,1,hp,hp]) when given, else standard normals from the counter hash of (seed, sample,
    pixel), seed a scalar or one int64 per sample (None = 0).  A sample whose record is off and a black plane are copied bit for bit.
    hp == wp, even, 128..512.  2 launches, no readback."""
    require_gpu(image, bias, noise)
    _arg(image, torch.float32, (None, 1, None, None), "aug_bias_field", "image")
    n, _, hp, wp = (int(v) for v in image.shape)
    if hp != wp or hp % 2 or not 128 <= hp <= 512:
        raise ValueError(f"aug_bias_field: the plane must be square with an even side of 128..512, got {hp}x{wp}")
    _arg(bias, torch.float32, (n, BIAS_FLOATS), "aug_bias_field", "bias")
    if noise is not None:
        _arg(noise, torch.float32, (n, 1, hp, wp), "aug_bias_field", "noise")
        noise = noise.contiguous()
    sd = _aug_vec(0 if seed is None else seed, n, torch.int64, image.device, "aug_bias_field", "seed")
    ws, nbytes = _aug_ws(lib.ctl_aug_bias_ws_bytes(n, hp, wp), n, hp, wp, hp, wp, image.device, "aug_bias_field")
    out = _out(out, torch.float32, (n, 1, hp, wp), image.device, "aug_bias_field")
    call("ctl_aug_bias", ptr(image.contiguous()), ptr(bias.contiguous()), ptr(noise), ptr(sd), n, hp, wp, ptr(out), ptr(ws), nbytes, stream_ptr())
    return out


def aug_coarse_field(n: int, hp: int, wp: int, coarse: torch.Tensor, device=None, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """Displacement of `MyElasticTransformCoarseGrid` (elastic_transform.py:105-172) for a batch -> float32 device tensor [n,2,hp,wp]
    (rows, cols): each sample's two 3x3 planes resized by a cubic spline (scipy.ndimage.zoom(order=3, mode='mirror', grid_mode=True))
    and clipped to their own range.  coarse: float32 [n,24], the record of include/ctl_hip.h (augment.coarse_record: prefiltered
    coefficients, clip bounds, on); a host tensor is uploaded, a device tensor is read by the kernel.  A sample that is off gets zeros.
    hp, wp <= 512.  1 launch."""
    n, hp, wp = int(n), int(hp), int(wp)
    if not isinstance(coarse, torch.Tensor):
        raise ValueError(f"aug_coarse_field: coarse must be a float32 tensor [n,{COARSE_FLOATS}], got {type(coarse)}")
    _arg(coarse, torch.float32, (n, COARSE_FLOATS), "aug_coarse_field", "coarse")
    if n < 1 or n > 65535 or hp < 1 or wp < 1 or hp > 512 or wp > 512:
        raise ValueError(f"aug_coarse_field: n={n}, {hp}x{wp} is refused: sizes must be positive and planes at most 512x512")
    if device is None:
        device = coarse.device if coarse.is_cuda else torch.device("cuda")
    coarse = coarse.to(device).contiguous()
    out = _out(out, torch.float32, (n, 2, hp, wp), device, "aug_coarse_field")
    call("ctl_aug_coarse_field", ptr(coarse), n, hp, wp, ptr(out), stream_ptr())
    return out


def _aug_class_count(n_class, lo: int, who: str) -> int:
    if n_class is None or not lo <= int(n_class) <= 16:
        raise ValueError(f"{who}: n_class must be {lo}..16, got {n_class!r}")
    return int(n_class)


def aug_spline_coeffs(image: torch.Tensor, label: Optional[torch.Tensor] = None, intensity: Optional[torch.Tensor] = None, n_class: int = 0,
                      out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """Cubic B-spline coefficients scipy.ndimage.spline_filter(v, order=3, mode='reflect') of a batch -> float32 [n,1+n_class,hp,wp]:
    plane 0 of image float32 [n,1,hp,wp] through the intensity map (float32 [n,2] = (scale, brightness), clamped to the plane's min / max;
    None = (1, 0)), plane 1 + k of the indicator label == k for k < n_class (label int64 [n,hp,wp]; not read when n_class is 0).  What
    aug_warp(interp="cubic") gathers from.  3 launches, no readback."""
    require_gpu(image, label, intensity)
    _arg(image, torch.float32, (None, 1, None, None), "aug_spline_coeffs", "image")
    n, _, hp, wp = (int(v) for v in image.shape)
    n_class = _aug_class_count(n_class, 0, "aug_spline_coeffs")
    if n_class and (label is None or label.dtype != torch.int64 or tuple(label.shape) != (n, hp, wp)):
        raise ValueError(f"aug_spline_coeffs: n_class={n_class} needs label int64 [n,hp,wp] = {(n, hp, wp)}")
    if intensity is None:
        intensity = torch.zeros((n, 2), dtype=torch.float32, device=image.device)
        intensity[:, 0] = 1.0
    _arg(intensity, torch.float32, (n, 2), "aug_spline_coeffs", "intensity")
    ws, nbytes = _aug_ws(lib.ctl_aug_spline_ws_bytes(n, hp, wp, n_class), n, hp, wp, 1, 1, image.device, "aug_spline_coeffs")
    out = _out(out, torch.float32, (n, 1 + n_class, hp, wp), image.device, "aug_spline_coeffs")
    call("ctl_aug_spline_coeffs", ptr(image.contiguous()), ptr(label.contiguous() if n_class else None), ptr(intensity.contiguous()), n, hp, wp,
         n_class, ptr(out), ptr(ws), nbytes, stream_ptr())
    return out


def aug_warp(image: torch.Tensor, label: torch.Tensor, matrix: torch.Tensor, intensity: torch.Tensor, crop,
             field: Optional[torch.Tensor] = None, out=None, interp: str = "linear", n_class: Optional[int] = None):
    """One resampling of a batch (transform.py:46-82 without the normalisation): image float32 [n,1,hp,wp] and label int64 [n,hp,wp] ->
    (image [n,1,hc,wc], label [n,hc,wc]) for crop = (hc, wc), the centre window of MySpecialCrop.  matrix: float32 [n,2,3], the
    output -> input map about the plane centre in (row, col) order; intensity: float32 [n,2] = (scale, brightness) applied to every tap
    and clamped to the plane's min / max; field: float32 [n,2,hp,wp] from aug_elastic_field, None = no elastic.  Image taps are
    bilinear with zeros outside, label taps nearest.  `out` = (image_out, label_out): contiguous device tensors of the result's shapes
    and dtypes that share no memory with each other or with any input (the gather reads whole input planes).  2 launches, no readback.
    interp="cubic": image and per-class label indicators (label == k for k < n_class, 1 <= n_class <= 16) are read through a cubic
    spline, map_coordinates(order=3, mode='reflect') inside the array and 0 outside it, the label being the largest class at or above
    0.5 (ctl_aug_warp_cubic in include/ctl_hip.h); 4 launches."""
    if interp not in ("linear", "cubic"):
        raise ValueError(f"aug_warp: interp must be 'linear' or 'cubic', got {interp!r}")
    if interp == "cubic":
        n_class = _aug_class_count(n_class, 1, "aug_warp(interp='cubic')")
    require_gpu(image, label, matrix, intensity, field)
    _arg(image, torch.float32, (None, 1, None, None), "aug_warp", "image")
    n, _, hp, wp = (int(v) for v in image.shape)
    _arg(label, torch.int64, (n, hp, wp), "aug_warp", "label")
    _arg(matrix, torch.float32, (n, 2, 3), "aug_warp", "matrix")
    _arg(intensity, torch.float32, (n, 2), "aug_warp", "intensity")
    if field is not None:
        _arg(field, torch.float32, (n, 2, hp, wp), "aug_warp", "field")
    hc, wc = int(crop[0]), int(crop[1])
    ws_bytes = lib.ctl_aug_warp_cubic_ws_bytes(n, hp, wp, hc, wc, n_class) if interp == "cubic" else lib.ctl_aug_warp_ws_bytes(n, hp, wp, hc, wc)
    ws, nbytes = _aug_ws(ws_bytes, n, hp, wp, hc, wc, image.device, "aug_warp")
    io, lo = (None, None) if out is None else out
    io = _out(io, torch.float32, (n, 1, hc, wc), image.device, "aug_warp", "out[0]")
    lo = _out(lo, torch.int64, (n, hc, wc), image.device, "aug_warp", "out[1]")
    image, label, matrix, intensity = image.contiguous(), label.contiguous(), matrix.contiguous(), intensity.contiguous()
    field = None if field is None else field.contiguous()
    if interp == "cubic":
        call("ctl_aug_warp_cubic", ptr(image), ptr(label), ptr(matrix), ptr(intensity), ptr(field), n, hp, wp, hc, wc, n_class, ptr(io), ptr(lo),
             ptr(ws), nbytes, stream_ptr())
        return io, lo
    call("ctl_aug_warp", ptr(image), ptr(label), ptr(matrix), ptr(intensity), ptr(field), n, hp, wp,
         hc, wc, ptr(io), ptr(lo), ptr(ws), nbytes, stream_ptr())
    return io, lo


def rescale_intensity(data: torch.Tensor, new_min: float = 0.0, new_max: float = 1.0, eps: float = 1e-20,
                      out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """basic_operations.py:232-245 on device; data: [N,C,H,W] float32 in plain NCHW memory (each (n,c) plane contiguous).  `out`:
    a contiguous float32 device tensor of data's shape to write into, not data itself."""
    require_gpu(data)
    x = data.float().contiguous()
    n, c, h, w = x.shape
    out = _out(out, torch.float32, x.shape, x.device, "rescale_intensity", not_input=x)
    ws, _ = _workspace("ctl_rescale_intensity_ws_floats", n * c, device=x.device, dtype=torch.float32, floor=0)
    call("ctl_rescale_intensity", ptr(x), ptr(out), ptr(ws), n * c, h * w, new_min, new_max, eps, stream_ptr())
    return out


def noise_clamp(x: torch.Tensor, noise: Optional[torch.Tensor] = None, sigma: float = 0.05, lo: float = 0.0, hi: float = 1.0,
                seed: int = 0) -> torch.Tensor:
    """clamp(x + noise, lo, hi); noise=None draws sigma*N(0,1) on device from `seed` (train...py:185-187)."""
    require_gpu(x)
    x = x.float().contiguous()
    if noise is not None:
        noise = noise.float().contiguous()
        if noise.shape != x.shape:
            raise ValueError("noise_clamp: noise must have the shape of x")
    out = torch.empty_like(x)
    call("ctl_noise_clamp", ptr(x), ptr(noise), seed & (2 ** 64 - 1), sigma, lo, hi, ptr(out), x.numel(), stream_ptr())
    return out


def crop_or_pad(image: torch.Tensor, crop_size, label: Optional[torch.Tensor] = None):
    """basic_operations.py:173-220 for [n,h,w] (or [h,w]) device tensors: (image, label) cropped / zero-padded to crop_size."""
    def one(a):
        require_gpu(a)
        squeeze = a.dim() == 2
        a3 = (a.unsqueeze(0) if squeeze else a).contiguous()
        if a3.dim() != 3 or a3.element_size() not in (1, 4, 8):
            raise ValueError("crop_or_pad: expected a [n,h,w] or [h,w] tensor with 1-, 4- or 8-byte elements")
        n, h, w = a3.shape
        out = torch.empty((n, int(crop_size[0]), int(crop_size[1])), dtype=a3.dtype, device=a3.device)
        call("ctl_crop_or_pad", ptr(a3), ptr(out), a3.element_size(), n, h, w, int(crop_size[0]), int(crop_size[1]), stream_ptr())
        return out[0] if squeeze else out
    return one(image), (None if label is None else one(label))


# ------------------------------------------------------------------------------------------------ volume preparation
def percentile_index(n: int, q: float):
    """np.percentile's 'linear' virtual index for n elements, on the host in fp64: v = (n - 1) * (q / 100) -> (k, k_upper, g) with
    k = floor(v), g = v - k and the upper rank clamped to n - 1."""
    q = float(q)
    if not 0.0 <= q <= 100.0:
        raise ValueError(f"percentile: q = {q} outside [0, 100]")
    v = (int(n) - 1) * (q / 100.0)
    k = int(np.floor(v))
    return k, min(k + 1, int(n) - 1), v - k


def resample_geometry(n: int, h: int, w: int, spacing, new_spacing):
    """The host arithmetic of `resample_by_spacing` (dataset_utils.py:39-63) for a [n,h,w] array: spacing and new_spacing are (x, y, z)
    as SimpleITK orders them, so entry 0 belongs to the WIDTH axis.  -> (new_h, new_w, r_h, r_w, identity): new sizes by numpy's round
    (half to even), r = new_spacing / spacing in fp64, identity = the scalings sum to within 1e-4 of their count (upstream returns the
    input then).  The slice axis is never resampled: new_spacing[2] must be negative, the only form the datasets use."""
    new_spacing, spacing = [float(v) for v in new_spacing], [float(v) for v in spacing]
    if len(spacing) != 3 or len(new_spacing) != 3:
        raise ValueError("resample_inplane: spacing and new_spacing are (x, y, z) triples")
    if new_spacing[2] >= 0:
        raise NotImplementedError("resample_inplane: the slice axis is not resampled here; pass new_spacing[2] < 0 (keep_z_spacing)")
    if min(spacing[:2]) <= 0 or min(new_spacing[:2]) <= 0:
        raise ValueError("resample_inplane: in-plane spacings must be positive")
    scaling = np.array(new_spacing, dtype=np.float64) / (1.0 * np.array(spacing, dtype=np.float64))
    new_size = np.round(np.array([w, h, n]) / scaling).astype("int").tolist()
    scaling[2] = 1
    identity = bool(abs(np.sum(scaling) - len(scaling)) < 1e-4)
    return int(new_size[1]), int(new_size[0]), float(scaling[1]), float(scaling[0]), identity


def _segmented(x: torch.Tensor, segments: int, who: str):
    """A float32 device tensor viewed as `segments` contiguous segments -> (contiguous tensor, segments, elements per segment)."""
    require_gpu(x)
    if x.dtype != torch.float32:
        raise TypeError(f"{who}: expected a float32 tensor, got {x.dtype}")
    segments = int(segments)
    if segments < 1 or x.numel() == 0 or x.numel() % segments:
        raise ValueError(f"{who}: {x.numel()} elements do not split into {segments} equal, non-empty segments")
    return x.contiguous(), segments, x.numel() // segments


def _order_stats(x: torch.Tensor, segments: int, seg_elems: int, ranks) -> torch.Tensor:
    ranks = np.ascontiguousarray(ranks, dtype=np.int64).reshape(-1)
    table = torch.empty((segments, ranks.size), dtype=torch.float32, device=x.device)
    ws, nbytes = _workspace("ctl_order_stats_ws_bytes", segments, int(ranks.size), device=x.device)
    call("ctl_order_stats", ptr(x), segments, seg_elems, ranks.ctypes.data, int(ranks.size), ptr(table), ptr(ws), nbytes, stream_ptr())
    return table


def order_statistics(x: torch.Tensor, ranks, segments: int = 1) -> torch.Tensor:
    """Exact order statistics of a float32 device tensor viewed as `segments` contiguous segments (1: the whole tensor; slices: every
    slice on its own): float32 device tensor [segments, len(ranks)] = the element of each zero-based rank (1 to 8 of them, duplicates and
    any order allowed) in the segment's ascending order, -0.0 before +0.0.  Inputs must be finite: a NaN gives unspecified elements and
    is not checked.  Radix select, integer atomics only: identical bits on every call.  5 launches, no readback."""
    x, segments, seg_elems = _segmented(x, segments, "order_statistics")
    return _order_stats(x, segments, seg_elems, ranks)


def _percentile_table(x: torch.Tensor, segments: int, seg_elems: int, q_lo: float, q_hi: float):
    k0, k0u, g_lo = percentile_index(seg_elems, q_lo)
    k1, k1u, g_hi = percentile_index(seg_elems, q_hi)
    return _order_stats(x, segments, seg_elems, [k0, k0u, k1, k1u]), g_lo, g_hi


def percentile(x: torch.Tensor, q, segments: int = 1) -> torch.Tensor:
    """np.percentile(x.astype(float64), q) ('linear') per segment, rounded once to float32: float32 device tensor [segments, len(q)].
    Exact order statistics, then numpy's _lerp in fp64 on the device.  6 launches per pair of percentiles, no readback."""
    x, segments, seg_elems = _segmented(x, segments, "percentile")
    q = [float(v) for v in np.asarray(q, dtype=np.float64).reshape(-1)]
    if not q:
        raise ValueError("percentile: q is empty")
    out = torch.empty((segments, len(q)), dtype=torch.float32, device=x.device)
    for i in range(0, len(q), 2):
        pair = q[i:i + 2] if i + 1 < len(q) else [q[i], q[i]]
        table, g_lo, g_hi = _percentile_table(x, segments, seg_elems, pair[0], pair[1])
        bounds = torch.empty((segments, 2), dtype=torch.float32, device=x.device)
        call("ctl_percentile_apply", ptr(x), ptr(table), segments, seg_elems, g_lo, g_hi, 0, 0.0, 1.0, None, ptr(bounds), stream_ptr())
        out[:, i:i + 2] = bounds[:, :len(q) - i]
    return out


PERCENTILE_FORMS = {"minmax": 0, "medic": 1}


def percentile_normalize(x: torch.Tensor, q=(2.0, 98.0), form: str = "minmax", segments: int = 1, new_min: float = 0.0,
                         new_max: float = 1.0, out: Optional[torch.Tensor] = None, want_bounds: bool = False):
    """Clip to the (q[0], q[1]) percentiles of each segment and scale, in float32 with one rounding per operation.  form "minmax":
    `normalize_minmax_data` (dataset_utils.py:15-36; upstream: q = (2, 98) over the whole volume), (clip(x) - lo) / ((1e-10 + hi) - lo);
    form "medic": `MyNormalizeMedicPercentile` (intensity_transform.py:216-269; upstream: per slice), clip(x) * a + b with
    a = (new_max - new_min) / ((hi - lo) + 1e-8), b = new_max - a * hi.  lo, hi: np.percentile of the float64 values, rounded to float32.
    `out`: a contiguous float32 device tensor of x's shape, not x itself.  want_bounds: also the device tensor [segments, 2] of lo, hi.
    6 launches, no readback."""
    if form not in PERCENTILE_FORMS:
        raise ValueError(f"percentile_normalize: form {form!r}, one of {sorted(PERCENTILE_FORMS)}")
    shape = x.shape
    x, segments, seg_elems = _segmented(x, segments, "percentile_normalize")
    if len(q) != 2:
        raise ValueError("percentile_normalize: q is a (low, high) pair of percentiles")
    out = _out(out, torch.float32, shape, x.device, "percentile_normalize", not_input=x)
    table, g_lo, g_hi = _percentile_table(x, segments, seg_elems, q[0], q[1])
    bounds = torch.empty((segments, 2), dtype=torch.float32, device=x.device) if want_bounds else None
    call("ctl_percentile_apply", ptr(x), ptr(table), segments, seg_elems, g_lo, g_hi, PERCENTILE_FORMS[form], float(new_min), float(new_max),
         ptr(out), ptr(bounds), stream_ptr())
    return (out, bounds) if want_bounds else out


def resample_inplane(image: torch.Tensor, spacing, new_spacing, label: Optional[torch.Tensor] = None):
    """`resample_by_spacing` with keep_z_spacing (dataset_utils.py:39-63) for device arrays [n,h,w]: image float32 (linear), label uint8
    or int64 (nearest) -> (image, label, spacing_out).  spacing / new_spacing: (x, y, z) as SimpleITK orders them (entry 0 = width);
    new_spacing[2] must be negative (the slice axis stays), anything else raises NotImplementedError.  Output index j reads source
    coordinate j * new_spacing / spacing; 0 where that reaches size - 0.5.  When the scalings sum to within 1e-4 of their count the inputs
    are returned unchanged, as upstream does.  One launch per array, no readback."""
    require_gpu(image)
    _arg(image, torch.float32, (None, None, None), "resample_inplane", "image")
    if label is not None:
        require_gpu(label)
        _arg(label, (torch.uint8, torch.int64), tuple(image.shape), "resample_inplane", "label")
    n, h, w = (int(v) for v in image.shape)
    new_h, new_w, r_h, r_w, identity = resample_geometry(n, h, w, spacing, new_spacing)
    if identity:
        return image, label, tuple(float(v) for v in spacing)
    image = image.contiguous()
    image_out = torch.empty((n, new_h, new_w), dtype=torch.float32, device=image.device)
    label_out = None
    if label is not None:
        label = label.contiguous()
        label_out = torch.empty((n, new_h, new_w), dtype=label.dtype, device=label.device)
    call("ctl_resample_inplane", ptr(image), ptr(label), 0 if label is None else label.element_size(), n, h, w, new_h, new_w, r_h, r_w,
         ptr(image_out), ptr(label_out), stream_ptr())
    return image_out, label_out, (float(new_spacing[0]), float(new_spacing[1]), float(spacing[2]))


# ------------------------------------------------------------------------------------------------ native-grid restoration
RESTORE_MODES = {"logit": 0, "prob": 1}


def _restore_args(geometry, n: int, window, who: str):
    """The scalars of a prepare.Geometry as ctl_restore_* takes them, after checking the window of the input against the record."""
    (h, w), (rh, rw), (hc, wc) = geometry.native_hw, geometry.resampled_hw, geometry.window_hw
    if tuple(int(v) for v in window) != (int(hc), int(wc)):
        raise ValueError(f"{who}: the input's window {tuple(int(v) for v in window)} is not the geometry's {(int(hc), int(wc))}")
    return (int(n), int(hc), int(wc), int(h), int(w), int(rh), int(rw), int(geometry.offset[0]), int(geometry.offset[1]),
            float(geometry.q[0]), float(geometry.q[1]))


def restore_scores(scores: torch.Tensor, geometry, mode: str = "logit", want_soft: bool = False, out: Optional[torch.Tensor] = None):
    """Window-grid class scores [n,C,Hc,Wc] (float32, what `predict` returns; 1 <= C <= 16) -> the uint8 label volume [n,h,w] on the
    native grid of `geometry` (prepare.Geometry), or (label, soft) with want_soft: soft float32 [n,C,h,w], plain contiguous planes.
    Bilinear in fp64 over the logits (mode "logit") or over each pixel's softmax (mode "prob"), arg-max on the fp64 values; outside the
    window or the resampled extent the label is 0 (ctl_restore_scores).  `out`: a contiguous uint8 device tensor [n,h,w], e.g. a slice
    [lo:hi] of a patient's volume.  One launch, no readback."""
    if mode not in RESTORE_MODES:
        raise ValueError(f"restore_scores: mode {mode!r}, one of {sorted(RESTORE_MODES)}")
    if scores.dim() != 4 or scores.dtype != torch.float32:
        raise ValueError(f"restore_scores: expected float32 scores [n,C,Hc,Wc], got {scores.dtype} {tuple(scores.shape)}")
    n, c = int(scores.shape[0]), int(scores.shape[1])
    args = _restore_args(geometry, n, scores.shape[2:], "restore_scores")
    require_gpu(scores, out)
    scores = as_nhwc(scores)
    h, w = args[3], args[4]
    label = _out(out, torch.uint8, (n, h, w), scores.device, "restore_scores")
    soft = torch.empty((n, c, h, w), dtype=torch.float32, device=scores.device) if want_soft else None
    call("ctl_restore_scores", ptr(scores), args[0], c, *args[1:], RESTORE_MODES[mode], ptr(label), ptr(soft), stream_ptr())
    return (label, soft) if want_soft else label


def restore_labels(labels: torch.Tensor, geometry, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """Window-grid uint8 labels [n,Hc,Wc] -> uint8 [n,h,w] on the native grid of `geometry`: the nearest window pixel, 0 outside
    (ctl_restore_labels).  `out` as in restore_scores.  One launch, no readback."""
    if labels.dim() != 3 or labels.dtype != torch.uint8:
        raise ValueError(f"restore_labels: expected uint8 labels [n,Hc,Wc], got {labels.dtype} {tuple(labels.shape)}")
    n = int(labels.shape[0])
    args = _restore_args(geometry, n, labels.shape[1:], "restore_labels")
    require_gpu(labels, out)
    labels = labels.contiguous()
    res = _out(out, torch.uint8, (n, args[3], args[4]), labels.device, "restore_labels")
    call("ctl_restore_labels", ptr(labels), *args, ptr(res), stream_ptr())
    return res


# ------------------------------------------------------------------------------------------------ MR artefact corruption
def _volume(x: torch.Tensor, who: str):
    """A float32 device volume [D,H,W] (a tester pack [D,1,H,W] is viewed as one) -> (contiguous [D,H,W] tensor, d, h, w)."""
    require_gpu(x)
    if x.dim() == 4 and x.shape[1] == 1:
        x = x[:, 0]
    if x.dim() != 3 or x.dtype != torch.float32 or x.numel() == 0:
        raise ValueError(f"{who}: expected a non-empty float32 [D,H,W] volume (or a [D,1,H,W] pack), got {x.dtype} {tuple(x.shape)}")
    x = x.contiguous()
    return (x,) + tuple(int(v) for v in x.shape)


def corrupt_bias_field(x: torch.Tensor, coefficients, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """x * exp(cubic polynomial of the normalised voxel coordinates) in float32 (ctl_corrupt_bias): x [D,H,W], coefficients = 20 host
    numbers in the loop order i, j, k of u^i v^j w^k (rounded to float32).  One launch."""
    x, d, h, w = _volume(x, "corrupt_bias_field")
    coef = np.ascontiguousarray(coefficients, dtype=np.float32).reshape(-1)
    if coef.size != 20:
        raise ValueError(f"corrupt_bias_field: {coef.size} coefficients, 20 expected (i + j + k <= 3)")
    out = _out(out, torch.float32, (d, h, w), x.device, "corrupt_bias_field")
    call("ctl_corrupt_bias", ptr(x), coef.ctypes.data, d, h, w, ptr(out), stream_ptr())
    return out


def corrupt_spike_workspace(shape, n_pairs: int, device) -> torch.Tensor:
    """The workspace of corrupt_spike for a volume shape and a number of wave-vector pairs (needs no initialisation)."""
    nbytes = lib.ctl_corrupt_spike_ws_bytes(int(shape[0]), int(shape[1]), int(shape[2]), int(n_pairs))
    return torch.empty(max(nbytes, 8) // 8, dtype=torch.float64, device=device)


def corrupt_spike(x: torch.Tensor, k, mult, intensity: float, out: Optional[torch.Tensor] = None,
                  workspace: Optional[torch.Tensor] = None) -> torch.Tensor:
    """The image-space form of setting the spectrum entries k[s] and -k[s] of x [D,H,W] to intensity * sum(x) (ctl_corrupt_spike): k = host
    integers [n,3] with 0 <= k < shape, each pair {k, -k} once, mult[s] = 1 where k[s] == -k[s] modulo the shape, else 2.  fp64 on the
    device, rounded once; x should be non-negative (then sum(x) is the peak of the spectrum).  Two launches, no readback."""
    x, d, h, w = _volume(x, "corrupt_spike")
    k = np.ascontiguousarray(k, dtype=np.int32).reshape(-1, 3)
    mult = np.ascontiguousarray(mult, dtype=np.int32).reshape(-1)
    if mult.size != k.shape[0]:
        raise ValueError("corrupt_spike: one multiplicity per wave vector")
    out = _out(out, torch.float32, (d, h, w), x.device, "corrupt_spike")
    ws = corrupt_spike_workspace((d, h, w), k.shape[0], x.device) if workspace is None else workspace
    call("ctl_corrupt_spike", ptr(x), d, h, w, k.ctypes.data, mult.ctypes.data, int(k.shape[0]), float(intensity), ptr(out), ptr(ws),
         ws.numel() * ws.element_size(), stream_ptr())
    return out


def corrupt_rigid3d(x: torch.Tensor, matrices, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """T copies [T,D,H,W] of x [D,H,W], copy t read at M_t p + o_t (matrices: host [T,3,4] in voxel space, rounded to float32), linear over
    the volume extended by zeros, float32 coordinates (ctl_corrupt_rigid3d).  An identity matrix returns x bit for bit.  One launch."""
    x, d, h, w = _volume(x, "corrupt_rigid3d")
    m = np.ascontiguousarray(matrices, dtype=np.float32).reshape(-1, 12)
    out = _out(out, torch.float32, (m.shape[0], d, h, w), x.device, "corrupt_rigid3d")
    call("ctl_corrupt_rigid3d", ptr(x), d, h, w, m.ctypes.data, int(m.shape[0]), ptr(out), stream_ptr())
    return out


def axis_operator(x: torch.Tensor, matrix: torch.Tensor, axis: int, stack: Optional[torch.Tensor] = None,
                  out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """out[r, j] = sum_k matrix[j, k] * volume_(k // L)[r, k % L] along `axis` of x [D,H,W] (L = its size): matrix = float32 DEVICE tensor
    [L, n L], volume 0 = x, volumes 1 .. n - 1 = stack [n - 1, D, H, W] (None: one volume).  float32, terms added in ascending k
    (ctl_axis_operator).  One launch."""
    x, d, h, w = _volume(x, "axis_operator")
    axis = int(axis)
    if axis not in (0, 1, 2):
        raise ValueError(f"axis_operator: axis {axis} (0, 1 or 2)")
    n_vol = 1
    if stack is not None:
        require_gpu(stack)
        if stack.dim() != 4 or tuple(stack.shape[1:]) != (d, h, w) or stack.dtype != torch.float32 or stack.shape[0] < 1:
            raise ValueError(f"axis_operator: expected a float32 stack [T,{d},{h},{w}], got {stack.dtype} {tuple(stack.shape)}")
        stack = stack.contiguous()
        n_vol += int(stack.shape[0])
    length = (d, h, w)[axis]
    require_gpu(matrix)
    _arg(matrix, torch.float32, (length, n_vol * length), "axis_operator", "matrix", dense=True)
    out = _out(out, torch.float32, (d, h, w), x.device, "axis_operator")
    call("ctl_axis_operator", ptr(x), ptr(stack), n_vol, d, h, w, axis, ptr(matrix), ptr(out), stream_ptr())
    return out


# ------------------------------------------------------------------------------------------------ device-resident training set
def _arenas(image_arena: torch.Tensor, label_arena: torch.Tensor, table: torch.Tensor, who: str):
    """The packed slices of a training set: float32 and uint8 arenas of one layout, int64 table [S,3] of (element offset, h, w)."""
    if image_arena is not None and (image_arena.dtype != torch.float32 or image_arena.dim() != 1 or not image_arena.is_contiguous()):
        raise TypeError(f"{who}: the image arena is a flat contiguous float32 tensor, got {image_arena.dtype} {tuple(image_arena.shape)}")
    if label_arena.dtype != torch.uint8 or label_arena.dim() != 1 or not label_arena.is_contiguous():
        raise TypeError(f"{who}: the label arena is a flat contiguous uint8 tensor, got {label_arena.dtype} {tuple(label_arena.shape)}")
    if table.dtype != torch.int64 or table.dim() != 2 or table.shape[1] != 3 or table.shape[0] < 1 or not table.is_contiguous():
        raise TypeError(f"{who}: the slice table is a contiguous int64 tensor [S,3] of (offset, h, w), got {table.dtype} {tuple(table.shape)}")
    if label_arena.numel() < 1 or (image_arena is not None and image_arena.numel() != label_arena.numel()):
        raise ValueError(f"{who}: the arenas hold the same, positive number of elements")
    return int(table.shape[0]), int(label_arena.numel())


def slice_foreground(label_arena: torch.Tensor, table: torch.Tensor, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """int32 device tensor [S]: the number of non-zero raw label bytes of every slice of the packed uint8 arena (ctl_slice_foreground;
    table: int64 [S,3] of element offset, h, w).  One launch, integer adds only, no readback."""
    n_slices, elems = _arenas(None, label_arena, table, "slice_foreground")
    out = _out(out, torch.int32, (n_slices,), label_arena.device, "slice_foreground", on_device=False)        # a host `out` is require_gpu's to refuse
    require_gpu(label_arena, table, out)
    call("ctl_slice_foreground", ptr(label_arena), ptr(table), n_slices, elems, ptr(out), stream_ptr())
    return out


def batch_gather(image_arena: torch.Tensor, label_arena: torch.Tensor, table: torch.Tensor, index, lut: torch.Tensor, canvas, crop=None,
                 out=None, orig_out=None):
    """The padded batch of the slices `index` names, and with `crop` upstream's original pair, in one launch (ctl_batch_gather).
    index: int32 DEVICE tensor [n], read on the device (its range is the caller's contract; nothing is synchronised), or host integers
    (numpy / list / CPU tensor), which are checked against [0, S) and uploaded.  lut: uint8 device tensor [256] (formulate_labels).
    canvas = (H, W) -> image [n,1,H,W] float32, label [n,H,W] int64; crop = (Hc, Wc) -> also orig_image [n,1,Hc,Wc], orig_label [n,Hc,Wc].
    out = (image, label), orig_out = (orig_image, orig_label): contiguous tensors to write into (views into a larger batch are fine).
    -> (image, label) or (image, label, orig_image, orig_label)."""
    who = "batch_gather"
    n_slices, elems = _arenas(image_arena, label_arena, table, who)
    if lut.dtype != torch.uint8 or tuple(lut.shape) != (256,) or not lut.is_contiguous():
        raise TypeError(f"{who}: the lookup table is a contiguous uint8 tensor [256], got {lut.dtype} {tuple(lut.shape)}")
    H, W = int(canvas[0]), int(canvas[1])
    if crop is None and orig_out is not None:
        raise ValueError(f"{who}: orig_out without a crop size")
    host_index = not (torch.is_tensor(index) and index.is_cuda)
    if host_index:
        index_h = np.ascontiguousarray(index.numpy() if torch.is_tensor(index) else index)
        if index_h.ndim != 1 or index_h.dtype.kind not in "iu":
            raise TypeError(f"{who}: a host index is a 1-D integer array, got {index_h.dtype} {index_h.shape}")
        n = int(index_h.size)
    else:
        if index.dtype != torch.int32 or index.dim() != 1 or not index.is_contiguous():
            raise TypeError(f"{who}: a device index is a contiguous int32 tensor [n], got {index.dtype} {tuple(index.shape)}")
        n = int(index.shape[0])
    if n < 1:
        raise ValueError(f"{who}: an empty index")
    if out is not None and int(out[0].shape[0]) != n:
        raise ValueError(f"{who}: an index of {n} entries for outputs of {int(out[0].shape[0])} samples")
    if host_index and (int(index_h.min()) < 0 or int(index_h.max()) >= n_slices):
        raise IndexError(f"{who}: host index outside [0, {n_slices}): min {int(index_h.min())}, max {int(index_h.max())}")
    dev = image_arena.device
    image = _out(None if out is None else out[0], torch.float32, (n, 1, H, W), dev, who, "out[0]", on_device=False)      # host outputs are
    label = _out(None if out is None else out[1], torch.int64, (n, H, W), dev, who, "out[1]", on_device=False)           # require_gpu's to refuse
    oi = ol = None
    Hc = Wc = 0
    if crop is not None:
        Hc, Wc = int(crop[0]), int(crop[1])
        oi = _out(None if orig_out is None else orig_out[0], torch.float32, (n, 1, Hc, Wc), dev, who, "orig_out[0]", on_device=False)
        ol = _out(None if orig_out is None else orig_out[1], torch.int64, (n, Hc, Wc), dev, who, "orig_out[1]", on_device=False)
    require_gpu(image_arena, label_arena, table, lut, image, label, oi, ol)
    if host_index:
        index = torch.from_numpy(index_h.astype(np.int32)).pin_memory().to(dev, non_blocking=True)
    call("ctl_batch_gather", ptr(image_arena), ptr(label_arena), ptr(table), n_slices, elems, ptr(index), n, ptr(lut), H, W, ptr(image),
         ptr(label), Hc, Wc, ptr(oi), ptr(ol), stream_ptr())
    return (image, label) if crop is None else (image, label, oi, ol)
