"""C-ABI of the consistency losses without a GPU: the entries of include/ctl_hip.h are exported and bound, the ABI version is unchanged,
every bad argument fails with -1 and a message before anything is launched, the workspace sizes are what the header says, and the Python
layers check names, weights and shapes before they look at the device."""
import ctypes
import os
import re

import pytest
import torch

from cooperative_training_and_latent_space_data_augmentation_amd import _ffi, autograd, consistency, ops, solver

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ["ctl_consistency_ws_doubles", "ctl_consistency_fwd", "ctl_consistency_bwd", "ctl_avgpool_fwd", "ctl_avgpool_bwd"]
lib = _ffi.lib
DUMMY = ctypes.cast((ctypes.c_double * 64)(), ctypes.c_void_p)            # never dereferenced: every check fails before a launch
KL, CE, WCE, MSE, DICE, CONTOUR = _ffi.CONS_KL, _ffi.CONS_CE, _ffi.CONS_WCE, _ffi.CONS_MSE, _ffi.CONS_DICE, _ffi.CONS_CONTOUR
ALL = KL | CE | WCE | MSE | DICE | CONTOUR


def refused(rc, *words):
    msg = lib.ctl_last_error()
    assert rc == -1 and msg and all(w in msg for w in words), (rc, msg)


def doubles(*v):
    return (ctypes.c_double * len(v))(*v)


ONES = doubles(1, 1, 1, 1, 1, 1)


def fwd(kinds=KL, weights=ONES, cw=None, x=DUMMY, r=DUMMY, mask=None, is_gt=0, b=2, h=3, w=5, c=4, ws=DUMMY, loss=DUMMY):
    return lib.ctl_consistency_fwd(kinds, weights, cw, x, r, mask, is_gt, b, h, w, c, ws, loss, None)


def bwd(kinds=KL, weights=ONES, cw=None, x=DUMMY, r=DUMMY, mask=None, is_gt=0, gout=DUMMY, ws=DUMMY, b=2, h=3, w=5, c=4, dlogit=DUMMY):
    return lib.ctl_consistency_bwd(kinds, weights, cw, x, r, mask, is_gt, gout, ws, b, h, w, c, dlogit, None)


def pool_fwd(x=DUMMY, b=2, h=8, w=8, c=4, scale=1, y=DUMMY):
    return lib.ctl_avgpool_fwd(x, b, h, w, c, scale, y, None)


def pool_bwd(x=DUMMY, b=2, h=8, w=8, c=4, scale=1, y=DUMMY):
    return lib.ctl_avgpool_bwd(x, b, h, w, c, scale, y, None)


def test_symbols_are_declared_exported_and_bound():
    header = open(os.path.join(ROOT, "include", "ctl_hip.h")).read()
    declared = set(re.findall(r"\b(ctl_[a-z0-9_]+)\s*\(", header))
    raw = ctypes.CDLL(_ffi.LIB_PATH)
    for name in NEW:
        assert name in declared and name in _ffi.EXPORTED and hasattr(raw, name), name
        assert getattr(lib, name).argtypes is not None, name
    assert len(lib.ctl_consistency_fwd.argtypes) == 14 and len(lib.ctl_consistency_bwd.argtypes) == 15
    assert int(re.search(r"#define\s+CTL_ABI_VERSION\s+(\d+)", header).group(1)) == 11 == lib.ctl_version() == _ffi.ABI_VERSION      # additive
    names = ("CTL_CONS_KL", "CTL_CONS_CE", "CTL_CONS_WCE", "CTL_CONS_MSE", "CTL_CONS_DICE", "CTL_CONS_CONTOUR")
    for t, name in enumerate(names):
        assert re.search(name + r"\s*=\s*%d\b" % (1 << t), header), name
    assert (KL, CE, WCE, MSE, DICE, CONTOUR) == (1, 2, 4, 8, 16, 32)
    assert ops.CONSISTENCY_KINDS == {"kl": KL, "ce": CE, "weighted ce": WCE, "mse": MSE, "Dice": DICE, "contour": CONTOUR}
    assert tuple(ops.CONSISTENCY_KINDS) == consistency.CONSISTENCY_NAMES
    assert "Consistency losses (ctl_consist.hip)" in header and "calc_segmentation_consistency :892-973" in header      # cites upstream
    for fn in ("consistency_fwd", "consistency_bwd", "avgpool_fwd", "avgpool_bwd"):
        assert callable(getattr(ops, fn)), fn
    assert callable(autograd.consistency_loss) and callable(autograd.avg_pool) and callable(consistency.consistency_and_grad)
    assert callable(solver.AdvancedTripletReconSegmentationModel.consistency_training)


def test_workspace_sizes():
    red = lib.ctl_red_blocks()
    size = lib.ctl_consistency_ws_doubles
    for b, h, w, c in ((1, 1, 1, 2), (3, 17, 31, 5), (16, 128, 128, 4), (16, 256, 256, 16), (1000, 64, 64, 4), (2, 33, 34, 4)):
        nb = lib.ctl_seg_loss_blocks(b, h * w)
        fixed = b * c * 2 + 8
        pw = b * nb * (5 + 3 * c)
        t = 32 if c <= 4 else 16
        tiles = min(b * -(-h // t) * -(-w // t), 2048)
        assert b * nb <= max(red, b)
        for kinds in (KL, CE, WCE, MSE, DICE, KL | MSE, KL | CE | WCE | MSE | DICE):
            assert size(kinds, b, h, w, c) == fixed + pw, (kinds, b, h, w, c)
        assert size(CONTOUR, b, h, w, c) == fixed + tiles
        assert size(KL | CONTOUR, b, h, w, c) == size(ALL, b, h, w, c) == fixed + pw + tiles
    assert size(CONTOUR, 2, 33, 34, 4) == 2 * 4 * 2 + 8 + 2 * 2 * 2 and size(CONTOUR, 2, 33, 34, 5) == 2 * 5 * 2 + 8 + 2 * 3 * 3
    for args in ((0, 2, 3, 5, 4), (64, 2, 3, 5, 4), (-1, 2, 3, 5, 4), (KL, 0, 3, 5, 4), (KL, 2, 0, 5, 4), (KL, 2, 3, -1, 4), (KL, 2, 3, 5, 17),
                 (KL, 2, 3, 5, 0), (CONTOUR, 2, 3, 5, 1), (ALL, 2, 3, 5, 1), (KL, 1 << 9, 1 << 9, 1 << 9, 4), (KL, 65536, 1, 1, 4)):
        assert size(*args) == 0, args
    assert size(KL | MSE | DICE, 2, 3, 5, 1) > 0             # the point-wise kinds take one class


@pytest.mark.parametrize("call, who", [(fwd, b"consistency_fwd"), (bwd, b"consistency_bwd")])
def test_refusals(call, who):
    before = lib.ctl_launch_count()
    nulls = (dict(x=None), dict(r=None), dict(ws=None)) + ((dict(loss=None),) if call is fwd else (dict(gout=None), dict(dlogit=None)))
    for kw in nulls + (dict(weights=None), dict(kinds=WCE), dict(kinds=ALL)):            # (weighted ce without class weights)
        refused(call(**kw), who, b"null")
    for kinds in (0, 64, -1, 128 | KL):
        refused(call(kinds=kinds), who, b"kinds")
    for kw in (dict(b=0), dict(b=-2), dict(h=0), dict(w=-5)):
        refused(call(**kw), who, b"sizes")
    for c in (0, 17, -1):
        refused(call(c=c), who, b"classes")
    refused(call(kinds=CONTOUR, c=1), who, b"contour", b"classes")
    refused(call(b=65536, h=1, w=1), who, b"65535")
    refused(call(b=1 << 9, h=1 << 9, w=1 << 9, c=4), who, b"2 GiB")
    refused(call(b=1, h=1 << 16, w=1 << 15, c=1), who, b"2 GiB")
    for bad in (float("nan"), float("inf"), float("-inf")):
        refused(call(kinds=KL | MSE, weights=doubles(1, 1, 1, bad, 1, 1)), who, b"weight", b"kind 3")
    assert call(kinds=0, weights=doubles(float("nan"), 1, 1, 1, 1, 1)) == -1               # (still refused: no kind)
    for cw in (doubles(0, 0, 0, 0), doubles(1, -1, 0, 0), doubles(float("nan"), 1, 1, 1), doubles(float("inf"), 1, 1, 1)):
        refused(call(kinds=WCE, cw=cw), who, b"class weights")
    assert lib.ctl_launch_count() == before, "a refused call launched something"
    with pytest.raises(_ffi.CtlError, match="classes"):
        _ffi.check(call(c=17), "ctl_consistency")


@pytest.mark.parametrize("call, who", [(pool_fwd, b"avgpool_fwd"), (pool_bwd, b"avgpool_bwd")])
def test_pool_refusals(call, who):
    before = lib.ctl_launch_count()
    for kw in (dict(x=None), dict(y=None)):
        refused(call(**kw), who, b"null")
    for kw in (dict(b=0), dict(h=0), dict(w=-1)):
        refused(call(**kw), who, b"sizes")
    for c in (0, 17):
        refused(call(c=c), who, b"channels")
    for s in (0, 5, -1):
        refused(call(scale=s), who, b"scale")
    refused(call(h=7, scale=3), who, b"smaller")
    refused(call(w=1, scale=1), who, b"smaller")
    refused(call(b=1 << 9, h=1 << 9, w=1 << 9), who, b"2 GiB")
    assert lib.ctl_launch_count() == before, "a refused call launched something"


def test_python_layers_check_before_the_device():
    x, r = torch.zeros(2, 4, 6, 5), torch.zeros(2, 4, 6, 5)
    for name in ("contour_smooth", "dice", "hausdorff"):
        with pytest.raises(NotImplementedError):
            autograd.consistency_loss(x, r, {name: 1.0})
        with pytest.raises(NotImplementedError):
            ops.consistency_fwd(x, r, {name: 1.0})
    with pytest.raises(ValueError, match="class weights"):
        ops.consistency_fwd(x, r, {"weighted ce": 1.0})
    with pytest.raises(ValueError, match="kinds"):
        autograd.consistency_loss(x, r, {})
    with pytest.raises(ValueError, match="constant"):
        autograd.consistency_loss(x, r.clone().requires_grad_(True), {"kl": 1.0})
    for call in (lambda: autograd.consistency_loss(x, r, {"kl": 1.0}), lambda: ops.consistency_fwd(x, r, {"kl": 1.0, "contour": 0.5}),
                 lambda: ops.avgpool_fwd(x, 1), lambda: autograd.avg_pool(x, 1),
                 lambda: ops.consistency_bwd(x, r, {"kl": 1.0}, torch.ones(()), torch.zeros(8, dtype=torch.float64))):
        with pytest.raises(_ffi.CtlError, match="device tensors"):       # no CPU fallback behind the kernels
            call()
    assert autograd.avg_pool(x, 0) is x
