"""C-ABI of the image-similarity losses without a GPU: the entries of include/ctl_hip.h are exported and bound, the ABI version is unchanged,
every bad argument fails with -1 and a message that names it before anything is launched, the workspace sizes are what the header says
and what the wrappers allocate, and the Python layers check names and parameters before they look at the device."""
import ctypes
import os
import re

import pytest
import torch

from cooperative_training_and_latent_space_data_augmentation_amd import _ffi, autograd, ops, recon, solver

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ["ctl_recon_ws_doubles", "ctl_recon_loss_fwd", "ctl_recon_loss_bwd"]
lib = _ffi.lib
DUMMY = ctypes.cast((ctypes.c_double * 64)(), ctypes.c_void_p)            # never dereferenced: every check fails before a launch
MSE, L1, SL1, NCC, LNCC = _ffi.RECON_MSE, _ffi.RECON_L1, _ffi.RECON_SMOOTH_L1, _ffi.RECON_NCC, _ffi.RECON_LNCC
STREAM = MSE | L1 | SL1 | NCC
ALL = STREAM | LNCC


def refused(rc, *words):
    msg = lib.ctl_last_error()
    assert rc == -1 and msg and all(w in msg for w in words), (rc, msg)


def doubles(*v):
    return (ctypes.c_double * len(v))(*v)


ONES = doubles(1, 1, 1, 1, 1)


def fwd(kinds=MSE, weights=ONES, x=DUMMY, t=DUMMY, mask=None, t_batch=2, b=2, h=9, w=11, c=4, beta=0.25, win=9, zero_mean=1, rsum=0, ws=DUMMY,
        loss=DUMMY):
    return lib.ctl_recon_loss_fwd(kinds, weights, x, t, mask, t_batch, b, h, w, c, beta, win, zero_mean, rsum, ws, loss, None)


def bwd(kinds=MSE, weights=ONES, x=DUMMY, t=DUMMY, mask=None, t_batch=2, gout=DUMMY, ws=DUMMY, b=2, h=9, w=11, c=4, beta=0.25, win=9, zero_mean=1,
        rsum=0, dx=DUMMY):
    return lib.ctl_recon_loss_bwd(kinds, weights, x, t, mask, t_batch, gout, ws, b, h, w, c, beta, win, zero_mean, rsum, dx, None)


def test_symbols_are_declared_exported_and_bound():
    header = open(os.path.join(ROOT, "include", "ctl_hip.h")).read()
    declared = set(re.findall(r"\b(ctl_[a-z0-9_]+)\s*\(", header))
    raw = ctypes.CDLL(_ffi.LIB_PATH)
    for name in NEW:
        assert name in declared and name in _ffi.EXPORTED and hasattr(raw, name), name
        assert getattr(lib, name).argtypes is not None, name
    assert len(lib.ctl_recon_loss_fwd.argtypes) == 17 and len(lib.ctl_recon_loss_bwd.argtypes) == 18
    assert int(re.search(r"#define\s+CTL_ABI_VERSION\s+(\d+)", header).group(1)) == 11 == lib.ctl_version() == _ffi.ABI_VERSION      # additive
    names = ("CTL_RECON_MSE", "CTL_RECON_L1", "CTL_RECON_SMOOTH_L1", "CTL_RECON_NCC", "CTL_RECON_LNCC")
    for k, name in enumerate(names):
        assert re.search(name + r"\s*=\s*%d\b" % (1 << k), header), name
    assert (MSE, L1, SL1, NCC, LNCC) == (1, 2, 4, 8, 16)
    assert ops.RECON_KINDS == {"mse": MSE, "l1": L1, "smooth l1": SL1, "ncc": NCC, "lncc": LNCC}
    assert tuple(ops.RECON_KINDS) == recon.RECON_NAMES
    for cite in ("(ctl_recon.hip)", "smooth_l1_loss :310-318", "CustomNormalizedCrossCorrelationLoss :514-571",
                 "CustomLocalNormalizedCrossCorrelationLoss :574-661"):
        assert cite in header, cite                                                                  # each entry cites upstream
    assert callable(ops.recon_loss_fwd) and callable(ops.recon_loss_bwd) and callable(autograd.image_similarity_loss)
    assert callable(recon.similarity_and_grad) and callable(recon.smooth_l1_loss)
    assert "ctl_recon.hip" in open(os.path.join(os.path.dirname(_ffi.LIB_PATH), "Makefile")).read()


def test_workspace_sizes():
    size = lib.ctl_recon_ws_doubles
    for b, h, w, c in ((1, 3, 3, 1), (3, 17, 31, 5), (16, 192, 192, 1), (16, 256, 256, 16), (1000, 64, 64, 4), (2, 33, 34, 4)):
        nb = lib.ctl_seg_loss_blocks(b, h * w)
        fixed = b * 2 + b * c * 2 + b * c * 5
        pw = b * nb * (3 + 5 * c)
        tiles = min(b * -(-h // 16) * -(-w // 16), 2048)
        for kinds in (MSE, L1, SL1, NCC, MSE | NCC, STREAM):
            assert size(kinds, b, h, w, c, 9) == size(kinds, b, h, w, c, 4) == fixed + pw, (kinds, b, h, w, c)      # win is not looked at
        assert size(LNCC, b, h, w, c, 3) == size(LNCC, b, h, w, c, 3 if min(h, w) < 15 else 15) == fixed + tiles + 3 * b * h * w
        assert size(MSE | LNCC, b, h, w, c, 3) == size(ALL, b, h, w, c, 3) == fixed + pw + tiles + 3 * b * h * w
    for args in ((0, 2, 9, 9, 4, 9), (32, 2, 9, 9, 4, 9), (-1, 2, 9, 9, 4, 9), (MSE, 0, 9, 9, 4, 9), (MSE, 2, 0, 9, 4, 9), (MSE, 2, 9, -1, 4, 9),
                 (MSE, 2, 9, 9, 17, 9), (MSE, 2, 9, 9, 0, 9), (LNCC, 2, 9, 9, 4, 4), (LNCC, 2, 9, 9, 4, 1), (LNCC, 2, 9, 9, 4, 17), (LNCC, 2, 9, 8, 4, 9),
                 (LNCC, 2, 8, 9, 4, 9), (ALL, 2, 9, 8, 4, 9), (MSE, 1 << 9, 1 << 9, 1 << 9, 16, 9), (MSE, 65536, 1, 1, 4, 9)):
        assert size(*args) == 0, args


@pytest.mark.parametrize("call, who", [(fwd, b"recon_loss_fwd"), (bwd, b"recon_loss_bwd")])
def test_refusals(call, who):
    before = lib.ctl_launch_count()
    nulls = (dict(x=None), dict(t=None), dict(ws=None)) + ((dict(loss=None),) if call is fwd else (dict(gout=None), dict(dx=None)))
    for kw in nulls + (dict(weights=None),):
        refused(call(**kw), who, b"null")
    for kinds in (0, 32, -1, 64 | MSE):
        refused(call(kinds=kinds), who, b"kinds")
    for kw in (dict(b=0, t_batch=1), dict(b=-2), dict(h=0), dict(w=-5)):
        refused(call(**kw), who, b"sizes")
    for c in (0, 17, -1):
        refused(call(c=c), who, b"c = ", b"channels")
    for win in (4, 8, 1, 17, -3, 0):
        refused(call(kinds=LNCC, win=win), who, b"win = ")
        refused(call(kinds=ALL, win=win), who, b"win = ")
        assert call(kinds=MSE, win=win, x=None) == -1 and b"null" in lib.ctl_last_error()            # (not read without 'lncc')
    refused(call(kinds=LNCC, win=11, h=9, w=11), who, b"win = 11", b"h = 9")
    refused(call(kinds=LNCC, win=11, h=11, w=9), who, b"win = 11", b"w = 9")
    refused(call(kinds=MSE | LNCC, win=15, h=14, w=14), who, b"win = 15", b"h = 14")
    for beta in (0.0, -0.5, float("nan"), float("inf")):
        refused(call(kinds=SL1, beta=beta), who, b"beta")
        refused(call(kinds=ALL, beta=beta), who, b"beta")
    refused(call(b=65536, t_batch=65536, h=1, w=1), who, b"65535")
    refused(call(b=1 << 9, t_batch=1 << 9, h=1 << 9, w=1 << 9, c=16), who, b"2^31")
    refused(call(b=1, t_batch=1, h=1 << 16, w=1 << 15, c=1), who, b"2^31")
    refused(call(b=8, t_batch=8, h=1 << 14, w=1 << 14, c=1), who, b"2^31")
    for tb in (0, 3, -1):
        refused(call(t_batch=tb), who, b"t_batch")
    for bad in (float("nan"), float("inf"), float("-inf")):
        refused(call(kinds=MSE | NCC, weights=doubles(1, 1, 1, bad, 1)), who, b"weight", b"kind 3")
    assert lib.ctl_launch_count() == before, "a refused call launched something"
    with pytest.raises(_ffi.CtlError, match="channels"):
        _ffi.check(call(c=17), "ctl_recon")


def test_python_layers_check_before_the_device():
    x, t = torch.zeros(2, 4, 16, 15), torch.zeros(2, 4, 16, 15)
    for name in ("ssim", "huber", "MSE"):
        with pytest.raises(NotImplementedError, match="image-similarity"):
            autograd.image_similarity_loss(x, t, {name: 1.0})
        with pytest.raises(NotImplementedError, match="image-similarity"):
            ops.recon_loss_fwd(x, t, {name: 1.0})
    with pytest.raises(ValueError, match="kinds"):
        ops.recon_loss_fwd(x, t, {})
    with pytest.raises(ValueError):
        autograd.image_similarity_loss(x, t, {})
    with pytest.raises(ValueError, match="constant"):
        autograd.image_similarity_loss(x, t.clone().requires_grad_(True), "mse")
    for fn in (lambda **kw: ops.recon_loss_fwd(x, t, {"mse": 1.0}, **kw), lambda **kw: autograd.image_similarity_loss(x, t, "mse", **kw)):
        with pytest.raises(NotImplementedError, match="none"):
            fn(reduction="none")
    with pytest.raises(NotImplementedError, match="none"):
        ops.recon_loss_bwd(x, t, {"mse": 1.0}, torch.ones(()), torch.zeros(8, dtype=torch.float64), reduction="none")
    with pytest.raises(ValueError, match="reduction"):
        ops.recon_loss_fwd(x, t, {"mse": 1.0}, reduction="batch")
    for win in (4, 17, 1):
        with pytest.raises(ValueError, match="win"):
            ops.recon_loss_fwd(x, t, {"lncc": 1.0}, win=win)
    with pytest.raises(ValueError, match="beta"):
        ops.recon_loss_fwd(x, t, {"smooth l1": 1.0}, beta=0.0)
    for call in (lambda: autograd.image_similarity_loss(x, t, {"mse": 1.0, "lncc": 0.1}), lambda: ops.recon_loss_fwd(x, t, {"ncc": 1.0}),
                 lambda: ops.recon_loss_bwd(x, t, {"l1": 1.0}, torch.ones(()), torch.zeros(8, dtype=torch.float64))):
        with pytest.raises(_ffi.CtlError, match="device tensors"):       # no CPU fallback behind the kernels
            call()
    # the solver parses and refuses its reconstruction loss at construction, before any storage is allocated
    parse = solver.AdvancedTripletReconSegmentationModel._parse_recon
    assert parse("mse", None, 1) == ("mse", {}, None)                                            # the default: today's scaled_mse call
    assert parse({"mse": 1, "lncc": 0.5}, {"win": 9}, 1) == ({"mse": 1, "lncc": 0.5}, {"win": 9}, {"mse": 0.5, "lncc": 0.25})
    assert parse("mse", {"reduction": "sum"}, 1)[2] == {"mse": 0.5} and parse("l1", None, 1)[2] == {"l1": 0.5}
    with pytest.raises(NotImplementedError, match="image-similarity"):
        parse("ssim", None, 1)
    for kinds, params in (("lncc", {"win": 4}), ("smooth l1", {"beta": 0.0}), ("mse", {"reduction": "none"}), ("mse", {"gamma": 2.0})):
        with pytest.raises(ValueError):
            parse(kinds, params, 1)
