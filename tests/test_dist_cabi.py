"""C-ABI of the distance-map entries without a GPU (include/ctl_hip.h, csrc/ctl_dist.hip, csrc/ctl_loss.hip): declared, exported and bound; the
ABI version is unchanged; every bad argument fails with -1 and a message before anything is launched; the Python layers check names, forms
and devices before they reach the library."""
import ctypes
import os
import re

import pytest
import torch

from cooperative_training_and_latent_space_data_augmentation_amd import _ffi, autograd, losses, ops, solver

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ["ctl_class_fields_ws_bytes", "ctl_class_fields", "ctl_confident_label", "ctl_dist_loss_ws_doubles", "ctl_dist_loss_fwd", "ctl_dist_loss_bwd"]
lib = _ffi.lib
DUMMY = ctypes.cast((ctypes.c_double * 64)(), ctypes.c_void_p)            # never dereferenced: every check fails before a launch
BOUNDARY, HDT = _ffi.DLOSS_BOUNDARY, _ffi.DLOSS_HAUSDORFF_DT


def refused(rc, *words):
    msg = lib.ctl_last_error()
    assert rc == -1 and msg and all(w in msg for w in words), (rc, msg)


def fields(label=DUMMY, dtype=_ffi.LABEL_I64, b=2, h=5, w=7, c=4, form=_ffi.FIELD_SIGNED, out=DUMMY, ws=DUMMY, nbytes=1 << 20):
    return lib.ctl_class_fields(label, dtype, b, h, w, c, form, out, ws, nbytes, None)


def fwd(kind=HDT, logit=DUMMY, label=DUMMY, fa=DUMMY, fb=DUMMY, b=2, hw=15, c=4, ws=DUMMY, loss=DUMMY):
    return lib.ctl_dist_loss_fwd(kind, logit, label, fa, fb, b, hw, c, ws, loss, None)


def bwd(kind=HDT, logit=DUMMY, label=DUMMY, fa=DUMMY, fb=DUMMY, gout=DUMMY, b=2, hw=15, c=4, dlogit=DUMMY):
    return lib.ctl_dist_loss_bwd(kind, logit, label, fa, fb, gout, b, hw, c, dlogit, None)


def test_symbols_are_declared_exported_and_bound():
    header = open(os.path.join(ROOT, "include", "ctl_hip.h")).read()
    declared = set(re.findall(r"\b(ctl_[a-z0-9_]+)\s*\(", header))
    raw = ctypes.CDLL(_ffi.LIB_PATH)
    for name in NEW:
        assert name in declared and name in _ffi.EXPORTED and hasattr(raw, name), name
        assert len(getattr(lib, name).argtypes) == len(_ffi.SIGNATURES[name][1]), name
    assert [len(_ffi.SIGNATURES[n][1]) for n in NEW] == [4, 11, 5, 4, 11, 11]
    assert int(re.search(r"#define\s+CTL_ABI_VERSION\s+(\d+)", header).group(1)) == 11 == lib.ctl_version() == _ffi.ABI_VERSION      # additive
    for name, value in (("CTL_DLOSS_BOUNDARY", BOUNDARY), ("CTL_DLOSS_HAUSDORFF_DT", HDT), ("CTL_FIELD_D2", _ffi.FIELD_D2),
                        ("CTL_FIELD_SIGNED", _ffi.FIELD_SIGNED), ("CTL_FIELD_SQUARED", _ffi.FIELD_SQUARED), ("CTL_LABEL_U8", _ffi.LABEL_U8),
                        ("CTL_LABEL_I64", _ffi.LABEL_I64)):
        assert re.search(name + r"\s*=\s*%d\b" % value, header), name
    assert ops.DIST_LOSS_KINDS == {"boundary": BOUNDARY, "hausdorff dt": HDT}
    srcs = re.search(r"^SRCS\s*:=(.*)$", open(os.path.join(os.path.dirname(_ffi.LIB_PATH), "Makefile")).read(), re.M).group(1).split()
    assert "ctl_dist.hip" in srcs
    for fn in ("class_fields", "confident_label", "dist_loss_fwd", "dist_loss_bwd"):
        assert callable(getattr(ops, fn)), fn


def test_scratch_sizes():
    align = lambda n: (n + 255) // 256 * 256
    for b, h, w, c in ((1, 1, 1, 1), (3, 5, 7, 4), (16, 256, 256, 4), (2, 2048, 2048, 16), (3, 65, 130, 5)):
        assert lib.ctl_class_fields_ws_bytes(b, h, w, c) == align(b * c * h * w * 2 * 2), (b, h, w, c)      # two uint16 row maps per class
    for args in ((0, 5, 7, 4), (2, 0, 7, 4), (2, 5, -1, 4), (2, 5, 7, 0), (2, 5, 7, 17), (2, 2049, 7, 4), (2, 5, 2049, 4), (64, 2048, 2048, 16)):
        assert lib.ctl_class_fields_ws_bytes(*args) == 0, args
    red = lib.ctl_red_blocks()
    for kind in (BOUNDARY, HDT):
        assert lib.ctl_dist_loss_ws_doubles(kind, 16, 256 * 256, 4) == red == lib.ctl_dist_loss_ws_doubles(kind, 1, 1, 2)
    for args in ((2, 2, 15, 4), (-1, 2, 15, 4), (HDT, 0, 15, 4), (HDT, 2, 0, 4), (HDT, 2, 15, 17), (HDT, 2, 15, 1), (BOUNDARY, 2, 15, 0),
                 (HDT, 1 << 9, 1 << 18, 4)):
        assert lib.ctl_dist_loss_ws_doubles(*args) == 0, args


def test_class_fields_refusals():
    before = lib.ctl_launch_count()
    for kw in (dict(label=None), dict(out=None), dict(ws=None)):
        refused(fields(**kw), b"class_fields", b"null")
    for dtype in (2, -1):
        refused(fields(dtype=dtype), b"class_fields", b"dtype %d" % dtype)
    for form in (3, -1, 17):
        refused(fields(form=form), b"class_fields", b"form %d" % form)
    for kw in (dict(b=0), dict(b=-2), dict(h=0), dict(w=0), dict(w=-5)):
        refused(fields(**kw), b"class_fields", b"sizes")
    for c in (0, 17, -1):
        refused(fields(c=c), b"class_fields", b"classes")
    for kw in (dict(h=2049), dict(w=2049), dict(h=65536)):
        refused(fields(**kw), b"class_fields", b"2048")
    refused(fields(b=64, h=2048, w=2048, c=16), b"class_fields", b"too large")
    refused(fields(nbytes=lib.ctl_class_fields_ws_bytes(2, 5, 7, 4) - 1), b"class_fields", b"workspace")
    assert lib.ctl_launch_count() == before, "a refused call launched something"


@pytest.mark.parametrize("call, who", [(fwd, b"dist_loss_fwd"), (bwd, b"dist_loss_bwd")])
def test_loss_refusals(call, who):
    before = lib.ctl_launch_count()
    own = (dict(ws=None), dict(loss=None)) if call is fwd else (dict(gout=None), dict(dlogit=None))
    for kw in (dict(logit=None), dict(fa=None), dict(fb=None), dict(label=None)) + own:
        refused(call(**kw), who, b"null")
    for kw in (dict(fa=None),) + own:
        refused(call(kind=BOUNDARY, **kw), who, b"null")
    for kind in (2, -1, 17):
        refused(call(kind=kind), who, b"kind %d" % kind)
    for kw in (dict(b=0), dict(b=-2), dict(hw=0), dict(hw=-5)):
        refused(call(**kw), who, b"sizes")
    for c in (0, 1, 17, -1):
        refused(call(c=c), who, b"classes")
    refused(call(b=1 << 9, hw=1 << 18, c=4), who, b"2 GiB")
    refused(call(b=1, hw=1 << 31, c=2), who, b"2 GiB")
    assert lib.ctl_launch_count() == before, "a refused call launched something"
    with pytest.raises(_ffi.CtlError, match="classes"):
        _ffi.check(call(c=17), "ctl_dist_loss")


def test_confident_label_refusals():
    before = lib.ctl_launch_count()
    refused(lib.ctl_confident_label(None, DUMMY, 10, 4, None), b"confident_label", b"null")
    refused(lib.ctl_confident_label(DUMMY, None, 10, 4, None), b"confident_label", b"null")
    for pixels in (0, -3, 1 << 31):
        refused(lib.ctl_confident_label(DUMMY, DUMMY, pixels, 4, None), b"confident_label", b"pixels")
    for c in (0, 17, -1):
        refused(lib.ctl_confident_label(DUMMY, DUMMY, 10, c, None), b"confident_label", b"classes")
    assert lib.ctl_launch_count() == before


def test_python_layers_check_before_the_device():
    x, y = torch.zeros(2, 4, 3, 5), torch.zeros(2, 3, 5, dtype=torch.long)
    f = torch.zeros(2, 4, 3, 5)
    for name in ("boundary", "hausdorff dt", {"dice": 1.0, "boundary": 0.01}, {"cross entropy": 1.0, "hausdorff dt": 1e-3}):
        with pytest.raises(_ffi.CtlError, match="device tensors"):
            solver.basic_loss_fn(x, y, name)
        if isinstance(name, str):
            with pytest.raises(_ffi.CtlError, match="device tensors"):
                autograd.segmentation_loss(x, y, name)
            with pytest.raises(_ffi.CtlError, match="device tensors"):
                autograd.segmentation_loss(x, y, name, fields=f)
            with pytest.raises(_ffi.CtlError, match="device tensors"):
                ops.dist_loss_fwd(x, y, name, f, f)
            with pytest.raises(_ffi.CtlError, match="device tensors"):
                ops.dist_loss_bwd(x, y, name, torch.ones(()), f, f)
    for name in ("hausdorff", "contour_smooth", "cross_entropy", "nope"):
        with pytest.raises(NotImplementedError):
            solver.basic_loss_fn(x, y, name)
        with pytest.raises(NotImplementedError):
            autograd.segmentation_loss(x, y, name)
        with pytest.raises(NotImplementedError):
            ops.dist_loss_fwd(x, y, name, f, f)
    with pytest.raises(NotImplementedError):
        solver.basic_loss_fn(x, y, {"boundary": 1.0, "hausdorff": 1.0})
    for name in ("boundary", "hausdorff dt"):
        with pytest.raises(ValueError, match="2 classes"):
            solver.basic_loss_fn(torch.zeros(2, 1, 3, 5), y, name)
        with pytest.raises(ValueError, match="2 classes"):
            autograd.segmentation_loss(torch.zeros(2, 1, 3, 5), y, name)
    with pytest.raises(ValueError, match="needs"):
        ops.dist_loss_fwd(x, y, "hausdorff dt", f)
    with pytest.raises(ValueError, match="form"):
        ops.class_fields(y, 4, "sdf")
    for c in (0, 17):
        with pytest.raises(ValueError, match="classes"):
            ops.class_fields(y, c)
    with pytest.raises(_ffi.CtlError, match="device tensors"):
        ops.class_fields(y, 4, "signed")
    with pytest.raises(_ffi.CtlError, match="device tensors"):
        ops.confident_label(x)
    with pytest.raises(_ffi.CtlError, match="device tensors"):
        autograd.LabelFields(y, 4)
    assert solver.needs_fields("boundary") and solver.needs_fields({"dice": 1.0, "hausdorff dt": 1.0})
    assert not solver.needs_fields("cross entropy") and not solver.needs_fields({"dice": 1.0, "focal": 1.0})
    assert set(losses.DIST_LOSS_NAMES) == set(ops.DIST_LOSS_KINDS) == set(ops.DIST_LOSS_FORM)


def test_solver_refuses_a_bad_loss_spec_before_it_touches_the_device():
    S = solver.AdvancedTripletReconSegmentationModel
    for kw, err in ((dict(seg_loss_type="hausdorff"), NotImplementedError), (dict(seg_loss_type={"boundary": 1.0, "nope": 1.0}), NotImplementedError),
                    (dict(seg_loss_type="boundary", num_classes=1), ValueError)):
        with pytest.raises(err):
            S(use_gpu=True, **kw)
