"""C-ABI of the device-resident training set without a GPU: ctl_slice_foreground and ctl_batch_gather are declared, exported and bound
with the declared argument lists, the ABI version is unchanged, and bad arguments are refused before anything is launched, in the C
entry points and in the ops wrappers."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

from cooperative_training_and_latent_space_data_augmentation_amd import _ffi, loader, ops, trainer

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = {"ctl_slice_foreground": 6, "ctl_batch_gather": 17}
lib = _ffi.lib
DUMMY = ctypes.cast((ctypes.c_double * 64)(), ctypes.c_void_p)            # never dereferenced: every check fails before a launch


def refused(rc, *words):
    msg = lib.ctl_last_error()
    assert rc == -1 and msg and all(w in msg for w in words), (rc, msg)


def test_symbols_are_declared_exported_and_bound():
    header = open(os.path.join(ROOT, "include", "ctl_hip.h")).read()
    raw = ctypes.CDLL(_ffi.LIB_PATH)
    for name, n_args in NEW.items():
        decl = re.search(r"\bint\s+" + name + r"\s*\(([^;]*)\)\s*;", header)
        assert decl is not None and len(decl.group(1).split(",")) == n_args, name
        assert name in _ffi.EXPORTED and hasattr(raw, name), name
        assert len(getattr(lib, name).argtypes) == n_args, name
    assert int(re.search(r"#define\s+CTL_ABI_VERSION\s+(\d+)", header).group(1)) == 11 == lib.ctl_version()      # additive: no bump
    for fn in ("slice_foreground", "batch_gather"):
        assert callable(getattr(ops, fn)), fn
    for fn in ("DeviceSliceSet", "DeviceBatchLoader", "gather_host", "resolve_empty_slices", "epoch_order"):
        assert callable(getattr(loader, fn)), fn
    for fn in ("get_batch", "eval_model", "train_network"):
        assert callable(getattr(trainer, fn)), fn


def test_slice_foreground_refusals():
    refused(lib.ctl_slice_foreground(None, DUMMY, 1, 10, DUMMY, None), b"null")
    refused(lib.ctl_slice_foreground(DUMMY, None, 1, 10, DUMMY, None), b"null")
    refused(lib.ctl_slice_foreground(DUMMY, DUMMY, 1, 10, None, None), b"null")
    refused(lib.ctl_slice_foreground(DUMMY, DUMMY, 0, 10, DUMMY, None), b"slices")
    refused(lib.ctl_slice_foreground(DUMMY, DUMMY, 1, 0, DUMMY, None), b"slices")


def test_batch_gather_refusals():
    ok = dict(image=DUMMY, label=DUMMY, table=DUMMY, n_slices=3, elems=100, index=DUMMY, n=2, lut=DUMMY, H=8, W=8, io=DUMMY, lo=DUMMY, Hc=4,
              Wc=4, oi=DUMMY, ol=DUMMY)

    def call(**kw):
        a = dict(ok, **kw)
        return lib.ctl_batch_gather(a["image"], a["label"], a["table"], a["n_slices"], a["elems"], a["index"], a["n"], a["lut"], a["H"], a["W"],
                                    a["io"], a["lo"], a["Hc"], a["Wc"], a["oi"], a["ol"], None)

    for k in ("image", "label", "table", "index", "lut", "io", "lo"):
        refused(call(**{k: None}), b"null")
    refused(call(oi=None), b"both")
    refused(call(ol=None), b"both")
    refused(call(n_slices=0), b"slices")
    refused(call(elems=0), b"slices")
    for n in (0, -1, 65536):
        refused(call(n=n), b"batch of")
    for kw in (dict(H=0), dict(W=0), dict(H=32769), dict(W=-3)):
        refused(call(**kw), b"canvas")
    for kw in (dict(Hc=0), dict(Wc=0), dict(Wc=32769)):
        refused(call(**kw), b"crop")
    refused(call(io=ctypes.c_void_p(DUMMY.value + 2)), b"aligned")
    refused(call(ol=ctypes.c_void_p(DUMMY.value + 4)), b"aligned")
    with pytest.raises(_ffi.CtlError, match="batch of 0"):
        _ffi.check(call(n=0), "ctl_batch_gather")


def _host_set():
    """valid arguments of ops.batch_gather, all on the host"""
    return dict(image_arena=torch.zeros(64), label_arena=torch.zeros(64, dtype=torch.uint8),
                table=torch.tensor([[0, 4, 4], [16, 4, 4], [32, 4, 8]]), lut=torch.arange(256, dtype=torch.uint8))


def _gather(index=(0, 2), canvas=(8, 8), crop=(4, 4), out=None, orig_out=None, **kw):
    a = dict(_host_set(), **kw)
    return ops.batch_gather(a["image_arena"], a["label_arena"], a["table"], index, a["lut"], canvas, crop, out=out, orig_out=orig_out)


def test_wrappers_refuse_host_tensors():
    a = _host_set()
    with pytest.raises(_ffi.CtlError, match="CPU tensor"):
        ops.slice_foreground(a["label_arena"], a["table"])
    with pytest.raises(_ffi.CtlError, match="CPU tensor"):
        _gather()
    with pytest.raises(_ffi.CtlError, match="CPU tensor"):
        _gather(index=np.array([1, 1, 0]))


def test_wrappers_refuse_wrong_dtypes_and_shapes():
    a = _host_set()
    with pytest.raises(TypeError, match="label arena"):
        ops.slice_foreground(a["label_arena"].long(), a["table"])
    with pytest.raises(TypeError, match="slice table"):
        ops.slice_foreground(a["label_arena"], a["table"].int())
    with pytest.raises(TypeError, match="image arena"):
        _gather(image_arena=a["image_arena"].double())
    with pytest.raises(TypeError, match="label arena"):
        _gather(label_arena=a["label_arena"].to(torch.int8))
    with pytest.raises(TypeError, match="slice table"):
        _gather(table=a["table"][:, :2].contiguous())
    with pytest.raises(TypeError, match="lookup table"):
        _gather(lut=a["lut"][:255])
    with pytest.raises(TypeError, match="host index"):
        _gather(index=np.array([0.0, 1.0]))
    with pytest.raises(ValueError, match="same, positive number"):
        _gather(label_arena=torch.zeros(63, dtype=torch.uint8))
    with pytest.raises(ValueError, match=r"`out\[1\]`"):
        _gather(out=(torch.zeros(2, 1, 8, 8), torch.zeros(2, 8, 8, dtype=torch.int32)))
    with pytest.raises(ValueError, match=r"`orig_out\[0\]`"):
        _gather(orig_out=(torch.zeros(2, 1, 4, 5), torch.zeros(2, 4, 4, dtype=torch.int64)))
    with pytest.raises(ValueError, match="without a crop"):
        _gather(crop=None, orig_out=(torch.zeros(2, 1, 4, 4), torch.zeros(2, 4, 4, dtype=torch.int64)))


def test_wrapper_refuses_an_index_of_the_wrong_length_or_range():
    out = (torch.zeros(3, 1, 8, 8), torch.zeros(3, 8, 8, dtype=torch.int64))
    with pytest.raises(ValueError, match="index of 2 entries for outputs of 3"):
        _gather(index=[0, 1], out=out)
    with pytest.raises(ValueError, match="empty index"):
        _gather(index=np.zeros(0, dtype=np.int64))
    for bad in ([0, 3], [-1, 0], np.array([2, 1, 7]), torch.tensor([0, 5])):
        with pytest.raises(IndexError, match=r"outside \[0, 3\)"):
            _gather(index=bad)
