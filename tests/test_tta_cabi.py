"""C-ABI boundary of the test-time-augmentation entries (include/ctl_hip.h, csrc/ctl_tta.hip): declared, exported and bound; the ABI
version did not move; every bad argument is refused with a message that names the reason, before any launch (no GPU here)."""
import ctypes
import os
import re

import pytest

from cooperative_training_and_latent_space_data_augmentation_amd import _ffi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRIES = ("ctl_tta_views", "ctl_tta_merge")
lib = _ffi.lib


def dummy():
    return ctypes.cast((ctypes.c_double * 8)(), ctypes.c_void_p)      # never dereferenced: the check fails before any launch


def codes_of(*v):
    return (ctypes.c_int32 * max(len(v), 1))(*v)


def views(n=2, h=8, w=8, c=1, codes=(0, 2), T=None, x=True, out=True):
    T = len(codes) if T is None else T
    return lib.ctl_tta_views(dummy() if x else None, n, h, w, c, codes_of(*codes) if codes is not None else None, T, dummy() if out else None, None)


def merge(T=None, n=2, h=8, w=8, c=4, codes=(0, 2), mode=_ffi.TTA_PROB, logits=True, outs=(True, True, True)):
    T = len(codes) if T is None else T
    a, m, p = (dummy() if o else None for o in outs)
    return lib.ctl_tta_merge(dummy() if logits else None, T, n, h, w, c, codes_of(*codes) if codes is not None else None, mode, a, m, p, None)


def test_entries_are_declared_exported_and_bound():
    header = open(os.path.join(ROOT, "include", "ctl_hip.h")).read()
    assert "test-time augmentation" in header
    raw = ctypes.CDLL(_ffi.LIB_PATH)
    for name in ENTRIES:
        assert re.search(r"\b%s\s*\(" % name, header), name
        assert hasattr(raw, name) and name in _ffi.SIGNATURES
        assert getattr(lib, name).argtypes is not None
    assert len(_ffi.SIGNATURES["ctl_tta_views"][1]) == 9 and len(_ffi.SIGNATURES["ctl_tta_merge"][1]) == 12
    for macro, value in (("CTL_TTA_MAX_VIEWS", _ffi.TTA_MAX_VIEWS), ("CTL_TTA_LOGIT", _ffi.TTA_LOGIT), ("CTL_TTA_PROB", _ffi.TTA_PROB)):
        assert int(re.search(r"#define\s+%s\s+(\d+)" % macro, header).group(1)) == value
    srcs = re.search(r"^SRCS\s*:=(.*)$", open(os.path.join(os.path.dirname(_ffi.LIB_PATH), "Makefile")).read(), re.M).group(1).split()
    assert "ctl_tta.hip" in srcs


def test_abi_version_is_still_11():
    header = open(os.path.join(ROOT, "include", "ctl_hip.h")).read()
    assert int(re.search(r"#define\s+CTL_ABI_VERSION\s+(\d+)", header).group(1)) == 11
    assert lib.ctl_version() == 11 == _ffi.ABI_VERSION


BAD = [
    ("views (1 .. 8)", dict(T=0)), ("views (1 .. 8)", dict(T=9, codes=(0, 1, 2, 3, 4, 5, 6, 7))), ("views (1 .. 8)", dict(T=-1)),
    ("view code 8", dict(codes=(0, 8))), ("view code -1", dict(codes=(-1,))),
    ("duplicate view code 2", dict(codes=(0, 2, 2))), ("duplicate view code 0", dict(codes=(0, 0))),
    ("channels", dict(c=0)), ("channels", dict(c=-3)),
    ("positive", dict(n=0)), ("positive", dict(h=0)), ("positive", dict(w=-4)),
    ("view code 3 transposes", dict(codes=(0, 3), h=8, w=9)), ("view code 1 transposes", dict(codes=(1,), h=5, w=7)),
    ("2 GiB", dict(n=1 << 12, h=1 << 10, w=1 << 10, c=1, codes=(0,))), ("2 GiB", dict(n=1, h=1 << 16, w=1 << 16, c=1, codes=(0,))),
    ("2 GiB", dict(n=(1 << 31) - 1, h=1 << 15, w=1 << 15, c=1, codes=(0,))),
    ("null pointer (codes)", dict(codes=None, T=2)),
]


@pytest.mark.parametrize("word,change", BAD, ids=lambda v: v if isinstance(v, str) else "-".join(f"{k}{x}" for k, x in v.items()))
def test_bad_arguments_are_refused_before_any_launch(word, change):
    for name, fn in (("tta_views", views), ("tta_merge", merge)):
        rc = fn(**change)
        msg = lib.ctl_last_error().decode()
        assert rc == -1 and name in msg and word in msg, (name, msg)
        with pytest.raises(_ffi.CtlError, match=name):
            _ffi.check(rc, "ctl_" + name)


def test_the_channel_ranges_differ():
    assert views(c=5) == -1 and "5 channels (1 .. 4)" in lib.ctl_last_error().decode()
    assert merge(c=17) == -1 and "17 channels (1 .. 16)" in lib.ctl_last_error().decode()
    # 2 GiB exactly is refused, one slice fewer is not a size error (T = 2, c = 16: 128 bytes per pixel)
    assert merge(n=1 << 12, h=64, w=64, c=16) == -1 and "2 GiB" in lib.ctl_last_error().decode()


def test_null_tensors_and_the_mode_are_refused_before_any_launch():
    assert views(x=False) == -1 and "null pointer" in lib.ctl_last_error().decode()
    assert views(out=False) == -1 and "null pointer" in lib.ctl_last_error().decode()
    assert merge(logits=False) == -1 and "null pointer (logits)" in lib.ctl_last_error().decode()
    assert merge(outs=(False, False, False)) == -1 and "no output" in lib.ctl_last_error().decode()
    for mode in (-1, 2):
        assert merge(mode=mode) == -1 and "mode" in lib.ctl_last_error().decode()
