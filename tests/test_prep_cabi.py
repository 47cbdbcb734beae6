"""C-ABI of the volume preparation without a GPU: the entries of include/ctl_hip.h ("volume preparation") are exported and bound,
the workspace query follows its formula, and every bad argument fails with -1 and a message before anything is launched."""
import ctypes
import os
import re

import numpy as np
import pytest

from cooperative_training_and_latent_space_data_augmentation_amd import _ffi, ops, prepare

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ["ctl_order_stats_ws_bytes", "ctl_order_stats", "ctl_percentile_apply", "ctl_resample_inplane"]
lib = _ffi.lib
DUMMY = ctypes.cast((ctypes.c_float * 64)(), ctypes.c_void_p)            # never dereferenced: every check fails before a launch
OTHER = ctypes.cast((ctypes.c_float * 64)(), ctypes.c_void_p)
BIG = 1 << 20                                                            # a workspace size that is never the reason of a refusal


def ranks(*v):
    return np.array(v, dtype=np.int64)


def refused(rc, *words):
    msg = lib.ctl_last_error()
    assert rc == -1 and msg and all(w in msg for w in words), (rc, msg)


def test_symbols_are_declared_exported_and_bound():
    header = open(os.path.join(ROOT, "include", "ctl_hip.h")).read()
    declared = set(re.findall(r"\b(ctl_[a-z0-9_]+)\s*\(", header))
    raw = ctypes.CDLL(_ffi.LIB_PATH)
    for name in NEW:
        assert name in declared and name in _ffi.EXPORTED and hasattr(raw, name), name
        assert getattr(lib, name).argtypes is not None, name
    assert int(re.search(r"#define\s+CTL_ABI_VERSION\s+(\d+)", header).group(1)) == 11 == lib.ctl_version()      # additive: no bump
    for fn in ("order_statistics", "percentile", "percentile_normalize", "resample_inplane"):
        assert callable(getattr(ops, fn)), fn
    for fn in ("load_volume", "prepare_patient", "percentile_host", "percentile_normalize_host", "resample_inplane_host", "prepare_patient_host"):
        assert callable(getattr(prepare, fn)), fn


def test_workspace_query():
    for segments, n_rank in ((1, 1), (1, 4), (10, 4), (7, 8), (65535, 8)):
        assert lib.ctl_order_stats_ws_bytes(segments, n_rank) == segments * 256 * (128 + 3 * n_rank) * 4
    for segments, n_rank in ((0, 4), (-1, 4), (65536, 4), (1, 0), (1, 9), (1, -1)):
        assert lib.ctl_order_stats_ws_bytes(segments, n_rank) == 0


def test_order_stats_refusals():
    r = ranks(0, 5, 5, 99)
    for x, rk, out, ws in ((None, r, DUMMY, DUMMY), (DUMMY, None, DUMMY, DUMMY), (DUMMY, r, None, DUMMY), (DUMMY, r, DUMMY, None)):
        refused(lib.ctl_order_stats(x, 1, 100, None if rk is None else rk.ctypes.data, 4, out, ws, BIG, None), b"null")
    r9 = ranks(*range(9))
    refused(lib.ctl_order_stats(DUMMY, 1, 100, r9.ctypes.data, 0, OTHER, DUMMY, BIG, None), b"n_rank 0")
    refused(lib.ctl_order_stats(DUMMY, 1, 100, r9.ctypes.data, 9, OTHER, DUMMY, BIG, None), b"n_rank 9")
    refused(lib.ctl_order_stats(DUMMY, 1, 100, ranks(0, 100).ctypes.data, 2, OTHER, DUMMY, BIG, None), b"rank 100", b"entry 1")
    refused(lib.ctl_order_stats(DUMMY, 1, 100, ranks(-1).ctypes.data, 1, OTHER, DUMMY, BIG, None), b"rank -1")
    refused(lib.ctl_order_stats(DUMMY, 4, 25, ranks(25).ctypes.data, 1, OTHER, DUMMY, BIG, None), b"rank 25")          # per segment, not per array
    refused(lib.ctl_order_stats(DUMMY, 0, 100, r.ctypes.data, 4, OTHER, DUMMY, BIG, None), b"segments")
    refused(lib.ctl_order_stats(DUMMY, 65536, 100, r.ctypes.data, 4, OTHER, DUMMY, 1 << 40, None), b"segments")
    refused(lib.ctl_order_stats(DUMMY, 1, 0, r.ctypes.data, 4, OTHER, DUMMY, BIG, None), b"segments")
    refused(lib.ctl_order_stats(DUMMY, 2, 1 << 28, r.ctypes.data, 4, OTHER, DUMMY, BIG, None), b"2 GiB")             # 2 * 2^28 * 4 = 2^31 bytes
    refused(lib.ctl_order_stats(DUMMY, 1, 1 << 29, r.ctypes.data, 4, OTHER, DUMMY, BIG, None), b"2 GiB")
    need = lib.ctl_order_stats_ws_bytes(1, 4)
    refused(lib.ctl_order_stats(DUMMY, 1, 100, r.ctypes.data, 4, OTHER, DUMMY, need - 1, None), b"workspace")
    with pytest.raises(_ffi.CtlError, match="n_rank 9"):
        _ffi.check(lib.ctl_order_stats(DUMMY, 1, 100, r9.ctypes.data, 9, OTHER, DUMMY, BIG, None), "ctl_order_stats")


def test_percentile_apply_refusals():
    ok = dict(segments=1, seg_elems=100, g_lo=0.25, g_hi=0.5, form=0)

    def call(x=DUMMY, table=DUMMY, out=OTHER, bounds=None, **kw):
        a = dict(ok, **kw)
        return lib.ctl_percentile_apply(x, table, a["segments"], a["seg_elems"], a["g_lo"], a["g_hi"], a["form"], 0.0, 1.0, out, bounds, None)

    refused(call(x=None), b"null")
    refused(call(table=None), b"null")
    refused(call(out=None), b"null")
    refused(call(out=DUMMY), b"aliases")                                   # out is x
    shifted = ctypes.c_void_p(DUMMY.value + 40)                            # overlaps x's 100 floats
    refused(call(out=shifted), b"aliases")
    refused(call(form=2), b"form 2")
    refused(call(segments=0), b"segments")
    refused(call(seg_elems=0), b"segments")
    refused(call(segments=2, seg_elems=1 << 28), b"2 GiB")
    refused(call(g_lo=1.0), b"weights")
    refused(call(g_hi=-0.5), b"weights")
    refused(call(g_lo=float("nan")), b"weights")


def test_resample_refusals():
    def call(image=DUMMY, label=None, label_bytes=0, n=2, h=8, w=8, nh=10, nw=10, rh=0.8, rw=0.8, image_out=OTHER, label_out=None):
        return lib.ctl_resample_inplane(image, label, label_bytes, n, h, w, nh, nw, rh, rw, image_out, label_out, None)

    refused(call(image=None), b"null")
    refused(call(image_out=None), b"null")
    refused(call(label=DUMMY, label_bytes=8), b"null")                     # a label without its output
    for kw in (dict(n=0), dict(h=0), dict(w=-1), dict(nh=0), dict(nw=0)):
        refused(call(**kw), b"sizes")
    for kw in (dict(rh=0.0), dict(rw=-1.0), dict(rh=float("inf")), dict(rw=float("nan"))):
        refused(call(**kw), b"ratios")
    refused(call(label=DUMMY, label_out=OTHER, label_bytes=4), b"element size 4")
    refused(call(n=1 << 10, h=1 << 10, w=1 << 9), b"2 GiB")                 # 2^29 floats in
    refused(call(n=1 << 10, nh=1 << 10, nw=1 << 9), b"2 GiB")               # 2^29 floats out
    refused(call(image=None, image_out=None, label=DUMMY, label_out=OTHER, label_bytes=8, n=1 << 10, h=1 << 9, w=1 << 9), b"2 GiB")      # int64: 2^28


def test_python_layer_refuses_host_tensors_and_bad_arguments():
    import torch
    x = torch.zeros(4, 4)
    for call in (lambda: ops.order_statistics(x, [0]), lambda: ops.percentile(x, [50]), lambda: ops.percentile_normalize(x),
                 lambda: ops.resample_inplane(x[None], (1, 1, 1), (2, 2, -1))):
        with pytest.raises(_ffi.CtlError):
            call()
    with pytest.raises(ValueError):
        ops.percentile_normalize(x, form="zscore")
    with pytest.raises(NotImplementedError):
        ops.resample_geometry(2, 8, 8, (1, 1, 1), (2, 2, 2))
