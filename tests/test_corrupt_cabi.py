"""C-ABI of the MR artefact corruption without a GPU: the entries of include/ctl_hip.h ("MR artefact corruption") are exported and
bound, the workspace query follows its formula, and every bad argument fails with -1 and a message before anything is launched."""
import ctypes
import os
import re

import numpy as np
import pytest

from cooperative_training_and_latent_space_data_augmentation_amd import _ffi, corrupt, ops

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ["ctl_corrupt_bias", "ctl_corrupt_spike_ws_bytes", "ctl_corrupt_spike", "ctl_corrupt_rigid3d", "ctl_axis_operator"]
lib = _ffi.lib
DUMMY = ctypes.cast((ctypes.c_float * 256)(), ctypes.c_void_p)           # never dereferenced: every check fails before a launch
OTHER = ctypes.cast((ctypes.c_float * 256)(), ctypes.c_void_p)
THIRD = ctypes.cast((ctypes.c_float * 256)(), ctypes.c_void_p)
BIG = 1 << 20                                                            # a workspace size that is never the reason of a refusal
COEF = np.zeros(20, dtype=np.float32)


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
    for fn in ("corrupt_bias_field", "corrupt_spike", "corrupt_rigid3d", "axis_operator"):
        assert callable(getattr(ops, fn)), fn
    for fn in ("bias_field", "spike", "ghosting", "motion", "bias_field_host", "spike_host", "ghosting_host", "motion_host", "draw_parameters",
               "corrupt_volume", "CorruptedDataset"):
        assert callable(getattr(corrupt, fn)), fn


def test_workspace_query():
    for (d, h, w), n in (((1, 1, 1), 1), ((3, 5, 7), 2), ((10, 192, 192), 1), ((40, 256, 256), 8), ((1, 1, 2049), 3)):
        blocks = min(-(-d * h * w // 2048), 256)
        assert lib.ctl_corrupt_spike_ws_bytes(d, h, w, n) == blocks * (1 + 2 * n) * 8
    for d, h, w, n in ((0, 4, 4, 1), (4, -1, 4, 1), (4, 4, 0, 1), (4, 4, 4, 0), (4, 4, 4, 9), (1 << 10, 1 << 10, 1 << 9, 1)):
        assert lib.ctl_corrupt_spike_ws_bytes(d, h, w, n) == 0


def test_bias_refusals():
    def call(x=DUMMY, coef=COEF, d=2, h=4, w=8, out=OTHER):
        return lib.ctl_corrupt_bias(x, None if coef is None else coef.ctypes.data, d, h, w, out, None)

    refused(call(x=None), b"null")
    refused(call(coef=None), b"null")
    refused(call(out=None), b"null")
    for kw in (dict(d=0), dict(h=-1), dict(w=0)):
        refused(call(**kw), b"sizes")
    refused(call(d=1 << 10, h=1 << 10, w=1 << 9), b"2 GiB")
    refused(call(out=DUMMY), b"aliases")
    refused(call(out=ctypes.c_void_p(DUMMY.value + 40)), b"aliases")
    bad = COEF.copy()
    bad[7] = np.nan
    refused(call(coef=bad), b"coefficient 7")
    bad[7] = np.inf
    refused(call(coef=bad), b"coefficient 7")


def test_spike_refusals():
    def call(x=DUMMY, d=2, h=4, w=8, k=(1, 2, 3), mult=(2,), n=1, intensity=2.0, out=OTHER, ws=THIRD, ws_bytes=BIG):
        ka = None if k is None else np.array(k, dtype=np.int32)
        ma = None if mult is None else np.array(mult, dtype=np.int32)
        return lib.ctl_corrupt_spike(x, d, h, w, None if ka is None else ka.ctypes.data, None if ma is None else ma.ctypes.data, n, intensity,
                                     out, ws, ws_bytes, None)

    for kw in (dict(x=None), dict(k=None), dict(mult=None), dict(out=None), dict(ws=None)):
        refused(call(**kw), b"null")
    for kw in (dict(d=0), dict(h=0), dict(w=-3)):
        refused(call(**kw), b"sizes")
    refused(call(d=1 << 10, h=1 << 10, w=1 << 9), b"2 GiB")
    refused(call(n=0), b"n_spikes 0")
    refused(call(n=9, k=(0,) * 27, mult=(1,) * 9), b"n_spikes 9")
    refused(call(intensity=float("nan")), b"intensity")
    refused(call(out=DUMMY), b"aliases")
    refused(call(k=(2, 0, 0)), b"wave number 2", b"axis 0")
    refused(call(k=(0, -1, 0)), b"wave number -1", b"axis 1")
    refused(call(k=(0, 0, 0, 1, 3, 8), mult=(1, 2), n=2), b"wave number 8", b"spike 1")
    refused(call(k=(1, 2, 4), mult=(2,)), b"multiplicity 2")                # (1, 2, 4) of (2, 4, 8) is its own mirror image
    refused(call(k=(1, 2, 3), mult=(1,)), b"multiplicity 1")
    refused(call(mult=(0,)), b"multiplicity 0")
    need = lib.ctl_corrupt_spike_ws_bytes(2, 4, 8, 1)
    assert need == 24
    refused(call(ws_bytes=need - 1), b"workspace")
    refused(call(ws=ctypes.c_void_p(THIRD.value + 4)), b"8-byte")
    with pytest.raises(_ffi.CtlError, match="n_spikes 0"):
        _ffi.check(call(n=0), "ctl_corrupt_spike")


def test_rigid_refusals():
    eye = np.tile(np.eye(3, 4, dtype=np.float32), (8, 1, 1))

    def call(x=DUMMY, d=2, h=4, w=4, m=eye, copies=2, out=OTHER):
        return lib.ctl_corrupt_rigid3d(x, d, h, w, None if m is None else m.ctypes.data, copies, out, None)

    for kw in (dict(x=None), dict(m=None), dict(out=None)):
        refused(call(**kw), b"null")
    for kw in (dict(d=0), dict(h=0), dict(w=-1)):
        refused(call(**kw), b"sizes")
    refused(call(copies=0), b"copies 0")
    refused(call(copies=9), b"copies 9")
    refused(call(d=1 << 10, h=1 << 10, w=1 << 9, copies=1), b"2 GiB")
    refused(call(d=1 << 9, h=1 << 9, w=1 << 9, copies=4), b"2 GiB")          # 2^27 floats each: the four copies reach the limit
    refused(call(out=DUMMY), b"aliases")
    refused(call(out=ctypes.c_void_p(DUMMY.value - 4 * 40)), b"aliases")      # the second copy lands on x
    bad = eye.copy()
    bad[1, 2, 3] = np.nan
    refused(call(m=bad), b"entry 11 of copy 1")


def test_axis_operator_refusals():
    def call(x0=DUMMY, xs=None, n_vol=1, d=2, h=4, w=4, axis=2, matrix=THIRD, out=OTHER):
        return lib.ctl_axis_operator(x0, xs, n_vol, d, h, w, axis, matrix, out, None)

    for kw in (dict(x0=None), dict(matrix=None), dict(out=None)):
        refused(call(**kw), b"null")
    refused(call(n_vol=2), b"null", b"stack")                               # two volumes without the stack
    for kw in (dict(d=0), dict(h=0), dict(w=-1)):
        refused(call(**kw), b"sizes")
    refused(call(axis=3), b"axis 3")
    refused(call(axis=-1), b"axis -1")
    refused(call(n_vol=0), b"n_volumes 0")
    refused(call(n_vol=10, xs=OTHER), b"n_volumes 10")
    refused(call(d=1 << 10, h=1 << 10, w=1 << 9), b"2 GiB")
    refused(call(d=1 << 9, h=1 << 9, w=1 << 9, n_vol=5, xs=OTHER), b"2 GiB")         # the stack of four
    refused(call(d=1, h=1, w=1 << 15, n_vol=1), b"2 GiB")                    # the matrix: 2^30 floats
    refused(call(out=DUMMY), b"aliases")
    refused(call(n_vol=2, xs=OTHER, out=ctypes.c_void_p(OTHER.value + 16)), b"aliases")


def test_python_layer_refuses_host_tensors_and_bad_arguments():
    import torch
    x = torch.zeros(2, 4, 4)
    for call in (lambda: ops.corrupt_bias_field(x, COEF), lambda: ops.corrupt_spike(x, [[0, 0, 0]], [1], 2.0),
                 lambda: ops.corrupt_rigid3d(x, np.eye(3, 4)[None]), lambda: ops.axis_operator(x, torch.zeros(4, 4), 2)):
        with pytest.raises(_ffi.CtlError):
            call()
    for kind in ("RandomBlur", "randombias"):
        with pytest.raises(ValueError):
            corrupt.Corruption(kind, {}, (2, 4, 4), device="cpu")
    with pytest.raises(ValueError):
        corrupt.Corruption("RandomBias", {"coefficients": [0.0] * 20}, (2, 4), device="cpu")
