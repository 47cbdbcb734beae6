"""C-ABI boundary of the optimizer-tail entries (include/ctl_hip.h, csrc/ctl_optim.hip): declared, exported and bound; the ABI version
did not move; the workspace query; every bad argument is refused with -1 and a message before any launch (no GPU here)."""
import ctypes
import os
import re

import pytest

from cooperative_training_and_latent_space_data_augmentation_amd import _ffi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRIES = ("ctl_optim_control", "ctl_grad_norm_work", "ctl_grad_norm", "ctl_adam_tail")
lib = _ffi.lib
CH = _ffi.GRAD_NORM_CHUNK

dummy = ctypes.cast((ctypes.c_double * 64)(), ctypes.c_void_p)      # never dereferenced on the device: every check fails before a launch
lr8 = (ctypes.c_float * 8)(*([1e-4] * 8))
LR = ctypes.cast(lr8, ctypes.c_void_p)


def _counts(*v):
    arr = (ctypes.c_int64 * len(v))(*v)
    return arr, ctypes.cast(arr, ctypes.c_void_p)


def _ptrs(n, null_at=None):
    arr = (ctypes.c_void_p * n)(*[None if j == null_at else dummy.value for j in range(n)])
    return arr, ctypes.cast(arr, ctypes.c_void_p)


def _refused(rc, who, word):
    msg = lib.ctl_last_error().decode()
    assert rc == -1 and who in msg and word in msg, (rc, msg)
    with pytest.raises(_ffi.CtlError, match=who):
        _ffi.check(rc, "ctl_" + who)


def test_entries_are_declared_exported_and_bound():
    header = open(os.path.join(ROOT, "include", "ctl_hip.h")).read()
    assert "optimizer tail" in header
    raw = ctypes.CDLL(_ffi.LIB_PATH)
    for name in ENTRIES:
        assert re.search(r"\b%s\s*\(" % name, header), name
        assert hasattr(raw, name) and name in _ffi.SIGNATURES
        assert getattr(lib, name).argtypes is not None
    assert _ffi.SIGNATURES["ctl_grad_norm_work"][0] is ctypes.c_size_t
    assert len(_ffi.SIGNATURES["ctl_adam_tail"][1]) == 15
    for name, value in (("CTRL_DOUBLES", 32), ("MAX_NETS", 8), ("LR", 0), ("MAX_NORM", 8), ("GUARD", 9), ("EMA_OMD", 10), ("SUMSQ", 16),
                        ("NORM", 17), ("CLIP", 18), ("FINITE", 19), ("SKIPPED", 20)):
        assert int(re.search(r"#define\s+CTL_OPTIM_%s\s+(\d+)" % name, header).group(1)) == value == getattr(_ffi, "OPTIM_" + name)
    assert int(re.search(r"#define\s+CTL_GRAD_NORM_CHUNK\s+(\d+)", header).group(1)) == CH


def test_abi_version_is_still_11():
    header = open(os.path.join(ROOT, "include", "ctl_hip.h")).read()
    assert int(re.search(r"#define\s+CTL_ABI_VERSION\s+(\d+)", header).group(1)) == 11
    assert lib.ctl_version() == 11 == _ffi.ABI_VERSION


def test_grad_norm_workspace_sizing():
    work = lambda *v: lib.ctl_grad_norm_work(_counts(*v)[1], len(v))      # noqa: E731
    assert [work(n) for n in (1, 63, CH - 1, CH, CH + 1, 3 * CH + 7)] == [1, 1, 1, 1, 2, 4]
    assert work(1, 3 * CH + 7, CH, 65, CH + 1) == 1 + 4 + 1 + 1 + 2          # one partial per chunk per buffer, buffers in order
    assert work(*([5 * CH] * 8)) == 40
    assert work(1 << 33) == (1 << 33) // CH                                 # counts past 2^31 are sized in 64 bits
    assert work(4, 0) == 0 and work(-3) == 0                                # a bad count
    assert lib.ctl_grad_norm_work(None, 1) == 0
    c9 = _counts(*([4] * 9))
    assert lib.ctl_grad_norm_work(c9[1], 9) == 0 and lib.ctl_grad_norm_work(c9[1], 0) == 0


def test_optim_control_refuses_bad_arguments():
    _refused(lib.ctl_optim_control(None, 5, LR, 0.0, 0, 0.0, None), "optim_control", "null")
    _refused(lib.ctl_optim_control(dummy, 5, None, 0.0, 0, 0.0, None), "optim_control", "null")
    for k in (0, 9, -1):
        _refused(lib.ctl_optim_control(dummy, k, LR, 0.0, 0, 0.0, None), "optim_control", "1 <= k <= 8")
    for mn in (-1.0, float("inf"), float("nan")):
        _refused(lib.ctl_optim_control(dummy, 5, LR, mn, 0, 0.0, None), "optim_control", "max_norm")
    for omd in (-0.1, 1.5, float("nan")):
        _refused(lib.ctl_optim_control(dummy, 5, LR, 0.0, 0, omd, None), "optim_control", "ema_omd")


def test_grad_norm_refuses_bad_arguments():
    cnt, cp = _counts(4, 4, 4)
    arr, gp = _ptrs(3)
    _refused(lib.ctl_grad_norm(None, cp, 3, 1.0, dummy, dummy, None), "grad_norm", "null")
    _refused(lib.ctl_grad_norm(gp, None, 3, 1.0, dummy, dummy, None), "grad_norm", "null")
    _refused(lib.ctl_grad_norm(gp, cp, 3, 1.0, None, dummy, None), "grad_norm", "null")
    _refused(lib.ctl_grad_norm(gp, cp, 3, 1.0, dummy, None, None), "grad_norm", "null")
    for k in (0, 9):
        _refused(lib.ctl_grad_norm(gp, cp, k, 1.0, dummy, dummy, None), "grad_norm", "1 <= k <= 8")
    arr2, gp2 = _ptrs(3, null_at=2)
    _refused(lib.ctl_grad_norm(gp2, cp, 3, 1.0, dummy, dummy, None), "grad_norm", "buffer 2")
    for bad in (0, -7):
        cnt2, cp2 = _counts(4, bad, 4)
        _refused(lib.ctl_grad_norm(gp, cp2, 3, 1.0, dummy, dummy, None), "grad_norm", "count of buffer 1")
    _refused(lib.ctl_grad_norm(gp, cp, 3, 1.0, dummy.value + 4, dummy, None), "grad_norm", "aligned")


def test_adam_tail_refuses_bad_arguments():
    ok = dict(p=dummy, g=dummy, m=dummy, v=dummy, ema=None, count=16, state=None, step=1, ctrl=dummy, net=0)

    def tail(**change):
        a = dict(ok, **change)
        return lib.ctl_adam_tail(a["p"], a["g"], a["m"], a["v"], a["ema"], a["count"], 0.9, 0.999, 1e-8, a["state"], a["step"], 1.0,
                                 a["ctrl"], a["net"], None)

    for name in ("p", "g", "m", "v", "ctrl"):
        _refused(tail(**{name: None}), "adam_tail", "null")
    for count in (0, -1):
        _refused(tail(count=count), "adam_tail", "count")
    for net in (8, -1, 100):                               # a record holds 8 networks: net >= k is out of it
        _refused(tail(net=net), "adam_tail", "net")
    _refused(tail(step=0), "adam_tail", "step")
