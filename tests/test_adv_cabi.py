"""C-ABI of the adversarial input augmentation without a GPU: the entries of include/ctl_hip.h are exported and bound, the ABI version is
unchanged, every bad argument fails with -1 and a message that names it before anything is launched, the workspace sizes are what the
header says, and the Python layers check their arguments before they look at the device."""
import ctypes
import os
import re

import pytest
import torch

from cooperative_training_and_latent_space_data_augmentation_amd import _ffi, adversarial, autograd, ops, solver

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = {"ctl_adv_bias_ws_bytes": 4, "ctl_adv_bias_fwd": 12, "ctl_adv_bias_bwd": 15, "ctl_adv_unit_scale_ws_bytes": 2, "ctl_adv_unit_scale": 9}
lib = _ffi.lib
BUF, BUF2 = (ctypes.c_double * 1024)(), (ctypes.c_double * 1024)()      # larger than the tensors the calls below describe: no chance overlap
DUMMY = ctypes.cast(BUF, ctypes.c_void_p)                  # never dereferenced: every check fails before a launch
OTHER = ctypes.cast(BUF2, ctypes.c_void_p)
BIG = 1 << 40


def refused(rc, *words):
    msg = lib.ctl_last_error()
    assert rc == -1 and msg and all(w in msg for w in words), (rc, msg)


def fwd(x=DUMMY, theta=DUMMY, n=2, h=9, w=11, c=4, s=4, gh=6, gw=6, y=OTHER, f=None):
    return lib.ctl_adv_bias_fwd(x, theta, n, h, w, c, s, gh, gw, y, f, None)


def bwd(g=DUMMY, x=DUMMY, theta=DUMMY, n=2, h=9, w=11, c=4, s=4, gh=6, gw=6, ws=DUMMY, ws_bytes=BIG, dtheta=DUMMY, dx=None):
    return lib.ctl_adv_bias_bwd(g, x, theta, n, h, w, c, s, gh, gw, ws, ws_bytes, dtheta, dx, None)


def unit(g=DUMMY, n=2, m=100, norm=0, scale=1.0, ws=DUMMY, ws_bytes=BIG, out=OTHER):
    return lib.ctl_adv_unit_scale(g, n, m, norm, scale, ws, ws_bytes, out, None)


def test_symbols_are_declared_exported_and_bound():
    header = open(os.path.join(ROOT, "include", "ctl_hip.h")).read()
    declared = set(re.findall(r"\b(ctl_[a-z0-9_]+)\s*\(", header))
    raw = ctypes.CDLL(_ffi.LIB_PATH)
    for name, nargs in NEW.items():
        assert name in declared and name in _ffi.SIGNATURES and name in _ffi.EXPORTED and hasattr(raw, name), name
        assert len(getattr(lib, name).argtypes) == nargs == len(_ffi.SIGNATURES[name][1]), name
    assert int(re.search(r"#define\s+CTL_ABI_VERSION\s+(\d+)", header).group(1)) == 11 == lib.ctl_version() == _ffi.ABI_VERSION      # additive
    for k, name in enumerate(("CTL_ADV_L2", "CTL_ADV_RMS", "CTL_ADV_LINF")):
        assert re.search(name + r"\s*=\s*%d\b" % k, header), name
    assert (_ffi.ADV_L2, _ffi.ADV_RMS, _ffi.ADV_LINF) == (0, 1, 2)
    assert ops.ADV_NORMS == {"l2": 0, "rms": 1, "linf": 2} and tuple(ops.ADV_NORMS) == adversarial.NORMS
    assert "(ctl_adv.hip" in header
    for fn in (ops.adv_bias_fwd, ops.adv_bias_bwd, ops.adv_unit_scale, ops.adv_bias_grid, autograd.adv_bias_field, autograd.adv_unit_scale,
               adversarial.generate, solver.AdvancedTripletReconSegmentationModel.adversarial_example_generation,
               solver.AdvancedTripletReconSegmentationModel.adversarial_training):
        assert callable(fn)
    assert "ctl_adv.hip" in open(os.path.join(os.path.dirname(_ffi.LIB_PATH), "Makefile")).read()


def test_abi_version_is_still_11():
    assert lib.ctl_version() == 11 == _ffi.ABI_VERSION


def test_workspace_sizes_and_grid():
    for h, w, s in ((1, 1, 2), (5, 7, 4), (31, 65, 5), (33, 64, 32), (256, 256, 32), (192, 192, 32), (16, 16, 100), (2048, 2048, 2)):
        gh, gw = ops.adv_bias_grid(h, w, s)
        assert (gh, gw) == ((h - 1) // s + 4, (w - 1) // s + 4) == adversarial.bias_grid(h, w, s)
        for n in (1, 3, 16):
            assert lib.ctl_adv_bias_ws_bytes(n, h, w, s) == 8 * n * gw * h
    assert ops.adv_bias_grid(256, 256, 32) == (11, 11) and ops.adv_bias_grid(1, 1, 32) == (4, 4)
    for args in ((0, 9, 9, 4), (65536, 9, 9, 4), (2, 0, 9, 4), (2, 9, 2049, 4), (2, 9, 9, 1), (2, 9, 9, 0), (2, 9, 9, -3)):
        assert lib.ctl_adv_bias_ws_bytes(*args) == 0, args
    for n, m in ((1, 1), (3, 16384), (3, 16385), (16, 65536), (2, 121), (1, 16 * 2048 * 2048)):
        assert lib.ctl_adv_unit_scale_ws_bytes(n, m) == 8 * n * -(-m // 16384)
    for args in ((0, 5), (65536, 5), (2, 0), (2, -1), (2, 16 * 2048 * 2048 + 1)):
        assert lib.ctl_adv_unit_scale_ws_bytes(*args) == 0, args
    for bad in (1, 0, 2.5):
        with pytest.raises(ValueError, match="spacing"):
            ops.adv_bias_grid(9, 9, bad)


@pytest.mark.parametrize("call, who", [(fwd, b"adv_bias_fwd"), (bwd, b"adv_bias_bwd")])
def test_bias_refusals(call, who):
    before = lib.ctl_launch_count()
    nulls = (dict(x=None), dict(theta=None)) + ((dict(y=None),) if call is fwd else (dict(g=None), dict(ws=None), dict(dtheta=None)))
    for kw in nulls:
        refused(call(**kw), who, b"null")
    for s in (1, 0, -4):
        refused(call(s=s), who, b"spacing")
    for kw in (dict(gh=5), dict(gw=7), dict(gh=6, gw=6, s=5), dict(h=13), dict(gh=0, gw=0)):
        refused(call(**kw), who, b"grid")
    for n in (0, -1, 65536):
        refused(call(n=n), who, b"n = ", b"65535")
    for kw in (dict(h=2049, gh=516), dict(w=2049, gw=516), dict(h=0), dict(w=-3)):
        refused(call(**kw), who, b"plane")
    for c in (0, 17, -1):
        refused(call(c=c), who, b"c = ", b"channels")
    refused(call(n=65535, h=2048, w=2048, c=16, s=4, gh=515, gw=515), who, b"2^31")
    if call is fwd:
        refused(call(y=DUMMY), who, b"in place")                                        # y == x
        refused(call(y=ctypes.c_void_p(ctypes.addressof(BUF) + 64)), who, b"in place")    # y inside x
        refused(call(f=DUMMY), who, b"field")
    else:
        need = lib.ctl_adv_bias_ws_bytes(2, 9, 11, 4)
        assert need == 8 * 2 * 6 * 9
        refused(call(ws_bytes=need - 1), who, b"workspace", b"needed")
        refused(call(ws_bytes=0), who, b"workspace")
        refused(call(ws=ctypes.c_void_p(ctypes.addressof(BUF) + 4)), who, b"aligned")
        refused(call(dx=DUMMY), who, b"in place")                                       # dx == g == x
    assert lib.ctl_launch_count() == before, "a refused call launched something"
    with pytest.raises(_ffi.CtlError, match="channels"):
        _ffi.check(call(c=17), "ctl_adv")


def test_unit_scale_refusals():
    who = b"adv_unit_scale"
    before = lib.ctl_launch_count()
    for kw in (dict(g=None), dict(ws=None), dict(out=None)):
        refused(unit(**kw), who, b"null")
    for n in (0, -1, 65536):
        refused(unit(n=n), who, b"n = ")
    for m in (0, -5, 16 * 2048 * 2048 + 1):
        refused(unit(m=m), who, b"m = ")
    for norm in (-1, 3, 7):
        refused(unit(norm=norm), who, b"norm = ")
    for scale in (float("nan"), float("inf")):
        refused(unit(scale=scale), who, b"scale")
    refused(unit(m=16385, ws_bytes=8 * 2 * 2 - 1), who, b"workspace", b"needed")
    refused(unit(ws=ctypes.c_void_p(ctypes.addressof(BUF) + 4)), who, b"aligned")
    refused(unit(out=DUMMY), who, b"in place")
    assert lib.ctl_launch_count() == before, "a refused call launched something"


def test_python_layers_check_before_the_device():
    x = torch.zeros(2, 1, 16, 15).contiguous(memory_format=torch.channels_last)
    theta = torch.zeros(2, 7, 7)
    for call in (lambda: ops.adv_bias_fwd(x, theta, 4), lambda: ops.adv_bias_bwd(x, x, theta, 4), lambda: ops.adv_unit_scale(theta, 1.0, "linf"),
                 lambda: autograd.adv_bias_field(x, theta, 4), lambda: autograd.adv_unit_scale(x, 1.0, "rms")):
        with pytest.raises(_ffi.CtlError, match="device tensors"):       # no CPU fallback behind the kernels
            call()
    with pytest.raises(ValueError, match="norm"):
        ops.adv_unit_scale(theta, 1.0, "l1")
    with pytest.raises(ValueError, match="spacing"):
        ops.adv_bias_fwd(x, theta, 1)
