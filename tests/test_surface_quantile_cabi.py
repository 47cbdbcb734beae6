"""CPU-side checks of ctl_surface_quantiles / ctl_surface_quantiles_ws_bytes: declared, exported, bound, workspace sizing, and every
argument error refused with a message that names the entry before anything touches a device."""
import ctypes
import os
import re

import pytest

from cooperative_training_and_latent_space_data_augmentation_amd import _ffi
from test_surface_cabi import STATS_ERRORS

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("ctl_surface_quantiles_ws_bytes", "ctl_surface_quantiles")


def test_entries_are_declared_exported_and_bound():
    header = open(os.path.join(ROOT, "include", "ctl_hip.h")).read()
    declared = set(re.findall(r"\b(ctl_[a-z0-9_]+)\s*\(", header))
    raw = ctypes.CDLL(_ffi.LIB_PATH)
    for name in NAMES:
        assert name in declared, name
        assert hasattr(raw, name), name
        assert name in _ffi.EXPORTED, name
        assert getattr(_ffi.lib, name).argtypes is not None, name
    assert len(_ffi.lib.ctl_surface_quantiles_ws_bytes.argtypes) == 7 and len(_ffi.lib.ctl_surface_quantiles.argtypes) == 17
    assert _ffi.lib.ctl_surface_quantiles_ws_bytes.restype is ctypes.c_size_t
    for ref in ("measure.py:402-455", "metrics.py:226-233"):         # the reference lines the entries follow
        assert ref in header, ref


def test_abi_version_stays_11():
    header = open(os.path.join(ROOT, "include", "ctl_hip.h")).read()
    assert re.search(r"#define\s+CTL_ABI_VERSION\s+11\b", header)
    assert _ffi.ABI_VERSION == 11 and _ffi.lib.ctl_version() == 11


def test_workspace_query():
    qws, sws = _ffi.lib.ctl_surface_quantiles_ws_bytes, _ffi.lib.ctl_surface_stats_ws_bytes
    for mode in (2, 3):
        for fg in (0, 1):
            last = 0
            for d, h, w in ((1, 1, 1), (1, 37, 53), (7, 37, 53), (10, 192, 192), (40, 256, 256), (40, 520, 300)):
                b = qws(d, h, w, 4, fg, mode, 1)
                assert b > last, (mode, d, h, w, b)
                assert b % 256 == 0
                assert b >= sws(d, h, w, 4, fg, mode) + 16 * d * h * w          # one 64-bit key per surface voxel of either side
                assert qws(d, h, w, 4, fg, mode, 4) >= b
                last = b
    for bad in ((0, 8, 8, 4, 0, 2, 1), (8, -1, 8, 4, 0, 2, 1), (8, 8, 0, 4, 0, 3, 1), (8, 8, 8, 1, 0, 2, 1), (8, 8, 8, 256, 0, 2, 1),
                (8, 8, 8, 4, 0, 1, 1), (8, 8, 8, 4, 0, 4, 1), (8, 8, 8, 4, 0, 2, 0), (8, 8, 8, 4, 0, 2, 5), (8, 8, 8, 4, 0, 3, -1),
                (8, 8, 65535, 4, 0, 2, 1)):
        assert qws(*bad) == 0, bad


def _dummy():
    buf = (ctypes.c_double * 64)()                     # never dereferenced: every call below fails its argument check first
    return buf, ctypes.cast(buf, ctypes.c_void_p)


def _call(pred, gt, table, ws, q=(95.0,), n_q=None, stats=None, d=4, h=8, w=8, n=4, fg=0, mode=2, conn=2, sampling=None, ws_bytes=1 << 30):
    """`table` is the required output, q_table: the names of STATS_ERRORS apply unchanged."""
    samp = None if sampling is None else (ctypes.c_double * len(sampling))(*sampling)
    qa = None if q is None else (ctypes.c_double * max(len(q), 1))(*q)
    n_q = (0 if q is None else len(q)) if n_q is None else n_q
    return _ffi.lib.ctl_surface_quantiles(pred, gt, d, h, w, n, fg, mode, conn, samp, qa, n_q, stats, table, ws, ws_bytes, None)


QUANTILE_ERRORS = dict(STATS_ERRORS)
QUANTILE_ERRORS.update({
    "null q": dict(q=None, n_q=1), "null q_table": dict(table=None),
    "n_q = 0": dict(q=(), n_q=0), "n_q = 5": dict(q=(1.0, 2.0, 3.0, 4.0, 5.0)),
    "q = -1": dict(q=(-1.0,)), "q = 100.5": dict(q=(50.0, 100.5)), "q nan": dict(q=(float("nan"),)), "q inf": dict(q=(95.0, float("inf"))),
    "q = -inf": dict(q=(float("-inf"),)),
})


def test_the_error_cases_include_every_stats_case():
    assert set(STATS_ERRORS) <= set(QUANTILE_ERRORS) and len(QUANTILE_ERRORS) == len(STATS_ERRORS) + 9
    for name in ("null pred", "null gt", "null table", "null workspace", "short workspace"):
        assert name in QUANTILE_ERRORS


@pytest.mark.parametrize("with_stats", [False, True], ids=["no_stats", "stats"])
@pytest.mark.parametrize("case", sorted(QUANTILE_ERRORS))
def test_surface_quantiles_argument_errors(case, with_stats):
    keep, p = _dummy()
    args = dict(pred=p, gt=p, table=p, ws=p, stats=p if with_stats else None)
    args.update(QUANTILE_ERRORS[case])
    before = _ffi.lib.ctl_launch_count()
    rc = _call(**args)
    msg = _ffi.lib.ctl_last_error()
    assert rc == -1 and msg and b"surface_quantiles" in msg, (case, rc, msg)
    assert _ffi.lib.ctl_launch_count() == before                    # refused before anything is launched
    with pytest.raises(_ffi.CtlError):
        _ffi.check(rc, "ctl_surface_quantiles")
