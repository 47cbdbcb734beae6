"""Host-side identity gate of the conv launch code (csrc/ctl_conv_host.h and the five conv units): what the library ANSWERS for a
descriptor, and what it REFUSES, as deterministic text on stdout.  Nothing is launched.

A refactor of the host side leaves the output unchanged: run it on both trees (`python tools/host_dispatch_digest.py > a.txt`) and `cmp`
the files.  Like tools/plan_digest.py this is not a golden file: every tuning of a tile or split heuristic changes it, and without a GPU
the occupancy queries answer with a constant, so grids and split counts are the real ones only on one.

Part 1, sizing: one line per descriptor with ctl_conv_stats_blocks, ctl_conv_stats_floats, ctl_conv_pool_ok, ctl_wgrad_splits,
ctl_wgrad_partial_floats, ctl_wgrad_bias_partial_floats and ctl_wgrad_group_class without / with a second output-gradient tensor, then
ctl_wgrad_group_plan over groups of 1, 2, 5 and 8 members.  The descriptors are every THIN-th row (a prime, so that every value of every
axis is met) of the product of
    dt         0 | X3 | BF16+X16+Y16+RES16 | BF16 with fp32-stored x | BF16+X16 with fp32-stored y
    shape      every (ks, stride, pad, in_mode, nsub) the library accepts, and five it refuses
    cin, cout  1 4 8 12 16 24 32 64 128 256        n  1 2 16 32        hout = wout  3 7 8 16 17 64 256        groups  1 2 4
    epilogue   none | RES | ACCUM | STATS | BNBWD+STATS | TAILBWD+STATS                                      pro_affine  0 1 2

Part 2, refusals (only where no GPU is visible: there a call that is not refused ends in a launch error instead of a launch): the return
code and ctl_last_error() of ctl_conv_forward_ex, ctl_conv_wgrad_ex, ctl_conv_wgrad_group and ctl_plan_run over malformed calls with
dummy pointers."""
import ctypes
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from cooperative_training_and_latent_space_data_augmentation_amd import _ffi        # noqa: E402

lib = _ffi.lib
P, U, Z, C4 = _ffi.IN_PLAIN, _ffi.IN_UP2, _ffi.IN_ZINS2, _ffi.IN_C4
B16 = _ffi.DT_BF16
DTS = [0, _ffi.DT_X3, B16 | _ffi.DT_X16 | _ffi.DT_Y16 | _ffi.DT_RES16, B16 | _ffi.DT_Y16 | _ffi.DT_RES16, B16 | _ffi.DT_X16]
SHAPES = [(3, 1, 1, P, 1), (3, 1, 1, U, 1), (3, 1, 1, Z, 1), (3, 1, 1, C4, 1), (3, 1, 1, P, 4), (3, 2, 1, P, 1), (1, 1, 0, P, 1), (1, 1, 0, U, 1),
          (1, 1, 0, C4, 1), (2, 2, 0, P, 1), (4, 2, 1, P, 1), (2, 1, 0, P, 4), (2, 1, 2, P, 4),
          (3, 2, 1, U, 1), (1, 1, 0, Z, 1), (2, 1, 0, P, 1), (5, 1, 2, P, 1), (3, 1, 0, P, 1)]      # (the last five are refused)
CH = [1, 4, 8, 12, 16, 24, 32, 64, 128, 256]
NS = [1, 2, 16, 32]
HW = [3, 7, 8, 16, 17, 64, 256]
GROUPS = [1, 2, 4]
S = _ffi.EPI_STATS
EPIS = [0, _ffi.EPI_RES, _ffi.EPI_ACCUM, S, _ffi.EPI_BNBWD | S, _ffi.EPI_TAILBWD | S]
PRO = [0, 1, 2]
AXES = [DTS, SHAPES, CH, CH, NS, HW, GROUPS, EPIS, PRO]
THIN = 53


def hin_of(hout, stride, in_mode):
    if in_mode in (U, Z):
        return max(1, hout // 2)
    return hout * stride


def matrix():
    dims = [len(a) for a in AXES]
    total = int(np.prod(dims))
    idx = np.arange(0, total, THIN)
    coords = np.unravel_index(idx, dims)
    descs = np.zeros(len(idx), dtype=_ffi.CONV_DTYPE)
    for r, c in enumerate(zip(*coords)):
        dt, (ks, stride, pad, in_mode, nsub), cin, cout, n, hw, groups, epi, pro = (a[i] for a, i in zip(AXES, c))
        d = _ffi.conv_desc(n=n, hin=hin_of(hw, stride, in_mode), win=hin_of(hw, stride, in_mode), cin=cin, hout=hw, wout=hw, cout=cout, ks=ks, stride=stride,
                           pad=pad, in_mode=in_mode, nsub=nsub, groups=groups, epi_flags=epi, pro_affine=pro, pro_slope=0.2, dt=dt)
        if nsub == 4:
            d["out_h"] = d["out_w"] = 2 * hw
            d["out_sy"] = d["out_sx"] = 2
        descs[r] = d
    return descs


def sizing(descs):
    base, step = descs.ctypes.data, descs.dtype.itemsize
    classes = {}
    for r in range(len(descs)):
        p = base + r * step
        d = descs[r]
        ans = (lib.ctl_conv_stats_blocks(p), lib.ctl_conv_stats_floats(p), lib.ctl_conv_pool_ok(p), lib.ctl_wgrad_splits(p),
               lib.ctl_wgrad_partial_floats(p), lib.ctl_wgrad_bias_partial_floats(p), lib.ctl_wgrad_group_class(p, 0), lib.ctl_wgrad_group_class(p, 1))
        print("S", int(d["dt"]), *(int(d[k]) for k in ("ks", "stride", "pad", "in_mode", "nsub", "cin", "cout", "n", "hout", "groups", "epi_flags", "pro_affine")),
              "|", *ans)
        for two in (0, 1):
            if ans[6 + two] >= 0:
                classes.setdefault((int(d["dt"]), two, ans[6 + two]), []).append(r)
    print(f"# {len(descs)} descriptors", file=sys.stderr)
    return classes


def plan(descs, label, rows):
    grp = np.ascontiguousarray(descs[rows])
    splits = np.full(len(rows), -7, dtype=np.int32)
    rc = lib.ctl_wgrad_group_plan(grp.ctypes.data, len(rows), splits.ctypes.data)
    print("G", label, rows, "|", rc, *(splits.tolist() if rc == 0 else [lib.ctl_last_error().decode()]))


def group_plans(descs, classes):
    for key in sorted(classes):
        rows = classes[key]
        for size in (1, 2, 5, 8):
            for start in (0, len(rows) // 3, len(rows) - size):
                if 0 <= start and start + size <= len(rows):
                    plan(descs, f"class {key} x{size}", rows[start:start + size])
            plan(descs, f"class {key} x{size} spread", rows[::max(1, len(rows) // size)][:size])
    for size in (1, 2, 5, 8):          # (members of any class, as the matrix has them: mostly refusals)
        for start in range(0, len(descs) - 8 * 997, len(descs) // 40):
            plan(descs, f"any x{size}", [start + 997 * j for j in range(size)])


# ------------------------------------------------------------------------------------------------ refusals
_buf = (ctypes.c_float * 4)()
DUMMY = ctypes.cast(_buf, ctypes.c_void_p)          # never dereferenced: a call that is not refused fails at the launch


def said(label, rc):
    print("R", label, "|", rc, lib.ctl_last_error().decode() if rc != 0 else "")


def fwd_call(d, **kw):
    names = ["x", "wpack", "bias", "pro_scale", "pro_shift", "res", "res_scale", "res_shift", "res2", "x2", "y", "stats_partial", "pool", "xout"]
    a = dict(x=DUMMY, wpack=DUMMY, y=DUMMY, bias=None, pro_scale=None, pro_shift=None, res=None, res_scale=None, res_shift=None, res2=None, x2=None,
             stats_partial=None, pool=None, xout=None)
    if d is not None and int(d["pro_affine"]):
        a.update(pro_scale=DUMMY, pro_shift=DUMMY)
    a.update(kw)
    return lib.ctl_conv_forward_ex(_ffi.desc_ptr(d) if d is not None else None, *[a[k] for k in names], None)


def wgrad_call(d, **kw):
    names = ["x", "pro_scale", "pro_shift", "dy", "dy2", "dy_coef", "w_partial", "b_partial"]
    a = dict(x=DUMMY, dy=DUMMY, w_partial=DUMMY, b_partial=DUMMY, pro_scale=None, pro_shift=None, dy2=None, dy_coef=None)
    if d is not None and int(d["pro_affine"]):
        a.update(pro_scale=DUMMY, pro_shift=DUMMY)
    a.update(kw)
    return lib.ctl_conv_wgrad_ex(_ffi.desc_ptr(d) if d is not None else None, *[a[k] for k in names], None)


def ptrs(vals):
    return (ctypes.c_void_p * len(vals))(*[v.value if v is not None else None for v in vals])


def group_call(members, splits=None, n=None, drop=()):
    """members: (descriptor, dict of that member's tensors, None = missing); drop: whole pointer arrays passed as NULL"""
    descs = np.ascontiguousarray(np.concatenate([np.atleast_1d(m[0]) for m in members]))
    names = ["x", "pro_scale", "pro_shift", "dy", "dy2", "dy_coef", "w_partial", "b_partial"]
    cols = {}
    for k in names:
        col = []
        for d, t in members:
            dflt = DUMMY if k in ("x", "dy", "w_partial", "b_partial") or (k in ("pro_scale", "pro_shift") and int(d["pro_affine"])) else None
            col.append(t.get(k, dflt))
        cols[k] = None if k in drop else ptrs(col)
    if splits is None:
        splits = [1] * len(members)
    sp = np.array(splits, dtype=np.int32)
    return lib.ctl_conv_wgrad_group(len(members) if n is None else n, descs.ctypes.data, sp.ctypes.data, *[cols[k] for k in names], None)


def refusals():
    base = dict(n=1, hin=8, win=8, cin=32, hout=8, wout=8, cout=32, ks=3)
    fams = [("fp32", 0), ("x3", _ffi.DT_X3), ("bf16", DTS[2])]
    for fam, dt in fams:
        D = lambda **kw: _ffi.conv_desc(**{**base, "dt": dt, **kw})
        # ---- ctl_conv_forward_ex
        said(f"{fam} fwd d null", fwd_call(None))
        for k in ("x", "wpack", "y"):
            said(f"{fam} fwd {k} null", fwd_call(D(), **{k: None}))
        said(f"{fam} fwd bias missing", fwd_call(D(epi_flags=_ffi.EPI_BIAS)))
        said(f"{fam} fwd res missing", fwd_call(D(epi_flags=_ffi.EPI_RES)))
        said(f"{fam} fwd stats missing", fwd_call(D(epi_flags=_ffi.EPI_STATS)))
        said(f"{fam} fwd prologue missing", fwd_call(D(pro_affine=1, pro_slope=0.2), pro_scale=None))
        said(f"{fam} fwd pro_affine 3", fwd_call(D(pro_affine=3)))
        said(f"{fam} fwd x2 missing", fwd_call(D(pro_affine=2)))
        said(f"{fam} fwd xout without prologue", fwd_call(D(), xout=DUMMY))
        said(f"{fam} fwd pool on a 3x3", fwd_call(D(), pool=DUMMY))
        said(f"{fam} fwd groups*cin 512", fwd_call(D(n=4, cin=128, groups=4, pro_affine=1, pro_slope=0.2)))
        said(f"{fam} fwd pro slope 1.5", fwd_call(D(pro_affine=1, pro_slope=1.5)))
        said(f"{fam} fwd epi slope -0.5", fwd_call(D(epi_act=_ffi.ACT_LEAKY, epi_slope=-0.5)))
        said(f"{fam} fwd 2 GiB in", fwd_call(D(hin=16384, win=16384, hout=16384, wout=16384, cin=16, cout=16)))
        said(f"{fam} fwd n 0", fwd_call(D(n=0)))
        said(f"{fam} fwd n 3 groups 2", fwd_call(D(n=3, groups=2)))
        said(f"{fam} fwd 5x5", fwd_call(D(ks=5, pad=2)))
        # ---- ctl_conv_wgrad_ex
        said(f"{fam} wgrad d null", wgrad_call(None))
        for k in ("x", "dy", "w_partial"):
            said(f"{fam} wgrad {k} null", wgrad_call(D(), **{k: None}))
        said(f"{fam} wgrad pro_affine 2", wgrad_call(D(pro_affine=2)))
        said(f"{fam} wgrad prologue missing", wgrad_call(D(pro_affine=1, pro_slope=0.2), pro_shift=None))
        said(f"{fam} wgrad dy2 without coefficients", wgrad_call(D(), dy2=DUMMY))
        said(f"{fam} wgrad dy2 on a 1x1", wgrad_call(D(ks=1), dy2=DUMMY, dy_coef=DUMMY))
        said(f"{fam} wgrad dy2 on stride 2", wgrad_call(D(stride=2, hin=16, win=16), dy2=DUMMY, dy_coef=DUMMY))
        said(f"{fam} wgrad groups*cin 512", wgrad_call(D(n=4, cin=128, groups=4, pro_affine=1, pro_slope=0.2)))
        said(f"{fam} wgrad groups*cout 512", wgrad_call(D(n=4, cout=128, groups=4), dy2=DUMMY, dy_coef=DUMMY))
        said(f"{fam} wgrad slope 1.5", wgrad_call(D(pro_affine=1, pro_slope=1.5)))
        said(f"{fam} wgrad slope -0.1", wgrad_call(D(pro_affine=1, pro_slope=-0.1)))
        said(f"{fam} wgrad 2 GiB in", wgrad_call(D(hin=16384, win=16384, hout=16384, wout=16384, cin=16, cout=16)))
        said(f"{fam} wgrad 2 GiB out", wgrad_call(D(hin=8192, win=8192, hout=8192, wout=8192, cin=4 if fam == "fp32" else 16, cout=16)))
        said(f"{fam} wgrad nsub 4", wgrad_call(D(nsub=4)))
        said(f"{fam} wgrad zero-insert", wgrad_call(D(in_mode=Z)))
        said(f"{fam} wgrad 4x4", wgrad_call(D(ks=4, stride=2, hin=16, win=16)))
        if not dt:
            continue
        # ---- ctl_conv_wgrad_group (the X3 and bf16 families)
        m = lambda t=None, **kw: (D(**kw), dict(t or {}))
        two = dict(dy2=DUMMY, dy_coef=DUMMY)
        said(f"{fam} group n 0", group_call([m()], n=0))
        said(f"{fam} group n 9", group_call([m()] * 9))
        for k in ("x", "dy", "w_partial"):
            said(f"{fam} group array {k} null", group_call([m(), m()], drop=(k,)))
            said(f"{fam} group member 1 {k} null", group_call([m(), m({k: None})]))
        said(f"{fam} group member 1 prologue missing", group_call([m(pro_affine=1, pro_slope=0.2), m({"pro_scale": None}, pro_affine=1, pro_slope=0.2)]))
        said(f"{fam} group prologue arrays null", group_call([m(pro_affine=1, pro_slope=0.2)] * 2, drop=("pro_scale", "pro_shift")))
        said(f"{fam} group member 1 dy2 without coefficients", group_call([m(two), m({"dy2": DUMMY})]))
        said(f"{fam} group dy2 on a 1x1", group_call([m(two, ks=1), m(two, ks=1)]))
        said(f"{fam} group member 1 groups*cin 512", group_call([m(pro_affine=1, pro_slope=0.2), m(n=4, cin=128, groups=4, pro_affine=1, pro_slope=0.2)]))
        said(f"{fam} group member 1 groups*cout 512", group_call([m(two), m(two, n=4, cout=128, groups=4)]))
        said(f"{fam} group member 0 slope 1.5", group_call([m(pro_affine=1, pro_slope=1.5), m(pro_affine=1, pro_slope=0.2)]))
        m64 = m(hin=64, win=64, hout=64, wout=64)          # (of the class of the large members below: the bf16 family's 16x16-pixel tiles)
        said(f"{fam} group member 1 2 GiB in", group_call([m64, m(hin=16384, win=16384, hout=16384, wout=16384)]))
        said(f"{fam} group member 0 2 GiB out", group_call([m(hin=8192, win=8192, hout=8192, wout=8192), m64]))
        said(f"{fam} group member 1 of another class", group_call([m(), m(in_mode=U, hin=4, win=4)]))
        said(f"{fam} group member 1 with dy2, member 0 without", group_call([m(), m(two)]))
        said(f"{fam} group member 1 of the other family", group_call([m(), m(dt=DTS[2] if fam == "x3" else _ffi.DT_X3)]))
        said(f"{fam} group member 0 not a grouped shape", group_call([m(ks=2, stride=2, pad=0, hin=16, win=16), m()]))
        said(f"{fam} group splits 0", group_call([m(), m()], splits=[1, 0]))
        said(f"{fam} group splits above the tiles", group_call([m(), m()], splits=[1, 1000]))
    # ---- ctl_plan_run
    d = _ffi.conv_desc(**base, dt=_ffi.DT_X3)

    def wgrad_op(splits, slots):
        """slots: tensor name -> slot (at byte offset 0)"""
        return _ffi.new_op(_ffi.OP_WGRAD, d, group_splits=splits, **{name: (s, 0) for name, s in slots.items()})

    def group_op(n):
        return _ffi.new_op(_ffi.OP_WGRAD_GROUP, members=n)

    def run(label, ops, bases):
        arr = np.ascontiguousarray(np.concatenate([np.atleast_1d(o) for o in ops]))
        said(label, lib.ctl_plan_run(arr.ctypes.data, len(ops), ptrs(bases), len(bases), None))

    full = dict(x=0, dy=0, w_partial=0, b_partial=0)
    run("plan member record without its GROUP record", [wgrad_op(3, full)], [DUMMY])
    run("plan op uses an empty slot", [wgrad_op(0, {**full, "dy": 1})], [DUMMY, None])
    run("plan op uses a slot past the table", [wgrad_op(0, {**full, "w_partial": 2})], [DUMMY, None])
    run("plan group member uses an empty slot", [group_op(2), wgrad_op(1, full), wgrad_op(1, {**full, "x": 1})], [DUMMY, None])
    run("plan group of 0", [group_op(0), wgrad_op(1, full)], [DUMMY])
    run("plan group of 9", [group_op(9)] + [wgrad_op(1, full)] * 9, [DUMMY])
    run("plan group past the end", [group_op(2), wgrad_op(1, full)], [DUMMY])
    run("plan group member is not a WGRAD record", [group_op(2), wgrad_op(1, full), group_op(1)], [DUMMY])
    run("plan group member misses a tensor", [group_op(2), wgrad_op(1, full), wgrad_op(1, dict(x=0, w_partial=0))], [DUMMY])
    run("plan unknown kind", [np.zeros((), dtype=_ffi.OP_DTYPE)], [DUMMY])


def main():
    descs = matrix()
    group_plans(descs, sizing(descs))
    import torch
    if torch.cuda.is_available():
        print("# a GPU is visible: the refusal part is skipped (a call that is not refused would launch)", file=sys.stderr)
        return
    refusals()


if __name__ == "__main__":
    main()
