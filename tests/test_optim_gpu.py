"""The optimizer-tail kernels of csrc/ctl_optim.hip through the C ABI, every device buffer between guard bands (oracle/guarded.py):
ctl_optim_control, ctl_grad_norm and ctl_adam_tail against the fp64 host statements optim.grad_norm_host / optim.adam_tail_host, against
math.fsum, and bit for bit against ctl_adam / ctl_adam_dev where the settings are neutral.

Bounds.  sumsq: fp32 squares are exact in fp64, so only the N - 1 additions round: N * 2^-53 relative.  norm, clip: 4 * 2^-53 relative of
the host formula on the device's own sumsq (a square root, a product, a sum, a quotient).  m, v under a clip factor: the existing Adam
test's 4 * 2^-24 plus the one extra rounding of the clip product, which enters v squared: 6 * 2^-24 relative, 2^-126 absolute below the
smallest normal; p: 2e-7 * max(1, |p|) as there.  The EMA shadow: bit for bit the fp32 statement on the device's own new weights."""
import ctypes
import math

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from cooperative_training_and_latent_space_data_augmentation_amd import _ffi, ops, optim  # noqa: E402
from cooperative_training_and_latent_space_data_augmentation_amd._ffi import lib, check  # noqa: E402
from oracle.guarded import Guarded  # noqa: E402

DEV = "cuda"
CH = _ffi.GRAD_NORM_CHUNK
EB, MAX_STREAM_BLOCKS = 256, 2048
U24, U53 = 2.0 ** -24, 2.0 ** -53
LR, B1, B2, AEPS = 1e-4, 0.9, 0.999, 1e-8
B1F, B2F, LRF, EPSF = (float(np.float32(v)) for v in (B1, B2, LR, AEPS))           # what the kernel receives
F = _ffi
HOST_WORDS = list(range(F.OPTIM_LR, F.OPTIM_LR + 8)) + [F.OPTIM_MAX_NORM, F.OPTIM_GUARD, F.OPTIM_EMA_OMD]
DEV_WORDS = [F.OPTIM_SUMSQ, F.OPTIM_NORM, F.OPTIM_CLIP, F.OPTIM_FINITE, F.OPTIM_SKIPPED]
RESERVED = [i for i in range(F.OPTIM_CTRL_DOUBLES) if i not in HOST_WORDS + DEV_WORDS]


def sp():
    return ops.stream_ptr()


def f32(x):
    return float(np.float32(x))


def gbuf(t, name):
    """a guarded device copy of the CPU tensor t"""
    b = Guarded(t.numel(), t.dtype, DEV, name=name)
    b.flat().copy_(t.reshape(-1))
    return b


def new_ctrl():
    """a poisoned record whose `skipped` word the caller has zeroed, as the header asks"""
    c = Guarded(F.OPTIM_CTRL_DOUBLES, torch.float64, DEV, name="ctrl")
    c.flat()[F.OPTIM_SKIPPED] = 0.0
    return c


def control(ctrl, lrs, max_norm=0.0, guard=False, omd=0.0):
    arr = (ctypes.c_float * len(lrs))(*lrs)
    check(lib.ctl_optim_control(ctrl.ptr, len(lrs), ctypes.cast(arr, ctypes.c_void_p), max_norm, int(guard), omd, sp()))


def norm_call(bufs, counts, gs, work, ctrl):
    ptrs = (ctypes.c_void_p * len(bufs))(*[b.ptr if isinstance(b, Guarded) else b for b in bufs])
    cnts = (ctypes.c_int64 * len(bufs))(*counts)
    check(lib.ctl_grad_norm(ctypes.cast(ptrs, ctypes.c_void_p), ctypes.cast(cnts, ctypes.c_void_p), len(bufs), gs, work.ptr, ctrl.ptr, sp()))


def tail(p, g, m, v, ema, count, ctrl, net, gs=1.0, step=1, state=None):
    check(lib.ctl_adam_tail(p.ptr, g.ptr, m.ptr, v.ptr, ema.ptr if ema is not None else None, count, B1, B2, AEPS,
                            state.data_ptr() if state is not None else None, step, gs, ctrl.ptr, net, sp()))


def reserved_untouched(ctrl):
    poison = Guarded(1, torch.float64, "cpu").bits()[0]
    return bool((ctrl.bits().cpu()[RESERVED] == poison).all())


def grads_of(pattern, count, g):
    if pattern == "zero":
        return torch.zeros(count)
    if pattern == "tiny":
        return torch.full((count,), 1e-20)
    if pattern == "huge":
        return torch.full((count,), 1e4) * torch.where(torch.rand(count, generator=g) < 0.5, -1.0, 1.0)
    pick = torch.randint(0, 4, (count,), generator=g)
    rnd = torch.randn(count, generator=g) * 0.1
    return torch.where(pick == 0, torch.zeros(count), torch.where(pick == 1, torch.full((count,), 1e-20), torch.where(pick == 2, torch.full((count,), 1e4), rnd)))


# ================================================================================================ control record
def test_control_writes_its_fields_and_nothing_else():
    ctrl = new_ctrl()
    ctrl.flat()[F.OPTIM_SKIPPED] = 7.0
    ctrl.flat()[F.OPTIM_SUMSQ] = 3.0
    control(ctrl, [1e-3, 2e-4, 3e-5], max_norm=2.5, guard=True, omd=0.1)
    c = ctrl.flat().cpu()
    assert c[:8].tolist() == [f32(1e-3), f32(2e-4), f32(3e-5), 0, 0, 0, 0, 0]      # the double of the fp32 value; slots past k: 0
    assert [c[F.OPTIM_MAX_NORM].item(), c[F.OPTIM_GUARD].item(), c[F.OPTIM_EMA_OMD].item()] == [2.5, 1.0, f32(0.1)]
    assert [c[F.OPTIM_CLIP].item(), c[F.OPTIM_FINITE].item()] == [1.0, 1.0]
    assert c[F.OPTIM_SKIPPED].item() == 7.0 and c[F.OPTIM_SUMSQ].item() == 3.0      # never touched
    assert math.isnan(c[F.OPTIM_NORM].item()) and reserved_untouched(ctrl)
    ctrl.check_guards()
    control(ctrl, [5e-4] * 8, max_norm=0.0, guard=False, omd=0.0)
    c = ctrl.flat().cpu()
    assert c[:8].tolist() == [f32(5e-4)] * 8 and c[8:11].tolist() == [0.0, 0.0, 0.0] and c[F.OPTIM_SKIPPED].item() == 7.0
    ctrl.check_guards()


# ================================================================================================ gradient norm
COUNTS = {1: [63], 2: [CH - 1, CH + 1], 5: [1, 3 * CH + 7, 64, CH, 65]}      # a 1-element buffer beside a multi-chunk one


@pytest.mark.parametrize("pattern", ["zero", "tiny", "huge", "mix"])
@pytest.mark.parametrize("k", [1, 2, 5])
def test_grad_norm_against_the_exact_sum(k, pattern):
    g = torch.Generator().manual_seed(10 * k + len(pattern))
    counts = COUNTS[k]
    host = [grads_of(pattern, n, g) for n in counts]
    bufs = [gbuf(t, f"g{j}") for j, t in enumerate(host)]
    N = sum(counts)
    exact = math.fsum((np.concatenate([t.numpy() for t in host]).astype(np.float64) ** 2).tolist())
    need = ops.grad_norm_work(counts)
    assert need == sum(-(-n // CH) for n in counts)
    work = Guarded(need, torch.float64, DEV, name="work")
    ctrl = new_ctrl()
    graph_done = False
    for gs in (1.0, 0.5, 0.125):
        base = gs * math.sqrt(exact)
        for mn in (0.0, f32(base * 0.5 or 1.0), f32(base or 1e-6), f32(base * 4 or 2.0)):      # off, below, at, above the norm (as fp32: it travels as one)
            control(ctrl, [LR] * k, max_norm=mn, guard=True)
            work.repoison()
            norm_call(bufs, counts, gs, work, ctrl)
            c = ctrl.flat().cpu().tolist()
            sumsq, norm, clip = c[F.OPTIM_SUMSQ], c[F.OPTIM_NORM], c[F.OPTIM_CLIP]
            assert abs(sumsq - exact) <= N * U53 * exact, (sumsq, exact)
            hn = gs * math.sqrt(sumsq)
            hc = min(1.0, mn / (hn + 1e-6)) if mn > 0 else 1.0
            assert abs(norm - hn) <= 4 * U53 * hn and abs(clip - hc) <= 4 * U53 * hc, (norm, hn, clip, hc)
            assert c[F.OPTIM_FINITE] == 1.0 and c[F.OPTIM_SKIPPED] == 0.0 and 0.0 < clip <= 1.0
            if mn == 0.0 or mn > 2 * hn + 1e-5:
                assert clip == 1.0
            elif mn < hn:
                assert clip < 1.0
            hs, hnorm, hclip, hfin = optim.grad_norm_host(host, gs, mn, True)          # the host statement end to end
            assert hfin and abs(hs - exact) <= N * U53 * exact and abs(hnorm - norm) <= 2 * N * U53 * norm and abs(hclip - clip) <= 2 * N * U53
            work.check_guards(); work.check_written(); ctrl.check_guards()              # noqa: E702
            assert reserved_untouched(ctrl)
            for b, t in zip(bufs, host):
                b.check_guards()
                assert torch.equal(b.flat().cpu(), t)
            first = (ctrl.snapshot(), work.snapshot())
            work.repoison()
            norm_call(bufs, counts, gs, work, ctrl)                                     # a second call: the same bits
            assert torch.equal(ctrl.snapshot(), first[0]) and torch.equal(work.snapshot(), first[1])
            if not graph_done and mn > 0:                                               # ... and in a graph replay
                graph_done = True
                side = torch.cuda.Stream()
                side.wait_stream(torch.cuda.current_stream())
                gr = torch.cuda.CUDAGraph()
                with torch.cuda.graph(gr, stream=side):
                    norm_call(bufs, counts, gs, work, ctrl)
                torch.cuda.current_stream().wait_stream(side)
                for _ in range(2):
                    work.repoison()
                    ctrl.flat()[F.OPTIM_SUMSQ:F.OPTIM_FINITE + 1] = -1.0
                    gr.replay()
                    torch.cuda.synchronize()
                    assert torch.equal(ctrl.snapshot(), first[0]) and torch.equal(work.snapshot(), first[1])
                    work.check_guards(); ctrl.check_guards()                            # noqa: E702


def test_grad_norm_bits_do_not_depend_on_alignment():
    """a 16-byte aligned buffer is read 16 bytes per lane, any other one element at a time: the same grouping"""
    g = torch.Generator().manual_seed(2)
    n = 2 * CH + 9
    t = torch.randn(n, generator=g)
    ctrl, work = new_ctrl(), Guarded(3, torch.float64, DEV, name="work")
    control(ctrl, [LR])
    res = []
    for shift in (0, 1, 2, 3):
        holder = Guarded(n + 3, torch.float32, DEV, name="holder")
        holder.flat()[shift:shift + n] = t.to(DEV)
        work.repoison()
        norm_call([holder.ptr + 4 * shift], [n], 1.0, work, ctrl)
        holder.check_guards(); work.check_guards(); work.check_written()                # noqa: E702
        res.append((ctrl.snapshot(), work.snapshot()))
    assert all(torch.equal(r[0], res[0][0]) and torch.equal(r[1], res[0][1]) for r in res[1:])


@pytest.mark.parametrize("where", ["nan-last-of-last", "inf-first-of-first"])
def test_nonfinite_gradient_guard(where):
    g = torch.Generator().manual_seed(7)
    counts = [300, CH + 5, 1, 64, 2 * CH + 3]
    host = [torch.randn(n, generator=g) * 0.1 for n in counts]
    if where == "nan-last-of-last":
        host[-1][-1] = float("nan")
    else:
        host[0][0] = float("inf")
    bufs = [gbuf(t, f"g{j}") for j, t in enumerate(host)]
    work = Guarded(ops.grad_norm_work(counts), torch.float64, DEV, name="work")
    ctrl = new_ctrl()
    state = [[gbuf(torch.rand(n, generator=g) + 0.1, f"{nm}{j}") for nm in "pmvs"] for j, n in enumerate(counts)]
    before = [[b.snapshot() for b in st] for st in state]
    for call in (1, 2):                                   # guard on: finite = 0, the count runs 0 -> 1 -> 2, no tail writes anything
        control(ctrl, [LR] * 5, max_norm=1.0, guard=True, omd=0.25)
        norm_call(bufs, counts, 1.0, work, ctrl)
        for j, n in enumerate(counts):
            tail(state[j][0], bufs[j], state[j][1], state[j][2], state[j][3], n, ctrl, j, step=call)
        c = ctrl.flat().cpu().tolist()
        assert c[F.OPTIM_FINITE] == 0.0 and c[F.OPTIM_SKIPPED] == float(call) and c[F.OPTIM_CLIP] == 1.0
        assert not math.isfinite(c[F.OPTIM_NORM])
        for st, snap in zip(state, before):
            for b, s in zip(st, snap):
                b.check_guards()
                assert torch.equal(b.snapshot(), s), b.name
    control(ctrl, [LR] * 5, max_norm=1.0, guard=False, omd=0.25)      # guard off: clip stays 1, the count stands, Adam proceeds as today
    norm_call(bufs, counts, 1.0, work, ctrl)
    c = ctrl.flat().cpu().tolist()
    assert c[F.OPTIM_FINITE] == 0.0 and c[F.OPTIM_SKIPPED] == 2.0 and c[F.OPTIM_CLIP] == 1.0
    for j, n in enumerate(counts):
        tail(state[j][0], bufs[j], state[j][1], state[j][2], state[j][3], n, ctrl, j, step=3)
    for j, (st, snap) in enumerate(zip(state, before)):
        for b, s in zip(st, snap):
            b.check_guards()
            assert not torch.equal(b.snapshot(), s), b.name
        pm, mm, vm = (s.view(torch.float32).cpu() for s in snap[:3])
        ref = optim.adam_tail_host(pm, host[j], mm, vm, None, LRF, (B1F, B2F), EPSF, 3)
        ok = torch.isfinite(host[j])
        assert bool(((state[j][0].flat().cpu().double() - ref[0]).abs()[ok] <= 2e-7 * ref[0].abs().clamp_min(1.0)[ok]).all())
    work.check_guards(); ctrl.check_guards()              # noqa: E702
    assert reserved_untouched(ctrl)


# ================================================================================================ Adam tail
@pytest.mark.parametrize("count", [1, 255, 257, 10007, MAX_STREAM_BLOCKS * EB + 5])
@pytest.mark.parametrize("step", [1, 2, 1000])
def test_adam_tail_neutral_and_clipped(step, count):
    g = torch.Generator().manual_seed(step % 1000 + count % 1000)
    p0 = torch.randn(count, generator=g)
    ctrl = new_ctrl()
    control(ctrl, [3.0, LR, 7.0])                         # this network is slot 1: the lr comes from the record
    for pattern in ("zero", "tiny", "huge", "mix"):
        gr = grads_of(pattern, count, g)
        gprev = gr * (torch.rand(count, generator=g) + 0.5)
        for gs in (1.0, 0.5, 0.125):
            gp = gprev.double() * gs
            m0 = ((1 - B1F ** (step - 1)) * gp).float()
            v0 = ((1 - B2F ** (step - 1)) * gp * gp).float()
            what = f"{pattern} gradient, grad_scale {gs}"
            gb = gbuf(gr, "g")
            res = {}
            for form in ("tail-step", "tail-state", "adam", "adam_dev"):
                pb, mb, vb = gbuf(p0, "p"), gbuf(m0, "m"), gbuf(v0, "v")
                st = torch.tensor([123, 8, step], dtype=torch.int64, device=DEV)
                if form == "tail-step":
                    tail(pb, gb, mb, vb, None, count, ctrl, 1, gs, step=step)
                elif form == "tail-state":
                    tail(pb, gb, mb, vb, None, count, ctrl, 1, gs, step=0, state=st)
                elif form == "adam":
                    check(lib.ctl_adam(pb.ptr, gb.ptr, mb.ptr, vb.ptr, count, LR, B1, B2, AEPS, step, gs, sp()))
                else:
                    check(lib.ctl_adam_dev(pb.ptr, gb.ptr, mb.ptr, vb.ptr, count, LR, B1, B2, AEPS, st.data_ptr(), gs, sp()))
                for b in (pb, mb, vb, gb):                # ema = NULL: nothing beyond p, m, v is written
                    b.check_guards()
                assert torch.equal(gb.flat().cpu(), gr) and st.tolist() == [123, 8, step]
                res[form] = (pb.snapshot(), mb.snapshot(), vb.snapshot())
            for k, name in enumerate("pmv"):
                assert torch.equal(res["tail-step"][k], res["tail-state"][k]), f"the step and state forms differ in {name} ({what})"
                assert torch.equal(res["tail-step"][k], res["adam"][k]), f"neutral tail differs from ctl_adam in {name} ({what})"
                assert torch.equal(res["tail-state"][k], res["adam_dev"][k]), f"neutral tail differs from ctl_adam_dev in {name} ({what})"
            for clip in (0.25, 0.999):
                ctrl.flat()[F.OPTIM_CLIP] = clip
                pb, mb, vb = gbuf(p0, "p"), gbuf(m0, "m"), gbuf(v0, "v")
                tail(pb, gb, mb, vb, None, count, ctrl, 1, gs, step=step)
                pr, mr, vr, _ = optim.adam_tail_host(p0, gr, m0, v0, None, LRF, (B1F, B2F), EPSF, step, grad_scale=gs, clip=f32(clip))
                pd, md, vd = (b.flat().cpu().double() for b in (pb, mb, vb))
                assert bool(((pd - pr).abs() <= 2e-7 * pr.abs().clamp_min(1.0)).all()), (what, clip, float((pd - pr).abs().max()))
                for name, got, ref in (("m", md, mr), ("v", vd, vr)):
                    tol = torch.where(ref.abs() < 2.0 ** -126, torch.full_like(ref, 2.0 ** -126), 6 * U24 * ref.abs())
                    assert bool(((got - ref).abs() <= tol).all()), (what, clip, name, float(((got - ref).abs() / ref.abs().clamp_min(1e-30)).max()))
                if float(gr.abs().max()) > 1e-3 and clip == 0.25:
                    assert not torch.equal(mb.snapshot(), res["adam"][1]), "the clip factor did not reach the moments"
                for b in (pb, mb, vb):
                    b.check_guards()
            ctrl.flat()[F.OPTIM_CLIP] = 1.0
    ctrl.check_guards()
    assert reserved_untouched(ctrl)


@pytest.mark.parametrize("count", [1, 257, 10007])
@pytest.mark.parametrize("rule", ["num_updates", "fixed"])
def test_ema_shadow_is_the_fp32_statement(rule, count):
    g = torch.Generator().manual_seed(count)
    u = lambda: torch.rand(count, generator=g) * (10 - 1e-3) + 1e-3      # noqa: E731  inputs in [1e-3, 10]: no subnormal arises
    p0, s0 = u(), u()
    pb, mb, vb, sb = gbuf(p0, "p"), gbuf(torch.zeros(count), "m"), gbuf(torch.zeros(count), "v"), gbuf(s0, "ema")
    ctrl = new_ctrl()
    shadow = s0.numpy().copy()
    for n in (1, 2, 3):
        omd = 1.0 - optim.ema_decay_at(0.999, n) if rule == "num_updates" else 1.0 - 0.9
        gb = gbuf(u() * torch.where(torch.rand(count, generator=g) < 0.5, -1.0, 1.0), "g")
        control(ctrl, [1e-2], omd=omd)
        tail(pb, gb, mb, vb, sb, count, ctrl, 0, 1.0, step=n)
        pn = pb.flat().cpu().numpy()                      # the device's own new weights
        d = (shadow - pn).astype(np.float32)
        shadow = (shadow - (np.float32(omd) * d).astype(np.float32)).astype(np.float32)
        assert np.array_equal(sb.flat().cpu().numpy().view(np.int32), shadow.view(np.int32)), (rule, n)
        for b in (pb, mb, vb, sb, gb):
            b.check_guards()
    assert not np.array_equal(shadow, s0.numpy()) and float(np.abs(pb.flat().cpu().numpy() - p0.numpy()).max()) > 0


def test_each_network_uses_its_own_lr():
    g = torch.Generator().manual_seed(9)
    count = 1000
    p0, gr, m0, v0 = torch.randn(count, generator=g), torch.randn(count, generator=g), torch.randn(count, generator=g) * 0.1, torch.rand(count, generator=g)
    ctrl = new_ctrl()
    lrs = [1e-3, 1e-5]
    control(ctrl, lrs)
    out = []
    for net, lr in enumerate(lrs):
        gb = gbuf(gr, "g")
        a, b = [gbuf(t, n) for t, n in ((p0, "p"), (m0, "m"), (v0, "v"))], [gbuf(t, n) for t, n in ((p0, "p"), (m0, "m"), (v0, "v"))]
        tail(a[0], gb, a[1], a[2], None, count, ctrl, net, step=5)
        check(lib.ctl_adam(b[0].ptr, gb.ptr, b[1].ptr, b[2].ptr, count, lr, B1, B2, AEPS, 5, 1.0, sp()))
        assert all(torch.equal(x.snapshot(), y.snapshot()) for x, y in zip(a, b)), net
        out.append(a[0].snapshot())
    assert not torch.equal(out[0], out[1])
