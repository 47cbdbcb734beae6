"""The segmentation-loss kernels (csrc/ctl_loss.hip) through the C ABI against the float64 host statements of losses.py: forward and
backward of every kind with gout = 0.7, outputs and scratch in guard-banded, poisoned buffers.

Bounds, those of the ce2d tests (tests/test_elem_gpu.py): |loss - ref| <= 2e-6 * max(1, |ref|); gradient within 1e-5 of the reference
relative to its largest entry (oracle.ref_elem.close); everything finite.

Shapes (B, H, W): one pixel; a few pixels; 255 and 257 pixels per sample (one block / a second block with one pixel, sample boundaries
off the block grid); 16 x 128 x 128, where the blocks-per-sample cap of the Dice forward is active (32 instead of 64)."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from oracle import ref_elem as R  # noqa: E402
from oracle.guarded import GuardedCall  # noqa: E402
from cooperative_training_and_latent_space_data_augmentation_amd import _ffi, autograd, losses, model_util, ops, solver  # noqa: E402

DEV = "cuda"
lib = _ffi.lib
check = _ffi.check
GOUT = float(np.float32(0.7))
KINDS = ["weighted cross entropy", "focal", "dice", "foreground dice"]
SHAPES = [(1, 1, 1), (2, 3, 5), (3, 1, 255), (3, 1, 257), (16, 128, 128)]
CLASSES = [2, 4, 5, 16]
VARIANTS = ["random", "absent", "one_class", "saturated", "bad_labels"]


def sp():
    return torch.cuda.current_stream().cuda_stream


def class_weights(c):
    return [0.5 + 0.75 * k + 0.1 * (k % 2) for k in range(c)]


def make_case(shape, c, variant):
    """logits [B,C,H,W] (NHWC memory) and label map [B,H,W] on the host"""
    b, h, w = shape
    g = torch.Generator().manual_seed(1000 * c + 10 * b + h + w + VARIANTS.index(variant))
    x = torch.randn(b, h, w, c, generator=g) * 3.0
    y = torch.randint(0, c, (b, h, w), generator=g)
    if variant == "absent":                      # class c-1 absent from sample 0
        y[0][y[0] == c - 1] = 0
    elif variant == "one_class":                 # the last sample is one class
        y[-1] = c - 1
    elif variant == "saturated":                 # every third pixel a row such as (60, -60, 0, ...), rotated over the classes
        row = torch.zeros(c)
        row[0], row[1] = 60.0, -60.0
        flat = x.view(-1, c)
        for i in range(0, flat.shape[0], 3):
            flat[i] = torch.roll(row, i % c)
    elif variant == "bad_labels":                # 255 and -1 among valid labels
        y.view(-1)[0] = 255
        y.view(-1)[-1] = -1
        if y.numel() > 4:
            y.view(-1)[y.numel() // 2] = -1
            y.view(-1)[1] = 255
    return x.permute(0, 3, 1, 2), y


def raw_fwd_bwd(kind, xd, yd, wts, gout, ws, loss, dlogit, gamma=2.0):
    """both launchers on raw pointers; xd is [B,C,H,W] with NHWC memory"""
    b, c, h, w = xd.shape
    k = ops.LOSS_KINDS[kind]
    cw = (_ffi.C.c_double * c)(*wts) if wts is not None else None
    check(lib.ctl_seg_loss_fwd(k, xd.data_ptr(), yd.data_ptr(), cw, gamma, b, h * w, c, ws, loss, sp()), "fwd")
    check(lib.ctl_seg_loss_bwd(k, xd.data_ptr(), yd.data_ptr(), cw, gamma, gout.data_ptr(), ws, b, h * w, c, dlogit, sp()), "bwd")


@pytest.mark.parametrize("variant", VARIANTS)
@pytest.mark.parametrize("c", CLASSES)
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_every_kind_matches_the_host_statement(shape, c, variant):
    x, y = make_case(shape, c, variant)
    b, h, w = shape
    xd, yd = x.to(DEV), y.to(DEV)
    assert xd.permute(0, 2, 3, 1).is_contiguous()
    gout = torch.tensor(0.7, device=DEV)
    wts = class_weights(c)
    if shape == (16, 128, 128):
        assert lib.ctl_seg_loss_blocks(b, h * w) < -(-h * w // 256)          # the blocks-per-sample cap is active
    for kind in KINDS:
        k = ops.LOSS_KINDS[kind]
        gc = GuardedCall(DEV)
        ws = gc.out("ws", lib.ctl_seg_loss_ws_doubles(k, b, h * w, c), torch.float64)
        loss = gc.out("loss", 1)
        dl = gc.out("dlogit", x.numel())
        launch = lambda: raw_fwd_bwd(kind, xd, yd, wts, gout, ws.ptr, loss.ptr, dl.ptr)      # noqa: E731
        gc.run(launch)
        ref_loss, ref_grad = losses.loss_and_grad(x, y, kind, wts, gamma=2.0, gout=GOUT)
        got_loss = float(loss.flat()[0])
        got_grad = dl.view((b, c, h, w), channels_last=True).cpu().double()
        lerr = abs(got_loss - float(ref_loss)) / max(1.0, abs(float(ref_loss)))
        gerr = R.rel_err(got_grad, ref_grad)
        print(f"loss-kernel-error {kind!r} shape={shape} c={c} {variant}: loss {lerr:.3e} grad {gerr:.3e}")
        assert np.isfinite(got_loss) and bool(torch.isfinite(got_grad).all()), kind
        assert lerr <= 2e-6, (kind, got_loss, float(ref_loss))
        R.close(got_grad, ref_grad, 1e-5, kind + " backward")
        gc.rerun(launch)                                                   # guards, every element written, the same bits again


@pytest.mark.parametrize("shape", [(2, 3, 5), (3, 1, 257), (16, 128, 128)], ids=lambda s: "x".join(map(str, s)))
def test_c4_at_storage_offset_1_gives_the_bits_of_the_aligned_call(shape):
    """Rows of 4 channels move as 16 bytes only when logits and gradient are 16-byte aligned; views 4 bytes off take the runtime-count
    kernels: the same arithmetic in the same order, so the same bits."""
    x, y = make_case(shape, 4, "saturated")
    b, h, w = shape
    n = x.numel()
    yd = y.to(DEV)
    gout = torch.tensor(0.7, device=DEV)

    def run(kind, aligned):
        buf_x, buf_d = torch.zeros(n + 8, device=DEV), torch.full((n + 8,), float("nan"), device=DEV)
        o = 0 if aligned else 1
        xv, dv = buf_x[o:o + n], buf_d[o:o + n]
        xv.copy_(x.permute(0, 2, 3, 1).reshape(-1))
        assert xv.data_ptr() % 16 == 4 * o and dv.data_ptr() % 16 == 4 * o
        xl = xv.view(b, h, w, 4).permute(0, 3, 1, 2)
        ws = torch.full((lib.ctl_seg_loss_ws_doubles(ops.LOSS_KINDS[kind], b, h * w, 4),), float("nan"), dtype=torch.float64, device=DEV)
        loss = torch.full((), float("nan"), device=DEV)
        raw_fwd_bwd(kind, xl, yd, class_weights(4), gout, ws.data_ptr(), loss.data_ptr(), dv.data_ptr())
        return loss.cpu(), dv.cpu().clone(), ws.cpu()

    for kind in KINDS:
        a, u = run(kind, True), run(kind, False)
        assert bool(torch.isfinite(a[1]).all()) and bool(torch.isfinite(a[2]).all())
        for p, q, what in zip(a, u, ("loss", "dlogit", "scratch")):
            assert torch.equal(p, q), (kind, what)


@pytest.mark.parametrize("c", [4, 5])
def test_graph_replay_gives_the_bits_of_the_eager_call(c):
    x, y = make_case((3, 1, 257), c, "bad_labels")
    xd, yd = x.to(DEV), y.to(DEV)
    gout = torch.tensor(0.7, device=DEV)
    wts = class_weights(c)
    for kind in KINDS:
        loss_e, ws_e = ops.seg_loss_fwd(xd, yd, kind, wts)
        d_e = ops.seg_loss_bwd(xd, yd, kind, gout, ws_e, wts)
        loss_2, ws_2 = ops.seg_loss_fwd(xd, yd, kind, wts)                 # a second call: the same bits
        d_2 = ops.seg_loss_bwd(xd, yd, kind, gout, ws_2, wts)
        assert torch.equal(loss_e, loss_2) and torch.equal(d_e, d_2) and torch.equal(ws_e, ws_2), kind
        torch.cuda.synchronize()
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph):
            loss_g, ws_g = ops.seg_loss_fwd(xd, yd, kind, wts)
            d_g = ops.seg_loss_bwd(xd, yd, kind, gout, ws_g, wts)
        for _ in range(2):
            loss_g.fill_(float("nan")); d_g.fill_(float("nan")); ws_g.fill_(float("nan"))
            graph.replay()
            torch.cuda.synchronize()
            assert torch.equal(loss_e, loss_g) and torch.equal(d_e, d_g) and torch.equal(ws_e, ws_g), kind
        del graph


def test_autograd_wrappers_return_the_tensors_of_the_raw_calls():
    c = 4
    x, y = make_case((2, 3, 5), c, "random")
    xd, yd = x.to(DEV), y.to(DEV)
    gout = torch.tensor(0.7, device=DEV)
    wts = class_weights(c)
    raw = {}
    for kind in KINDS + ["weighted dice"]:
        loss_r, ws = ops.seg_loss_fwd(xd, yd, kind, wts)
        raw[kind] = (loss_r, ops.seg_loss_bwd(xd, yd, kind, gout, ws, wts))
        for fn in (lambda xr: autograd.segmentation_loss(xr, yd, kind, wts), lambda xr: solver.basic_loss_fn(xr, yd, kind, wts)):
            xr = xd.clone().requires_grad_(True)
            loss = fn(xr)
            loss.backward(gout)
            assert torch.equal(loss.detach(), raw[kind][0]) and torch.equal(xr.grad, raw[kind][1]), kind
    assert torch.equal(raw["weighted dice"][0], raw["dice"][0]) and torch.equal(raw["weighted dice"][1], raw["dice"][1])
    # cross_entropy_2D with a weight is the weighted kernel; uniform weights are plain cross entropy (up to the rounding of another kernel)
    xr = xd.clone().requires_grad_(True)
    wt = torch.tensor(wts)                                   # (upstream hands over a float32 tensor: these are the weights rounded to it)
    loss = model_util.cross_entropy_2D(xr, yd, weight=wt)
    loss.backward(gout)
    loss_r, _ = ops.seg_loss_fwd(xd, yd, "weighted cross entropy", wt.tolist())
    assert torch.equal(loss.detach(), loss_r) and torch.equal(xr.grad, ops.seg_loss_bwd(xd, yd, "weighted cross entropy", gout, None, wt.tolist()))
    ce = ops.ce2d_fwd(xd, yd)
    for uw in (None, [1.0] * c, [0.25] * c):
        u, _ = ops.seg_loss_fwd(xd, yd, "weighted cross entropy", uw)
        assert abs(float(u) - float(ce)) <= 2e-6 * max(1.0, abs(float(ce)))
    R.close(ops.seg_loss_bwd(xd, yd, "weighted cross entropy", gout).cpu(), ops.ce2d_bwd(xd, yd, gout).cpu(), 1e-5, "uniform weights")
    # the mapping form: sum of weight * L_name, value and gradient
    spec = {"cross entropy": 1.0, "dice": 0.5, "focal": 2.0}
    xr = xd.clone().requires_grad_(True)
    loss = solver.basic_loss_fn(xr, yd, spec, wts)
    loss.backward(gout)
    ref_loss, ref_grad = losses.loss_and_grad(x, y, spec, wts, gout=GOUT)
    assert abs(float(loss) - float(ref_loss)) <= 2e-6 * max(1.0, abs(float(ref_loss)))
    R.close(xr.grad.cpu(), ref_grad, 1e-5, "mapping backward")
    # gamma is an argument of the kernel
    for gamma in (0.0, 0.5, 3.0):
        lg, _ = ops.seg_loss_fwd(xd, yd, "focal", None, gamma)
        dg = ops.seg_loss_bwd(xd, yd, "focal", gout, None, None, gamma)
        ref_loss, ref_grad = losses.loss_and_grad(x, y, "focal", gamma=gamma, gout=GOUT)
        assert abs(float(lg) - float(ref_loss)) <= 2e-6 * max(1.0, abs(float(ref_loss))), gamma
        R.close(dg.cpu(), ref_grad, 1e-5, f"focal gamma {gamma}")
