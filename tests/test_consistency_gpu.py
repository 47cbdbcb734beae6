"""The consistency-loss kernels (csrc/ctl_consist.hip) through the C ABI against the host statement consistency.consistency_and_grad; every
buffer a kernel writes sits in a guard-banded, poisoned buffer (oracle/guarded.py) and every launch is repeated for the same bits.

Bounds, from the number formats.  The kernels form q = softmax(x) and p = softmax(r) in fp32 and everything behind them in fp64 (the Sobel
responses of the backward are stored as fp32).  With eps = (C + 10) 2^-24 (tests/test_dist_loss_gpu.py) and u = 2^-24:
  |dq_k| <= eps;  |dp_k| <= ep = eps, or 0 with is_gt (p = r is exact);  log q_k = x_k - log Z with |d log Z| <= eps (the fp32 partition
  sum has that relative error; x_k - max is exact in fp64), the same for log p_k.
Per masked-in pixel, unit weight, gout = 1 (m is the 0/1 mask, a = m / M):
  kl        value: sum_k dp_k (log p_k - log q_k) + p_k (d log Z_r - d log Z_x) <= eps (sum_k |log p_k - log q_k| + 2.01);
                   is_gt: the p_k are exact constants: <= eps sum_k p_k.
            gradient a (S q_j - p_j), S the sum of the rounded p_k: <= a eps (C q_j + 2.01);  is_gt: a eps S.
  ce        value: sum_k w'_k (ep |log q_k| + p_k eps) / R.   gradient (m/R)(q_j sw - w'_j p_j), sw = sum w'_k p_k:
                   <= (m/R)(eps sw + ep (q_j sum_k w'_k + w'_j)).
  mse       value: sum_k (2 |q_k - p_k| e2 + e2^2) / M with e2 = eps + ep.   g_k = 2 a (q_k - p_k): |dg_k| <= 2 a e2.
  Dice      I and U of a (sample, class) move by dI <= sum m (q ep + p eps + eps ep) and dU <= sum m (eps + ep); the term 2I/U then lies in
            [2 (I - dI) / (U + dU), 2 (I + dI) / (U - dU)] and the coefficients 2/U and 2I/U^2 of g_k = -(m / BC)(2 p_k / U - 2I / U^2)
            in the like intervals: |dg_k| <= m (dc0 (p_k + ep) + c0 ep + dc1).
  contour   d_k = q_k - p_k is formed in fp32: |dd_k| <= e_d = eps + ep + 2^-25.  A Sobel response has sum |coefficient| = 8:
            |dE| <= 8 e_d = e_E, value: 1/2 sum m (2 (|E_x| + |E_y|) e_E + 2 e_E^2) / ((C-1) M).  The backward rounds m E to fp32
            (|E| <= 8: + 8 u) and applies two transposed stencils: |dg_k| <= 16 (e_E + 8 u) / ((C-1) M).
  The kinds with a g go through J_j = q_j sum_k q_k (g_j - g_k) with S the sum of the rounded q_k; with G = max_k |g_k| and Gm = max_k |dg_k|:
            |dJ_j| <= 2 eps G + q_j (2 Gm + 2 C eps G).
A loss adds one fp32 rounding of the result, u |ref|.  A gradient element adds u |ref_j| for its one rounding; when 'contour' is combined
with other kinds its launch ADDS into dlogit, three roundings in all: u (|ref_j of the others| + |ref_j of contour| + |ref_j|).  All first-
order figures are multiplied by 1.001 for the second-order terms.  A fused set is linear in its terms: its bound is the weighted sum of
theirs.  The largest error seen per kind is printed as a fraction of its bound (README, "consistency losses")."""
import ctypes

import numpy as np
import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

from oracle.guarded import GuardedCall  # noqa: E402
from cooperative_training_and_latent_space_data_augmentation_amd import _ffi, consistency as K, ops  # noqa: E402
from cooperative_training_and_latent_space_data_augmentation_amd.losses import SMOOTH, normalised_weights  # noqa: E402

DEV = "cuda"
lib = _ffi.lib
check = _ffi.check
U = 2.0 ** -24
GOUT = float(np.float32(0.7))
NAMES = list(ops.CONSISTENCY_KINDS)
PLANES = [(1, 1), (1, 7), (5, 7), (16, 16), (17, 31), (33, 34), (31, 65)]
CLASSES = [1, 2, 4, 5, 16]
VARIANTS = ["random", "saturated", "equal", "gt_onehot", "gt_soft"]
MASKS = ["none", "random", "zero", "one"]
WEIGHTS = {"kl": 1.0, "ce": 0.5, "weighted ce": 0.3, "mse": 2.0, "Dice": 0.7, "contour": 1.5}
WORST = {}


def sp():
    return torch.cuda.current_stream().cuda_stream


def nhwc_dev(t):
    return t.float().contiguous(memory_format=torch.channels_last).to(DEV)


def make_case(b, c, h, w, variant, mask_kind, seed):
    """(x, r, mask, is_gt): fp32 logits [B,C,H,W] on the host, a uint8 mask [B,H,W] or None"""
    g = torch.Generator().manual_seed(seed)
    x = (torch.randn(b, h, w, c, generator=g) * 3.0).permute(0, 3, 1, 2)
    r = (torch.randn(b, h, w, c, generator=g) * 3.0).permute(0, 3, 1, 2)
    is_gt = variant.startswith("gt")
    if variant == "saturated":                   # every third pixel a row such as (80, -80, 0, ...), rotated over the classes, in both
        for t, shift in ((x, 0), (r, 1)):
            flat = t.permute(0, 2, 3, 1).reshape(-1, c)
            row = torch.zeros(c)
            row[0] = 80.0
            if c > 1:
                row[1] = -80.0
            for i in range(0, flat.shape[0], 3):
                flat[i] = torch.roll(row, (i + shift) % c)          # (flat is a view of t)
    elif variant == "equal":
        r = x.clone()
    elif variant == "gt_onehot":
        r = F.one_hot(torch.randint(0, c, (b, h, w), generator=g), c).permute(0, 3, 1, 2).float()
    elif variant == "gt_soft":                   # soft probabilities with exact zeros among them (the 'kl' rule looks at r == 0)
        r = torch.softmax(r, 1) * (torch.rand(b, c, h, w, generator=g) > 0.3)
    mask = None
    if mask_kind == "random":
        mask = (torch.rand(b, h, w, generator=g) < 0.6).to(torch.uint8) * 7          # nonzero -> 1
    elif mask_kind == "zero":
        mask = torch.zeros(b, h, w, dtype=torch.uint8)
    elif mask_kind == "one":
        mask = torch.zeros(b, h, w, dtype=torch.uint8)
        mask[b - 1, h // 2, w - 1] = 1
    x, r = (t.contiguous(memory_format=torch.channels_last) for t in (x, r))
    return x, r, mask, is_gt


def jac_bound(q, G, Gm, eps, c):
    return 2.0 * eps * G + q * (2.0 * Gm + 2.0 * c * eps * G)


def kind_bounds(name, x, r, mask, is_gt, cw):
    """(bound of the value, bound per gradient element) of one kind at unit weight and gout = 1, without the final roundings"""
    x, r = x.double(), r.double()
    b, c, h, w = x.shape
    M, eps = float(b * h * w), (c + 10) * U
    ep = 0.0 if is_gt else eps
    m = torch.ones(b, 1, h, w, dtype=torch.float64) if mask is None else (mask != 0).double().view(b, 1, h, w)
    q, logq = torch.softmax(x, 1), torch.log_softmax(x, 1)
    p = r if is_gt else torch.softmax(r, 1)
    if name == "kl":
        if is_gt:
            pk = torch.where(r != 0, torch.ones_like(r), torch.full_like(r, K.P8))
            S = pk.sum(1, keepdim=True)
            return float((m * eps * S).sum()) / M, (m / M) * eps * S * torch.ones_like(q)
        pix = eps * ((torch.log_softmax(r, 1) - logq).abs().sum(1, keepdim=True) + 2.01)
        return float((m * pix).sum()) / M, (m / M) * eps * (c * q + 2.01)
    if name in ("ce", "weighted ce"):
        wv = (torch.ones(c, dtype=torch.float64) if name == "ce" else normalised_weights(cw, c)).view(1, c, 1, 1)
        R = float(m.sum())
        if R == 0.0:
            return 0.0, torch.zeros_like(q)
        pix = (wv * (ep * logq.abs() + p * eps)).sum(1, keepdim=True)
        return float((m * pix).sum()) / R, (m / R) * (eps * (wv * p).sum(1, keepdim=True) + ep * (q * float(wv.sum()) + wv))
    if name == "mse":
        e2, d = eps + ep, (q - p).abs()
        a = 2.0 * m / M
        return float((m * (2.0 * d * e2 + e2 * e2)).sum()) / M, jac_bound(q, a * d.amax(1, keepdim=True), a * e2, eps, c)
    if name == "Dice":
        bc = float(b * c)
        I = (m * q * p).sum((2, 3), keepdim=True) + SMOOTH
        Un = (m * q).sum((2, 3), keepdim=True) + (m * p).sum((2, 3), keepdim=True) + SMOOTH
        dI = (m * (q * ep + p * eps + eps * ep)).sum((2, 3), keepdim=True)
        dU = (m * (eps + ep)).sum((2, 3), keepdim=True)
        assert bool((Un > 2.0 * dU).all())
        lo, hi = (I - dI).clamp_min(0.0), I + dI
        term = torch.maximum(2.0 * hi / (Un - dU) - 2.0 * I / Un, 2.0 * I / Un - 2.0 * lo / (Un + dU))
        c0, c1 = 2.0 / Un, 2.0 * I / (Un * Un)
        dc0 = 2.0 / (Un - dU) - c0
        dc1 = torch.maximum(2.0 * hi / (Un - dU) ** 2 - c1, c1 - 2.0 * lo / (Un + dU) ** 2)
        g = -(m / bc) * (c0 * p - c1)
        dg = (m / bc) * (dc0 * (p + ep) + c0 * ep + dc1)
        return float(term.sum()) / bc, jac_bound(q, g.abs().amax(1, keepdim=True), dg.amax(1, keepdim=True), eps, c)
    e_d = eps + ep + 2.0 ** -25
    e_E = 8.0 * e_d
    ex, ey = K.sobel((q - p)[:, 1:])
    coef = 1.0 / (float(c - 1) * M)
    g = K.sobel_t(m * ex, m * ey) * coef
    G = g.abs().amax(1, keepdim=True)
    Gm = torch.full_like(G, 16.0 * (e_E + 8.0 * U) * coef)
    return 0.5 * float((m * (2.0 * (ex.abs() + ey.abs()) * e_E + 2.0 * e_E * e_E)).sum()) * coef, jac_bound(q, G, Gm, eps, c)


class Reference:
    """Per kind, once per input: the statement's value and gradient (unit weight, gout = 1) and their bounds."""

    def __init__(self, x, r, mask, is_gt, cw):
        self.args, self.memo = (x, r, mask, is_gt, cw), {}

    def __getitem__(self, name):
        if name not in self.memo:
            x, r, mask, is_gt, cw = self.args
            loss, grad = K.consistency_and_grad(x, r, [name], [1.0], cw, [0], mask, is_gt)
            self.memo[name] = (float(loss), grad) + kind_bounds(name, x, r, mask, is_gt, cw)
        return self.memo[name]


def kind_args(kinds, cw):
    bits, weights = 0, [0.0] * len(NAMES)
    for name, wt in kinds.items():
        bits |= ops.CONSISTENCY_KINDS[name]
        weights[NAMES.index(name)] = wt
    cwa = (ctypes.c_double * len(cw))(*cw) if "weighted ce" in kinds else None
    return bits, (ctypes.c_double * len(weights))(*weights), cwa


def run_guarded(xd, rd, md, is_gt, kinds, cw, rerun=True):
    """(loss[7] on the host, gradient [B,C,H,W] float64 on the host) of one guarded forward + backward through the C ABI"""
    b, c, h, w = xd.shape
    bits, weights, cwa = kind_args(kinds, cw)
    gout = torch.tensor(0.7, device=DEV)
    gc = GuardedCall(DEV)
    ws = gc.out("ws", lib.ctl_consistency_ws_doubles(bits, b, h, w, c), torch.float64)
    loss = gc.out("loss", 1 + len(NAMES))
    dl = gc.out("dlogit", xd.numel())
    pm = None if md is None else md.data_ptr()

    def launch():
        check(lib.ctl_consistency_fwd(bits, weights, cwa, xd.data_ptr(), rd.data_ptr(), pm, int(is_gt), b, h, w, c, ws.ptr, loss.ptr, sp()), "fwd")
        check(lib.ctl_consistency_bwd(bits, weights, cwa, xd.data_ptr(), rd.data_ptr(), pm, int(is_gt), gout.data_ptr(), ws.ptr, b, h, w, c,
                                      dl.ptr, sp()), "bwd")

    pw, ct = any(n != "contour" for n in kinds), "contour" in kinds
    before = lib.ctl_launch_count()
    gc.run(launch)
    assert lib.ctl_launch_count() - before == 2 * (int(pw) + int(ct)) + 1          # forward passes, one finalize, backward passes
    if rerun:
        gc.rerun(launch)                        # guards, every element written, the same bits again
    return loss.flat().cpu().clone(), dl.view((b, c, h, w), channels_last=True).cpu().double()


def check_set(tag, kinds, ref, got_loss, got_grad):
    """a kind set against the statement: the total, each term and every gradient element within the bounds of the module docstring"""
    total = sum(wt * ref[n][0] for n, wt in kinds.items())
    lb = 1.001 * sum(abs(wt) * ref[n][2] for n, wt in kinds.items()) + U * abs(total) + 1e-12
    assert torch.isfinite(got_loss).all() and torch.isfinite(got_grad).all(), tag
    lerr = abs(float(got_loss[0]) - total)
    assert lerr <= lb, (tag, "total", float(got_loss[0]), total, lb)
    for t, n in enumerate(NAMES):
        if n not in kinds:
            assert float(got_loss[1 + t]) == 0.0, (tag, n)
            continue
        tb = 1.001 * ref[n][2] + U * abs(ref[n][0]) + 1e-12
        terr = abs(float(got_loss[1 + t]) - ref[n][0])
        assert terr <= tb, (tag, n, float(got_loss[1 + t]), ref[n][0], tb)
    gref = GOUT * sum(wt * ref[n][1] for n, wt in kinds.items())
    gb = 1.001 * GOUT * sum(abs(wt) * ref[n][3] for n, wt in kinds.items())
    if "contour" in kinds and len(kinds) > 1:
        gct = GOUT * kinds["contour"] * ref["contour"][1]
        gb = gb + U * ((gref - gct).abs() + gct.abs() + gref.abs()) + 3.0 * U * gb
    else:
        gb = gb + U * gref.abs() + U * gb
    gb = gb + 1e-12 * float(gref.abs().max()) + 1e-30
    frac = float(((got_grad - gref).abs() / gb).max())
    key = "+".join(kinds)
    WORST[key] = (max(WORST.get(key, (0.0, 0.0))[0], lerr / lb), max(WORST.get(key, (0.0, 0.0))[1], frac))
    assert frac <= 1.0, (tag, "gradient", frac, float((got_grad - gref).abs().max()))


@pytest.mark.parametrize("c", CLASSES)
@pytest.mark.parametrize("plane", PLANES, ids=lambda s: "x".join(map(str, s)))
def test_kernels_match_the_host_statement(plane, c):
    h, w = plane
    names = [n for n in NAMES if c > 1 or n != "contour"]
    cw = [0.5 + 0.75 * k + 0.1 * (k % 2) for k in range(c)]
    sets = [{n: WEIGHTS[n]} for n in names] + ([{"kl": 1.0, "contour": 0.5}] if c > 1 else []) + [{n: WEIGHTS[n] for n in names if n != "contour"}]
    if c > 1:
        sets.append({n: WEIGHTS[n] for n in names})
    for b in (1, 3):
        for vi, variant in enumerate(VARIANTS):
            mask_kind = MASKS[(vi + PLANES.index(plane) + CLASSES.index(c) + b) % len(MASKS)]      # every pair occurs over the planes and classes
            x, r, mask, is_gt = make_case(b, c, h, w, variant, mask_kind, 1000 * c + 10 * h + w + b + 7 * vi)
            xd, rd, md = x.to(DEV), r.to(DEV), None if mask is None else mask.to(DEV)
            assert xd.permute(0, 2, 3, 1).is_contiguous() and rd.permute(0, 2, 3, 1).is_contiguous()
            ref = Reference(x, r, mask, is_gt, cw)
            single, bounds = {}, {}
            for kinds in sets:
                tag = (plane, c, b, variant, mask_kind, tuple(kinds))
                loss, grad = run_guarded(xd, rd, md, is_gt, kinds, cw, rerun=len(kinds) != 1 or vi == 0)
                check_set(tag, kinds, ref, loss, grad)
                if len(kinds) == 1:
                    n = next(iter(kinds))
                    single[n], bounds[n] = loss[1 + NAMES.index(n)].clone(), 1.001 * ref[n][2] + U * abs(ref[n][0]) + 1e-12
                    if variant == "equal" and n in ("kl", "mse", "contour") and mask_kind != "zero":
                        assert ref[n][0] == 0.0 and float(ref[n][1].abs().max()) <= 1e-15     # (the bounds above are bounds of 0 here)
                    continue
                # fusion: a term has the bits of the single-kind call, the total is the weighted sum of those terms within the sum of their bounds
                for n in kinds:
                    assert torch.equal(loss[1 + NAMES.index(n)], single[n]), (tag, n)
                fused = sum(wt * float(single[n]) for n, wt in kinds.items())
                assert abs(float(loss[0]) - fused) <= sum(abs(wt) * bounds[n] for n, wt in kinds.items()) + U * abs(fused), tag
    print("consistency-error (largest loss error / bound, largest gradient error / bound): " +
          "; ".join(f"{k}: {v[0]:.3f} / {v[1]:.3f}" for k, v in WORST.items()))


@pytest.mark.parametrize("c", [4, 5])
def test_contour_support(c):
    """output == reference except at one pixel: the gradient is non-zero only inside that pixel's clipped 5x5 neighbourhood (the diagonal
    neighbours get none: that entry of S_x^T S_x + S_y^T S_y is 0) and exactly zero elsewhere (a halo or padding fault would leak); a masked-out pixel contributes nothing."""
    b, h, w = 2, 33, 34
    g = torch.Generator().manual_seed(3 + c)
    base = (torch.randn(b, h, w, c, generator=g) * 2.0).permute(0, 3, 1, 2)
    t = 32 if c <= 4 else 16
    spots = [(0, 0), (h - 1, w - 1)] + [(y, x) for y in (t - 1, t) for x in (t - 1, t)] + [(y, x) for y in (15, 16, 31, 32) for x in (15, 16, 31, 32)]
    rd = base.to(DEV)
    for y, x in dict.fromkeys(spots):
        out = base.clone()
        out[1, :, y, x] += torch.arange(c, dtype=torch.float32) - 1.0
        _, grad = run_guarded(out.to(DEV), rd, None, False, {"contour": 1.0}, None, rerun=False)
        inside = torch.zeros(b, h, w, dtype=torch.bool)
        inside[1, max(0, y - 2):y + 3, max(0, x - 2):x + 3] = True
        nz = (grad != 0).any(1)
        assert not bool((nz & ~inside).any()), (c, y, x, torch.nonzero(nz & ~inside)[:4].tolist())
        assert bool(nz[1, y, x]) and int(nz.sum()) > 1, (c, y, x)
        _, ref = K.consistency_and_grad(out, base, ["contour"], [1.0], gout=GOUT)
        assert float((grad - ref).abs().max()) <= 1e-4 * float(ref.abs().max())
        # the 3x3 responses around the pixel are the only non-zero ones: masked out, nothing is left
        mask = torch.ones(b, h, w, dtype=torch.uint8)
        mask[1, max(0, y - 1):y + 2, max(0, x - 1):x + 2] = 0
        loss, grad = run_guarded(out.to(DEV), rd, mask.to(DEV), False, {"contour": 1.0}, None, rerun=False)
        assert float(loss[0]) == 0.0 and float(grad.abs().max()) == 0.0, (c, y, x)


def test_same_bits_again_in_a_graph_replay_and_off_the_16_byte_rows():
    b, c, h, w = 3, 4, 33, 34
    x, r, mask, _ = make_case(b, c, h, w, "random", "random", 77)
    xd, rd, md = x.to(DEV), r.to(DEV), mask.to(DEV)
    kinds = dict(WEIGHTS)
    cw = [1.0, 2.0, 0.5, 3.0]
    gout = torch.tensor(0.7, device=DEV)
    loss1, terms1, ws = ops.consistency_fwd(xd, rd, kinds, cw, md)
    g1 = ops.consistency_bwd(xd, rd, kinds, gout, ws, cw, md)
    loss2, terms2, ws2 = ops.consistency_fwd(xd, rd, kinds, cw, md)
    g2 = ops.consistency_bwd(xd, rd, kinds, gout, ws2, cw, md)
    assert torch.equal(loss1, loss2) and torch.equal(terms1, terms2) and torch.equal(g1, g2) and torch.equal(ws, ws2)
    # the guarded C-ABI call gives the same bits as the ops wrappers
    gl, gg = run_guarded(xd, rd, md, False, kinds, cw)
    assert torch.equal(gl[0], loss1.cpu()) and torch.equal(gl[1:], terms1.cpu()) and torch.equal(gg, g1.cpu().double())
    # rows of 4 classes off the 16-byte grid take the runtime-count kernels: the same arithmetic, the same bits
    flat = torch.empty(xd.numel() + 1, device=DEV), torch.empty(rd.numel() + 1, device=DEV)
    xo, ro = (f[1:].view(b, h, w, c).permute(0, 3, 1, 2) for f in flat)
    xo.copy_(xd), ro.copy_(rd)
    assert xo.data_ptr() % 16 == 4 and xo.permute(0, 2, 3, 1).is_contiguous()
    loss3, terms3, ws3 = ops.consistency_fwd(xo, ro, kinds, cw, md)
    g3 = ops.consistency_bwd(xo, ro, kinds, gout, ws3, cw, md)
    assert torch.equal(loss3, loss1) and torch.equal(terms3, terms1) and torch.equal(g3, g1)
    # a graph replay of forward + backward
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, stream=side):
        lossg, termsg, wsg = ops.consistency_fwd(xd, rd, kinds, cw, md)
        gg = ops.consistency_bwd(xd, rd, kinds, gout, wsg, cw, md)
    torch.cuda.current_stream().wait_stream(side)
    for _ in range(2):
        termsg.fill_(float("nan")), gg.fill_(float("nan")), wsg.fill_(float("nan"))
        graph.replay()
        torch.cuda.synchronize()
        assert torch.equal(lossg, loss1) and torch.equal(termsg, terms1) and torch.equal(gg, g1) and torch.equal(wsg, ws)


@pytest.mark.parametrize("plane", [(16, 16), (17, 31), (64, 64)], ids=lambda s: "x".join(map(str, s)))
def test_pooling(plane):
    h, w = plane
    for c in (1, 4, 5):
        g = torch.Generator().manual_seed(h + w + c)
        x = (torch.randn(3, h, w, c, generator=g) * 3.0).permute(0, 3, 1, 2)
        xd = x.to(DEV)
        for s in (1, 2, 3, 4):
            ho, wo = h >> s, w >> s
            gc = GuardedCall(DEV)
            y = gc.out("y", 3 * ho * wo * c)
            launch = lambda: check(lib.ctl_avgpool_fwd(xd.data_ptr(), 3, h, w, c, s, y.ptr, sp()), "avgpool_fwd")      # noqa: E731
            gc.run(launch)
            gc.rerun(launch)
            got = y.view((3, c, ho, wo), channels_last=True).cpu()
            want = K.pool(x.double(), s)                                             # the float64 window mean
            spacing = torch.maximum(torch.abs(torch.nextafter(got, got + 1) - got), torch.abs(got - torch.nextafter(got, got - 1))).double()
            assert bool(((got.double() - want).abs() <= spacing).all()), (plane, c, s)
            assert torch.equal(ops.avgpool_fwd(xd, s).cpu(), got)
            gy = (torch.randn(3, ho, wo, c, generator=g)).permute(0, 3, 1, 2)
            gyd = gy.to(DEV)
            gc = GuardedCall(DEV)
            gx = gc.out("gx", x.numel())
            launch = lambda: check(lib.ctl_avgpool_bwd(gyd.data_ptr(), 3, h, w, c, s, gx.ptr, sp()), "avgpool_bwd")     # noqa: E731
            gc.run(launch)
            gc.rerun(launch)
            got = gx.view((3, c, h, w), channels_last=True).cpu()
            want = K.unpool(gy.double(), s, h, w).float()                            # g * 4^-s is exact in fp32
            assert torch.equal(got, want), (plane, c, s)
            assert float(got[:, :, ho << s:].abs().max() if (ho << s) < h else 0.0) == 0.0
            assert float(got[:, :, :, wo << s:].abs().max() if (wo << s) < w else 0.0) == 0.0
            assert torch.equal(ops.avgpool_bwd(gyd, s, (h, w)).cpu(), got)
