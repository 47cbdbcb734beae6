"""The float64 host statement of the consistency losses (consistency.consistency_and_grad) against the recorded outputs of upstream
(tests/golden/consistency_cases.pt, written by tools/gen_golden_consistency.py), against torch.autograd of a restatement written here with
F.conv2d / F.avg_pool2d, and against the CPU branch of the public functions.  No GPU."""
import os

import pytest
import torch
import torch.nn.functional as F

from cooperative_training_and_latent_space_data_augmentation_amd import consistency as K

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "consistency_cases.pt")
NAMES = ["kl", "ce", "weighted ce", "mse", "Dice", "contour"]
U32 = 2.0 ** -24            # unit roundoff of float32


@pytest.fixture(scope="module")
def cases():
    return torch.load(GOLDEN, weights_only=True)["cases"]


def test_recorded_cases_cover_what_they_should(cases):
    got = sorted((q["name"], q["c"], q["is_gt"], q["mask"] is not None) for q in cases)
    want = []
    for c in (2, 4, 5):
        for name in ("kl", "mse", "Dice"):
            want += [(name, c, g, m) for g in (False, True) for m in (False, True)]
        for name in ("ce", "weighted ce"):
            want += [(name, c, g, False) for g in (False, True)]
        want += [("contour", c, True, m) for m in (False, True)]
    assert got == sorted(want)
    for q in cases:
        c, x, r, m = q["c"], q["output"], q["reference"], q["mask"]
        f32 = q["name"] == "contour"
        assert q["dtype"] == ("float32" if f32 else "float64")
        assert x.dtype == r.dtype == q["grad"].dtype == (torch.float32 if f32 else torch.float64)
        assert tuple(x.shape) == tuple(r.shape) == tuple(q["grad"].shape) == (3, c, 7, 9)
        assert len(set(q["class_weights"].tolist())) == c
        if m is not None:
            assert tuple(m.shape) == (3, 1, 7, 9) and set(m.unique().tolist()) == {0.0, 1.0}
        if f32:      # probabilities that are multiples of 2^-4 with rows summing to 1: upstream's float32 Sobel sums and squares are exact
            for t in (x, r):
                assert torch.equal(t * 16, (t * 16).round()) and float(t.min()) >= 1 / 16 and torch.equal(t.sum(1), torch.ones(3, 7, 9))
        elif q["is_gt"]:
            assert set(r.unique().tolist()) == {0.0, 1.0} and torch.equal(r.sum(1), torch.ones(3, 7, 9, dtype=torch.float64))


def test_host_statement_matches_upstream_float64(cases):
    n = 0
    for q in cases:
        if q["dtype"] != "float64":
            continue
        n += 1
        cw = q["class_weights"].tolist() if q["name"] == "weighted ce" else None
        loss, grad = K.consistency_and_grad(q["output"], q["reference"], [q["name"]], [1.0], cw, [0], q["mask"], q["is_gt"])
        assert loss.dtype == grad.dtype == torch.float64
        tag = (q["name"], q["c"], q["is_gt"], q["mask"] is not None)
        assert abs(float(loss) - q["loss"]) <= 1e-12 * abs(q["loss"]), (tag, float(loss), q["loss"])
        assert float((grad - q["grad"]).abs().max()) <= 1e-12 * float(q["grad"].abs().max()), tag
    assert n == 48


def test_host_contour_matches_upstream_float32(cases):
    """Upstream's contour_loss runs in float32 only.  The recorded inputs are probabilities q, p that are multiples of 2^-4 in [1/16, 1]; the
    statement gets x = log q (softmax(log q) = q to 1e-16) and is_gt, and its gradient is compared with the recorded g = d loss / d q taken
    through the softmax Jacobian, q_j (g_j - sum_k q_k g_k).  With u = 2^-24:
      value     Sobel responses are multiples of 2^-4 below 8, their differences and squares (multiples of 2^-8, at most 64) and the sum of
                the 189 squares of a class (below 2^14: 22 bits) are exact.  Each of the two means rounds at most twice, their sum once, the
                factor 1/2 is exact; the C-1 class terms, all >= 0, are added with one rounding each and divided once:
                |loss32 - loss| <= (C + 4) u loss.
      gradient  g is a sum of at most 12 products (6 per filter) of exact small integers with 2 m E / (N (C-1)), which carry at most 3
                roundings each (the division by the class count and the two of the mean's backward), and the sum adds at most 6 more:
                |dg_k| <= 10 u A_k with A_k = (|S_x|^T |m E_x| + |S_y|^T |m E_y|)_k / ((C-1) M), hence
                |d(dloss/dx_j)| <= q_j (|dg_j| + sum_k q_k |dg_k|).
    1e-12 relative is added for the float64 side."""
    n = 0
    for q in cases:
        if q["dtype"] != "float32":
            continue
        n += 1
        c, qq, p = q["c"], q["output"].double(), q["reference"].double()
        m = torch.ones(3, 1, 7, 9, dtype=torch.float64) if q["mask"] is None else q["mask"].double()
        loss, grad = K.consistency_and_grad(torch.log(qq), p, ["contour"], [1.0], None, [0], q["mask"], True)
        assert abs(float(loss) - q["loss"]) <= (c + 4) * U32 * float(loss) + 1e-12 * float(loss), (c, float(loss), q["loss"])
        g = q["grad"].double()
        assert torch.equal(g[:, 0], torch.zeros(3, 7, 9, dtype=torch.float64))
        want = qq * (g - (qq * g).sum(1, keepdim=True))
        ex, ey = K.sobel((qq - p)[:, 1:])
        ax, ay = (m * ex).abs(), (m * ey).abs()
        wx = torch.tensor([[1.0, 0, 1], [2, 0, 2], [1, 0, 1]], dtype=torch.float64).view(1, 1, 3, 3)
        a = torch.zeros_like(qq)
        for k in range(c - 1):
            a[:, k + 1] = (F.conv2d(ax[:, [k]], wx, padding=1) + F.conv2d(ay[:, [k]], wx.transpose(2, 3), padding=1))[:, 0]
        dg = 10 * U32 * a / ((c - 1) * 189.0)
        bound = qq * (dg + (qq * dg).sum(1, keepdim=True)) + 1e-12 * want.abs().max()
        worst = float(((grad - want).abs() / bound).max())
        print(f"contour float32 C={c} mask={q['mask'] is not None}: loss rel err {abs(float(loss) - q['loss']) / float(loss):.2e}, "
              f"gradient err / bound {worst:.3f}")
        assert worst <= 1.0, (c, worst)
    assert n == 6


SX = torch.tensor([[1.0, 0, -1], [2, 0, -2], [1, 0, -1]], dtype=torch.float64).view(1, 1, 3, 3)
SY = torch.tensor([[1.0, 2, 1], [0, 0, 0], [-1, -2, -1]], dtype=torch.float64).view(1, 1, 3, 3)


def restated(x, r, names, weights, cw, scales, mask, is_gt):
    """The module docstring's total from torch primitives (conv2d, avg_pool2d), for autograd."""
    b, c = x.shape[:2]
    total = 0.0
    for s in scales:
        xs, rs = (F.avg_pool2d(x, 2 ** s), F.avg_pool2d(r, 2 ** s)) if s else (x, r)
        h, w = xs.shape[2:]
        M = b * h * w
        m = torch.ones(b, 1, h, w, dtype=torch.float64) if mask is None else (mask.reshape(b, 1, h, w) != 0).double()
        q, logq = torch.softmax(xs, 1), torch.log_softmax(xs, 1)
        p = rs if is_gt else torch.softmax(rs, 1)
        for name, weight in zip(names, weights):
            if name == "kl":
                if is_gt:
                    p32 = torch.where(rs == 0, 1e-8, 1 - 1e-8)               # upstream's line: a float32 tensor
                    assert p32.dtype == torch.float32
                    pk, plogp = p32.double(), (p32 * torch.log(p32)).double()
                else:
                    pk, plogp = p, p * torch.log_softmax(rs, 1)
                l = (m * (plogp - pk * logq)).sum(1).sum() / M
            elif name in ("ce", "weighted ce"):
                wn = torch.ones(c, dtype=torch.float64) if name == "ce" else torch.tensor(cw, dtype=torch.float64) / sum(cw) * c
                l = -(m * wn.view(1, c, 1, 1) * p * logq).sum() / m.sum() if float(m.sum()) else xs.sum() * 0.0
            elif name == "mse":
                l = F.mse_loss(q * m, p * m, reduction="sum") / M
            elif name == "Dice":
                qm, pm = (q * m).flatten(2), (p * m).flatten(2)
                l = 1.0 - (2.0 * ((qm * pm).sum(2) + 0.01) / (qm.sum(2) + pm.sum(2) + 0.01)).sum() / (b * c)
            else:
                l = 0.0
                for k in range(1, c):
                    gx = (F.conv2d(q[:, [k]], SX, padding=1) - F.conv2d(p[:, [k]], SX, padding=1)) * m
                    gy = (F.conv2d(q[:, [k]], SY, padding=1) - F.conv2d(p[:, [k]], SY, padding=1)) * m
                    l = l + 0.5 * ((gx ** 2).mean() + (gy ** 2).mean())
                l = l / (c - 1)
            total = total + 2 ** s * weight * l
    return total / len(scales)


def inputs(c, h, w, is_gt, masked, seed):
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(2, c, h, w, generator=g, dtype=torch.float64) * 3.0
    r = torch.randn(2, c, h, w, generator=g, dtype=torch.float64) * 3.0
    if is_gt:      # soft probabilities with some exact zeros (the 'kl' rule looks at r == 0)
        r = torch.softmax(r, 1) * (torch.rand(2, c, h, w, generator=g, dtype=torch.float64) > 0.3)
    m = (torch.rand(2, 1, h, w, generator=g) < 0.6).to(torch.int32) * 3 if masked else None      # any dtype, nonzero -> 1
    return x, r, m


@pytest.mark.parametrize("c", [1, 2, 4, 5, 16])
@pytest.mark.parametrize("is_gt", [False, True])
@pytest.mark.parametrize("scales, hw, masked", [([0], (7, 9), False), ([0], (7, 9), True), ([1], (7, 9), False), ([0, 1, 2], (13, 18), False)])
def test_statement_is_exact(c, is_gt, scales, hw, masked):
    x, r, m = inputs(c, hw[0], hw[1], is_gt, masked, 100 * c + len(scales))
    names = [n for n in NAMES if c > 1 or n != "contour"]
    weights = [1.0, 0.5, 0.3, 2.0, 0.7, 1.5][:len(names)]
    cw = [0.5 + 0.75 * k for k in range(c)]
    for sel in [[n] for n in names] + [names]:
        ws = [weights[names.index(n)] for n in sel]
        loss, grad = K.consistency_and_grad(x, r, sel, ws, cw, scales, m, is_gt, gout=1.7)
        xr = x.clone().requires_grad_(True)
        want = restated(xr, r, sel, ws, cw, scales, m, is_gt)
        gwant, = torch.autograd.grad(want * 1.7, [xr])
        want = want.detach()
        assert abs(float(loss) - float(want)) <= 1e-12 * max(abs(float(want)), 1e-3), (sel, float(loss), float(want))
        assert float((grad - gwant).abs().max()) <= 1e-12 * max(float(gwant.abs().max()), 1e-6), sel
        # the CPU branch of the public function: the same arithmetic from torch ops, differentiable
        xp = x.clone().requires_grad_(True)
        pub = K.calc_segmentation_consistency(xp, r, sel, ws, cw, scales, m, is_gt)
        gpub, = torch.autograd.grad(pub * 1.7, [xp])
        pub = pub.detach()
        assert pub.dtype == torch.float64 and abs(float(pub) - float(loss)) <= 1e-12 * max(abs(float(loss)), 1e-3), sel
        assert float((gpub - grad).abs().max()) <= 1e-12 * max(float(grad.abs().max()), 1e-6), sel


def test_floor_drops_rows_and_columns_and_an_empty_mask_is_zero():
    x, r, _ = inputs(3, 7, 9, False, False, 5)
    _, grad = K.consistency_and_grad(x, r, ["kl", "mse"], [1.0, 1.0], None, [2])
    assert float(grad[:, :, 4:].abs().max()) == 0.0 == float(grad[:, :, :, 8:].abs().max()) and float(grad[:, :, :4, :8].abs().min()) > 0.0
    zero = torch.zeros(2, 7, 9, dtype=torch.uint8)
    for name in NAMES:
        loss, grad = K.consistency_and_grad(x, r, [name], [1.0], [1.0, 2.0, 3.0], [0], zero)
        assert float(grad.abs().max()) == 0.0 and float(loss) == (1.0 - 2.0 * 0.01 / 0.01 if name == "Dice" else 0.0), name


def test_public_wrappers_on_the_cpu_in_float32():
    x, r, m = inputs(4, 7, 9, False, True, 9)
    x32 = x.float().requires_grad_(True)
    loss = K.calc_segmentation_consistency(x32, r.float(), mask=m)
    assert loss.dtype == torch.float32 and loss.requires_grad
    assert abs(float(loss.detach()) - float(K.consistency_and_grad(x.float(), r.float(), mask=m)[0])) < 1e-5
    for got, want in ((K.kl_divergence(r, x, mask=m), K.consistency_and_grad(x, r, ["kl"], [1.0], mask=m)[0]),
                      (K.kl_divergence(r, x, is_gt=True), K.consistency_and_grad(x, r, ["kl"], [1.0], is_gt=True)[0]),
                      (K.calc_segmentation_mse_consistency(x, r), K.consistency_and_grad(x, r, ["mse"], [1.0])[0]),
                      (K.calc_segmentation_kl_consistency(x, r), K.consistency_and_grad(x, r, ["kl"], [1.0])[0])):
        assert abs(float(got) - float(want)) <= 1e-12 * abs(float(want))


@pytest.mark.parametrize("fn", [K.consistency_and_grad, K.calc_segmentation_consistency])
def test_errors(fn):
    x, r = torch.zeros(2, 4, 6, 5, dtype=torch.float64), torch.zeros(2, 4, 6, 5, dtype=torch.float64)
    m = torch.ones(2, 1, 6, 5)
    for name in ("contour_smooth", "dice", "KL", "hausdorff"):
        with pytest.raises(NotImplementedError):
            fn(x, r, [name], [1.0])
    with pytest.raises(ValueError, match="class weights"):
        fn(x, r, ["weighted ce"], [1.0])
    with pytest.raises(ValueError, match="weight"):
        fn(x, r, ["weighted ce"], [1.0], [1.0, 2.0, 3.0])
    with pytest.raises(ValueError, match="mask"):
        fn(x, r, ["kl"], [1.0], None, [0, 1], m)
    with pytest.raises(ValueError, match="mask"):
        fn(x, r, ["kl"], [1.0], None, [0], torch.ones(2, 4, 6, 5))
    with pytest.raises(ValueError, match="smaller"):
        fn(x, r, ["kl"], [1.0], None, [3])                     # 6x5 against an 8x8 window
    for scales in ([5], [-1], []):
        with pytest.raises(ValueError, match="scales"):
            fn(x, r, ["kl"], [1.0], None, scales)
    with pytest.raises(ValueError, match="2 classes"):
        fn(x[:, :1], r[:, :1], ["contour"], [1.0])
    with pytest.raises(ValueError, match="constant"):
        fn(x, r.clone().requires_grad_(True), ["kl"], [1.0])
    with pytest.raises(ValueError, match="shape"):
        fn(x, r[:, :3], ["kl"], [1.0])
    with pytest.raises(ValueError, match="weights"):
        fn(x, r, ["kl", "mse"], [1.0])
    fn(x, r, ["kl"], [1.0], None, [2])                         # 6x5 holds one 4x4 window
