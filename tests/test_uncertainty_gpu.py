"""The predictive-uncertainty kernels (csrc/ctl_uncert.hip) through the C ABI against the float64 host statement
uncertainty.predictive_stats_host (never against the code under test).  Every written buffer is exact-sized and poisoned between guard
bands (oracle/guarded.py); every case is launched twice and must give the same bits.

Bounds, from the number formats (u = 2^-24, the unit roundoff of fp32; C classes, T members; expf / logf / log2f are taken as faithful
to 2 u, the division and every add as correctly rounded).  The host reads the SAME fp32 inputs (and the fp32 value of eps), so only the
kernel's own roundings count:
  PB = (C + T + 10) u     on every pbar_k and on conf.  e_k = expf(x_k - m): the subtraction's rounding is an absolute |x_k - m| u in the
       argument, i.e. a relative one in e_k, plus 2 u of expf.  p_k = e_k / s then errs by p_k (|x_k - m| + 2) u from e_k, by
       p_k (sum_j p_j (|x_j - m| + 2) + C) u from s (the members' errors weighted by their share, <= ln C + 3, and C - 1 adds), and u from the
       division.  p_k |x_k - m| <= |d| e^-|d| <= 0.37, so |dp_k| <= (0.37 + 2 + ln 16 + 3 + C + 1) u <= (C + 10) u; the T - 1 adds and
       the division by T add (T + 1) u p <= T u + u.  A probability that underflows to 0 in fp32 is below 2^-126 on the host.
  HB = C (2 C + 2 T + 24) u  on H and on a member's entropy.  A term -p log2(p + eps): d/dp = -(log2 p + 1.45), so dp contributes
       |dp| (|log2 p| + 1.45); with dp <= p (|d| + C + T + 10) u and p |log2 p| (1 + |d|) <= 1.4 this is <= (1.4 + 2 (C + T + 10)) u;
       rounding p + eps, log2f, the product and the running sum add <= 5 u p (|log2 p| + 1) <= 4 u.  C terms.
  MB = 2 HB + 4 u         on MI = H - E (E is a mean of T member entropies, one more division).
  NB = (2 C + T + 32) u max(1, nll)  per labelled pixel.  log p_y = (x_y - m) - logf(s): <= |x_y - m| u + (C + 3 + 2 ln C) u + u |log p_y|,
       and |x_y - m| <= |log p_y|; the log-sum-exp over the members adds expf / logf once more: (T + 6) u.
  BB = C (2 PB + 4 u)     per labelled pixel on brier = sum_k (pbar_k - t_k)^2, |pbar_k - t_k| <= 1.
  The fp64 sums are sums of those fp32 values: a sum's bound is the sum of its pixels' bounds (fp64 rounding is 2^-29 of that).
Exact quantities: the labelled count is equal; yhat is equal except at pixels whose two largest host probabilities are closer than 2 PB
(each may move by PB), and the correct counts differ by no more than the number of such labelled pixels (counted and printed; on an
MI355X: 16 pixel-cases at 4097 pixels and 4 classes, none elsewhere).
  Bin counts are equal except for pixels whose host confidence lies within PB of an edge
float32(j) / float32(B): those are counted, may not exceed 1 % of a case's labelled pixels, and (with the near-ties, for the correct
column) bound the per-bin difference; sum conf (the device's exact integer sum of conf * 2^32) is within pixels * PB of the host's per
slice, summed over the bins.

The seeds of the random cases are such that the host statement alone stays inside the 1 % cap at the small shapes too (one pixel of 56
is 1.8 %); at most 22 pixel-cases per shape lie within PB of an edge.
Largest error / bound seen is printed per test ("uncert-error ..."); on an MI355X: pbar and conf 4.1e-7 / 1.6e-6, H 9.9e-7 / 5.9e-5,
MI 9.4e-7 / 1.1e-4, the sums at most 0.09 of their bounds (the README records them)."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from oracle.guarded import GuardedCall  # noqa: E402
from cooperative_training_and_latent_space_data_augmentation_amd import _ffi, ops, uncertainty as U  # noqa: E402

DEV = "cuda"
lib = _ffi.lib
u = 2.0 ** -24
EPS = float(np.float32(1e-7))
PIXELS = [1, 63, 64, 65, 257, 4097]
CLASSES = [1, 2, 4, 5, 16]
MAPS = ("entropy", "mi", "conf", "pred", "mean_prob")


def PB(c, t): return (c + t + 10) * u                                          # noqa: E704
def HB(c, t): return c * (2 * c + 2 * t + 24) * u                              # noqa: E704
def MB(c, t): return 2 * HB(c, t) + 4 * u                                      # noqa: E704
def NB(c, t, nll): return (2 * c + t + 32) * u * np.maximum(1.0, np.abs(nll))  # noqa: E704
def BB(c, t): return c * (2 * PB(c, t) + 4 * u)                                # noqa: E704


def sp():
    return torch.cuda.current_stream().cuda_stream


def make_logits(t, n, hw, c, seed, kind="random"):
    """fp32 NHWC logits [t*n, hw, c] and labels [n, hw] on the host.  random: 3 N(0,1) with a fifth of the labels out of range (255, -1);
    saturated: every third pixel a row such as (80, -80, 0, ...) rotated over the classes, every member the same there"""
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(t * n, hw, c, generator=g) * 3.0
    y = torch.randint(0, c, (n, hw), generator=g)
    drop = torch.rand(n, hw, generator=g)
    y[drop < 0.1] = 255
    y[(drop >= 0.1) & (drop < 0.2)] = -1
    if kind == "saturated":
        row = torch.zeros(c)
        row[0] = 80.0
        if c > 1:
            row[1] = -80.0
        xv = x.view(t, n * hw, c)
        for i in range(0, n * hw, 3):
            xv[:, i] = torch.roll(row, i % c)
        y = torch.randint(0, c, (n, hw), generator=g)      # every pixel labelled, the far class among them
    return x, y


def as_host_input(x, t, n, hw, c):
    """[t*n, hw, c] fp32 -> the [t*n, c, 1, hw] float64 array the host statement reads"""
    return x.double().numpy().reshape(t * n, 1, hw, c).transpose(0, 3, 1, 2)


class Run:
    """one guarded call of ctl_predictive_stats: every output asked for in `want` (maps) / `tables`, exact-sized"""

    def __init__(self, x, y, t, n, hw, c, b, is_prob, eps=EPS, want=MAPS, tables=True, offset=0):
        self.args = (t, n, hw, c, b)
        self.xd = x.to(DEV).contiguous()
        self.yd = None if y is None else y.to(DEV).contiguous()
        self.gc = GuardedCall(DEV)
        dt = {"pred": torch.uint8}
        self.bufs = {m: self.gc.out(m, n * hw * (c if m == "mean_prob" else 1), dt.get(m, torch.float32)) for m in want}
        if tables:
            self.bufs["stats"] = self.gc.out("stats", n * 6, torch.float64)
            self.bufs["bins"] = self.gc.out("bins", n * b * 3, torch.int64)
        nbytes = lib.ctl_predictive_stats_ws_bytes(t, n, hw, c, b)
        assert nbytes > 0
        ws = self.gc.out("ws", nbytes, torch.uint8, written=False)      # (its 256-byte section padding is never written)
        p = lambda m: self.bufs[m].ptr if m in self.bufs else None      # noqa: E731
        self.launch = lambda: _ffi.check(lib.ctl_predictive_stats(                                        # noqa: E731
            self.xd.data_ptr(), None if self.yd is None else self.yd.data_ptr(), t, n, hw, c, b, eps, int(is_prob), p("entropy"), p("mi"),
            p("conf"), p("pred"), p("mean_prob"), p("stats"), p("bins"), ws.ptr, sp()), "ctl_predictive_stats")
        self.gc.run(self.launch)

    def get(self, m):
        t, n, hw, c, b = self.args
        shape = {"mean_prob": (n, hw, c), "stats": (n, 6), "bins": (n, b, 3)}.get(m, (n, hw))
        return self.bufs[m].flat().view(shape).cpu().numpy()

    def bits(self):
        return {m: g.snapshot().cpu() for m, g in self.bufs.items()}

    def again(self):
        self.gc.rerun(self.launch)                                             # guards, every element written, the same bits


worst, ties = {}, [0]


def note(key, err, bound):
    r = float(err) / float(bound) if bound > 0 else 0.0
    if r >= worst.get(key, (-1.0,))[0]:
        worst[key] = (r, float(err), float(bound))


def compare(run, ref, c, t, b, tag):
    """device outputs of `run` against the host result `ref`; returns the number of near-edge pixels"""
    n = ref.stats.shape[0]
    pb, hb = PB(c, t), HB(c, t)
    ent, mi, conf, pred, mp = (run.get(m) for m in MAPS)
    h_ent, h_mi, h_conf = (np.asarray(a).reshape(n, -1) for a in (ref.entropy, ref.mi, ref.conf))
    h_mp = np.asarray(ref.mean_prob).reshape(n, c, -1).transpose(0, 2, 1)
    for a in (ent, mi, conf, mp):
        assert np.isfinite(a).all(), tag
    for key, got, want, bound in (("H", ent, h_ent, hb), ("MI", mi, h_mi, MB(c, t)), ("conf", conf, h_conf, pb), ("pbar", mp, h_mp, pb)):
        err = np.max(np.abs(got.astype(np.float64) - want))
        note(key, err, bound)
        assert err <= bound, (tag, key, err, bound)
    if t == 1:
        assert (mi == 0).all(), tag
    # arg-max, labelled and correct: exact away from top-two near-ties
    h_nll = np.asarray(ref.nll).reshape(n, -1)
    valid = ~np.isnan(h_nll)
    top2 = np.sort(h_mp, axis=-1)[..., -2:] if c > 1 else None
    tie = (top2[..., 1] - top2[..., 0]) < 2 * pb if c > 1 else np.zeros_like(valid)
    n_tie = (tie & valid).sum(axis=1)
    ties[0] += int(tie.sum())
    assert np.array_equal(pred[~tie], np.asarray(ref.pred).reshape(n, -1)[~tie]), tag
    stats, bins = run.get("stats"), run.get("bins")
    assert np.array_equal(stats[:, 0], ref.stats[:, 0]), (tag, stats[:, 0], ref.stats[:, 0])
    assert (np.abs(stats[:, 1] - ref.stats[:, 1]) <= n_tie).all(), (tag, stats[:, 1], ref.stats[:, 1], n_tie)
    pixels = h_ent.shape[1]
    assert np.isfinite(stats).all(), tag
    sums = (("sum H", 2, np.full(n, pixels * hb)), ("sum MI", 3, np.full(n, pixels * MB(c, t))),
            ("sum nll", 4, np.where(valid, NB(c, t, np.where(valid, h_nll, 0.0)), 0.0).sum(axis=1)), ("sum brier", 5, valid.sum(axis=1) * BB(c, t)))
    for key, col, bound in sums:
        err = np.abs(stats[:, col] - ref.stats[:, col])
        k = int(np.argmax(err - bound))
        note(key, err[k], max(bound[k], 1e-300))
        assert (err <= bound).all(), (tag, key, err, bound)
    # reliability bins
    edges = U.bin_edges(b)
    near = valid & (np.abs(h_conf[..., None] - edges).min(axis=-1) <= pb if b > 1 else np.zeros_like(valid))
    n_near, labelled = near.sum(axis=1), valid.sum(axis=1)
    assert n_near.sum() <= 0.01 * labelled.sum(), (tag, n_near, labelled)
    assert np.array_equal(bins[..., 0].sum(axis=1), stats[:, 0]) and np.array_equal(bins[..., 1].sum(axis=1), stats[:, 1]), tag
    for col, slack in ((0, n_near), (1, n_near + n_tie)):
        assert (np.abs(bins[..., col] - ref.bins[..., col]).max(axis=1) <= slack).all(), (tag, col, bins[..., col], ref.bins[..., col])
    csum = (bins[..., 2].astype(np.float64) / U.CONF_SCALE).sum(axis=1)
    err = np.abs(csum - ref.bins[..., 2].sum(axis=1))
    note("sum conf", err.max(), max(float((labelled * pb).max()), 1e-300))
    assert (err <= labelled * pb + 1e-300).all(), (tag, err, labelled * pb)
    moved = near.sum()
    if moved == 0:                                                              # no pixel near an edge: the per-bin sums agree as well
        assert (np.abs(bins[..., 2].astype(np.float64) / U.CONF_SCALE - ref.bins[..., 2]) <= ref.bins[..., 0] * pb).all(), tag
    return int(moved)


def report(name):
    print(f"uncert-error {name}, {ties[0]} top-two near-ties: " + "; ".join(f"{k} {e:.3e} / {b:.3e}" for k, (r, e, b) in sorted(worst.items())))
    worst.clear()
    ties[0] = 0


@pytest.mark.parametrize("c", CLASSES)
@pytest.mark.parametrize("hw", PIXELS)
def test_every_shape_matches_the_host_statement(hw, c):
    """n in {1, 3} x T in {1, 2, 3} x is_prob off / on x B in {1, 10, 15, 64}, all outputs together, labelled and unlabelled pixels mixed"""
    near = 0
    for n in (1, 3):
        for t in (1, 2, 3):
            x, y = make_logits(t, n, hw, c, seed=20000 * c + 10 * hw + 3 * n + t)
            for is_prob in (False, True):
                xin = torch.softmax(x, dim=-1) if is_prob else x
                host_in = as_host_input(xin, t, n, hw, c)
                for b in (1, 10, 15, 64):
                    ref = U.predictive_stats_host(host_in, y.numpy().reshape(n, 1, hw), members=t, n_bins=b, eps=EPS, is_prob=is_prob)
                    run = Run(xin, y, t, n, hw, c, b, is_prob)
                    near += compare(run, ref, c, t, b, (hw, c, n, t, is_prob, b))
                    if b == 15:
                        run.again()
    report(f"hw={hw} c={c} ({near} pixel-cases within PB of an edge)")


@pytest.mark.parametrize("c", CLASSES)
def test_saturated_rows(c):
    """rows such as (80, -80, 0, ...): entropy 0 there, nothing NaN or Inf, the nll of the far class finite (160)"""
    for t in (1, 2):
        n, hw = 3, 257
        x, y = make_logits(t, n, hw, c, seed=77 + c + t, kind="saturated")
        ref = U.predictive_stats_host(as_host_input(x, t, n, hw, c), y.numpy().reshape(n, 1, hw), members=t, n_bins=15, eps=EPS)
        run = Run(x, y, t, n, hw, c, 15, False)
        compare(run, ref, c, t, 15, ("saturated", c, t))
        ent = run.get("entropy").reshape(-1)[::3]
        assert (np.abs(ent) <= HB(c, t)).all()
        assert np.isfinite(run.get("stats")).all()
        if c > 1:
            assert ref.stats[:, 4].sum() > 160.0 and np.nanmax(ref.nll) >= 159.0     # the far class is among the labels
        run.again()
        # is_prob on the same rows: fp32 probabilities with exact zeros; the labels are moved to the arg-max where the probability of the
        # label is 0 (there nll = +inf by definition, on the host and on the device alike)
        p = torch.softmax(x, dim=-1)
        py = torch.gather(p.view(t, n, hw, c), 3, y.view(1, n, hw, 1).expand(t, n, hw, 1))[..., 0]
        y2 = torch.where((py == 0).any(dim=0), p.view(t, n, hw, c).sum(dim=0).argmax(dim=-1), y)
        ref = U.predictive_stats_host(as_host_input(p, t, n, hw, c), y2.numpy().reshape(n, 1, hw), members=t, n_bins=15, eps=EPS, is_prob=True)
        run = Run(p, y2, t, n, hw, c, 15, True)
        compare(run, ref, c, t, 15, ("saturated-prob", c, t))
    report(f"saturated c={c}")


def test_uniform_logits_sit_beside_an_edge():
    """C = 5, B = 15: conf = float(1) / float(5) exactly, equal to the edge float(3) / float(15), so the strict comparison leaves the pixel
    in bin 2; the expected bin is np.float32 arithmetic, and the device must match it exactly"""
    t, n, hw, c, b = 1, 3, 257, 5, 15
    conf32 = np.float32(1) / np.float32(5)
    want_bin = int(sum(conf32 > np.float32(j) / np.float32(b) for j in range(1, b)))
    assert want_bin == 2 and conf32 == np.float32(3) / np.float32(15)
    for value in (0.0, 0.7, -12.25):
        x = torch.full((t * n, hw, c), value)
        y = torch.zeros((n, hw), dtype=torch.int64)
        run = Run(x, y, t, n, hw, c, b, False)
        assert (run.get("conf").view(np.int32) == conf32.view(np.int32)).all()
        assert (run.get("mean_prob").view(np.int32) == conf32.view(np.int32)).all()
        assert (run.get("pred") == 0).all()                                     # the tie -> the lowest index
        bins = run.get("bins")
        assert (bins[:, want_bin, 0] == hw).all() and (bins[:, want_bin, 1] == hw).all() and bins[..., 0].sum() == n * hw
        assert (bins[:, want_bin, 2] == hw * int(conf32.astype(np.float64) * U.CONF_SCALE)).all()      # the exact integer sum
        ref = U.predictive_stats_host(as_host_input(x, t, n, hw, c), y.numpy().reshape(n, 1, hw), n_bins=b, eps=EPS)
        assert np.abs(run.get("entropy") - ref.entropy.reshape(n, hw)).max() <= HB(c, t)
        assert np.abs(run.get("stats")[:, 4] - ref.stats[:, 4]).max() <= hw * NB(c, t, np.log(5.0))
        run.again()


@pytest.mark.parametrize("c", [4, 5])
def test_unlabelled_pixels_and_absent_label(c):
    """all labels out of range: the tables' labelled columns are zero, the maps are written and are those of the labelled call; label
    NULL: the same"""
    t, n, hw, b = 2, 3, 257, 10
    x, y = make_logits(t, n, hw, c, seed=5 + c)
    full = Run(x, y, t, n, hw, c, b, False)
    out = Run(x, torch.full((n, hw), c, dtype=torch.int64), t, n, hw, c, b, False)
    null = Run(x, None, t, n, hw, c, b, False)
    ref = U.predictive_stats_host(as_host_input(x, t, n, hw, c), None, members=t, n_bins=b, eps=EPS)
    for r in (out, null):
        stats, bins = r.get("stats"), r.get("bins")
        assert (stats[:, [0, 1, 4, 5]] == 0).all() and (bins == 0).all()
        assert np.abs(stats[:, 2] - ref.stats[:, 2]).max() <= hw * HB(c, t) and np.abs(stats[:, 3] - ref.stats[:, 3]).max() <= hw * MB(c, t)
        for m in MAPS:
            assert torch.equal(r.bits()[m], full.bits()[m]), m
        assert np.array_equal(stats[:, 2:4], full.get("stats")[:, 2:4])
        r.again()


@pytest.mark.parametrize("c", [4, 5])
def test_each_output_alone_gives_the_bits_of_all_together(c):
    t, n, hw, b = 2, 3, 257, 15
    x, y = make_logits(t, n, hw, c, seed=31 + c)
    full = Run(x, y, t, n, hw, c, b, False).bits()
    for m in MAPS:
        alone = Run(x, y, t, n, hw, c, b, False, want=(m,), tables=False)
        assert torch.equal(alone.bits()[m], full[m]), m
        alone.again()
    tables = Run(x, y, t, n, hw, c, b, False, want=())
    assert torch.equal(tables.bits()["stats"], full["stats"]) and torch.equal(tables.bits()["bins"], full["bins"])
    tables.again()


def test_c4_off_the_16_byte_grid_gives_the_bits_of_the_aligned_call():
    """rows of 4 channels move as 16 bytes only in 16-byte aligned tensors; views 4 bytes off take the runtime-count kernel: same bits"""
    t, n, hw, c, b = 2, 3, 257, 4, 15
    x, y = make_logits(t, n, hw, c, seed=9, kind="saturated")
    yd = y.to(DEV)
    res = []
    for o in (0, 1):
        bx = torch.zeros(x.numel() + 8, device=DEV)
        xv = bx[o:o + x.numel()]
        xv.copy_(x.reshape(-1))
        assert xv.data_ptr() % 16 == 4 * o
        outs = [torch.full((n * hw,), float("nan"), device=DEV) for _ in range(3)]
        pred = torch.full((n * hw,), 255, dtype=torch.uint8, device=DEV)
        mp = torch.full((n * hw * c,), float("nan"), device=DEV)
        stats = torch.full((n * 6,), float("nan"), dtype=torch.float64, device=DEV)
        bins = torch.full((n * b * 3,), -1, dtype=torch.int64, device=DEV)
        ws = torch.empty(lib.ctl_predictive_stats_ws_bytes(t, n, hw, c, b), dtype=torch.uint8, device=DEV)
        _ffi.check(lib.ctl_predictive_stats(xv.data_ptr(), yd.data_ptr(), t, n, hw, c, b, EPS, 0, outs[0].data_ptr(), outs[1].data_ptr(),
                                            outs[2].data_ptr(), pred.data_ptr(), mp.data_ptr(), stats.data_ptr(), bins.data_ptr(), ws.data_ptr(),
                                            sp()), "ctl_predictive_stats")
        res.append([v.cpu() for v in outs + [pred, mp, stats, bins]])
    for a, q in zip(*res):
        assert torch.equal(a, q)


@pytest.mark.parametrize("c,t", [(4, 1), (4, 2), (5, 3)])
def test_two_calls_and_a_graph_replay_give_identical_bits(c, t):
    n, h, w = 3, 1, 257
    x, y = make_logits(t, n, h * w, c, seed=50 + c)
    xd = x.view(t * n, h, w, c).permute(0, 3, 1, 2).to(DEV)
    yd = y.view(n, h, w).to(DEV)
    assert xd.permute(0, 2, 3, 1).is_contiguous()
    first = ops.predictive_stats(xd, yd, members=t, want=MAPS)
    second = ops.predictive_stats(xd, yd, members=t, want=MAPS)
    for a, q in zip(first, second):
        assert torch.equal(a, q)
    assert first.entropy.shape == (n, h, w) and first.pred.dtype == torch.uint8 and first.mean_prob.shape == (n, c, h, w)
    assert first.stats.shape == (n, 6) and first.bins.shape == (n, 15, 3) and first.bins.dtype == torch.int64
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        replayed = ops.predictive_stats(xd, yd, members=t, want=MAPS)
    for _ in range(2):
        for v in replayed:
            v.fill_(0)
        graph.replay()
        torch.cuda.synchronize()
        for a, q in zip(first, replayed):
            assert torch.equal(a, q)
    del graph
    ref = U.predictive_stats_host(x.double().numpy().reshape(t * n, h, w, c).transpose(0, 3, 1, 2), y.numpy().reshape(n, h, w), members=t, eps=EPS)
    assert np.array_equal(first.pred.cpu().numpy(), ref.pred) and np.array_equal(first.stats[:, :2].cpu().numpy(), ref.stats[:, :2])
    assert np.abs(first.entropy.cpu().numpy() - ref.entropy).max() <= HB(c, t)


def test_entropy_maps_of_a_device_tensor():
    """cal_entropy_maps / cal_batch_entropy_maps with a CUDA tensor: the kernel with is_prob=True; against the numpy path on the same values"""
    g = torch.Generator().manual_seed(3)
    p = torch.softmax(torch.randn(3, 4, 9, 7, generator=g) * 3.0, dim=1)
    for use_max in (False, True):
        for thr in (0.0, 0.3):
            want = U.cal_batch_entropy_maps(p.double().numpy(), eps=EPS, threhold=thr, use_max=use_max)
            got = U.cal_batch_entropy_maps(p.to(DEV), eps=EPS, threhold=thr, use_max=use_max)
            assert got.is_cuda and got.shape == (3, 9, 7)
            got = got.cpu().numpy()
            flipped = (got == 0) != (want == 0)                               # a value within the bound of the threshold may fall either way
            assert (np.abs(want[flipped] - thr) <= HB(4, 1)).all() if flipped.any() else True
            assert np.abs(got - want)[~flipped].max() <= HB(4, 1)
            one = U.cal_entropy_maps(p[1].to(DEV), eps=EPS, threhold=thr, use_max=use_max).cpu().numpy()
            assert np.array_equal(one, got[1])
    with pytest.raises(ValueError):
        ops.predictive_stats(p.to(DEV), want=("variance",))
    with pytest.raises(ValueError):
        ops.predictive_stats(p.to(DEV), members=2)
    with pytest.raises(_ffi.CtlError, match="bins"):
        ops.predictive_stats(p.to(DEV), n_bins=65)
