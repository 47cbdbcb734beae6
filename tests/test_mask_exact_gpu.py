"""ctl_latent_score, ctl_latent_mask_apply and ctl_latent_mask_fused (csrc/ctl_mask.hip) through the C ABI against the host statement
of scores, selection and masking in oracle/ref_mask.py (checked on the CPU by tests/test_ref_mask_rng_io_cpu.py), with no tolerance.

Gradients are small integers in [-3, 3] stored as fp32 (oracle/mask_cases.py): every partial sum is exact whatever the order, so the
device score must be fp32(sum) * fp32(1 / count) bit for bit, ties are real ties, and masks and masked codes must equal the reference
exactly.  The fixtures put ties where the three rankings (the one-block-per-image kernel, the apply kernel with and without the
split-sum finalise, the bitonic threshold of rows longer than 1024) could treat them differently from the strict '>' of
model_util.py:231-244; the shapes are the smallest that reach each branch of the launch selection.  Codes hold +-0.0, +-inf and
denormals: inf * 0 is NaN on both sides, and NaN payloads are not compared (every other element bit for bit).

Channel-mode rows longer than 1024 cannot be reached: the widest accepted c is 256.  The sign of a ZERO score is not part of the
contract and is the one thing not compared: the channel kernels start their sums from +0.0 and never give -0.0, the spatial kernels
add a pixel's channels to each other and give -0.0 where every gradient of the pixel is -0.0 (the signed_zero fixture does that at
c = 4).  The two zeros compare equal, so they tie in the selection, and masks and masked codes are compared bit for bit all the same.
Score rows that mix +0.0 and -0.0 at will are handed to ctl_latent_mask_apply directly.

The randn checks keep one non-integer case per dispatch branch: the score against float64 within terms * 2^-24 * sum|g| / count, the
first-order bound of a sum of `terms` fp32 summands (terms = hw in channel mode, c in spatial mode, where the final scaling by a
power of two is exact), and the masks against the reference selection applied to the device's own scores."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from cooperative_training_and_latent_space_data_augmentation_amd import ops  # noqa: E402
from cooperative_training_and_latent_space_data_augmentation_amd._ffi import lib, check, CtlError  # noqa: E402
from oracle import mask_cases as MC  # noqa: E402
from oracle import ref_mask as R  # noqa: E402

DEV = "cuda"
GUARD = 1024
NAN = float("nan")


def sp():
    return ops.stream_ptr()


def ptr(t):
    return None if t is None else t.data_ptr()


def dev(a):
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def host(t):
    return t.cpu().numpy()


def same_bits(got, ref, nan_ok=False, zero_sign_ok=False):
    got, ref = np.ascontiguousarray(got), np.ascontiguousarray(ref)
    if got.shape != ref.shape or got.dtype != np.float32 or ref.dtype != np.float32:
        return False
    eq = got.view(np.int32) == ref.view(np.int32)
    if nan_ok:
        eq |= np.isnan(got) & np.isnan(ref)
    if zero_sign_ok:
        eq |= (got == 0) & (ref == 0)
    return bool(eq.all())


def same_score(got, ref):
    """bit for bit, except that a zero score may carry either sign (see the module docstring)"""
    return same_bits(got, ref, zero_sign_ok=True)


class Buffers:
    """device outputs and workspaces of one (shape, mode), every workspace followed by a NaN guard that must stay NaN"""

    def __init__(self, shape, mode):
        n, c, h, w = shape
        self.n, self.c, self.hw, self.mode = n, c, h * w, mode
        self.L = c if mode == 0 else h * w
        self.dims = (n, h * w, c)
        self.masked = torch.empty(n, h * w, c, device=DEV)
        self.mask = torch.empty(n, self.L, device=DEV)
        self.score = torch.empty(n, self.L, device=DEV)
        self.ws_floats = {"score": lib.ctl_latent_score_ws_floats(mode, *self.dims), "apply": lib.ctl_latent_mask_apply_ws_floats(mode, *self.dims),
                          "fused": lib.ctl_latent_mask_fused_ws_floats(mode, *self.dims)}
        self.ws = {k: torch.full((v + GUARD,), NAN, device=DEV) for k, v in self.ws_floats.items()}

    def fresh(self):
        for t in (self.masked, self.mask, self.score):
            t.fill_(NAN)

    def guards_intact(self):
        return all(bool(torch.isnan(self.ws[k][v:]).all()) for k, v in self.ws_floats.items())

    def k_args(self, k, via_device):
        if via_device:
            self.k_dev = torch.tensor([k], dtype=torch.int32, device=DEV)
            return (self.L - 1) // 2, ptr(self.k_dev)          # (the host value is ignored)
        return k, None

    def latent_score(self, grad):
        self.fresh()
        check(lib.ctl_latent_score(self.mode, ptr(grad), ptr(self.score), ptr(self.ws["score"]), *self.dims, sp()), "ctl_latent_score")
        return self.score.clone()

    def apply(self, code, score, k, noise, via_device=False):
        self.fresh()
        kh, kd = self.k_args(k, via_device)
        check(lib.ctl_latent_mask_apply(self.mode, ptr(code), ptr(score), ptr(noise), kh, kd, ptr(self.masked), ptr(self.mask),
                                        ptr(self.ws["apply"]), *self.dims, sp()), "ctl_latent_mask_apply")
        return host(self.masked), host(self.mask)

    def fused(self, grad, code, k, noise, via_device=False, refill=True):
        if refill:
            self.fresh()
        kh, kd = self.k_args(k, via_device)
        check(lib.ctl_latent_mask_fused(self.mode, ptr(grad), ptr(code), ptr(noise), kh, kd, ptr(self.masked), ptr(self.mask), ptr(self.score),
                                        ptr(self.ws["fused"]), *self.dims, sp()), "ctl_latent_mask_fused")
        return host(self.masked), host(self.mask), host(self.score)


def _k_plan(fixture, score_ref, L):
    """(k as passed, the k it means, through a device int32?)"""
    plan = [(k, k, k == MC.device_k_in_range(L)) for k in MC.all_ks(fixture, score_ref)]
    return plan + [(k, R.clamp_k(k, L), True) for k in MC.device_ks_outside(L)]


SHAPE_MODE = [(s, m) for s in MC.SHAPES for m in (0, 1)]
IDS = ["x".join(map(str, s)) + ("-channel" if m == 0 else "-spatial") for s, m in SHAPE_MODE]


@pytest.mark.parametrize("shape,mode", SHAPE_MODE, ids=IDS)
def test_integer_gradients_scores_masks_and_codes_are_exact(shape, mode):
    n, c, h, w = shape
    L = MC.row_len(shape, mode)
    B = Buffers(shape, mode)
    code = MC.code_for(shape, MC.rng_for(shape, "code"))
    code_d = dev(code)
    done = set()
    for fx, grad, T in MC.fixtures_for(shape, mode):
        done.add(fx)
        grad_d = dev(grad)
        score_ref = R.score_exact_f32(grad, mode)
        score_d = B.latent_score(grad_d)
        assert same_score(host(score_d), score_ref), (fx, "score")
        noise = MC.rng_for(shape, mode, fx, "noise").random((n, L), dtype=np.float32)
        noise_d = dev(noise)
        for k_arg, k, via_dev in _k_plan(fx, score_ref, L):
            for soft, soft_d in ((None, None), (noise, noise_d)):
                what = (fx, k_arg, "soft" if soft is not None else "hard")
                mask_ref = R.select(score_ref, k, soft)
                masked_ref = R.apply(code, mask_ref, mode)
                if fx == "all_equal":
                    assert (mask_ref == 1).all()
                masked, mask = B.apply(code_d, score_d, k_arg, soft_d, via_dev)
                assert same_bits(mask, mask_ref), what + ("apply mask",)
                assert same_bits(masked, masked_ref, nan_ok=True), what + ("apply masked",)
                masked, mask, sc = B.fused(grad_d, code_d, k_arg, soft_d, via_dev)
                assert same_score(sc, score_ref), what + ("fused score",)
                assert same_bits(mask, mask_ref), what + ("fused mask",)
                assert same_bits(masked, masked_ref, nan_ok=True), what + ("fused masked",)
                masked2, mask2, sc2 = B.fused(grad_d, code_d, k_arg, soft_d, via_dev, refill=False)
                assert same_bits(sc2, sc) and same_bits(mask2, mask) and same_bits(masked2, masked, nan_ok=True), what + ("second fused call",)
        assert B.guards_intact(), fx
    assert done == {fx for fx in MC.FIXTURES if L >= MC.MIN_LEN[fx]}
    if L >= 2:          # score rows that mix +0.0 and -0.0: they compare equal, so they tie
        score = MC.signed_zero_scores(n, L, MC.rng_for(shape, mode, "szs"))
        assert (np.signbit(score) & (score == 0)).any() and (~np.signbit(score) & (score == 0)).any()
        score_d = dev(score)
        noise = MC.rng_for(shape, mode, "szs", "noise").random((n, L), dtype=np.float32)
        for k_arg, k, via_dev in _k_plan("random", score, L):
            for soft in (None, noise):
                mask_ref = R.select(score, k, soft)
                masked, mask = B.apply(code_d, score_d, k_arg, dev(soft), via_dev)
                assert same_bits(mask, mask_ref), ("signed zero scores", k_arg)
                assert same_bits(masked, R.apply(code, mask_ref, mode), nan_ok=True), ("signed zero scores", k_arg)
        assert B.guards_intact()


@pytest.mark.parametrize("shape,mode", SHAPE_MODE, ids=IDS)
def test_random_gradients_score_bound_and_selection_on_device_scores(shape, mode):
    n, c, h, w = shape
    L, terms = MC.row_len(shape, mode), MC.summands(shape, mode)
    rng = MC.rng_for(shape, mode, "randn")
    grad = rng.standard_normal((n, h * w, c)).astype(np.float32)
    code = rng.standard_normal((n, h * w, c)).astype(np.float32)
    noise = rng.random((n, L), dtype=np.float32)
    B = Buffers(shape, mode)
    grad_d, code_d, noise_d = dev(grad), dev(code), dev(noise)
    ref64 = R.score(grad, mode)
    bound = terms * 2.0 ** -24 * np.abs(grad.astype(np.float64)).sum(axis=1 if mode == 0 else 2) / terms
    score_d = B.latent_score(grad_d)
    err = np.abs(host(score_d).astype(np.float64) - ref64)
    print(f"score: max error / bound = {float((err / bound).max()):.3f}")
    assert (err <= bound).all()
    k = int(L * 0.37)
    for soft, soft_d in ((None, None), (noise, noise_d)):
        mask_ref = R.select(host(score_d), k, soft)
        masked, mask = B.apply(code_d, score_d, k, soft_d)
        assert same_bits(mask, mask_ref) and same_bits(masked, R.apply(code, mask_ref, mode))
        masked, mask, sc = B.fused(grad_d, code_d, k, soft_d)
        assert (np.abs(sc.astype(np.float64) - ref64) <= bound).all()
        mask_ref = R.select(sc, k, soft)
        assert same_bits(mask, mask_ref) and same_bits(masked, R.apply(code, mask_ref, mode))
        assert int((R.select(sc, k) == 0).sum(axis=1).max()) <= k
    assert B.guards_intact()


def test_refusals():
    """every case is refused by the launcher before anything is launched"""
    def bufs(n, hw, c, L):
        return (torch.zeros(n, hw, c, device=DEV), torch.zeros(n, hw, c, device=DEV), torch.zeros(n, L, device=DEV), torch.zeros(n, hw, c, device=DEV),
                torch.zeros(n, L, device=DEV), torch.zeros(max(n * L, n * hw * c) + 64, device=DEV))

    def all_three(mode, n, hw, c, k, scratch=True):
        L = c if mode == 0 else hw
        grad, code, score, masked, mask, ws = bufs(n, hw, c, L)
        w = ptr(ws) if scratch else None
        return [lambda: check(lib.ctl_latent_score(mode, ptr(grad), ptr(score), w, n, hw, c, sp())),
                lambda: check(lib.ctl_latent_mask_apply(mode, ptr(code), ptr(score), None, k, None, ptr(masked), ptr(mask), w, n, hw, c, sp())),
                lambda: check(lib.ctl_latent_mask_fused(mode, ptr(grad), ptr(code), None, k, None, ptr(masked), ptr(mask), ptr(score), w, n, hw, c, sp()))]

    for c in (2, 12, 24, 100, 512):                          # c not in {4, 8, 16, 32, 64, 128, 256}
        for mode in (0, 1):
            for call in all_three(mode, 2, 16, c, 0):
                with pytest.raises(CtlError):
                    call()
    for call in all_three(1, 1, 8193, 4, 0)[1:]:             # spatial L = 8193 (channel-mode L > 1024 would need c > 256: not reachable)
        with pytest.raises(CtlError):
            call()
    for mode, hw, c in ((0, 16, 8), (1, 16, 8), (1, 2048, 4), (0, 2048, 64)):
        L = c if mode == 0 else hw
        for k in (L, -1):                                    # a host k outside [0, L)
            for call in all_three(mode, 1, hw, c, k)[1:]:
                with pytest.raises(CtlError):
                    call()
    score_call, apply_call, fused_call = all_three(0, 1, 2048, 64, 0, scratch=False)      # channel scores need split-sum scratch; 2048 * 64 > 64 Ki
    for call in (score_call, fused_call):
        with pytest.raises(CtlError):
            call()
    score_call, apply_call, fused_call = all_three(1, 1, 2048, 4, 0, scratch=False)       # rows longer than 1024 need threshold scratch
    for call in (apply_call, fused_call):
        with pytest.raises(CtlError):
            call()
    torch.cuda.synchronize()
