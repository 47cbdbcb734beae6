"""Host emulation of CTL_DT_X3 (csrc/ctl_conv_x3_stage.h), product by product, on inputs that make the low-order products visible.

The X3 kernels split both fp32 operands exactly into three bf16 numbers and accumulate six of the nine plane products:
hi*hi + hi*mid + mid*hi + mid*mid + hi*lo + lo*hi.  On Gaussian data the last three are 2^-16 ... 2^-18 of a result that hi*hi dominates,
so no tolerance separates a kernel that forms six products from one that forms five.  The operands built here are `big + tail`:
`big` a small bf16-exact integer arranged so that the hi*hi products CANCEL exactly inside one matrix instruction, `tail` 15 random bits
below 2^-8 that fill the mid and lo planes.  What is left of the result are the cross terms, of which mid*mid, hi*lo and lo*hi are about
1e-3 each: a missing, duplicated or mis-addressed product moves the result by >= 3e-4 of max|ref|, a correct kernel by ~1e-6.

  forward / data gradients (contraction over tap x input channel):  big_x[:, 2j+1] = big_x[:, 2j],  big_w[:, 2j+1] = -big_w[:, 2j]
  weight gradients (contraction over n x pixel):  big_x constant along every row,  big_dy[..., 2j+1] = -big_dy[..., 2j] along x, and
      big_dy = 0 in the first and last pixel pair of a row (and in the last column of an odd width), where the zero padding of x breaks
      the pairing.

Everything is fp64 arithmetic on exact bf16 planes with exact products and sums (tests/test_x3_products_cpu.py checks the conditions this
relies on); only the final result is rounded to fp32.  tests/test_x3_products_gpu.py runs the same operands through the kernels.
No GPU code here."""
import functools
from collections import namedtuple

import torch
import torch.nn.functional as F

TERMS = ("hh", "hm", "mh", "mm", "hl", "lh")             # plane of the first operand (x), plane of the second (weights / output gradient)
# what a kernel with ONE wrong matrix instruction computes: each of the five low-order products missing, and a cross term formed twice
# in place of its mirror image (a swapped plane offset)
VARIANTS = ("drop hm", "drop mh", "drop mm", "drop hl", "drop lh", "hm for mh", "hl for lh")


def _bf16(x64):
    """round-to-nearest-even bf16 of values that are exact in fp32 (asserted), as fp64"""
    x32 = x64.float()
    assert torch.equal(x32.double(), x64), "not an fp32 number"
    return x32.to(torch.bfloat16).double()


def split3(x):
    """the exact three-way split of an fp32 tensor: fp64 planes (hi, mid, lo) with hi = bf16(x), mid = bf16(x - hi), lo = x - hi - mid"""
    assert x.dtype == torch.float32
    x64 = x.double()
    hi = _bf16(x64)
    mid = _bf16(x64 - hi)
    lo = x64 - hi - mid
    assert torch.equal(hi + mid + lo, x64), "hi + mid + lo != x"
    assert torch.equal(_bf16(lo), lo), "lo is not a bf16 number"
    return hi, mid, lo


# ------------------------------------------------------------------------------------------------ operands
def _bigs(shape, g, values=(1, 2, 3)):
    v = torch.tensor(values, dtype=torch.float64)[torch.randint(0, len(values), shape, generator=g)]
    return v * (torch.randint(0, 2, shape, generator=g).double() * 2 - 1)


def with_tail(big, g, step=2.0 ** -23, kmax=32768, same_sign=False):
    """fp32(big + k * step), k uniform in [-kmax, kmax): |tail| <= 2^-8 with the defaults, so bf16(big + tail) == big -- except just BELOW
    a power of two, where bf16 is twice as fine: a tail that points towards zero from |big| = 1 is halved (same_sign: it takes the sign of
    `big` instead, for operands whose sums must stay exact).  Asserts hi == big wherever big != 0."""
    k = torch.randint(-kmax, kmax, big.shape, generator=g).double()
    tail = k * step
    if same_sign:
        tail = torch.where(big != 0, tail.abs() * torch.sign(big), tail)
    else:
        tail = torch.where((big.abs() == 1) & (tail * big < 0), tail * 0.5, tail)
    x = (big + tail).float()
    hi = split3(x)[0]
    assert torch.equal(hi[big != 0], big[big != 0]), "bf16(big + tail) != big"
    return x


def forward_operands(n, cin, cout, h, w, ks, g, summed=False):
    """x [n, cin, h, w] and the source weights [cout, cin, ks, ks] with their `big` parts.  summed: the pack kernel adds up to four of these
    weights in fp32 (phase and pooled packs) -- big = +-1 and tails of the same sign on a 2^-21 grid keep every partial sum exact."""
    bx = _bigs((n, cin // 2, h, w), g).repeat_interleave(2, 1)
    bw = _bigs((cout, cin // 2, ks, ks), g, (1,) if summed else (1, 2, 3)).repeat_interleave(2, 1)
    bw[:, 1::2] = -bw[:, 1::2]
    x = with_tail(bx, g)
    wt = with_tail(bw, g, 2.0 ** -21, 8192, True) if summed else with_tail(bw, g)
    return x, wt, bx, bw


LIVE_PIXELS = 2048


def wgrad_operands(n, cin, cout, h, w, ho, wo, g):
    """x [n, cin, h, w] and dy [n, cout, ho, wo] of a weight gradient, with their `big` parts.  Of a large problem only LIVE_PIXELS pixels
    (expected; whole rows, drawn at random) carry an output gradient, the other rows of dy are zero: every hi*hi instruction whose
    +-1 ... +-9 products cancel costs the small sum it meets a few low bits (as if the matrix pipe aligned its accumulator to the largest
    product it adds) -- a loss that grows with the NUMBER of such instructions behind one output element (measured on the dense
    (8, 64, 64, 48, 64) problem: 3.8e-5 of max|ref| on conv_wgrad_x3pc16_kernel, 2.3e-5 on conv_wgrad_x3_kernel, next to 1.4e-5 of the
    fp32-MFMA kernel; 1.8e-7 with the same tails and no integers) and says nothing about WHICH products are formed."""
    bx = _bigs((n, cin, h, 1), g).expand(n, cin, h, w).contiguous()
    half = _bigs((n, cout, ho, wo // 2), g)
    bdy = torch.zeros(n, cout, ho, wo, dtype=torch.float64)
    bdy[..., 0:2 * (wo // 2):2] = half
    bdy[..., 1:2 * (wo // 2):2] = -half
    bdy[..., :2] = 0
    bdy[..., 2 * (wo // 2) - 2:] = 0          # the last pair, and the last column of an odd width
    x, dy = with_tail(bx, g), with_tail(bdy, g)
    live = torch.rand((n, 1, ho, 1), generator=g) < LIVE_PIXELS / float(n * ho * wo)
    return x, dy * live, bx, bdy * live


# ------------------------------------------------------------------------------------------------ the operations, bilinear, in fp64
def virtual_input(x, in_mode):
    """what the conv sees of the stored tensor: 0 itself, 1 its nearest up-sampling, 2 its zero-inserted form (the CTL_IN_* codes)"""
    if in_mode == 1:
        return F.interpolate(x, scale_factor=2, mode="nearest")
    if in_mode == 2:
        z = torch.zeros(x.shape[0], x.shape[1], 2 * x.shape[2], 2 * x.shape[3], dtype=x.dtype)
        z[:, :, ::2, ::2] = x
        return z
    return x


def effective_weights(wt, pack):
    """The weights the conv kernel is handed, [phase][cout][cin][k][k] in fp64, as the pack kernels form them from the source weights
    [cout][cin][3][3] (x3_pack_value in csrc/ctl_conv_x3.hip): pack 0 the weights themselves; 1 the 4x4 stride-2 kernel of
    sumpool2(conv3x3^T(.)); 2 the four 2x2 phase kernels of a 3x3 conv on a nearest-up-sampled input; 3 the four 2x2 phase kernels of the
    data gradient of a stride-2 3x3 conv.  Linear in wt."""
    w64 = wt.double()
    co, ci = w64.shape[:2]
    if pack == 0:
        return w64[None]
    if pack == 1:
        out = torch.zeros(1, co, ci, 4, 4, dtype=torch.float64)
        for kh in range(4):
            for kw in range(4):
                for a in range(2):
                    for b in range(2):
                        sh, sw = a + 2 - kh, b + 2 - kw
                        if 0 <= sh <= 2 and 0 <= sw <= 2:
                            out[0, :, :, kh, kw] += w64[:, :, sh, sw]
        return out
    out = torch.zeros(4, co, ci, 2, 2, dtype=torch.float64)
    for z in range(4):
        a, b = z >> 1, z & 1
        for kh in range(2):
            for kw in range(2):
                if pack == 2:
                    rows = range(0, (1 if a else 0) + 1) if kh == 0 else range(2 if a else 1, 3)
                    cols = range(0, (1 if b else 0) + 1) if kw == 0 else range(2 if b else 1, 3)
                    for sh in rows:
                        for sw in cols:
                            out[z, :, :, kh, kw] += w64[:, :, sh, sw]
                else:
                    sh = (2 if kh == 0 else 0) if a else (1 if kh == 0 else -1)
                    sw = (2 if kw == 0 else 0) if b else (1 if kw == 0 else -1)
                    if sh >= 0 and sw >= 0:
                        out[z, :, :, kh, kw] = w64[:, :, sh, sw]
    return out


def forward_op(c):
    """(x plane [n, cin, h, w], effective-weight plane [phase][cout][cin][k][k]) -> the conv of case `c` in fp64"""
    def op(xp, wp):
        if c.pack in (2, 3):        # four 2x2 convs on the stored input, scattered to the phases of a 2h x 2w output
            n, _, h, w = xp.shape
            pad = F.pad(xp, (1, 1, 1, 1)) if c.pack == 2 else F.pad(xp, (0, 1, 0, 1))
            y = torch.zeros(n, wp.shape[1], 2 * h, 2 * w, dtype=torch.float64)
            for z in range(4):
                a, b = z >> 1, z & 1
                src = pad[:, :, a:a + h + 1, b:b + w + 1] if c.pack == 2 else pad
                y[:, :, a::2, b::2] = F.conv2d(src, wp[z])
            return y
        return F.conv2d(virtual_input(xp, c.in_mode), wp[0], stride=c.stride, padding=1 if c.ks in (3, 4) else 0)
    return op


def forward_check(c, x, wt):
    """the same result from the SOURCE weights through torch's own up-sampling / transposed convs: the phase and pooled forms above are
    not assumed to be right"""
    x64, w64 = x.double(), wt.double()
    if c.pack == 1:
        return F.avg_pool2d(F.conv_transpose2d(x64, w64.permute(1, 0, 2, 3), padding=1), 2) * 4.0
    if c.pack == 2:
        return F.conv2d(F.interpolate(x64, scale_factor=2, mode="nearest"), w64, padding=1)
    if c.pack == 3:
        return F.conv_transpose2d(x64, w64.permute(1, 0, 2, 3), stride=2, padding=1, output_padding=1)
    return F.conv2d(virtual_input(x64, c.in_mode), w64, stride=c.stride, padding=1 if c.ks in (3, 4) else 0)


def wgrad_op(c):
    """(x plane [n, cin, h, w], dy plane [n, cout, ho, wo]) -> dW [cout, cin, ks, ks] in fp64, one matrix product per tap"""
    def op(xp, dyp):
        p = 1 if c.ks == 3 else 0
        xin = F.pad(virtual_input(xp, 1 if c.up else 0), (p, p, p, p))
        ho, wo = dyp.shape[2:]
        dw = torch.zeros(dyp.shape[1], xp.shape[1], c.ks, c.ks, dtype=torch.float64)
        for kh in range(c.ks):
            for kw in range(c.ks):
                xs = xin[:, :, kh:kh + c.stride * (ho - 1) + 1:c.stride, kw:kw + c.stride * (wo - 1) + 1:c.stride]
                dw[:, :, kh, kw] = torch.einsum("noyx,niyx->oi", dyp, xs)
        return dw
    return op


# ------------------------------------------------------------------------------------------------ six products, five products
def terms(xplanes, wplanes, op):
    """the six results of `op` over the plane pairs the kernels multiply, by name (TERMS)"""
    idx = {"h": 0, "m": 1, "l": 2}
    return {t: op(xplanes[idx[t[0]]], wplanes[idx[t[1]]]) for t in TERMS}


def variant(tm, name):
    """fp64 sum of the six terms with ONE product wrong: "drop t" or "t for u" (t formed twice, u never)"""
    six = sum(tm.values())
    if name.startswith("drop "):
        return six - tm[name[5:]]
    t, u = name.split(" for ")
    return six - tm[u] + tm[t]


def _rel(got64, ref, scale):
    return float((got64.float().double() - ref).abs().max()) / scale      # (one rounding to fp32, as the kernel's store)


Emulation = namedtuple("Emulation", "case x w big_zero check_err ref scale e6 five five_min hh_max")


def emulate(c, x, w2, op, big_zero, check_err):
    """ref = op on the full operands; e6 = error of the six-product sum; five = error of every VARIANT (all relative to max|ref|)"""
    ref = op(x.double(), w2.double())
    tm = terms(split3(x), split3(w2), op)
    scale = max(float(ref.abs().max()), 1e-300)
    five = {v: _rel(variant(tm, v), ref, scale) for v in VARIANTS}
    return Emulation(c, x, w2, big_zero, check_err, ref, scale, _rel(sum(tm.values()), ref, scale), five, min(five.values()),
                     float(tm["hh"].abs().max()) / scale)


# ------------------------------------------------------------------------------------------------ cases
# Forward and data-gradient launches (ctl_conv_forward_ex).  h, w: the STORED input; pack: effective_weights; pro: ctl_conv.pro_affine,
# run with identity coefficients; epi: "" | "res" (residual epilogue, res = 0) | "bnbwd" (CTL_EPI_BNBWD, factor 1) | "tail"
# (CTL_EPI_TAILBWD, factor 1); form: the profiling id of the instantiation the library must pick (ctl_prof_begin: kernel family, kernel
# size, stride, input mode, pixel tile mt x tw, cout tiles per block, epilogue class, two-tensor prologue, narrow cout).
Fwd = namedtuple("Fwd", "name n cin cout h w ks stride in_mode pack nsub pro epi form")


def _fwd(name, n, cin, cout, h, w, form, ks=3, stride=1, in_mode=0, pack=0, nsub=1, pro=0, epi=""):
    return Fwd(name, n, cin, cout, h, w, ks, stride, in_mode, pack, nsub, pro, epi, form)


FWD_CASES = [
    # 3x3 stride 1, plain input, single-role kernel: the three pixel tiles, one and two cout tiles per block, a padded cout tile
    _fwd("s1_4x16_nt1", 2, 16, 16, 32, 32, "conv_igemm_x3<ks3,s1,in0,mt1,tw16,nt1>"),
    _fwd("s1_4x16_nt1_ragged", 2, 16, 16, 9, 8, "conv_igemm_x3<ks3,s1,in0,mt1,tw16,nt1>", pro=1),
    _fwd("s1_4x16_nt1_cout4", 2, 16, 4, 40, 40, "conv_igemm_x3<ks3,s1,in0,mt1,tw16,nt1,co4>"),
    _fwd("s1_4x16_nt2", 2, 32, 64, 16, 16, "conv_igemm_x3<ks3,s1,in0,mt1,tw16,nt2>"),
    _fwd("s1_8x16_nt1", 4, 16, 16, 128, 128, "conv_igemm_x3<ks3,s1,in0,mt2,tw16,nt1>"),
    _fwd("s1_8x16_nt2_ragged", 6, 16, 64, 62, 60, "conv_igemm_x3<ks3,s1,in0,mt2,tw16,nt2>", pro=1),
    _fwd("s1_8x32_nt1", 8, 16, 16, 128, 128, "conv_igemm_x3<ks3,s1,in0,mt4,tw32,nt1>"),
    _fwd("s1_8x32_nt2", 4, 16, 64, 128, 128, "conv_igemm_x3<ks3,s1,in0,mt4,tw32,nt2>"),
    _fwd("s1_bnbwd_x2", 2, 16, 16, 32, 32, "conv_igemm_x3<ks3,s1,in0,mt1,tw16,nt1,e3,x2>", pro=2, epi="bnbwd"),
    # 3x3 stride 1, plain input, producer / consumer kernel
    _fwd("pc_4x16", 16, 128, 128, 16, 16, "conv_igemm_x3pc<ks3,s1,in0,mt1,tw16,nt2>"),
    _fwd("pc_8x16", 8, 128, 128, 32, 32, "conv_igemm_x3pc<ks3,s1,in0,mt2,tw16,nt2>", pro=1),
    _fwd("pc_8x32", 8, 64, 64, 64, 64, "conv_igemm_x3pc<ks3,s1,in0,mt4,tw32,nt2>"),
    _fwd("pc_bnbwd", 16, 128, 128, 16, 16, "conv_igemm_x3pc<ks3,s1,in0,mt1,tw16,nt2,e3>", epi="bnbwd"),
    _fwd("pc_x2", 8, 128, 128, 32, 32, "conv_igemm_x3pc<ks3,s1,in0,mt2,tw16,nt2,x2>", pro=2),
    # the other forward and data-gradient forms
    _fwd("k4s2_x2", 2, 32, 32, 16, 16, "conv_igemm_x3<ks4,s2,in0,mt1,tw16,nt1,x2>", ks=4, stride=2, pro=2),
    _fwd("up2_res", 2, 16, 16, 16, 16, "conv_igemm_x3<ks3,s1,in1,mt1,tw16,nt1,e1>", in_mode=1, epi="res"),
    _fwd("zins2_res", 2, 32, 16, 12, 10, "conv_igemm_x3<ks3,s1,in2,mt1,tw16,nt1,e1>", in_mode=2, epi="res"),
    _fwd("zins2_tail", 2, 16, 32, 8, 8, "conv_igemm_x3<ks3,s1,in2,mt1,tw16,nt2,e2>", in_mode=2, epi="tail"),
    _fwd("k3s2", 2, 16, 32, 32, 32, "conv_igemm_x3<ks3,s2,in0,mt1,tw16,nt1>", stride=2, pro=1),
    _fwd("k4s2_pooled", 2, 32, 16, 16, 16, "conv_igemm_x3<ks4,s2,in0,mt1,tw16,nt1>", ks=4, stride=2, pack=1),
    _fwd("phases_up2", 2, 16, 16, 16, 16, "conv_igemm_x3<ks2,s1,in0,mt1,tw16,nt1>", ks=2, pack=2, nsub=4),
    _fwd("phases_dgrad", 3, 32, 16, 12, 10, "conv_igemm_x3<ks2,s1,in0,mt1,tw16,nt1>", ks=2, pack=3, nsub=4),
    _fwd("k2s2", 2, 16, 16, 16, 16, "conv_igemm_x3<ks2,s2,in0,mt1,tw16,nt1>", ks=2, stride=2),
    _fwd("k2s2_tail", 2, 32, 32, 12, 20, "conv_igemm_x3<ks2,s2,in0,mt1,tw16,nt2,e2>", ks=2, stride=2, epi="tail"),
]

# Weight gradients.  h, w: the STORED input; up: behind a nearest up-sampling; pro: activation prologue (identity coefficients); virt: the
# output gradient is the virtual tensor A * dy + B * dy2 + C with (A, B, C) = (1, 0, 0); grouped: through ctl_conv_wgrad_group (the only
# entry that runs conv_wgrad_x3pc16_kernel in the shipped build) instead of ctl_conv_wgrad_ex (conv_wgrad_x3_kernel).
Wg = namedtuple("Wg", "name n cin cout h w ks stride up pro virt groups accumulate grouped form")


def _wg(name, n, cin, cout, h, w, form, ks=3, stride=1, up=False, pro=False, virt=False, groups=1, accumulate=False, grouped=False):
    return Wg(name, n, cin, cout, h, w, ks, stride, up, pro, virt, groups, accumulate, grouped, form)


WGRAD_CASES = [
    _wg("plain", 2, 16, 16, 32, 32, "conv_wgrad_x3<ks3,s1,in0,mt2,tw16,nt1>"),
    _wg("ragged", 2, 64, 32, 24, 20, "conv_wgrad_x3<ks3,s1,in0,mt2,tw16,nt2>", pro=True),
    _wg("ragged_odd_width", 2, 16, 16, 9, 7, "conv_wgrad_x3<ks3,s1,in0,mt2,tw16,nt1>"),
    _wg("low_4x16", 2, 32, 32, 6, 12, "conv_wgrad_x3<ks3,s1,in0,mt1,tw16,nt2>"),
    _wg("up2", 2, 32, 16, 16, 16, "conv_wgrad_x3<ks3,s1,in1,mt2,tw16,nt1>", up=True),
    _wg("s2", 2, 16, 32, 32, 32, "conv_wgrad_x3<ks3,s2,in0,mt1,tw16,nt2>", stride=2, pro=True),
    _wg("k2s2", 2, 32, 32, 16, 16, "conv_wgrad_x3<ks2,s2,in0,mt2,tw16,nt2>", ks=2, stride=2),
    _wg("virtual_dy_groups2", 4, 32, 64, 24, 40, "conv_wgrad_x3<ks3,s1,in0,mt2,tw16,nt2,x2>", virt=True, groups=2),
    _wg("accumulate", 2, 32, 16, 12, 20, "conv_wgrad_x3<ks3,s1,in0,mt2,tw16,nt1>", accumulate=True),
    _wg("pc16_128", 8, 128, 128, 32, 32, "conv_wgrad_x3grp<in0>", grouped=True),
    _wg("pc16_64", 8, 64, 64, 48, 64, "conv_wgrad_x3grp<in0>", grouped=True),
    _wg("pc16_virtual_dy_groups2", 4, 32, 64, 16, 24, "conv_wgrad_x3grp<in0,x2>", virt=True, groups=2, grouped=True),
    _wg("pc16_up2", 8, 128, 64, 16, 16, "conv_wgrad_x3grp<in1>", up=True, pro=True, grouped=True),
    _wg("pc16_up2_virtual_dy", 4, 32, 32, 8, 12, "conv_wgrad_x3grp<in1,x2>", up=True, virt=True, grouped=True),
]
# one grouped launch with two members of different shape (ragged tiles, another split count each)
GROUP_PAIR = (_wg("pair_a", 3, 64, 32, 20, 28, "conv_wgrad_x3grp<in0>", pro=True, grouped=True),
              _wg("pair_b", 2, 32, 96, 33, 17, "conv_wgrad_x3grp<in0>", grouped=True))


def _gen(c):
    return torch.Generator().manual_seed(sum((i + 1) * 7919 * ord(ch) for i, ch in enumerate(c.name)) % (2 ** 31))


@functools.lru_cache(maxsize=None)
def forward_case(c):
    """Emulation of a FWD_CASES entry; .w holds the SOURCE weights [cout, cin, 3 or ks, ...] the pack kernels are given.  Computed once
    per process: the CPU and the GPU test of a case share it."""
    g = _gen(c)
    x, wt, bx, bw = forward_operands(c.n, c.cin, c.cout, c.h, c.w, 3 if c.pack else c.ks, g, summed=c.pack in (1, 2))
    eff = effective_weights(wt, c.pack)
    assert torch.equal(eff.float().double(), eff), "an effective weight is not an fp32 number: the pack kernel's sum would round"
    op = forward_op(c)
    big_eff = effective_weights(bw, c.pack)
    assert torch.equal(big_eff[:, :, 1::2], -big_eff[:, :, 0::2]), "the pairing of big_w does not survive the pack"
    big_zero = float(op(bx, big_eff).abs().max())
    e = emulate(c, x, eff.float(), op, big_zero, 0.0)
    chk = float((forward_check(c, x, wt) - e.ref).abs().max()) / e.scale
    return e._replace(w=wt, check_err=chk)


@functools.lru_cache(maxsize=None)
def wgrad_case(c):
    """Emulation of a WGRAD_CASES / GROUP_PAIR entry; .w holds dy"""
    g = _gen(c)
    ho, wo = (c.h * 2, c.w * 2) if c.up else ((c.h + c.stride - 1) // c.stride, (c.w + c.stride - 1) // c.stride)
    x, dy, bx, bdy = wgrad_operands(c.n, c.cin, c.cout, c.h, c.w, ho, wo, g)
    op = wgrad_op(c)
    big_zero = float(op(bx, bdy).abs().max())
    wt = torch.zeros(c.cout, c.cin, c.ks, c.ks, dtype=torch.float64, requires_grad=True)
    xin = virtual_input(x.double(), 1 if c.up else 0)
    F.conv2d(xin, wt, stride=c.stride, padding=1 if c.ks == 3 else 0).backward(dy.double())
    e = emulate(c, x, dy, op, big_zero, 0.0)
    return e._replace(check_err=float((wt.grad - e.ref).abs().max()) / e.scale)
