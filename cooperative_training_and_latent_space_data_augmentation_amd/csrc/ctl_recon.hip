// Image-similarity (reconstruction) losses between a prediction x and a constant target t (medseg/models/custom_loss.py: smooth_l1_loss
// :310-318, CustomNormalizedCrossCorrelationLoss :514-571, CustomLocalNormalizedCrossCorrelationLoss :574-661, next to 'mse' and 'l1') of
// fp32 NHWC tensors with an optional per-pixel uint8 mask that multiplies both.  Definitions: include/ctl_hip.h, "image-similarity losses".
//
// 'mse', 'l1', 'smooth l1' and 'ncc' read x, t and the mask ONCE: one streaming pass leaves ordered fp64 block sums (the three point-wise
// sums and, per channel, sum x, t, x^2, t^2, x t: the products of two floats are exact in fp64), one finalize block forms every term, the
// weighted total and the per-sample table of the 'ncc' gradient.  'lncc' is a windowed second-order statistic: it works over 16 x 16 pixel
// tiles with the channel-summed I, J, I^2, J^2, I J of the tile plus a halo of win / 2 in LDS as fp64, takes separable row-then-column window
// sums, keeps the per-centre arithmetic in fp64 and leaves three coefficient maps in the workspace.  Backward: ONE launch writes
// gout * sum_k weight_k dL_k/dx rounded once -- a streaming launch, or with 'lncc' a tiled launch that stages the three maps with the same
// halo, takes their window sums and adds the point-wise kinds in the same thread.  Sums are two-stage and ordered: no float atomics,
// nothing is read back, the same bits on every call and in a graph replay.
#include "ctl_rows.h"

#define EB CTL_ROW_THREADS   // threads per block
#define RECON_NK 5           // kinds
#define RECON_STREAM (CTL_RECON_MSE | CTL_RECON_L1 | CTL_RECON_SMOOTH_L1 | CTL_RECON_NCC)
#define RECON_ALL (RECON_STREAM | CTL_RECON_LNCC)
#define RECON_T 16           // tile edge of the 'lncc' passes: T * T = EB, one thread per centre
#define RECON_MAX_WIN 15
#define RECON_MAX_STREAM_BLOCKS 2048
#define RECON_MAX_TILE_BLOCKS 2048
#define RECON_PW_SCALARS 3   // per-block sums in front of the per-channel ones: mse, l1, smooth l1
#define RECON_EPS 1e-6
#define RECON_FLAT 0x1p-40   // a variance <= RECON_FLAT * (its sum of squares) counts as 0

struct recon_wk { double v[RECON_NK]; };      // weight of each kind (0 where the kind is not selected)
// the backward's constants: 2 w_mse / N, w_l1 / N, w_sl1 / N, w_ncc / b, w_lncc / (b h w) (the sum forms: without the divisors, lncc times c)
struct recon_bw { double cm, cl, cs, cn, cw, beta; int kinds; };

// ------------------------------------------------------------------------------------------------ streaming kinds, forward
// grid (blocks of a sample, sample); partial[b][block][3 + 5c]: sum d^2, sum |d|, sum smooth-l1(d), then per channel sum x, t, x^2, t^2, x t
// of the masked-in pixels (a masked-out pixel has J = I = 0 and adds nothing).  Every entry is written (0 for a kind that is not selected).
template <int CT>
__global__ __launch_bounds__(EB) void recon_stream_partial_kernel(const float* __restrict__ xs, const float* __restrict__ ts,
                                                                   const uint8_t* __restrict__ mask, int64_t hw, int c_rt, int64_t t_stride,
                                                                   int kinds, double beta, double* __restrict__ partial) {
#pragma clang fp contract(off)
    constexpr int NC = CT ? CT : CTL_ROW_MAXC;
    constexpr int NV = RECON_PW_SCALARS + 5 * CTL_ROW_MAXC;
    __shared__ double sm[EB / 64][NV];
    const int c = CT ? CT : c_rt;
    const int64_t b = blockIdx.y;
    const float* __restrict__ x = xs + b * hw * c;
    const float* __restrict__ t = ts + b * t_stride;
    const uint8_t* __restrict__ mk = mask ? mask + b * hw : nullptr;
    const bool mse = kinds & CTL_RECON_MSE, l1 = kinds & CTL_RECON_L1, sl1 = kinds & CTL_RECON_SMOOTH_L1, ncc = kinds & CTL_RECON_NCC;
    double sc[RECON_PW_SCALARS], ch[5][NC];
#pragma unroll
    for (int j = 0; j < RECON_PW_SCALARS; ++j) sc[j] = 0.0;
#pragma unroll
    for (int k = 0; k < NC; ++k) { ch[0][k] = 0.0; ch[1][k] = 0.0; ch[2][k] = 0.0; ch[3][k] = 0.0; ch[4][k] = 0.0; }
    const int64_t stride = (int64_t)gridDim.x * EB;
    for (int64_t i = (int64_t)blockIdx.x * EB + threadIdx.x; i < hw; i += stride) {
        if (mk && mk[i] == 0) continue;
        float xv[NC], tv[NC];
        ctl_row_load<CT>(x, i, c, xv);
        ctl_row_load<CT>(t, i, c, tv);
#pragma unroll
        for (int k = 0; k < NC; ++k) if (k < c) {
            const double xd = (double)xv[k], td = (double)tv[k], d = xd - td, n = fabs(d);
            if (mse) sc[0] += d * d;
            if (l1) sc[1] += n;
            if (sl1) sc[2] += n < beta ? 0.5 * (n * n) / beta : n - 0.5 * beta;
            if (ncc) { ch[0][k] += xd; ch[1][k] += td; ch[2][k] += xd * xd; ch[3][k] += td * td; ch[4][k] += xd * td; }
        }
    }
    const int wv = threadIdx.x >> 6;
    const bool first = (threadIdx.x & 63) == 0;
#pragma unroll
    for (int j = 0; j < RECON_PW_SCALARS; ++j) { const double a = wave_sum_double(sc[j]); if (first) sm[wv][j] = a; }
#pragma unroll
    for (int k = 0; k < NC; ++k) if (k < c) {
#pragma unroll
        for (int q = 0; q < 5; ++q) { const double a = wave_sum_double(ch[q][k]); if (first) sm[wv][RECON_PW_SCALARS + 5 * k + q] = a; }
    }
    const int nv = RECON_PW_SCALARS + 5 * c;
    CTL_BLOCK_ROWS_STORE(sm, EB / 64, nv, partial + (b * gridDim.x + blockIdx.x) * nv);
}

// ------------------------------------------------------------------------------------------------ 'lncc': the separable window sums
// Q planes of HD x HD doubles in `src` (HD = T + win - 1) -> window sums at the T x T centres.  Rows first (rs[Q][HD][T], each sum in
// index order), then columns.  Every thread of the block calls it; thread i owns centre (i / T, i % T) and gets out[Q].
template <int Q>
__device__ __forceinline__ void recon_window_sums(const double* __restrict__ src, double* __restrict__ rs, int hd, int win, double* out) {
    constexpr int T = RECON_T;
    for (int i = threadIdx.x; i < hd * T; i += EB) {
        const int yy = i / T, lx = i % T;
#pragma unroll
        for (int q = 0; q < Q; ++q) {
            const double* __restrict__ row = src + (q * hd + yy) * hd + lx;
            double a = 0.0;
            for (int k = 0; k < win; ++k) a += row[k];
            rs[q * hd * T + i] = a;
        }
    }
    __syncthreads();
    const int ly = threadIdx.x / T, lx = threadIdx.x % T;
#pragma unroll
    for (int q = 0; q < Q; ++q) {
        const double* __restrict__ col = rs + (q * hd + ly) * T + lx;
        double a = 0.0;
        for (int k = 0; k < win; ++k) a += col[k * T];
        out[q] = a;
    }
}

// ------------------------------------------------------------------------------------------------ 'lncc', forward
// One block per tile of T x T centres (grid-stride over the tiles of every sample).  LDS: the channel sums of I, J, I^2, J^2, I J at halo
// win / 2 (zero outside the plane and where the mask is 0), then the row sums.  maps[b][h][w][3] = a_p, b_p, b_p uJ_p - a_p uI_p;
// partial[block] = the sum of the scores of its tiles.
template <int CT>
__global__ __launch_bounds__(EB) void recon_lncc_fwd_kernel(const float* __restrict__ xs, const float* __restrict__ ts,
                                                             const uint8_t* __restrict__ mask, int b, int h, int w, int c_rt, int64_t t_stride,
                                                             int win, int tiles_y, int tiles_x, double* __restrict__ maps,
                                                             double* __restrict__ partial) {
#pragma clang fp contract(off)
    constexpr int NC = CT ? CT : CTL_ROW_MAXC;
    constexpr int T = RECON_T;
    extern __shared__ __attribute__((aligned(16))) double lds[];
    __shared__ double sm[EB / 64];
    const int c = CT ? CT : c_rt;
    const int r = win / 2, hd = T + 2 * r;
    double* __restrict__ st = lds;                    // [5][hd][hd]
    double* __restrict__ rs = lds + 5 * hd * hd;      // [5][hd][T]
    const double A = (double)(win * win);
    const int64_t ntiles = (int64_t)b * tiles_y * tiles_x;
    double acc = 0.0;
    for (int64_t tl = blockIdx.x; tl < ntiles; tl += gridDim.x) {
        const int tx = (int)(tl % tiles_x), ty = (int)((tl / tiles_x) % tiles_y);
        const int64_t s = tl / ((int64_t)tiles_x * tiles_y);
        const int y0 = ty * T, x0 = tx * T;
        const float* __restrict__ x = xs + s * (int64_t)h * w * c;
        const float* __restrict__ t = ts + s * t_stride;
        for (int i = threadIdx.x; i < hd * hd; i += EB) {
            const int yy = i / hd, xx = i % hd, gy = y0 + yy - r, gx = x0 + xx - r;
            double v[5] = {0.0, 0.0, 0.0, 0.0, 0.0};
            bool on = gy >= 0 && gy < h && gx >= 0 && gx < w;
            if (on && mask) on = mask[(s * h + gy) * w + gx] != 0;
            if (on) {
                float xv[NC], tv[NC];
                const int64_t pix = (int64_t)gy * w + gx;
                ctl_row_load<CT>(x, pix, c, xv);
                ctl_row_load<CT>(t, pix, c, tv);
#pragma unroll
                for (int k = 0; k < NC; ++k) if (k < c) {
                    const double jd = (double)xv[k], id = (double)tv[k];
                    v[0] += id; v[1] += jd; v[2] += id * id; v[3] += jd * jd; v[4] += id * jd;
                }
            }
#pragma unroll
            for (int q = 0; q < 5; ++q) st[q * hd * hd + i] = v[q];
        }
        __syncthreads();
        double ws5[5];
        recon_window_sums<5>(st, rs, hd, win, ws5);
        const int gy = y0 + (int)threadIdx.x / T, gx = x0 + (int)threadIdx.x % T;
        if (gy < h && gx < w) {
            const double I_sum = ws5[0], J_sum = ws5[1], I2_sum = ws5[2], J2_sum = ws5[3], IJ_sum = ws5[4];
            const double uI = I_sum / A, uJ = J_sum / A;
            const double cross = IJ_sum - uJ * I_sum - uI * J_sum + uI * uJ * A;
            const double I_var = I2_sum - 2.0 * uI * I_sum + uI * uI * A;
            const double J_var = J2_sum - 2.0 * uJ * J_sum + uJ * uJ * A;
            const bool flat_i = I_var <= RECON_FLAT * I2_sum, flat_j = J_var <= RECON_FLAT * J2_sum;
            const double sI = flat_i ? 0.0 : sqrt(I_var), sJ = flat_j ? 0.0 : sqrt(J_var);
            const double D = sI * sJ + RECON_EPS;
            const double ap = 1.0 / D;
            const double bp = flat_j ? 0.0 : cross * sI / (D * D * sJ);
            acc += cross / D;
            double* __restrict__ mp = maps + ((s * h + gy) * w + gx) * 3;
            mp[0] = ap; mp[1] = bp; mp[2] = bp * uJ - ap * uI;
        }
        __syncthreads();
    }
    acc = ctl_block_sum_double<EB / 64>(acc, sm);
    if (threadIdx.x == 0) partial[blockIdx.x] = acc;
}

// ------------------------------------------------------------------------------------------------ finalize, one block
// Sums the block rows in a fixed order; the first lane of each 16-lane group leaves the five sums of a (sample, channel) in chs; one thread
// per sample then forms s_b, the subtracted means and the two coefficients of the 'ncc' gradient; thread 0 forms the terms (fp64, each
// rounded once) and the weighted total.
__global__ __launch_bounds__(EB) void recon_finalize_kernel(const double* __restrict__ pw, int b, int nb, int c, double hw,
                                                             const double* __restrict__ lp, int ncb, int kinds, recon_wk wk, int zero_mean,
                                                             int reduce_sum, double* __restrict__ coefb, double* __restrict__ bars,
                                                             double* __restrict__ chs, float* __restrict__ loss) {
#pragma clang fp contract(off)
    __shared__ double sm[EB / 64];
    const int nv = RECON_PW_SCALARS + 5 * c;
    double tot[RECON_NK];      // sum d^2, sum |d|, sum smooth-l1, sum of the ncc scores, sum of the lncc scores
#pragma unroll
    for (int j = 0; j < RECON_PW_SCALARS; ++j) {
        double s = 0.0;
        if (pw) for (int i = threadIdx.x; i < b * nb; i += EB) s += pw[(int64_t)i * nv + j];
        tot[j] = ctl_block_sum_double<EB / 64>(s, sm);
        __syncthreads();
    }
    const bool ncc = pw && (kinds & CTL_RECON_NCC);
    const int lane = threadIdx.x & 15, grp = threadIdx.x >> 4;
    for (int base = 0; base < b * c; base += EB / 16) {
        const int it = base + grp;
        const bool ok = it < b * c;
        const int64_t sb = ok ? it / c : 0;
        const int k = ok ? it % c : 0;
        double v[5] = {0.0, 0.0, 0.0, 0.0, 0.0};
        if (ok && ncc) {
            for (int j = lane; j < nb; j += 16) {
                const double* __restrict__ e = pw + (sb * nb + j) * nv + RECON_PW_SCALARS + 5 * k;
#pragma unroll
                for (int q = 0; q < 5; ++q) v[q] += e[q];
            }
        }
#pragma unroll
        for (int q = 0; q < 5; ++q) CTL_GROUP16_SUM(v[q]);
        if (ok && lane == 0) {
#pragma unroll
            for (int q = 0; q < 5; ++q) chs[(int64_t)it * 5 + q] = v[q];
        }
    }
    __threadfence_block();
    __syncthreads();
    double acc = 0.0;
    for (int s = threadIdx.x; s < b; s += EB) {
        double dot = 0.0, nx2 = 0.0, nt2 = 0.0;
        for (int k = 0; k < c; ++k) {
            const double* __restrict__ e = chs + ((int64_t)s * c + k) * 5;
            const double sx = e[0], st = e[1], sxx = e[2], stt = e[3], sxt = e[4];
            const double xbar = (ncc && zero_mean) ? sx / hw : 0.0, tbar = (ncc && zero_mean) ? st / hw : 0.0;
            dot += sxt - sx * tbar;
            nx2 += sxx - sx * xbar;
            nt2 += stt - st * tbar;
            bars[((int64_t)s * c + k) * 2] = xbar;
            bars[((int64_t)s * c + k) * 2 + 1] = tbar;
        }
        const double na = sqrt(nx2 > 0.0 ? nx2 : 0.0), nu = sqrt(nt2 > 0.0 ? nt2 : 0.0);
        const double Na = na > RECON_EPS ? na : RECON_EPS, Nu = nu > RECON_EPS ? nu : RECON_EPS;
        coefb[(int64_t)s * 2] = ncc ? 1.0 / (Na * Nu) : 0.0;
        coefb[(int64_t)s * 2 + 1] = (ncc && na > RECON_EPS) ? dot / (Na * Na * Na * Nu) : 0.0;
        acc += ncc ? dot / (Na * Nu) : 0.0;
    }
    tot[3] = ctl_block_sum_double<EB / 64>(acc, sm);
    __syncthreads();
    double s = 0.0;
    if (lp) for (int j = threadIdx.x; j < ncb; j += EB) s += lp[j];
    tot[4] = ctl_block_sum_double<EB / 64>(s, sm);
    if (threadIdx.x == 0) {
        const double nel = reduce_sum ? 1.0 : (double)b * (double)c * hw;
        double term[RECON_NK];
        term[0] = tot[0] / nel;
        term[1] = tot[1] / nel;
        term[2] = tot[2] / nel;
        term[3] = 1.0 - (reduce_sum ? tot[3] : tot[3] / (double)b);
        term[4] = 1.0 - (reduce_sum ? (double)c * tot[4] : tot[4] / ((double)b * hw));
        double total = 0.0;
#pragma unroll
        for (int k = 0; k < RECON_NK; ++k) {
            const bool on = (kinds >> k) & 1;
            total += on ? wk.v[k] * term[k] : 0.0;
            loss[1 + k] = on ? (float)term[k] : 0.f;
        }
        loss[0] = (float)total;
    }
}

// ------------------------------------------------------------------------------------------------ backward
// d(sum of the weighted streaming kinds)/dJ of one element, fp64
__device__ __forceinline__ double recon_pw_grad(double xd, double td, const recon_bw& k, double alpha, double bet, double xbar, double tbar) {
#pragma clang fp contract(off)
    const double d = xd - td;
    const double sgn = d > 0.0 ? 1.0 : (d < 0.0 ? -1.0 : 0.0);
    double g = 0.0;
    if (k.kinds & CTL_RECON_MSE) g += k.cm * d;
    if (k.kinds & CTL_RECON_L1) g += k.cl * sgn;
    if (k.kinds & CTL_RECON_SMOOTH_L1) g += k.cs * (fabs(d) < k.beta ? d / k.beta : sgn);
    if (k.kinds & CTL_RECON_NCC) g -= k.cn * (alpha * (td - tbar) - bet * (xd - xbar));
    return g;
}

// grid (blocks of a sample, sample): the streaming kinds alone
template <int CT>
__global__ __launch_bounds__(EB) void recon_stream_bwd_kernel(const float* __restrict__ xs, const float* __restrict__ ts,
                                                               const uint8_t* __restrict__ mask, const float* __restrict__ gout,
                                                               const double* __restrict__ coefb, const double* __restrict__ bars, int64_t hw,
                                                               int c_rt, int64_t t_stride, recon_bw kb, float* __restrict__ dxs) {
#pragma clang fp contract(off)
    constexpr int NC = CT ? CT : CTL_ROW_MAXC;
    const int c = CT ? CT : c_rt;
    const int64_t b = blockIdx.y;
    const float* __restrict__ x = xs + b * hw * c;
    const float* __restrict__ t = ts + b * t_stride;
    const uint8_t* __restrict__ mk = mask ? mask + b * hw : nullptr;
    float* __restrict__ dx = dxs + b * hw * c;
    const double go = (double)gout[0], alpha = coefb[b * 2], bet = coefb[b * 2 + 1];
    double xbar[NC], tbar[NC];
#pragma unroll
    for (int k = 0; k < NC; ++k) {
        xbar[k] = k < c ? bars[(b * c + k) * 2] : 0.0;
        tbar[k] = k < c ? bars[(b * c + k) * 2 + 1] : 0.0;
    }
    const int64_t stride = (int64_t)gridDim.x * EB;
    for (int64_t i = (int64_t)blockIdx.x * EB + threadIdx.x; i < hw; i += stride) {
        float xv[NC], tv[NC];
        if (mk && mk[i] == 0) {
#pragma unroll
            for (int k = 0; k < NC; ++k) xv[k] = 0.f;
            ctl_row_store<CT>(dx, i, c, xv);
            continue;
        }
        ctl_row_load<CT>(x, i, c, xv);
        ctl_row_load<CT>(t, i, c, tv);
#pragma unroll
        for (int k = 0; k < NC; ++k) if (k < c)
            xv[k] = (float)(go * recon_pw_grad((double)xv[k], (double)tv[k], kb, alpha, bet, xbar[k], tbar[k]));
        ctl_row_store<CT>(dx, i, c, xv);
    }
}

// 'lncc' (and whatever streaming kinds are selected beside it): one block per tile.  LDS: the three maps at halo win / 2 (zero outside the
// plane: no centre there), then the row sums.  dx_q = gout m_q (streaming part - cw (I_q Sa - J_q Sb + Sc)).
template <int CT>
__global__ __launch_bounds__(EB) void recon_lncc_bwd_kernel(const float* __restrict__ xs, const float* __restrict__ ts,
                                                             const uint8_t* __restrict__ mask, const float* __restrict__ gout,
                                                             const double* __restrict__ coefb, const double* __restrict__ bars,
                                                             const double* __restrict__ maps, int b, int h, int w, int c_rt, int64_t t_stride,
                                                             int win, int tiles_y, int tiles_x, recon_bw kb, float* __restrict__ dxs) {
#pragma clang fp contract(off)
    constexpr int NC = CT ? CT : CTL_ROW_MAXC;
    constexpr int T = RECON_T;
    extern __shared__ __attribute__((aligned(16))) double lds[];
    const int c = CT ? CT : c_rt;
    const int r = win / 2, hd = T + 2 * r;
    double* __restrict__ st = lds;                    // [3][hd][hd]
    double* __restrict__ rs = lds + 3 * hd * hd;      // [3][hd][T]
    const double go = (double)gout[0];
    const int64_t ntiles = (int64_t)b * tiles_y * tiles_x;
    for (int64_t tl = blockIdx.x; tl < ntiles; tl += gridDim.x) {
        const int tx = (int)(tl % tiles_x), ty = (int)((tl / tiles_x) % tiles_y);
        const int64_t s = tl / ((int64_t)tiles_x * tiles_y);
        const int y0 = ty * T, x0 = tx * T;
        for (int i = threadIdx.x; i < hd * hd; i += EB) {
            const int yy = i / hd, xx = i % hd, gy = y0 + yy - r, gx = x0 + xx - r;
            const bool on = gy >= 0 && gy < h && gx >= 0 && gx < w;
            const double* __restrict__ mp = maps + ((s * h + (on ? gy : 0)) * w + (on ? gx : 0)) * 3;
#pragma unroll
            for (int q = 0; q < 3; ++q) st[q * hd * hd + i] = on ? mp[q] : 0.0;
        }
        __syncthreads();
        double sw[3];
        recon_window_sums<3>(st, rs, hd, win, sw);
        const int gy = y0 + (int)threadIdx.x / T, gx = x0 + (int)threadIdx.x % T;
        if (gy < h && gx < w) {
            const int64_t pix = (int64_t)gy * w + gx;
            float* __restrict__ dx = dxs + s * (int64_t)h * w * c;
            float xv[NC], tv[NC];
            if (mask && mask[s * (int64_t)h * w + pix] == 0) {
#pragma unroll
                for (int k = 0; k < NC; ++k) xv[k] = 0.f;
            } else {
                ctl_row_load<CT>(xs + s * (int64_t)h * w * c, pix, c, xv);
                ctl_row_load<CT>(ts + s * t_stride, pix, c, tv);
                const double alpha = coefb[s * 2], bet = coefb[s * 2 + 1];
#pragma unroll
                for (int k = 0; k < NC; ++k) if (k < c) {
                    const double xd = (double)xv[k], td = (double)tv[k];
                    double g = 0.0;
                    if (kb.kinds & RECON_STREAM) g = recon_pw_grad(xd, td, kb, alpha, bet, bars[(s * c + k) * 2], bars[(s * c + k) * 2 + 1]);
                    g -= kb.cw * (td * sw[0] - xd * sw[1] + sw[2]);
                    xv[k] = (float)(go * g);
                }
            }
            ctl_row_store<CT>(dx, pix, c, xv);
        }
        __syncthreads();
    }
}

// ------------------------------------------------------------------------------------------------ launchers
static int recon_check(const char* who, int kinds, int64_t b, int64_t h, int64_t w, int c, int win, double beta) {
    CTL_REQUIRE(kinds > 0 && (kinds & ~RECON_ALL) == 0, "%s: kinds 0x%x (a non-empty set of the bits 0x01 .. 0x10)", who, kinds);
    CTL_REQUIRE(b > 0 && h > 0 && w > 0, "%s: sizes must be positive (batch %lld, plane %lld x %lld)", who, (long long)b, (long long)h, (long long)w);
    CTL_REQUIRE(c >= 1 && c <= CTL_ROW_MAXC, "%s: c = %d channels (1 .. %d)", who, c, CTL_ROW_MAXC);
    if (int rc = ctl_check_batch(who, b)) return rc;
    CTL_REQUIRE(h < ((int64_t)1 << 31) / w && b * h * w < ((int64_t)1 << 31) / c,
                "%s: %lld x %lld x %lld pixels of %d channels reach the limit of 2^31 elements", who, (long long)b, (long long)h, (long long)w, c);
    if (kinds & CTL_RECON_SMOOTH_L1) CTL_REQUIRE(std::isfinite(beta) && beta > 0.0, "%s: beta = %g (smooth l1 needs a finite beta > 0)", who, beta);
    if (kinds & CTL_RECON_LNCC) {
        CTL_REQUIRE(win >= 3 && win <= RECON_MAX_WIN && (win & 1), "%s: win = %d (odd, 3 .. %d)", who, win, RECON_MAX_WIN);
        CTL_REQUIRE(win <= h, "%s: win = %d exceeds h = %lld", who, win, (long long)h);
        CTL_REQUIRE(win <= w, "%s: win = %d exceeds w = %lld", who, win, (long long)w);
    }
    return CTL_OK;
}

struct recon_layout { size_t coefb, bars, chs, pw, lp, maps, total; int nb, ncb; };
static recon_layout recon_ws(int kinds, int64_t b, int h, int w, int c) {
    recon_layout l;
    l.nb = ctl_sample_blocks(b, (int64_t)h * w, EB, CTL_RED_BLOCKS);
    l.ncb = ctl_tile_blocks(b, h, w, RECON_T, RECON_MAX_TILE_BLOCKS);
    l.coefb = 0;
    l.bars = l.coefb + (size_t)b * 2;
    l.chs = l.bars + (size_t)b * c * 2;
    l.pw = l.chs + (size_t)b * c * 5;
    l.lp = l.pw + ((kinds & RECON_STREAM) ? (size_t)b * l.nb * (RECON_PW_SCALARS + 5 * c) : 0);
    l.maps = l.lp + ((kinds & CTL_RECON_LNCC) ? (size_t)l.ncb : 0);
    l.total = l.maps + ((kinds & CTL_RECON_LNCC) ? (size_t)b * h * w * 3 : 0);
    return l;
}
static size_t recon_lds(int win, int planes) {
    const int hd = RECON_T + 2 * (win / 2);
    return sizeof(double) * (size_t)planes * (hd * hd + hd * RECON_T);
}

extern "C" size_t ctl_recon_ws_doubles(int32_t kinds, int32_t b, int32_t h, int32_t w, int32_t c, int32_t win) {
    if (recon_check("recon_ws_doubles", kinds, b, h, w, c, win, 1.0) != CTL_OK) return 0;
    return recon_ws(kinds, b, h, w, c).total;
}

extern "C" int ctl_recon_loss_fwd(int32_t kinds, const double* weights, const float* x, const float* t, const uint8_t* mask, int32_t t_batch,
                                  int32_t b, int32_t h, int32_t w, int32_t c, double beta, int32_t win, int32_t zero_mean,
                                  int32_t reduce_sum, double* ws, float* loss, ctl_stream stream) {
    CTL_REQUIRE(x && t && ws && loss, "recon_loss_fwd: null pointer");
    if (int rc = recon_check("recon_loss_fwd", kinds, b, h, w, c, win, beta)) return rc;
    CTL_REQUIRE(t_batch == 1 || t_batch == b, "recon_loss_fwd: t_batch = %d (1, or the batch %d)", t_batch, b);
    recon_wk wk;
    if (int rc = ctl_kind_weights("recon_loss_fwd", kinds, RECON_NK, weights, wk.v)) return rc;
    const recon_layout l = recon_ws(kinds, b, h, w, c);
    const int64_t hw = (int64_t)h * w, t_stride = t_batch == 1 ? 0 : hw * c;
    const bool v4 = ctl_vec4(c, x, t);
    int extra = 0;
    if (kinds & RECON_STREAM) {
        const dim3 grid(l.nb, b);
        CTL_ROW_DISPATCH_C1(recon_stream_partial_kernel, c, v4, grid, 0, x, t, mask, hw, c, t_stride, kinds, beta, ws + l.pw);
        ++extra;
    }
    if (kinds & CTL_RECON_LNCC) {
        const int ty = ctl_cdiv(h, RECON_T), tx = ctl_cdiv(w, RECON_T);
        const size_t lds = recon_lds(win, 5);
        CTL_ROW_DISPATCH_C1(recon_lncc_fwd_kernel, c, v4, dim3(l.ncb), lds, x, t, mask, b, h, w, c, t_stride, win, ty, tx, ws + l.maps, ws + l.lp);
        ++extra;
    }
    recon_finalize_kernel<<<dim3(1), dim3(EB), 0, S_>>>((kinds & RECON_STREAM) ? ws + l.pw : nullptr, b, l.nb, c, (double)hw,
                                                        (kinds & CTL_RECON_LNCC) ? ws + l.lp : nullptr, l.ncb, kinds, wk, zero_mean != 0,
                                                        reduce_sum != 0, ws + l.coefb, ws + l.bars, ws + l.chs, loss);
    ctl_count_launches(extra);
    CTL_LAUNCH_CHECK("recon_loss_fwd");
    return CTL_OK;
}

extern "C" int ctl_recon_loss_bwd(int32_t kinds, const double* weights, const float* x, const float* t, const uint8_t* mask, int32_t t_batch,
                                  const float* gout, const double* ws, int32_t b, int32_t h, int32_t w, int32_t c, double beta, int32_t win,
                                  int32_t zero_mean, int32_t reduce_sum, float* dx, ctl_stream stream) {
    CTL_REQUIRE(x && t && gout && ws && dx, "recon_loss_bwd: null pointer");
    if (int rc = recon_check("recon_loss_bwd", kinds, b, h, w, c, win, beta)) return rc;
    CTL_REQUIRE(t_batch == 1 || t_batch == b, "recon_loss_bwd: t_batch = %d (1, or the batch %d)", t_batch, b);
    recon_wk wk;
    if (int rc = ctl_kind_weights("recon_loss_bwd", kinds, RECON_NK, weights, wk.v)) return rc;
    const recon_layout l = recon_ws(kinds, b, h, w, c);
    const int64_t hw = (int64_t)h * w, t_stride = t_batch == 1 ? 0 : hw * c;
    const double nel = reduce_sum ? 1.0 : (double)b * (double)c * (double)hw;
    recon_bw kb;
    kb.kinds = kinds;
    kb.beta = beta;
    kb.cm = 2.0 * wk.v[0] / nel;
    kb.cl = wk.v[1] / nel;
    kb.cs = wk.v[2] / nel;
    kb.cn = reduce_sum ? wk.v[3] : wk.v[3] / (double)b;
    kb.cw = reduce_sum ? wk.v[4] * (double)c : wk.v[4] / ((double)b * (double)hw);
    const bool v4 = ctl_vec4(c, x, t, dx);
    if (kinds & CTL_RECON_LNCC) {
        const int ty = ctl_cdiv(h, RECON_T), tx = ctl_cdiv(w, RECON_T);
        const size_t lds = recon_lds(win, 3);
        CTL_ROW_DISPATCH_C1(recon_lncc_bwd_kernel, c, v4, dim3(l.ncb), lds, x, t, mask, gout, ws + l.coefb, ws + l.bars, ws + l.maps, b, h, w, c, t_stride, win, ty, tx, kb, dx);
    } else {
        const dim3 grid(ctl_sample_blocks(b, hw, EB, RECON_MAX_STREAM_BLOCKS), b);
        CTL_ROW_DISPATCH_C1(recon_stream_bwd_kernel, c, v4, grid, 0, x, t, mask, gout, ws + l.coefb, ws + l.bars, hw, c, t_stride, kb, dx);
    }
    CTL_LAUNCH_CHECK("recon_loss_bwd");
    return CTL_OK;
}
