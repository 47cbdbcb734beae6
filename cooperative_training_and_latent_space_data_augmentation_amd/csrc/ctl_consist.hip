// Consistency losses between two predictions (medseg/models/custom_loss.py: calc_segmentation_consistency :892-973, kl_divergence :863-889,
// soft-target cross_entropy_2D :741-766, the softmax 'mse' :942-952, SoftDiceLoss with a 4-D target :356-396, contour_loss :784-860) of fp32
// NHWC output logits x and reference r, with an optional per-pixel uint8 mask.  Definitions: include/ctl_hip.h, "consistency losses".
//
// Any set of the point-wise / Dice kinds reads x, r and the mask ONCE: one streaming pass leaves fp64 block sums (the masked count among
// them), one finalize block forms every term, the weighted total, 1/R and the Dice coefficient table.  'contour' works over square pixel
// tiles with the softmax difference d = q - p of the classes 1..c-1 in LDS (halo 1; the backward holds d at halo 2 and the masked Sobel
// responses at halo 1) and hands its block sums to the same finalize block.  Backward: one streaming launch writes gout * sum_t weight_t
// dL_t/dx of the point-wise / Dice kinds with both softmaxes recomputed in registers; the contour gradient is a second, tiled launch that
// ADDS into dlogit (it writes dlogit when 'contour' is the only kind).  Sums are two-stage and ordered: no float atomics, nothing is read
// back, the same bits on every call and in a graph replay.
#include "ctl_rows.h"

#define EB CTL_ROW_THREADS   // threads per block
#define CONS_NK 6            // kinds
#define CONS_PW (CTL_CONS_KL | CTL_CONS_CE | CTL_CONS_WCE | CTL_CONS_MSE | CTL_CONS_DICE)
#define CONS_ALL (CONS_PW | CTL_CONS_CONTOUR)
#define CONS_MAX_STREAM_BLOCKS 2048
#define CONS_MAX_TILE_BLOCKS 2048
#define CONS_SCAL 8          // doubles of the scalar record: [0] = 1/R (0 where R = 0), [1] = R
#define CONS_PW_SCALARS 5    // per-block sums in front of the per-class ones: count, kl, ce, weighted ce, mse

struct cons_wc { double v[CTL_ROW_MAXC]; };    // normalised class weights of 'weighted ce' (ones otherwise), a launch argument
struct cons_wk { double v[CONS_NK]; };    // weight of each kind (0 where the kind is not selected)

// v <- softmax(v) = exp(v - max) * (1 / sum), fp32 (a reciprocal and a product, as ctl_loss.hip forms it; ctl_uncert.hip divides); returns log of the partition sum, max + log(sum) in fp64 (log softmax_k = x_k - it)
template <int CT> __device__ __forceinline__ double crow_softmax(float* v, int c) {
#pragma clang fp contract(off)
    constexpr int NC = CT ? CT : CTL_ROW_MAXC;
    float s;
    const float m = ctl_row_exp<CT>(v, c, s);
    const float r = 1.f / s;
#pragma unroll
    for (int k = 0; k < NC; ++k) if (k < c) v[k] = v[k] * r;
    return (double)m + log((double)s);
}

// ------------------------------------------------------------------------------------------------ point-wise and Dice kinds, forward
// grid (blocks of a sample, sample); partial[b][block][5 + 3c]: masked count, kl, sum p log q, sum w' p log q, sum (q-p)^2, then per class
// sum m q p, sum m q, sum m p.  Every entry is written (0 for a kind that is not selected).
template <int CT>
__global__ __launch_bounds__(EB) void cons_pw_partial_kernel(const float* __restrict__ xo, const float* __restrict__ xr,
                                                              const uint8_t* __restrict__ mask, int64_t hw, int c_rt, int kinds, int is_gt,
                                                              cons_wc wc, double p8, double p8logp8, double* __restrict__ partial) {
#pragma clang fp contract(off)
    constexpr int NC = CT ? CT : CTL_ROW_MAXC;
    constexpr int NV = CONS_PW_SCALARS + 3 * CTL_ROW_MAXC;
    __shared__ double sm[EB / 64][NV];
    const int c = CT ? CT : c_rt;
    const int64_t b = blockIdx.y;
    const float* __restrict__ x = xo + b * hw * c;
    const float* __restrict__ r = xr + b * hw * c;
    const uint8_t* __restrict__ mk = mask ? mask + b * hw : nullptr;
    const bool kl = kinds & CTL_CONS_KL, ce = kinds & (CTL_CONS_CE | CTL_CONS_WCE), mse = kinds & CTL_CONS_MSE, dice = kinds & CTL_CONS_DICE;
    double sc[CONS_PW_SCALARS], si[NC], sq[NC], sp[NC];
#pragma unroll
    for (int t = 0; t < CONS_PW_SCALARS; ++t) sc[t] = 0.0;
#pragma unroll
    for (int k = 0; k < NC; ++k) { si[k] = 0.0; sq[k] = 0.0; sp[k] = 0.0; }
    const int64_t stride = (int64_t)gridDim.x * EB;
    for (int64_t i = (int64_t)blockIdx.x * EB + threadIdx.x; i < hw; i += stride) {
        if (mk && mk[i] == 0) continue;
        float q[NC], p[NC], xv[NC], rv[NC];
        ctl_row_load<CT>(x, i, c, q);
        ctl_row_load<CT>(r, i, c, p);
#pragma unroll
        for (int k = 0; k < NC; ++k) if (k < c) { xv[k] = q[k]; rv[k] = p[k]; }
        const double lzx = crow_softmax<CT>(q, c);
        const double lzr = is_gt ? 0.0 : crow_softmax<CT>(p, c);
        sc[0] += 1.0;
#pragma unroll
        for (int k = 0; k < NC; ++k) if (k < c) {
            const double qd = (double)q[k], pd = (double)p[k], logq = (double)xv[k] - lzx;
            if (kl) {
                const double pk = is_gt ? (rv[k] != 0.f ? 1.0 : p8) : pd;
                const double plogp = is_gt ? (rv[k] != 0.f ? 0.0 : p8logp8) : pd * ((double)rv[k] - lzr);
                sc[1] += plogp - pk * logq;
            }
            if (ce) { const double t = pd * logq; sc[2] += t; sc[3] += wc.v[k] * t; }
            if (mse) { const double d = qd - pd; sc[4] += d * d; }
            if (dice) { si[k] += qd * pd; sq[k] += qd; sp[k] += pd; }
        }
    }
    const int wv = threadIdx.x >> 6;
    const bool first = (threadIdx.x & 63) == 0;
#pragma unroll
    for (int t = 0; t < CONS_PW_SCALARS; ++t) { const double a = wave_sum_double(sc[t]); if (first) sm[wv][t] = a; }
#pragma unroll
    for (int k = 0; k < NC; ++k) if (k < c) {
        const double a = wave_sum_double(si[k]), u = wave_sum_double(sq[k]), t = wave_sum_double(sp[k]);
        if (first) { sm[wv][CONS_PW_SCALARS + 3 * k] = a; sm[wv][CONS_PW_SCALARS + 3 * k + 1] = u; sm[wv][CONS_PW_SCALARS + 3 * k + 2] = t; }
    }
    const int nv = CONS_PW_SCALARS + 3 * c;
    CTL_BLOCK_ROWS_STORE(sm, EB / 64, nv, partial + (b * gridDim.x + blockIdx.x) * nv);
}

// ------------------------------------------------------------------------------------------------ contour, forward
// One block per tile of T x T pixels (grid-stride over the tiles of every sample).  LDS: d[c-1][T+2][T+2], zero outside the plane (the
// filters pad q and p with zeros, so d is zero there).  partial[block] = sum over its tiles of m (E_x^2 + E_y^2), summed over the classes 1..c-1.
#define SOBEL_X(D) ((D(0, 0) - D(0, 2)) + 2.0 * (D(1, 0) - D(1, 2)) + (D(2, 0) - D(2, 2)))
#define SOBEL_Y(D) ((D(0, 0) + 2.0 * D(0, 1) + D(0, 2)) - (D(2, 0) + 2.0 * D(2, 1) + D(2, 2)))
// d = softmax(x) - p of one pixel for the classes 1..c-1 into the planes of `dst` (plane stride `plane`) at offset `at`
template <int CT>
__device__ __forceinline__ void cons_store_d(const float* __restrict__ xo, const float* __restrict__ xr, int64_t pix, int c, int is_gt,
                                             float* __restrict__ dst, int plane, int at) {
#pragma clang fp contract(off)
    constexpr int NC = CT ? CT : CTL_ROW_MAXC;
    float q[NC], p[NC];
    ctl_row_load<CT>(xo, pix, c, q);
    ctl_row_load<CT>(xr, pix, c, p);
    crow_softmax<CT>(q, c);
    if (!is_gt) crow_softmax<CT>(p, c);
#pragma unroll
    for (int k = 1; k < NC; ++k) if (k < c) dst[(k - 1) * plane + at] = q[k] - p[k];
}
template <int CT, int T>
__global__ __launch_bounds__(EB) void cons_contour_fwd_kernel(const float* __restrict__ xo, const float* __restrict__ xr,
                                                               const uint8_t* __restrict__ mask, int b, int h, int w, int c_rt, int is_gt,
                                                               int tiles_y, int tiles_x, double* __restrict__ partial) {
#pragma clang fp contract(off)
    constexpr int HD = T + 2;
    extern __shared__ __attribute__((aligned(16))) float lds[];
    __shared__ double sm[EB / 64];
    const int c = CT ? CT : c_rt;
    const int nk = c - 1;
    const int64_t ntiles = (int64_t)b * tiles_y * tiles_x;
    double acc = 0.0;
    for (int64_t t = blockIdx.x; t < ntiles; t += gridDim.x) {
        const int tx = (int)(t % tiles_x), ty = (int)((t / tiles_x) % tiles_y);
        const int64_t s = t / ((int64_t)tiles_x * tiles_y);
        const int y0 = ty * T, x0 = tx * T;
        for (int i = threadIdx.x; i < HD * HD; i += EB) {
            const int yy = i / HD, xx = i % HD, gy = y0 + yy - 1, gx = x0 + xx - 1;
            if (gy >= 0 && gy < h && gx >= 0 && gx < w) cons_store_d<CT>(xo, xr, (s * h + gy) * w + gx, c, is_gt, lds, HD * HD, i);
            else for (int k = 0; k < nk; ++k) lds[k * HD * HD + i] = 0.f;
        }
        __syncthreads();
        for (int i = threadIdx.x; i < T * T; i += EB) {
            const int ly = i / T, lx = i % T, gy = y0 + ly, gx = x0 + lx;
            if (gy >= h || gx >= w) continue;
            if (mask && mask[(s * h + gy) * w + gx] == 0) continue;
            for (int k = 0; k < nk; ++k) {
                const float* __restrict__ dk = lds + k * HD * HD + ly * HD + lx;
#define D_(a, bb) (double)dk[(a) * HD + (bb)]
                const double ex = SOBEL_X(D_), ey = SOBEL_Y(D_);
#undef D_
                acc += ex * ex + ey * ey;
            }
        }
        __syncthreads();
    }
    acc = ctl_block_sum_double<EB / 64>(acc, sm);
    if (threadIdx.x == 0) partial[blockIdx.x] = acc;
}

// ------------------------------------------------------------------------------------------------ finalize, one block
// Sums the block rows in a fixed order, then thread 0 forms the terms (fp64, each rounded once), the weighted total, the scalar record
// and, through the first lane of each 16-lane group, the Dice coefficient table of the backward: g_k = dL/dq_k = m (coef[b][k][0] p_k + coef[b][k][1]).
__global__ __launch_bounds__(EB) void cons_finalize_kernel(const double* __restrict__ pw, int b, int nb, int c, const double* __restrict__ ct,
                                                            int ncb, int kinds, cons_wk wk, double pixels, double* __restrict__ coef,
                                                            double* __restrict__ scal, float* __restrict__ loss) {
#pragma clang fp contract(off)
    __shared__ double sm[EB / 64];
    const double smooth = 0.01;
    const int nv = CONS_PW_SCALARS + 3 * c;
    double tot[CONS_PW_SCALARS + 2];      // count, kl, ce, weighted ce, mse, sum of the Dice terms, contour
#pragma unroll
    for (int t = 0; t < CONS_PW_SCALARS; ++t) {
        double s = 0.0;
        if (pw) for (int j = threadIdx.x; j < b * nb; j += EB) s += pw[(int64_t)j * nv + t];
        tot[t] = ctl_block_sum_double<EB / 64>(s, sm);
        __syncthreads();
    }
    const int lane = threadIdx.x & 15, grp = threadIdx.x >> 4;
    const bool dice = pw && (kinds & CTL_CONS_DICE);
    const double div = (double)b * (double)c;
    double acc = 0.0;
    for (int base = 0; base < b * c; base += EB / 16) {
        const int it = base + grp;
        const bool ok = it < b * c;
        const int64_t sb = ok ? it / c : 0;
        const int k = ok ? it % c : 0;
        double si = 0.0, sq = 0.0, sp = 0.0;
        if (ok && dice) {
            for (int j = lane; j < nb; j += 16) {
                const double* __restrict__ e = pw + (sb * nb + j) * nv + CONS_PW_SCALARS + 3 * k;
                si += e[0]; sq += e[1]; sp += e[2];
            }
        }
        CTL_GROUP16_SUM3(si, sq, sp);
        if (ok && lane == 0) {
            const double I = si + smooth, U = sq + sp + smooth;
            coef[(int64_t)it * 2] = dice ? -(2.0 / U) / div : 0.0;
            coef[(int64_t)it * 2 + 1] = dice ? (2.0 * I / (U * U)) / div : 0.0;
            acc += dice ? 2.0 * I / U : 0.0;
        }
    }
    tot[CONS_PW_SCALARS] = ctl_block_sum_double<EB / 64>(acc, sm);
    __syncthreads();
    double s = 0.0;
    if (ct) for (int j = threadIdx.x; j < ncb; j += EB) s += ct[j];
    tot[CONS_PW_SCALARS + 1] = ctl_block_sum_double<EB / 64>(s, sm);
    if (threadIdx.x == 0) {
        const double R = tot[0];
        double term[CONS_NK];
        term[0] = tot[1] / pixels;
        term[1] = R > 0.0 ? -tot[2] / R : 0.0;
        term[2] = R > 0.0 ? -tot[3] / R : 0.0;
        term[3] = tot[4] / pixels;
        term[4] = 1.0 - tot[5] / div;
        term[5] = c > 1 ? 0.5 * tot[6] / ((double)(c - 1) * pixels) : 0.0;
        double total = 0.0;
#pragma unroll
        for (int t = 0; t < CONS_NK; ++t) {
            const bool on = (kinds >> t) & 1;
            total += on ? wk.v[t] * term[t] : 0.0;
            loss[1 + t] = on ? (float)term[t] : 0.f;
        }
        loss[0] = (float)total;
        scal[0] = R > 0.0 ? 1.0 / R : 0.0;
        scal[1] = R;
#pragma unroll
        for (int t = 2; t < CONS_SCAL; ++t) scal[t] = 0.0;
    }
}

// ------------------------------------------------------------------------------------------------ point-wise and Dice kinds, backward
// grid (blocks of a sample, sample).  With q, p recomputed and S the sum of the ROUNDED q_k (as the Dice backward of ctl_loss.hip has it):
//   dlogit_j = gout [ q_j (g_j S - sum_k q_k g_k) + a_kl (Sp q_j - pk_j) + a_ce (q_j sum_k p_k - p_j) + a_wce (q_j sum_k w'_k p_k - w'_j p_j) ]
//   g_k = a_mse (q_k - p_k) + w_dice (coef0 p_k + coef1),  a_kl = w_kl / M,  a_ce = w_ce / R,  a_wce = w_wce / R,  a_mse = 2 w_mse / M
// formed in fp64 and rounded once; a masked-out pixel gets zeros.
template <int CT>
__global__ __launch_bounds__(EB) void cons_pw_bwd_kernel(const float* __restrict__ xo, const float* __restrict__ xr,
                                                          const uint8_t* __restrict__ mask, const float* __restrict__ gout,
                                                          const double* __restrict__ coef, const double* __restrict__ scal, int64_t hw, int c_rt,
                                                          int kinds, int is_gt, cons_wc wc, cons_wk wk, double p8, double pixels,
                                                          float* __restrict__ dlogit) {
#pragma clang fp contract(off)
    constexpr int NC = CT ? CT : CTL_ROW_MAXC;
    const int c = CT ? CT : c_rt;
    const int64_t b = blockIdx.y;
    const float* __restrict__ x = xo + b * hw * c;
    const float* __restrict__ r = xr + b * hw * c;
    const uint8_t* __restrict__ mk = mask ? mask + b * hw : nullptr;
    float* __restrict__ dx = dlogit + b * hw * c;
    const double go = (double)gout[0], inv_r = scal[0];
    const bool kl = kinds & CTL_CONS_KL, ce = kinds & CTL_CONS_CE, wce = kinds & CTL_CONS_WCE, mse = kinds & CTL_CONS_MSE,
               dice = kinds & CTL_CONS_DICE;
    const double a_kl = kl ? wk.v[0] / pixels : 0.0, a_ce = ce ? wk.v[1] * inv_r : 0.0, a_wce = wce ? wk.v[2] * inv_r : 0.0,
                 a_mse = mse ? 2.0 * wk.v[3] / pixels : 0.0;
    double ca[NC], cb[NC];
#pragma unroll
    for (int k = 0; k < NC; ++k) {
        const bool on = dice && k < c;
        ca[k] = on ? wk.v[4] * coef[(b * c + k) * 2] : 0.0;
        cb[k] = on ? wk.v[4] * coef[(b * c + k) * 2 + 1] : 0.0;
    }
    const int64_t stride = (int64_t)gridDim.x * EB;
    for (int64_t i = (int64_t)blockIdx.x * EB + threadIdx.x; i < hw; i += stride) {
        float q[NC], p[NC];
        if (mk && mk[i] == 0) {
#pragma unroll
            for (int k = 0; k < NC; ++k) q[k] = 0.f;
            ctl_row_store<CT>(dx, i, c, q);
            continue;
        }
        float rv[NC];
        ctl_row_load<CT>(x, i, c, q);
        ctl_row_load<CT>(r, i, c, p);
#pragma unroll
        for (int k = 0; k < NC; ++k) if (k < c) rv[k] = p[k];
        crow_softmax<CT>(q, c);
        if (!is_gt) crow_softmax<CT>(p, c);
        double g[NC], S = 0.0, dot = 0.0, skl = 0.0, sp = 0.0, swp = 0.0;
#pragma unroll
        for (int k = 0; k < NC; ++k) if (k < c) {
            const double qd = (double)q[k], pd = (double)p[k];
            g[k] = a_mse * (qd - pd) + (ca[k] * pd + cb[k]);
            S += qd;
            dot += qd * g[k];
            skl += is_gt ? (rv[k] != 0.f ? 1.0 : p8) : pd;
            sp += pd;
            swp += wc.v[k] * pd;
        }
#pragma unroll
        for (int k = 0; k < NC; ++k) if (k < c) {
            const double qd = (double)q[k], pd = (double)p[k];
            const double pk = is_gt ? (rv[k] != 0.f ? 1.0 : p8) : pd;
            const double v = qd * (g[k] * S - dot) + a_kl * (skl * qd - pk) + a_ce * (qd * sp - pd) + a_wce * (qd * swp - wc.v[k] * pd);
            q[k] = (float)(go * v);
        }
        ctl_row_store<CT>(dx, i, c, q);
    }
}

// ------------------------------------------------------------------------------------------------ contour, backward
// LDS: d[c-1][T+4][T+4] (halo 2), then the masked responses m E_x and m E_y, each [c-1][T+2][T+2] (halo 1; zero outside the plane and where
// the mask is 0), rounded to fp32.  A centre pixel applies the transposed stencils: g_k = coef (S_x^T(m E_x) + S_y^T(m E_y))_k with
// coef = w_contour / ((c-1) M), g_0 = 0, and dlogit_j (+)= gout q_j (g_j S - sum_k q_k g_k) with q recomputed from x.
template <int CT, int T>
__global__ __launch_bounds__(EB) void cons_contour_bwd_kernel(const float* __restrict__ xo, const float* __restrict__ xr,
                                                               const uint8_t* __restrict__ mask, const float* __restrict__ gout, int b, int h,
                                                               int w, int c_rt, int is_gt, int tiles_y, int tiles_x, double coef, int accumulate,
                                                               float* __restrict__ dlogit) {
#pragma clang fp contract(off)
    constexpr int NC = CT ? CT : CTL_ROW_MAXC;
    constexpr int HD = T + 4, HE = T + 2;
    extern __shared__ __attribute__((aligned(16))) float lds[];
    const int c = CT ? CT : c_rt;
    const int nk = c - 1;
    float* __restrict__ ldd = lds;
    float* __restrict__ lex = lds + nk * HD * HD;
    float* __restrict__ ley = lex + nk * HE * HE;
    const double go = (double)gout[0];
    const int64_t ntiles = (int64_t)b * tiles_y * tiles_x;
    for (int64_t t = blockIdx.x; t < ntiles; t += gridDim.x) {
        const int tx = (int)(t % tiles_x), ty = (int)((t / tiles_x) % tiles_y);
        const int64_t s = t / ((int64_t)tiles_x * tiles_y);
        const int y0 = ty * T, x0 = tx * T;
        for (int i = threadIdx.x; i < HD * HD; i += EB) {
            const int yy = i / HD, xx = i % HD, gy = y0 + yy - 2, gx = x0 + xx - 2;
            if (gy >= 0 && gy < h && gx >= 0 && gx < w) cons_store_d<CT>(xo, xr, (s * h + gy) * w + gx, c, is_gt, ldd, HD * HD, i);
            else for (int k = 0; k < nk; ++k) ldd[k * HD * HD + i] = 0.f;
        }
        __syncthreads();
        for (int i = threadIdx.x; i < HE * HE; i += EB) {
            const int yy = i / HE, xx = i % HE, gy = y0 + yy - 1, gx = x0 + xx - 1;
            bool on = gy >= 0 && gy < h && gx >= 0 && gx < w;
            if (on && mask) on = mask[(s * h + gy) * w + gx] != 0;
            for (int k = 0; k < nk; ++k) {
                const float* __restrict__ dk = ldd + k * HD * HD + yy * HD + xx;
#define D_(a, bb) (double)dk[(a) * HD + (bb)]
                lex[k * HE * HE + i] = on ? (float)SOBEL_X(D_) : 0.f;
                ley[k * HE * HE + i] = on ? (float)SOBEL_Y(D_) : 0.f;
#undef D_
            }
        }
        __syncthreads();
        for (int i = threadIdx.x; i < T * T; i += EB) {
            const int ly = i / T, lx = i % T, gy = y0 + ly, gx = x0 + lx;
            if (gy >= h || gx >= w) continue;
            const int64_t pix = (s * h + gy) * w + gx;
            float q[NC];
            ctl_row_load<CT>(xo, pix, c, q);
            crow_softmax<CT>(q, c);
            double g[NC], S = (double)q[0], dot = 0.0;
            g[0] = 0.0;
#pragma unroll
            for (int k = 1; k < NC; ++k) if (k < c) {
                const float* __restrict__ fx = lex + (k - 1) * HE * HE + ly * HE + lx;
                const float* __restrict__ fy = ley + (k - 1) * HE * HE + ly * HE + lx;
#define X_(a, bb) (double)fx[(a) * HE + (bb)]
#define Y_(a, bb) (double)fy[(a) * HE + (bb)]
                const double tx_ = (X_(2, 2) - X_(2, 0)) + 2.0 * (X_(1, 2) - X_(1, 0)) + (X_(0, 2) - X_(0, 0));
                const double ty_ = (Y_(2, 2) + 2.0 * Y_(2, 1) + Y_(2, 0)) - (Y_(0, 2) + 2.0 * Y_(0, 1) + Y_(0, 0));
#undef X_
#undef Y_
                g[k] = coef * (tx_ + ty_);
                S += (double)q[k];
                dot += (double)q[k] * g[k];
            }
            float o[NC];
            if (accumulate) ctl_row_load<CT>(dlogit, pix, c, o);
#pragma unroll
            for (int k = 0; k < NC; ++k) if (k < c) {
                const float v = (float)(go * ((double)q[k] * (g[k] * S - dot)));
                o[k] = accumulate ? o[k] + v : v;
            }
            ctl_row_store<CT>(dlogit, pix, c, o);
        }
        __syncthreads();
    }
}

// ------------------------------------------------------------------------------------------------ average pooling
// y[b][ho][wo][c] = mean of the 2^s x 2^s window: rows in order, columns in order, fp64, one rounding.  One thread per output element.
__global__ __launch_bounds__(EB) void cons_avgpool_fwd_kernel(const float* __restrict__ x, int h, int w, int c, int s, int ho, int wo,
                                                               int64_t total, float* __restrict__ y) {
    const int k = 1 << s;
    const double inv = 1.0 / (double)(k * k);
    const int64_t stride = (int64_t)gridDim.x * EB;
    for (int64_t i = (int64_t)blockIdx.x * EB + threadIdx.x; i < total; i += stride) {
        const int ch = (int)(i % c);
        const int64_t pix = i / c;
        const int ox = (int)(pix % wo), oy = (int)((pix / wo) % ho);
        const int64_t n = pix / ((int64_t)wo * ho);
        double a = 0.0;
        for (int dy = 0; dy < k; ++dy) {
            const float* __restrict__ row = x + (((n * h + ((int64_t)oy * k + dy)) * w + (int64_t)ox * k) * c + ch);
            for (int dx = 0; dx < k; ++dx) a += (double)row[(int64_t)dx * c];
        }
        y[i] = (float)(a * inv);
    }
}
// gx[b][h][w][c] = gy[b][y >> s][x >> s][c] * 4^-s, zero on the rows and columns the floor drops.  One thread per input element.
__global__ __launch_bounds__(EB) void cons_avgpool_bwd_kernel(const float* __restrict__ gy, int h, int w, int c, int s, int ho, int wo,
                                                               int64_t total, float* __restrict__ gx) {
    const float inv = 1.f / (float)(1 << (2 * s));
    const int64_t stride = (int64_t)gridDim.x * EB;
    for (int64_t i = (int64_t)blockIdx.x * EB + threadIdx.x; i < total; i += stride) {
        const int ch = (int)(i % c);
        const int64_t pix = i / c;
        const int px = (int)(pix % w), py = (int)((pix / w) % h);
        const int64_t n = pix / ((int64_t)w * h);
        const int oy = py >> s, ox = px >> s;
        gx[i] = (oy < ho && ox < wo) ? gy[((n * ho + oy) * wo + ox) * c + ch] * inv : 0.f;
    }
}

// ------------------------------------------------------------------------------------------------ launchers
static inline int cons_tile(int c) { return c <= 4 ? 32 : 16; }
static int cons_check(const char* who, int kinds, int64_t b, int64_t h, int64_t w, int c) {
    CTL_REQUIRE(kinds > 0 && (kinds & ~CONS_ALL) == 0, "%s: kinds 0x%x (a non-empty set of the bits 0x01 .. 0x20)", who, kinds);
    CTL_REQUIRE(b > 0 && h > 0 && w > 0, "%s: sizes must be positive (batch %lld, plane %lld x %lld)", who, (long long)b, (long long)h, (long long)w);
    if (int rc = ctl_check_channels(who, c, "classes")) return rc;
    CTL_REQUIRE(!(kinds & CTL_CONS_CONTOUR) || c >= 2, "%s: contour needs at least 2 classes (got %d): it runs over the classes 1 .. c-1", who, c);
    if (int rc = ctl_check_batch(who, b)) return rc;
    return ctl_check_2gib(who, b, h, w, c, "classes");
}
static int cons_weights(const char* who, int kinds, int c, const double* weights, const double* class_weights, cons_wk* wk, cons_wc* wc) {
    if (int rc = ctl_kind_weights(who, kinds, CONS_NK, weights, wk->v)) return rc;
    for (int k = 0; k < CTL_ROW_MAXC; ++k) wc->v[k] = k < c ? 1.0 : 0.0;
    if (kinds & CTL_CONS_WCE) {
        CTL_REQUIRE(class_weights, "%s: null pointer (weighted ce needs the class weights)", who);
        if (int rc = ctl_class_weights_norm(who, c, class_weights, wc->v)) return rc;
    }
    return CTL_OK;
}
// upstream's is_gt rule of 'kl': torch.where(reference == 0, 1e-8, 1 - 1e-8) is a float32 tensor, and so is its p log p
static inline double cons_p8() { return (double)1e-8f; }
static inline double cons_p8logp8() { return (double)(1e-8f * logf(1e-8f)); }

struct cons_layout { size_t coef, scal, pw, ct, total; int nb, ncb; };
static cons_layout cons_ws(int kinds, int64_t b, int h, int w, int c) {
    cons_layout l;
    l.nb = ctl_sample_blocks(b, (int64_t)h * w, EB, CTL_RED_BLOCKS);
    l.ncb = ctl_tile_blocks(b, h, w, cons_tile(c), CONS_MAX_TILE_BLOCKS);
    l.coef = 0;
    l.scal = (size_t)b * c * 2;
    l.pw = l.scal + CONS_SCAL;
    l.ct = l.pw + ((kinds & CONS_PW) ? (size_t)b * l.nb * (CONS_PW_SCALARS + 3 * c) : 0);
    l.total = l.ct + ((kinds & CTL_CONS_CONTOUR) ? (size_t)l.ncb : 0);
    return l;
}

extern "C" size_t ctl_consistency_ws_doubles(int32_t kinds, int32_t b, int32_t h, int32_t w, int32_t c) {
    if (cons_check("consistency_ws_doubles", kinds, b, h, w, c) != CTL_OK) return 0;
    return cons_ws(kinds, b, h, w, c).total;
}
static size_t cons_contour_lds(int c, int bwd) {
    const int t = cons_tile(c), nk = c - 1;
    return sizeof(float) * (size_t)nk * (bwd ? (t + 4) * (t + 4) + 2 * (t + 2) * (t + 2) : (t + 2) * (t + 2));
}
extern "C" int ctl_consistency_fwd(int32_t kinds, const double* weights, const double* class_weights, const float* x, const float* r,
                                   const uint8_t* mask, int32_t is_gt, int32_t b, int32_t h, int32_t w, int32_t c, double* ws, float* loss,
                                   ctl_stream stream) {
    CTL_REQUIRE(x && r && ws && loss, "consistency_fwd: null pointer");
    if (int rc = cons_check("consistency_fwd", kinds, b, h, w, c)) return rc;
    cons_wk wk;
    cons_wc wc;
    if (int rc = cons_weights("consistency_fwd", kinds, c, weights, class_weights, &wk, &wc)) return rc;
    const cons_layout l = cons_ws(kinds, b, h, w, c);
    const int64_t hw = (int64_t)h * w;
    const bool v4 = ctl_vec4(c, x, r);
    int extra = 0;
    if (kinds & CONS_PW) {
        const dim3 grid(l.nb, b);
        CTL_ROW_DISPATCH(cons_pw_partial_kernel, v4, grid, x, r, mask, hw, c, kinds, is_gt != 0, wc, cons_p8(), cons_p8logp8(), ws + l.pw);
        ++extra;
    }
    if (kinds & CTL_CONS_CONTOUR) {
        const int t = cons_tile(c), ty = ctl_cdiv(h, t), tx = ctl_cdiv(w, t);
        const size_t lds = cons_contour_lds(c, 0);
        if (v4) cons_contour_fwd_kernel<4, 32><<<dim3(l.ncb), dim3(EB), lds, S_>>>(x, r, mask, b, h, w, c, is_gt != 0, ty, tx, ws + l.ct);
        else if (t == 32) cons_contour_fwd_kernel<0, 32><<<dim3(l.ncb), dim3(EB), lds, S_>>>(x, r, mask, b, h, w, c, is_gt != 0, ty, tx, ws + l.ct);
        else cons_contour_fwd_kernel<0, 16><<<dim3(l.ncb), dim3(EB), lds, S_>>>(x, r, mask, b, h, w, c, is_gt != 0, ty, tx, ws + l.ct);
        ++extra;
    }
    cons_finalize_kernel<<<dim3(1), dim3(EB), 0, S_>>>((kinds & CONS_PW) ? ws + l.pw : nullptr, b, l.nb, c,
                                                       (kinds & CTL_CONS_CONTOUR) ? ws + l.ct : nullptr, l.ncb, kinds, wk, (double)b * (double)hw,
                                                       ws + l.coef, ws + l.scal, loss);
    ctl_count_launches(extra);
    CTL_LAUNCH_CHECK("consistency_fwd");
    return CTL_OK;
}
extern "C" int ctl_consistency_bwd(int32_t kinds, const double* weights, const double* class_weights, const float* x, const float* r,
                                   const uint8_t* mask, int32_t is_gt, const float* gout, const double* ws, int32_t b, int32_t h, int32_t w,
                                   int32_t c, float* dlogit, ctl_stream stream) {
    CTL_REQUIRE(x && r && gout && ws && dlogit, "consistency_bwd: null pointer");
    if (int rc = cons_check("consistency_bwd", kinds, b, h, w, c)) return rc;
    cons_wk wk;
    cons_wc wc;
    if (int rc = cons_weights("consistency_bwd", kinds, c, weights, class_weights, &wk, &wc)) return rc;
    const cons_layout l = cons_ws(kinds, b, h, w, c);
    const int64_t hw = (int64_t)h * w;
    const double pixels = (double)b * (double)hw;
    const bool v4 = ctl_vec4(c, x, r, dlogit);
    int extra = -1;
    if (kinds & CONS_PW) {
        const dim3 grid(ctl_sample_blocks(b, hw, EB, CONS_MAX_STREAM_BLOCKS), b);
        CTL_ROW_DISPATCH(cons_pw_bwd_kernel, v4, grid, x, r, mask, gout, ws + l.coef, ws + l.scal, hw, c, kinds, is_gt != 0, wc, wk, cons_p8(), pixels, dlogit);
        ++extra;
    }
    if (kinds & CTL_CONS_CONTOUR) {
        const int t = cons_tile(c), ty = ctl_cdiv(h, t), tx = ctl_cdiv(w, t);
        const size_t lds = cons_contour_lds(c, 1);
        const double coef = wk.v[5] / ((double)(c - 1) * pixels);
        const int acc = (kinds & CONS_PW) ? 1 : 0;
        if (v4) cons_contour_bwd_kernel<4, 32><<<dim3(l.ncb), dim3(EB), lds, S_>>>(x, r, mask, gout, b, h, w, c, is_gt != 0, ty, tx, coef, acc, dlogit);
        else if (t == 32) cons_contour_bwd_kernel<0, 32><<<dim3(l.ncb), dim3(EB), lds, S_>>>(x, r, mask, gout, b, h, w, c, is_gt != 0, ty, tx, coef, acc, dlogit);
        else cons_contour_bwd_kernel<0, 16><<<dim3(l.ncb), dim3(EB), lds, S_>>>(x, r, mask, gout, b, h, w, c, is_gt != 0, ty, tx, coef, acc, dlogit);
        ++extra;
    }
    ctl_count_launches(extra);
    CTL_LAUNCH_CHECK("consistency_bwd");
    return CTL_OK;
}

static int cons_pool_check(const char* who, int64_t b, int64_t h, int64_t w, int c, int s) {
    CTL_REQUIRE(b > 0 && h > 0 && w > 0, "%s: sizes must be positive (batch %lld, plane %lld x %lld)", who, (long long)b, (long long)h, (long long)w);
    if (int rc = ctl_check_channels(who, c, "channels")) return rc;
    CTL_REQUIRE(s >= 1 && s <= 4, "%s: scale %d (1 .. 4: windows of 2 .. 16 pixels)", who, s);
    CTL_REQUIRE((h >> s) >= 1 && (w >> s) >= 1, "%s: a %lld x %lld plane is smaller than the window of scale %d", who, (long long)h, (long long)w, s);
    return ctl_check_2gib(who, b, h, w, c, "channels");
}
extern "C" int ctl_avgpool_fwd(const float* x, int32_t b, int32_t h, int32_t w, int32_t c, int32_t scale, float* y, ctl_stream stream) {
    CTL_REQUIRE(x && y, "avgpool_fwd: null pointer");
    if (int rc = cons_pool_check("avgpool_fwd", b, h, w, c, scale)) return rc;
    const int ho = h >> scale, wo = w >> scale;
    const int64_t total = (int64_t)b * ho * wo * c;
    cons_avgpool_fwd_kernel<<<dim3(ctl_blocks(total, EB, CONS_MAX_STREAM_BLOCKS)), dim3(EB), 0, S_>>>(x, h, w, c, scale, ho, wo, total, y);
    CTL_LAUNCH_CHECK("avgpool_fwd");
    return CTL_OK;
}
extern "C" int ctl_avgpool_bwd(const float* gy, int32_t b, int32_t h, int32_t w, int32_t c, int32_t scale, float* gx, ctl_stream stream) {
    CTL_REQUIRE(gy && gx, "avgpool_bwd: null pointer");
    if (int rc = cons_pool_check("avgpool_bwd", b, h, w, c, scale)) return rc;
    const int ho = h >> scale, wo = w >> scale;
    const int64_t total = (int64_t)b * h * w * c;
    cons_avgpool_bwd_kernel<<<dim3(ctl_blocks(total, EB, CONS_MAX_STREAM_BLOCKS)), dim3(EB), 0, S_>>>(gy, h, w, c, scale, ho, wo, total, gx);
    CTL_LAUNCH_CHECK("avgpool_bwd");
    return CTL_OK;
}
