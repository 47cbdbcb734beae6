// Predictive uncertainty and calibration tables of fp32 NHWC logits the device already holds (include/ctl_hip.h, "predictive
// uncertainty"): entropy / mutual-information / confidence / arg-max / mean-probability maps of a T-member ensemble, and per slice the
// sums behind ECE, NLL, Brier and the mean entropy.  Upstream's entropy maps are medseg/common_utils/uncertainty.py:7-54, its Brier sum
// medseg/models/custom_loss.py:495-511.  One streaming pass: every pixel is read once, its channel rows live in registers.
// Sums are two-stage and ordered (per-block fp64 partials and integer bin rows, one finalize block per slice): no float atomics, no
// global atomics at all, the same bits on every call.  Nothing is read back; no launch argument changes from call to call.
//
// A label outside 0..c-1 is no class: the pixel gets its maps and enters none of the labelled sums.  Labels are only ever compared with
// a class index.
#include "ctl_rows.h"

#define UB CTL_ROW_THREADS          // threads per block
#define UNCERT_MAX_BLOCKS 2048    // blocks over all slices of the streaming pass: the number of partial rows, part of the result's bits

// v <- softmax(v) with a true division (uniform logits give exactly float(1) / float(c)); returns log of the sum of exp(v - max),
// `m` = the row maximum: log p_k = v_k - m - (the return value) without going through p_k, which underflows for a far-off class
template <int CT> __device__ __forceinline__ float urow_softmax(float* v, int c, float& m) {
#pragma clang fp contract(off)
    constexpr int NC = CT ? CT : CTL_ROW_MAXC;
    float s;
    m = ctl_row_exp<CT>(v, c, s);
#pragma unroll
    for (int k = 0; k < NC; ++k) if (k < c) v[k] = v[k] / s;
    return logf(s);
}
// -sum_k p_k log2(p_k + eps) in bits; a term whose p_k + eps is 0 contributes 0
template <int CT> __device__ __forceinline__ float urow_entropy(const float* p, int c, float eps) {
#pragma clang fp contract(off)
    constexpr int NC = CT ? CT : CTL_ROW_MAXC;
    float h = 0.f;
#pragma unroll
    for (int k = 0; k < NC; ++k) if (k < c) {
        const float q = p[k] + eps;
        h += q > 0.f ? p[k] * log2f(q) : 0.f;
    }
    return -h;
}

struct uncert_maps { float* entropy; float* mi; float* conf; uint8_t* pred; float* mean_prob; };

// pass 1: grid (blocks of a slice, slice).  pstats[slice][block][6] = labelled, correct, sum H, sum MI, sum nll, sum brier over the block's
// pixels; pbins[slice][block][bin][3] = count, correct, sum of conf * 2^32 (an exact integer: see ctl_hip.h) of its labelled pixels.
template <int CT>
__global__ __launch_bounds__(UB) void uncert_partial_kernel(const float* __restrict__ logit, const int64_t* __restrict__ label, int T, int n,
                                                             int64_t hw, int c_rt, int B, float eps, int is_prob, uncert_maps o,
                                                             double* __restrict__ pstats, unsigned long long* __restrict__ pbins) {
#pragma clang fp contract(off)
    constexpr int NC = CT ? CT : CTL_ROW_MAXC;
    __shared__ float edge[CTL_UNCERT_MAX_BINS];
    __shared__ unsigned long long bcc[CTL_UNCERT_MAX_BINS], bsum[CTL_UNCERT_MAX_BINS];      // bcc: count | correct << 32, one atomic for both
    __shared__ double sm[UB / 64][6];
    const int c = CT ? CT : c_rt;
    const int64_t b = blockIdx.y;
    const int tid = threadIdx.x;
    if (tid < CTL_UNCERT_MAX_BINS) {      // edge j = float(j) / float(B): the one rounding every comparison below sees
        edge[tid] = (float)tid / (float)B;
        bcc[tid] = 0ull; bsum[tid] = 0ull;
    }
    __syncthreads();
    const int64_t* __restrict__ y = label ? label + b * hw : nullptr;
    const float Tf = (float)T, Bf = (float)B;
    const float log_t = logf(Tf);
    double aH = 0.0, aMI = 0.0, aN = 0.0, aB = 0.0;
    unsigned int n_lab = 0u, n_cor = 0u;
    const int64_t stride = (int64_t)gridDim.x * UB;
    for (int64_t i = (int64_t)blockIdx.x * UB + tid; i < hw; i += stride) {
        const int64_t l = y ? y[i] : (int64_t)-1;
        float pb[NC];
#pragma unroll
        for (int k = 0; k < NC; ++k) pb[k] = 0.f;
        float E = 0.f;
        float M = -INFINITY, S = 0.f;      // running log-sum-exp of the members' log p_y
        for (int t = 0; t < T; ++t) {
            float v[NC];
            ctl_row_load<CT>(logit + ((int64_t)t * n + b) * hw * c, i, c, v);
            float vl = 0.f;                // the label's entry of the row as it was read
#pragma unroll
            for (int k = 0; k < NC; ++k) if (k < c) vl = (l == (int64_t)k) ? v[k] : vl;
            float lp;
            if (is_prob) {
                lp = logf(vl);
            } else {
                float m;
                const float ls = urow_softmax<CT>(v, c, m);
                lp = vl - m - ls;
            }
            if (lp > M) { S = S * expf(M - lp) + 1.f; M = lp; }
            else if (lp > -INFINITY) S += expf(lp - M);
            if (T > 1) E += urow_entropy<CT>(v, c, eps);
#pragma unroll
            for (int k = 0; k < NC; ++k) if (k < c) pb[k] += v[k];
        }
        float conf = -INFINITY;
        int yh = 0;
        float brier = 0.f;
        bool valid = false;
#pragma unroll
        for (int k = 0; k < NC; ++k) if (k < c) {
            pb[k] = pb[k] / Tf;
            if (pb[k] > conf) { conf = pb[k]; yh = k; }      // strict: a tie keeps the lowest index (ctl_argmax_c)
            const bool hit = l == (int64_t)k;
            const float d = pb[k] - (hit ? 1.f : 0.f);
            brier += d * d;
            valid = valid || hit;
        }
        const float H = urow_entropy<CT>(pb, c, eps);
        const float MI = T > 1 ? H - E / Tf : 0.f;
        const int64_t at = b * hw + i;
        if (o.entropy) o.entropy[at] = H;
        if (o.mi) o.mi[at] = MI;
        if (o.conf) o.conf[at] = conf;
        if (o.pred) o.pred[at] = (uint8_t)yh;
        if (o.mean_prob) ctl_row_store<CT>(o.mean_prob + b * hw * c, i, c, pb);
        aH += (double)H;
        aMI += (double)MI;
        if (valid) {
            const bool cor = l == (int64_t)yh;
            n_lab += 1u;
            n_cor += cor ? 1u : 0u;
            aN += (double)(-(M + logf(S) - log_t));
            aB += (double)brier;
            // the bin = the number of edges 1..B-1 below conf: a guess from the product, moved until it satisfies the comparisons themselves
            int g = (int)fminf(fmaxf(conf * Bf, 0.f), Bf - 1.f);
            while (g > 0 && !(conf > edge[g])) --g;
            while (g < B - 1 && conf > edge[g + 1]) ++g;
            atomicAdd(&bcc[g], cor ? (1ull << 32) + 1ull : 1ull);      // (a block sees fewer than 2^31 pixels: neither half overflows)
            atomicAdd(&bsum[g], conf > 0.f ? (unsigned long long)(conf * 4294967296.f) : 0ull);
        }
    }
    const double vals[6] = {(double)n_lab, (double)n_cor, aH, aMI, aN, aB};
    const int wv = tid >> 6;
#pragma unroll
    for (int q = 0; q < 6; ++q) {
        const double r = wave_sum_double(vals[q]);
        if ((tid & 63) == 0) sm[wv][q] = r;
    }
    __syncthreads();      // also: every LDS bin update of the block has landed
    const int64_t row = b * gridDim.x + blockIdx.x;
    if (tid < 6) {
        double r = 0.0;
        for (int i = 0; i < UB / 64; ++i) r += sm[i][tid];
        pstats[row * 6 + tid] = r;
    }
    if (tid < B) {
        unsigned long long* __restrict__ q = pbins + (row * B + tid) * 3;
        q[0] = bcc[tid] & 0xffffffffull; q[1] = bcc[tid] >> 32; q[2] = bsum[tid];
    }
}

// pass 2: one block per slice.  A group of 16 lanes adds the slice's `nb` block rows of one column: lane l takes the rows l, l + 16, ..
// in order, then an xor tree over the group -- a fixed order for the fp64 columns (the bin columns are integers: any order, same sum).
__global__ __launch_bounds__(UB) void uncert_finalize_kernel(const double* __restrict__ pstats, const unsigned long long* __restrict__ pbins,
                                                              int nb, int B, double* __restrict__ stats, int64_t* __restrict__ bins) {
    const int64_t b = blockIdx.x;
    const int tid = threadIdx.x;
    const int lane = tid & 15, grp = tid >> 4;
    if (bins) {
        const int ncol = B * 3;
        for (int base = 0; base < ncol; base += UB / 16) {      // (every thread takes every turn: the shuffles need whole groups)
            const int col = base + grp;
            unsigned long long s = 0ull;
            if (col < ncol) for (int j = lane; j < nb; j += 16) s += pbins[(b * nb + j) * ncol + col];
            CTL_GROUP16_SUM(s);
            if (col < ncol && lane == 0) bins[b * ncol + col] = (int64_t)s;
        }
    }
    double s = 0.0;
    if (grp < 6) for (int j = lane; j < nb; j += 16) s += pstats[(b * nb + j) * 6 + grp];
    CTL_GROUP16_SUM(s);
    if (stats && grp < 6 && lane == 0) stats[b * 6 + grp] = s;
}

// ------------------------------------------------------------------------------------------------ launchers
static int uncert_check(const char* who, int T, int64_t n, int64_t hw, int c, int B) {
    CTL_REQUIRE(T >= 1 && T <= CTL_UNCERT_MAX_MEMBERS, "%s: %d members (1 .. %d)", who, T, CTL_UNCERT_MAX_MEMBERS);
    CTL_REQUIRE(n > 0 && hw > 0, "%s: sizes must be positive (slices %lld, pixels per slice %lld)", who, (long long)n, (long long)hw);
    if (int rc = ctl_check_channels(who, c, "classes")) return rc;
    CTL_REQUIRE(B >= 1 && B <= CTL_UNCERT_MAX_BINS, "%s: %d reliability bins (1 .. %d)", who, B, CTL_UNCERT_MAX_BINS);
    CTL_REQUIRE(n <= 65535, "%s: %lld slices (at most 65535)", who, (long long)n);
    const int64_t row_bytes = c * 4 > 8 ? c * 4 : 8;      // logits: c floats per pixel and member, labels: 8 bytes per pixel
    CTL_REQUIRE(hw < ((int64_t)1 << 31) && (int64_t)T * n * hw < ((int64_t)1 << 31) / row_bytes,
                "%s: %d x %lld x %lld pixels of %d classes reach the 2 GiB tensor limit", who, T, (long long)n, (long long)hw, c);
    return CTL_OK;
}

extern "C" size_t ctl_predictive_stats_ws_bytes(int32_t T, int32_t n, int64_t hw, int32_t C, int32_t B) {
    if (uncert_check("predictive_stats_ws_bytes", T, n, hw, C, B) != CTL_OK) return 0;
    const size_t rows = (size_t)n * ctl_sample_blocks(n, hw, UB, UNCERT_MAX_BLOCKS);
    return ctl_align256(rows * 6 * sizeof(double)) + rows * B * 3 * sizeof(unsigned long long);
}
extern "C" int ctl_predictive_stats(const float* logits, const int64_t* label, int32_t T, int32_t n, int64_t hw, int32_t C, int32_t B, float eps,
                                    int32_t is_prob, float* entropy, float* mi, float* conf, uint8_t* pred, float* mean_prob, double* stats,
                                    int64_t* bins, void* workspace, ctl_stream stream) {
    CTL_REQUIRE(logits, "predictive_stats: null pointer (logits)");
    if (int rc = uncert_check("predictive_stats", T, n, hw, C, B)) return rc;
    CTL_REQUIRE(std::isfinite(eps) && eps >= 0.f, "predictive_stats: eps %g (finite, >= 0)", (double)eps);
    CTL_REQUIRE(workspace && ((uintptr_t)workspace & 7) == 0, "predictive_stats: null or misaligned workspace (8-byte alignment)");
    const int nb = ctl_sample_blocks(n, hw, UB, UNCERT_MAX_BLOCKS);
    const size_t rows = (size_t)n * nb;
    double* pstats = (double*)workspace;
    unsigned long long* pbins = (unsigned long long*)((char*)workspace + ctl_align256(rows * 6 * sizeof(double)));
    const uncert_maps o{entropy, mi, conf, pred, mean_prob};
    const dim3 grid(nb, n);
    CTL_ROW_DISPATCH(uncert_partial_kernel, ctl_vec4(C, logits, mean_prob), grid, logits, label, T, n, hw, C, B, eps, is_prob != 0, o, pstats, pbins);
    if (stats || bins) {
        uncert_finalize_kernel<<<dim3(n), dim3(UB), 0, S_>>>(pstats, pbins, nb, B, stats, bins);
        ctl_count_launches(1);      // partial + finalize
    }
    CTL_LAUNCH_CHECK("predictive_stats");
    return CTL_OK;
}
