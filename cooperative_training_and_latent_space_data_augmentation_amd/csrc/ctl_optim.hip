// The optimizer tail (include/ctl_hip.h, "optimizer tail"): a per-solver control record the host refreshes with ONE launch, the global
// gradient norm of up to 8 flat gradient buffers in two launches, and an Adam pass that reads its learning rate, the clip factor and the
// skip decision from that record and carries the EMA shadow of the weights along.  Upstream: ExponentialMovingAverage
// (medseg/models/model_util.py:21-101), get_scheduler (621-671), torch.nn.utils.clip_grad_norm_.
// Nothing here changes from step to step as a launch argument except what ctl_optim_control carries, so the norm and the tails can sit
// in a captured graph and the record is refreshed eagerly in front of each replay.  Sums are two-stage and ordered (fp64 partials over
// fixed chunks, one finalize wave): no atomics, no readback, the same bits on every call.
#include <cmath>
#include "ctl_device.h"

#define OB 256                    // threads per block
#define OPT_MAX_STREAM_BLOCKS 2048     // the grid cap of ctl_adam (ctl_elem.hip): the tail walks a buffer exactly as adam_kernel does
#define CH CTL_GRAD_NORM_CHUNK    // elements per pass-1 block: fixes the grouping of the sum, and with it its bits
static_assert(CH % (4 * OB) == 0, "a chunk is a whole number of quads per thread");

struct optim_lr8 { float v[CTL_OPTIM_MAX_NETS]; };
struct optim_bufs { const float* g[CTL_OPTIM_MAX_NETS]; int64_t count[CTL_OPTIM_MAX_NETS]; int64_t woff[CTL_OPTIM_MAX_NETS]; };

// ------------------------------------------------------------------------------------------------ control record
__global__ __launch_bounds__(64) void optim_control_kernel(double* __restrict__ ctrl, int k, optim_lr8 lr, float max_norm, int guard, float ema_omd) {
    const int t = threadIdx.x;
    if (t < CTL_OPTIM_MAX_NETS) ctrl[CTL_OPTIM_LR + t] = t < k ? (double)lr.v[t] : 0.0;
    if (t == 8) ctrl[CTL_OPTIM_MAX_NORM] = (double)max_norm;
    if (t == 9) ctrl[CTL_OPTIM_GUARD] = guard ? 1.0 : 0.0;
    if (t == 10) ctrl[CTL_OPTIM_EMA_OMD] = (double)ema_omd;
    if (t == 11) ctrl[CTL_OPTIM_CLIP] = 1.0;
    if (t == 12) ctrl[CTL_OPTIM_FINITE] = 1.0;
}

// ------------------------------------------------------------------------------------------------ gradient norm
// pass 1: grid (chunks of the longest buffer, k).  Block b of buffer j owns elements [b CH, (b + 1) CH): thread t adds the squares of
// quads t, t + 256, ... of the chunk in that order, elements of a quad in order, in fp64 (the square of an fp32 value is exact there);
// the block sum is ctl_block_sum_double.  A 16-byte aligned buffer is read 16 bytes per lane, any other one element at a time: the same
// elements in the same order, so alignment changes no bit.
__global__ __launch_bounds__(OB) void grad_norm_partial_kernel(optim_bufs a, double* __restrict__ work) {
    __shared__ double sm[OB / 64];
    const int j = blockIdx.y;
    const int64_t count = a.count[j];
    const int64_t lo = (int64_t)blockIdx.x * CH;
    if (lo >= count) return;                                   // (whole block: no barrier is skipped by part of one)
    const float* __restrict__ g = a.g[j];
    const int64_t hi = lo + CH < count ? lo + CH : count;
    const bool vec = ((uintptr_t)g & 15) == 0;
    double s = 0.0;
    for (int64_t q = lo + 4 * (int64_t)threadIdx.x; q < hi; q += 4 * OB) {
        if (vec && q + 4 <= hi) {
            const f32x4 t = *reinterpret_cast<const f32x4*>(g + q);
            s += (double)t.x * (double)t.x;
            s += (double)t.y * (double)t.y;
            s += (double)t.z * (double)t.z;
            s += (double)t.w * (double)t.w;
        } else {
            for (int64_t i = q; i < q + 4 && i < hi; ++i) s += (double)g[i] * (double)g[i];
        }
    }
    s = ctl_block_sum_double<OB / 64>(s, sm);
    if (threadIdx.x == 0) work[a.woff[j] + blockIdx.x] = s;
}

// pass 2: one wave.  Lane l adds partials l, l + 64, ... of the flat [buffer][chunk] list in index order; the 64 lane sums meet in the
// xor butterfly.  Lane 0 writes the five device fields.
__global__ __launch_bounds__(64) void grad_norm_final_kernel(const double* __restrict__ work, int64_t n_partials, float grad_scale,
                                                              double* __restrict__ ctrl) {
    double s = 0.0;
    for (int64_t i = threadIdx.x; i < n_partials; i += 64) s += work[i];
    s = wave_sum_double(s);
    if (threadIdx.x == 0) {
        const double norm = (double)grad_scale * sqrt(s);
        const bool finite = isfinite(norm);
        const double max_norm = ctrl[CTL_OPTIM_MAX_NORM];
        double clip = 1.0;
        if (max_norm > 0.0 && finite) clip = fmin(1.0, max_norm / (norm + 1e-6));
        ctrl[CTL_OPTIM_SUMSQ] = s;
        ctrl[CTL_OPTIM_NORM] = norm;
        ctrl[CTL_OPTIM_CLIP] = clip;
        ctrl[CTL_OPTIM_FINITE] = finite ? 1.0 : 0.0;
        if (ctrl[CTL_OPTIM_GUARD] != 0.0 && !finite) ctrl[CTL_OPTIM_SKIPPED] += 1.0;
    }
}

// ------------------------------------------------------------------------------------------------ Adam tail
// adam_kernel (ctl_elem.hip) statement for statement, with lr, the clip factor and the skip decision read from the record.  clip == 1
// changes no bit of gi, so with neutral settings this is ctl_adam / ctl_adam_dev (tests/test_optim_gpu.py holds the two together).
// s <- s - omd (s - p_new) as three separately rounded fp32 operations (contraction off: no fma), the arithmetic of upstream's
// `s_param.sub_(one_minus_decay * (s_param - param))` on fp32 tensors
__device__ __forceinline__ float ema_update(float s, float pn, float omd) {
#pragma clang fp contract(off)
    const float d = s - pn;
    const float t = omd * d;
    return s - t;
}

template <bool EMA>
__global__ __launch_bounds__(OB) void adam_tail_kernel(float* __restrict__ p, const float* __restrict__ g, float* __restrict__ m,
                                                        float* __restrict__ v, float* __restrict__ ema, int64_t count, float b1, float b2,
                                                        float eps, float bc1, float bc2_sqrt, float gscale,
                                                        const int64_t* __restrict__ state, const double* __restrict__ ctrl, int net) {
    // every word of the record is requested at once and the skip decision becomes an empty loop, not an early branch: a branch on the
    // guard in front of the other reads made a chain of dependent memory round trips out of one (measured: 0.3 us per launch of a
    // 9 us kernel; the one round trip that remains is what the tail costs over adam_kernel, whose lr is a launch argument)
    const double guard = ctrl[CTL_OPTIM_GUARD], finite = ctrl[CTL_OPTIM_FINITE];
    const float lr = (float)ctrl[CTL_OPTIM_LR + net];
    const float clip = (float)ctrl[CTL_OPTIM_CLIP];
    const float omd = (float)ctrl[CTL_OPTIM_EMA_OMD];
    if ((guard != 0.0) & (finite == 0.0)) count = 0;                                // a skipped step writes nothing
    if (state) {
        const double st = (double)state[2];
        bc1 = (float)(1.0 - pow((double)b1, st));
        bc2_sqrt = (float)sqrt(1.0 - pow((double)b2, st));
    }
    const int64_t stride = (int64_t)gridDim.x * OB;
    const float step_size = lr / bc1;
    for (int64_t i = (int64_t)blockIdx.x * OB + threadIdx.x; i < count; i += stride) {
        const float gi = g[i] * gscale * clip;
        const float mi = b1 * m[i] + (1.f - b1) * gi;
        const float vi = b2 * v[i] + (1.f - b2) * gi * gi;
        m[i] = mi;
        v[i] = vi;
        const float denom = sqrtf(vi) / bc2_sqrt + eps;
        const float pn = p[i] - step_size * (mi / denom);
        p[i] = pn;
        if (EMA) ema[i] = ema_update(ema[i], pn, omd);
    }
}

// ------------------------------------------------------------------------------------------------ launchers
extern "C" int ctl_optim_control(double* ctrl, int32_t k, const float* lr, float max_norm, int32_t skip_nonfinite, float ema_omd,
                                 ctl_stream stream) {
    CTL_REQUIRE(ctrl && lr, "optim_control: null pointer");
    CTL_REQUIRE(k >= 1 && k <= CTL_OPTIM_MAX_NETS, "optim_control: k = %d networks (1 <= k <= %d)", k, CTL_OPTIM_MAX_NETS);
    CTL_REQUIRE(max_norm >= 0.f && std::isfinite(max_norm), "optim_control: max_norm must be finite and >= 0 (0 = no clipping)");
    CTL_REQUIRE(ema_omd >= 0.f && ema_omd <= 1.f, "optim_control: ema_omd = 1 - decay must lie in [0, 1]");
    optim_lr8 a;
    for (int j = 0; j < CTL_OPTIM_MAX_NETS; ++j) a.v[j] = j < k ? lr[j] : 0.f;
    optim_control_kernel<<<dim3(1), dim3(64), 0, S_>>>(ctrl, k, a, max_norm, skip_nonfinite != 0, ema_omd);
    CTL_LAUNCH_CHECK("optim_control");
    return CTL_OK;
}

extern "C" size_t ctl_grad_norm_work(const int64_t* counts, int32_t k) {
    if (!counts || k < 1 || k > CTL_OPTIM_MAX_NETS) return 0;
    size_t total = 0;
    for (int j = 0; j < k; ++j) {
        if (counts[j] <= 0) return 0;
        total += (size_t)ctl_cdiv64(counts[j], CH);
    }
    return total;
}

extern "C" int ctl_grad_norm(const float* const* grads, const int64_t* counts, int32_t k, float grad_scale, double* work, double* ctrl,
                             ctl_stream stream) {
    CTL_REQUIRE(grads && counts && work && ctrl, "grad_norm: null pointer");
    CTL_REQUIRE(k >= 1 && k <= CTL_OPTIM_MAX_NETS, "grad_norm: k = %d buffers (1 <= k <= %d)", k, CTL_OPTIM_MAX_NETS);
    CTL_REQUIRE(((uintptr_t)work & 7) == 0 && ((uintptr_t)ctrl & 7) == 0, "grad_norm: work and ctrl must be 8-byte aligned");
    optim_bufs a;
    int64_t total = 0, widest = 0;
    for (int j = 0; j < CTL_OPTIM_MAX_NETS; ++j) {
        a.g[j] = nullptr;
        a.count[j] = a.woff[j] = 0;
        if (j >= k) continue;
        CTL_REQUIRE(grads[j], "grad_norm: null pointer (buffer %d)", j);
        CTL_REQUIRE(counts[j] > 0, "grad_norm: count of buffer %d must be positive", j);
        CTL_REQUIRE(((uintptr_t)grads[j] & 3) == 0, "grad_norm: buffer %d is not 4-byte aligned", j);
        const int64_t chunks = ctl_cdiv64(counts[j], CH);
        a.g[j] = grads[j];
        a.count[j] = counts[j];
        a.woff[j] = total;
        total += chunks;
        widest = chunks > widest ? chunks : widest;
    }
    CTL_REQUIRE(widest <= 0x7fffffff, "grad_norm: a buffer of more than 2^31 chunks");
    grad_norm_partial_kernel<<<dim3((unsigned)widest, (unsigned)k), dim3(OB), 0, S_>>>(a, work);
    CTL_LAUNCH_CHECK("grad_norm");
    grad_norm_final_kernel<<<dim3(1), dim3(64), 0, S_>>>(work, total, grad_scale, ctrl);
    CTL_LAUNCH_CHECK("grad_norm");
    return CTL_OK;
}

extern "C" int ctl_adam_tail(float* p, const float* g, float* m, float* v, float* ema, int64_t count, float beta1, float beta2, float eps,
                             const int64_t* state, int32_t step, float grad_scale, const double* ctrl, int32_t net, ctl_stream stream) {
    CTL_REQUIRE(p && g && m && v && ctrl, "adam_tail: null pointer");
    CTL_REQUIRE(count > 0, "adam_tail: count must be positive");
    CTL_REQUIRE(net >= 0 && net < CTL_OPTIM_MAX_NETS, "adam_tail: net = %d (0 <= net < %d)", net, CTL_OPTIM_MAX_NETS);
    CTL_REQUIRE(state || step >= 1, "adam_tail: step must be >= 1 when no device state is given");
    float bc1 = 1.f, bc2_sqrt = 1.f;
    if (!state) {
        bc1 = (float)(1.0 - pow((double)beta1, (double)step));
        bc2_sqrt = (float)sqrt(1.0 - pow((double)beta2, (double)step));
    }
    const dim3 grid(ctl_blocks(count, OB, OPT_MAX_STREAM_BLOCKS)), blk(OB);
    if (ema)
        adam_tail_kernel<true><<<grid, blk, 0, S_>>>(p, g, m, v, ema, count, beta1, beta2, eps, bc1, bc2_sqrt, grad_scale, state, ctrl, net);
    else
        adam_tail_kernel<false><<<grid, blk, 0, S_>>>(p, g, m, v, nullptr, count, beta1, beta2, eps, bc1, bc2_sqrt, grad_scale, state, ctrl, net);
    CTL_LAUNCH_CHECK("adam_tail");
    return CTL_OK;
}
