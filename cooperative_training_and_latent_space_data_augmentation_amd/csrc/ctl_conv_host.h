// Host side shared by the conv units (ctl_conv.hip, ctl_conv_x3.hip, ctl_conv_bf16.hip, ctl_wgrad_bf16.hip, ctl_wgrad_x3.hip) and
// ctl_plan.cpp: the record a descriptor becomes on its way to a launch, the occupancy query, the weight gradients' geometry, split
// sizing and argument check, the profiler's work model.  Host only: plain structs, static inline functions and templates -- nothing here
// allocates, formats a string outside a refusal, or asks the runtime anything per launch.
#pragma once
#include <type_traits>

#include "ctl_common.h"
#include "ctl_conv_common.h"

// One forward-type launch (conv, data gradient).  Tensors are untyped: the fp32 and X3 families cast at the launch (ctl_f), the bf16
// family's kernels take them as they are.
struct ctl_conv_call {
    const ctl_conv* d; ctl_conv_cfg c;
    const void *x, *x2, *wpack, *res, *res2; void *y, *pool, *xout;
    const float *bias, *pro_scale, *pro_shift, *res_scale, *res_shift; float* stats_partial;
    hipStream_t stream;
    bool query;                   // only answer (grid_x, stat_rows_per_block), launch nothing
    int grid_x;
    int stat_rows_per_block;      // X3: 4 for the producer / consumer form (one statistics row per consumer wave), else 1
};

// One weight-gradient launch.  ntw ... cout_p: ctl_wgrad_geometry; splits, cap, key: the answers of a query.
struct wg16_group;
struct ctl_wgrad_call {
    const ctl_conv* d; ctl_conv_cfg c; int ntw, ntiles, cin_p, cout_p;
    const void *x, *dy, *dy2; const float *pro_scale, *pro_shift, *dy_coef; float *w_partial, *b_partial;
    hipStream_t stream;
    bool query;                   // only answer (splits, cap, key), launch nothing
    int splits;
    int cap;                      // bf16: blocks of this instantiation the chip holds at once
    int key;                      // bf16: the instantiation the dispatch ends in (members of a grouped launch must agree)
    const wg16_group* grp;        // bf16: launch this stacked group instead of the single problem
    int grp_blocks;
    int pc;                       // X3: the producer / consumer kernel (32 x 32 blocks) was chosen
};

static inline const float* ctl_f(const void* p) { return (const float*)p; }
static inline float* ctl_f(void* p) { return (float*)p; }

// Resident 256-thread blocks per CU of a kernel instantiation; `fallback` where the runtime cannot say (no device).  Every site keeps
// the answer in a function-local static: one query per instantiation per process.
template <typename K>
static inline int ctl_resident_blocks(K kernel, int fallback) {
    int n = 0;
    if (hipOccupancyMaxActiveBlocksPerMultiprocessor(&n, kernel, 256, 0) != hipSuccess || n < 1) {
        (void)hipGetLastError();
        n = fallback;
    }
    return n;
}

// The (ks, stride, in_mode) combinations kernels are written for.  ctl_visit_shape hands the one of a descriptor to a generic
// f(K, S, MODE) -> bool as std::integral_constants, which become the template arguments of a family's dispatch; f answers false
// for what its family does not build (with `if constexpr`: nothing else is instantiated).  false: no kernel for the combination.
template <int V> using ctl_ic = std::integral_constant<int, V>;
template <typename F>
static inline bool ctl_visit_shape(int k, int s, int m, F&& f) {
    if (k == 3 && s == 1 && m == CTL_IN_PLAIN) return f(ctl_ic<3>{}, ctl_ic<1>{}, ctl_ic<CTL_IN_PLAIN>{});
    if (k == 3 && s == 1 && m == CTL_IN_UP2) return f(ctl_ic<3>{}, ctl_ic<1>{}, ctl_ic<CTL_IN_UP2>{});
    if (k == 3 && s == 1 && m == CTL_IN_ZINS2) return f(ctl_ic<3>{}, ctl_ic<1>{}, ctl_ic<CTL_IN_ZINS2>{});
    if (k == 3 && s == 1 && m == CTL_IN_C4) return f(ctl_ic<3>{}, ctl_ic<1>{}, ctl_ic<CTL_IN_C4>{});
    if (k == 3 && s == 2 && m == CTL_IN_PLAIN) return f(ctl_ic<3>{}, ctl_ic<2>{}, ctl_ic<CTL_IN_PLAIN>{});
    if (k == 1 && s == 1 && m == CTL_IN_PLAIN) return f(ctl_ic<1>{}, ctl_ic<1>{}, ctl_ic<CTL_IN_PLAIN>{});
    if (k == 1 && s == 1 && m == CTL_IN_UP2) return f(ctl_ic<1>{}, ctl_ic<1>{}, ctl_ic<CTL_IN_UP2>{});
    if (k == 2 && s == 2 && m == CTL_IN_PLAIN) return f(ctl_ic<2>{}, ctl_ic<2>{}, ctl_ic<CTL_IN_PLAIN>{});
    if (k == 2 && s == 1 && m == CTL_IN_PLAIN) return f(ctl_ic<2>{}, ctl_ic<1>{}, ctl_ic<CTL_IN_PLAIN>{});
    if (k == 4 && s == 2 && m == CTL_IN_PLAIN) return f(ctl_ic<4>{}, ctl_ic<2>{}, ctl_ic<CTL_IN_PLAIN>{});
    return false;
}

// cout tiles per block, pixel tiles and padded channel counts of a weight gradient, from a.d and the tile configuration a.c
static inline void ctl_wgrad_geometry(ctl_wgrad_call& a) {
    a.ntw = (a.c.cot >= 2 && a.c.cot % 2 == 0) ? 2 : 1;
    a.ntiles = a.d->n * a.c.tiles_h * a.c.tiles_w;
    a.cin_p = a.c.g * 16;
    a.cout_p = a.c.cot * 16;
}

// Pixel splits = blocks along x: the resident blocks dealt over the `par` (cin chunk, cout tile group) pairs, no more than `cap`,
// no empty split, at least one.
static inline int ctl_wgrad_clamp_splits(int resident_blocks, int par, int cap, int ntiles) {
    int splits = resident_blocks / par;
    if (splits > cap) splits = cap;
    if (splits > ntiles) splits = ntiles;
    return splits < 1 ? 1 : splits;
}

// The argument check of one weight-gradient problem: its tensors are there, the coefficient tables it stages fit their LDS copies
// (groups * cin of the prologue, groups * cout of the two-tensor output gradient: CTL_PRO_MAX), its tensors stay below 2 GiB.
// member < 0: a launch of its own (`who` = "conv_wgrad"), which names every condition; member >= 0: that member of a grouped launch.
static inline int ctl_wgrad_check(const ctl_conv* d, const void* x, const float* pro_scale, const float* pro_shift, const void* dy, const void* dy2,
                                  const float* dy_coef, const void* w_partial, const char* who, int member) {
    CTL_REQUIRE(d, "%s: null argument", who);
    const int ng = d->groups > 1 ? d->groups : 1;
    if (member < 0) {
        CTL_REQUIRE(x && dy && w_partial, "%s: null argument", who);
        CTL_REQUIRE(d->pro_affine == 0 || d->pro_affine == 1, "%s: pro_affine must be 0 or 1", who);
        CTL_REQUIRE(!dy2 || (dy_coef && d->ks == 3 && d->stride == 1 && d->cout % 16 == 0 && ng * d->cout <= CTL_PRO_MAX),
                    "%s: the two-tensor output gradient needs coefficients, a 3x3 stride-1 conv, cout %% 16 == 0 and groups * cout <= %d (got cout %d)", who, CTL_PRO_MAX, d->cout);
        CTL_REQUIRE(!d->pro_affine || (pro_scale && pro_shift), "%s: prologue without scale/shift", who);
        CTL_REQUIRE(!d->pro_affine || ng * d->cin <= CTL_PRO_MAX, "%s: groups * cin = %d prologue coefficients exceed %d", who, ng * d->cin, CTL_PRO_MAX);
        CTL_REQUIRE(!d->pro_affine || (d->pro_slope >= 0.f && d->pro_slope <= 1.f), "%s: prologue slope must be in [0, 1]", who);
    } else {
        CTL_REQUIRE(x && dy && w_partial && (!d->pro_affine || (pro_scale && pro_shift)) && (!dy2 || dy_coef), "%s: member %d misses a tensor", who, member);
        CTL_REQUIRE((!d->pro_affine || ng * d->cin <= CTL_PRO_MAX) && (!dy2 || ng * d->cout <= CTL_PRO_MAX),
                    "%s: member %d: groups * channels of a staged coefficient table > %d", who, member, CTL_PRO_MAX);
    }
    CTL_REQUIRE((int64_t)d->n * d->hin * d->win * d->cin * 4 < (1ll << 31) && (int64_t)d->n * d->hout * d->wout * d->cout * 4 < (1ll << 31),
                "%s: tensors must stay below 2 GiB (32-bit buffer offsets)", who);
    return CTL_OK;
}

// The profiler's algorithmic work of one problem: the contraction's flops, and x and y (a weight gradient: dy) once at their storage
// width -- twice where the operand is a tensor pair (x / x2 of the BatchNorm-backward prologue, dy / dy2 with `two_tensor`).
static inline void ctl_conv_work(const ctl_conv* d, bool two_tensor, double* flops, double* bytes) {
    const double pix = (double)d->n * d->hout * d->wout * d->nsub;
    *flops = 2.0 * pix * d->cout * d->cin * d->ks * d->ks;
    const double in_b = ((d->dt & CTL_DT_X16) ? 2.0 : 4.0) * d->n * d->hin * d->win * d->cin, out_b = ((d->dt & CTL_DT_Y16) ? 2.0 : 4.0) * pix * d->cout;
    *bytes = in_b * (d->pro_affine == 2 ? 2 : 1) + out_b * (two_tensor ? 2 : 1);
}
