/*
 * ctl_hip.h -- C-ABI of libctl_hip.so: the MI355X (gfx950) kernels behind the cooperative-training hot path.
 *
 * The reference (cherise215/Cooperative_Training_and_Latent_Space_Data_Augmentation) is pure PyTorch-eager and has
 * no FFI of its own; every entry point below replaces the ATen ops that the cited reference lines dispatch.
 * "model.py" = medseg/models/advanced_triplet_recon_segmentation_model.py,
 * "encdec.py" = medseg/models/ebm/encoder_decoder.py, "util.py" = medseg/models/model_util.py.
 *
 * Conventions
 *   - all tensors are fp32 NHWC ("channels_last") in device memory owned by the caller (bf16 where a ctl_conv.dt / op flag says so:
 *     the `float*` in those signatures is then the base address of bf16 data); labels are int64 NHW
 *   - every call only enqueues work on `stream`; no allocation, no host sync, no retained pointers
 *   - return 0 on success, negative ctl_status on error; ctl_last_error() gives a thread-local message
 *   - scratch / partial-sum buffers are sized by the *_ws_* helpers and passed in by the caller
 */
#ifndef CTL_HIP_H
#define CTL_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef void* ctl_stream;            /* hipStream_t */

enum ctl_status { CTL_OK = 0, CTL_EINVAL = -1, CTL_EUNSUPPORTED = -2, CTL_ELAUNCH = -3 };

/* ABI version: bumped whenever a struct layout, an argument list or a plan-op slot assignment changes.  Bindings must compare
 * ctl_version() with the CTL_ABI_VERSION they were written against (and ctl_sizeof_conv / ctl_sizeof_op with their struct sizes)
 * at load time and refuse to run on a mismatch.  3 = round 3: fused-finalize entry points and side lanes removed, `ds` argument of
 * ctl_bwd_reduce_dt, ctl_red_blocks().  4 = CTL_EPI_TAILBWD / ctl_conv_forward_ex (plan op CONV slot 10).
 * 5 = ctl_bn_finalize_ex (save_uvar, plan op BN_FINALIZE slot 10), ctl_bn_replay_running / CTL_OP_BN_REPLAY.
 * 6 = the BatchNorm-backward prologue: ctl_conv.pro_affine == 2 + the x2 argument of ctl_conv_forward_ex (plan op CONV slot 11),
 *     ctl_conv_wgrad_ex (plan op WGRAD slots 6, 7); CTL_EPI_TAILBWD in the bf16 family.
 * 7 = the `pool` argument of ctl_conv_forward_ex (plan op CONV slot 12; CTL_OP_MAX_T 12 -> 14: sizeof(ctl_op) 304 -> 328), ctl_conv_pool_ok.
 * 8 = the `xout` argument of ctl_conv_forward_ex (plan op CONV slot 13).
 * 9 = CTL_DT_X3 / CTL_PACK_X3, ctl_conv_wpack_floats_x3, ctl_pack_weights_x3_batched; plan op PACK_BATCH i[1] is a bit mask.
 * 10 = grouped weight gradients: ctl_wgrad_group_class / ctl_wgrad_group_plan / ctl_conv_wgrad_group, plan op CTL_OP_WGRAD_GROUP.
 * 11 = ctl_bn_bwd_finalize_ex (per-group gamma / beta gradient switch; plan op BN_BWD_FINALIZE i[4]); a WGRAD record with i[24] != 0 is refused
 *      outside its WGRAD_GROUP. */
#define CTL_ABI_VERSION 11
int         ctl_version(void);
const char* ctl_last_error(void);

/* ------------------------------------------------------------------------------------------------ convolution
 * One implicit-GEMM kernel family (MFMA f32 16x16x4, LDS-staged NHWC input tiles) serves
 *   nn.Conv2d 3x3 s1/s2 p1 and 1x1          encdec.py:40-55, 323-335, 371-376, 390-391, 439-440, 469-474
 *   nn.ConvTranspose2d k2 s2                 encdec.py:302            (4 scattered 1x1 problems, `nsub` = 4)
 *   nn.UpsamplingNearest2d folded into the consumer conv's input indexing   encdec.py:294-296 (in_mode 1)
 *   every dgrad (conv over dy with transposed/flipped weights; stride-2 dgrad via zero-insertion, in_mode 2)
 * with BatchNorm-apply + LeakyReLU fused into the input staging ("prologue") and bias / residual / activation /
 * BatchNorm statistics fused into the epilogue.
 */
enum { CTL_IN_PLAIN = 0, CTL_IN_UP2 = 1, CTL_IN_ZINS2 = 2, CTL_IN_C4 = 3 /* plain input with <= 4 channels, 3x3 stride 1: the taps are
       K-packed (weights from ctl_pack_weights_batched mode 4); 12 MFMAs per pixel tile instead of 36 */ };
enum { CTL_ACT_NONE = 0, CTL_ACT_LEAKY = 1, CTL_ACT_SIGMOID = 2 };
enum { CTL_EPI_BIAS = 1, CTL_EPI_ACCUM = 2, CTL_EPI_RES = 4, CTL_EPI_STATS = 8, CTL_EPI_BNBWD = 16, CTL_EPI_TAILBWD = 32 };

typedef struct ctl_conv {
    int32_t n, hin, win, cin;        /* stored input tensor [n,hin,win,cin]                                   */
    int32_t hout, wout, cout;        /* output pixel grid of this problem and its channel count               */
    int32_t ks, stride, pad;         /* 3/1|2/1, 1/1/0, 2/2/0                                                  */
    int32_t in_mode;                 /* CTL_IN_*: virtual input = stored | nearest-up x2 | zero-insert x2     */
    int32_t pro_affine;              /* 1: x <- leaky(x*pro_scale[c]+pro_shift[c], pro_slope) while staging;
                                        needs max(groups,1)*cin <= 256 (the coefficients sit in an LDS table)   */
    float   pro_slope;
    int32_t epi_flags;               /* CTL_EPI_*                                                             */
    int32_t epi_act;                 /* CTL_ACT_* applied after bias/residual                                  */
    float   epi_slope;
    int32_t out_h, out_w;            /* output tensor [n,out_h,out_w,cout]; pixel (ho,wo) of sub-problem z     */
    int32_t out_sy, out_sx;          /*   lands at (ho*out_sy + z/2*out_sub, wo*out_sx + z%2*out_sub)          */
    int32_t nsub, out_sub;           /* nsub = 1 (plain) or 4 (ConvTranspose k2s2: out_sy=out_sx=2,out_sub=1)  */
    int32_t groups;                  /* BatchNorm groups along n (0/1 = one): images [g*n/groups, (g+1)*n/groups) use row g of
                                        pro_scale/pro_shift/res_scale/res_shift ([groups][c]) and get their own statistics
                                        partials -- several independent passes of one network batched into one launch   */
    int32_t dt;                      /* CTL_DT_* : 0 = everything fp32 (BASELINE config 2).  CTL_DT_BF16 selects the bf16 kernel family
                                        (v_mfma_f32_16x16x32_bf16: operands rounded to bf16 AFTER the fp32 prologue, fp32 accumulate,
                                        fp32 bias / BatchNorm statistics / epilogue; weights packed as bf16 by the *_batched pack with
                                        the same flag); CTL_DT_X16 / _Y16 / _RES16: that tensor is STORED as bf16 (activation storage
                                        of BASELINE config 3) -- network inputs / outputs stay fp32.
                                        CTL_DT_X3 (alone; fp32 tensors; cin a multiple of 16, cout a multiple of 16 or 4 / 8 / 12 (the
                                        weight gradient: both multiples of 16); 2x2 / 3x3 / 4x4 kernels): the SAME
                                        fp32 computation with the contraction on the bf16 matrix pipe -- every operand is split
                                        exactly into three bf16 numbers while it is staged, six v_mfma_f32_16x16x32_bf16 per
                                        contraction step (hi*hi + hi*mid + mid*hi + mid*mid + hi*lo + lo*hi, fp32 accumulate): error
                                        per product <= 2^-24 (1 + 2^-8) worst case (the rounding of one fp32 multiply), typically 2^-25; 16/6 of the fp32 MFMA rate.
                                        Weights come from ctl_pack_weights_x3_batched (records with CTL_PACK_X3)                    */
} ctl_conv;
enum { CTL_DT_BF16 = 1, CTL_DT_X16 = 2, CTL_DT_Y16 = 4, CTL_DT_RES16 = 8, CTL_DT_X3 = 16 };
enum { CTL_PACK_X3 = 16 };          /* or-ed into the mode word of a pack record: three-plane bf16 fragments for CTL_DT_X3 launches */

/* number of floats of the packed weight buffer for one sub-problem, and of the statistics partial buffer */
size_t ctl_conv_wpack_floats(int32_t cin, int32_t cout, int32_t ks);
size_t ctl_conv_stats_floats(const ctl_conv* d);     /* [groups][blocks][2][cout] */
int    ctl_conv_stats_blocks(const ctl_conv* d);

/* Pack weights into MFMA-fragment order.  Element (co,ci,kh,kw) of the *effective* conv is read from
 * src[co*s_co + ci*s_ci + kh'*s_kh + kw'*s_kw] with (kh',kw') = flip ? (ks-1-kh, ks-1-kw) : (kh,kw).  Covers OIHW
 * forward weights, their dgrad transposes and both ConvTranspose2d uses.
 * Destination contract of every pack entry point (this one and the *_batched forms below): the destination need NOT be zeroed.  A pack
 * writes every element of its record's layout that a conv kernel reads, the zero padding of the cin / cout fragments up to whole
 * 16-channel tiles and of an odd last tap included, and nothing outside [dst_off, dst_off + ctl_conv_wpack_floats(_x3)) (mode 4: + ceil(cout / 16) * 3 * 256): a repack after
 * an optimizer step does not depend on what the buffer held.  The fp32 and X3 layouts fill that range completely; the bf16 layout fills
 * its first ceil(taps / 2) / taps part and neither writes nor reads the rest (tests/test_pack_guard_gpu.py). */
int ctl_pack_weights(const float* src, float* dst, int32_t cout, int32_t cin, int32_t ks,
                     int64_t s_co, int64_t s_ci, int64_t s_kh, int64_t s_kw, int32_t flip, ctl_stream stream);

/* y = epi( conv(pro(x)) ).  res/res_scale/res_shift: CTL_EPI_RES adds res*res_scale[c]+res_shift[c] (the
 * BatchNorm'ed main branch of res_convdown / res_up_family, encdec.py:64,344).  stats_partial: CTL_EPI_STATS.
 * CTL_EPI_BNBWD (with CTL_EPI_STATS; a data-gradient conv whose result is dL/da of a = leaky(BN(u), epi_slope)): res = u,
 * res_scale/res_shift = the BatchNorm coefficients; y = g = conv * leaky'(u*scale+shift) and stats_partial receives
 * (sum g, sum g*u) -- the reduction pass of the BatchNorm backward (ctl_bwd_reduce mode 1) folded into the producer. */
int ctl_conv_forward(const ctl_conv* d, const float* x, const float* wpack, const float* bias,
                     const float* pro_scale, const float* pro_shift,
                     const float* res, const float* res_scale, const float* res_shift,
                     float* y, float* stats_partial, ctl_stream stream);
/* ... with a second epilogue tensor.  CTL_EPI_TAILBWD (with CTL_EPI_STATS, optionally CTL_EPI_ACCUM; cout % 16 == 0; fp32, or the bf16
 * family with bf16-stored y / res / res2 -- there the sums come from the unrounded g and dOut is never rounded on its own; the 1x1 / 2x2 /
 * zero-insert 3x3 launches that write the output gradient of a residual block, encdec.py:64,344): the conv result (+ y with
 * CTL_EPI_ACCUM) is dL/dOut of out = leaky(S + BN(v), epi_slope); res = out, res2 = v.  y receives g = dOut * leaky'(out) and
 * stats_partial (sum g, sum g*v) per BatchNorm group: the reduction pass of the residual tail (ctl_bwd_reduce mode 0) folded into the
 * producer of dOut, which is then never materialised.  res2 == NULL: plain ctl_conv_forward. */
/* x2 (with ctl_conv.pro_affine == 2; BOTH families -- fp32 tensors, or the bf16 family with bf16-stored x / x2 / y; cin % 16 == 0,
 * plain (CTL_IN_PLAIN) 3x3 stride-1 or 4x4 stride-2 conv, groups * cin <= 256, not together with CTL_EPI_TAILBWD): the
 * BatchNorm-backward prologue.  The conv input is the VIRTUAL tensor
 *     A[c] * x + B[c] * x2 + C[c]     (zero outside the image; bf16 family: rounded to bf16 as the stored tensor would have been)
 * with pro_scale = the [group][A | B | C][cin] coefficients ctl_bn_bwd_finalize writes (pro_shift is not read): x = g = dL/da * leaky',
 * x2 = the BatchNorm input.  This is ctl_bwd_apply (mode 2) run inside the staging of its consumer: the data-gradient convs of a
 * residual block read (g, u) instead of dU, which is never written.  x2 == NULL and pro_affine <= 1: as before. */
int ctl_conv_forward_ex(const ctl_conv* d, const float* x, const float* wpack, const float* bias,
                        const float* pro_scale, const float* pro_shift,
                        const float* res, const float* res_scale, const float* res_shift, const float* res2, const float* x2,
                        float* y, float* stats_partial, float* pool, float* xout, ctl_stream stream);
/* pool (with CTL_EPI_TAILBWD on a 1x1 conv with even output sizes; ctl_conv_pool_ok(d) says whether d's tile configuration can do it):
 * the epilogue also writes the 2x2 sum-pool of g, [n, out_h/2, out_w/2, cout] -- the input of the consuming block's 1x1 weight / data
 * gradients behind a nearest-neighbour up-sampling (encdec.py:344): the stand-alone ctl_sumpool2 pass disappears.  fp32: the same
 * association as ctl_sumpool2, bit-identical; bf16: pooled from the unrounded g, rounded once.  NULL: not written. */
int ctl_conv_pool_ok(const ctl_conv* d);
/* xout (with pro_affine == 2; a tensor of x's geometry and storage type): the conv also WRITES the virtual input A*x + B*x2 + C it stages --
 * every input pixel by the tile that owns it, from the blocks of the first output-channel group -- so that the weight-gradient kernel of
 * the same layer reads it as a plain output gradient (ctl_conv_wgrad) instead of evaluating it again in each of its cin-chunk blocks
 * (ctl_conv_wgrad_ex: +10-18 % fp32, +14-44 % bf16 in isolation).  Issue this conv BEFORE that weight gradient.  NULL: not written. */

/* Weight gradient of the conv described by d (x [n,hin,win,cin] -> dy [n,hout,wout,cout], nsub must be 1):
 * partial[split][tap][cin16][cout16] (+ bias partial[split][cout16]); then ctl_wgrad_reduce sums the splits and
 * (accumulate ? += : =) into a gradient tensor with the same generic strides as ctl_pack_weights. */
int    ctl_wgrad_splits(const ctl_conv* d);
size_t ctl_wgrad_partial_floats(const ctl_conv* d);          /* weights part  */
size_t ctl_wgrad_bias_partial_floats(const ctl_conv* d);     /* bias part     */
int ctl_conv_wgrad(const ctl_conv* d, const float* x, const float* pro_scale, const float* pro_shift,
                   const float* dy, float* w_partial, float* b_partial, ctl_stream stream);
/* ... whose output gradient is the virtual BatchNorm-backward result  A[c] * dy + B[c] * dy2 + C[c]  (dy_coef = [group][A | B | C][cout]
 * from ctl_bn_bwd_finalize; BOTH families -- fp32 dy / dy2, or the bf16 family with bf16-stored dy / dy2; 3x3 stride-1 convs,
 * cout % 16 == 0, groups * cout <= 256): the other
 * consumer of a block's dU / dV (see ctl_conv_forward_ex).  The bias gradient is the sum of the virtual tensor.  dy2 == NULL: ctl_conv_wgrad. */
int ctl_conv_wgrad_ex(const ctl_conv* d, const float* x, const float* pro_scale, const float* pro_shift,
                      const float* dy, const float* dy2, const float* dy_coef, float* w_partial, float* b_partial, ctl_stream stream);

/* Grouped weight gradients (ABI 10).  The reference computes every layer's dW inside autograd's backward sweep, one cuDNN/MKL call per layer
 * (encoder_decoder.py:19-68, 285-348 under loss.backward(), train_adv_supervised_segmentation_triplet.py:225).  Nothing downstream of a backward
 * pass reads dW before the optimizer (or the gradient all-reduce), so the plan compiler defers the X3 weight gradients of a pass and serves up to
 * 8 of one class with ONE launch: the CUs are dealt to the members in proportion to their work.  Per launch ~15 us are fixed (launch, exposed first
 * loads, reduction tail) against ~25 us of work for an n = 16 layer; a member of a group gets fewer CUs, more tiles per block, fewer split-K partials.
 *   ctl_wgrad_group_class: >= 0 (the class: members of one launch must agree) if `d` (CTL_DT_X3, 3x3 stride 1, plain / nearest-up-sampled input,
 *                          cin and cout multiples of 32, hout >= 8) can ride in a group, -1 otherwise.  has_dy2: the two-tensor output gradient.
 *   ctl_wgrad_group_plan : the members' pixel splits; member i then needs splits[i] * 9 * cin * cout floats of w_partial (and splits[i] * cout of
 *                          b_partial), laid out and reduced exactly like ctl_conv_wgrad's ([split][tap][cin][cout]; ctl_wgrad_reduce_batched).
 *   ctl_conv_wgrad_group : the launch.  Arrays of n pointers; pro_scale / pro_shift / dy2 / dy_coef / b_partial entries (or the arrays) may be NULL
 *                          where a member has none.
 * The bf16 family (CTL_DT_BF16) rides the same three entry points: class = 0x100 | the kernel instantiation its dispatch ends in (any bf16 weight
 * gradient has one), the launch stacks the members' own grids along blockIdx.x, ctl_wgrad_group_plan deals the resident blocks in proportion to
 * the work (never more splits than a launch of its own); with splits[i] = ctl_wgrad_splits(d_i) a member's partial sums are bit for bit those of
 * ctl_conv_wgrad_ex (tests/test_bf16_gpu.py). */
int ctl_wgrad_group_class(const ctl_conv* d, int32_t has_dy2);
int ctl_wgrad_group_plan(const ctl_conv* descs, int32_t n, int32_t* splits);
int ctl_conv_wgrad_group(int32_t n, const ctl_conv* descs, const int32_t* splits, const float* const* x, const float* const* pro_scale,
                         const float* const* pro_shift, const float* const* dy, const float* const* dy2, const float* const* dy_coef,
                         float* const* w_partial, float* const* b_partial, ctl_stream stream);
int ctl_wgrad_reduce(const ctl_conv* d, const float* w_partial, const float* b_partial,
                     float* dw, int64_t s_co, int64_t s_ci, int64_t s_kh, int64_t s_kw,
                     float* dbias, int32_t accumulate, ctl_stream stream);

/* Batched forms (one launch for a whole network): `table` is a device array of int64 records.
 * pack record   (12 words): src_off, dst_off (floats into params / wpack), cout, cin, ks, flip, s_co, s_ci, s_kh, s_kw, total, mode;
 *                           total = the float count of the record's packed buffer, max_total the largest; mode = the layout (0 plain, 1 the 4x4 kernel
 *                           summed from 3x3 taps, 2 / 3 a 2x2 phase with the phase in `flip`, 4 K-packed first layer), | CTL_PACK_X3
 * reduce record (16 words): w_off, b_off (floats into scratch; b_off < 0: none), dw_off, db_off (floats into grad; db_off < 0:
 *                           none), splits, taps_ks (taps | ks << 8), cin, cout, cin_p, cout_p, s_co, s_ci, s_kh, s_kw, accumulate,
 *                           reserved (0); max_blocks = max over records of ceil((elements + cout) / (splits <= 64 ? 64 : 8)) */
int ctl_pack_weights_batched(const float* params, float* wpack, const int64_t* table, int32_t n_rec, int64_t max_total,
                             ctl_stream stream);
int ctl_wgrad_reduce_batched(const float* scratch, float* grad, const int64_t* table, int32_t n_rec, int64_t max_blocks,
                             ctl_stream stream);
/* bf16 MFMA fragments for the CTL_DT_BF16 kernels from the same pack records (modes 0-3): per 16-channel chunk a fragment carries a PAIR
 * of taps (v_mfma_f32_16x16x32_bf16 has 32 k-slots), values rounded to bf16 (RNE) from the fp32 master weights; written at the same
 * float offsets as the fp32 layout (it is smaller: 5 of 9 fragments for a 3x3 kernel).  max_total as for ctl_pack_weights_batched. */
int ctl_pack_weights_bf16_batched(const float* params, float* wpack, const int64_t* table, int32_t n_rec, int64_t max_total,
                                  ctl_stream stream);
/* Fragments for the CTL_DT_X3 launches from the pack records whose mode word carries CTL_PACK_X3 (the other records are skipped; the
 * fp32 / bf16 pack entries skip these): [cout tile][tap pair][chunk][split hi | mid | lo][64 lanes][8 bf16], the three bf16 numbers of
 * a split summing EXACTLY to the fp32 weight.  ctl_conv_wpack_floats_x3 = the float count of one sub-problem's buffer (15 KB per
 * (cout tile, chunk) of a 3x3 kernel against 9 KB of the fp32 layout); max_total = the largest such count among the records. */
size_t ctl_conv_wpack_floats_x3(int32_t cin, int32_t cout, int32_t ks);
int ctl_pack_weights_x3_batched(const float* params, float* wpack, const int64_t* table, int32_t n_rec, int64_t max_total,
                                ctl_stream stream);

/* ------------------------------------------------------------------------------------------------ BatchNorm2d
 * encdec.py: every `norm(out_ch)`; three modes of SURVEY 8a row 4 (util.py:414-451).
 * `groups` (>= 1): independent passes of one network batched along n (ctl_conv.groups).  Statistics partials are
 * [groups][blocks][2][c], every coefficient vector is [groups][c] (coef: [groups][3][c]), `count` is the pixel count of
 * ONE group, `pixels` the total; running statistics and dgamma/dbeta see the groups in order, as consecutive calls would.
 * finalize: partial [blocks][2][c] (sum, sum of squares over `count` pixels) -> scale=gamma*invstd,
 * shift=beta-mean*scale, save_mean, save_invstd; if update_running: running stats (momentum, unbiased var) and
 * num_batches_tracked (int64) are updated in place. */
int ctl_bn_finalize(const float* partial, int32_t blocks, int32_t c, int64_t count, const float* gamma,
                    const float* beta, float eps, float momentum, int32_t update_running, float* running_mean,
                    float* running_var, int64_t* num_batches_tracked, float* scale, float* shift, float* save_mean,
                    float* save_invstd, int32_t groups, ctl_stream stream);
/* ... additionally saving the unbiased batch variance as the float the running update used (save_uvar, [groups][c], may be NULL) */
int ctl_bn_finalize_ex(const float* partial, int32_t blocks, int32_t c, int64_t count, const float* gamma,
                       const float* beta, float eps, float momentum, int32_t update_running, float* running_mean,
                       float* running_var, int64_t* num_batches_tracked, float* scale, float* shift, float* save_mean,
                       float* save_invstd, float* save_uvar, int32_t groups, ctl_stream stream);
/* The running-statistics update of n_rec BatchNorm layers replayed from saved batch statistics (save_mean / save_uvar of a forward pass
 * whose activations are re-used instead of recomputed: the saliency pass of the targeted latent masks decodes, in training mode, the very
 * code the standard pass has just decoded -- util.py:214 after model.py:444 / 436-440).  table: n_rec int64 records,
 * replay record (6 words): save_mean_off, save_uvar_off (bytes into `act`), running_mean_off, running_var_off (floats into `buffers`),
 *                           nbt_idx (index into num_batches_tracked), c;
 * Bit-identical to running the pass again: the same two floats enter the same momentum update. */
int ctl_bn_replay_running(const void* act, float* buffers, int64_t* num_batches_tracked, const int64_t* table, int32_t n_rec,
                          float momentum, ctl_stream stream);
/* eval mode: scale = gamma/sqrt(running_var+eps), shift = beta - running_mean*scale */
int ctl_bn_eval_coeffs(int32_t c, const float* gamma, const float* beta, const float* running_mean,
                       const float* running_var, float eps, float* scale, float* shift, int32_t groups, ctl_stream stream);
/* y = leaky(x*scale[c]+shift[c], slope)  (slope 0 = ReLU, slope 1 = identity) */
int ctl_bn_act(const float* x, const float* scale, const float* shift, float slope, float* y, int64_t pixels,
               int32_t c, int32_t groups, ctl_stream stream);

/* backward helpers; `partial` buffers are [groups][rows][2][c] floats, rows = ctl_bwd_reduce_rows() <= CTL_RED_BLOCKS */
#ifndef CTL_RED_BLOCKS
#define CTL_RED_BLOCKS 512
#endif
/* mode 0 (residual tail, encdec.py:64,344): g = dout * leaky'(out);        sums: sum g, sum g*v
 * mode 1 (BN->act tail):                    g = da * leaky'(u*scale+shift); sums: sum g, sum g*u
 * mode 2 (plain):                           g = da;                         sums: sum g, (unused)          */
int ctl_bwd_reduce(int32_t mode, const float* dy, const float* act_src, const float* bn_src, const float* scale,
                   const float* shift, float slope, int64_t pixels, int32_t c, float* partial, int32_t groups,
                   ctl_stream stream);
/* rows per group that ctl_bwd_reduce* writes for this problem: min(CTL_RED_BLOCKS, max(16, ceil(quads per group / 2048))) for modes
 * 0 / 1, CTL_RED_BLOCKS for mode 2; ctl_red_blocks() returns the compiled CTL_RED_BLOCKS (bindings size their scratch with it) */
int ctl_bwd_reduce_rows(int32_t mode, int64_t pixels_per_group, int32_t c);
int ctl_red_blocks(void);
/* partial -> coefficients A,B,C with dx = A*g + B*bn_src + C (training-mode BN backward), and, if dgamma/dbeta
 * are non-NULL, dgamma += sum g*xhat, dbeta += sum g (accumulate ? += : =). */
/* `blocks` = rows per group of `partial` (0 = CTL_RED_BLOCKS, i.e. written by ctl_bwd_reduce; a conv with CTL_EPI_BNBWD
 * writes ctl_conv_stats_blocks rows) */
int ctl_bn_bwd_finalize(const float* partial, int32_t c, int64_t count, const float* gamma, const float* save_mean,
                        const float* save_invstd, float* coef, float* dgamma, float* dbeta, int32_t accumulate,
                        int32_t groups, int32_t blocks, ctl_stream stream);
/* the same with a per-group switch for the gamma / beta gradients: bit g of `affine_groups` set = group g adds its sums (0 = every group).
 * A launch that stacks passes of different BatchNorm modes along n (round 6: the standard pass, mode A, and the hard-example pass, mode B =
 * gamma / beta frozen for that pass, model_util.py:414-451) clears the bits of the frozen passes; every group still gets its coefficients. */
int ctl_bn_bwd_finalize_ex(const float* partial, int32_t c, int64_t count, const float* gamma, const float* save_mean,
                           const float* save_invstd, float* coef, float* dgamma, float* dbeta, int32_t accumulate,
                           int32_t groups, int32_t blocks, uint32_t affine_groups, ctl_stream stream);
/* mode 0: ds = dout*leaky'(out) (written if ds != NULL), dv = A*ds + B*v + C;  mode 1: du = A*g + B*u + C with g = dy*leaky'(..);
 * mode 2: dy is already g (CTL_EPI_BNBWD): du = A*dy + B*u + C */
int ctl_bwd_apply(int32_t mode, const float* dy, const float* act_src, const float* bn_src, const float* scale,
                  const float* shift, float slope, const float* coef, int64_t pixels, int32_t c, float* ds,
                  float* dx, int32_t groups, ctl_stream stream);
/* partial[blocks][2][c] -> out[c] (+)= sum over blocks of row 0 (bias gradient of ConvTranspose2d) */
int ctl_chan_sum_finalize(const float* partial, int32_t c, float* out, int32_t accumulate, ctl_stream stream);
/* nearest-upsample backward: dx[n,h,w,c] = sum of the 2x2 block of dup[n,2h,2w,c]; accumulate ? += : = */
int ctl_sumpool2(const float* dup, float* dx, int32_t n, int32_t h, int32_t w, int32_t c, int32_t accumulate,
                 ctl_stream stream);
/* dlogit = dy * y * (1-y)  (nn.Sigmoid of image_decoder, model.py:100) */
int ctl_sigmoid_bwd(const float* dy, const float* y, float* dx, int64_t count, ctl_stream stream);

/* ------------------------------------------------------------------------------------------------ STN input, losses
 * construct_input (medseg/common_utils/basic_operations.py:110-158): softmax(x/T, dim=C) or one-hot(label) */
int ctl_softmax_t_fwd(const float* x, float inv_t, float* p, int64_t pixels, int32_t c, ctl_stream stream);
int ctl_softmax_t_bwd(const float* p, const float* dp, float inv_t, float* dx, int64_t pixels, int32_t c,
                      ctl_stream stream);
int ctl_onehot(const int64_t* label, float* y, int64_t pixels, int32_t c, ctl_stream stream);
/* cross_entropy_2D (medseg/models/custom_loss.py:706-740, util.py:104-115): loss = mean_pixels -log_softmax[label].
 * fwd writes loss[0]; partial is [CTL_RED_BLOCKS] doubles.  bwd: dlogit = gout[0] * (softmax - onehot) / pixels */
int ctl_ce2d_fwd(const float* logit, const int64_t* label, int64_t pixels, int32_t c, double* partial, float* loss,
                 ctl_stream stream);
int ctl_ce2d_bwd(const float* logit, const int64_t* label, const float* gout, int64_t pixels, int32_t c,
                 float* dlogit, ctl_stream stream);
/* The other supervised losses of basic_loss_fn (medseg/models/custom_loss.py:8-40), fp32 NHWC logits [b][hw][c] against an int64 label map
 * [b][hw] (ctl_loss.hip).  p = softmax over c, t = one-hot of the label, M = b * hw, s = 0.01:
 *   CTL_LOSS_WCE     cross_entropy_2D with class weights (:720-740): w' = w / sum(w) * c;  loss = (1/M) sum_pix w'[y] * -log p_y (the divisor
 *                    is M, not sum w');  dlogit_k = gout * w'[y] (p_k - t_k) / M.  class_weights = NULL: upstream's uniform 1/c, i.e. w' = 1.
 *   CTL_LOSS_FOCAL   FocalLoss(gamma) (:222-255): loss = (1/M) sum_pix -(1 - p_y)^gamma log p_y.  Upstream detaches p_y (:243), so the gradient
 *                    is gout * (1 - p_y)^gamma (p_k - t_k) / M -- not the derivative of the value.
 *   CTL_LOSS_DICE    SoftDiceLoss (:356-396): per sample and class I = sum p t + s, U = sum p + sum t + s; loss = 1 - (sum 2I/U) / (b c).
 *   CTL_LOSS_FG_DICE SelectiveSoftDiceLoss over the classes 1..c-1 (:434-471): term (2 sum p t + s) / (sum p + sum t + s), divisor b (c - 1).
 *                    Both Dice forms: g_k = dL/dp_k = coef[b][k][0] t_k + coef[b][k][1], dlogit_j = gout p_j (g_j - sum_k p_k g_k).
 * A label outside 0..c-1 is no class (t = 0 for every k, weight 0); labels are compared, never used as an index.
 * class_weights: HOST array of c doubles (read during the call, CTL_LOSS_WCE only) or NULL; gamma: CTL_LOSS_FOCAL only.
 * ws: ctl_seg_loss_ws_doubles(kind, b, hw, c) doubles, every one written by the forward.  Point-wise kinds: [CTL_RED_BLOCKS] block sums.
 *   Dice kinds: [b][ctl_seg_loss_blocks(b, hw)][c][3] block sums (sum p, sum p t, count of y == k), then the [b][c][2] coefficient table the
 *   backward reads -- hand the forward's ws to the backward (the point-wise kinds ignore it there, NULL allowed).  The blocks per sample are
 *   capped at CTL_RED_BLOCKS / b (at least 1), so the block sums never exceed max(CTL_RED_BLOCKS, b) * c * 3 doubles.
 * fwd: two launches (partial sums, one finalize block) write loss[0]; bwd: one launch reads gout[0] on the device and writes every element of
 * dlogit.  Sums are ordered, fp64, free of atomics: the same bits on every call and in a graph replay.  Rows of c == 4 in 16-byte aligned
 * tensors move as 16 bytes; any other case takes the runtime-count kernels, same arithmetic in the same order.
 * Null pointers, an unknown kind, non-positive sizes, c outside 1..16 (foreground Dice: 2..16), more than 65535 samples, a tensor at or past
 * 2 GiB, class weights whose sum is not finite and positive, and a gamma that is not finite and >= 0 are refused with CTL_EINVAL before any
 * launch; ctl_seg_loss_ws_doubles returns 0 for them. */
enum { CTL_LOSS_WCE = 0, CTL_LOSS_FOCAL = 1, CTL_LOSS_DICE = 2, CTL_LOSS_FG_DICE = 3 };
int32_t ctl_seg_loss_blocks(int32_t b, int64_t hw);
size_t ctl_seg_loss_ws_doubles(int32_t kind, int32_t b, int64_t hw, int32_t c);
int ctl_seg_loss_fwd(int32_t kind, const float* logit, const int64_t* label, const double* class_weights, float gamma, int32_t b,
                     int64_t hw, int32_t c, double* ws, float* loss, ctl_stream stream);
int ctl_seg_loss_bwd(int32_t kind, const float* logit, const int64_t* label, const double* class_weights, float gamma, const float* gout,
                     const double* ws, int32_t b, int64_t hw, int32_t c, float* dlogit, ctl_stream stream);
/* Distance-map losses (no upstream counterpart; ctl_dist.hip, ctl_loss.hip): the boundary loss of Kervadec et al. (MIDL 2019) and the
 * distance-transform Hausdorff loss of Karimi & Salcudean (IEEE TMI 2019, alpha = 2), with the distance maps computed per step on the device.
 *
 * ctl_class_fields: label uint8 or int64 [b][h][w] (label_dtype CTL_LABEL_*), n_class in 1..16, unit spacing, per slice.  With S the pixels
 *   of a slice that carry class k (a label outside 0..n_class-1 belongs to no S), the class field F_k(p) is the exact Euclidean distance from p
 *   to the nearest pixel of S for p outside S and to the nearest pixel NOT in S for p inside S; F_k = 0 everywhere when S is empty or fills
 *   the plane.  D2_k = F_k^2 is an integer.  out, by `form`:
 *     CTL_FIELD_D2       double [b][n_class][h][w]   D2
 *     CTL_FIELD_SIGNED   float  [b][h][w][n_class]   the signed map phi: F outside S, -(F - 1) inside, 0 where F = 0; the fp64 value rounded once
 *     CTL_FIELD_SQUARED  float  [b][h][w][n_class]   D2 (exact: every D2 < 2^24)
 *   The float forms have the layout of NHWC logits.  h, w <= 2048: the transform runs in 32-bit integers; longer axes are refused.
 *   workspace: ctl_class_fields_ws_bytes(b, h, w, n_class) bytes (two uint16 row-distance maps per class).  Two launches whatever the sizes and
 *   the content are; no readback, no atomics, the same bits on every call and in a graph replay.
 * ctl_confident_label: logit float NHWC [pixels][c] -> out uint8 [pixels]: k if softmax(logit)_k > 0.5 (strictly; at most one class can), else
 *   255.  The softmax is the fp32 one of the loss kernels.  One launch.
 * ctl_dist_loss_fwd / _bwd: logit float NHWC [b][hw][c], c in 2..16, p = softmax over c, t = one-hot of the int64 label [b][hw] (out of range:
 *   t = 0), classes 1..c-1, div = b (c - 1) hw.  The fields are INPUTS, float [b][hw][c] as ctl_class_fields writes them:
 *     CTL_DLOSS_BOUNDARY      field_a = signed map of the label (field_b and label unused, NULL allowed):
 *                             loss = (1/div) sum p_k a_k;  g_k = a_k / div
 *     CTL_DLOSS_HAUSDORFF_DT  field_a = squared field of the label, field_b = squared field of ctl_confident_label(logit), a constant:
 *                             loss = (1/div) sum (p_k - t_k)^2 (a_k + b_k);  g_k = 2 (p_k - t_k)(a_k + b_k) / div
 *   g_0 = 0 and dlogit_j = gout p_j (g_j - sum_k p_k g_k).  fwd: two launches (fp64 block sums into ws, ctl_dist_loss_ws_doubles doubles, then
 *   one finalize block in a fixed order) write loss[0]; bwd: one launch recomputes the softmax, reads gout[0] on the device and writes every
 *   element of dlogit.
 * Null pointers, an unknown dtype / form / kind, non-positive sizes, a class count out of range, an axis above 2048, a tensor at or past 2 GiB
 * and a workspace that is too small are refused with CTL_EINVAL before any launch; the size queries return 0 for them. */
enum { CTL_LABEL_U8 = 0, CTL_LABEL_I64 = 1 };
enum { CTL_FIELD_D2 = 0, CTL_FIELD_SIGNED = 1, CTL_FIELD_SQUARED = 2 };
enum { CTL_DLOSS_BOUNDARY = 0, CTL_DLOSS_HAUSDORFF_DT = 1 };
size_t ctl_class_fields_ws_bytes(int32_t b, int32_t h, int32_t w, int32_t n_class);
int ctl_class_fields(const void* label, int32_t label_dtype, int32_t b, int32_t h, int32_t w, int32_t n_class, int32_t form, void* out,
                     void* workspace, size_t workspace_bytes, ctl_stream stream);
int ctl_confident_label(const float* logit, uint8_t* out, int64_t pixels, int32_t c, ctl_stream stream);
size_t ctl_dist_loss_ws_doubles(int32_t kind, int32_t b, int64_t hw, int32_t c);
int ctl_dist_loss_fwd(int32_t kind, const float* logit, const int64_t* label, const float* field_a, const float* field_b, int32_t b,
                      int64_t hw, int32_t c, double* ws, float* loss, ctl_stream stream);
int ctl_dist_loss_bwd(int32_t kind, const float* logit, const int64_t* label, const float* field_a, const float* field_b, const float* gout,
                      int32_t b, int64_t hw, int32_t c, float* dlogit, ctl_stream stream);
/* Consistency losses (ctl_consist.hip): losses between two PREDICTIONS, medseg/models/custom_loss.py calc_segmentation_consistency :892-973 with
 * kl_divergence :863-889, soft-target cross_entropy_2D :741-766, the softmax 'mse' :942-952, SoftDiceLoss with a 4-D target :356-396 and the
 * Sobel contour_loss :784-860.  x = output logits, r = reference, both float NHWC [b][h][w][c], c in 1..16; mask uint8 [b][h][w] (nonzero = 1)
 * or NULL.  q = softmax(x); p = softmax(r), or p = r when is_gt.  M = b h w, R = sum m (M without a mask), s = 0.01.  r is a constant.
 *   CTL_CONS_KL       (1/M) sum_pix m sum_k p_k (log p_k - log q_k).  is_gt: upstream's rule, p_k = 1 where r_k != 0 else float(1e-8), with
 *                     p_k log p_k = 0 resp. the float product 1e-8f * logf(1e-8f).  dlogit_j = (m/M)(S q_j - p_j), S = sum_k p_k.
 *   CTL_CONS_CE       -(1/R) sum_pix m sum_k p_k log q_k;  R = 0: loss 0, gradient 0.
 *   CTL_CONS_WCE      -(1/R) sum_pix m sum_k w'_k p_k log q_k, w' = w / sum(w) * c.  Both: dlogit_j = (m/R)(q_j sum_k w'_k p_k - w'_j p_j).
 *   CTL_CONS_MSE      (1/M) sum_pix m sum_k (q_k - p_k)^2;  g_k = 2 m (q_k - p_k) / M.
 *   CTL_CONS_DICE     1 - (sum_{b,k} 2I/U) / (b c), per (b,k): I = sum m q p + s, U = sum m q + sum m p + s;  g_k = -(m/(b c))(2 p_k/U - 2I/U^2).
 *   CTL_CONS_CONTOUR  (1/(c-1)) sum_{k=1..c-1} 1/2 (1/M) sum_pix m (E_x^2 + E_y^2), c >= 2: with d = q - p, E_x / E_y are the 3x3 zero-padded
 *                     cross-correlations of d_k with [[1,0,-1],[2,0,-2],[1,0,-1]] / [[1,2,1],[0,0,0],[-1,-2,-1]] (:823-841);
 *                     g_k = (1/((c-1) M)) (S_x^T(m E_x) + S_y^T(m E_y))_k, g_0 = 0.
 *   The kinds with a g: dlogit_j = q_j (g_j - sum_k q_k g_k).
 * kinds: a non-empty set of CTL_CONS_* bits; bit t is kind t.  weights: HOST array of 6 doubles, entry t the weight of kind t (read for
 * the selected kinds only).  class_weights: HOST array of c doubles, CTL_CONS_WCE only, else NULL allowed.
 * ctl_consistency_fwd writes loss[7]: loss[0] = sum_t weights[t] term_t, loss[1 + t] = term_t (0 for a kind that is not selected); a term has
 *   the same bits whichever other kinds are selected beside it.  Launches: one streaming pass over x, r and the mask for ANY set of the
 *   first five kinds (fp64 block sums, the masked count among them), one tiled pass for CTL_CONS_CONTOUR (d of the classes 1..c-1 in LDS at
 *   halo 1; tiles of 32x32 pixels up to 4 classes, 16x16 above), then one finalize block.
 * ws: ctl_consistency_ws_doubles(kinds, b, h, w, c) doubles: the Dice coefficient table [b][c][2] (g_k = m (coef0 p_k + coef1); zeros
 *   without CTL_CONS_DICE), a record of 8 doubles ([0] = 1/R or 0, [1] = R, the rest 0), then -- with one of the first five kinds -- the block
 *   sums [b][ctl_seg_loss_blocks(b, h w)][5 + 3c] and -- with CTL_CONS_CONTOUR -- min(tiles, 2048) block sums.  Every double is written by the
 *   forward; hand the forward's ws to the backward with the same kinds.
 * ctl_consistency_bwd writes every element of dlogit = gout[0] * sum_t weights[t] dterm_t/dx (gout read on the device), q and p recomputed:
 *   one streaming launch for the first five kinds together; the contour gradient is a SECOND, tiled launch (d at halo 2 and the masked
 *   responses at halo 1 in LDS, the transposed stencil at the centre) that adds into dlogit -- it writes dlogit when it is the only kind.
 * ctl_avgpool_fwd: AvgPool2d(2^scale) of float NHWC [b][h][w][c] -> [b][h >> scale][w >> scale][c], scale in 1..4: each window summed in a
 *   fixed order in fp64, rounded once.  ctl_avgpool_bwd: gx = gy * 4^-scale on every pixel of a window, zero on the rows / columns the floor drops.
 * No float atomics, no readback: the same bits on every call and in a graph replay.  Null pointers, an empty or unknown kind set, non-positive
 * sizes, c outside 1..16 (contour: 2..16), more than 65535 samples, a tensor at or past 2 GiB, a weight that is not finite, class weights
 * whose sum is not finite and positive, a scale outside 1..4 and a plane smaller than the window are refused with CTL_EINVAL before any
 * launch; ctl_consistency_ws_doubles returns 0 for them. */
enum { CTL_CONS_KL = 1, CTL_CONS_CE = 2, CTL_CONS_WCE = 4, CTL_CONS_MSE = 8, CTL_CONS_DICE = 16, CTL_CONS_CONTOUR = 32 };
size_t ctl_consistency_ws_doubles(int32_t kinds, int32_t b, int32_t h, int32_t w, int32_t c);
int ctl_consistency_fwd(int32_t kinds, const double* weights, const double* class_weights, const float* x, const float* r,
                        const uint8_t* mask, int32_t is_gt, int32_t b, int32_t h, int32_t w, int32_t c, double* ws, float* loss,
                        ctl_stream stream);
int ctl_consistency_bwd(int32_t kinds, const double* weights, const double* class_weights, const float* x, const float* r,
                        const uint8_t* mask, int32_t is_gt, const float* gout, const double* ws, int32_t b, int32_t h, int32_t w,
                        int32_t c, float* dlogit, ctl_stream stream);
int ctl_avgpool_fwd(const float* x, int32_t b, int32_t h, int32_t w, int32_t c, int32_t scale, float* y, ctl_stream stream);
int ctl_avgpool_bwd(const float* gy, int32_t b, int32_t h, int32_t w, int32_t c, int32_t scale, float* gx, ctl_stream stream);
/* Image-similarity (reconstruction) losses (ctl_recon.hip) between a prediction x and a constant target t, medseg/models/custom_loss.py:
 * smooth_l1_loss :310-318, CustomNormalizedCrossCorrelationLoss :514-571, CustomLocalNormalizedCrossCorrelationLoss :574-661, next to
 * 'mse' and 'l1'.  x float NHWC [b][h][w][c], c in 1..16; t the same, or one sample [1][h][w][c] broadcast over the batch (t_batch = 1:
 * upstream's single template, :536); mask uint8 [b][h][w] (nonzero = 1) or NULL multiplies both first: J = m x, I = m t.  N = b c h w;
 * reduce_sum = 0: the means below, 1: the sums (every 1/N, 1/b below becomes 1; CTL_RECON_LNCC: 1 - c * sum of the scores).
 *   CTL_RECON_MSE        (1/N) sum (J - I)^2;  dJ = 2 (J - I) / N.
 *   CTL_RECON_L1         (1/N) sum |J - I|;  dJ = sign(J - I) / N, 0 where they are equal.
 *   CTL_RECON_SMOOTH_L1  (1/N) sum (n < beta ? 0.5 n^2 / beta : n - 0.5 beta), n = |J - I| (:313-315);  dJ = (n < beta ? (J - I) / beta : sign) / N.
 *   CTL_RECON_NCC        1 - (1/b) sum_b s_b, s_b = <a, u> / (max(|a|, 1e-6) max(|u|, 1e-6)) over the c h w elements of a sample, with
 *                        a = J - mean_hw J, u = I - mean_hw I per sample and channel when zero_mean (:545-549), else a = J, u = I (the
 *                        clamped norms of torch's CosineSimilarity(dim=1, eps=1e-6), :556);  dJ = -(1/b)(u / (Na Nu) - [|a| > eps] <a,u> a / (Na^3 Nu)).
 *   CTL_RECON_LNCC       1 - (1/(b h w)) sum_p score_p (:608-661): the five sums I, J, I^2, J^2, I J over the win x win window (zero padding
 *                        win / 2) AND all c channels, A = win^2, uI = I_sum / A, uJ = J_sum / A, cross = IJ_sum - uJ I_sum - uI J_sum +
 *                        uI uJ A, I_var = I2_sum - 2 uI I_sum + uI^2 A (J_var alike), score = cross / (sqrt(I_var) sqrt(J_var) + 1e-6).
 *                        A variance <= 2^-40 (its sum of squares) counts as exactly 0 (and its b_p as 0).  dJ_q = -(1/(b h w)) (I_q Sa -
 *                        J_q Sb + Sc) with Sa, Sb, Sc the window sums of a_p = 1 / D_p, b_p = cross_p sqrt(I_var_p) / (D_p^2 sqrt(J_var_p))
 *                        and b_p uJ_p - a_p uI_p.  win odd, 3..15, win <= h, win <= w.
 * kinds: a non-empty set of CTL_RECON_* bits; bit k is kind k.  weights: HOST array of 5 doubles, entry k the weight of kind k (read for the
 * selected kinds only).  beta is read with CTL_RECON_SMOOTH_L1, win with CTL_RECON_LNCC, zero_mean with CTL_RECON_NCC.
 * ctl_recon_loss_fwd writes loss[6]: loss[0] = sum_k weights[k] term_k, loss[1 + k] = term_k (0 for a kind that is not selected); a term has
 *   the same bits whichever other kinds are selected beside it.  Launches: one streaming pass over x, t and the mask for ANY set of the
 *   first four kinds (ordered fp64 block sums: the three point-wise sums and, per channel, sum x, t, x^2, t^2, x t), one tiled pass for
 *   CTL_RECON_LNCC (16x16 pixel tiles, the channel-summed I, J, I^2, J^2, I J of the tile plus a halo of win / 2 in LDS as fp64, separable
 *   row-then-column window sums; it leaves the maps a_p, b_p, b_p uJ_p - a_p uI_p in ws), then one finalize block.
 * ws: ctl_recon_ws_doubles(kinds, b, h, w, c, win) doubles, every one written by the forward: per sample (1 / (Na Nu), [|a| > eps] <a,u> /
 *   (Na^3 Nu)) [b][2], the subtracted means [b][c][2], the channel sums [b][c][5] (zeros without CTL_RECON_NCC), then -- with one of the first
 *   four kinds -- the block sums [b][ctl_seg_loss_blocks(b, h w)][3 + 5c] and -- with CTL_RECON_LNCC -- min(tiles, 2048) block sums and the
 *   three maps [b][h][w][3].  Hand the forward's ws to the backward with the same arguments.
 * ctl_recon_loss_bwd writes every element of dx = gout[0] * sum_k weights[k] dterm_k/dx (gout read on the device) in ONE launch, formed in
 *   fp64 and rounded once: a streaming launch for the first four kinds; with CTL_RECON_LNCC a tiled launch that stages the three maps
 *   with a halo of win / 2, takes their window sums and adds the point-wise kinds' gradient in the same thread.  dx is exactly 0 where the mask is 0.
 * No float atomics, no readback: the same bits on every call and in a graph replay.  Null pointers, an empty or unknown kind set,
 * non-positive sizes, c outside 1..16, more than 65535 samples, t_batch other than 1 or b, tensors of 2^31 elements or more, a weight that
 * is not finite, beta <= 0, win even or outside 3..15, win > h or win > w are refused with CTL_EINVAL before any launch;
 * ctl_recon_ws_doubles returns 0 for them. */
enum { CTL_RECON_MSE = 1, CTL_RECON_L1 = 2, CTL_RECON_SMOOTH_L1 = 4, CTL_RECON_NCC = 8, CTL_RECON_LNCC = 16 };
size_t ctl_recon_ws_doubles(int32_t kinds, int32_t b, int32_t h, int32_t w, int32_t c, int32_t win);
int ctl_recon_loss_fwd(int32_t kinds, const double* weights, const float* x, const float* t, const uint8_t* mask, int32_t t_batch, int32_t b,
                       int32_t h, int32_t w, int32_t c, double beta, int32_t win, int32_t zero_mean, int32_t reduce_sum, double* ws,
                       float* loss, ctl_stream stream);
int ctl_recon_loss_bwd(int32_t kinds, const double* weights, const float* x, const float* t, const uint8_t* mask, int32_t t_batch,
                       const float* gout, const double* ws, int32_t b, int32_t h, int32_t w, int32_t c, double beta, int32_t win,
                       int32_t zero_mean, int32_t reduce_sum, float* dx, ctl_stream stream);
/* Adversarial input augmentation (ctl_adv.hip; adversarial.py holds the float64 statement; a project addition, no upstream counterpart).
 * Bias field: x float NHWC [n][h][w][c], c in 1..16, planes up to 2048 x 2048, n in 1..65535; integer control-point spacing s >= 2; theta
 * float [n][gh][gw] in log space with gh = (h - 1) / s + 4, gw = (w - 1) / s + 4 (integer division).  For pixel row y: i = y / s,
 * t = (y - i s) / s, columns alike; S(y, x) = sum_{a,b = 0..3} B_a(t_y) B_b(t_x) theta[i_y + a][i_x + b] with the uniform cubic B-spline
 * basis B0 = (1 - t)^3 / 6, B1 = (3 t^3 - 6 t^2 + 4) / 6, B2 = (-3 t^3 + 3 t^2 + 3 t + 1) / 6, B3 = t^3 / 6 (the approximating spline, no
 * prefilter: the weights are non-negative and sum to 1, |S| <= max |theta|); f = exp(S); x' = x f, the same field for every channel.
 * ctl_adv_bias_fwd writes every element of y = x' and, unless f is NULL, of f [n][h][w] in ONE launch: the 16-term sum and exp in fp64, f
 *   rounded to fp32 once, x' the fp64 product rounded once.  y (and f) must not overlap x: in place is refused.
 * ctl_adv_bias_bwd, given g = dL/dx': dtheta [n][gh][gw] = My^T (f sum_c g_c x_c) Mx with M the [h][gh] / [w][gw] weight matrices above,
 *   and, unless dx is NULL, dx = g f (rounded once from fp64).  TWO launches, separable: one block per image row recomputes f, keeps
 *   q = f sum_c g_c x_c of the row in LDS as fp64 and leaves sum_x Mx[x][b] q[x] for every control column b in ws ([n][gw][h] doubles,
 *   ctl_adv_bias_ws_bytes; 8-byte aligned); one wave per control point then sums My[y][a] times those over the rows of its support.
 *   Every dtheta element is an ordered fp64 sum (lanes stride the support, then the xor butterfly) rounded once; a control point with an
 *   empty support gets exactly 0.
 * Unit step: g float [n][m], m in 1 .. 16 * 2048 * 2048; per sample out = scale g / norm(g) with norm CTL_ADV_L2 sqrt(sum g^2), CTL_ADV_RMS
 *   sqrt(sum g^2 / m), CTL_ADV_LINF max |g|; a sample whose norm is 0 or not finite gives zeros.  TWO launches: ordered fp64 partials over
 *   fixed chunks of 16384 elements (the result does not depend on the grid) in ws (ctl_adv_unit_scale_ws_bytes), then every block combines
 *   its sample's chunks in order and writes its elements, each formed in fp64 and rounded once.  out must not overlap g.
 * No float atomics, no readback: the same bits on every call, at every alignment and in a graph replay.  s < 2, a grid that disagrees
 * with h, w and s, n outside 1..65535, a plane edge above 2048, c outside 1..16, n h w c of 2^31 or more, an unknown norm, a scale that is
 * not finite, null required pointers, an undersized or misaligned workspace and overlapping outputs are refused with CTL_EINVAL before any
 * launch; the size queries return 0 for sizes the entries refuse. */
enum { CTL_ADV_L2 = 0, CTL_ADV_RMS = 1, CTL_ADV_LINF = 2 };
size_t ctl_adv_bias_ws_bytes(int32_t n, int32_t h, int32_t w, int32_t s);
int ctl_adv_bias_fwd(const float* x, const float* theta, int32_t n, int32_t h, int32_t w, int32_t c, int32_t s, int32_t gh, int32_t gw,
                     float* y, float* f, ctl_stream stream);
int ctl_adv_bias_bwd(const float* g, const float* x, const float* theta, int32_t n, int32_t h, int32_t w, int32_t c, int32_t s, int32_t gh,
                     int32_t gw, void* ws, size_t ws_bytes, float* dtheta, float* dx, ctl_stream stream);
size_t ctl_adv_unit_scale_ws_bytes(int32_t n, int64_t m);
int ctl_adv_unit_scale(const float* g, int32_t n, int64_t m, int32_t norm, double scale, void* ws, size_t ws_bytes, float* out,
                       ctl_stream stream);
/* loss = scale * mean((a-b)^2) (model.py:445-447: scale 0.5; util.py:216: scale 1); bwd: da = gout*2*scale*(a-b)/count */
int ctl_mse_fwd(const float* a, const float* b, int64_t count, float scale, double* partial, float* loss,
                ctl_stream stream);
int ctl_mse_bwd(const float* a, const float* b, const float* gout, int64_t count, float scale, float* da,
                ctl_stream stream);
/* pred.max(1)[1] (model.py:657): first maximal channel, uint8 out */
int ctl_argmax_c(const float* logit, uint8_t* out, int64_t pixels, int32_t c, ctl_stream stream);

/* Storage-type aware forms of the element-wise kernels that touch network-internal tensors (BASELINE config 3 stores those as bf16):
 * `bf16_mask` bit k = tensor argument k (in the order x,y | dy,act_src,bn_src | dy,act_src,bn_src,ds,dx | dup,dx) is bf16; the
 * arithmetic is fp32, a store rounds once (RNE).  mask 0 == the plain entry points above. */
int ctl_bn_act_dt(const float* x, const float* scale, const float* shift, float slope, float* y, int64_t pixels, int32_t c,
                  int32_t groups, uint32_t bf16_mask, ctl_stream stream);
/* ds (mode 0 only, may be NULL): also writes ds = dy * leaky'(act_src) (bf16_mask bit 3 = its storage), so that the apply pass can run
 * in mode 2 on ds instead of recomputing it from dy and act_src */
int ctl_bwd_reduce_dt(int32_t mode, const float* dy, const float* act_src, const float* bn_src, const float* scale,
                      const float* shift, float slope, int64_t pixels, int32_t c, float* partial, int32_t groups,
                      uint32_t bf16_mask, float* ds, ctl_stream stream);
int ctl_bwd_apply_dt(int32_t mode, const float* dy, const float* act_src, const float* bn_src, const float* scale,
                     const float* shift, float slope, const float* coef, int64_t pixels, int32_t c, float* ds, float* dx,
                     int32_t groups, uint32_t bf16_mask, ctl_stream stream);
int ctl_sumpool2_dt(const float* dup, float* dx, int32_t n, int32_t h, int32_t w, int32_t c, int32_t accumulate,
                    uint32_t bf16_mask, ctl_stream stream);

/* ------------------------------------------------------------------------------------------------ latent masking
 * util.py:224-249 (channel) / 285-312 (spatial).  mode 0: score[n,c] = mean_hw grad; mode 1: score[n,hw] = mean_c grad.
 * `scratch` holds ctl_latent_score_ws_floats() floats (deterministic two-stage sum, no float atomics).
 * ctl_latent_mask_apply: entry i of row n is masked iff
 * #{j : score[n,j] >= score[n,i]} <= k  (== "score > sort(desc)[k]", strict, util.py:231-244);
 * mask value = soft_noise ? 0.5*soft_noise[n,i] : 0; kept = 1.  k is read from k_dev[0] if k_dev != NULL (graph replay)
 * else from k_host.  masked = code * mask (broadcast), mask_out [n,L].  Rows up to 1024 entries are ranked inside the apply
 * kernel; longer rows (spatial mode on large latents) take the threshold from a per-image bitonic sort (scratch). */
size_t ctl_latent_score_ws_floats(int32_t mode, int32_t n, int32_t hw, int32_t c);
int ctl_latent_score(int32_t mode, const float* grad, float* score, float* scratch, int32_t n, int32_t hw, int32_t c,
                     ctl_stream stream);
size_t ctl_latent_mask_apply_ws_floats(int32_t mode, int32_t n, int32_t hw, int32_t c);   /* 0 unless the row is > 1024 long */
int ctl_latent_mask_apply(int32_t mode, const float* code, const float* score, const float* soft_noise,
                          int32_t k_host, const int32_t* k_dev, float* masked, float* mask_out, float* scratch, int32_t n,
                          int32_t hw, int32_t c, ctl_stream stream);
/* The whole generator tail behind one call (reference: util.py:224-249 / 285-312).  Latent codes up to 64 Ki elements per image with
 * rows <= 1024 (the configured 128 x 16 x 16 included) run as ONE launch: one 1024-thread block per image holds the image's grad and
 * code in registers, builds the score row in LDS, ranks, and stores code * mask -- no workspace (ctl_latent_mask_fused_ws_floats == 0).
 * Larger problems are HBM streams and run as the score + apply launches above on `workspace`.  Scores (and therefore masks) are
 * bit-identical between the two forms.  score_out (nullable) receives the [n,L] scores.  Rows up to 8192 entries. */
size_t ctl_latent_mask_fused_ws_floats(int32_t mode, int32_t n, int32_t hw, int32_t c);
int ctl_latent_mask_fused(int32_t mode, const float* grad, const float* code, const float* soft_noise, int32_t k_host,
                          const int32_t* k_dev, float* masked, float* mask_out, float* score_out, float* workspace, int32_t n,
                          int32_t hw, int32_t c, ctl_stream stream);
/* F.dropout2d(z,p) (model.py:333): out = z * keep[n,c] / (1-p).  keep != NULL: injected {0,1} floats; else drawn on
 * device from a counter hash of (seed, n*c index) and written to keep_out. */
int ctl_dropout2d(const float* z, const float* keep, uint64_t seed, float p, float* out, float* keep_out, int32_t n,
                  int32_t hw, int32_t c, ctl_stream stream);
/* 0.5*U[0,1) style uniform fill from the same counter hash (soft-mask noise, util.py:239) */
int ctl_uniform(float* out, int64_t count, uint64_t seed, ctl_stream stream);
/* HIP-graph-safe forms: nothing that changes from step to step is a launch ARGUMENT.  `state` is a device int64[3]:
 * [0] RNG seed, [1] RNG step counter, [2] Adam step count; ctl_step_tick (one launch at the head of a training step, replaces the
 * host-side `step += 1` of torch.optim.Adam and the per-call host seed draw) advances [1] and [2].  With state != NULL the first
 * integer argument is a per-call-site salt.  ctl_dropout2d_ex additionally writes (mask_full != NULL) upstream's dropout `mask`
 * (model.py:334-336: 1 where the dropped-out tensor equals the input element, else 0; [n,hw,c] like out). */
int ctl_step_tick(int64_t* state, ctl_stream stream);
/* One idle wave for `microseconds` on `stream`: the host-side probe for "do these two streams overlap?" (streams share a few hardware
 * queues; the two launch chains of a training step must not sit on the same one, see solver.py) */
int ctl_spin(int32_t microseconds, ctl_stream stream);
int ctl_dropout2d_ex(const float* z, const float* keep, uint64_t seed_or_salt, const int64_t* state, float p, float* out,
                     float* keep_out, float* mask_full, int32_t n, int32_t hw, int32_t c, ctl_stream stream);
int ctl_uniform_dev(float* out, int64_t count, uint64_t salt, const int64_t* state, ctl_stream stream);
/* nn.Dropout2d behind every residual block (encoder_dropout / decoder_dropout, model.py:27-28, 92-106; encoder_decoder.py:58-66, 338-347):
 * ctl_dropout2d_ex on network-internal tensors, which BASELINE config 3 stores as bf16.  bf16_mask: bit 0 = z, bit 1 = out are bf16
 * ([n,hw,c] either way); the product z * keep / (1-p) is formed in fp32 and rounded once by the store. */
int ctl_dropout2d_dt(const void* z, const float* keep, uint64_t seed_or_salt, const int64_t* state, float p, void* out,
                     float* keep_out, int32_t n, int32_t hw, int32_t c, uint32_t bf16_mask, ctl_stream stream);

/* ------------------------------------------------------------------------------------------------ SURVEY 8(f) rows 1, 3
 * Validation metrics and the input pipeline on device (no host round trip per batch).
 * ctl_confusion_hist: `runningScore._fast_hist` (medseg/common_utils/metrics.py:18-23): hist[n_class*t + p] += 1 for every
 *   element with 0 <= t < n_class (p = predicted label, uint8 as written by ctl_argmax_c); hist is int64 [n_class*n_class] and
 *   ACCUMULATES (zero it to start a new evaluation); n_class <= 16.  Integer atomics only: order-independent, bit-exact.
 * ctl_rescale_intensity: per plane (n*c planes of plane_elems floats) (x-min)/(max-min+eps)*(new_max-new_min)+new_min
 *   (medseg/common_utils/basic_operations.py:232-245), torch's operation order, one rounding per operation.
 * ctl_noise_clamp: out = clamp(x + noise, lo, hi) (train_adv_supervised_segmentation_triplet.py:185-187); noise == NULL:
 *   sigma * N(0,1) drawn on device from a counter hash of (seed, index) (Box-Muller).
 * ctl_crop_or_pad: centre crop / zero pad of [n,h,w] arrays to [n,new_h,new_w] (medseg/common_utils/basic_operations.py:
 *   173-220): dst[y][x] = src[y + floor((h-new_h)/2)][x + floor((w-new_w)/2)] or 0 outside; elem_bytes 1, 4 or 8. */
int ctl_confusion_hist(const int64_t* label_true, const uint8_t* label_pred, int64_t count, int32_t n_class, int64_t* hist,
                       ctl_stream stream);
size_t ctl_rescale_intensity_ws_floats(int32_t planes);
int ctl_rescale_intensity(const float* x, float* out, float* workspace, int32_t planes, int64_t plane_elems, float new_min,
                          float new_max, float eps, ctl_stream stream);
int ctl_noise_clamp(const float* x, const float* noise, uint64_t seed, float sigma, float lo, float hi, float* out,
                    int64_t count, ctl_stream stream);
int ctl_crop_or_pad(const void* src, void* dst, int32_t elem_bytes, int32_t n, int32_t h, int32_t w, int32_t new_h,
                    int32_t new_w, ctl_stream stream);

/* ------------------------------------------------------------------------------------------------ surface distances
 * 'HD' / 'ASD' of the patient score table (medseg/common_utils/metrics.py:224-230) = medpy 0.4.0 `hd` / `asd` as carried by
 * medseg/common_utils/measure.py:333-548 on the surface-distance construction of measure.py:1096-1128, which upstream runs on
 * the host per class, per direction and (HD) per slice: scipy binary_erosion + distance_transform_edt.  Here, for EVERY class and
 * BOTH directions of one patient in 4 (mode 2) or 5 (mode 3) kernel launches, whatever D, H, W and n_class are:
 *   masks     class c (1 <= c < n_class): pred == c and gt == c; foreground_only: pred > 0 and gt > 0 (one class).  pred is uint8
 *             [D,H,W] (as written by ctl_argmax_c), gt int64 [D,H,W]; a gt label outside [0, n_class) belongs to no class.
 *   surface   mask XOR erosion(mask), scipy defaults: border_value 0 (a mask voxel on the edge of the array is a surface voxel),
 *             structuring element generate_binary_structure(mode, connectivity) = the neighbours at L1 offset <= connectivity.
 *   mode      2: every [H,W] slice on its own (`hd_2D_stack`), sampling = {s_y, s_x};  3: the volume, sampling = {s_z, s_y, s_x};
 *             `sampling` is a HOST array in array-axis order, read during the call, NULL = 1; 1 <= connectivity <= mode.
 *   distance  EXACT Euclidean distance to the nearest surface voxel of the other mask: separable lower envelope evaluated over all
 *             candidates of a row / column / slice axis in fp64 (no window, no chamfer, no jump flooding); with unit sampling every
 *             squared distance is an exact integer.
 *   table     fp64 [rows][4], row = (class_index * 2 + side) * (mode == 2 ? D : 1) + (mode == 2 ? z : 0), class_index = c - 1,
 *             rows as ctl_surface_stats_rows says.  Row (c, side) takes the distance map of the surface of side's mask (0 = pred,
 *             1 = gt) and samples it at the surface voxels of the OTHER side's mask: {max d^2, sum of d, number of sampled voxels,
 *             1.0 if either mask (of this slice, mode 2) is empty else 0.0}.  With an empty target mask d is +inf.
 *             HD of a slice = sqrt(max of the two sides' max d^2); ASD(pred -> gt) = sum / number of row (c, 1).
 *             Sums are per-block partials combined in a fixed order: no floating-point atomics, identical bits on every call.
 * ctl_surface_map: the same passes for ONE mask (uint8, non-zero = inside): d2_out (fp64 [D,H,W], may be NULL) = squared distance of
 *   every voxel to the nearest surface voxel of the mask (+inf when there is none), surface_out (uint8 [D,H,W] of 0 / 1, may be NULL) =
 *   the surface map itself; 1 to 4 launches.  The workspace is needed only with d2_out.
 * ctl_surface_quantiles: order statistics of the POOLED surface distances of a class, i.e. of both directions in ONE list, which is what
 *   the 95th-percentile Hausdorff distance needs ('HD95': medpy >= 0.4 `hd95` = np.percentile(np.hstack((d(result -> reference),
 *   d(reference -> result))), 95); in the score table per slice and averaged, by analogy with 'HD' of
 *   medseg/common_utils/metrics.py:226-233).  The average symmetric surface distance ('ASSD', measure.py:402-455) needs no selection: it
 *   is the mean of sum / number of rows (c, 0) and (c, 1) of the 3-D statistics table.
 *   Masks, surfaces, mode, connectivity, sampling, the axis limit and the workspace alignment are those of ctl_surface_stats.
 *   q         HOST array of n_q (1..4) percentages, each finite and in [0, 100], read during the call; the call passes q[j] / 100.0
 *             (one fp64 division on the host) to the device by value.
 *   q_table   fp64 [classes][G][n_q][4], G = D in mode 2 and 1 in mode 3, classes as in ctl_surface_stats (class_index = c - 1).  A
 *             group (class, slice in mode 2) pools the n sampled squared distances of both sides; with k = floor((n - 1) * q / 100)
 *             (one fp64 multiply on the device) the entry is {d^2 of rank k, d^2 of rank min(k + 1, n - 1), n, flag} in ascending
 *             order, from which the host finishes numpy's linear-interpolation percentile of the distances exactly (sqrt is monotone).
 *             flag = 1.0 when either mask of the group is empty; the entry is then {+inf, +inf, 0, 1}.
 *   stats_table  NULL, or the table ctl_surface_stats writes for the same arguments: the same rows, reduction order and bits.
 *   launches  those of ctl_surface_stats (4 / 5; the last one is left out when stats_table is NULL) plus exactly 3: surface-voxel counts
 *             per (side, slice, class), their scan into key-list offsets, and the selection.  The number does not depend on D, H, W,
 *             n_class, n_q or the content; there is no readback and no synchronisation.  Selection is an exact most-significant-digit-
 *             first radix selection over the 64 bits of the squared distances with integer atomics only; the order in which keys land in
 *             the workspace differs from call to call, every output is the same bits on every call.
 * Workspaces are caller-owned, sized by the *_ws_bytes queries (0 for arguments the call itself would refuse) and need 256-byte
 * alignment.  Every axis is limited to 65534 elements.  Every argument error of ctl_surface_quantiles returns CTL_EINVAL with a
 * message that names surface_quantiles, before anything is launched. */
int32_t ctl_surface_stats_rows(int32_t d, int32_t n_class, int32_t foreground_only, int32_t mode);
size_t ctl_surface_stats_ws_bytes(int32_t d, int32_t h, int32_t w, int32_t n_class, int32_t foreground_only, int32_t mode);
int ctl_surface_stats(const uint8_t* pred, const int64_t* gt, int32_t d, int32_t h, int32_t w, int32_t n_class,
                      int32_t foreground_only, int32_t mode, int32_t connectivity, const double* sampling, double* table,
                      void* workspace, size_t workspace_bytes, ctl_stream stream);
size_t ctl_surface_quantiles_ws_bytes(int32_t d, int32_t h, int32_t w, int32_t n_class, int32_t foreground_only, int32_t mode,
                                      int32_t n_q);
int ctl_surface_quantiles(const uint8_t* pred, const int64_t* gt, int32_t d, int32_t h, int32_t w, int32_t n_class,
                          int32_t foreground_only, int32_t mode, int32_t connectivity, const double* sampling, const double* q,
                          int32_t n_q, double* stats_table, double* q_table, void* workspace, size_t workspace_bytes,
                          ctl_stream stream);
size_t ctl_surface_map_ws_bytes(int32_t d, int32_t h, int32_t w, int32_t mode);
int ctl_surface_map(const uint8_t* mask, int32_t d, int32_t h, int32_t w, int32_t mode, int32_t connectivity,
                    const double* sampling, double* d2_out, uint8_t* surface_out, void* workspace, size_t workspace_bytes,
                    ctl_stream stream);

/* ------------------------------------------------------------------------------------------------ connected components
 * Largest-connected-component post-processing of a predicted label volume (medseg/common_utils/post_process.py:5-22,
 * `keep_largest_connected_components`, which upstream runs on the host with skimage.measure.label per class), and the labelling under it.
 *   labelmap  uint8 [D,H,W] (as written by ctl_argmax_c).  A component is a maximal connected set of voxels that carry the SAME class c,
 *             1 <= c < n_class (2..255); voxels of class 0 and voxels whose value is >= n_class belong to no component.
 *   mode      2: every [H,W] slice on its own;  3: the volume (the numbering of ctl_surface_stats).
 *   connectivity  1..mode, as scipy.ndimage.generate_binary_structure(mode, connectivity): neighbours at L1 offset <= connectivity
 *             (1 = the 4- / 6-neighbourhood, what upstream uses).
 * ctl_cc_label: labels (int32 [D,H,W]) = for a voxel of a component the smallest C-order linear index (within the volume in mode 3,
 *   within its slice in mode 2) of any voxel of that component, -1 elsewhere.  The numbering is canonical: it does not depend on the
 *   launch geometry or on the order of the merges.  3 launches; `labels` itself is the union-find parent array, no workspace.
 * ctl_cc_keep_largest: out (uint8 [D,H,W], may alias labelmap) = labelmap with every voxel set to 0 that is not in the largest
 *   component of its class (per slice in mode 2).  Largest = most voxels; among components of equal size the one whose first voxel in C
 *   order comes first (np.argmax over components numbered in scan order).  table (int64 [groups][n_class - 1][3], may be NULL;
 *   groups = D in mode 2, 1 in mode 3) = {number of components, voxels of the kept one, its label (-1: the class is absent)}.  5 launches.
 * The sequence of launches is fixed (no loop "until nothing changes", no readback), whatever the volume holds; only integer atomics
 * (min / max / add) are used, so every result is the same bits on every call.  Labels are 32-bit: D * H * W must be below 2^31.
 * The workspace is caller-owned, sized by ctl_cc_ws_bytes (0 for arguments the call itself would refuse), 256-byte aligned. */
size_t ctl_cc_ws_bytes(int32_t d, int32_t h, int32_t w, int32_t n_class, int32_t mode);
int ctl_cc_label(const uint8_t* labelmap, int32_t d, int32_t h, int32_t w, int32_t n_class, int32_t mode, int32_t connectivity,
                 int32_t* labels, ctl_stream stream);
int ctl_cc_keep_largest(const uint8_t* labelmap, int32_t d, int32_t h, int32_t w, int32_t n_class, int32_t mode, int32_t connectivity,
                        uint8_t* out, int64_t* table, void* workspace, size_t workspace_bytes, ctl_stream stream);

/* ------------------------------------------------------------------------------------------------ predictive uncertainty
 * Entropy maps (medseg/common_utils/uncertainty.py:7-54) and the sums behind ECE / NLL / Brier (medseg/models/custom_loss.py:495-511 is the
 * Brier double sum) of logits the device already holds, for an ensemble of T members (ctl_uncert.hip).
 *   logits  fp32 NHWC [T][n][hw][C], member-major: member t of slice b is row t * n + b.  1 <= T <= CTL_UNCERT_MAX_MEMBERS, 1 <= C <= 16.
 *           is_prob != 0: the rows already are probabilities (what upstream's entropy functions take) and the softmax is skipped.
 *   label   int64 [n][hw] or NULL.  A label outside 0..C-1 (and every pixel when label is NULL) is unlabelled: it gets its maps and enters
 *           none of the labelled sums, the rule of the losses above.
 * Per pixel, in fp32:  p_t = softmax(x_t) with a true division (uniform logits give exactly float(1) / float(C));
 *   pbar = (sum_t p_t) / float(T);  conf = max_k pbar_k;  yhat = argmax_k pbar_k, a tie -> the lowest index (ctl_argmax_c);
 *   H  = -sum_k pbar_k log2(pbar_k + eps)                    predictive entropy, in BITS (upstream's form has eps = 1e-7; a term whose
 *                                                            pbar_k + eps is 0 contributes 0, so eps = 0 is allowed)
 *   E  = (1/T) sum_t -sum_k p_tk log2(p_tk + eps)            expected entropy
 *   MI = H - E                                               mutual information; exactly 0 for T = 1
 *   labelled pixels (label y):  nll = -ln pbar_y, formed as a log-sum-exp over the members of x_ty - max_k x_tk - ln sum_k exp(..), so a
 *   class 160 logits below the maximum still has a finite nll (is_prob: from ln p_ty; +inf where every member gives 0);
 *   brier = sum_k (pbar_k - [k == y])^2;  correct = [yhat == y].
 * Reliability bins: B equal-width bins, 1 <= B <= CTL_UNCERT_MAX_BINS.  The bin of a labelled pixel is the number of edges
 *   e_j = float(j) / float(B), j = 1..B-1, with conf > e_j, an fp32 comparison against the fp32 edge: every conf has exactly one bin.
 * Outputs, each may be NULL:
 *   entropy, mi, conf   fp32 [n][hw]        pred  uint8 [n][hw] (yhat)        mean_prob  fp32 NHWC [n][hw][C] (pbar)
 *   stats   double [n][6] per slice: labelled pixels, correct pixels, sum H over ALL pixels, sum MI over all pixels, sum nll, sum brier
 *   bins    int64 [n][B][3] per slice and bin: labelled pixels, correct pixels, sum of conf * 2^32.  The last is an exact integer (an fp32
 *           conf >= 2^-8 is a multiple of 2^-31, and conf >= 1/16 up to rounding), so the sum does not depend on the order of the adds
 *           and cannot overflow below 2^31 pixels per slice.
 *   ECE = sum_b (n_b / N) |correct_b / n_b - (sum conf)_b / n_b| over the non-empty bins is finished on the host in fp64 from `bins`.
 * Two launches: a streaming pass, grid (blocks of a slice, slice), that reads every pixel once, keeps a block's bins in LDS (integer LDS
 * atomics) and writes one row of fp64 sums and one of bin sums per block to the workspace; and one finalize block per slice that adds
 * the rows in a fixed order (skipped when stats and bins are both NULL).  No float atomics, no global atomics, nothing read back, no
 * argument that changes from call to call: the same bits on every call and in a graph replay.  Rows of C == 4 in 16-byte aligned
 * tensors move as 16 bytes; any other case takes the runtime-count kernel, same arithmetic in the same order, same bits.
 * workspace: ctl_predictive_stats_ws_bytes(T, n, hw, C, B) bytes, 8-byte aligned, caller-owned.
 * A NULL logits or workspace pointer, T, C or B out of range, non-positive sizes, more than 65535 slices, a tensor at or past 2 GiB and
 * an eps that is not finite and >= 0 are refused with CTL_EINVAL before any launch; ctl_predictive_stats_ws_bytes returns 0 for them. */
#define CTL_UNCERT_MAX_MEMBERS 64
#define CTL_UNCERT_MAX_BINS 64
size_t ctl_predictive_stats_ws_bytes(int32_t T, int32_t n, int64_t hw, int32_t C, int32_t B);
int ctl_predictive_stats(const float* logits, const int64_t* label, int32_t T, int32_t n, int64_t hw, int32_t C, int32_t B, float eps,
                         int32_t is_prob, float* entropy, float* mi, float* conf, uint8_t* pred, float* mean_prob, double* stats,
                         int64_t* bins, void* workspace, ctl_stream stream);

/* ------------------------------------------------------------------------------------------------ test-time augmentation
 * Predict several flipped / rotated views of a batch of slices, put the logits back on the native grid and average them (ctl_tta.hip).  A
 * project addition: upstream has no counterpart.
 * A view is an element of the dihedral group of the square, coded v = 0..7: bit 0 = transpose, bit 1 = flip along H, bit 2 = flip
 * along W, applied in that order.  For a plane X [H][W]: A = X^T if bit 0 else X, (Ho, Wo) = the shape of A, and
 *   view_v(X)[y][x] = A[bit1 ? Ho-1-y : y][bit2 ? Wo-1-x : x].
 * Native pixel (i, j) is found in view v at (y, x): (a, b) = bit0 ? (j, i) : (i, j), y = bit1 ? Ho-1-a : a, x = bit2 ? Wo-1-b : b.
 * codes: T distinct view codes (HOST array, read during the call: launch constants), 1 <= T <= CTL_TTA_MAX_VIEWS; the identity need
 * not be among them.  A code with bit 0 needs h == w.
 * ctl_tta_views: x fp32 NHWC [n][h][w][c], 1 <= c <= 4 -> out fp32 [T][n][Ho][Wo][c], member-major: member t is view codes[t] of every
 *   slice.  A pure permutation.
 * ctl_tta_merge: logits fp32 NHWC [T][n][Ho][Wo][c], the network's output on those views, 1 <= c <= 16; (h, w) is the NATIVE grid.
 *   Outputs, each may be NULL, at least one is not:
 *   aligned  fp32 [T][n][h][w][c]   every member on the native grid: a pure permutation, what ctl_predictive_stats reads with T members
 *   merged   fp32 [n][h][w][c]      mode CTL_TTA_LOGIT: (((x_0 + x_1) + ..) + x_T-1) / float(T) in fp32, in member order, plain adds and one
 *                                   true division;  mode CTL_TTA_PROB: pbar of "predictive uncertainty" above with the same arithmetic
 *                                   in the same order (per member: subtract the maximum, expf, sum, divide; T-1 adds; divide by float(T))
 *   pred     uint8 [n][h][w]        arg-max of merged, a tie -> the lowest index (ctl_argmax_c)
 *   An output that is not asked for changes no bit of the others.
 * One launch each over square pixel tiles (32 x 32 up to 4 channels, else 16 x 16); a pixel is c contiguous floats and moves as 16
 * bytes when c == 4 and every tensor is 16-byte aligned (the same bits either way).  A view without a transpose is read along its rows,
 * forwards or backwards; a transposed one goes through a padded LDS tile so that neither side of the copy is strided by a row per lane.
 * No workspace, no atomics, nothing read back, no argument that changes from call to call: the same bits on every call and in a graph
 * replay.  Refused with CTL_EINVAL before any launch: T outside 1..8, a code outside 0..7, a duplicate code, c out of range, non-positive
 * sizes, a transposing code with h != w, a tensor at or past 2 GiB, a NULL x / out / logits / codes, all three outputs NULL, an unknown
 * mode. */
#define CTL_TTA_MAX_VIEWS 8
#define CTL_TTA_LOGIT 0
#define CTL_TTA_PROB 1
int ctl_tta_views(const float* x, int32_t n, int32_t h, int32_t w, int32_t c, const int32_t* codes, int32_t T, float* out, ctl_stream stream);
int ctl_tta_merge(const float* logits, int32_t T, int32_t n, int32_t h, int32_t w, int32_t c, const int32_t* codes, int32_t mode,
                  float* aligned, float* merged, uint8_t* pred, ctl_stream stream);

/* ------------------------------------------------------------------------------------------------ training augmentation
 * The per-slice host chain of medseg/dataset_loader/transform.py:46-86 (flip, contrast / brightness, random affine, choice rotation,
 * elastic deformation, centre crop) for a whole batch that is already on the device: image float [n,1,Hp,Wp] and label int64 [n,Hp,Wp]
 * -> image_out float [n,1,Hc,Wc] and label_out int64 [n,Hc,Wc].  Every array is resampled ONCE (upstream resamples up to three times).
 * The min-max normalisation that ends the chain (MyNormalizeMedicPercentile with percentiles (0, 100), transform.py:83-84) is
 * ctl_rescale_intensity on image_out.
 *   source    output pixel (y, x) is p = (y + cy, x + cx) on the padded grid, cy = ceil((Hp - Hc) / 2), cx = ceil((Wp - Wc) / 2)
 *             (MySpecialCrop, _utils/affine_transform.py:280-283).  Its source coordinate is s = M (p + d(p) - c) + c with
 *             c = ((Hp - 1) / 2, (Wp - 1) / 2), d = the sample's elastic displacement (rows, cols; zero without a field) and M = the
 *             sample's 2x3 output -> input matrix in (row, col) order: s_r = m[0] q_r + m[1] q_c + m[2] + c_r, s_c = m[3] q_r + m[4] q_c +
 *             m[5] + c_c for q = p + d - c.  The host composes M = F A Rc from the flips (MyRandomFlip, affine_transform.py:200-244), the
 *             random affine A = R(theta) T(ty, tx) Sh(phi) Z(zy, zx) (ts.RandomAffine, transform.py:70-73) and the choice rotation
 *             (MyRandomChoiceRotate, affine_transform.py:750-804): upstream's flip -> affine -> rotate -> elastic chain as one map.
 *             Coordinates are fp32.
 *   image     bilinear over the four taps around s; a tap outside the array contributes 0 (scipy.ndimage.map_coordinates(order=1,
 *             mode='grid-constant', cval=0)).  Every tap first goes through clamp(v * scale + brightness, mn, mx) with intensity[b] =
 *             {scale, brightness} and mn / mx = the minimum / maximum of the sample's whole padded input plane
 *             (RandomBrightnessFluctuation with preserve_range, _utils/intensity_transform.py:136-162, which upstream applies pointwise
 *             before any geometry: the same function).  {1, 0} switches it off.  The taps are combined in fp64 and rounded once.
 *   label     nearest neighbour: the tap at floor(s + 0.5) per axis, 0 outside the array.  (Upstream's per-class cubic spline and
 *             threshold, _utils/elastic_transform.py:84-92, is what ctl_aug_warp_cubic below offers.)
 *   field     float [n,2,Hp,Wp], d of sample b = (field[b][0], field[b][1]); NULL = no elastic deformation for the whole batch.
 * ctl_aug_field: field[b][axis] = alpha[b] * G_sigma[b](u[b][axis]) (MyElasticTransform.gen_deformation_field, elastic_transform.py:41-58,
 *   with alpha / sigma drawn as in :72-75).  G_sigma = scipy.ndimage.gaussian_filter(mode='constant', cval=0, truncate=4.0): separable,
 *   radius int(4 sigma + 0.5) (clamped to 1024 = twice the largest side), weights normalised over the whole radius in fp64, fp32
 *   accumulation; sigma <= 0 is the identity.  u is uniform in [-1, 1): noise (float [n,2,Hp,Wp]) when given, as ctl_noise_clamp takes
 *   one, else 2^-23 * (h >> 40) - 1 for the counter hash h of (seeds[b], b * 2 + axis, y * Wp + x) (the splitmix64 finaliser of
 *   ctl_noise_clamp / ctl_dropout2d).  alpha, sigma: device float [n]; seeds: device uint64 [n] (may be NULL with noise).  A sample with
 *   alpha == 0 gets zeros without filtering.  2 launches: rows from an LDS-staged row, columns from an LDS-staged 16-column tile.
 * ctl_aug_warp: the gather above, 2 launches: per-plane min / max partials (the scheme of ctl_rescale_intensity), then one pass over the
 *   crop window that writes image_out and label_out together.
 * Hp, Wp <= 512 (the LDS staging of the field passes), Hc <= Hp, Wc <= Wp, n <= 65535.  The launch counts do not depend on n; there is no
 * host synchronisation and no atomic: two calls give the same bits.  Workspaces are caller-owned, 256-byte aligned and sized by
 * ctl_aug_ws_bytes for ctl_aug_field (the row-filtered planes) and by ctl_aug_warp_ws_bytes for ctl_aug_warp (the min / max partials);
 * both return 0 for arguments the call would refuse.  No written array (field, image_out, label_out, a workspace) may overlap another
 * array of the same call.
 *
 * Cubic-spline resampling (an option: ctl_aug_warp above is unchanged).  Source coordinates, crop window, field and the closing rescale are
 * as above; only how a value is read at s changes.
 *   coefficients  of a plane v [Hp,Wp]: C(v) = scipy.ndimage.spline_filter(v, order=3, mode='reflect'), the separable inverse of the cubic
 *             B-spline under the half-sample symmetric extension d c b a | a b c d | d c b a, for any plane length (a line shorter than
 *             the filter's reach is folded as often as it takes).  Per axis the one-pole recursion with z = sqrt(3) - 2 is the two-sided
 *             sequence h[k] = (-6 z / (1 - z^2)) z^|k| = sqrt(3) z^|k| over the extended line; it is applied for |k| <= 40 (the dropped
 *             tail is below 1e-23 of the sum), rows then columns, accumulated in fp64, each stage stored as fp32.  A line of fewer than
 *             16 samples is where scipy itself leaves that inverse (its causal initialisation is off by about |z|^(2 len): 4e-7 at 5
 *             samples, below 1e-17 from 16 on); such a line is filtered by scipy's own recursion, so the result is scipy's at any length.
 *   value at s  if -0.5 <= s_r <= Hp - 0.5 and -0.5 <= s_c <= Wp - 0.5: the 4x4 cubic B-spline sum over C(v) at the taps floor(s) - 1 ..
 *             floor(s) + 2 per axis with reflected tap indices = scipy.ndimage.map_coordinates(v, s, order=3, mode='reflect'); the 16 taps
 *             are combined in fp64 and rounded once.  Otherwise 0: a border pulled into view is zero, as above.
 *   image     v = clamp(x * scale + brightness, mn, mx), the intensity map above, applied pointwise (in fp64) to the padded plane before
 *             the prefilter.
 *   label     each indicator plane 1[label == k], k in [0, n_class), is resampled like the image; the output is the largest k whose value
 *             is >= 0.5, and 0 if there is none or s is outside (upstream's ascending result[res_new >= 0.5] = c,
 *             _utils/elastic_transform.py:84-92).  n_class <= 16 as for ctl_confusion_hist; a label outside [0, n_class) belongs to no
 *             class.  The indicator planes are formed while a row is staged and never written.
 * ctl_aug_spline_coeffs: coeffs float [n, 1 + n_class, Hp, Wp] = C of the image plane (plane 0) and of the n_class indicator planes;
 *   n_class may be 0 (label may then be NULL).  3 launches: min / max partials, rows from an LDS-staged reflected row, columns from an
 *   LDS-staged reflected 16-column tile.  Workspace: ctl_aug_spline_ws_bytes (the partials and the row-filtered planes).
 * ctl_aug_warp_cubic: ctl_aug_warp's arguments plus n_class (1..16), 4 launches: the three above into the workspace, then one pass over
 *   the crop window that writes image_out and label_out together, the tap weights formed once per pixel for all 1 + n_class planes.
 *   Workspace: ctl_aug_warp_cubic_ws_bytes (the partials, the row-filtered planes and the coefficients).
 * Limits, determinism, alignment and the overlap rule are those above; both size queries return 0 for arguments the call would refuse.
 *
 * Bias field and coarse-grid displacement: the two stages of transform.py:46-86 that BatchAugmenter.from_config adds to the chain above.
 * Both take their per-sample parameters as a float record that the host fills (augment.bias_record / augment.coarse_record).
 * ctl_aug_bias: MyRandomPurtarbationV2 (_utils/intensity_transform.py:373-546; the constructor pins the control-point spacing to 64, :404)
 *   as a pre-pass image float [n,1,Hp,Wp] -> out of the same shape, which the warp then reads.  Upstream fits
 *   RectBivariateSpline(x, x, z, s=3) through z = 1 + U(-m, m) on x = arange(-xmax, xmax + 1, 64), xmax = (Hp + 96) // 2, evaluates it on
 *   arange(-xmax, xmax)^2 (an argument beyond the last data point is clamped by FITPACK), multiplies by h w / (sum + 1e-12) and keeps the
 *   centre Hp x Wp window: pixel (y, x) sits at the argument (y - Hp / 2, x - Wp / 2).  The fit and the sum are the host's (the sum from
 *   separability, in fp64); the record bias float [n,192] of sample b holds
 *     [0] on (0 = the sample is copied through)   [1] knots along the rows   [2] knots along the columns (8..16 each)
 *     [3] scale = h w / (sum + 1e-12)   [4] m   [5] eps (0 = no noise)   [6..7] unused
 *     [8..23] row knots   [24..39] column knots   [40..183] B-spline coefficients, entry (i, j) at 40 + 12 i + j   [184..191] unused
 *   Launch 1, per pixel: the span of each axis and its four non-zero cubic basis values (FITPACK's fpbspl; the argument clamped to
 *   [t[3], t[nt - 4]]), S = the 4x4 sum, v = image * clamp(scale * S, 1 - m, 1 + m), all in fp64 from the fp32 record and rounded once,
 *   written to the workspace with per-plane {min v, max v, sum of the input} partials (64 blocks per plane, the scheme of ctl_aug_warp /
 *   ctl_rescale_intensity, as doubles).  Launch 2: the partials reduced in a fixed order, out = (v - min) / (max - min + 1e-8), and with
 *   eps > 0 out = clamp(out + eps * N, 0, 1), in fp64 and rounded once; N = noise (float [n,1,Hp,Wp]) when given, else the standard normal
 *   sqrt(-2 ln u1) cos(2 pi u2) in fp64 with u1 = 2^-24 ((h >> 40) + 1), u2 = 2^-24 ((h >> 8) & 0xFFFFFF) for the counter hash h of
 *   (seeds[b], b, y * Wp + x) (the hash and the uniforms of ctl_noise_clamp, keyed like ctl_aug_field).  A sample that is off and a plane
 *   with |sum of the input| <= 1e-6 (upstream's black image, :436) are copied bit for bit.  Hp == Wp, even, 128..512 (upstream's own
 *   assertions, :439 and :448).  Workspace: ctl_aug_bias_ws_bytes (v and the partials).
 * ctl_aug_coarse_field: MyElasticTransformCoarseGrid.gen_deformation_field (_utils/elastic_transform.py:105-172): two 3x3 planes of N(0, 10)
 *   pixels resized to Hp x Wp = scipy.ndimage.zoom(m, (Hp / 3, Wp / 3), order=3, mode='mirror', grid_mode=True) clipped to [min m, max m]
 *   (what skimage.transform.resize(order=3, mode='reflect') documents from 0.19 on): the cubic B-spline sum over
 *   spline_filter(m, order=3, mode='mirror') at ((r + 0.5) 3 / Hp - 0.5, (c + 0.5) 3 / Wp - 0.5) with the tap indices mirrored about the
 *   first and last sample (c b | a b c | b a).  The record coarse float [n,24] of sample b holds [0..8] the coefficients of the row
 *   displacement, [9..17] of the column displacement, [18..21] {min, max} of either plane, [22] on, [23] unused.  1 launch: weights and
 *   sum in fp64, clipped, rounded once into field float [n,2,Hp,Wp] (the field argument of ctl_aug_warp); zeros for a sample that is off.
 *   Any Hp, Wp <= 512; no workspace. */
size_t ctl_aug_ws_bytes(int32_t n, int32_t hp, int32_t wp);
size_t ctl_aug_warp_ws_bytes(int32_t n, int32_t hp, int32_t wp, int32_t hc, int32_t wc);
int ctl_aug_field(const float* noise, const uint64_t* seeds, const float* alpha, const float* sigma, int32_t n, int32_t hp, int32_t wp,
                  float* field, void* workspace, size_t workspace_bytes, ctl_stream stream);
int ctl_aug_warp(const float* image, const int64_t* label, const float* matrix, const float* intensity, const float* field, int32_t n,
                 int32_t hp, int32_t wp, int32_t hc, int32_t wc, float* image_out, int64_t* label_out, void* workspace,
                 size_t workspace_bytes, ctl_stream stream);
size_t ctl_aug_spline_ws_bytes(int32_t n, int32_t hp, int32_t wp, int32_t n_class);
size_t ctl_aug_warp_cubic_ws_bytes(int32_t n, int32_t hp, int32_t wp, int32_t hc, int32_t wc, int32_t n_class);
int ctl_aug_spline_coeffs(const float* image, const int64_t* label, const float* intensity, int32_t n, int32_t hp, int32_t wp,
                          int32_t n_class, float* coeffs, void* workspace, size_t workspace_bytes, ctl_stream stream);
int ctl_aug_warp_cubic(const float* image, const int64_t* label, const float* matrix, const float* intensity, const float* field, int32_t n,
                       int32_t hp, int32_t wp, int32_t hc, int32_t wc, int32_t n_class, float* image_out, int64_t* label_out,
                       void* workspace, size_t workspace_bytes, ctl_stream stream);
size_t ctl_aug_bias_ws_bytes(int32_t n, int32_t hp, int32_t wp);
int ctl_aug_bias(const float* image, const float* bias, const float* noise, const uint64_t* seeds, int32_t n, int32_t hp, int32_t wp,
                 float* out, void* workspace, size_t workspace_bytes, ctl_stream stream);
int ctl_aug_coarse_field(const float* coarse, int32_t n, int32_t hp, int32_t wp, float* field, ctl_stream stream);

/* ------------------------------------------------------------------------------------------------ volume preparation
 * The per-volume host work of `load_img_label_from_path` (medseg/common_utils/basic_operations.py:337-365), which upstream runs once per
 * patient in testing (cardiac_ACDC_dataset.py:204-232) and once per slice sample in training (:117-161): resample the in-plane spacing
 * (`resample_by_spacing`, medseg/dataset_loader/dataset_utils.py:39-63), then np.percentile 2 / 98, clip, scale (`normalize_minmax_data`,
 * dataset_utils.py:15-36); and the per-slice form with arbitrary percentiles, `MyNormalizeMedicPercentile`
 * (medseg/dataset_loader/_utils/intensity_transform.py:216-269).
 * ctl_order_stats: x = `segments` contiguous segments of `seg_elems` floats (1 = the whole volume, slices = per slice).  ranks = HOST array
 *   of n_rank (1..8) zero-based ranks in [0, seg_elems), duplicates and any order allowed, read during the call.  out (float
 *   [segments][n_rank]) = the element of that rank in the segment's ascending order.  Exact: a radix select over the order-preserving key
 *   bits ^ (sign ? 0xFFFFFFFF : 0x80000000), most significant digit first, four 8-bit passes with per-block LDS histograms (equal digits
 *   of a wave are counted together first) and integer atomics only, so every call gives the same bits.  -0.0 sorts before +0.0.  Inputs
 *   must be finite: with a NaN in a segment the elements returned for it are unspecified, and this is NOT checked on the device.
 *   5 launches whatever the sizes and the content, no readback, no synchronisation: the call can be captured in a graph.  The workspace
 *   is caller-owned, needs no initialisation, 4-byte alignment and ctl_order_stats_ws_bytes(segments, n_rank) bytes (0 for counts the call
 *   would refuse); at most 65535 segments.
 * ctl_percentile_apply: one launch over x with the table [segments][4] of ctl_order_stats for the ranks {k_lo, k_lo + 1, k_hi, k_hi + 1}
 *   (the upper ranks clamped to seg_elems - 1).  For q in percent the HOST computes v = (seg_elems - 1) * (q / 100) in fp64, k = floor(v),
 *   g = v - k, and passes g_lo, g_hi by value.  The device forms each percentile as numpy's _lerp does, in fp64 without fused multiply-
 *   add: d = B - A, A + d * g when g < 0.5, else B - d * (1 - g), and rounds it once to float32 (lo, hi).  Then, in float32 with one
 *   rounding per operation and no contraction:
 *     form 0 "minmax" (dataset_utils.py:29-34):           x < lo -> lo, x > hi -> hi, out = (x - lo) / ((1e-10f + hi) - lo)
 *     form 1 "medic"  (intensity_transform.py:260-266):   x <= lo -> lo, x >= hi -> hi, a = (new_max - new_min) / ((hi - lo) + 1e-8f),
 *                                                          b = new_max - a * hi, out = x * a + b (multiply, then add)
 *   bounds (float [segments][2], may be NULL) receives lo, hi.  out must not overlap x; out == NULL with bounds: only lo, hi are written.
 * ctl_resample_inplane: [n,h,w] -> [n,new_h,new_w], the slice axis is never resampled (keep_z_spacing, the only form the datasets use).
 *   image (float) and / or label (label_bytes 1 = uint8, 8 = int64), one launch each; new_h, new_w and the ratios r = new_spacing /
 *   old_spacing of the height and width axes come from the host (fp64).  Output index j reads source coordinate c = j * r, one fp64
 *   multiply.  Image: linear in fp64 over the two neighbours per axis, row pairs first (v0 * (1 - t) + v1 * t), indices clamped to
 *   [0, size - 1], rounded once to float32.  Label: the element at floor(c + 0.5).  Both are 0 where c >= size - 0.5 on either axis
 *   (ITK's inside-buffer rule and default pixel).  SimpleITK itself maps through physical points, which can differ from j * r in the
 *   last bit of c; this statement is the contract.
 * Every tensor obeys the 32-bit byte-offset limit (below 2 GiB). */
size_t ctl_order_stats_ws_bytes(int32_t segments, int32_t n_rank);
int ctl_order_stats(const float* x, int32_t segments, int64_t seg_elems, const int64_t* ranks, int32_t n_rank, float* out,
                    void* workspace, size_t workspace_bytes, ctl_stream stream);
int ctl_percentile_apply(const float* x, const float* table, int32_t segments, int64_t seg_elems, double g_lo, double g_hi,
                         int32_t form, float new_min, float new_max, float* out, float* bounds, ctl_stream stream);
int ctl_resample_inplane(const float* image, const void* label, int32_t label_bytes, int32_t n, int32_t h, int32_t w, int32_t new_h,
                         int32_t new_w, double r_h, double r_w, float* image_out, void* label_out, ctl_stream stream);

/* ------------------------------------------------------------------------------------------------ native-grid restoration
 * The inverse of the forward trip ctl_resample_inplane -> ctl_crop_or_pad: a prediction made on the network window is put back on the
 * patient's native [n,h,w] grid.  Upstream has no counterpart (it scores on the prepared grid).  The geometry is passed as scalars:
 *   h, w            native size                       res_h, res_w   size after the forward resampling (== h, w without one)
 *   win_h, win_w    network window                    off_y, off_x   floor((res - win) / 2), negative when the window was padded (the
 *   q_h, q_w        native spacing / new spacing                     number ctl_crop_or_pad uses)
 *                   (fp64, from the host; exactly 1 when nothing was resampled)
 * Per axis: native index i has resampled-grid coordinate c = i * q, ONE fp64 multiply that is never contracted into what follows (the
 * corner-aligned convention of ctl_resample_inplane), and window coordinate u = c - off.  The voxel is INSIDE iff on both axes
 * c < res - 0.5 and -0.5 <= u < win - 0.5 (half a voxel beyond the last sample centre, as the forward statement).
 * ctl_restore_scores: scores float [n][win_h][win_w][c] (NHWC, what `predict` returns), 1 <= c <= 16.  Tap value s of a window pixel:
 *   mode 0 "logit" the score as fp64; mode 1 "prob" exp(x_k - max_j x_j) / sum_j exp(x_j - max_j x_j) of that pixel in fp64 (sum in
 *   ascending j).  Taps per axis: f = floor(u), t = u - f, i0 = clamp(f, 0, win - 1), i1 = clamp(f + 1, 0, win - 1), clamped SEPARATELY
 *   (u in [-0.5, 0) reads pixel 0 twice).  Per class, in fp64, every operation rounded on its own, in the order of ctl_resample_inplane:
 *   top = s00 (1 - tx) + s01 tx, bot = s10 (1 - tx) + s11 tx, v = top (1 - ty) + bot ty.  label (uint8 [n][h][w]) = the lowest class
 *   index with maximal v, decided on the fp64 values by a strict > scan as ctl_argmax_c does.  soft (float [n][c][h][w], plain contiguous
 *   planes, may be NULL) = v rounded once.  Outside voxels: label 0; soft all 0 in mode 0, (1, 0, ..., 0) in mode 1.  With q == 1 on both
 *   axes t is exactly 0, so inside the window mode 0 returns the bits of ctl_argmax_c and of the scores.  One launch, no workspace, no
 *   atomics, no readback; for c == 4 and a 16-byte aligned `scores` a tap is one 16-byte load.
 * ctl_restore_labels: labels uint8 [n][win_h][win_w] -> out uint8 [n][h][w]: the element at clamp(floor(u + 0.5), 0, win - 1) per axis
 *   for inside voxels, 0 outside.  One launch.
 * Every element of every output is written.  Null pointers, non-positive sizes, c outside 1..16, a non-finite or non-positive q, an
 * unknown mode and a tensor at or past the 2 GiB limit are refused with CTL_EINVAL before any launch. */
int ctl_restore_scores(const float* scores, int32_t n, int32_t c, int32_t win_h, int32_t win_w, int32_t h, int32_t w, int32_t res_h,
                       int32_t res_w, int32_t off_y, int32_t off_x, double q_h, double q_w, int32_t mode, uint8_t* label, float* soft,
                       ctl_stream stream);
int ctl_restore_labels(const uint8_t* labels, int32_t n, int32_t win_h, int32_t win_w, int32_t h, int32_t w, int32_t res_h, int32_t res_w,
                       int32_t off_y, int32_t off_x, double q_h, double q_w, uint8_t* out, ctl_stream stream);

/* ------------------------------------------------------------------------------------------------ MR artefact corruption (ACDC-C)
 * The four corruptions of medseg/dataset_loader/generate_artefacted_data.py:56-83 (TorchIO's RandomBiasField, RandomSpike, RandomGhosting,
 * RandomMotion) for one volume x [d][h][w] of floats, axes 0, 1, 2; N = d h w.  The host draws the random parameters and passes them by
 * value or as small HOST arrays read during the call; nothing is read back, every call is a fixed launch sequence that can be captured
 * in a graph, there are no floating-point atomics and every sum has a fixed order: identical bits on every call.  `out` never overlaps an
 * input.  Every tensor obeys the 32-bit byte-offset limit (below 2 GiB).
 * ctl_corrupt_bias: out = x * expf(p), p = sum of coefficients[n] u^i v^j w^k over i + j + k <= 3 in the loop order i, j, k (20 HOST floats),
 *   in float32.  The coordinate of index t on an axis of size n is (t - h + 0.5) / (h - 0.5) with h = n / 2 (integer), 0 where h == 0.
 *   One launch.
 * ctl_corrupt_spike: out = x + (1 / N) sum_s mult[s] ((A - Re X[k_s]) cos th_s + Im X[k_s] sin th_s), the image-space form of setting the
 *   spectrum entries k_s and -k_s to A = intensity * sum(x): X[k] = sum_r x[r] exp(-i th), th = 2 pi sum_a k_a r_a / size_a.  k: HOST int32
 *   [n_spikes][3] with 0 <= k_a < size_a, mult: HOST int32 [n_spikes] = 1 where k == -k (mod size) on every axis, else 2 (checked); the
 *   caller lists each pair {k, -k} once, 1..CTL_CORRUPT_MAX_SPIKES pairs.  (k_a r_a) mod size_a is reduced in integers, everything else
 *   is fp64, the result is rounded once.  Two launches: a reduction into the workspace (per-block partials summed in block order), then
 *   one element-wise pass.  The workspace is caller-owned, needs no initialisation, 8-byte alignment and
 *   ctl_corrupt_spike_ws_bytes(d, h, w, n_spikes) = min(ceil(N / 2048), CTL_CORRUPT_RED_BLOCKS) * (1 + 2 n_spikes) * 8 bytes (0 for
 *   arguments the call would refuse).
 * ctl_corrupt_rigid3d: out [copies][d][h][w]; copy t at voxel p = (i0, i1, i2) is the volume, extended by zeros, interpolated linearly at
 *   s_a = fma(m[4a+2], i2, fma(m[4a+1], i1, fma(m[4a], i0, m[4a+3]))) in float32, m = matrices[t] (HOST float [copies][12], row-major 3 x 4,
 *   voxel space; the host composes rotation about the physical centre, spacing and translation in fp64).  Along each axis
 *   v0 + f (v1 - v0), last axis first: an identity matrix returns x bit for bit.  1..CTL_CORRUPT_MAX_COPIES copies, one launch.
 * ctl_axis_operator: out[r][j] = sum over v < n_volumes, k < L of matrix[j][v L + k] * volume_v[r][k] along `axis` (0, 1 or 2; L = its
 *   size; r = the other two indices), terms added in ascending (v, k) with one float32 fused multiply-add each.  Volume 0 is x0, volumes
 *   1.. are stacked in xs ([n_volumes - 1][d][h][w], NULL for one volume); matrix: DEVICE float [L][n_volumes L], row-major.  A spectrum
 *   mask along one axis, real part of the inverse transform, is such a matrix (ghosting: one volume; motion: the original and its
 *   rigid copies).  LDS-tiled, strided for axes 0 and 1: nothing is transposed in memory.  One launch. */
#define CTL_CORRUPT_MAX_SPIKES 8
#define CTL_CORRUPT_MAX_COPIES 8
#define CTL_CORRUPT_RED_BLOCKS 256
int ctl_corrupt_bias(const float* x, const float* coefficients, int32_t d, int32_t h, int32_t w, float* out, ctl_stream stream);
size_t ctl_corrupt_spike_ws_bytes(int32_t d, int32_t h, int32_t w, int32_t n_spikes);
int ctl_corrupt_spike(const float* x, int32_t d, int32_t h, int32_t w, const int32_t* k, const int32_t* mult, int32_t n_spikes,
                      double intensity, float* out, void* workspace, size_t workspace_bytes, ctl_stream stream);
int ctl_corrupt_rigid3d(const float* x, int32_t d, int32_t h, int32_t w, const float* matrices, int32_t copies, float* out,
                        ctl_stream stream);
int ctl_axis_operator(const float* x0, const float* xs, int32_t n_volumes, int32_t d, int32_t h, int32_t w, int32_t axis,
                      const float* matrix, float* out, ctl_stream stream);

/* ------------------------------------------------------------------------------------------------ device-resident training set
 * What upstream's per-slice Dataset does on the host before the augmentation chain, for a batch picked by an index list:
 * formulate_labels (medseg/dataset_loader/base_segmentation_dataset.py:190-202), PadNumpy (transform.py:46-97 builds the chain; the pad
 * itself is torchsample's, defined here as: an axis shorter than the target gets ceil(d / 2) zeros in front and floor(d / 2) behind, a
 * longer one is left alone) and the origin_image / origin_label pair of keep_orig_image_label_pair (base_segmentation_dataset.py:149-186),
 * plus the "slice without objects" test of cardiac_ACDC_dataset.py:141-149.
 * The training volumes are packed slice after slice into two arenas with the same element layout: `image` float32 and `label` uint8,
 * arena_elems elements each.  table: DEVICE int64 [n_slices][3] = (element offset, h, w) of every slice; 64-bit offsets, an arena may
 * pass 2^31 elements.
 * ctl_slice_foreground: counts[s] = number of non-zero RAW label bytes of slice s (int32).  One launch over all slices, integer adds in
 *   a fixed order: identical on every call.
 * ctl_batch_gather: for b < n, slice s = index[b] (DEVICE int32 [n], read on the device: a captured launch replays with refreshed
 *   indices) is placed on the canvas: image_out [n][1][H][W] float32 (a copy, bit for bit) and label_out [n][H][W] int64 =
 *   lut[raw label] (lut: DEVICE uint8 [256], formulate_labels; values without an entry hold 0).  Placement per axis is upstream's
 *   crop_or_pad rule: a slice axis of size a on a target of size A starts at target index ceil((A - a) / 2) when a < A, and is read from
 *   source index (a - A) / 2 (floor) when a > A; everything else is 0 (the padding is 0 whatever lut[0] is: upstream pads after the
 *   remap).  With orig_image / orig_label (both or neither) the same launch also places the RAW slice and its remapped label on
 *   [n][1][Hc][Wc] / [n][Hc][Wc] by the same rule: upstream's origin pair for crop size (Hc, Wc).  Every element of every output is
 *   written.  Outputs are dense, 4-byte (float) / 8-byte (int64) aligned and may sit at any such address, e.g. the second half of a
 *   [2 n] batch tensor; rows are stored as 16-byte vectors wherever the address allows.  The range of a device-side index is the
 *   caller's contract; as a guard, an index outside [0, n_slices) or a table row that leaves the arena yields an all-zero sample, never
 *   a read outside the arenas.  1 <= n <= 65535, 1 <= H, W, Hc, Wc <= 32768.  One launch, no atomics, no readback. */
int ctl_slice_foreground(const uint8_t* label, const int64_t* table, int32_t n_slices, int64_t arena_elems, int32_t* counts,
                         ctl_stream stream);
int ctl_batch_gather(const float* image, const uint8_t* label, const int64_t* table, int32_t n_slices, int64_t arena_elems,
                     const int32_t* index, int32_t n, const uint8_t* lut, int32_t H, int32_t W, float* image_out, int64_t* label_out,
                     int32_t Hc, int32_t Wc, float* orig_image, int64_t* orig_label, ctl_stream stream);

/* ------------------------------------------------------------------------------------------------ optimizer
 * torch.optim.Adam defaults (model.py:774-785), one flat buffer: p,g,m,v [count].  step = 1-based step index.
 * grad_scale folds the 1/world_size of the data-parallel all-reduce. */
int ctl_adam(float* p, const float* g, float* m, float* v, int64_t count, float lr, float beta1, float beta2,
             float eps, int32_t step, float grad_scale, ctl_stream stream);
/* dst[i] += srcs[0][i] + ... + srcs[k-1][i] in that order (1 <= k <= 8; `srcs` is a HOST array of device pointers): the flat parameter
 * gradients that the passes of one network produced in a step, added into the network's gradient buffer by ONE launch after
 * loss.backward() instead of one autograd accumulation per pass (which, with two launch chains, is a cross-stream dependency each). */
int ctl_accumulate(float* dst, const float* const* srcs, int32_t k, int64_t count, ctl_stream stream);
/* same update with the step count read from state[2] on the device (bias corrections computed in double there) */
int ctl_adam_dev(float* p, const float* g, float* m, float* v, int64_t count, float lr, float beta1, float beta2,
                 float eps, const int64_t* state, float grad_scale, ctl_stream stream);

/* ------------------------------------------------------------------------------------------------ optimizer tail
 * Learning-rate schedules, global-norm clipping, a guard against a non-finite gradient and the EMA shadow of the weights, folded into
 * the pass that already streams p, g, m, v once per step (upstream: ExponentialMovingAverage, medseg/models/model_util.py:21-101,
 * get_scheduler 621-671; torch.nn.utils.clip_grad_norm_).  Opt-in: ctl_adam / ctl_adam_dev above are untouched.
 *
 * Control record: `double ctrl[CTL_OPTIM_CTRL_DOUBLES]` on the device, one per solver, for up to CTL_OPTIM_MAX_NETS networks.  fp32
 * values are stored as the double of the fp32 value, so reading one back as float is exact.
 *   host-written (ctl_optim_control)          device-written (ctl_grad_norm)
 *   [CTL_OPTIM_LR + j]   lr of network j      [CTL_OPTIM_SUMSQ]    sum of g^2 over all buffers (fp64)
 *   [CTL_OPTIM_MAX_NORM] 0 = no clipping      [CTL_OPTIM_NORM]     grad_scale * sqrt(sumsq)
 *   [CTL_OPTIM_GUARD]    1 = skip a step      [CTL_OPTIM_CLIP]     factor on every gradient, 1 = none (also reset by ctl_optim_control)
 *                        whose norm is not    [CTL_OPTIM_FINITE]   1 = the norm is finite (also reset to 1 by ctl_optim_control)
 *                        finite               [CTL_OPTIM_SKIPPED]  running count of skipped steps; never reset by the library
 *   [CTL_OPTIM_EMA_OMD]  1 - decay of this step
 * Every other word is reserved and never written.  The caller zeroes the record once.
 *
 * ctl_optim_control: ONE launch; the values travel as launch arguments (`lr` is a HOST array of k floats), so the host may run any
 *   number of steps ahead of the device.  Writes the host fields (lr of networks >= k: 0), clip = 1 and finite = 1; leaves the rest.
 * ctl_grad_norm_work: doubles of workspace ctl_grad_norm needs for these counts (a HOST array): sum_j ceil(counts[j] / CTL_GRAD_NORM_CHUNK);
 *   0 for a bad argument.
 * ctl_grad_norm: two launches for all k flat gradient buffers (`grads`, `counts`: HOST arrays).  Pass 1: block b of buffer j sums g^2 in
 *   fp64 over the fixed chunk [b CH, (b + 1) CH) into work[j][b]; CH = CTL_GRAD_NORM_CHUNK is a compile-time constant, so the grouping
 *   of the sum depends on the counts alone, not on the grid or the alignment.  Pass 2: one wave adds the partials in a fixed order and
 *   writes sumsq, norm = grad_scale * sqrt(sumsq), finite = isfinite(norm),
 *   clip = (max_norm > 0 && finite) ? min(1, max_norm / (norm + 1e-6)) : 1 (fp64), skipped += (guard && !finite).
 *   No atomics, no readback; the same bits on every call and in a graph replay.
 * ctl_adam_tail: one launch per network.  Guard on and finite == 0: returns without writing.  Otherwise gi = (g * grad_scale) * clip
 *   (clip == 1 changes no bit), then ctl_adam's arithmetic with lr = (float)ctrl[CTL_OPTIM_LR + net]; bias corrections from state[2]
 *   as ctl_adam_dev when `state` is given, else from `step` as ctl_adam.  `ema` (nullable): s <- s - omd * (s - p_new) as three
 *   separately rounded fp32 operations.  Reads p, g, m, v, s and writes p, m, v, s: 36 bytes per parameter. */
#define CTL_OPTIM_CTRL_DOUBLES 32
#define CTL_OPTIM_MAX_NETS 8
#define CTL_OPTIM_LR 0
#define CTL_OPTIM_MAX_NORM 8
#define CTL_OPTIM_GUARD 9
#define CTL_OPTIM_EMA_OMD 10
#define CTL_OPTIM_SUMSQ 16
#define CTL_OPTIM_NORM 17
#define CTL_OPTIM_CLIP 18
#define CTL_OPTIM_FINITE 19
#define CTL_OPTIM_SKIPPED 20
#define CTL_GRAD_NORM_CHUNK 16384
int ctl_optim_control(double* ctrl, int32_t k, const float* lr, float max_norm, int32_t skip_nonfinite, float ema_omd, ctl_stream stream);
size_t ctl_grad_norm_work(const int64_t* counts, int32_t k);
int ctl_grad_norm(const float* const* grads, const int64_t* counts, int32_t k, float grad_scale, double* work, double* ctrl,
                  ctl_stream stream);
int ctl_adam_tail(float* p, const float* g, float* m, float* v, float* ema, int64_t count, float beta1, float beta2, float eps,
                  const int64_t* state, int32_t step, float grad_scale, const double* ctrl, int32_t net, ctl_stream stream);

/* ------------------------------------------------------------------------------------------------ plans
 * A plan is an array of ctl_op executed in order on one stream: one C call per network pass (the Python host builds
 * it once per (network, shape, mode)).  Tensor arguments are (slot, byte offset) pairs resolved against `bases`.
 *
 * Plan record layout: where ctl_plan_run reads each operand of a record, one line per kind.  `KIND -> entry`: the fields are handed to
 * that entry under these, its parameter names (a `groups` word of 0 is passed as 1).  Banks: `i:` int32 words i[0], i[1], ... in order,
 * `k=name` = word i[k], `conv` = a ctl_conv in i[0..23]; `l:` l[0..]; `f:` f[0..]; `t:` tensor slots slot[0] / off[0], ... (slot -1 =
 * NULL).  What a line does not name is not read to run the record (the in-process profiler also looks at i[25] and slot[6] of any
 * non-conv record).  The binding keeps the same table (_ffi.OP_LAYOUT; tests/test_plan_layout_cpu.py compares them).
 *   CONV -> ctl_conv_forward_ex | i: conv | t: x wpack bias pro_scale pro_shift res res_scale res_shift y stats_partial res2 x2 pool xout
 *   WGRAD -> ctl_conv_wgrad_ex | i: conv 24=group_splits | t: x pro_scale pro_shift dy w_partial b_partial dy2 dy_coef
 *   WGRAD_GROUP | i: members
 *   WGRAD_REDUCE -> ctl_wgrad_reduce | i: conv 24=accumulate | l: s_co s_ci s_kh s_kw | t: w_partial b_partial dw dbias
 *   PACK -> ctl_pack_weights | i: cout cin ks flip | l: s_co s_ci s_kh s_kw | t: src dst
 *   BN_FINALIZE -> ctl_bn_finalize_ex | i: blocks c update_running groups | l: count | f: eps momentum | t: partial gamma beta running_mean running_var num_batches_tracked scale shift save_mean save_invstd save_uvar
 *   BN_REPLAY -> ctl_bn_replay_running | i: n_rec | f: momentum | t: act buffers num_batches_tracked table
 *   BN_EVAL -> ctl_bn_eval_coeffs | i: c groups | f: eps | t: gamma beta running_mean running_var scale shift
 *   BN_ACT -> ctl_bn_act_dt | i: c groups 25=bf16_mask | l: pixels | f: slope | t: x scale shift y
 *   BWD_REDUCE -> ctl_bwd_reduce_dt | i: mode c groups 25=bf16_mask | l: pixels | f: slope | t: dy act_src bn_src scale shift partial ds
 *   BN_BWD_FINALIZE -> ctl_bn_bwd_finalize_ex | i: c accumulate groups blocks affine_groups | l: count | t: partial gamma save_mean save_invstd coef dgamma dbeta
 *   BWD_APPLY -> ctl_bwd_apply_dt | i: mode c groups 25=bf16_mask | l: pixels | f: slope | t: dy act_src bn_src scale shift coef ds dx
 *   CHAN_SUM_FINALIZE -> ctl_chan_sum_finalize | i: c accumulate | t: partial out
 *   SUMPOOL2 -> ctl_sumpool2_dt | i: n h w c accumulate 25=bf16_mask | t: dup dx
 *   SIGMOID_BWD -> ctl_sigmoid_bwd | l: count | t: dy y dx
 *   ZERO | l: nbytes | t: dst
 *   COPY | l: nbytes | t: src dst
 *   PACK_BATCH -> ctl_pack_weights_batched | i: n_rec form | l: max_total | t: params wpack table
 *   WGRAD_REDUCE_BATCH -> ctl_wgrad_reduce_batched | i: n_rec | l: max_blocks | t: scratch grad table
 *   DROPOUT2D -> ctl_dropout2d_dt | i: n hw c 25=bf16_mask | l: seed_or_salt | f: p | t: z keep state out keep_out
 * Not parameters of the entry named: group_splits (0: a launch of its own; else the record is a member of the WGRAD_GROUP record in front
 * of it, with that many pixel splits), members (the next `members` records are WGRAD records served by one ctl_conv_wgrad_group launch),
 * form (bit 0: bf16 fragments, ctl_pack_weights_bf16_batched instead; bit 1: the table has CTL_PACK_X3 records, ctl_pack_weights_x3_batched
 * as well), and the ZERO / COPY fields (hipMemsetAsync of nbytes at dst / device-to-device hipMemcpyAsync of nbytes from src to dst). */
enum ctl_op_kind {
    CTL_OP_CONV = 1, CTL_OP_WGRAD = 2, CTL_OP_WGRAD_REDUCE = 3, CTL_OP_PACK = 4, CTL_OP_BN_FINALIZE = 5,
    CTL_OP_BN_EVAL = 6, CTL_OP_BN_ACT = 7, CTL_OP_BWD_REDUCE = 8, CTL_OP_BN_BWD_FINALIZE = 9, CTL_OP_BWD_APPLY = 10,
    CTL_OP_CHAN_SUM_FINALIZE = 11, CTL_OP_SUMPOOL2 = 12, CTL_OP_SIGMOID_BWD = 13, CTL_OP_ZERO = 14, CTL_OP_COPY = 15, CTL_OP_PACK_BATCH = 16,
    CTL_OP_WGRAD_REDUCE_BATCH = 17, CTL_OP_DROPOUT2D = 18, CTL_OP_BN_REPLAY = 19,
    CTL_OP_WGRAD_GROUP = 20           /* i[0] = n members (<= 8): the next n records are WGRAD records served by ONE launch (ctl_conv_wgrad_group), i[24] of each
                                         member = its pixel splits (ctl_wgrad_group_plan).  The members' partial buffers and reduction records are sized for
                                         THOSE split counts: a member record (i[24] != 0) must never be launched on its own -- ctl_plan_run refuses one that is
                                         not preceded by its GROUP record */
};
#define CTL_OP_MAX_T 14
typedef struct ctl_op {
    int32_t kind;
    int32_t i[27];                    /* per kind: the "plan record layout" table above.  CONV / WGRAD / WGRAD_REDUCE: i[0..23] = ctl_conv as
                                         int32 words; i[24] = the group's split count on a WGRAD record, accumulate on a WGRAD_REDUCE
                                         record; i[25] = bf16 storage mask of the element-wise ops */
    float   f[4];
    int32_t slot[CTL_OP_MAX_T];       /* -1 = NULL */
    int64_t off[CTL_OP_MAX_T];
    int64_t l[4];                     /* 64-bit scalars (strides, counts) */
} ctl_op;
int ctl_plan_run(const ctl_op* ops, int32_t n_ops, void* const* bases, int32_t n_bases, ctl_stream stream);

/* ------------------------------------------------------------------------------------------------ in-process profiling
 * Brackets every conv-family launch whose kernel id contains `filter` ("" = all) with hipEvents recorded on the launch
 * stream, and sums the ALGORITHMIC work of those launches: flops = 2*pixels*cout*cin*ks*ks (real channels), bytes =
 * input + output (+ residual / accumulate reads) tensors once each.  Kernel ids look like
 * "conv_igemm<ks3,s1,in0,mt4,tw32,nt1>" / "conv_wgrad<...>" (the template instantiation rocprofv3 reports).
 * ctl_prof_stop synchronises the recorded events and writes one text line per kernel id:
 *   "<id> launches=<n> ms=<total> flops=<sum> bytes=<sum>\n".  Not for use under graph capture. */
int ctl_prof_start(const char* filter);
/* the same, bracketing only every `every`-th matching launch (bench.py samples inside its timed region: two event records per launch
 * are not free on a launch-bound step) */
int ctl_prof_start_sampled(const char* filter, int32_t every);
int ctl_prof_stop(char* out, size_t cap);
/* launch census: kernels / stream memsets / copies enqueued by this library since it was loaded (bench.py reports launches per step) */
unsigned long long ctl_launch_count(void);
size_t ctl_sizeof_op(void);
size_t ctl_sizeof_conv(void);

#ifdef __cplusplus
}
#endif
#endif
