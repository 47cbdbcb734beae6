"""Shared by tests/test_form_ladder_gpu.py (MI355X) and tests/test_form_ladder_cpu.py (no GPU): the ladder of shapes at which the
conv / weight-gradient launches of a compiled plan change their kernel form, and the measured-tolerance comparison against fp64.

FORM CENSUS.  `census(fn)` runs fn between _ffi.prof_start("") and _ffi.prof_stop() and returns the profiling ids whose kind begins
`conv_` (ctl_prof_begin, csrc/ctl_plan.cpp: kind<ks,stride,in_mode,mt,tw,nt[,eN][,x2][,coN]>, one id per kernel instantiation family;
kinds: conv_igemm = fp32 pipe, conv_igemm_x3 / conv_igemm_x3pc = X3 single-role / producer-consumer form, conv_wgrad / conv_wgrad_x3 /
conv_wgrad_x3pc, conv_wgrad_x3grp<class> = a grouped launch).  mt,tw = 4,32 / 2,16 / 1,16 are the 8x32 / 8x16 / 4x16 pixel tiles.

LADDER.  Per network, (n, h, w) inputs sorted by pixel count.  Each training rung is the smallest shape found (candidates: n in 1..32 at
64^2 .. 256^2, the odd and non-square shapes below; census of every candidate on the MI355X) whose forward + backward takes a form no
smaller rung of that network takes; RUNG_NEW lists those ids, and test_rung_takes_its_forms compares them with what the library does
today.  blocks(tile) = n * ceil(h/th) * ceil(w/tw) * (cout tiles / nt) * nsub is the figure ctl_conv_pick_cfg thresholds (8x32 while
512 <= blocks, and <= 768 when nt = 2; else 8x16 while blocks >= 384; else 4x16); conv3_pick_cfg moves cin >= 64, nt = 2 layers to the
producer / consumer form on the largest tile that gives all 256 CUs a block, if the shares are equal and the steps suffice.

  image_encoder (1 channel) and shape_encoder (4 channels): layers 16ch @ h, 32ch @ h/2, 64ch @ h/4, 128ch @ h/8 and h/16
    3 x  40 x  56   everything on 4x16; 40->20->10->5->3: the s2d phase data gradient (ks2,s1) at the even levels AND the zero-insert
                    form (ks3,s1,in2) at 5x7 -> 3x4; PC 4x16 on the 128ch layers; grouped wgrad (x2 class)
    1 x 128 x 128   (image_encoder) grouped wgrad without the two-tensor gradient (class in0); 128->128 @ 8x8 is ONE 8x16 tile:
                    ctl_wgrad_splits == 1
    1 x 256 x 256   16ch @ 256^2: blocks(8x32) = 256 < 512, blocks(8x16) = 512 >= 384 -> 8x16, nt 1 (BASELINE config 4)
    2 x 256 x 256   16ch @ 256^2: blocks(8x32) = 512 -> 8x32, nt 1
    3 x 256 x 256   32ch @ 128^2: blocks(8x32) = 192, blocks(8x16) = 3*16*8 = 384 exactly -> 8x16 nt 2; stride-2 16->16: 8x16
    4 x 256 x 256   64ch @ 64^2: 4*8*4 = 128 8x16 tiles x 2 cout pairs = 256 blocks = every CU -> PC 8x16
    8 x 256 x 256   32ch @ 128^2: blocks(8x32) = 8*16*4 = 512 <= 768 -> 8x32 with two cout tiles (bs16: 1024 > 768 rejects it);
                    64ch @ 64^2: PC 8x32; 128ch @ 32^2: PC 8x16; 16ch @ 256^2: 2048 8x32 tiles on a persistent grid of <= 1024
    10 x 192 x 192  (training at the inference shape) 64ch @ 48^2: 180 8x16 tiles over 128 blocks are unequal shares, the gate of
                    conv3_pick_cfg leaves the PC form; blocks(8x16) = 360 < 384 -> single-role 4x16 nt 2 with the two-tensor prologue
    12 x 256 x 256  (image_encoder) 32ch @ 128^2: 768 < blocks(8x32) -> back to 8x16 nt 2 with the two-tensor prologue
    16 x 256 x 256  (image_encoder, the workload's own shape) 128ch @ 32^2: 16*4*1 = 64 8x32 tiles x 4 cout pairs = 256 blocks:
                    PC 8x32 with the two-tensor prologue needs the full batch by the "every CU a block" rule
  segmentation_decoder / shape_decoder (NN up-sampling; latent 128 x h x w, output 4 x 16h x 16w), image_decoder (ConvTranspose)
    3 x 3 x 4, 3 x 4 x 3   everything on 4x16; ctl_conv_pool_ok == 0 on the tail 1x1 (sum-pool is a pass of its own)
    1 x 16 x 16     16ch @ 256^2 on 8x16: the tail 1x1 writes the 2x2 sum-pool (ctl_conv_pool_ok == 1)
    2 x 16 x 16     16ch @ 256^2 on 8x32
    3 x 16 x 16     (image_decoder) 32ch @ 128^2 8x16 nt 2
    8 x 16 x 16     (image_decoder) 32ch 8x32 nt 2, 64ch PC 8x16
    12 x 16 x 16    32ch @ 128^2: 8x16 nt 2 (above 768 blocks of 8x32)
    16 x 16 x 16    64ch @ 64^2 PC (seg / image decoder)
    32 x 16 x 16    (segmentation_decoder only: the step decodes two stacked batches of 16) 16->32 1x1 @ 64^2 and the 32ch phase
                    convs: blocks(8x32) = n*8*2*1 = 16 n >= 512 needs n = 32
  candidates that add no id and are no rung: 5 x 96 x 160 (16ch: 300 blocks of 8x32, 1200 of 8x16 -> the forms of 1 x 256 x 256),
  3 x 64 x 48 / 3 x 72 x 104 (the forms of 3 x 40 x 56), n = 2 .. 16 at 128^2, 32 x 64 x 64, 6 x 256 x 256, 32 x 256 x 256
  inference (forward, eval-mode BatchNorm): 10 x 192 x 192 (predict) and 40 x 192 x 192 (whole volume; the equal-shares gate of
  conv3_pick_cfg: 128ch @ 12^2 n40 leaves the PC form), decoders from the 12 x 12 latents

TOLERANCE.  For every tensor e_hip and e_cpu are errors against the fp64 oracle of the HIP result and of the SAME oracle in fp32 on the
CPU; the assertion is e_hip <= max(3 * e_cpu, floor) (factor 3: tests/test_golden_r2.py).  Metrics: relative L2 everywhere; for
outputs and buffers (continuous in the input) also max-abs / max|ref|; for gradients the 99.9th-percentile abs error / max|ref|
(LeakyReLU slope ties are unavoidable at these sizes and hit the fp32 CPU run alike).  floor = the largest e_cpu of the tensor class
over the whole ladder (FLOORS, measured on the MI355X host; MEASURED has the figures per rung).  The max-abs and percentile errors are
taken relative to max|ref| so that one floor serves tensors of every scale.

FINDINGS (every e_hip / e_cpu above 3 met while measuring; none is an error, no tensor is outside max(3 e_cpu, floor)).
  1. Slope ties.  Where a rung shows e_hip ~ 1e-3 against e_cpu ~ 1e-6 (shape_encoder 4x256x256, shape_decoder 1x16x16,
     segmentation_decoder 2x16x16, image_decoder 3x16x16 / 8x16x16, shape_encoder 3x256x256, image_encoder 16x256x256) the excess covers exactly the parameters upstream of one activation and
     none downstream of it (shape_encoder 4x256x256: down3.* and everything before it at 2e-3, down4.* / final_conv at 1e-6), the
     outputs and buffers of the same run agree to 2e-6, and the fp64 oracle has a pre-activation within fp32 rounding of zero in that
     very tensor (down3.last_act: -7.2e-7 where the fp32 CPU run itself is off by 1.6e-6; segmentation_decoder 2x16x16 up4.conv.2:
     -3.8e-9).  One (Leaky)ReLU slope taken on the other side moves the gradient of its cone by ~1/sqrt(elements) = 1e-3.  The fp32 CPU
     run does the same at other rungs (its sign flips against fp64 were counted: 1-3 per affected tensor), which is where the gradient
     floors come from, and at image_encoder 2x / 3x256x256 both runs take the same tie (ratio 1.0 at 8e-4).
  2. dbeta of the first BatchNorm of a block (*.conv.1.bias, code_decoupler.1.bias, final_conv.1.bias), ratio 3-9 at 3e-6 .. 1e-5:
     the sums ride in the data-gradient epilogue, one fp32 row per persistent block accumulated over all tiles of that block, rows
     added in double by bn_bwd_finalize_kernel; the CPU sums pairwise.  The figure grows with the tiles per block (3e-6 at n = 1,
     1e-5 at n = 16) and stays three orders below the ties.
  3. running_mean of one layer per network, ratio 3-4 at 2e-7: both sides within two ulp of the fp32 buffer."""
import math

import torch

NETS = ("image_encoder", "shape_encoder", "segmentation_decoder", "shape_decoder", "image_decoder")
IN_CH = {"image_encoder": 1, "shape_encoder": 4, "segmentation_decoder": 128, "shape_decoder": 128, "image_decoder": 128}

# training rungs (mode A on each; MODE_B_RUNG also in mode B)
LADDER = {
    "image_encoder": [(3, 40, 56), (1, 128, 128), (1, 256, 256), (2, 256, 256), (3, 256, 256), (4, 256, 256), (10, 192, 192), (8, 256, 256),
                      (12, 256, 256), (16, 256, 256)],
    "shape_encoder": [(3, 40, 56), (1, 256, 256), (2, 256, 256), (3, 256, 256), (4, 256, 256), (8, 256, 256)],
    "segmentation_decoder": [(3, 3, 4), (3, 4, 3), (1, 16, 16), (2, 16, 16), (12, 16, 16), (16, 16, 16), (32, 16, 16)],
    "shape_decoder": [(3, 3, 4), (3, 4, 3), (1, 16, 16), (2, 16, 16), (12, 16, 16)],
    "image_decoder": [(3, 3, 4), (1, 16, 16), (2, 16, 16), (3, 16, 16), (8, 16, 16), (12, 16, 16), (16, 16, 16)],
}
MODE_B_RUNG = {"image_encoder": (8, 256, 256), "shape_encoder": (8, 256, 256), "segmentation_decoder": (12, 16, 16),
               "shape_decoder": (12, 16, 16), "image_decoder": (8, 16, 16)}
# inference rungs: the networks `predict` runs (n_iter = 2 adds the shape pair)
EVAL_LADDER = {
    "image_encoder": [(10, 192, 192), (40, 192, 192)], "shape_encoder": [(10, 192, 192), (40, 192, 192)],
    "segmentation_decoder": [(10, 12, 12), (40, 12, 12)], "shape_decoder": [(10, 12, 12), (40, 12, 12)],
}

CLASSES = ("output", "dx", "conv_weight", "bias_affine", "buffer")
# the second metric of a class next to the relative L2 error
SECOND = {"output": "max", "buffer": "max", "dx": "q999", "conv_weight": "q999", "bias_affine": "q999"}
FACTOR = 3.0
# floor[class][metric] = the largest e_cpu of the class over every rung and mode of the ladder (measured, rounded up to three digits)
FLOORS = {
    "output": {"l2": 1.48e-06, "max": 1.79e-06},
    "dx": {"l2": 3.78e-03, "q999": 7.03e-03},
    "conv_weight": {"l2": 7.11e-03, "q999": 1.97e-02},
    "bias_affine": {"l2": 7.35e-03, "q999": 2.71e-02},
    "buffer": {"l2": 2.97e-07, "max": 6.09e-07},
}
# ids first reached at a rung, walking up the network's ladder (training rungs, then the inference rungs)
RUNG_NEW = {
    "image_encoder": {
        "train": {
            "3x40x56": ["conv_igemm<ks1,s1,in0,mt1,tw16,nt1,e1>", "conv_igemm<ks1,s1,in0,mt1,tw16,nt2,e1>", "conv_igemm<ks1,s1,in0,mt1,tw16,nt2,e2>", "conv_igemm<ks1,s1,in0,mt1,tw16,nt2>", "conv_igemm<ks3,s1,in0,mt1,tw16,nt1,x2,co1>", "conv_igemm<ks3,s1,in3,mt1,tw16,nt1>", "conv_igemm_x3<ks2,s1,in0,mt1,tw16,nt1,e1>", "conv_igemm_x3<ks2,s1,in0,mt1,tw16,nt2,e2>", "conv_igemm_x3<ks3,s1,in0,mt1,tw16,nt1,e3,x2>", "conv_igemm_x3<ks3,s1,in0,mt1,tw16,nt1,x2>", "conv_igemm_x3<ks3,s1,in0,mt1,tw16,nt1>", "conv_igemm_x3<ks3,s1,in0,mt1,tw16,nt2,e1>", "conv_igemm_x3<ks3,s1,in0,mt1,tw16,nt2,e3,x2>", "conv_igemm_x3<ks3,s1,in0,mt1,tw16,nt2>", "conv_igemm_x3<ks3,s1,in2,mt1,tw16,nt2,e2>", "conv_igemm_x3<ks3,s2,in0,mt1,tw16,nt1>", "conv_igemm_x3pc<ks3,s1,in0,mt1,tw16,nt2,e3,x2>", "conv_igemm_x3pc<ks3,s1,in0,mt1,tw16,nt2,x2>", "conv_igemm_x3pc<ks3,s1,in0,mt1,tw16,nt2>", "conv_wgrad<ks1,s1,in0,mt1,tw16,nt2>", "conv_wgrad<ks1,s1,in0,mt2,tw16,nt2>", "conv_wgrad<ks3,s1,in3,mt2,tw16,nt1,x2>", "conv_wgrad_x3<ks3,s1,in0,mt1,tw16,nt2,x2>", "conv_wgrad_x3<ks3,s1,in0,mt1,tw16,nt2>", "conv_wgrad_x3<ks3,s1,in0,mt2,tw16,nt1,x2>", "conv_wgrad_x3<ks3,s1,in0,mt2,tw16,nt2,x2>", "conv_wgrad_x3<ks3,s2,in0,mt1,tw16,nt2>", "conv_wgrad_x3<ks3,s2,in0,mt2,tw16,nt1>", "conv_wgrad_x3grp<in0,x2>"],
            "1x128x128": ["conv_wgrad_x3grp<in0>"],
            "1x256x256": ["conv_igemm<ks3,s1,in0,mt2,tw16,nt1,x2,co1>", "conv_igemm<ks3,s1,in3,mt2,tw16,nt1>", "conv_igemm_x3<ks2,s1,in0,mt2,tw16,nt1,e1>", "conv_igemm_x3<ks3,s1,in0,mt2,tw16,nt1,e3,x2>", "conv_igemm_x3<ks3,s1,in0,mt2,tw16,nt1>"],
            "2x256x256": ["conv_igemm<ks3,s1,in0,mt4,tw32,nt1,x2,co1>", "conv_igemm<ks3,s1,in3,mt4,tw32,nt1>", "conv_igemm_x3<ks2,s1,in0,mt4,tw32,nt1,e1>", "conv_igemm_x3<ks3,s1,in0,mt4,tw32,nt1,e3,x2>", "conv_igemm_x3<ks3,s1,in0,mt4,tw32,nt1>"],
            "3x256x256": ["conv_igemm<ks1,s1,in0,mt2,tw16,nt1,e1>", "conv_igemm<ks1,s1,in0,mt2,tw16,nt2,e1>", "conv_igemm_x3<ks2,s1,in0,mt2,tw16,nt2,e2>", "conv_igemm_x3<ks3,s1,in0,mt2,tw16,nt1,x2>", "conv_igemm_x3<ks3,s1,in0,mt2,tw16,nt2,e3,x2>", "conv_igemm_x3<ks3,s1,in0,mt2,tw16,nt2>", "conv_igemm_x3<ks3,s2,in0,mt2,tw16,nt1>"],
            "4x256x256": ["conv_igemm_x3pc<ks3,s1,in0,mt2,tw16,nt2,e3,x2>", "conv_igemm_x3pc<ks3,s1,in0,mt2,tw16,nt2>"],
            "10x192x192": ["conv_igemm_x3<ks3,s1,in0,mt1,tw16,nt2,x2>"],
            "8x256x256": ["conv_igemm<ks1,s1,in0,mt4,tw32,nt1,e1>", "conv_igemm<ks1,s1,in0,mt4,tw32,nt2,e1>", "conv_igemm_x3<ks2,s1,in0,mt4,tw32,nt2,e2>", "conv_igemm_x3<ks3,s1,in0,mt4,tw32,nt1,x2>", "conv_igemm_x3<ks3,s1,in0,mt4,tw32,nt2,e3,x2>", "conv_igemm_x3<ks3,s1,in0,mt4,tw32,nt2>", "conv_igemm_x3pc<ks3,s1,in0,mt2,tw16,nt2,x2>", "conv_igemm_x3pc<ks3,s1,in0,mt4,tw32,nt2,e3,x2>", "conv_igemm_x3pc<ks3,s1,in0,mt4,tw32,nt2>"],
            "12x256x256": ["conv_igemm_x3<ks3,s1,in0,mt2,tw16,nt2,x2>"],
            "16x256x256": ["conv_igemm_x3pc<ks3,s1,in0,mt4,tw32,nt2,x2>"],
        },
        "eval": {
            "10x192x192": [],
            "40x192x192": [],
        },
    },
    "shape_encoder": {
        "train": {
            "3x40x56": ["conv_igemm<ks1,s1,in0,mt1,tw16,nt1,e1>", "conv_igemm<ks1,s1,in0,mt1,tw16,nt2,e1>", "conv_igemm<ks1,s1,in0,mt1,tw16,nt2,e2>", "conv_igemm<ks1,s1,in0,mt1,tw16,nt2>", "conv_igemm<ks3,s1,in3,mt1,tw16,nt1>", "conv_igemm_x3<ks2,s1,in0,mt1,tw16,nt1,e1>", "conv_igemm_x3<ks2,s1,in0,mt1,tw16,nt2,e2>", "conv_igemm_x3<ks3,s1,in0,mt1,tw16,nt1,e3,x2>", "conv_igemm_x3<ks3,s1,in0,mt1,tw16,nt1,x2,co4>", "conv_igemm_x3<ks3,s1,in0,mt1,tw16,nt1,x2>", "conv_igemm_x3<ks3,s1,in0,mt1,tw16,nt1>", "conv_igemm_x3<ks3,s1,in0,mt1,tw16,nt2,e3,x2>", "conv_igemm_x3<ks3,s1,in0,mt1,tw16,nt2>", "conv_igemm_x3<ks3,s1,in2,mt1,tw16,nt2,e2>", "conv_igemm_x3<ks3,s2,in0,mt1,tw16,nt1>", "conv_igemm_x3pc<ks3,s1,in0,mt1,tw16,nt2,e3,x2>", "conv_igemm_x3pc<ks3,s1,in0,mt1,tw16,nt2,x2>", "conv_igemm_x3pc<ks3,s1,in0,mt1,tw16,nt2>", "conv_wgrad<ks1,s1,in0,mt1,tw16,nt2>", "conv_wgrad<ks1,s1,in0,mt2,tw16,nt2>", "conv_wgrad<ks3,s1,in3,mt2,tw16,nt1,x2>", "conv_wgrad_x3<ks3,s1,in0,mt1,tw16,nt2,x2>", "conv_wgrad_x3<ks3,s1,in0,mt2,tw16,nt1,x2>", "conv_wgrad_x3<ks3,s1,in0,mt2,tw16,nt2,x2>", "conv_wgrad_x3<ks3,s2,in0,mt1,tw16,nt2>", "conv_wgrad_x3<ks3,s2,in0,mt2,tw16,nt1>", "conv_wgrad_x3grp<in0,x2>"],
            "1x256x256": ["conv_igemm<ks3,s1,in3,mt2,tw16,nt1>", "conv_igemm_x3<ks2,s1,in0,mt2,tw16,nt1,e1>", "conv_igemm_x3<ks3,s1,in0,mt2,tw16,nt1,e3,x2>", "conv_igemm_x3<ks3,s1,in0,mt2,tw16,nt1,x2,co4>", "conv_igemm_x3<ks3,s1,in0,mt2,tw16,nt1>"],
            "2x256x256": ["conv_igemm<ks3,s1,in3,mt4,tw32,nt1>", "conv_igemm_x3<ks2,s1,in0,mt4,tw32,nt1,e1>", "conv_igemm_x3<ks3,s1,in0,mt4,tw32,nt1,e3,x2>", "conv_igemm_x3<ks3,s1,in0,mt4,tw32,nt1,x2,co4>", "conv_igemm_x3<ks3,s1,in0,mt4,tw32,nt1>"],
            "3x256x256": ["conv_igemm<ks1,s1,in0,mt2,tw16,nt1,e1>", "conv_igemm<ks1,s1,in0,mt2,tw16,nt2,e1>", "conv_igemm_x3<ks2,s1,in0,mt2,tw16,nt2,e2>", "conv_igemm_x3<ks3,s1,in0,mt2,tw16,nt1,x2>", "conv_igemm_x3<ks3,s1,in0,mt2,tw16,nt2,e3,x2>", "conv_igemm_x3<ks3,s1,in0,mt2,tw16,nt2>", "conv_igemm_x3<ks3,s2,in0,mt2,tw16,nt1>"],
            "4x256x256": ["conv_igemm_x3pc<ks3,s1,in0,mt2,tw16,nt2,e3,x2>", "conv_igemm_x3pc<ks3,s1,in0,mt2,tw16,nt2>"],
            "8x256x256": ["conv_igemm<ks1,s1,in0,mt4,tw32,nt1,e1>", "conv_igemm<ks1,s1,in0,mt4,tw32,nt2,e1>", "conv_igemm_x3<ks2,s1,in0,mt4,tw32,nt2,e2>", "conv_igemm_x3<ks3,s1,in0,mt4,tw32,nt1,x2>", "conv_igemm_x3<ks3,s1,in0,mt4,tw32,nt2,e3,x2>", "conv_igemm_x3<ks3,s1,in0,mt4,tw32,nt2>", "conv_igemm_x3pc<ks3,s1,in0,mt2,tw16,nt2,x2>", "conv_igemm_x3pc<ks3,s1,in0,mt4,tw32,nt2,e3,x2>", "conv_igemm_x3pc<ks3,s1,in0,mt4,tw32,nt2>"],
        },
        "eval": {
            "10x192x192": [],
            "40x192x192": [],
        },
    },
    "segmentation_decoder": {
        "train": {
            "3x3x4": ["conv_igemm<ks1,s1,in0,mt1,tw16,nt1,co4>", "conv_igemm<ks1,s1,in0,mt1,tw16,nt1,e2>", "conv_igemm<ks1,s1,in0,mt1,tw16,nt2,e1>", "conv_igemm<ks1,s1,in0,mt1,tw16,nt2,e2>", "conv_igemm<ks1,s1,in1,mt1,tw16,nt1,e1>", "conv_igemm<ks1,s1,in1,mt1,tw16,nt2,e1>", "conv_igemm_x3<ks2,s1,in0,mt1,tw16,nt1>", "conv_igemm_x3<ks2,s1,in0,mt1,tw16,nt2>", "conv_igemm_x3<ks3,s1,in0,mt1,tw16,nt1,e3,x2>", "conv_igemm_x3<ks3,s1,in0,mt1,tw16,nt1>", "conv_igemm_x3<ks3,s1,in0,mt1,tw16,nt2,e3,x2>", "conv_igemm_x3<ks3,s1,in0,mt1,tw16,nt2>", "conv_igemm_x3<ks4,s2,in0,mt1,tw16,nt1,x2>", "conv_igemm_x3pc<ks3,s1,in0,mt1,tw16,nt2,e3,x2>", "conv_igemm_x3pc<ks3,s1,in0,mt1,tw16,nt2>", "conv_wgrad<ks1,s1,in0,mt1,tw16,nt2>", "conv_wgrad<ks1,s1,in0,mt2,tw16,nt1,co4>", "conv_wgrad<ks1,s1,in0,mt2,tw16,nt1>", "conv_wgrad_x3<ks3,s1,in0,mt1,tw16,nt2,x2>", "conv_wgrad_x3<ks3,s1,in0,mt2,tw16,nt1,x2>", "conv_wgrad_x3<ks3,s1,in0,mt2,tw16,nt2,x2>", "conv_wgrad_x3<ks3,s1,in1,mt1,tw16,nt2,x2>", "conv_wgrad_x3<ks3,s1,in1,mt2,tw16,nt1,x2>", "conv_wgrad_x3<ks3,s1,in1,mt2,tw16,nt2,x2>"],
            "3x4x3": ["conv_wgrad<ks1,s1,in0,mt2,tw16,nt2>", "conv_wgrad_x3grp<in0,x2>", "conv_wgrad_x3grp<in1,x2>"],
            "1x16x16": ["conv_igemm<ks1,s1,in0,mt2,tw16,nt1,co4>", "conv_igemm<ks1,s1,in0,mt2,tw16,nt1,e2>", "conv_igemm<ks1,s1,in1,mt2,tw16,nt1,e1>", "conv_igemm_x3<ks2,s1,in0,mt2,tw16,nt1>", "conv_igemm_x3<ks3,s1,in0,mt2,tw16,nt1,e3,x2>", "conv_igemm_x3<ks3,s1,in0,mt2,tw16,nt1>"],
            "2x16x16": ["conv_igemm<ks1,s1,in0,mt4,tw32,nt1,co4>", "conv_igemm<ks1,s1,in0,mt4,tw32,nt1,e2>", "conv_igemm<ks1,s1,in1,mt4,tw32,nt1,e1>", "conv_igemm_x3<ks2,s1,in0,mt4,tw32,nt1>", "conv_igemm_x3<ks3,s1,in0,mt4,tw32,nt1,e3,x2>", "conv_igemm_x3<ks3,s1,in0,mt4,tw32,nt1>"],
            "12x16x16": ["conv_igemm<ks1,s1,in0,mt2,tw16,nt2,e2>", "conv_igemm<ks1,s1,in1,mt2,tw16,nt2,e1>", "conv_igemm_x3<ks2,s1,in0,mt2,tw16,nt2>", "conv_igemm_x3<ks3,s1,in0,mt2,tw16,nt2,e3,x2>", "conv_igemm_x3<ks3,s1,in0,mt2,tw16,nt2>"],
            "16x16x16": ["conv_igemm_x3pc<ks3,s1,in0,mt2,tw16,nt2,e3,x2>", "conv_igemm_x3pc<ks3,s1,in0,mt2,tw16,nt2>"],
            "32x16x16": ["conv_igemm<ks1,s1,in0,mt4,tw32,nt2,e2>", "conv_igemm<ks1,s1,in1,mt4,tw32,nt2,e1>", "conv_igemm_x3<ks2,s1,in0,mt4,tw32,nt2>", "conv_igemm_x3<ks3,s1,in0,mt4,tw32,nt2,e3,x2>", "conv_igemm_x3<ks3,s1,in0,mt4,tw32,nt2>", "conv_igemm_x3pc<ks3,s1,in0,mt4,tw32,nt2,e3,x2>", "conv_igemm_x3pc<ks3,s1,in0,mt4,tw32,nt2>"],
        },
        "eval": {
            "10x12x12": [],
            "40x12x12": [],
        },
    },
    "shape_decoder": {
        "train": {
            "3x3x4": ["conv_igemm<ks1,s1,in0,mt1,tw16,nt1,co4>", "conv_igemm<ks1,s1,in0,mt1,tw16,nt1,e2>", "conv_igemm<ks1,s1,in0,mt1,tw16,nt2,e1>", "conv_igemm<ks1,s1,in0,mt1,tw16,nt2,e2>", "conv_igemm<ks1,s1,in1,mt1,tw16,nt1,e1>", "conv_igemm<ks1,s1,in1,mt1,tw16,nt2,e1>", "conv_igemm_x3<ks2,s1,in0,mt1,tw16,nt1>", "conv_igemm_x3<ks2,s1,in0,mt1,tw16,nt2>", "conv_igemm_x3<ks3,s1,in0,mt1,tw16,nt1,e3,x2>", "conv_igemm_x3<ks3,s1,in0,mt1,tw16,nt1>", "conv_igemm_x3<ks3,s1,in0,mt1,tw16,nt2,e3,x2>", "conv_igemm_x3<ks3,s1,in0,mt1,tw16,nt2>", "conv_igemm_x3<ks4,s2,in0,mt1,tw16,nt1,x2>", "conv_igemm_x3pc<ks3,s1,in0,mt1,tw16,nt2,e3,x2>", "conv_igemm_x3pc<ks3,s1,in0,mt1,tw16,nt2>", "conv_wgrad<ks1,s1,in0,mt1,tw16,nt2>", "conv_wgrad<ks1,s1,in0,mt2,tw16,nt1,co4>", "conv_wgrad<ks1,s1,in0,mt2,tw16,nt1>", "conv_wgrad_x3<ks3,s1,in0,mt1,tw16,nt2,x2>", "conv_wgrad_x3<ks3,s1,in0,mt2,tw16,nt1,x2>", "conv_wgrad_x3<ks3,s1,in0,mt2,tw16,nt2,x2>", "conv_wgrad_x3<ks3,s1,in1,mt1,tw16,nt2,x2>", "conv_wgrad_x3<ks3,s1,in1,mt2,tw16,nt1,x2>", "conv_wgrad_x3<ks3,s1,in1,mt2,tw16,nt2,x2>"],
            "3x4x3": ["conv_wgrad<ks1,s1,in0,mt2,tw16,nt2>", "conv_wgrad_x3grp<in0,x2>", "conv_wgrad_x3grp<in1,x2>"],
            "1x16x16": ["conv_igemm<ks1,s1,in0,mt2,tw16,nt1,co4>", "conv_igemm<ks1,s1,in0,mt2,tw16,nt1,e2>", "conv_igemm<ks1,s1,in1,mt2,tw16,nt1,e1>", "conv_igemm_x3<ks2,s1,in0,mt2,tw16,nt1>", "conv_igemm_x3<ks3,s1,in0,mt2,tw16,nt1,e3,x2>", "conv_igemm_x3<ks3,s1,in0,mt2,tw16,nt1>"],
            "2x16x16": ["conv_igemm<ks1,s1,in0,mt4,tw32,nt1,co4>", "conv_igemm<ks1,s1,in0,mt4,tw32,nt1,e2>", "conv_igemm<ks1,s1,in1,mt4,tw32,nt1,e1>", "conv_igemm_x3<ks2,s1,in0,mt4,tw32,nt1>", "conv_igemm_x3<ks3,s1,in0,mt4,tw32,nt1,e3,x2>", "conv_igemm_x3<ks3,s1,in0,mt4,tw32,nt1>"],
            "12x16x16": ["conv_igemm<ks1,s1,in0,mt2,tw16,nt2,e2>", "conv_igemm<ks1,s1,in1,mt2,tw16,nt2,e1>", "conv_igemm_x3<ks2,s1,in0,mt2,tw16,nt2>", "conv_igemm_x3<ks3,s1,in0,mt2,tw16,nt2,e3,x2>", "conv_igemm_x3<ks3,s1,in0,mt2,tw16,nt2>"],
        },
        "eval": {
            "10x12x12": [],
            "40x12x12": [],
        },
    },
    "image_decoder": {
        "train": {
            "3x3x4": ["conv_igemm<ks1,s1,in0,mt1,tw16,nt1,co1>", "conv_igemm<ks1,s1,in0,mt1,tw16,nt1,e1>", "conv_igemm<ks1,s1,in0,mt1,tw16,nt1,e2>", "conv_igemm<ks1,s1,in0,mt1,tw16,nt1>", "conv_igemm<ks1,s1,in0,mt1,tw16,nt2,e1>", "conv_igemm<ks1,s1,in0,mt1,tw16,nt2>", "conv_igemm_x3<ks2,s2,in0,mt1,tw16,nt1,e2>", "conv_igemm_x3<ks2,s2,in0,mt1,tw16,nt2,e2>", "conv_igemm_x3<ks2,s2,in0,mt1,tw16,nt2>", "conv_igemm_x3<ks3,s1,in0,mt1,tw16,nt1,e3,x2>", "conv_igemm_x3<ks3,s1,in0,mt1,tw16,nt1,x2>", "conv_igemm_x3<ks3,s1,in0,mt1,tw16,nt1>", "conv_igemm_x3<ks3,s1,in0,mt1,tw16,nt2,e3,x2>", "conv_igemm_x3<ks3,s1,in0,mt1,tw16,nt2,x2>", "conv_igemm_x3<ks3,s1,in0,mt1,tw16,nt2>", "conv_igemm_x3pc<ks3,s1,in0,mt1,tw16,nt2,e3,x2>", "conv_igemm_x3pc<ks3,s1,in0,mt1,tw16,nt2,x2>", "conv_igemm_x3pc<ks3,s1,in0,mt1,tw16,nt2>", "conv_wgrad<ks1,s1,in0,mt1,tw16,nt2>", "conv_wgrad<ks1,s1,in0,mt2,tw16,nt1,co1>", "conv_wgrad<ks1,s1,in0,mt2,tw16,nt1>", "conv_wgrad<ks1,s1,in0,mt2,tw16,nt2>", "conv_wgrad_x3<ks2,s2,in0,mt1,tw16,nt2>", "conv_wgrad_x3<ks2,s2,in0,mt2,tw16,nt1>", "conv_wgrad_x3<ks2,s2,in0,mt2,tw16,nt2>", "conv_wgrad_x3<ks3,s1,in0,mt1,tw16,nt2,x2>", "conv_wgrad_x3<ks3,s1,in0,mt2,tw16,nt1,x2>", "conv_wgrad_x3grp<in0,x2>"],
            "1x16x16": ["conv_igemm<ks1,s1,in0,mt2,tw16,nt1,co1>", "conv_igemm<ks1,s1,in0,mt2,tw16,nt1,e1>", "conv_igemm<ks1,s1,in0,mt2,tw16,nt1,e2>", "conv_igemm<ks1,s1,in0,mt2,tw16,nt1>", "conv_igemm_x3<ks3,s1,in0,mt2,tw16,nt1,e3,x2>", "conv_igemm_x3<ks3,s1,in0,mt2,tw16,nt1,x2>", "conv_igemm_x3<ks3,s1,in0,mt2,tw16,nt1>"],
            "2x16x16": ["conv_igemm<ks1,s1,in0,mt4,tw32,nt1,co1>", "conv_igemm<ks1,s1,in0,mt4,tw32,nt1,e1>", "conv_igemm<ks1,s1,in0,mt4,tw32,nt1,e2>", "conv_igemm<ks1,s1,in0,mt4,tw32,nt1>", "conv_igemm_x3<ks3,s1,in0,mt4,tw32,nt1,e3,x2>", "conv_igemm_x3<ks3,s1,in0,mt4,tw32,nt1,x2>", "conv_igemm_x3<ks3,s1,in0,mt4,tw32,nt1>"],
            "3x16x16": ["conv_igemm<ks1,s1,in0,mt2,tw16,nt2,e1>", "conv_igemm<ks1,s1,in0,mt2,tw16,nt2>", "conv_igemm_x3<ks2,s2,in0,mt2,tw16,nt1,e2>", "conv_igemm_x3<ks3,s1,in0,mt2,tw16,nt2,x2>"],
            "8x16x16": ["conv_igemm<ks1,s1,in0,mt4,tw32,nt2,e1>", "conv_igemm<ks1,s1,in0,mt4,tw32,nt2>", "conv_igemm_x3<ks3,s1,in0,mt4,tw32,nt2,x2>", "conv_igemm_x3pc<ks3,s1,in0,mt2,tw16,nt2,x2>", "conv_igemm_x3pc<ks3,s1,in0,mt2,tw16,nt2>"],
            "12x16x16": ["conv_igemm_x3<ks2,s2,in0,mt2,tw16,nt2,e2>", "conv_igemm_x3<ks3,s1,in0,mt2,tw16,nt2,e3,x2>", "conv_igemm_x3<ks3,s1,in0,mt2,tw16,nt2>"],
            "16x16x16": ["conv_igemm_x3pc<ks3,s1,in0,mt2,tw16,nt2,e3,x2>", "conv_igemm_x3pc<ks3,s1,in0,mt4,tw32,nt2,x2>", "conv_igemm_x3pc<ks3,s1,in0,mt4,tw32,nt2>"],
        },
    },
}

# Measured on the MI355X host: per rung and tensor class, relative L2 error against fp64 -- the largest e_cpu, the largest e_hip and the
# largest e_hip / e_cpu of the class.  Reading it: see "FINDINGS" in the module docstring.
MEASURED = """
  network rung mode                     output             | dx                 | conv_weight        | bias_affine        | buffer            
  image_encoder 3x40x56 mode A          1e-6 2e-6    1.4 | 9e-7 1e-6    1.3 | 2e-6 2e-6    1.4 | 2e-6 2e-6    2.2 | 3e-7 4e-7    1.8
  image_encoder 1x128x128 mode A        1e-6 2e-6    1.3 | 9e-7 1e-6    1.3 | 3e-6 2e-6    1.4 | 2e-6 3e-6    2.3 | 2e-7 3e-7    1.9
  image_encoder 1x256x256 mode A        1e-6 2e-6    1.5 | 7e-7 1e-6    1.4 | 5e-6 2e-6    1.4 | 4e-6 4e-6    3.8 | 1e-7 2e-7    2.3
  image_encoder 2x256x256 mode A        1e-6 2e-6    1.4 | 8e-4 8e-4    1.0 | 8e-4 8e-4    1.6 | 1e-3 1e-3    4.7 | 1e-7 2e-7    2.3
  image_encoder 3x256x256 mode A        1e-6 2e-6    1.4 | 4e-4 4e-4    1.0 | 3e-4 3e-4    1.8 | 8e-4 8e-4    5.8 | 1e-7 2e-7    3.1
  image_encoder 4x256x256 mode A        1e-6 2e-6    1.4 | 2e-3 1e-6    0.0 | 2e-3 5e-6    1.5 | 3e-3 1e-5    5.9 | 1e-7 2e-7    2.3
  image_encoder 10x192x192 mode A       1e-6 2e-6    1.4 | 2e-4 3e-6    0.0 | 3e-4 7e-6    3.1 | 5e-4 1e-5    7.1 | 1e-7 2e-7    2.6
  image_encoder 8x256x256 mode A        1e-6 2e-6    1.4 | 5e-4 6e-4    1.2 | 6e-4 7e-4    1.2 | 9e-4 8e-4    7.0 | 1e-7 2e-7    2.7
  image_encoder 12x256x256 mode A       1e-6 2e-6    1.4 | 9e-4 7e-4    0.8 | 1e-3 8e-4    4.8 | 3e-3 1e-3    7.1 | 1e-7 2e-7    2.9
  image_encoder 16x256x256 mode A       1e-6 2e-6    1.4 | 7e-4 7e-4    1.1 | 8e-4 1e-3  129.0 | 2e-3 2e-3  184.9 | 9e-8 2e-7    3.0
  shape_encoder 3x40x56 mode A          1e-6 1e-6    1.2 | 8e-7 9e-7    1.1 | 2e-6 1e-6    1.3 | 1e-6 2e-6    1.7 | 2e-7 4e-7    1.8
  shape_encoder 1x256x256 mode A        1e-6 1e-6    1.3 | 4e-3 8e-7    0.0 | 4e-3 3e-6    1.4 | 5e-3 5e-6    4.2 | 1e-7 2e-7    2.2
  shape_encoder 2x256x256 mode A        1e-6 1e-6    1.3 | 8e-4 8e-4    1.0 | 7e-4 7e-4    1.7 | 9e-4 9e-4    5.2 | 1e-7 2e-7    1.9
  shape_encoder 3x256x256 mode A        1e-6 1e-6    1.3 | 1e-3 1e-3    1.0 | 3e-3 3e-3  212.3 | 7e-3 7e-3 2534.8 | 2e-7 2e-7    2.1
  shape_encoder 4x256x256 mode A        1e-6 1e-6    1.3 | 1e-3 2e-3    1.8 | 1e-3 2e-3 1823.4 | 3e-3 4e-3 3964.6 | 1e-7 2e-7    2.0
  shape_encoder 8x256x256 mode A        1e-6 1e-6    1.3 | 1e-3 7e-4    0.7 | 1e-3 6e-4    1.3 | 2e-3 1e-3    5.7 | 2e-7 2e-7    2.5
  segmentation_decoder 3x3x4 mode A     7e-7 8e-7    1.2 | 3e-3 3e-5    0.0 | 7e-3 4e-5    1.0 | 7e-3 4e-5    1.0 | 9e-8 1e-7    1.7
  segmentation_decoder 3x4x3 mode A     7e-7 8e-7    1.2 | 5e-7 7e-7    1.3 | 1e-6 1e-6    1.2 | 2e-6 2e-6    1.7 | 9e-8 1e-7    1.5
  segmentation_decoder 1x16x16 mode A   7e-7 8e-7    1.3 | 6e-4 7e-7    0.0 | 8e-4 2e-6    0.8 | 2e-3 5e-6    1.0 | 1e-7 9e-8    1.5
  segmentation_decoder 2x16x16 mode A   7e-7 8e-7    1.3 | 5e-7 3e-4  609.2 | 5e-6 5e-4  420.2 | 6e-6 1e-3  651.7 | 7e-8 9e-8    2.2
  segmentation_decoder 12x16x16 mode A  7e-7 8e-7    1.3 | 1e-3 9e-4    0.9 | 1e-3 1e-3    1.1 | 1e-3 2e-3    1.3 | 1e-7 1e-7    1.6
  segmentation_decoder 16x16x16 mode A  7e-7 8e-7    1.3 | 4e-4 7e-4    2.0 | 5e-4 8e-4    2.3 | 7e-4 2e-3    3.3 | 1e-7 1e-7    1.6
  segmentation_decoder 32x16x16 mode A  7e-7 8e-7    1.3 | 9e-4 7e-4    0.9 | 9e-4 9e-4    1.3 | 1e-3 1e-3    2.5 | 9e-8 1e-7    1.7
  shape_decoder 3x3x4 mode A            7e-7 9e-7    1.2 | 5e-7 7e-7    1.4 | 1e-6 1e-6    1.2 | 1e-6 2e-6    1.8 | 1e-7 2e-7    1.5
  shape_decoder 3x4x3 mode A            7e-7 8e-7    1.2 | 5e-7 6e-7    1.2 | 1e-6 1e-6    1.2 | 1e-6 2e-6    1.9 | 1e-7 1e-7    1.4
  shape_decoder 1x16x16 mode A          8e-7 1e-6    1.3 | 5e-7 1e-3 2339.1 | 2e-6 2e-3 1964.2 | 4e-6 4e-3 2554.8 | 1e-7 9e-8    1.6
  shape_decoder 2x16x16 mode A          7e-7 9e-7    1.3 | 9e-4 8e-4    0.9 | 1e-3 9e-4    1.0 | 1e-3 1e-3    1.0 | 2e-7 1e-7    1.4
  shape_decoder 12x16x16 mode A         7e-7 9e-7    1.3 | 9e-4 6e-4    0.6 | 1e-3 6e-4    1.4 | 1e-3 9e-4    1.6 | 9e-8 2e-7    2.2
  image_decoder 3x3x4 mode A            5e-7 7e-7    1.4 | 8e-7 1e-6    1.3 | 1e-6 2e-6    1.5 | 4e-6 3e-6    2.7 | 9e-8 2e-7    2.1
  image_decoder 1x16x16 mode A          5e-7 8e-7    1.4 | 2e-4 2e-4    1.0 | 2e-4 2e-4    1.1 | 3e-4 3e-4    1.0 | 8e-8 2e-7    2.9
  image_decoder 2x16x16 mode A          5e-7 8e-7    1.4 | 3e-4 2e-4    0.5 | 4e-4 2e-4    1.2 | 7e-4 2e-4    1.0 | 8e-8 2e-7    3.9
  image_decoder 3x16x16 mode A          5e-7 8e-7    1.4 | 1e-4 1e-3   10.1 | 2e-4 2e-3   11.6 | 2e-4 3e-3   17.6 | 6e-8 2e-7    3.9
  image_decoder 8x16x16 mode A          5e-7 8e-7    1.4 | 1e-3 1e-3    1.0 | 2e-3 1e-3   66.6 | 2e-3 3e-3  113.0 | 7e-8 2e-7    3.2
  image_decoder 12x16x16 mode A         5e-7 8e-7    1.4 | 1e-3 2e-3    1.9 | 1e-3 2e-3    2.6 | 2e-3 3e-3   10.6 | 7e-8 2e-7    3.9
  image_decoder 16x16x16 mode A         5e-7 8e-7    1.4 | 1e-3 2e-3    1.5 | 2e-3 2e-3    1.8 | 2e-3 3e-3    2.2 | 7e-8 2e-7    3.2
  image_encoder 8x256x256 mode B        1e-6 2e-6    1.4 | 5e-4 6e-4    1.2 | 6e-4 7e-4    1.2 | 6e-4 8e-4    1.5 | 0e+00 0e+00    0.0
  shape_encoder 8x256x256 mode B        1e-6 1e-6    1.3 | 1e-3 7e-4    0.7 | 1e-3 6e-4    1.3 | 5e-4 5e-4    1.3 | 0e+00 0e+00    0.0
  segmentation_decoder 12x16x16 mode B  7e-7 8e-7    1.3 | 1e-3 9e-4    0.9 | 1e-3 1e-3    1.1 | 1e-3 2e-3    1.2 | 0e+00 0e+00    0.0
  shape_decoder 12x16x16 mode B         7e-7 9e-7    1.3 | 9e-4 6e-4    0.6 | 1e-3 6e-4    1.4 | 1e-3 8e-4    0.9 | 0e+00 0e+00    0.0
  image_decoder 8x16x16 mode B          5e-7 8e-7    1.4 | 1e-3 1e-3    1.0 | 2e-3 1e-3   66.6 | 2e-3 3e-3   42.6 | 0e+00 0e+00    0.0
  image_encoder 10x192x192 eval         7e-7 1e-6    1.7 |                    |                    |                    |                   
  image_encoder 40x192x192 eval         7e-7 1e-6    1.7 |                    |                    |                    |                   
  shape_encoder 10x192x192 eval         8e-7 1e-6    1.4 |                    |                    |                    |                   
  shape_encoder 40x192x192 eval         8e-7 1e-6    1.4 |                    |                    |                    |                   
  segmentation_decoder 10x12x12 eval    7e-7 8e-7    1.1 |                    |                    |                    |                   
  segmentation_decoder 40x12x12 eval    7e-7 8e-7    1.1 |                    |                    |                    |                   
  shape_decoder 10x12x12 eval           8e-7 9e-7    1.2 |                    |                    |                    |                   
  shape_decoder 40x12x12 eval           8e-7 9e-7    1.2 |                    |                    |                    |                   
"""


def rung_id(rung):
    return "x".join(str(v) for v in rung)


def census(fn):
    """The set of conv / weight-gradient profiling ids launched by fn()."""
    from cooperative_training_and_latent_space_data_augmentation_amd import _ffi
    _ffi.prof_start("")
    try:
        fn()
        torch.cuda.synchronize()
    finally:
        rec = _ffi.prof_stop()
    return {k for k in rec if k.startswith("conv_")}


def rung_input(name, rung, seed=0):
    """Inputs as tests/test_engine_gpu.py draws them: U[0, 1) images / one-hot-like maps, relu(N(0, 1)) latents; and the generator the
    output gradients are drawn from afterwards."""
    n, h, w = rung
    g = torch.Generator().manual_seed(seed)
    x = torch.rand(n, IN_CH[name], h, w, generator=g)
    if "decoder" in name:
        x = torch.relu(torch.randn(n, IN_CH[name], h, w, generator=g))
    return x, g


def grad_class(ref):
    """conv / transposed-conv weights are 4-D, biases and the BatchNorm affine pair 1-D"""
    return "conv_weight" if ref.dim() == 4 else "bias_affine"


def errors(x, ref):
    """Errors of x against the fp64 tensor ref: relative L2, max-abs and 99.9th-percentile abs error, the last two over max|ref|."""
    x, ref = x.detach().cpu().double().flatten(), ref.detach().cpu().double().flatten()
    assert x.shape == ref.shape, (x.shape, ref.shape)
    d = (x - ref).abs()
    scale = max(float(ref.abs().max()), 1e-300)
    k = max(1, math.ceil(0.999 * d.numel()))
    return {"l2": float(d.norm()) / max(float(ref.norm()), 1e-300), "max": float(d.max()) / scale, "q999": float(d.kthvalue(k)[0]) / scale}


def judge(cls, what, hip, cpu, ref, figures=None):
    """e_hip <= max(3 * e_cpu, floor) on the two metrics of the class.  Returns the list of violations (strings); appends
    (what, class, metric, e_cpu, e_hip) to `figures` when given."""
    e_hip, e_cpu = errors(hip, ref), errors(cpu, ref)
    bad = []
    for m in ("l2", SECOND[cls]):
        if figures is not None:
            figures.append((what, cls, m, e_cpu[m], e_hip[m]))
        bound = max(FACTOR * e_cpu[m], FLOORS[cls][m])
        if not e_hip[m] <= bound:
            bad.append(f"{what} [{cls}, {m}]: HIP-vs-fp64 {e_hip[m]:.3e} > max(3 x fp32-CPU-vs-fp64 {e_cpu[m]:.3e}, floor {FLOORS[cls][m]:.3e})")
    return bad
