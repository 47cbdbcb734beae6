"""Fixtures shared by the native-grid restoration tests (tests/test_restore_*.py): the (shape, spacing, new_spacing, window) cases, their
scores, and the near-tie bound below which a label comparison between two fp64 evaluations is not decided.

The cases cover cropping and padding (also mixed per axis), up- and down-sampling, the [-0.5, 0) band that reads pixel 0 twice, the
c >= size - 0.5 rule, odd native sizes and the identity."""
import functools

import numpy as np

from cooperative_training_and_latent_space_data_augmentation_amd import prepare

F32 = np.float32
CASES = [
    ((2, 20, 24), (1, 1, 10), (0.8, 0.8, -1), (16, 16)),
    ((2, 20, 24), (1, 1, 10), (1.25, 1.25, -1), (32, 32)),
    ((3, 33, 17), (1, 1, 8), (0.7, 1.2, -1), (32, 16)),
    ((2, 20, 24), (1, 1, 10), (0.76, 0.93, -1), (16, 48)),
    ((2, 40, 36), (1.5625, 1.5625, 10), (1.36719, 1.36719, -1), (32, 32)),
    ((1, 25, 27), (2, 3, 5), (4, 6, -1), (16, 16)),
    ((2, 21, 19), (1, 1, 5), None, (16, 32)),
    ((1, 16, 16), (1, 1, 1), None, None),
]
IDS = ["x".join(map(str, c[0])) + "-" + ("id" if c[2] is None else "%g_%g" % c[2][:2]) + "-" + ("full" if c[3] is None else "%dx%d" % c[3])
       for c in CASES]
CLASSES = (2, 4, 5)
MODES = ("logit", "prob")
TIE = 1e-9                   # a voxel is decided when its top-two margin exceeds TIE * max |v| of the case


def geometry_of(case):
    shape, spacing, new_spacing, window = case
    return prepare.geometry(*shape, spacing=spacing, new_spacing=new_spacing, crop_size=window)


@functools.lru_cache(maxsize=None)
def scores_of(index, c):
    """float32 scores [n,C,Hc,Wc] of case `index`: default_rng(prod(shape)).normal(0, 3); computed once, never modified"""
    case = CASES[index]
    geo = geometry_of(case)
    s = np.random.default_rng(int(np.prod(case[0]))).normal(0.0, 3.0, size=(case[0][0], c) + tuple(geo.window_hw)).astype(F32)
    s.setflags(write=False)
    return s


@functools.lru_cache(maxsize=None)
def host_of(index, c, mode):
    """the host statement of case `index`: (label uint8 [n,h,w], soft float32 [n,C,h,w], v float64 [n,C,h,w], inside [h,w],
    decided bool [n,h,w]); computed once and shared, read-only"""
    geo = geometry_of(CASES[index])
    s = scores_of(index, c)
    label, soft = prepare.restore_scores_host(s, geo, mode=mode, want_soft=True)
    v, inside = prepare.restore_values_host(s, geo, mode=mode)
    out = (label, soft, v, inside, decided(v, inside))
    for a in out:
        a.setflags(write=False)
    return out


def decided(v, inside):
    """bool [n,h,w]: the top-two margin of the fp64 values exceeds TIE * max |v| (outside voxels are decided: their label is the rule's)"""
    top2 = np.sort(v, axis=1)[:, -2:]
    margin = top2[:, 1] - top2[:, 0] if v.shape[1] > 1 else np.full(top2[:, 0].shape, np.inf)
    return (margin > TIE * np.abs(v).max()) | ~inside[None]
