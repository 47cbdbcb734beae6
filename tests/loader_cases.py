"""The fixture the loader tests share (no test in here): five small volumes of different in-plane sizes, seeded."""
import itertools

import numpy as np

SHAPES = [(3, 20, 28), (2, 37, 31), (1, 33, 32), (4, 32, 32), (2, 45, 26)]
EMPTY = [(0, 1), (3, 2)]                                # (volume, slice) with an all-zero label
LABEL_MAP = {1: 3, 2: 1, 3: 2}                          # 0 and 7 have no entry: both map to 0
PAD = (32, 32)
CROPS = [(24, 24), (23, 25)]
CANVASES = [None, (32, 32), (40, 40)]                   # None: the default, (45, 32) for these volumes
DEFAULT_CANVAS = (45, 32)
INDEX = {1: [4], 5: [11, 0, 11, 7, 3], 16: [0, 1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 11, 11, 0, 6, 6]}


def make_volumes():
    """[(image [s,h,w] float32 with negative values, label [s,h,w] in {0, 1, 2, 3, 7}; uint8 and int64 alternate)]"""
    rng = np.random.default_rng(20240)
    out = []
    for k, (s, h, w) in enumerate(SHAPES):
        image = rng.normal(0.0, 40.0, (s, h, w)).astype(np.float32)
        label = rng.choice(np.array([0, 1, 2, 3, 7]), size=(s, h, w), p=[0.5, 0.15, 0.15, 0.15, 0.05])
        for v, i in EMPTY:
            if v == k:
                label[i] = 0
        out.append((image, label.astype(np.uint8 if k % 2 == 0 else np.int64)))
    return out


def slice_list(volumes):
    return [(im[i], la[i].astype(np.uint8)) for im, la in volumes for i in range(im.shape[0])]


def combos():
    return list(itertools.product(range(len(CANVASES)), range(len(CROPS)), sorted(INDEX)))
