"""Post-processing of predicted label maps (medseg/common_utils/post_process.py)."""
import numpy as np
import torch

from . import ops


def keep_largest_connected_components(mask, n_classes):
    """Keeps only the largest connected component of each label 1 .. n_classes - 1 of a segmentation mask (post_process.py:5-22).

    The whole array is one object: a 2-D mask is labelled in 2-D, a 3-D mask in 3-D, with the 4- / 6-neighbourhood (upstream's
    `connectivity=1`).  Among components of equal size the one whose first voxel in C order comes first is kept (`np.argmax` over
    components numbered in scan order); values >= n_classes are dropped.
      CUDA uint8 tensor -> CUDA uint8 tensor, on the device (ops.keep_largest_components: no copy to the host)
      numpy array       -> numpy uint8 array, on the host as upstream.  Upstream labels with skimage.measure.label(connectivity=1); the
                           host branch here uses scipy.ndimage.label with generate_binary_structure(mask.ndim, 1), which gives the same
                           partition and the same scan-order numbering without the scikit-image dependency."""
    if isinstance(mask, torch.Tensor):
        if not mask.is_cuda:
            raise TypeError("keep_largest_connected_components: a CUDA tensor (device path) or a numpy array (host path) is expected")
        return ops.keep_largest_components(mask, int(n_classes), connectivity=1, per_slice=False)
    from scipy import ndimage
    mask = np.asarray(mask)
    kept = np.zeros(mask.shape, dtype=np.uint8)
    structure = ndimage.generate_binary_structure(mask.ndim, 1)
    for c in range(1, int(n_classes)):
        comp, count = ndimage.label(mask == c, structure=structure)
        if count:
            voxels = np.bincount(comp.ravel(), minlength=count + 1)[1:]
            kept[comp == int(np.argmax(voxels)) + 1] = c
    return kept
