"""Shared cases of the surface-metric tests (tests/test_surface_cpu.py, tests/test_surface_gpu.py): masks, blob scenes and the
definitions of the scores written directly with scipy."""
import functools

import numpy as np
from scipy import ndimage

EDT_SHAPES = ((1, 1), (1, 131), (131, 1), (63, 65), (64, 129), (70, 300), (37, 53))
DENSITIES = (0.5, 0.05, 0.001)          # share of zero pixels
N_PAIRS = 20
PAIR_SHAPE = (96, 80)
CROSS = ndimage.generate_binary_structure(2, 1)


def random_mask(h, w, zero_density, seed):
    """bool; may have no zero pixel at all (small shapes at a low density)."""
    return np.random.default_rng(seed).random((h, w)) >= zero_density


def edt_cases():
    """(name, mask) over the shapes and densities of the issue, all ones / all zeros and a (3, 37, 53) batch of the three."""
    out = []
    for h, w in EDT_SHAPES:
        for d in DENSITIES:
            out.append((f'{h}x{w}@{d}', random_mask(h, w, d, seed=h * 1000 + w + int(d * 1000))))
    out.append(('ones', np.ones((37, 53), bool)))
    out.append(('zeros', np.zeros((37, 53), bool)))
    out.append(('batch', np.stack([random_mask(37, 53, 0.05, 5), np.ones((37, 53), bool), np.zeros((37, 53), bool)])))
    return out


def edt_sq_scipy(mask):
    """rint(distance_transform_edt^2) per image; 2^31 - 1 for an image without a zero pixel (scipy has no answer there)."""
    F = np.asarray(mask) != 0
    if F.ndim == 3:
        return np.stack([edt_sq_scipy(f) for f in F])
    if F.all():
        return np.full(F.shape, 2 ** 31 - 1, np.int64)
    return np.rint(ndimage.distance_transform_edt(F) ** 2).astype(np.int64)


def border_scipy(mask):
    F = np.asarray(mask) != 0
    if F.ndim == 3:
        return np.stack([border_scipy(f) for f in F])
    return F & ~ndimage.binary_erosion(F, CROSS, border_value=0)


def blobs(h, w, n, rng, rmin=4, rmax=14):
    yy, xx = np.mgrid[:h, :w]
    out = np.zeros((h, w), bool)
    for _ in range(n):
        cy, cx = rng.uniform(0, h), rng.uniform(0, w)
        ry, rx = rng.uniform(rmin, rmax, 2)
        out |= ((yy - cy) / ry) ** 2 + ((xx - cx) / rx) ** 2 <= 1.0
    return out


def blob_pair(seed, shape=PAIR_SHAPE):
    """(pred, gt): a few ellipses, the prediction shifted by a pixel or two, grown or shrunk, with a blob missed or made up."""
    rng = np.random.default_rng(1000 + seed)
    h, w = shape
    scale = max(min(h, w) / 80.0, 0.25)
    gt = blobs(h, w, int(rng.integers(2, 6)), rng, 4 * scale, 14 * scale)
    pred = np.roll(gt, (int(rng.integers(-2, 3)), int(rng.integers(-2, 3))), (0, 1))
    k = int(rng.integers(0, 3))
    if k == 1:
        pred = ndimage.binary_dilation(pred, iterations=int(rng.integers(1, 4)))
    elif k == 2:
        pred = ndimage.binary_erosion(pred, iterations=int(rng.integers(1, 3)))
    if seed % 3 == 0:
        pred |= blobs(h, w, 1, rng, 3 * scale, 6 * scale)
    return pred, gt


@functools.lru_cache(maxsize=None)
def blob_pairs():
    return tuple(blob_pair(s) for s in range(N_PAIRS))


def directed_scipy(pred, gt):
    """(d_pg, d_gp): the border-to-border distances of both directions by scipy's transform, float64."""
    SP, SG = border_scipy(pred), border_scipy(gt)
    return ndimage.distance_transform_edt(~SG)[SP], ndimage.distance_transform_edt(~SP)[SG]


def rel_sum_bound(n):
    """Relative bound between two float64 sums of the same n non-negative terms when each term (a square root) is within one
    ulp of the exact value and the additions are in any order: (n + 2) 2^-52."""
    return (n + 2) * 2.0 ** -52
