"""Label maps for the outline tests (tests/test_contour_cpu.py, tests/test_contour_gpu.py): the named cases of DESIGN.md 3.21 and
seeded random maps.  Nothing here depends on a GPU."""
import numpy as np


def named_cases():
    ring3 = np.ones((3, 3), np.int32)
    ring3[1, 1] = 0
    two_holes = np.ones((4, 4), np.int32)
    two_holes[1, 1] = two_holes[2, 2] = 0
    return [('pixel', np.array([[1]], np.int32)),
            ('saddle', np.array([[1, 0], [0, 1]], np.int32)),
            ('ring3', ring3),
            ('two_holes', two_holes),
            ('touching', np.array([[1, 2]], np.int32)),
            ('row511', np.ones((1, 511), np.int32))]


def random_map(seed, H, W, n_labels=1):
    """A seeded map with labels 0 .. n_labels, the foreground share drawn from the seed too."""
    rs = np.random.RandomState(seed)
    fg = rs.rand(H, W) < rs.uniform(0.2, 0.8)
    return (fg * rs.randint(1, n_labels + 1, (H, W))).astype(np.int32)


def checkerboard(H, W):
    return (np.indices((H, W)).sum(0) & 1).astype(np.int32)


def isolated_pixels(n):
    """n isolated pixels: one every second column and row, 4 n cracks."""
    side = int(np.ceil(np.sqrt(n)))
    a = np.zeros((2 * side, 2 * side), np.int32)
    k = np.arange(n)
    a[2 * (k // side), 2 * (k % side)] = 1
    return a


def serpentine(n=64):
    """A one-pixel-wide path winding through n x n: rows 0, 2, 4, ... joined at alternating ends -- one ring."""
    a = np.zeros((n, n), np.int32)
    a[0::2] = 1
    for k, r in enumerate(range(1, n, 2)):
        a[r, n - 1 if k % 2 == 0 else 0] = 1
    return a


def hole_count(mask):
    """4-connected background components that do not reach the outside of the image."""
    from scipy import ndimage
    pad = np.pad(np.asarray(mask) == 0, 1, constant_values=True)
    lab, n = ndimage.label(pad)
    return n - 1
