"""The polygon fill's definition pixel by pixel in plain Python integers: for every pixel centre the edges that
count are counted one by one.  It shares nothing with the scanline form of wesup_amd/raster.py:fill_host -- no c*, no division,
no CSR tables: it reads the feature dicts of tests/_rastercases.py directly.  Nothing here depends on a GPU."""
import numpy as np


def counts(x0, y0, x1, y1, Xc, Yc):
    """Does the edge count for the centre (Xc, Yc)?  Python integers: no width to overflow."""
    if y0 == y1:
        return False
    if y0 > y1:
        x0, y0, x1, y1 = x1, y1, x0, y0
    return y0 <= Yc < y1 and (x1 - x0) * (Yc - y0) <= (Xc - x0) * (y1 - y0)


def covers(rings, Xc, Yc):
    n = 0
    for ring in rings:
        pts = [(int(x), int(y)) for x, y in ring]
        for i, (x0, y0) in enumerate(pts):
            x1, y1 = pts[(i + 1) % len(pts)]
            n += counts(x0, y0, x1, y1, Xc, Yc)
    return n & 1 == 1


def labels_ref(features, shape):
    """features: dicts {image, rings_fixed}; shape (B, H, W) -> int32 labels: 1 + the largest index of a covering feature."""
    B, H, W = shape
    out = np.zeros((B, H, W), np.int32)
    for f, feat in enumerate(features):
        b = int(feat.get('image', 0))
        rings = [np.asarray(r).reshape(-1, 2).tolist() for r in feat['rings_fixed']]
        if not rings:
            continue
        ys = [y for r in rings for _, y in r]
        r_lo, r_hi = max(0, (min(ys) - 128) // 256), min(H, (max(ys) - 128) // 256 + 2)      # a superset of the rows that can be covered
        for r in range(r_lo, r_hi):
            for c in range(W):
                if covers(rings, 256 * c + 128, 256 * r + 128):
                    out[b, r, c] = f + 1
    return out
