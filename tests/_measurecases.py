"""Label maps and host helpers for the measurement tests (tests/test_measure_cpu.py, tests/test_measure_gpu.py).
Nothing here depends on a GPU."""
import numpy as np

from _contourcases import isolated_pixels


def isolated_labels(n):
    """n isolated pixels labelled 1 .. n in raster order."""
    a = isolated_pixels(n)
    r, c = np.nonzero(a)
    a[r, c] = np.arange(1, n + 1)
    return a


def bar(h):
    """A vertical bar, one pixel wide and h rows high, off the image's edges."""
    a = np.zeros((h + 2, 3), np.int32)
    a[1:-1, 1] = 1
    return a


def parabola(h):
    """The one-pixel-wide object c = floor(r^2 / 64), r < h: its left chain is convex, most of its candidates are vertices."""
    r = np.arange(h)
    c = r * r // 64
    a = np.zeros((h, int(c.max()) + 1), np.int32)
    a[r, c] = 1
    return a


def disc(radius):
    r, c = np.indices((2 * radius + 1, 2 * radius + 1))
    return ((r - radius) ** 2 + (c - radius) ** 2 <= radius * radius).astype(np.int32)


def empty_rows():
    """One label with empty rows inside its box (two of them adjacent: a lattice line without candidates) beside another."""
    a = np.zeros((12, 9), np.int32)
    a[1, 2:5] = 1
    a[3, 6] = 1
    a[6, 0:2] = 1
    a[10, 4] = 1
    a[7:9, 4:8] = 2
    return a


def interleaved(h=11, w=7):
    """Two labels that alternate row by row: each has an empty row between any two of its rows."""
    a = np.zeros((h, w), np.int32)
    a[0::2, 1:] = 1
    a[1::2, :-2] = 2
    a[4, :] = 1
    return a


def brute_hull(mask):
    """The hull of the pixel corners by gift wrapping: from the smallest (y, x) take as next vertex the point with no point
    strictly to the right of the edge towards it, the farthest such; (n, 2) (x, y) in the order of measure.hull_host."""
    r, c = np.nonzero(np.asarray(mask))
    pts = sorted({(int(y + dy), int(x + dx)) for y, x in zip(r, c) for dy in (0, 1) for dx in (0, 1)})
    start = pts[0]
    ring, cur = [start], start
    while True:
        best = None
        for p in pts:
            if p == cur:
                continue
            if best is None:
                best = p
                continue
            # in (u, v) = (y, x) the ring runs with the points on its left: cross < 0 means p lies to the right of cur -> best
            cr = (best[0] - cur[0]) * (p[1] - cur[1]) - (best[1] - cur[1]) * (p[0] - cur[0])
            far = (p[0] - cur[0]) ** 2 + (p[1] - cur[1]) ** 2 > (best[0] - cur[0]) ** 2 + (best[1] - cur[1]) ** 2
            if cr < 0 or (cr == 0 and far):
                best = p
        if best == start:
            break
        ring.append(best)
        cur = best
        assert len(ring) <= len(pts)
    return np.array([(x, y) for y, x in ring], np.int64)


def full_row(H, W, d2max=None):
    """The row of the table of an all-ones H x W map in closed form (words 21, 22 from ``d2max`` = (value, pixel) or 0)."""
    n = H * W
    if H >= 2 and W >= 2:
        border = 2 * (H + W) - 4
    else:
        border = max(max(H, W) - 2, 0)
    q = H * (W + 1) + W
    return [n, W * H * (H - 1) // 2, H * W * (W - 1) // 2, W * (H - 1) * H * (2 * H - 1) // 6, H * (H - 1) // 2 * (W * (W - 1) // 2),
            H * (W - 1) * W * (2 * W - 1) // 6, 0, 0, H - 1, W - 1, border, 0, 0, 4, 0, 0, 2 * n, 4, H * H + W * W, 0, q,
            d2max[0] if d2max else 0, d2max[1] if d2max else 0, 0]
