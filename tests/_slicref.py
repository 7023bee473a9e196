"""Teacher-forced, round-by-round fp64 reference of the SLIC assignment (csrc/slic.hip), and the case list of
tests/test_slic_rounds_gpu.py and tests/test_slicref_cpu.py.

Ten rounds of k-means amplify one flipped pixel.  Instead of tolerating that, the reference is forced onto the trajectory of
the implementation under test (the "teacher"): before round i+1 its fp64 centres move to the mean of the pixels the teacher
gave each centre in round i, and only the assignment of that one round is compared.  The assignment is the published one:
centre-wise 2S windows around the centres' current positions, D^2 = |lab/m - c|^2 + (dy^2 + dx^2)/S^2, ascending centre index
with strict <, Lab in fp64 from the textbook formula.  A pixel inside no window takes the centre of its home grid cell (the
device's documented rule).

The same code runs in float32 with the arithmetic of oracle/slic_oracle.kmeans_labels (``dtype=np.float32``); the distance
between that and fp64, forced the same way, is what TAU is derived from.
"""
import functools

import numpy as np

import _tol
from oracle import slic_oracle as so

EDGE = 1e-4          # pixels: a window edge this close to a pixel may fall on either side
CAP = 0.002          # at most this fraction of a case's pixels may be excused as near ties in one round

# Largest relative excess (d64(p, k32) - d64(p, k64)) / (1 + d64(p, k64)) over all disagreeing pixels, all rounds and all of
# CASES below, of the float32 evaluation against the fp64 one; printed by
#     python -m pytest tests/test_slicref_cpu.py -k tau -s
# TAU = 4 x that: the margin covers powf / cbrtf / fma differences between numpy and the device and the 2^-20 fixed-point
# centre sums.  tests/test_slicref_cpu.py::test_tau_is_four_times_the_measured_fp32_excess pins both numbers.
FP32_EXCESS = 1.492e-06                     # measured 1.4920e-06 at synth-96x128-n60-m1, the only disagreeing pixel
TAU = 4 * FP32_EXCESS                       # 5.968e-06


# ---------------------------------------------------------------- colour
def lab64(img):
    """img (3,H,W) in [0,1] -> (H,W,3) CIE Lab (D65, 2 degree observer) in fp64: sRGB companding, the sRGB -> XYZ matrix,
    white point (0.95047, 1, 1.08883), f(t) = t^(1/3) above 0.008856 and 7.787 t + 16/116 below."""
    rgb = np.moveaxis(np.asarray(img, dtype=np.float64), 0, -1)
    lin = np.where(rgb > 0.04045, ((rgb + 0.055) / 1.055) ** 2.4, rgb / 12.92)
    m = np.array([[0.412453, 0.357580, 0.180423], [0.212671, 0.715160, 0.072169], [0.019334, 0.119193, 0.950227]])
    xyz = lin @ m.T / np.array([0.95047, 1.0, 1.08883])
    f = np.where(xyz > 0.008856, np.cbrt(xyz), 7.787 * xyz + 16.0 / 116.0)
    return np.stack([116.0 * f[..., 1] - 16.0, 500.0 * (f[..., 0] - f[..., 1]), 200.0 * (f[..., 1] - f[..., 2])], axis=-1)


def lab_branches(img):
    """(pixels' channel values, XYZ / white values) of an image: the operands of the two piecewise tests of lab64."""
    rgb = np.moveaxis(np.asarray(img, dtype=np.float64), 0, -1)
    lin = np.where(rgb > 0.04045, ((rgb + 0.055) / 1.055) ** 2.4, rgb / 12.92)
    m = np.array([[0.412453, 0.357580, 0.180423], [0.212671, 0.715160, 0.072169], [0.019334, 0.119193, 0.950227]])
    return rgb, lin @ m.T / np.array([0.95047, 1.0, 1.08883])


# ---------------------------------------------------------------- geometry
class Grid:
    def __init__(self, H, W, n_segments):
        ys, xs, step = so.grid(H, W, n_segments)
        self.H, self.W, self.step, self.start = H, W, int(step), int(ys[0])
        self.ys, self.xs = ys, xs
        self.gy, self.gx, self.K = len(ys), len(xs), len(ys) * len(xs)

    def home(self):
        """(HW,) centre index of every pixel's home grid cell: the nearest grid position, clipped to the grid."""
        cy = np.clip((np.arange(self.H) - self.start + self.step // 2) // self.step, 0, self.gy - 1)
        cx = np.clip((np.arange(self.W) - self.start + self.step // 2) // self.step, 0, self.gx - 1)
        return (cy[:, None] * self.gx + cx[None, :]).ravel()

    def tile_table_sizes(self, radius=3, tile=16):
        """Centres a 16 x 16 tile of the device's tile kernel stages (its ``nc``), per tile."""
        def span(size, g):
            cell = lambda v: min(max((v - self.start + self.step // 2) // self.step, 0), g - 1)
            return [min(cell(min(t + tile, size) - 1) + radius, g - 1) - max(cell(t) - radius, 0) + 1 for t in range(0, size, tile)]
        return np.outer(span(self.H, self.gy), span(self.W, self.gx))


def init_centres(lab, grid, dtype=np.float64):
    """(K,5) {y, x, L, a, b} of the grid centres; lab (H,W,3) already divided by the compactness."""
    cy, cx = np.meshgrid(grid.ys, grid.xs, indexing='ij')
    return np.concatenate([cy.reshape(-1, 1), cx.reshape(-1, 1), lab[cy.ravel(), cx.ravel()]], axis=1).astype(dtype)


def dist(lab, cen, grid, pix, k):
    """D^2 of pixel indices ``pix`` to centres ``k`` in the dtype of ``cen`` (the expression of slic_oracle.kmeans_labels)."""
    dt = cen.dtype.type
    S = dt(grid.step)
    y, x = (pix // grid.W).astype(dt), (pix % grid.W).astype(dt)
    dy, dx = y - cen[k, 0], x - cen[k, 1]
    dc = lab.reshape(-1, 3)[pix] - cen[k, 2:5]
    return (dc[:, 0] ** 2 + dc[:, 1] ** 2 + dc[:, 2] ** 2) + (dy * dy + dx * dx) / (S * S)


def assign(lab, cen, grid):
    """One exact assignment round -> (HW,) centre indices.  Every (centre, pixel) pair of every centre's window is evaluated; a
    pixel takes the smallest D^2, the lowest centre index among equals, and its home cell if no window holds it.  lab and cen
    share a dtype; in float32 the window bounds and D^2 are slic_oracle.kmeans_labels' to the bit."""
    dt = cen.dtype.type
    assert lab.dtype == cen.dtype
    H, W, S = grid.H, grid.W, dt(grid.step)
    y0 = np.maximum(0, np.ceil(cen[:, 0] - 2 * S)).astype(np.int64)
    y1 = np.minimum(H - 1, np.floor(cen[:, 0] + 2 * S)).astype(np.int64)
    x0 = np.maximum(0, np.ceil(cen[:, 1] - 2 * S)).astype(np.int64)
    x1 = np.minimum(W - 1, np.floor(cen[:, 1] + 2 * S)).astype(np.int64)
    off = np.arange(4 * grid.step + 1)
    yy, xx = y0[:, None] + off, x0[:, None] + off                          # (K, 4S+1): a window has at most 4S+1 rows
    ok = (yy <= y1[:, None])[:, :, None] & (xx <= x1[:, None])[:, None, :]
    k, iy, ix = np.nonzero(ok)                                             # k ascending
    pix = yy[k, iy] * W + xx[k, ix]
    d = dist(lab, cen, grid, pix, k)
    order = np.lexsort((k, d, pix))                                        # by pixel, then D^2, then centre index
    pix, k = pix[order], k[order]
    first = np.ones(len(pix), dtype=bool)
    first[1:] = pix[1:] != pix[:-1]
    labels = grid.home().copy()
    labels[pix[first]] = k[first]
    return labels


def in_no_window(cen, grid):
    """(HW,) bool: pixels that no centre's window holds."""
    y, x = np.divmod(np.arange(grid.H * grid.W), grid.W)
    S2 = 2.0 * grid.step
    held = (np.abs(y[None, :] - cen[:, 0:1]) <= S2) & (np.abs(x[None, :] - cen[:, 1:2]) <= S2)
    return ~held.any(axis=0)


def update(cen, labels, lab):
    """Centres move to the fp64 mean of their members (stored in cen's dtype); a centre without members keeps its value."""
    K = cen.shape[0]
    cnt = np.bincount(labels, minlength=K)
    y, x = np.divmod(np.arange(len(labels)), lab.shape[1])
    out = cen.copy()
    flat = lab.reshape(-1, 3)
    for j, v in enumerate([y, x, flat[:, 0], flat[:, 1], flat[:, 2]]):
        s = np.bincount(labels, weights=v.astype(np.float64), minlength=K)
        out[cnt > 0, j] = (s[cnt > 0] / cnt[cnt > 0]).astype(cen.dtype)
    return out


# ---------------------------------------------------------------- the comparison rule
def compare(got, ref, lab, cen, grid, tau):
    """Compares one round's labels ``got`` (HW,) with the reference's ``ref`` under fp64 lab / cen.

    A differing pixel is excused when the reference's centre has a window edge within EDGE of the pixel, or when the centre
    that was chosen holds the pixel in its window (to within EDGE) and is at most ``tau`` worse, relative to 1 + D^2.
    Returns dict(n_diff, n_excused, worst (largest excess among pixels whose chosen centre's window holds them), bad (pixel
    indices not excused))."""
    got = np.asarray(got).ravel().astype(np.int64)
    assert got.min() >= 0 and got.max() < grid.K, (got.min(), got.max(), grid.K)
    pix = np.nonzero(got != ref)[0]
    if len(pix) == 0:
        return dict(n_diff=0, n_excused=0, worst=0.0, bad=pix)
    kg, kr = got[pix], ref[pix]
    y, x = pix // grid.W, pix % grid.W
    S2 = 2.0 * grid.step
    dr = dist(lab, cen, grid, pix, kr)
    excess = (dist(lab, cen, grid, pix, kg) - dr) / (1.0 + dr)
    held_g = (np.abs(y - cen[kg, 0]) <= S2 + EDGE) & (np.abs(x - cen[kg, 1]) <= S2 + EDGE)
    edge_r = (np.abs(np.abs(y - cen[kr, 0]) - S2) <= EDGE) | (np.abs(np.abs(x - cen[kr, 1]) - S2) <= EDGE)
    excused = edge_r | (held_g & (excess <= tau))
    judged = held_g & ~edge_r
    return dict(n_diff=len(pix), n_excused=int(excused.sum()), worst=float(excess[judged].max()) if judged.any() else 0.0,
                bad=pix[~excused])


def forced_rounds(img, n_segments, compactness, teacher, rounds=10, tau=np.inf):
    """Runs the fp64 reference along the teacher's trajectory.  ``teacher(i)`` returns the labels (HW,) of the teacher's
    assignment round i (1-based).  Yields per round (i, result of compare, reference labels, reference centres)."""
    H, W = img.shape[1:]
    grid = Grid(H, W, n_segments)
    lab = lab64(img) / float(compactness)
    cen = init_centres(lab, grid)
    for i in range(1, rounds + 1):
        ref = assign(lab, cen, grid)
        got = np.asarray(teacher(i)).ravel().astype(np.int64)
        yield i, compare(got, ref, lab, cen, grid, tau), ref, cen
        cen = update(cen, got, lab)


def fp32_teacher(img, n_segments, compactness):
    """The float32 evaluation as a teacher: slic_oracle.kmeans_labels' arithmetic, round i from its own round i-1."""
    H, W = img.shape[1:]
    grid = Grid(H, W, n_segments)
    lab = so.rgb2lab(img) / np.float32(compactness)
    state = {'cen': init_centres(lab, grid, np.float32), 'i': 0, 'labels': None}

    def teacher(i):
        assert i == state['i'] + 1
        if i > 1:
            state['cen'] = update(state['cen'], state['labels'], lab)
        state['labels'], state['i'] = assign(lab, state['cen'], grid), i
        return state['labels']
    return teacher


def unforced(img, n_segments, compactness, rounds=10, dtype=np.float64):
    """``rounds`` rounds from the evaluation's own labels: what slic_oracle.kmeans_labels computes."""
    H, W = img.shape[1:]
    grid = Grid(H, W, n_segments)
    lab = (lab64(img) / float(compactness)) if dtype == np.float64 else so.rgb2lab(img) / np.float32(compactness)
    cen = init_centres(lab, grid, dtype)
    for _ in range(rounds):
        labels = assign(lab, cen, grid)
        cen = update(cen, labels, lab)
    return labels.reshape(H, W)


# ---------------------------------------------------------------- the device as the teacher
ROUNDS = 10


def device_rounds(imgs, n_seg, m):
    """imgs (B,3,H,W) numpy -> list over rounds 1..ROUNDS of (B, HW) int64 centre indices."""
    import torch
    from wesup_amd import ops
    t = torch.from_numpy(np.array(imgs, dtype=np.float32)).to('cuda:0')        # a copy: the cached images are read-only
    return [ops.slic(t, n_seg, m, i, enforce_connectivity=False)[0].cpu().numpy().reshape(len(imgs), -1).astype(np.int64)
            for i in range(1, ROUNDS + 1)]


def check_rounds(name, img, n_seg, m, rounds):
    """The rule of the module docstring for one image; ``rounds[i-1]`` (HW,) are the device's labels of round i.  Returns the
    number of pixels, over all rounds, whose label differs from the reference's (all of them excused)."""
    H, W = img.shape[1:]
    failures, worst, n_diff = [], 0.0, 0
    for i, r, _, _ in forced_rounds(img, n_seg, m, lambda i: rounds[i - 1], ROUNDS, tau=TAU):
        print(f'{name} round {i}: {r["n_diff"]} differ, {r["n_excused"]} excused, worst excess {r["worst"]:.3e}, '
              f'{len(r["bad"])} not excused')
        worst, n_diff = max(worst, r['worst']), n_diff + r['n_diff']
        if len(r['bad']):
            failures.append((i, 'not a near tie', [(int(p) // W, int(p) % W) for p in r['bad'][:8]], len(r['bad'])))
        if r['n_excused'] > CAP * H * W:
            failures.append((i, 'excused pixels over the cap', r['n_excused'], CAP * H * W))
    ok = _tol.within(name, 'slic_tie_excess', worst, TAU, 'relative D^2 excess of a label that differs from the fp64 choice')
    assert not failures, failures
    assert ok, (worst, TAU)
    return n_diff


# ---------------------------------------------------------------- images
def dark_image(seed, H, W):
    """A diagonal ramp from 0 to 0.1 (the linear branches of the companding and of f) with a little noise, and small patches
    of saturated primaries (the power branches)."""
    rs = np.random.RandomState(seed)
    yy, xx = np.meshgrid(np.arange(H), np.arange(W), indexing='ij')
    ramp = 0.1 * (yy + xx) / max(H + W - 2, 1)
    img = np.clip(ramp[None] * (1.0 + 0.1 * rs.rand(3, H, W)), 0.0, 0.1).astype(np.float32)
    img[:, 0, 0] = 0.0
    img[:, H - 1, W - 1] = 0.1
    n = max(3, H * W // 400)
    for j in range(n):
        y, x = rs.randint(0, H), rs.randint(0, W)
        col = np.zeros(3, dtype=np.float32)
        col[j % 3] = 1.0
        img[:, y:y + 3, x:x + 3] = col[:, None, None]
    return img


@functools.lru_cache(maxsize=None)
def image(kind, H, W):
    from wesup_amd import synth
    if kind == 'synth':
        img = synth.synth_image(5, H, W)
    elif kind == 'region':
        from test_slic_gpu import _region_image                 # piecewise-constant colours over a Voronoi tessellation
        img = _region_image(7, H, W, 4 if min(H, W) >= 32 else (2 if min(H, W) >= 4 else 1))[0]
    elif kind == 'noise':
        img = np.random.RandomState(SEEDS['noise']).rand(3, H, W).astype(np.float32)
    elif kind == 'dark':
        img = dark_image(SEEDS['dark'], H, W)
    else:
        raise KeyError(kind)
    img.setflags(write=False)
    return img


SEEDS = {'noise': 21, 'dark': 33}
IMAGES = ('synth', 'region', 'noise', 'dark')

# (H, W, n_segments, compactness, images): what each row reaches is in its comment (test_slicref_cpu pins steps and kernels)
_ROWS = [
    (96, 128, 60, 40.0, IMAGES),            # tile kernel, step 14, drift 0.4 S
    (96, 128, 60, 10.0, IMAGES),            # drift about 2 S
    (96, 128, 60, 1.0, IMAGES),             # drift beyond 2 S: a search of 7 x 7 cells misses candidates here
    (96, 128, 1400, 10.0, IMAGES),          # tile kernel at step 3, its LDS centre table fullest (12 x 12 of 176)
    (96, 128, 4000, 10.0, ('synth',)),      # per-pixel kernel at step 2, more than one block, drift beyond 2 S
    (33, 47, 388, 10.0, IMAGES),            # per-pixel kernel at step 2, H and W no multiples of 16
    (33, 47, 1551, 40.0, IMAGES),           # step 1, start 0: every pixel a centre
    (5, 7, 100, 40.0, IMAGES),              # smaller than a tile, n_segments > HW
    (5, 7, 1, 40.0, IMAGES),                # a 1 x 1 grid
    (1, 40, 4, 40.0, IMAGES),               # start clipped to H - 1
    (40, 1, 4, 40.0, IMAGES),               # start clipped to W - 1
    (50, 21, 30, 20.0, IMAGES),             # HW just over one scan block of 1024
]
CASES = [(kind, H, W, n, m) for H, W, n, m, kinds in _ROWS for kind in kinds]
# one call with three different images: a wrong image index in the grid, the centre table or the sums shows.  In the last
# one drift widens the search at step 3 beyond the tile kernel's table, so its blocks take the per-pixel form
BATCHES = [(('synth', 'region', 'noise'), 96, 128, 60, 10.0), (('dark', 'noise', 'synth'), 33, 47, 388, 10.0),
           (('noise', 'dark', 'region'), 96, 128, 1400, 1.0)]


def case_id(c):
    kind = c[0] if isinstance(c[0], str) else '+'.join(c[0])
    return f'{kind}-{c[1]}x{c[2]}-n{c[3]}-m{c[4]:g}'
