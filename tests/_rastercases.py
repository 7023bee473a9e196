"""Polygons for the fill tests (tests/test_raster_cpu.py, tests/test_raster_gpu.py): the named cases of DESIGN.md 3.23, seeded
random polygons, and the cases that sit on either side of the device path's constants.  A case is (features, (B, H, W)); a
feature is {image, rings_fixed, class}, its rings lists of (x, y) in fixed point (256 units per pixel).  Coordinates are written
in pixels and are exact multiples of 1/256.  Nothing here depends on a GPU."""
import numpy as np


def fx(points):
    """Pixel coordinates that are multiples of 1/256 -> exact fixed-point integers."""
    a = np.asarray(points, np.float64).reshape(-1, 2) * 256
    assert (a == np.round(a)).all(), 'a case coordinate is not on the 1/256 grid'
    return a.astype(np.int64).astype(np.int32)


def feat(*rings, image=0, cls=1):
    return {'image': image, 'rings_fixed': [fx(r) for r in rings], 'class': cls}


def box(x0, y0, x1, y1):
    return [(x0, y0), (x1, y0), (x1, y1), (x0, y1)]


def comb(teeth=40):
    pts = [(0, 9)]
    for i in range(teeth):
        pts += [(2 * i + 0.25, 9), (2 * i + 0.25, 0.25), (2 * i + 1.125, 0.25), (2 * i + 1.125, 9)]
    return pts + [(2 * teeth, 9), (2 * teeth, 11), (0, 11)]


def saw(teeth):
    """A saw-tooth of 2 teeth + 3 true vertices: no three consecutive ones on a line."""
    return [(0.5 * i, 1 + (i % 2) * 3.25) for i in range(2 * teeth + 1)] + [(teeth, 9), (0, 9)]


def named_cases():
    M = 2 ** 20 - 1
    c = {
        'unit_square': ([feat(box(0, 0, 1, 1))], (1, 3, 3)),
        'centre_square': ([feat(box(0.5, 0.5, 2.5, 2.5))], (1, 4, 4)),                       # fills 2 x 2
        'diamond': ([feat([(2.5, 0.5), (4.5, 2.5), (2.5, 4.5), (0.5, 2.5)])], (1, 6, 6)),   # slopes +-1 through centres
        'sliver': ([feat(box(0.625, 0.625, 3.375, 1.375))], (1, 4, 5)),                      # holds no centre
        'edge_on_centre_row': ([feat(box(0, 0.5, 3, 2.5))], (1, 4, 4)),
        'bow_tie': ([feat([(0, 0), (4, 4), (4, 0), (0, 4)])], (1, 5, 5)),
        'hole_and_island': ([feat(box(0, 0, 8, 8), box(2, 2, 6, 6)), feat(box(3, 3, 5, 5), cls=2)], (1, 9, 9)),
        'overlap_ab': ([feat(box(0, 0, 4, 4)), feat(box(2, 2, 6, 6), cls=2)], (1, 7, 7)),
        'overlap_ba': ([feat(box(2, 2, 6, 6), cls=2), feat(box(0, 0, 4, 4))], (1, 7, 7)),
        'degenerate': ([feat([(1, 1)]), feat([(1, 1), (3, 3)]),
                        feat([(0, 0), (0, 0), (4, 0), (4, 0), (4, 4), (0, 4), (0, 4)], [(2, 2)], cls=3),
                        feat([(5, 0), (9, 0), (9, 2), (12, 2.5), (9, 2), (9, 4), (5, 4)], cls=4),     # a zero-area spike
                        {'image': 0, 'rings_fixed': [], 'class': 5}], (1, 6, 14)),
        'whole_image': ([feat(box(-M, -M, M, M))], (1, 5, 7)),
        'far_triangle': ([feat([(-M, -M + 3), (M, M), (-M, M)])], (1, 9, 11)),                      # its long side crosses the image
        'comb40': ([feat(comb(40))], (1, 12, 82)),                                           # 80 crossings in a row
        'batch3': ([feat(box(1, 1, 4, 3), image=0), feat([(0.5, 0.5), (5.5, 1.5), (2.5, 4.5)], image=2, cls=2),
                    feat(box(0, 0, 2, 2), image=2, cls=3)], (3, 5, 6)),
    }
    H, W = 6, 7
    for side, (dx, dy) in {'left': (-1, 0), 'right': (1, 0), 'top': (0, -1), 'bottom': (0, 1)}.items():
        # a 3.5 x 2.5 box, wholly outside / straddling the side
        ox, oy = 1.25 + dx * (W + 1), 1.75 + dy * (H + 1)
        c[f'outside_{side}'] = ([feat(box(ox, oy, ox + 3.5, oy + 2.5))], (1, H, W))
        sx = {-1: -1.75, 0: 1.25, 1: W - 1.75}[dx]
        sy = {-1: -1.25, 0: 1.75, 1: H - 1.25}[dy]
        c[f'straddle_{side}'] = ([feat(box(sx, sy, sx + 3.5, sy + 2.5))], (1, H, W))
    return c


GRIDS = {'fine': 1, 'half': 128, 'integer': 256}          # half: every coordinate k + 0.5 -- every vertex a tie
SIZES = [(1, 1), (1, 257), (257, 1), (17, 15), (33, 65), (40, 40)]


def random_polygons(seed, H, W, grid, n=3):
    """n seeded polygons of 3 - 12 vertices on the named grid, coordinates from -3 to size + 3."""
    rs = np.random.RandomState(seed)
    out = []
    for _ in range(n):
        k = rs.randint(3, 13)
        if grid == 'half':
            x, y = rs.randint(-4, W + 3, k) * 256 + 128, rs.randint(-4, H + 3, k) * 256 + 128
        else:
            g = GRIDS[grid]
            x, y = rs.randint(-3 * 256 // g, (W + 3) * 256 // g + 1, k) * g, rs.randint(-3 * 256 // g, (H + 3) * 256 // g + 1, k) * g
        out.append({'image': 0, 'rings_fixed': [np.stack([x, y], 1).astype(np.int32)], 'class': 1 + len(out)})
    return out


def random_cases():
    c = {}
    for i, (H, W) in enumerate(SIZES):
        for j, grid in enumerate(GRIDS):
            c[f'random_{H}x{W}_{grid}'] = (random_polygons(100 + 10 * i + j, H, W, grid), (1, H, W))
    return c


def constant_cases(tile_rows, tile_cols, block):
    """Cases on either side of the device path's constants (taken from _lib by the caller)."""
    c = {}
    for name, n in (('minus', -1), ('equal', 0), ('plus', 1)):
        w, h = tile_cols + n, tile_rows + n
        # aligned to the tile lattice, and shifted by a pixel and a fraction so that the feature straddles the lattice
        c[f'cols_{name}'] = ([feat(box(0, 0.25, w, 2.75)), feat([(1.5, 3), (1.5 + w, 3.5), (1.25 + w, 6.5), (1.25, 6)], cls=2)],
                             (1, 7, 2 * tile_cols + 3))
        c[f'rows_{name}'] = ([feat(box(0.25, 0, 2.75, h)), feat([(3, 1.5), (3.5, 1.5 + h), (6.5, 1.25 + h), (6, 1.25)], cls=2)],
                             (1, 2 * tile_rows + 3, 7))
    c['tile_corner'] = ([feat([(tile_cols - 5.25, tile_rows - 4.5), (tile_cols + 6.5, tile_rows - 2.25),
                               (tile_cols + 3.75, tile_rows + 7.5), (tile_cols - 2.5, tile_rows + 5.25)])],
                        (1, 2 * tile_rows, 2 * tile_cols))
    teeth = 4 * block + 37                                                   # 2 teeth + 3 vertices: more than 2048 at block = 256
    c['saw'] = ([feat(saw(teeth))], (1, 10, teeth + 1))
    c['all_tiles_outside'] = ([feat(box(-3 * tile_cols, -2 * tile_rows, -tile_cols - 0.5, -0.75)),
                               feat(box(3, 3, 5, 5), cls=2)], (1, 8, 8))
    return c


def one_pixel_features(n, W):
    """n features, feature i the pixel (i // W, i % W): as CSR arrays, built without a loop over the features."""
    i = np.arange(n)
    r, c = i // W, i % W
    x = np.stack([c, c + 1, c + 1, c], 1) * 256
    y = np.stack([r, r, r + 1, r + 1], 1) * 256
    verts = np.stack([x, y], 2).reshape(-1, 2).astype(np.int32)
    first = (4 * np.arange(n + 1)).astype(np.int32)
    return verts, first, np.arange(n + 1, dtype=np.int32), np.zeros(n, np.int32), (1 + i % 251).astype(np.uint8)
