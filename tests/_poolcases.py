"""The case list of tests/test_pooling_branches_gpu.py: label maps, shapes, inputs and -- per case -- the fp64 reference, the
honest fp32 evaluation on the CPU and the bars derived from it (tests/_poolref.py).  tests/test_poolref_cpu.py walks the same
list without a GPU: it checks the branch every map is built for and records the fp32-CPU figures."""
import functools

import numpy as np

import _poolref as pr


# ---------------------------------------------------------------- label maps
@functools.lru_cache(maxsize=None)
def label_map(name):
    """dict(labels (B,H,W) int32, masks (B,2,H,W) uint8, Kmax, probe): ``probe`` names pixels of the constructed superpixels."""
    from wesup_amd import synth
    probe, kpad = {}, 0
    if name.startswith('vor') or name.startswith('ms'):
        H, W, g, B, kpad = {'vor96': (96, 96, 8, 2, 5), 'vor240': (240, 240, 12, 1, 0), 'vor32': (32, 32, 4, 1, 3), 'vor480': (480, 480, 24, 1, 0),
                            'ms197': (197, 293, 17, 1, 3), 'ms182': (182, 271, 16, 1, 0), 'ms156': (156, 232, 13, 1, 2)}[name]
        labs = np.stack([synth.voronoi_labels(11 + b, H, W, g) for b in range(B)])
    elif name in ('lens', 'lensP'):                      # Kmax equal to the count / padded beyond it
        lab, probe = pr.lengths_map()
        labs, kpad = lab[None], (7 if name == 'lensP' else 0)
    elif name in ('skew', 'skewS'):
        labs, kpad = synth.skewed_labels(31, *((240, 200) if name == 'skew' else (120, 100)), 20)[None], 4
    elif name == 'diag':
        lab, p = pr.diagonal_map()
        labs, probe, kpad = lab[None], {'diag': p}, 1
    elif name in ('box32', 'box33'):
        lab, p = pr.corner_map(128, 128, 64, 64, 32 if name == 'box32' else 33, 32)
        labs, probe, kpad = lab[None], {'box': p}, 2
    else:
        raise KeyError(name)
    masks = np.stack([synth.point_mask(70 + b, labs[b], 0.3, 2) for b in range(len(labs))])
    n = int(labs.max()) + 1
    assert all(int(l.max()) + 1 == n for l in labs)
    return dict(labels=labs.astype(np.int32), masks=masks, Kmax=n + kpad, n=n, probe=probe)


@functools.lru_cache(maxsize=None)
def rows(name):
    """[(new_row, area_new, K)] per image, the reference's row order."""
    m = label_map(name)
    return [pr.rows_of(m['labels'][b], m['masks'][b]) for b in range(len(m['labels']))]


# ---------------------------------------------------------------- forward cases
# (map, h, w, C, coff, zero_mean); the output is (B, Kmax, coff + C + 32) filled with a sentinel.  h, w = 0: native resolution.
# Tolerance class = kind of map: the skewed maps' rows of thousands of pixels are where the sequential fp32 sum is the noisy part.
FWD = [
    # Voronoi, batch 2: every template instance and the slab loop at native resolution ...
    ('vor96', 0, 0, 32, 0, False), ('vor96', 0, 0, 64, 32, False), ('vor96', 0, 0, 128, 256, False),
    ('vor96', 0, 0, 256, 0, False), ('vor96', 0, 0, 512, 32, False),
    # ... and on coarse grids H/2, H/4, H/8, H/16; an axis of one cell; zero-mean data
    ('vor96', 48, 48, 32, 256, False), ('vor96', 24, 24, 64, 0, False), ('vor96', 12, 12, 128, 32, False),
    ('vor96', 6, 6, 256, 256, False), ('vor96', 48, 48, 512, 0, False), ('vor96', 1, 1, 128, 0, False),
    ('vor96', 1, 48, 32, 32, False), ('vor96', 48, 1, 64, 0, False), ('vor96', 48, 48, 64, 0, True),
    # the constructed lengths (1 ... 1025 pixels), Kmax equal to the count and padded
    ('lens', 0, 0, 32, 32, False), ('lensP', 0, 0, 64, 0, False), ('lens', 0, 0, 128, 0, False), ('lensP', 0, 0, 256, 32, False),
    ('lens', 0, 0, 512, 256, False), ('lensP', 64, 64, 32, 0, False), ('lens', 32, 32, 64, 256, False),
    ('lensP', 16, 16, 128, 32, False), ('lens', 8, 8, 256, 0, False), ('lensP', 64, 64, 512, 0, False),
    # rows of many segments
    ('skew', 0, 0, 128, 0, False), ('skew', 0, 0, 256, 32, False), ('skew', 30, 25, 512, 0, False),
    ('skew', 120, 100, 64, 0, True), ('skew', 60, 50, 32, 256, False),
    # the cell-wise branch at its capacity, one cell beyond it, and far beyond it
    ('box32', 64, 64, 64, 0, False), ('box32', 64, 64, 512, 32, False), ('box33', 64, 64, 64, 32, False),
    ('box33', 64, 64, 512, 0, False), ('diag', 64, 64, 128, 0, False), ('diag', 64, 64, 512, 256, False),
    # the step's real geometry, an odd multi-scale shape, non-integer ratios
    ('vor480', 0, 0, 64, 32, False), ('vor480', 120, 120, 128, 0, False), ('vor480', 60, 60, 256, 256, False),
    ('vor480', 30, 30, 512, 0, False), ('vor240', 0, 0, 256, 0, False), ('vor240', 15, 15, 512, 32, False),
    ('vor240', 120, 120, 64, 0, False), ('ms197', 0, 0, 128, 0, False), ('ms197', 98, 146, 32, 0, False),
    ('ms197', 49, 73, 64, 32, False), ('ms197', 24, 36, 256, 0, False), ('ms156', 39, 58, 128, 256, False),
]


def map_class(name):
    return {'skew': 'skewed', 'skewS': 'skewed', 'lens': 'lengths', 'lensP': 'lengths', 'box32': 'cell-box', 'box33': 'cell-box',
            'diag': 'cell-box'}.get(name, 'voronoi')


def fwd_id(c):
    mp, h, w, C, coff, zm = c
    return f"{mp}-{'native' if h == 0 else f'{h}x{w}'}-C{C}-off{coff}" + ('-zeromean' if zm else '')


def geometry(c):
    m = label_map(c[0])
    B, H, W = m['labels'].shape
    h, w = (H, W) if c[1] == 0 else (c[1], c[2])
    return B, H, W, h, w


def fwd_input(i, c):
    B, H, W, h, w = geometry(c)
    return pr.relu_like(1000 + i, (B, h, w, c[3]), zero_mean=c[5])


def fwd_reference(i, c):
    """Per image: (ref64 (K, C), scale (K,), fp32 whole, fp32 per_row) -- the fp32 figures are measures() of the CPU fp32 result."""
    B, H, W, h, w = geometry(c)
    s = fwd_input(i, c).numpy()
    out = []
    for b, (new_row, area, K) in enumerate(rows(c[0])):
        ref, scale = pr.forward(s[b], new_row, area, H, W)
        f_whole, f_row = pr.measures(pr.fp32_forward(s[b], new_row, area, H, W), ref, scale)
        out.append((ref, scale, f_whole, f_row))
    return out


# ---------------------------------------------------------------- backward cases
# (route, map, h, w, channels, coff): g is (B, Kmax, coff + C + (32 if coff else 0)) -- coff = 0 means dense rows (ldf == C).
#   ident / cell / wide / strided / generic: ops.upsample_bwd_fused, the route of wesup_upsample_bwd the shape reaches;
#   group: ops.upsample_bwd_fused_group with a channel list; unfused: ops.upsample_bwd on a random dfm; pool: ops.sp_pool_bwd.
BWD = [
    ('ident', 'vor96', 0, 0, 32, 0), ('ident', 'vor96', 0, 0, 256, 32), ('ident', 'lensP', 0, 0, 64, 0), ('ident', 'vor96', 0, 0, 512, 0),
    ('cell', 'vor96', 48, 48, 64, 32), ('cell', 'vor96', 24, 24, 128, 0), ('cell', 'vor96', 6, 6, 256, 0),      # ratio 2, 4, 16
    ('cell', 'vor96', 3, 3, 32, 0), ('cell', 'vor32', 1, 1, 64, 0), ('cell', 'vor96', 1, 48, 32, 32),            # ratio 32, one cell
    ('cell', 'ms156', 39, 58, 64, 0), ('cell', 'ms156', 9, 14, 256, 32), ('cell', 'vor480', 30, 30, 64, 0),
    ('cell', 'vor480', 15, 15, 128, 0), ('cell', 'skewS', 30, 25, 32, 0), ('cell', 'lensP', 64, 64, 64, 0),
    ('wide', 'vor96', 24, 24, 512, 0), ('strided', 'vor96', 24, 24, 512, 32),                                    # the same data
    ('wide', 'vor96', 12, 12, 768, 0), ('wide', 'vor96', 6, 6, 320, 0), ('generic', 'vor96', 12, 12, 1024, 0),
    ('generic', 'vor32', 1, 1, 1024, 0),
    ('group', 'vor96', 24, 24, (64,), 0), ('group', 'vor96', 24, 24, (128, 128), 0), ('group', 'vor96', 24, 24, (256, 256, 256), 0),
    ('group', 'vor96', 24, 24, (32, 256), 0), ('group', 'vor96', 3, 3, (128, 128), 0), ('group', 'ms156', 39, 58, (256, 256, 256), 0),
    ('group', 'vor96', 1, 96, (32, 256), 0),
    ('unfused', 'vor96', 48, 48, 64, 32), ('unfused', 'vor32', 1, 1, 32, 0), ('unfused', 'vor96', 6, 6, 128, 0),
    ('unfused', 'ms156', 39, 58, 32, 32), ('unfused', 'vor96', 0, 0, 32, 0),
    ('pool', 'vor96', 0, 0, 64, 0), ('pool', 'lensP', 0, 0, 32, 0), ('pool', 'skew', 0, 0, 128, 0),
]
SENTINEL_G = 1e30        # rows of g beyond n_sp, and the columns outside the slice: no pixel refers to them


def bwd_id(c):
    route, mp, h, w, C, coff = c
    cs = 'x'.join(str(v) for v in C) if isinstance(C, tuple) else str(C)
    return f"{route}-{mp}-{'native' if h == 0 else f'{h}x{w}'}-C{cs}-off{coff}"


def bwd_input(i, c):
    """The gradient rows (B, Kmax, sum C) of a case (zero-mean for every third case), or a (B, H, W, C) dfm for 'unfused'.
    'wide' and 'strided' of one shape share their data."""
    route, mp, h, w, C, coff = c
    m = label_map(mp)
    B, H, W = m['labels'].shape
    Ct = sum(C) if isinstance(C, tuple) else C
    seed = 2000 + (Ct * 1000 + (h or H)) if route in ('wide', 'strided') else 3000 + i
    zm = i % 3 == 0 and route not in ('wide', 'strided')
    return pr.relu_like(seed, (B, H, W, Ct) if route == 'unfused' else (B, m['Kmax'], Ct), zero_mean=zm)


def bwd_reference(i, c):
    """Per image: (ref64, scale, fp32 whole, fp32 per-cell) with ref64 (h, w, C) -- (HW, C) for 'pool'."""
    route, mp, _, _, C, coff = c
    B, H, W, h, w = geometry((mp, c[2], c[3]))
    x = bwd_input(i, c).numpy()
    out = []
    for b, (new_row, area, K) in enumerate(rows(mp)):
        if route == 'unfused':
            ref = pr.up_adjoint(x[b], H, W, h, w)
            scale = pr.up_adjoint(np.abs(x[b]), H, W, h, w).max(axis=2)
            f = pr.fp32_up_adjoint(x[b], H, W, h, w)
        elif route == 'pool':
            ref = pr.pool_bwd(x[b, :K], new_row, area)
            scale = np.abs(ref).max(axis=1)
            f = pr.fp32_pool_bwd(x[b, :K], new_row, area)
        else:
            ref, scale = pr.adjoint(x[b, :K], new_row, area, H, W, h, w)
            f = pr.fp32_adjoint(x[b, :K], new_row, area, H, W, h, w)
        out.append((ref, scale) + pr.measures(f, ref, scale))
    return out


def bwd_cap(c):
    return pr.CAP_POOL if c[0] == 'pool' else pr.CAP_FUSED
