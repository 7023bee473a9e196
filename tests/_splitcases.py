"""Shared cases of the split tests (tests/test_split_cpu.py, tests/test_split_gpu.py): masks, seeds, the scene of two merged
discs and the four properties of the cut."""
import numpy as np
from scipy import ndimage

from wesup_amd import split
from wesup_amd.utils import metrics as M

RADII = (1, 2, 3, 17, 255)
EDT_CASES = ((37, 53, 0.2), (70, 300, 0.02), (64, 64, 0.001), (5, 7, 0.3))     # H, W, density of zeros


def random_mask(h, w, zero_density, seed):
    """A mask with at least one zero."""
    rng = np.random.default_rng(seed)
    F = rng.random((h, w)) >= zero_density
    if F.all():
        F[rng.integers(h), rng.integers(w)] = False
    return F.astype(np.uint8)


def serpentine(h=41, w=67):
    """Even rows set across the full width, joined at alternating ends by one pixel in the odd rows: one long corridor."""
    F = np.zeros((h, w), np.uint8)
    F[0::2] = 1
    for i, y in enumerate(range(1, h, 2)):
        F[y, w - 1 if i % 2 == 0 else 0] = 1
    return F


def serpentine_ends(F):
    h, w = F.shape
    n_turns = (h - 1) // 2
    return (0, 0), (h - 1, w - 1 if n_turns % 2 == 0 else 0)


def disc_scene():
    """Two discs of radius 24 at (40, 45) and (40, 100) in 80 x 150; the prediction is their union dilated four times: one blob."""
    yy, xx = np.mgrid[:80, :150]
    gt = np.zeros((80, 150), np.int32)
    gt[(yy - 40) ** 2 + (xx - 45) ** 2 <= 24 * 24] = 1
    gt[(yy - 40) ** 2 + (xx - 100) ** 2 <= 24 * 24] = 2
    pred = ndimage.binary_dilation(gt > 0, iterations=4).astype(np.uint8)
    return pred, gt


def random_seeds(F, n, seed):
    """About n random pixels (wherever they fall) with random positive labels up to 2^30, no two within Chebyshev distance 3 of
    each other.  'No seed pixel is cut' needs that much room: a neighbour q of a seed pixel p is labelled by round 2 at the
    latest, from a seed pixel within distance 1 (round 1, 4-neighbourhood) or 2 (round 2) of q, so only a seed within distance
    3 of p can hand q a smaller label than p's (test_close_seeds_cut_the_larger_one shows it happening at distance 2)."""
    rng = np.random.default_rng(seed)
    S = np.zeros(F.shape, np.int32)
    h, w = F.shape
    for p in rng.choice(h * w, size=n, replace=False):
        y, x = divmod(int(p), w)
        if not S[max(y - 3, 0):y + 4, max(x - 3, 0):x + 4].any():
            S[y, x] = rng.integers(1, 2 ** 30, endpoint=True)
    return S


def seeds_apart(seeds):
    """No two pixels of different positive labels within Chebyshev distance 3 (the room 'no seed pixel is cut' needs)."""
    S = np.asarray(seeds).astype(np.int64)
    for dy in range(-3, 4):
        for dx in range(-3, 4):
            n = split._shifted(S, dy, dx)
            if ((S > 0) & (n > 0) & (n != S)).any():
                return False
    return True


def check_properties(F, seeds, L, out):
    """The four consequences of the cut, for one image."""
    F = np.asarray(F) != 0
    seeded = F & (np.asarray(seeds) > 0)
    assert seeds_apart(np.where(seeded, seeds, 0)), 'the seeds of this case are too close for the second property'
    assert not (out.astype(bool) & ~F).any(), 'out is not a subset of the mask'
    assert out[seeded].all(), 'a seed pixel was cut'
    comp = M.label(out)
    for c in range(1, int(comp.max()) + 1):
        labs = np.unique(L[comp == c])
        assert (labs > 0).sum() <= 1, f'component {c} carries the labels {labs}'
    compF = M.label(F)
    with_seed = np.unique(compF[seeded])
    unseeded = F & ~np.isin(compF, with_seed)
    assert (L[unseeded] == 0).all() and out[unseeded].all(), 'a component without a seed was changed'
    assert (L[F & ~unseeded] > 0).all(), 'a pixel of a seeded component has no label at the fixed point'
    assert (L[~F] == 0).all()


def write_scene(tmp_path):
    from PIL import Image
    pred, gt = disc_scene()
    (tmp_path / 'pred').mkdir()
    (tmp_path / 'gt').mkdir()
    Image.fromarray(pred * 255).save(tmp_path / 'pred' / 'scene.png')
    Image.fromarray(gt.astype(np.uint8)).save(tmp_path / 'gt' / 'scene.png')
    return tmp_path / 'pred', tmp_path / 'gt'
