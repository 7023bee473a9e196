"""Surface-distance metrics on the device (csrc/surface.hip) against the numpy definitions of wesup_amd/surface.py:
the distance map, the border, the integer select and the eight integer quantities bit for bit, the two float64 sums within
(n + 2) 2^-52 relative (n non-negative terms, each square root within one ulp, any order of additions)."""
import functools
import math

import numpy as np
import pytest
import torch

from wesup_amd import _lib, evaluate, ops, surface
from wesup_amd.utils import metrics as M

from _surfacecases import blob_pair, blob_pairs, edt_cases, random_mask, rel_sum_bound

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
EDGES = sorted({_lib.EDT_CHUNK, _lib.EDT_COLS, _lib.EDT_SEG, _lib.EDT_ROWS})


def dev(mask):
    return torch.tensor(np.ascontiguousarray(mask)).to(DEV).to(torch.uint8).contiguous()


def edge_shapes():
    """Every (h, w) in {E-1, E, E+1} x {E-1, E, E+1, 2E+1} for each tile constant E of the distance map."""
    return sorted({(h, w) for E in EDGES for h in (E - 1, E, E + 1) for w in (E - 1, E, E + 1, 2 * E + 1)})


@functools.lru_cache(maxsize=None)
def all_masks():
    """(name, mask): the CPU test's cases, the tile edges at two densities, and two maps whose distances pass the old cap."""
    out = list(edt_cases())
    for h, w in edge_shapes():
        out.append((f'edge{h}x{w}', random_mask(h, w, 0.02 if (h + w) % 2 else 0.3, seed=h * 7919 + w)))
    far = np.ones((300, 300), bool)
    far[0, 0] = False
    out.append(('corner300', far))
    one = np.ones((70, 300), bool)
    one[35, 3] = False
    out.append(('one70x300', one))
    tall = np.ones((200, 3), bool)                 # chunks without a zero between chunks with one
    tall[1, 0] = tall[198, 1] = False
    out.append(('tall200x3', tall))
    return tuple(out)


@functools.lru_cache(maxsize=None)
def host_edt(i, invert):
    m = all_masks()[i][1]
    return surface.edt_sq_full_host(~m if invert else m)


@pytest.mark.parametrize('invert', (False, True))
def test_edt_sq_full_equals_host(invert):
    for i, (name, m) in enumerate(all_masks()):
        got = ops.edt_sq_full(dev(m), invert=invert)
        assert got.dtype == torch.int32 and tuple(got.shape) == m.shape
        assert np.array_equal(got.cpu().numpy(), host_edt(i, invert)), (name, invert)


def test_edt_sq_full_beyond_the_old_cap():
    far = dict(all_masks())['corner300']
    got = ops.edt_sq_full(dev(far)).cpu().numpy()
    assert got.max() == 178802 == got[299, 299] and got[0, 0] == 0 and got[0, 299] == 299 * 299
    ones = ops.edt_sq_full(dev(np.ones((5, 9), bool))).cpu().numpy()
    assert (ones == ops.EDT_NONE).all() and ops.EDT_NONE == 2 ** 31 - 1
    assert (ops.edt_sq_full(dev(np.ones((5, 9), bool)), invert=True).cpu().numpy() == 0).all()
    vals = dev(np.array([[0, 1, 2, 255, 0, 7]], np.uint8))                       # any non-zero value is foreground
    assert ops.edt_sq_full(vals).tolist() == [[0, 1, 4, 1, 0, 1]]


def test_bad_arguments_raise():
    m = dev(np.ones((4, 5), bool))
    with pytest.raises(_lib.WesupHipError):
        ops.edt_sq_full(m.to(torch.int32))
    with pytest.raises(_lib.WesupHipError):
        ops.edt_sq_full(m.cpu())
    with pytest.raises(_lib.WesupHipError):
        ops.edt_sq_full(m[None, None])
    with pytest.raises(_lib.WesupHipError):
        ops.edt_sq_full(m[:, ::2])                                               # not contiguous
    with pytest.raises(_lib.WesupHipError):
        ops.edt_sq_full(torch.empty(0, 5, dtype=torch.uint8, device=DEV))
    with pytest.raises(_lib.WesupHipError):
        ops.edt_sq_full(torch.empty(1, 1, 46342, dtype=torch.uint8, device=DEV))  # squared distances would reach 2^31 - 1
    with pytest.raises(_lib.WesupHipError):
        ops.mask_border(m.to(torch.float32))
    with pytest.raises(_lib.WesupHipError):
        ops.surface_stats(m, dev(np.ones((4, 6), bool)), 2.0)
    for tol in (-1.0, math.inf, math.nan):
        with pytest.raises(_lib.WesupHipError):
            ops.surface_stats(m, m, tol)
    with pytest.raises(_lib.WesupHipError):
        ops.surface_stats(m, m, 2.0, q=101.0)
    keys = torch.zeros(8, dtype=torch.int32, device=DEV)
    ranks = torch.zeros(2, dtype=torch.int64, device=DEV)
    with pytest.raises(_lib.WesupHipError):
        ops.select_i32(keys.float(), ranks)
    with pytest.raises(_lib.WesupHipError):
        ops.select_i32(keys, ranks.cpu())
    with pytest.raises(_lib.WesupHipError):
        ops.select_i32(keys, torch.zeros(5, dtype=torch.int64, device=DEV))
    with pytest.raises(_lib.WesupHipError):
        ops.select_i32(keys[:0], ranks)


def test_mask_border_equals_host():
    for name, m in all_masks():
        got = ops.mask_border(dev(m))
        assert got.dtype == torch.uint8 and tuple(got.shape) == m.shape
        assert np.array_equal(got.cpu().numpy().astype(bool), surface.border_host(m)), name
        assert int(got.max()) <= 1


@pytest.mark.parametrize('n', (1, 2, 255, 256, 257, 100003))
def test_select_i32_equals_sort(n):
    rng = np.random.default_rng(n)
    keys = rng.integers(0, 2 ** 31 - 1, size=n, dtype=np.int64)
    special = np.array([0, 0x7F800000, 0x7F800001, 0x7FFFFFFE], np.int64)        # +inf and NaN patterns to a float reader
    if n >= 255:
        keys[rng.choice(n, 4, replace=False)] = special
    ranks = np.array([0, n - 1, n // 3, (2 * n) // 3], np.int64)

    def check(k):
        got = ops.select_i32(torch.tensor(k.astype(np.int32)).to(DEV), torch.tensor(ranks).to(DEV))
        assert got.dtype == torch.int32 and np.array_equal(got.cpu().numpy(), np.sort(k)[ranks])

    check(keys)
    if n < 255:                                                                  # too short to hold all four: each alone, and together
        for v in special:
            k = keys.copy()
            k[0] = v
            check(k)
    check(np.full(n, 0x7F800001, np.int64))                                      # all equal
    check(np.zeros(n, np.int64))
    if n == 257:                                                                 # the four patterns alone, every rank
        got = ops.select_i32(torch.tensor(special[::-1].astype(np.int32).copy()).to(DEV), torch.arange(4, device=DEV))
        assert got.tolist() == special.tolist()
        one = ops.select_i32(torch.tensor(special.astype(np.int32)).to(DEV), torch.tensor([2], device=DEV),
                             out=torch.empty(1, dtype=torch.int32, device=DEV))
        assert one.tolist() == [0x7F800001]


def stat_pairs():
    """The 20 blob pairs and pairs at the edge shapes of the distance map."""
    out = [(f'blob{i}', p, g) for i, (p, g) in enumerate(blob_pairs())]
    for j, (h, w) in enumerate(edge_shapes()):
        if h >= 8 and w >= 8 and j % 3 == 0:
            p, g = blob_pair(100 + j, (h, w))
            out.append((f'edge{h}x{w}', p, g))
    out.append(('tiny3x9', random_mask(3, 9, 0.4, 1), random_mask(3, 9, 0.4, 2)))
    out.append(('one-pixel', np.ones((1, 1), bool), np.ones((1, 1), bool)))
    return out


def check_stats(got, ref, name):
    for k in surface.STAT_KEYS[:8]:
        assert isinstance(got[k], int) and got[k] == ref[k], (name, k, got[k], ref[k])
    for k, n in (('sum_pg', ref['n_p']), ('sum_gp', ref['n_g'])):
        assert isinstance(got[k], float) and abs(got[k] - ref[k]) <= rel_sum_bound(n) * ref[k], (name, k, got[k], ref[k])


def test_surface_stats_equals_host():
    for name, p, g in stat_pairs():
        for tol, q in ((2.0, 95.0), (0.5, 50.0)):
            got = ops.surface_stats(dev(p), dev(g), tol, q)
            assert tuple(got) == surface.STAT_KEYS
            check_stats(got, surface.surface_stats_host(p, g, tol, q), name)
    pairs = blob_pairs()[:5]                                                     # a batch: one chain, the same numbers
    P, G = np.stack([p for p, _ in pairs]), np.stack([g for _, g in pairs])
    rows = ops.surface_stats(dev(P), dev(G), 2.0)
    assert len(rows) == 5
    for i, row in enumerate(rows):
        check_stats(row, surface.surface_stats_host(P[i], G[i], 2.0), f'batch{i}')
    a = ops.surface_stats_blocks(dev(P), dev(G), 2.0).cpu()                      # two runs: the same bits, the sums included
    b = ops.surface_stats_blocks(dev(P), dev(G), 2.0).cpu()
    assert a.dtype == torch.int64 and tuple(a.shape) == (5, 10) and torch.equal(a, b)


def test_surface_stats_empty_borders():
    empty, p = np.zeros((40, 50), bool), blob_pairs()[0][0][:40, :50]
    for a, b in ((empty, empty), (empty, p), (p, empty), (p, p)):
        check_stats(ops.surface_stats(dev(a), dev(b), 2.0), surface.surface_stats_host(a, b, 2.0), 'empty')
        got, ref = surface.surface_scores(a, b, 2.0, device=DEV), surface.surface_scores_host(a, b, 2.0)
        assert got == ref
    assert surface.surface_scores(empty, empty, device=DEV) == {'hd': 0.0, 'hd95': 0.0, 'assd': 0.0, 'nsd': 1.0}
    assert surface.surface_scores(empty, p, device=DEV) == {'hd': math.inf, 'hd95': math.inf, 'assd': math.inf, 'nsd': 0.0}


def check_scores(got, ref, n_terms, name):
    """hd, hd95 and nsd come from integers: equal.  assd is two sums over counts: the bound of the sums."""
    for k in ('hd', 'hd95', 'nsd'):
        assert got[k] == ref[k], (name, k, got[k], ref[k])
    if math.isfinite(ref['assd']):
        assert abs(got['assd'] - ref['assd']) <= rel_sum_bound(n_terms) * ref['assd'], (name, got['assd'], ref['assd'])
    else:
        assert got['assd'] == ref['assd'], name


def n_terms(p, g):
    """The longer of the two sums of an image pair."""
    return int(max(surface.border_host(p).sum(), surface.border_host(g).sum()))


def test_surface_scores_device_equals_host():
    for i, (p, g) in enumerate(blob_pairs()):
        for tol in (2.0, 1.0):
            check_scores(surface.surface_scores(p, g, tol, device=DEV), surface.surface_scores_host(p, g, tol), n_terms(p, g),
                         f'blob{i}')


def test_surface_scores_classes_device_equals_host():
    rng = np.random.default_rng(3)
    gt = np.zeros((64, 48), np.uint8)
    gt[10:40, 5:30] = 1
    gt[30:60, 25:45] = 2
    pred = np.roll(gt, (1, -2), (0, 1))
    pred[rng.random(pred.shape) < 0.01] = 0
    got = surface.surface_scores_classes(pred, gt, 3, 2.0, device=DEV)
    ref = surface.surface_scores_classes_host(pred, gt, 3, 2.0)
    assert len(got) == 3
    for c in range(3):
        check_scores(got[c], ref[c], n_terms(pred == c, gt == c), f'class{c}')
    only = surface.surface_scores_classes(pred, gt, 4, 2.0, device=DEV)[3]        # a class neither map holds
    assert only == {'hd': 0.0, 'hd95': 0.0, 'assd': 0.0, 'nsd': 1.0}


def test_evaluate_score_device_equals_host():
    pairs = blob_pairs()[:4]
    preds = [p.astype(np.float64) for p, _ in pairs] + [np.zeros(pairs[0][0].shape)]
    gts = [M.label(g) for _, g in pairs] + [M.label(pairs[0][1])]
    rows_h, means_h = evaluate.score(preds, gts, surface=2.0)
    rows_d, means_d = evaluate.score(preds, gts, surface=2.0, device=DEV)
    for i, (h, d) in enumerate(zip(rows_h, rows_d)):
        assert list(d) == list(h) and len(d) == 8
        for k in ('hd95', 'nsd'):
            assert d[k] == h[k] or (math.isnan(d[k]) and math.isnan(h[k])), (i, k)
        n = n_terms(preds[i] != 0, gts[i] > 0)
        assert (math.isnan(d['assd']) and math.isnan(h['assd'])) or abs(d['assd'] - h['assd']) <= rel_sum_bound(n) * h['assd'], i
    assert math.isnan(rows_d[4]['hd95']) and rows_d[4]['nsd'] == 0.0
    assert means_d['hd95'] == means_h['hd95'] and means_d['nsd'] == means_h['nsd']
    rows_0, _ = evaluate.score(preds, gts, device=DEV)
    assert all(len(r) == 5 for r in rows_0)


def test_hausdorff_full_device_equals_metrics_hausdorff():
    for i, (p, g) in enumerate(blob_pairs()):
        assert surface.hausdorff_full(p, g, device=DEV) == M.hausdorff(p, g), i
    empty = np.zeros(blob_pairs()[0][0].shape, bool)
    assert surface.hausdorff_full(empty, empty, device=DEV) == 0
    assert surface.hausdorff_full(empty, blob_pairs()[0][0], device=DEV) == np.inf
