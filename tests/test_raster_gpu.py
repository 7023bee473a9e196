"""Polygon fill on the device (csrc/raster.hip) against wesup_amd/raster.py:fill_host: every word of labels, out8
and status is equal -- the work is integer and its result is defined by the data, so there is no tolerance -- and the guard band
behind every output keeps its sentinel.  Cases: the named and random cases of the host tests; features one pixel narrower than,
equal to and one pixel wider than a tile, in columns and in rows, on and off the tile lattice; rings with more edges than a block
has threads (a serpentine's outline by its corners and with every crack a vertex, a saw-tooth of more than 2048 true vertices); 70 000 one-pixel features (the
feature and tile counts pass 65 535); features whose tiles all lie outside; refused features beside painted ones; F = 0.  The
constants come from _lib, never from the code under test."""
import functools
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _contourcases as CC                                                                   # noqa: E402
from _rastercases import constant_cases, fx, named_cases, one_pixel_features, random_cases  # noqa: E402
from wesup_amd import _lib                                                                   # noqa: E402
from wesup_amd import contour as C                                                           # noqa: E402
from wesup_amd import raster as R                                                            # noqa: E402

pytestmark = pytest.mark.gpu

DEV = 'cuda:0'
SENTINEL = 0x5a5a5a5a
GUARD = 4096               # words (bytes for out8) behind every output that no call may touch

CASES = {**named_cases(), **random_cases(), **constant_cases(_lib.RASTER_TILE_ROWS, _lib.RASTER_TILE_COLS, _lib.RASTER_BLOCK)}


def _serpentine_csr():
    lab = np.zeros((66, 64), np.int32)
    lab[:64] = CC.serpentine(64)
    lab[65, 63] = 2
    return R.pack(C.polygons(*C.trace_host(lab)[:2])), lab


def _raw_fill(csr, shape, values):
    """The entry itself with a guard band behind labels, out8 and status -> (status words, labels, out8) incl. the bands."""
    from wesup_amd import ops
    B, H, W = shape
    t = [torch.from_numpy(np.ascontiguousarray(a)).to(DEV) for a in csr[:4]]
    F, Rn, V = t[3].numel(), t[1].numel() - 1, t[0].shape[0]
    n = B * H * W
    labels = torch.full((n + GUARD,), SENTINEL, dtype=torch.int32, device=DEV)
    status = torch.full((2,), SENTINEL, dtype=torch.int32, device=DEV)
    out8 = val = None
    if values is not None:
        val = torch.from_numpy(np.ascontiguousarray(values)).to(DEV)
        out8 = torch.full((n + GUARD,), 0x5a, dtype=torch.uint8, device=DEV)
    nb = _lib.load().wesup_polygon_fill_workspace_bytes(B, H, W, F)
    assert nb > 0
    ws = torch.empty(nb, dtype=torch.uint8, device=DEV)
    _lib.call('wesup_polygon_fill', ops._p(t[0]), ops._p(t[1]), ops._p(t[2]), ops._p(t[3]), ops._p(val), ops._p(labels), ops._p(out8),
              ops._p(status), B, H, W, F, Rn, V, ops._p(ws), nb, ops._stream())
    torch.cuda.synchronize()
    return status.cpu().numpy(), labels.cpu().numpy(), (None if out8 is None else out8.cpu().numpy())


def _check(csr, shape, values, expect):
    e_labels, e_out8, e_status = expect
    n = int(np.prod(shape))
    status, labels, out8 = _raw_fill(csr, shape, values)
    assert status.tolist() == [e_status, SENTINEL]
    bad = np.argwhere(labels[:n].reshape(shape) != e_labels.reshape(shape))
    assert len(bad) == 0, f'{len(bad)} differing pixels, the first (image, row, column): {bad[:8].tolist()}'
    assert (labels[n:] == SENTINEL).all()
    if values is not None:
        assert (out8[:n].reshape(shape) == e_out8.reshape(shape)).all() and (out8[n:] == 0x5a).all()


@functools.lru_cache(maxsize=None)
def _host(name):
    feats, shape = CASES[name]
    p = R.pack(feats)
    out = R.fill_host(p.verts, p.ring_first, p.feature_first_ring, p.feature_image, shape, p.values)
    out[0].setflags(write=False)
    return p, out


def test_the_constants_are_the_library_s():
    h = _lib.load()
    assert [h.wesup_raster_limit(k) for k in range(5)] == [_lib.RASTER_TILE_ROWS, _lib.RASTER_TILE_COLS, _lib.RASTER_BLOCK,
                                                           _lib.RASTER_COORD_MAX, _lib.RASTER_FRAC_BITS]
    saw = CASES['saw'][0][0]['rings_fixed'][0]
    assert len(saw) > 2048 and len(saw) > 8 * _lib.RASTER_BLOCK
    for name in ('minus', 'equal', 'plus'):                                  # the cases do span one and two tiles
        lab = _host(f'cols_{name}')[1][0][0]
        assert (lab[0] == 1).sum() == _lib.RASTER_TILE_COLS + {'minus': -1, 'equal': 0, 'plus': 1}[name]
        lab = _host(f'rows_{name}')[1][0][0]
        assert (lab[:, 0] == 1).sum() == _lib.RASTER_TILE_ROWS + {'minus': -1, 'equal': 0, 'plus': 1}[name]
    assert not (_host('all_tiles_outside')[1][0] == 1).any() and (_host('all_tiles_outside')[1][0] == 2).any()


@pytest.mark.parametrize('name', list(CASES))
def test_fill_equals_fill_host(name):
    p, expect = _host(name)
    _check(p, CASES[name][1], p.values, expect)


def _unit_steps(ring):
    """Every unit crack of an outline as a vertex: the corners and the lattice points between them."""
    out = []
    for p, q in zip(ring, np.roll(ring, -1, axis=0)):
        n = int(np.abs(q - p).max())
        out += [p + (q - p) // n * k for k in range(n)]
    return np.array(out)


def test_labels_alone_and_rings_longer_than_a_block():
    """The serpentine's outline, over 2048 cracks: by its corners, and with every crack a vertex (runs of collinear vertices,
    more than eight per thread of a block); labels only, no class table."""
    p, lab = _serpentine_csr()
    polys = C.polygons(*C.trace_host(lab)[:2])
    assert C.trace_host(lab)[0][0, 4] > 2048
    expect = R.fill_host(*p[:4], (1,) + lab.shape)
    assert (expect[0][0] == lab).all()
    _check(p, (1,) + lab.shape, None, expect)
    long = R.pack([{'rings': [_unit_steps(q['outer'])] + [_unit_steps(h) for h in q['holes']]} for q in polys])
    assert long.ring_first[1] - long.ring_first[0] == C.trace_host(lab)[0][0, 4] > 8 * _lib.RASTER_BLOCK
    assert (R.fill_host(*long[:4], (1,) + lab.shape)[0] == expect[0]).all()
    _check(long, (1,) + lab.shape, None, expect)


def test_seventy_thousand_features_pass_every_grid_limit():
    csr = one_pixel_features(70000, 265)
    expect = R.fill_host(*csr[:4], (1, 265, 265), csr[4])
    assert expect[2] == 0 and (expect[0].ravel()[:70000] == np.arange(1, 70001)).all()
    _check(csr, (1, 265, 265), csr[4], expect)


def test_refused_features_paint_nothing_beside_painted_ones():
    far = R.COORD_MAX + 1
    verts = np.concatenate([fx([(0, 0), (3, 0), (3, 3), (0, 3)]), np.array([[0, 0], [far, 0], [0, 512]], np.int32),
                            fx([(1, 1), (5, 1), (5, 5)]), fx([(2, 0), (6, 0), (6, 2)])]).astype(np.int32)
    rf, fr = np.array([0, 4, 7, 10, 13], np.int32), np.arange(5, dtype=np.int32)
    val = np.array([9, 8, 7, 6], np.uint8)
    inside = verts.copy()
    inside[5, 0] = 0
    for v, ring_first, ffr, image in ((verts, rf, fr, [0, 0, 2, 1]),                  # a far vertex, an image index at B
                                      (verts, rf, fr, [1, 0, -1, 0]),
                                      (inside, [0, 4, 2, 10, 13], fr, [0, 0, 0, 0]),    # vertex offsets that decrease
                                      (inside, [0, 4, 7, 10, 14], fr, [0, 0, 0, 1]),    # ... that end behind V
                                      (inside, rf, [0, 1, 3, 2, 4], [0, 1, 0, 0]),      # ring offsets that decrease
                                      (inside, rf, [0, 1, 2, 3, 5], [0, 0, 0, 0]),      # ... that end behind R
                                      (inside, rf, [0, -1, 2, 3, 4], [0, 0, 0, 0])):
        csr = (v, np.array(ring_first, np.int32), np.array(ffr, np.int32), np.array(image, np.int32))
        expect = R.fill_host(*csr, (2, 6, 7), val)
        assert expect[2] == 1 and expect[0].any()
        _check(csr, (2, 6, 7), val, expect)


def test_no_features_and_no_vertices_give_zeros():
    none = (np.zeros((0, 2), np.int32), np.zeros(1, np.int32), np.zeros(1, np.int32), np.zeros(0, np.int32))
    zeros = (np.zeros((2, 5, 9), np.int32), np.zeros((2, 5, 9), np.uint8), 0)
    _check(none, (2, 5, 9), np.zeros(0, np.uint8), zeros)
    _check(none, (2, 5, 9), None, zeros)
    empty = (np.zeros((0, 2), np.int32), np.zeros(3, np.int32), np.array([0, 1, 2], np.int32), np.array([0, 1], np.int32))
    _check(empty, (2, 5, 9), np.array([3, 4], np.uint8), zeros)


def test_trace_then_fill_on_the_device_gives_the_map_back():
    from wesup_amd import ops
    lab = np.stack([CC.random_map(3, 70, 131, 3), CC.random_map(4, 70, 131, 2), np.zeros((70, 131), np.int32)])
    lab[0, 5:60, 20:120] = 7
    lab[0, 20:40, 40:100] = 0
    t = torch.from_numpy(lab).to(DEV)
    rings, verts, _ = ops.contour_trace(t)
    v, rf, fr, fi, fl = R.rings_to_csr(rings, verts)
    assert all(x.is_cuda and x.dtype == torch.int32 for x in (v, rf, fr, fi, fl))
    labels, out8, status = ops.polygon_fill(v, rf, fr, fi, lab.shape)
    assert labels.is_cuda and out8 is None and int(status.item()) == 0
    back = torch.where(labels > 0, fl[(labels - 1).clamp(min=0).long()], torch.zeros_like(labels))
    assert torch.equal(back, torch.where(t > 0, t, torch.zeros_like(t)))
    img = torch.where(labels > 0, fi[(labels - 1).clamp(min=0).long()], torch.zeros_like(labels))
    assert torch.equal(img, torch.arange(3, device=DEV, dtype=torch.int32).reshape(3, 1, 1).expand_as(labels) * (labels > 0))


def test_wrapper_and_module_paths_equal_the_host():
    from wesup_amd import ops
    name = 'random_33x65_fine'
    p, (e_labels, e_out8, _) = _host(name)
    t = [torch.from_numpy(a).to(DEV) for a in p[:4]]
    labels, out8, status = ops.polygon_fill(*t, (33, 65), torch.from_numpy(p.values).to(DEV))
    assert labels.shape == out8.shape == (33, 65) and labels.dtype == torch.int32 and out8.dtype == torch.uint8 and status.shape == (1,)
    assert (labels.cpu().numpy() == e_labels[0]).all() and (out8.cpu().numpy() == e_out8[0]).all() and int(status.item()) == 0
    feats = CASES[name][0]
    l, o = R.fill(feats, (33, 65), DEV, values=True)
    assert (l == e_labels[0]).all() and (o == e_out8[0]).all()
    cmap = CC.random_map(42, 23, 31, n_labels=3).astype(np.uint8)
    doc = C.to_geojson(C.classmap_polygons(cmap, 4), scale=2.0, offset=(5, 7))
    assert (R.geojson_to_classes(doc, cmap.shape, 2.0, (5, 7), device=DEV) == cmap).all()
    assert (R.geojson_to_mask(doc, cmap.shape, 2.0, (5, 7), device=DEV) == (cmap > 0)).all()
    with pytest.raises(_lib.WesupHipError):
        ops.polygon_fill(t[0], t[1], t[2][:-1], t[3], (33, 65))
