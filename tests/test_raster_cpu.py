"""Polygon fill and the GeoJSON reader without a GPU (wesup_amd/raster.py): the scanline form fill_host against
the per-pixel crossing count of tests/_rasterref.py on the named cases and on seeded random polygons (3 - 12 vertices on the
1/256, half-pixel and integer grids, reaching 3 pixels outside, at 1 x 1, 1 x 257, 257 x 1, 17 x 15, 33 x 65 and 40 x 40); the
round trip label map -> trace -> polygons -> fill, directly and through GeoJSON with a scale and an offset; the reader, the
command line, and the library's new entries on the host.  Everything is integer: every comparison is exact."""
import ctypes
import functools
import json
import os
import re
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _contourcases as CC                                                                   # noqa: E402
from _rastercases import constant_cases, fx, named_cases, one_pixel_features, random_cases  # noqa: E402
from _rasterref import labels_ref                                                            # noqa: E402
from wesup_amd import contour as C                                                           # noqa: E402
from wesup_amd import raster as R                                                            # noqa: E402
from wesup_amd.utils import metrics as M                                                     # noqa: E402

CASES = {**named_cases(), **random_cases()}


@functools.lru_cache(maxsize=None)
def _host(name):
    feats, shape = CASES[name]
    p = R.pack(feats)
    labels, out8, status = R.fill_host(p.verts, p.ring_first, p.feature_first_ring, p.feature_image, shape, p.values)
    labels.setflags(write=False)
    return labels, out8, status, p


@pytest.mark.parametrize('name', list(CASES))
def test_scanline_fill_equals_the_crossing_count(name):
    feats, shape = CASES[name]
    labels, out8, status, p = _host(name)
    ref = labels_ref(feats, shape)
    assert status == 0 and labels.dtype == np.int32 and labels.shape == shape and out8.dtype == np.uint8
    bad = np.argwhere(labels != ref)
    assert len(bad) == 0, f'first differing pixels (image, row, column): {bad[:8].tolist()}'
    assert (out8 == np.concatenate([[0], p.values])[ref]).all()


def test_the_named_cases_are_what_they_claim():
    lab = lambda name: _host(name)[0][0]
    assert lab('unit_square').tolist() == [[1, 0, 0], [0, 0, 0], [0, 0, 0]]
    assert np.argwhere(lab('centre_square')).tolist() == [[0, 0], [0, 1], [1, 0], [1, 1]]      # top and left in, bottom and right out
    # the top vertex lies on a centre: both of its edges toggle there and cancel; the bottom vertex is excluded
    assert lab('diamond').tolist() == [[0, 0, 0, 0, 0, 0], [0, 1, 1, 0, 0, 0], [1, 1, 1, 1, 0, 0], [0, 1, 1, 0, 0, 0],
                                       [0, 0, 0, 0, 0, 0], [0, 0, 0, 0, 0, 0]]
    assert not lab('sliver').any()
    assert lab('edge_on_centre_row').tolist() == [[1, 1, 1, 0], [1, 1, 1, 0], [0, 0, 0, 0], [0, 0, 0, 0]]
    # the wings at the left and the right; the wedges above and below the crossing are outside
    assert lab('bow_tie').tolist() == [[0, 0, 0, 1, 0], [1, 0, 1, 1, 0], [1, 0, 1, 1, 0], [0, 0, 0, 1, 0], [0, 0, 0, 0, 0]]
    h = lab('hole_and_island')
    assert h[0, 0] == 1 and h[2, 2] == 0 and h[3, 3] == 2 and h[5, 5] == 0 and h[6, 6] == 1 and (h[8] == 0).all()
    assert lab('overlap_ab')[3, 3] == 2 and lab('overlap_ba')[3, 3] == 2 and lab('overlap_ab')[1, 1] == 1 and lab('overlap_ba')[5, 5] == 1
    assert ((lab('overlap_ab') > 0) == (lab('overlap_ba') > 0)).all()
    assert _host('overlap_ab')[1][0, 3, 3] == 2 and _host('overlap_ba')[1][0, 3, 3] == 1       # the class of the later feature
    d = lab('degenerate')
    assert sorted(np.unique(d).tolist()) == [0, 3, 4] and (d[:4, :4] == 3).all() and (d[:4, 5:9] == 4).all() and not d[:, 9:].any()
    assert lab('whole_image').all() and lab('far_triangle').any() and not lab('far_triangle').all()
    assert np.abs(np.diff((lab('comb40')[3] > 0).astype(int), prepend=0)).sum() == 80           # 40 teeth: 80 crossings in the row
    for side in ('left', 'right', 'top', 'bottom'):
        assert not lab(f'outside_{side}').any()
        s = lab(f'straddle_{side}')
        edge = {'left': s[:, 0], 'right': s[:, -1], 'top': s[0], 'bottom': s[-1]}[side]
        assert edge.any() and 0 < s.sum() < 3 * 4
    b = _host('batch3')[0]
    assert b[0].any() and not b[1].any() and set(np.unique(b[2]).tolist()) == {0, 2, 3}
    assert all(np.asarray(f['rings_fixed'][0]).shape[0] > 2048 for f in constant_cases(64, 64, 256)['saw'][0])


def test_fill_is_the_same_tile_by_tile():
    """Clamping c* to the left edge of a rectangle keeps the parity inside it: the fill of a shifted window equals the window of
    the fill (what lets the device fill every tile of a bounding box on its own)."""
    feats, (_, H, W) = CASES['random_33x65_fine']
    whole = _host('random_33x65_fine')[0][0]
    for r0, c0, h, w in ((0, 0, 33, 65), (5, 7, 11, 13), (20, 64, 13, 1), (32, 0, 1, 65)):
        moved = [{'image': 0, 'rings_fixed': [np.asarray(r) - np.array([256 * c0, 256 * r0]) for r in f['rings_fixed']]} for f in feats]
        assert (R.fill(moved, (h, w)) == whole[r0:r0 + h, c0:c0 + w]).all()


def test_refused_features_paint_nothing_and_set_the_status():
    far = R.COORD_MAX + 1
    verts = np.concatenate([fx([(0, 0), (3, 0), (3, 3), (0, 3)]), np.array([[0, 0], [far, 0], [0, 512]], np.int32),
                            fx([(1, 1), (5, 1), (5, 5)]), fx([(2, 0), (6, 0), (6, 2)])]).astype(np.int32)
    ring_first = np.array([0, 4, 7, 10, 13], np.int32)
    ffr = np.arange(5, dtype=np.int32)
    for image, expect in (([0, 0, 1, 0], {0, 1, 4}), ([0, 0, -1, 0], {0, 1, 4}), ([0, 0, 0, 0], {0, 1, 3, 4})):
        labels, _, status = R.fill_host(verts, ring_first, ffr, np.array(image, np.int32), (6, 7))
        assert status == 1 and set(np.unique(labels).tolist()) == expect
    # offsets that decrease or leave their table: only the features that hold them are refused
    img = np.zeros(4, np.int32)
    v = verts.copy()
    v[5, 0] = 0                                                                       # (the far vertex back inside)
    for rf, fr, refused in (([0, 4, 2, 10, 13], [0, 1, 2, 3, 4], {1}),               # ring 1 = [4, 2); ring 2 = [2, 10) is in order
                            ([0, 4, 7, 10, 14], [0, 1, 2, 3, 4], {3}),               # the last ring ends behind V
                            ([0, 4, 7, 10, 13], [0, 1, 3, 2, 4], {2}),               # feature 1 = rings [1, 3), 2 = [3, 2), 3 = [2, 4)
                            ([0, 4, 7, 10, 13], [0, 1, 2, 3, 5], {3}),
                            ([0, 4, 7, 10, 13], [0, -1, 2, 3, 4], {0, 1}),
                            ([-1, 4, 7, 10, 13], [0, 1, 2, 3, 4], {0})):
        labels, _, status = R.fill_host(v, np.array(rf, np.int32), np.array(fr, np.int32), img, (6, 7))
        kept = [{'rings_fixed': [] if f in refused else [v[rf[k]:rf[k + 1]] for k in range(fr[f], fr[f + 1])]} for f in range(4)]
        assert status == 1 and (labels == R.fill(kept, (6, 7))).all(), (rf, fr)
        assert not np.isin(labels, [f + 1 for f in refused]).any() and len(np.unique(labels)) > 2
    labels, out8, status = R.fill_host(np.zeros((0, 2), np.int32), [0], [0], [], (2, 3, 4), np.zeros(0, np.uint8))
    assert status == 0 and labels.shape == out8.shape == (2, 3, 4) and not labels.any() and not out8.any()


def test_many_one_pixel_features():
    verts, rf, fr, img, val = one_pixel_features(300, 17)
    labels, out8, status = R.fill_host(verts, rf, fr, img, (18, 17), val)
    assert status == 0 and (labels.ravel()[:300] == np.arange(1, 301)).all() and not labels.ravel()[300:].any()
    assert (out8.ravel()[:300] == val).all()


# ------------------------------------------------------------------------------------------------- round trips
def _one_object_per_label(a):
    """Relabel so that every label is one 8-connected object (what contour.polygons asks for)."""
    out = np.zeros(a.shape, np.int32)
    for l in np.unique(a[a > 0]).tolist():
        comp = M.label(a == l)
        out[comp > 0] = comp[comp > 0] + out.max()
    return out


ROUND = dict(CC.named_cases())
for _k, (_h, _w) in enumerate([(16, 16), (17, 15), (1, 257), (257, 1), (33, 65), (40, 40)]):
    ROUND[f'mask_{_h}x{_w}'] = CC.random_map(10 + _k, _h, _w)
    ROUND[f'labels_{_h}x{_w}'] = CC.random_map(20 + _k, _h, _w, n_labels=3)
ROUND['checker_31x33'] = CC.checkerboard(31, 33)
ROUND['isolated_257'] = CC.isolated_pixels(257)
ROUND['serpentine'] = CC.serpentine(64)


@pytest.mark.parametrize('name', list(ROUND))
def test_trace_then_fill_gives_the_map_back(name):
    lab = _one_object_per_label(ROUND[name])
    polys = C.polygons(*C.trace_host(lab)[:2])
    expect = np.zeros(lab.shape, np.int32)
    for i, p in enumerate(polys):
        expect[lab == p['label']] = i + 1
    assert len(polys) == lab.max() and (R.fill(polys, lab.shape) == expect).all()
    # ... and through GeoJSON, with a scale and an offset
    doc = json.loads(json.dumps(C.to_geojson(polys, scale=2.5, offset=(100, -40))))
    feats, points, skipped = R.read_geojson(doc, scale=2.5, offset=(100, -40))
    assert len(feats) == len(polys) and not points and not skipped
    for f, p in zip(feats, polys):
        assert len(f['rings_fixed']) == 1 + len(p['holes']) and (f['rings_fixed'][0] == 256 * p['outer']).all()
    assert (R.fill(feats, lab.shape) == expect).all()
    assert (R.geojson_to_labels(doc, lab.shape, 2.5, (100, -40)) == expect).all()
    mask = C.geojson_to_mask_host(doc, lab.shape, 2.5, (100, -40))
    assert (R.geojson_to_mask(doc, lab.shape, 2.5, (100, -40)) == mask).all() and (mask == (lab > 0)).all()


def test_classmap_round_trip():
    cmap = CC.random_map(42, 23, 31, n_labels=3).astype(np.uint8)
    polys = C.classmap_polygons(cmap, 4)
    assert (R.fill(polys, cmap.shape, values=True)[1] == cmap).all()
    doc = C.to_geojson(polys)                                                # 'class k' names
    assert (R.geojson_to_classes(doc, cmap.shape) == cmap).all()
    names = ['background', 'stroma', 'gland', 'tumour']
    doc = C.to_geojson(polys, class_names=names)
    assert (R.geojson_to_classes(doc, cmap.shape, class_names=names) == cmap).all()
    with pytest.raises(ValueError, match='gland|stroma|tumour'):
        R.geojson_to_classes(doc, cmap.shape, class_names=['background'])
    with pytest.raises(ValueError, match='give class_names'):
        R.geojson_to_classes(doc, cmap.shape)
    assert (R.geojson_to_mask(doc, cmap.shape) == (cmap > 0)).all()          # masks and instance maps do not look at the names


# ------------------------------------------------------------------------------------------------- the reader
def _feature(geometry, name=None):
    props = {} if name is None else {'classification': {'name': name}}
    return {'type': 'Feature', 'geometry': geometry, 'properties': props}


def test_reader_takes_collections_lists_and_single_features():
    sq = [[1, 1], [4, 1], [4, 3], [1, 3], [1, 1]]
    poly = _feature({'type': 'Polygon', 'coordinates': [sq]})
    for doc in ({'type': 'FeatureCollection', 'features': [poly]}, [poly], poly):
        feats, points, skipped = R.read_geojson(doc)
        assert len(feats) == 1 and feats[0]['class'] == 1 and not points and skipped == 0
        assert feats[0]['rings_fixed'][0].tolist() == [[256, 256], [1024, 256], [1024, 768], [256, 768]]     # the closing vertex is dropped
    tri_open = [[5.5, 0.5], [7.5, 0.5], [5.5, 2.5]]                                                             # not closed: kept whole
    multi = _feature({'type': 'MultiPolygon', 'coordinates': [[sq, [[2, 1.5], [3, 1.5], [3, 2.5], [2, 2.5], [2, 1.5]]], [tri_open]]},
                     'gland')
    feats, _, _ = R.read_geojson([poly, multi], class_names=['background', 'stroma', 'gland'])
    assert [f['class'] for f in feats] == [1, 2] and [len(r) for r in feats[1]['rings_fixed']] == [4, 4, 3]
    lab, cls = R.fill(feats, (4, 9), values=True)
    # the hole of the second feature shows the first one; the hole's bottom row is outside it (exclusive)
    assert lab[1, 1] == 2 and lab[1, 2] == 1 and lab[2, 2] == 2 and lab[0, 5] == 2 and lab[0, 6] == 2 and lab[1, 5] == 2
    assert cls[1, 1] == 2 and cls[1, 2] == 1 and lab[3].sum() == 0
    with pytest.raises(ValueError, match="'lumen'"):
        R.read_geojson([_feature({'type': 'Polygon', 'coordinates': [sq]}, 'lumen')], class_names=['background', 'gland'])
    assert R.read_geojson([_feature({'type': 'Polygon', 'coordinates': [sq]}, 'class 7')])[0][0]['class'] == 7
    # a third coordinate is ignored; scale and offset are undone
    f3 = _feature({'type': 'Polygon', 'coordinates': [[[110, -30, 9], [120, -30, 9], [120, -20, 9], [110, -20, 9]]]})
    assert R.read_geojson(f3, scale=2.5, offset=(100, -40))[0][0]['rings_fixed'][0].tolist() == \
        [[1024, 1024], [2048, 1024], [2048, 2048], [1024, 2048]]


def test_reader_points_lines_and_range(tmp_path):
    from wesup_amd.utils.data import PointSupervisionDataset
    from PIL import Image
    doc = {'type': 'FeatureCollection', 'features': [
        _feature({'type': 'Point', 'coordinates': [12.75, 3.25]}, 'gland'),
        _feature({'type': 'LineString', 'coordinates': [[0, 0], [5, 5]]}),
        _feature({'type': 'MultiPoint', 'coordinates': [[0.5, 0.999], [7, 8]]}),
        _feature({'type': 'GeometryCollection', 'geometries': []}),
        _feature(None)]}
    feats, points, skipped = R.read_geojson(doc, class_names=['background', 'other', 'gland'])
    assert not feats and skipped == 3 and points == [(12.75, 3.25, 2), (0.5, 0.999, 1), (7.0, 8.0, 1)]
    assert R.point_rows(points).tolist() == [[12, 3, 2], [0, 0, 1], [7, 8, 1]]
    assert R.point_rows(R.read_geojson(doc, scale=0.5, offset=(-1, 1), class_names=['b', 'o', 'gland'])[1]).tolist() == \
        [[27, 4, 2], [3, -1, 1], [16, 14, 1]]
    assert R.point_rows([]).shape == (0, 3)
    root = tmp_path / 'train'
    (root / 'images').mkdir(parents=True)
    Image.fromarray(np.zeros((16, 20, 3), np.uint8)).save(root / 'images' / 'a.png')
    R.write_points(root / 'points' / 'a.csv', points)
    ds = PointSupervisionDataset(root, train=False)
    pts = ds[0][2].numpy()
    assert pts[:3].tolist() == [[12, 3, 2], [0, 0, 1], [7, 8, 1]] and (pts[3:] == -1).all()
    for bad in ([[0, 0], [2 ** 20 + 1, 0], [0, 5]], [[0, 0], [float('nan'), 0], [0, 5]], [[0, -2.0 ** 20 - 1], [4, 0], [0, 5]]):
        with pytest.raises(ValueError, match='range'):
            R.read_geojson(_feature({'type': 'Polygon', 'coordinates': [bad]}))
    assert R.to_fixed([[2 ** 20, -2 ** 20]]).tolist() == [[2 ** 28, -2 ** 28]]                   # the limit itself is inside
    assert R.to_fixed([[0.5 / 256, 0.499 / 256], [-0.5 / 256, -0.501 / 256]]).tolist() == [[1, 0], [0, -1]]      # floor(v + 0.5)


# ------------------------------------------------------------------------------------------------- the command line
def test_command_line_every_mode(tmp_path):
    from PIL import Image
    cmap = CC.random_map(43, 21, 27, n_labels=2).astype(np.uint8)
    names = ['background', 'gland', 'tumour']
    polys = C.classmap_polygons(cmap, 3)
    ann, img = tmp_path / 'ann', tmp_path / 'images'
    img.mkdir()
    doc = C.to_geojson(polys, class_names=names)
    doc['features'].append(_feature({'type': 'Point', 'coordinates': [3.5, 4.5]}, 'tumour'))
    doc['features'].append(_feature({'type': 'LineString', 'coordinates': [[0, 0], [1, 1]]}))
    ann.mkdir()
    (ann / 'a.geojson').write_text(json.dumps(doc))
    Image.fromarray(np.zeros((21, 27, 3), np.uint8)).save(img / 'a.jpg')
    R.main([str(ann), str(tmp_path / 'classes'), '--images', str(img), '--classes', ','.join(names), '--points', str(tmp_path / 'points')])
    assert (np.asarray(Image.open(tmp_path / 'classes' / 'a.png')) == cmap).all()
    assert (tmp_path / 'points' / 'a.csv').read_text().split() == ['3,4,2']
    R.main([str(ann), str(tmp_path / 'labels'), '--shape', '21', '27', '--labels'])
    inst = np.asarray(Image.open(tmp_path / 'labels' / 'a.png'))
    expect = np.zeros(cmap.shape, np.int32)
    for i, p in enumerate(polys):
        expect[(M.label(cmap == p['class']) == p['label'])] = i + 1
    assert inst.dtype == np.uint16 and (inst == expect).all()
    # binary: unclassified annotations give a 0 / 1 map; scale and offset are undone
    (ann / 'a.geojson').write_text(json.dumps(C.to_geojson(C.mask_polygons(cmap > 0), scale=4.0, offset=(8, -12))))
    R.main([str(ann), str(tmp_path / 'masks'), '--shape', '21', '27', '--scale', '4', '--offset', '8', '-12'])
    m = np.asarray(Image.open(tmp_path / 'masks' / 'a.png'))
    assert m.dtype == np.uint8 and (m == (cmap > 0)).all()
    for argv in ([str(ann), str(tmp_path / 'x')], [str(ann), str(tmp_path / 'x'), '--shape', '4', '4', '--images', str(img)],
                 [str(ann), str(tmp_path / 'x'), '--shape', '4', '4', '--labels', '--classes', 'a,b']):
        with pytest.raises(SystemExit):
            R.main(argv)
    r = subprocess.run([sys.executable, '-m', 'wesup_amd.raster', str(ann), str(tmp_path / 'sub'), '--shape', '21', '27', '--scale', '4',
                        '--offset', '8', '-12'], cwd=ROOT, capture_output=True, text=True)
    assert r.returncode == 0 and 'a.geojson' in r.stdout and (np.asarray(Image.open(tmp_path / 'sub' / 'a.png')) == m).all()


# ------------------------------------------------------------------------------------------------- the library's new entries
@pytest.fixture(scope='module')
def lib():
    from wesup_amd import _lib
    if not os.path.exists(_lib.LIB_PATH):
        _lib.build()
    return _lib


NEW_ENTRIES = ('wesup_raster_limit', 'wesup_polygon_fill_workspace_bytes', 'wesup_polygon_fill')


def test_header_library_and_binding_agree(lib):
    hdr = open(os.path.join(ROOT, 'include', 'wesup_hip.h')).read()
    nm = subprocess.run(['nm', '-D', '--defined-only', lib.LIB_PATH], check=True, capture_output=True, text=True).stdout
    exported = set(re.findall(r' T (wesup_\w+)', nm))
    handle = lib.load()
    for name in NEW_ENTRIES:
        assert re.search(r'\b%s\s*\(' % name, hdr), name
        assert name in exported and name in lib._SIGS and hasattr(handle, name), name
    assert handle.wesup_abi_version() == lib.ABI_VERSION == 6
    limits = [handle.wesup_raster_limit(k) for k in range(7)]
    assert limits[:5] == [lib.RASTER_TILE_ROWS, lib.RASTER_TILE_COLS, lib.RASTER_BLOCK, lib.RASTER_COORD_MAX, lib.RASTER_FRAC_BITS]
    assert limits[5] > 0 and limits[6] == -1
    assert (R.FRAC_BITS, R.COORD_MAX) == (lib.RASTER_FRAC_BITS, lib.RASTER_COORD_MAX)
    for macro, v in (('TILE_ROWS', lib.RASTER_TILE_ROWS), ('TILE_COLS', lib.RASTER_TILE_COLS), ('BLOCK', lib.RASTER_BLOCK),
                     ('FRAC_BITS', lib.RASTER_FRAC_BITS)):
        assert f'#define WESUP_RASTER_{macro} {v}' in hdr
    assert 'raster.hip' in open(os.path.join(ROOT, 'wesup_amd', 'csrc', 'Makefile')).read()


def test_entries_refuse_bad_arguments_on_the_host(lib):
    h = lib.load()
    assert h.wesup_polygon_fill_workspace_bytes(2, 5, 7, 0) > 0
    assert h.wesup_polygon_fill_workspace_bytes(2, 5, 7, 3000) >= 3000 * 24 + 3 * 8
    assert h.wesup_polygon_fill_workspace_bytes(1, 2 ** 10, 2 ** 21 - 1, 1) > 0 and h.wesup_polygon_fill_workspace_bytes(1, 2 ** 10, 2 ** 21, 1) == 0
    buf = ctypes.create_string_buffer(1 << 17)       # non-null addresses; no entry gets as far as using them
    base = (ctypes.cast(buf, ctypes.c_void_p).value + 255) // 256 * 256
    v, rf, fr, fi, val, lab, o8, st, w = (base + 8192 * k for k in range(9))
    big = 1 << 16
    ok = (3, 2, 8)                                    # F, R, V: small enough for the 8 KiB between the addresses
    bad = ((0, 5, 7), (1, 0, 7), (1, 5, -1), (-1, 5, 7), (1, 2 ** 21 + 1, 1), (1, 1, 2 ** 21 + 1), (2, 2 ** 15, 2 ** 15),
           (1, 2 ** 31 - 1, 2 ** 31 - 1))
    for B, H, W in bad:
        assert h.wesup_polygon_fill_workspace_bytes(B, H, W, 3) == 0
        assert h.wesup_polygon_fill(v, rf, fr, fi, val, lab, o8, st, B, H, W, *ok, w, big, None) == -1
    assert h.wesup_polygon_fill_workspace_bytes(1, 5, 7, -1) == 0
    # null pointers, before any launch: values and out8 go together
    for k in (0, 1, 2, 3, 4, 5, 6, 7):
        a = [v, rf, fr, fi, val, lab, o8, st]
        a[k] = None
        assert h.wesup_polygon_fill(*a, 1, 5, 7, *ok, w, big, None) == -1, k
    assert h.wesup_polygon_fill(v, rf, fr, fi, val, lab, o8, st, 1, 5, 7, *ok, None, big, None) == -1
    # negative counts, a short workspace
    for counts in ((-1, 2, 8), (3, -1, 8), (3, 2, -1)):
        assert h.wesup_polygon_fill(v, rf, fr, fi, val, lab, o8, st, 1, 5, 7, *counts, w, big, None) == -1
    need = h.wesup_polygon_fill_workspace_bytes(1, 5, 7, 3)
    assert h.wesup_polygon_fill(v, rf, fr, fi, val, lab, o8, st, 1, 5, 7, *ok, w, need - 1, None) == -1
    # overlapping operands, misaligned vertices
    assert h.wesup_polygon_fill(v, rf, fr, fi, val, lab, lab + 64, st, 1, 5, 7, *ok, w, big, None) == -1
    assert h.wesup_polygon_fill(v, rf, fr, fi, val, lab, o8, lab + 4, 1, 5, 7, *ok, w, big, None) == -1
    assert h.wesup_polygon_fill(v, v + 32, fr, fi, val, lab, o8, st, 1, 5, 7, *ok, w, big, None) == -1
    assert h.wesup_polygon_fill(v, rf, fr, fi, val, lab, o8, st, 1, 5, 7, *ok, lab, big, None) == -1
    assert h.wesup_polygon_fill(v + 4, rf, fr, fi, val, lab, o8, st, 1, 5, 7, *ok, w, big, None) == -1


_EDGE_PROBE = """
#include "raster.hpp"
extern "C" int edge_cols(int x0, int y0, int x1, int y1, int rlo, int rhi, int* ra, int* cols) {
    RsEdge e;
    if (!rs_edge_setup(x0, y0, x1, y1, rlo, rhi, e)) return 0;
    *ra = e.ra;
    int n = 0;
    for (int r = e.ra; r < e.rb; ++r) { cols[n++] = e.q; rs_edge_step(e); }
    return n;
}
"""


def test_the_kernels_edge_stepping_equals_the_closed_form(tmp_path):
    """csrc/raster.hpp, the arithmetic of the fill kernel (one division per edge, then additions with a carry), built for the host:
    every c* of every crossed row against ceil((N - 128 D) / (256 D)) in Python integers."""
    import random
    import shutil
    cxx = shutil.which('g++') or shutil.which('c++') or shutil.which('clang++') or '/opt/rocm/llvm/bin/clang++'
    (tmp_path / 'probe.cpp').write_text(_EDGE_PROBE)
    so = tmp_path / 'libprobe.so'
    subprocess.run([cxx, '-O1', '-shared', '-fPIC', '-I', os.path.join(ROOT, 'wesup_amd', 'csrc'), str(tmp_path / 'probe.cpp'), '-o',
                    str(so)], check=True)
    probe = ctypes.CDLL(str(so))
    cols, ra = (ctypes.c_int * 64)(), ctypes.c_int()
    rnd = random.Random(5)
    edges = [(-2 ** 28, -2 ** 28, 2 ** 28, 2 ** 28, -2 ** 20 - 2), (2 ** 28, -2 ** 28, -2 ** 28, 2 ** 28, 2 ** 20 - 63),
             (-2 ** 28, -2 ** 28, 2 ** 28, -2 ** 28 + 1, -2 ** 20 - 1), (2 ** 28, 2 ** 28 - 1, -2 ** 28, -2 ** 28, 17)]
    for _ in range(20000):
        m, g = rnd.choice([256 * 8, 256 * 64, 2 ** 20, 2 ** 28]), rnd.choice([1, 1, 128, 256])
        x0, y0, x1, y1 = (rnd.randint(-m, m) // g * g for _ in range(4))
        x1 = x0 if rnd.random() < 0.2 else x1
        y1 = y0 if rnd.random() < 0.1 else y1
        rlo = (min(y0, y1) >> 8) + rnd.randint(-3, 3) if rnd.random() < 0.7 else (max(y0, y1) >> 8) - rnd.randint(0, 40)
        edges.append((x0, y0, x1, y1, rlo))
    for x0, y0, x1, y1, rlo in edges:
        rhi = rlo + 64
        n = probe.edge_cols(x0, y0, x1, y1, rlo, rhi, ctypes.byref(ra), cols)
        a, b, c, d = (x0, y0, x1, y1) if y0 < y1 else (x1, y1, x0, y0)
        want = []
        for r in range(rlo, rhi):
            Yc = 256 * r + 128
            if b <= Yc < d:
                D, N = d - b, a * (d - b) + (c - a) * (Yc - b)
                want.append((r, -((128 * D - N) // (256 * D))))
        assert [(ra.value + i, cols[i]) for i in range(n)] == want, (x0, y0, x1, y1, rlo)


def test_wrapper_fails_loudly_without_gpu_tensors(lib):
    import torch
    from wesup_amd import ops
    p = R.pack(named_cases()['unit_square'][0])
    with pytest.raises(lib.WesupHipError):
        ops.polygon_fill(*(torch.from_numpy(a) for a in p[:4]), (3, 3))
