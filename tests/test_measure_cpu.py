"""The host definitions of the object measurements (wesup_amd/measure.py): sums against np.nonzero, the quad Euler
number against scipy's components and holes and against the hole rings of the tracer, the hull against gift wrapping, the
perimeter classes and the moments against closed forms, absent and out-of-range labels, and the GeoJSON export unchanged without
measurements."""
import json
import math
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from _contourcases import hole_count, random_map      # noqa: E402
from _measurecases import brute_hull, disc, empty_rows, full_row, interleaved, parabola      # noqa: E402

from wesup_amd import contour as C      # noqa: E402
from wesup_amd import measure as MS      # noqa: E402


@pytest.mark.parametrize('seed,H,W,n', [(1, 17, 15, 1), (2, 33, 65, 3), (3, 1, 257, 3), (4, 257, 1, 1), (5, 40, 40, 5)])
def test_sums_and_boxes_equal_nonzero_sums(seed, H, W, n):
    lab = random_map(seed, H, W, n)
    table, verts, status = MS.measure_host(lab, n)
    assert table.shape == (1, n + 1, MS.MEASURE_WORDS) and table.dtype == np.int64 and status.tolist() == [0]
    assert (table[0, 0] == 0).all()
    for l in range(1, n + 1):
        r, c = np.nonzero(lab == l)
        assert len(r) > 0
        assert table[0, l, :10].tolist() == [len(r), r.sum(), c.sum(), (r * r).sum(), (r * c).sum(), (c * c).sum(), r.min(), c.min(),
                                             r.max(), c.max()]
    assert table[0, 1, 23] == 0 and len(verts) == table[0, :, 17].sum()
    assert (np.diff(table[0, 1:, 23]) == table[0, 1:-1, 17]).all()


@pytest.mark.parametrize('seed', range(8))
def test_quad_euler_number_is_components_minus_holes(seed):
    from scipy import ndimage
    rs = np.random.RandomState(seed)
    mask = random_map(100 + seed, int(rs.randint(3, 14)), int(rs.randint(3, 16)))
    t = MS.measure_host(mask, 1)[0][0, 1]
    n8 = ndimage.label(mask, np.ones((3, 3)))[1]
    assert (t[13] - t[14] - 2 * t[15]) % 4 == 0
    assert (t[13] - t[14] - 2 * t[15]) // 4 == n8 - hole_count(mask)


def test_holes_of_connected_labels_are_the_hole_rings_of_the_tracer():
    from scipy import ndimage
    mask = random_map(7, 12, 15)
    mask[2:9, 3:11] = 1
    mask[4, 5] = mask[6, 7:9] = 0
    lab, n = ndimage.label(mask, np.ones((3, 3)))
    table = MS.measure_host(lab, n)[0][0]
    rings = C.trace_host(lab)[0]
    a2 = C.area2_of(rings)
    total = 0
    for l in range(1, n + 1):
        holes = int(((rings[:, 1] == l) & (a2 < 0)).sum())
        assert MS.features(table[l])['holes'] == holes == hole_count(lab == l)
        total += holes
    assert total >= 2


@pytest.mark.parametrize('seed', range(12))
def test_hull_equals_gift_wrapping(seed):
    rs = np.random.RandomState(200 + seed)
    H, W = int(rs.randint(1, 14)), int(rs.randint(1, 14))
    mask = rs.rand(H, W) < rs.uniform(0.1, 0.9)
    mask[rs.randint(H), rs.randint(W)] = True
    got, want = MS.hull_host(mask), brute_hull(mask)
    assert got.tolist() == want.tolist()
    assert MS.hull_area2(got) >= 2 * mask.sum()
    assert got[0].tolist() == min(got.tolist(), key=lambda p: (p[1], p[0]))


@pytest.mark.parametrize('mask', [empty_rows() == 1, interleaved() == 1, interleaved() == 2, parabola(40), disc(9)])
def test_hull_of_shaped_cases_equals_gift_wrapping(mask):
    assert MS.hull_host(mask).tolist() == brute_hull(mask).tolist()


def test_hull_of_a_staircase_has_only_its_end_vertices_and_rectangles_are_their_own_hull():
    st = np.eye(8, dtype=np.int32)
    assert MS.hull_host(st).tolist() == [[0, 0], [0, 1], [7, 8], [8, 8], [8, 7], [1, 0]]
    for a, b in [(1, 1), (1, 9), (4, 3), (2, 2)]:
        t, v, _ = MS.measure_host(np.ones((a, b), np.int32), 1)
        assert t[0, 1, 16] == 2 * a * b and v.tolist() == [[0, 0], [0, a], [b, a], [b, 0]]
    t = MS.measure_host(random_map(3, 20, 20), 1)[0][0, 1]
    assert t[16] > 2 * t[0]
    assert MS.hull_host(np.zeros((3, 3))).shape == (0, 2)


def test_perimeter_classes():
    for a, b in [(2, 2), (2, 7), (3, 5), (6, 4)]:
        assert MS.measure_host(np.ones((a, b), np.int32), 1)[0][0, 1, 10:13].tolist() == [2 * (a + b) - 4, 0, 0]
    assert MS.measure_host(np.ones((1, 9), np.int32), 1)[0][0, 1, 10:13].tolist() == [7, 0, 0]
    assert MS.measure_host(np.ones((1, 1), np.int32), 1)[0][0, 1, 10:13].tolist() == [0, 0, 0]
    r, c = np.indices((61, 61))
    d = ((r - 30) ** 2 + (c - 30) ** 2 <= 28 ** 2).astype(np.int32)
    assert MS.measure_host(d, 1)[0][0, 1, 10:13].tolist() == [48, 28, 80]
    # a neighbouring label bounds a label as the outside does
    two = np.ones((4, 6), np.int32)
    two[:, 3:] = 2
    assert MS.measure_host(two, 2)[0][0, 1:, 10:13].tolist() == [[2 * (4 + 3) - 4, 0, 0]] * 2


@pytest.mark.parametrize('H,W', [(1, 1), (1, 12), (7, 1), (5, 9), (32, 31)])
def test_all_ones_map_in_closed_form(H, W):
    t = MS.measure_host(np.ones((H, W), np.int32), 1)[0][0, 1]
    assert t[3] == W * (H - 1) * H * (2 * H - 1) // 6 and t[4] == H * (H - 1) // 2 * (W * (W - 1) // 2)
    assert t.tolist() == full_row(H, W)


def test_features_of_a_row_and_of_a_disc():
    b = 9
    f = MS.features(MS.measure_host(np.ones((1, b), np.int32), 1)[0][0, 1], width=b)
    assert f['major_axis'] == pytest.approx(4 * math.sqrt((b * b - 1) / 12), rel=1e-12) and f['minor_axis'] == 0
    assert f['area'] == b and f['centroid_x'] == 4.5 and f['centroid_y'] == 0.5 and f['extent'] == 1 and f['solidity'] == 1
    assert f['orientation'] == 0 and f['eccentricity'] == 1 and f['holes'] == 0 and f['bbox'] == [0, 0, 9, 1]
    assert f['feret_max'] == pytest.approx(math.sqrt(82)) and f['feret_p'] == [0, 0] and f['feret_q'] == [9, 1]
    assert f['inradius'] == 0 and MS.features(np.zeros(24, np.int64)) is None
    f1 = MS.features(MS.measure_host(np.ones((1, 1), np.int32), 1)[0][0, 1])
    assert f1['circularity'] is None and f1['perimeter'] == 0
    t = MS.measure(disc(20))[0][0, 1]
    f, g = MS.features(t, width=41), MS.features(t, scale=2.0, width=41)
    assert f['inradius'] == math.sqrt(20 * 20 + 1) and f['inradius_point'] == [20.5, 20.5]      # the nearest zero pixel: (0, 19)
    assert 0.85 < f['circularity'] < 1.1 and f['eccentricity'] < 1e-6 and f['major_axis'] == pytest.approx(40.5, rel=0.02)
    assert g['area'] == 4 * f['area'] and g['perimeter'] == 2 * f['perimeter'] and g['feret_max'] == 2 * f['feret_max']
    assert g['solidity'] == f['solidity'] and g['convex_area'] == 4 * f['convex_area']
    # big sums: the central moments come from Python integers
    big = np.array([2 ** 30, 2 ** 44, 2 ** 44, 2 ** 59, 2 ** 58, 2 ** 59] + [0] * 18, np.int64)
    big[8:10] = 32767
    big[16] = 2 ** 31
    assert MS.features(big)['major_axis'] > 0


def test_absent_and_out_of_range_labels():
    lab = np.array([[0, 3, 3], [7, 0, -2], [1, 1, 0]], np.int32)
    table, verts, status = MS.measure_host(lab, 4)
    assert status.tolist() == [1]
    assert table[0, 2].tolist() == [0] * 6 + [3, 3, -1, -1] + [0] * 14 == table[0, 4].tolist()
    assert (table[0, 0] == 0).all()
    clean = np.where((lab < 0) | (lab > 4), 0, lab)
    t2, v2, s2 = MS.measure_host(clean, 4)
    assert s2.tolist() == [0] and (t2[0, [0, 2, 4]] == table[0, [0, 2, 4]]).all() and (v2 == verts).all()
    # an out-of-range neighbour bounds a label like any other label; its own pixels are skipped
    assert (t2 == table).all()
    both = np.stack([lab, clean])
    tb, vb, sb = MS.measure_host(both, 4)
    assert sb.tolist() == [1, 0] and (tb[0] == table[0]).all() and tb[1, 1, 23] == len(verts) and len(vb) == 2 * len(verts)


def test_inscribed_radius_takes_the_first_pixel_in_raster_order():
    lab = np.zeros((7, 9), np.int32)
    lab[1:6, 1:6] = 1
    lab[1:6, 6:8] = 2
    table = MS.measure(lab)[0][0]
    assert table[1, 21:23].tolist() == [9, 3 * 9 + 3]                      # the distance to the background, through label 2
    assert table[2, 21:23].tolist() == [4, 2 * 9 + 6]
    assert MS.measure_host(lab, 2)[0][0, 1:, 21:23].tolist() == [[0, 0], [0, 0]]


def test_geojson_without_measurements_is_unchanged():
    a = np.zeros((3, 4), np.int32)
    a[0, 1] = 1
    a[1:3, 2:4] = 2
    polys = C.polygons(*C.trace_host(a)[:2])
    want = ('{"type": "FeatureCollection", "features": [{"type": "Feature", "geometry": {"type": "Polygon", "coordinates": '
            '[[[5.0, 3.0], [3.0, 3.0], [3.0, 5.0], [5.0, 5.0], [5.0, 3.0]]]}, "properties": {"objectType": "annotation", "label": 1, '
            '"area_px": 1, "perimeter_px": 4, "bbox": [1, 0, 2, 1]}}, {"type": "Feature", "geometry": {"type": "Polygon", '
            '"coordinates": [[[5.0, 5.0], [5.0, 9.0], [9.0, 9.0], [9.0, 5.0], [5.0, 5.0]]]}, "properties": {"objectType": '
            '"annotation", "label": 2, "area_px": 4, "perimeter_px": 8, "bbox": [2, 1, 4, 3]}}]}')
    assert json.dumps(C.to_geojson(polys, 2.0, (1, 3))) == want == json.dumps(C.to_geojson(polys, 2.0, (1, 3), measurements=None))
    table = MS.measure(a)[0][0]
    meas = {(0, 2): MS.features(table[2], 2.0, 4)}
    doc = C.to_geojson(polys, 2.0, (1, 3), measurements=meas)
    assert 'measurements' not in doc['features'][0]['properties']
    assert doc['features'][1]['properties']['measurements']['area'] == 16.0
    json.dumps(doc)


def test_command_line_on_the_host(tmp_path):
    from PIL import Image
    mask = (random_map(41, 45, 52) * 255).astype(np.uint8)
    mask[10:30, 10:40] = 255
    mask[15:20, 15:20] = 0
    (tmp_path / 'in').mkdir()
    Image.fromarray(mask).save(tmp_path / 'in' / 'a.png')
    MS.main([str(tmp_path / 'in'), str(tmp_path / 'out.csv'), '--min-area', '3', '--scale', '0.5', '--geojson', str(tmp_path / 'gj')])
    lines = (tmp_path / 'out.csv').read_text().splitlines()
    polys = C.mask_polygons(mask, min_area=3)
    assert lines[0].startswith('image,object,class,area,') and len(lines) == 1 + len(polys)
    doc = json.loads((tmp_path / 'gj' / 'a.geojson').read_text())
    assert [f['properties']['measurements']['area'] for f in doc['features']] == [p['area_px'] * 0.25 for p in polys]
    assert [f['properties']['measurements']['holes'] for f in doc['features']] == [len(p['holes']) for p in polys]


def test_split_driver_writes_the_table_of_its_instances(tmp_path):
    from PIL import Image
    from wesup_amd import split as SP
    from wesup_amd.utils import metrics as M
    r, c = np.indices((40, 70))
    mask = (((r - 20) ** 2 + (c - 20) ** 2 <= 15 ** 2) | ((r - 20) ** 2 + (c - 46) ** 2 <= 15 ** 2)).astype(np.uint8) * 255
    (tmp_path / 'in').mkdir()
    Image.fromarray(mask).save(tmp_path / 'in' / 'pair.png')
    SP.main([str(tmp_path / 'in'), str(tmp_path / 'out'), '--radius', '8', '--measure', str(tmp_path / 'm' / 'pair.csv')])
    inst = M.label(np.asarray(Image.open(tmp_path / 'out' / 'pair.png')) != 0)
    lines = (tmp_path / 'm' / 'pair.csv').read_text().splitlines()
    assert inst.max() >= 1 and len(lines) == 1 + inst.max()
    assert [float(l.split(',')[3]) for l in lines[1:]] == [float((inst == k).sum()) for k in range(1, inst.max() + 1)]
