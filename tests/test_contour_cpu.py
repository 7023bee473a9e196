"""Object outlines: the sequential tracer wesup_amd/contour.py:trace_host on the named cases and against the
properties that define a correct outline (ring counts against scipy's components, the even-odd fill, the area sums, the order of
the rings), polygons, the GeoJSON export and its command line, and the host-side checks of the new C entries.  No GPU."""
import ctypes
import json
import os
import re
import subprocess

import numpy as np
import pytest

from wesup_amd import contour as C
from wesup_amd.utils import metrics as M

from _contourcases import checkerboard, hole_count, named_cases, random_map

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMED = dict(named_cases())


def _rec(r):
    return dict(zip(C.RING_FIELDS[:10], (int(v) for v in r[:10])), area2=int(C.area2_of(r[None])[0]))


def _pts(rings, verts, i):
    return [tuple(p) for p in verts[rings[i, 2]:rings[i, 2] + rings[i, 3]].tolist()]


# ------------------------------------------------------------------------------------------------------------ named cases
def test_single_pixel():
    r, v, n = C.trace_host(NAMED['pixel'])
    assert n.tolist() == [1] and r.dtype == v.dtype == n.dtype == np.int32 and r.shape == (1, 12) and v.shape == (4, 2)
    assert _rec(r[0]) == dict(image=0, label=1, first_vertex=0, n_vertices=4, n_cracks=4, xmin=0, ymin=0, xmax=1, ymax=1,
                              leader_slot=0, area2=2)
    assert _pts(r, v, 0) == [(1, 0), (0, 0), (0, 1), (1, 1)]


def test_saddle_is_one_ring_through_the_vertex_twice():
    r, v, n = C.trace_host(NAMED['saddle'])
    assert n.tolist() == [1] and _rec(r[0])['n_cracks'] == 8 and _rec(r[0])['area2'] == 4
    assert _pts(r, v, 0) == [(1, 0), (0, 0), (0, 1), (1, 1), (1, 2), (2, 2), (2, 1), (1, 1)]


def test_ring_with_a_hole():
    r, v, n = C.trace_host(NAMED['ring3'])
    assert n.tolist() == [2]
    outer, hole = _rec(r[0]), _rec(r[1])
    assert (outer['n_cracks'], outer['area2'], outer['leader_slot']) == (12, 18, 0)
    assert _pts(r, v, 0) == [(0, 0), (0, 3), (3, 3), (3, 0)]            # the leader's start (1, 0) is no corner
    assert (hole['n_cracks'], hole['area2'], hole['leader_slot']) == (4, -2, 6)
    assert _pts(r, v, 1) == [(1, 1), (2, 1), (2, 2), (1, 2)]
    assert (hole['xmin'], hole['ymin'], hole['xmax'], hole['ymax']) == (1, 1, 2, 2)


def test_diagonal_holes_stay_two():
    r, v, n = C.trace_host(NAMED['two_holes'])
    a2 = C.area2_of(r)
    assert n.tolist() == [3] and (a2 > 0).sum() == 1 and r[a2 < 0, 9].tolist() == [6, 26]


def test_touching_labels_keep_their_own_side():
    r, v, n = C.trace_host(NAMED['touching'])
    assert n.tolist() == [2] and r[:, 1].tolist() == [1, 2] and r[:, 4].tolist() == [4, 4] and C.area2_of(r).tolist() == [2, 2]
    assert (1, 0) in _pts(r, v, 0) and (1, 0) in _pts(r, v, 1)


def test_long_row():
    r, v, n = C.trace_host(NAMED['row511'])
    assert n.tolist() == [1] and r[0, 4] == 1024 and r[0, 3] == 4 and C.area2_of(r)[0] == 1022


# ------------------------------------------------------------------------------------------------------------- invariants
def _check_invariants(lab):
    r, v, n = C.trace_host(lab)
    a2 = C.area2_of(r)
    assert n.sum() == len(r) and (np.diff(r[:, 9]) > 0).all()                        # ordered by leader slot
    assert r[:, 3].sum() == len(v) and (r[:, 2] == np.cumsum(r[:, 3]) - r[:, 3]).all()
    assert (r[:, 3] % 2 == 0).all() and (r[:, 3] >= 4).all()
    assert (C.count_host(lab) == [[r[:, 4].sum(), len(v)]]).all()
    for l in np.unique(lab[lab > 0]):
        assert (C.rings_to_mask_host(r, v, lab.shape, label=l) == (lab == l)).all()
        assert a2[r[:, 1] == l].sum() == 2 * (lab == l).sum()
    assert not (r[:, 1] <= 0).any()
    return r, v, a2


@pytest.mark.parametrize('seed', range(60))
def test_binary_masks_against_scipy(seed):
    rs = np.random.RandomState(seed)
    H, W = rs.randint(1, 14, 2)
    mask = random_map(seed, H, W)
    lab = M.label(mask).astype(np.int32)                                             # 8-connected, as cc_label(..., 8)
    r, v, a2 = _check_invariants(lab)
    assert (a2 > 0).sum() == lab.max() and sorted(r[a2 > 0, 1].tolist()) == list(range(1, lab.max() + 1))
    assert (a2 < 0).sum() == hole_count(mask)
    polys = C.polygons(r, v)                                                         # every component: one outer ring
    assert len(polys) == lab.max() and sum(p['area_px'] for p in polys) == mask.sum()
    # the unlabelled mask: the same cracks, and the fill gives the mask back
    r1, v1, _ = C.trace_host(mask)
    assert r1[:, 4].sum() == r[:, 4].sum() and (C.rings_to_mask_host(r1, v1, mask.shape) == (mask != 0)).all()


@pytest.mark.parametrize('seed', range(30))
def test_three_label_maps(seed):
    rs = np.random.RandomState(100 + seed)
    H, W = rs.randint(1, 14, 2)
    _check_invariants(random_map(100 + seed, H, W, n_labels=3))


def test_edges_of_the_domain():
    for shape in ((1, 9), (9, 1), (1, 1), (5, 7)):
        full = np.ones(shape, np.int32)
        r, v, n = C.trace_host(full)
        assert n.tolist() == [1] and r[0, 4] == 2 * (shape[0] + shape[1]) and r[0, 3] == 4
        assert C.area2_of(r)[0] == 2 * full.size and r[0, 5:9].tolist() == [0, 0, shape[1], shape[0]]
        r, v, n = C.trace_host(np.zeros(shape, np.int32))
        assert r.shape == (0, 12) and v.shape == (0, 2) and n.tolist() == [0]
    _check_invariants(random_map(7, 1, 13))
    _check_invariants(random_map(8, 13, 1))
    _check_invariants(checkerboard(6, 7))


def test_negative_labels_are_ignored_and_the_largest_label_fits():
    big = 2 ** 31 - 1
    lab = np.array([[-3, big, big], [0, -1, big], [5, 0, -3]], np.int64)
    r, v, n = C.trace_host(lab)
    assert sorted(r[:, 1].tolist()) == [5, big] and r.dtype == np.int32
    assert (C.rings_to_mask_host(r, v, lab.shape, label=big) == (lab == big)).all()
    assert (C.trace_host(np.where(lab > 0, lab, 0))[0] == r).all()


def test_batches_are_concatenated_image_major():
    maps = np.stack([random_map(1, 6, 5, 2), np.zeros((6, 5), np.int32), np.ones((6, 5), np.int32)])
    r, v, n = C.trace_host(maps)
    each = [C.trace_host(m) for m in maps]
    assert n.tolist() == [len(e[0]) for e in each] and n[1] == 0 and n[2] == 1
    assert (v == np.concatenate([e[1] for e in each])).all()
    assert (r[:, 0] == np.repeat(np.arange(3), n)).all()
    off = 0
    for b, e in enumerate(each):
        got = r[r[:, 0] == b].copy()
        got[:, 0] = 0
        got[:, 2] -= off
        assert (got == e[0]).all()
        assert (C.rings_to_mask_host(r, v, maps[b].shape, image=b) == (maps[b] > 0)).all() or maps[b].max() > 1
        off += len(e[1])


# ------------------------------------------------------------------------------------------------------ polygons, GeoJSON
def test_polygons_refuse_a_label_of_two_components():
    lab = np.array([[1, 0, 1]], np.int32)
    with pytest.raises(ValueError, match='label the components first'):
        C.polygons(*C.trace_host(lab)[:2])
    polys = C.mask_polygons(lab)
    assert [p['label'] for p in polys] == [1, 2] and [p['area_px'] for p in polys] == [1, 1]


def test_polygons_fields():
    mask = np.zeros((7, 8), np.uint8)
    mask[1:6, 1:7] = 255
    mask[2:4, 2:4] = 0
    mask[6, 7] = 255                                  # touches the block diagonally: the same object
    (p,) = C.mask_polygons(mask)
    assert p['label'] == 1 and p['area_px'] == 30 - 4 + 1 and len(p['holes']) == 1 and p['bbox'] == [1, 1, 8, 7]
    assert p['perimeter_px'] == 22 + 8 + 4 and p['outer'].dtype == np.int32
    assert C.mask_polygons(mask, min_area=28) == [] and len(C.mask_polygons(mask, min_area=27)) == 1


def test_classmap_polygons():
    cmap = np.array([[0, 1, 1, 0, 2], [0, 1, 0, 0, 2], [3, 0, 0, 1, 0]], np.uint8)
    polys = C.classmap_polygons(cmap, 4)
    assert [(p['class'], p['label'], p['area_px']) for p in polys] == [(1, 1, 3), (1, 2, 1), (2, 1, 2), (3, 1, 1)]
    doc = C.to_geojson(polys, class_names=['bg', 'gland', 'stroma', 'fat'])
    assert [f['properties']['classification']['name'] for f in doc['features']] == ['gland', 'gland', 'stroma', 'fat']
    assert (C.geojson_to_mask_host(doc, cmap.shape) == (cmap > 0)).all()
    with pytest.raises(ValueError):
        C.classmap_polygons(cmap, 1)


@pytest.mark.parametrize('scale,offset', [(1.0, (0, 0)), (4.0, (100, -20)), (0.5, (3, 7))])
def test_geojson_round_trip(tmp_path, scale, offset):
    mask = random_map(11, 12, 13)
    mask[4:9, 3:9] = 1
    mask[5:7, 5:7] = 0
    polys = C.mask_polygons(mask)
    path = C.write_geojson(tmp_path / 'sub' / 'a.geojson', polys, scale=scale, offset=offset)
    doc = json.loads(path.read_text())
    assert doc['type'] == 'FeatureCollection' and len(doc['features']) == len(polys) == M.label(mask).max()
    assert any(len(f['geometry']['coordinates']) > 1 for f in doc['features'])      # a hole is exported
    for f, p in zip(doc['features'], polys):
        g = f['geometry']
        assert f['type'] == 'Feature' and g['type'] == 'Polygon' and len(g['coordinates']) == 1 + len(p['holes'])
        for ring, src in zip(g['coordinates'], [p['outer']] + p['holes']):
            assert ring[0] == ring[-1] and len(ring) == len(src) + 1
            assert ring[:-1] == [[x * scale + offset[0], y * scale + offset[1]] for x, y in src.tolist()]
        pr = f['properties']
        assert pr['objectType'] == 'annotation' and 'classification' not in pr
        assert (pr['label'], pr['area_px'], pr['perimeter_px'], pr['bbox']) == (p['label'], p['area_px'], p['perimeter_px'], p['bbox'])
    assert (C.geojson_to_mask_host(doc, mask.shape, scale, offset) == (mask != 0)).all()


def test_command_line(tmp_path):
    from PIL import Image
    pred, out = tmp_path / 'pred', tmp_path / 'out'
    pred.mkdir()
    mask = random_map(3, 20, 30)
    Image.fromarray((mask * 255).astype(np.uint8)).save(pred / 'a.png')
    C.main([str(pred), str(out), '--scale', '2', '--min-area', '2'])
    doc = json.loads((out / 'a.geojson').read_text())
    lab = M.label(mask)
    keep = np.isin(lab, [l for l in range(1, lab.max() + 1) if (lab == l).sum() >= 2])
    assert (C.geojson_to_mask_host(doc, mask.shape, scale=2.0) == keep).all()
    # instance maps: labels as they are, not re-labelled
    inst = np.zeros((6, 9), np.uint16)
    inst[1:3, 1:4], inst[1:3, 4:7] = 300, 7
    pred2 = tmp_path / 'pred2'
    pred2.mkdir()
    Image.fromarray(inst).save(pred2 / 'b_labels.png')
    C.main([str(pred2), str(out), '--labels'])
    doc = json.loads((out / 'b_labels.geojson').read_text())
    assert sorted(f['properties']['label'] for f in doc['features']) == [7, 300]
    # class maps
    Image.fromarray(np.array([[0, 1, 2], [2, 2, 0]], np.uint8)).save(pred2 / 'b_labels.png')
    C.main([str(pred2), str(out), '--classes', '3'])
    doc = json.loads((out / 'b_labels.geojson').read_text())
    assert [f['properties']['classification']['name'] for f in doc['features']] == ['class 1', 'class 2']


def test_split_command_line_writes_outlines(tmp_path):
    from PIL import Image
    from wesup_amd import split
    from _splitcases import write_scene
    pred, _ = write_scene(tmp_path)
    out, gj = tmp_path / 'out', tmp_path / 'gj'
    split.main([str(pred), str(out), '--radius', '6', '--geojson', str(gj)])
    assert list(out.glob('*.png'))
    for path in sorted(out.glob('*.png')):
        written = np.asarray(Image.open(path))
        doc = json.loads((gj / (path.stem + '.geojson')).read_text())
        assert len(doc['features']) == M.label(written).max()
        assert (C.geojson_to_mask_host(doc, written.shape) == (written != 0)).all()


# ------------------------------------------------------------------------------------------------- the library's new entries
@pytest.fixture(scope='module')
def lib():
    from wesup_amd import _lib
    if not os.path.exists(_lib.LIB_PATH):
        _lib.build()
    return _lib


NEW_ENTRIES = ('wesup_contour_workspace_bytes', 'wesup_contour_trace_workspace_bytes', 'wesup_contour_count', 'wesup_contour_trace')


def test_header_library_and_binding_agree(lib):
    hdr = open(os.path.join(ROOT, 'include', 'wesup_hip.h')).read()
    nm = subprocess.run(['nm', '-D', '--defined-only', lib.LIB_PATH], check=True, capture_output=True, text=True).stdout
    exported = set(re.findall(r' T (wesup_\w+)', nm))
    handle = lib.load()
    for name in NEW_ENTRIES:
        assert re.search(r'\b%s\s*\(' % name, hdr), name
        assert name in exported and name in lib._SIGS and hasattr(handle, name), name
    assert handle.wesup_abi_version() == lib.ABI_VERSION == 6
    assert '#define WESUP_CONTOUR_RING 12' in hdr and lib.CONTOUR_RING == 12 == C.RING == len(C.RING_FIELDS)
    assert 'contour.hip' in open(os.path.join(ROOT, 'wesup_amd', 'csrc', 'Makefile')).read()


def test_entries_refuse_bad_arguments_on_the_host(lib):
    h = lib.load()
    assert h.wesup_contour_workspace_bytes(2, 5, 7) >= h.wesup_contour_trace_workspace_bytes(2, 5, 7, 280) > \
        h.wesup_contour_trace_workspace_bytes(2, 5, 7, 0) >= 2 * 5 * 7 * 5
    assert h.wesup_contour_trace_workspace_bytes(2, 5, 7, 281) == 0 and h.wesup_contour_trace_workspace_bytes(2, 5, 7, -1) == 0
    # 4 B H W below 2^31 and not at it
    assert h.wesup_contour_workspace_bytes(1, 1, 2 ** 29 - 1) > 0 and h.wesup_contour_workspace_bytes(1, 1, 2 ** 29) == 0
    assert h.wesup_contour_workspace_bytes(2, 2 ** 14, 2 ** 14) == 0 and h.wesup_contour_workspace_bytes(1, 2 ** 14, 2 ** 14) > 0
    buf = ctypes.create_string_buffer(1 << 17)       # non-null addresses; no entry gets as far as using them
    base = (ctypes.cast(buf, ctypes.c_void_p).value + 255) // 256 * 256
    l, r, v, n, s, w = (base + 8192 * k for k in range(6))
    big = 1 << 16
    bad = ((0, 5, 7), (1, 0, 7), (1, 5, -1), (-1, 5, 7), (65536, 5, 7), (1, 1, 2 ** 29), (1, 2 ** 15, 2 ** 14), (4, 2 ** 14, 2 ** 13),
           (1, 2 ** 31 - 1, 2 ** 31 - 1))
    for B, H, W in bad:
        assert h.wesup_contour_workspace_bytes(B, H, W) == 0 and h.wesup_contour_trace_workspace_bytes(B, H, W, 0) == 0
        assert h.wesup_contour_count(l, r, B, H, W, w, big, None) == -1
        assert h.wesup_contour_trace(l, r, v, n, s, B, H, W, 4, 4, 1, w, big, None) == -1
    # null pointers, before any launch
    for k in range(2):
        a = [l, r]
        a[k] = None
        assert h.wesup_contour_count(*a, 1, 5, 7, w, big, None) == -1
    assert h.wesup_contour_count(l, r, 1, 5, 7, None, big, None) == -1
    for k in range(5):
        a = [l, r, v, n, s]
        a[k] = None
        assert h.wesup_contour_trace(*a, 1, 5, 7, 8, 8, 2, w, big, None) == -1
    assert h.wesup_contour_trace(l, r, v, n, s, 1, 5, 7, 8, 8, 2, None, big, None) == -1
    # short workspaces: the count's, and the trace's for the cracks it is told of
    need0, need = h.wesup_contour_trace_workspace_bytes(1, 5, 7, 0), h.wesup_contour_trace_workspace_bytes(1, 5, 7, 8)
    assert h.wesup_contour_count(l, r, 1, 5, 7, w, need0 - 1, None) == -1
    assert h.wesup_contour_trace(l, r, v, n, s, 1, 5, 7, 8, 8, 2, w, need - 1, None) == -1
    assert h.wesup_contour_trace(l, r, v, n, s, 1, 5, 7, 8, 8, 2, w, 16, None) == -1
    # negative counts, more cracks than the shape has edges
    for counts in ((-1, 8, 2), (8, -1, 2), (8, 8, -1), (4 * 35 + 1, 8, 2)):
        assert h.wesup_contour_trace(l, r, v, n, s, 1, 5, 7, *counts, w, big, None) == -1
    # overlapping operands
    assert h.wesup_contour_count(l, l + 64, 1, 5, 7, w, big, None) == -1 and h.wesup_contour_count(l, w + 64, 1, 5, 7, w, big, None) == -1
    assert h.wesup_contour_trace(l, r, r + 48, n, s, 1, 5, 7, 8, 8, 2, w, big, None) == -1          # rings and verts
    assert h.wesup_contour_trace(l, r, r, n, s, 1, 5, 7, 8, 8, 2, w, big, None) == -1
    assert h.wesup_contour_trace(l, r, v, n, n, 1, 5, 7, 8, 8, 2, w, big, None) == -1               # n_rings and status
    assert h.wesup_contour_trace(l, l + 16, v, n, s, 1, 5, 7, 8, 8, 2, w, big, None) == -1
    assert h.wesup_contour_trace(l, r, v, n, s, 1, 5, 7, 8, 8, 2, r, big, None) == -1
    assert h.wesup_contour_trace(l, r + 4, v, n, s, 1, 5, 7, 8, 8, 2, w, big, None) == -1           # rings: 8-byte aligned


def test_wrappers_fail_loudly_without_gpu_tensors(lib):
    import torch
    from wesup_amd import ops
    for call in (lambda: ops.contour_count(torch.zeros(4, 4, dtype=torch.int32)),
                 lambda: ops.contour_trace(torch.zeros(4, 4, dtype=torch.int32))):
        with pytest.raises(lib.WesupHipError):
            call()
