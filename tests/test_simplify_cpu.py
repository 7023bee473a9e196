"""Ring simplification on the host (wesup_amd/contour.py:simplify_host) against an independent restatement in
``fractions.Fraction`` (tests/_simplifycases.py:ref_simplify) and against the properties the definition promises: the kept
vertices are a subsequence with both anchors, every dropped vertex lies within the tolerance of the segment between its kept
neighbours, every kept vertex was needed, the kept sets nest, the fill at tolerance 0 is the map, the fill at a tolerance changes
only pixels within it of the traced boundary, no ring changes its orientation.  The flags are checked, never skipped: a flag is
set exactly where the restatement says rule 5 asks for it (the 20-pixel diagonal and the smallest named cases collapse to their
two anchors at 2.5 px, which rule 5 answers with flag 1), and never at the cases and tolerances of DESIGN.md 3.24's table."""
import json
import os
import sys
from fractions import Fraction

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _simplifycases as S      # noqa: E402
from _simplifycases import TOLS      # noqa: E402

CASES = list(S.label_cases())
SMALL = list(S.small_maps())


def _rings_of(r, v):
    return [v[rec[2]:rec[2] + rec[3]] for rec in r]


def _subsequence_indices(full, part):
    """The indices at which ``part`` appears in ``full`` as a subsequence, greedily -- exact here because a ring's vertices that
    coincide (saddles) are told apart by the order."""
    idx, j = [], 0
    for i, p in enumerate(full.tolist()):
        if j < len(part) and p == part[j].tolist():
            idx.append(i)
            j += 1
    assert j == len(part), 'the kept vertices are not a subsequence of the ring'
    return idx


@pytest.mark.parametrize('name', CASES)
def test_equal_to_the_restatement_and_consistent(name):
    from wesup_amd import contour as C
    lab, r, v = S.traced(name)
    for tol in TOLS:
        r2, v2, fl = S.host(name, tol)
        e = S.ref_simplify(r, v, tol)
        assert (r2 == e[0]).all() and v2.shape == e[1].shape and (v2 == e[1]).all() and (fl == e[2]).all(), (name, tol)
        assert r2.dtype == v2.dtype == fl.dtype == np.int32
        # records: kept fields as traced, first vertices consecutive, bounding box and area2 of the output
        assert (r2[:, [0, 1, 4, 9]] == r[:, [0, 1, 4, 9]]).all()
        assert r2[:, 2].tolist() == (np.cumsum(r2[:, 3]) - r2[:, 3]).tolist() and r2[:, 3].sum() == len(v2)
        for rec, a2, pts, full, f in zip(r2, C.area2_of(r2), _rings_of(r2, v2), _rings_of(r, v), fl):
            assert rec[5:9].tolist() == [pts[:, 0].min(), pts[:, 1].min(), pts[:, 0].max(), pts[:, 1].max()]
            assert int(a2) == S.area2(pts)
            idx = _subsequence_indices(full, pts)
            assert idx[0] == 0
            if len(full) > 4 and not f:
                d = ((full.astype(np.int64) - full[0]) ** 2).sum(1)
                assert int(np.argmax(d)) in idx                                       # the far anchor
        # orientation, and polygons() takes the result
        assert (np.sign(C.area2_of(r2)) == np.sign(C.area2_of(r))).all()
        try:
            n_polys = len(C.polygons(r, v))
        except ValueError:                                                           # (a random map's label is several objects)
            continue
        assert len(C.polygons(r2, v2)) == n_polys


@pytest.mark.parametrize('name', CASES)
def test_guarantee_necessity_and_nesting(name):
    lab, r, v = S.traced(name)
    before = None
    for tol in TOLS:
        r2, v2, fl = S.host(name, tol)
        lim = Fraction(tol * tol, 256)
        kept_sets = []
        for full, pts, f in zip(_rings_of(r, v), _rings_of(r2, v2), fl):
            idx = _subsequence_indices(full, pts)
            kept_sets.append(set(idx) if not f else None)
            P = full.tolist()
            n = len(P)
            # guarantee: a dropped vertex lies within the tolerance of the segment between its two kept neighbours
            for a, b in zip(idx, idx[1:] + [idx[0] + n]):
                for k in range(a + 1, b):
                    assert S.seg_dist2(P[k % n], P[a], P[b % n]) <= lim, (name, tol, k)
            # necessity: replay the recursion from the output -- every kept vertex is the one the tie rule names, and beyond the tolerance
            if n > 4 and not f:
                far = [i for i in idx if i][int(np.argmax([((full[i].astype(np.int64) - full[0]) ** 2).sum() for i in idx if i]))]
                stack = [(0, far), (far, n)]
                while stack:
                    lo, hi = stack.pop()
                    inner = [i for i in idx if lo < i < hi]
                    if not inner:
                        continue
                    d = {k: S.seg_dist2(P[k], P[lo], P[hi % n]) for k in range(lo + 1, hi)}
                    m = min(d, key=lambda k: (-d[k], abs(2 * k - lo - hi), k))
                    assert m in inner and d[m] > lim, (name, tol, lo, hi, m)
                    stack += [(lo, m), (m, hi)]
        # nesting: what a larger tolerance keeps, a smaller one kept (flagged rings are whole: they contain everything)
        if before is not None:
            for small, large in zip(before, kept_sets):
                if small is not None and large is not None:
                    assert large <= small
        before = kept_sets


def test_flags_on_traced_rings_are_what_rule_5_asks_and_none_in_the_table():
    """No flag at the cases and tolerances of DESIGN.md 3.24's table; elsewhere a flag only where rule 5 asks for it."""
    for name, tols in (('ellipses', (0, 8, 16)), ('diamond', (0, 8, 12)), ('diagonal', (0, 8, 12)), ('comb', (0, 8, 12, 16, 40)),
                       ('random3_3', (0, 8, 12, 16)), ('serpentine32', (0, 8, 12, 16, 40)), ('checker8', (0, 8, 12, 16))):
        for tol in tols:
            assert not S.host(name, tol)[2].any(), (name, tol)
    seen = 0
    for name in CASES:
        lab, r, v = S.traced(name)
        for tol in TOLS:
            fl = S.host(name, tol)[2]
            assert not (fl & 2).any()
            for rec, f in zip(r, fl):
                pts = v[rec[2]:rec[2] + rec[3]].tolist()
                if f:
                    k = S.ref_kept(pts, tol)
                    s = S.area2([pts[i] for i in k]) if len(k) >= 3 else 0
                    assert len(pts) > 4 and (s == 0 or (s > 0) != (S.area2(pts) > 0))
                    seen += 1
    assert seen > 0


@pytest.mark.parametrize('name', CASES)
def test_tolerance_0_fills_back_to_the_map(name):
    from wesup_amd import contour as C
    lab, r, v = S.traced(name)
    r2, v2, fl = S.host(name, 0)
    assert len(v2) <= len(v)
    for l in np.unique(lab[lab > 0]).tolist():
        assert (C.rings_to_mask_host(r2, v2, lab.shape, label=l) == (lab == l)).all(), (name, l)
    assert C.simplify_change(lab, r2, v2) == (0, {})


@pytest.mark.parametrize('name', SMALL + ['diamond'])
def test_changed_pixels_lie_within_the_tolerance_of_the_traced_boundary(name):
    from wesup_amd import raster as Rs
    lab, r, v = S.traced(name)
    for tol in TOLS[1:]:
        r2, v2, fl = S.host(name, tol)
        lim = Fraction(tol * tol, 256)
        for l in np.unique(lab[lab > 0]).tolist():
            sel = np.flatnonzero(r2[:, 1] == l)
            pts = [v2[r2[i, 2]:r2[i, 2] + r2[i, 3]] for i in sel]
            first = np.concatenate([[0], np.cumsum([len(p) for p in pts])]).astype(np.int32)
            filled = Rs.fill_host(np.concatenate(pts) * Rs.ONE, first, np.array([0, len(pts)], np.int32), np.zeros(1, np.int32),
                                  lab.shape)[0] > 0
            edges = []
            for i in np.flatnonzero(r[:, 1] == l):
                q = (2 * v[r[i, 2]:r[i, 2] + r[i, 3]]).tolist()                     # doubled: pixel centres are integers
                edges += list(zip(q, q[1:] + q[:1]))
            for rr, cc in np.argwhere(filled != (lab == l)).tolist():
                c = (2 * cc + 1, 2 * rr + 1)
                assert min(S.seg_dist2(c, a, b) for a, b in edges) <= 4 * lim, (name, tol, l, rr, cc)


def test_the_tie_rule_by_name():
    from wesup_amd import contour as C
    lab, r, v = S.traced('diamond')
    assert len(v) == 132 and len(S.host('diamond', 8)[1]) == 68 and len(S.host('diamond', 12)[1]) == 8
    lab, r, v = S.traced('diagonal')
    assert len(v) == 80 and len(S.host('diagonal', 12)[1]) == 3 and not S.host('diagonal', 12)[2].any()
    lab, r, v = S.traced('comb')
    assert len(v) == 258 and len(S.host('comb', 16)[1]) == 192
    # three equidistant maxima: the middle one splits, and its neighbours then lie within half a pixel of the new chords
    r, v = S.make_rings([S.THREE_MAXIMA])
    r2, v2, fl = C.simplify_host(r, v, 8)
    assert v2.tolist() == [[0, 0], [4, 1], [8, 0], [4, -5]] and fl.tolist() == [0]
    assert (np.sign(C.area2_of(r2)) == np.sign(C.area2_of(r))).all()
    # L = 0: five times one point -- every piece runs from the point to itself, D = |p - a|^2 = 0 never exceeds a tolerance
    r, v = S.make_rings([S.ONE_POINT])
    for tol in TOLS:
        r2, v2, fl = C.simplify_host(r, v, tol)
        assert (v2 == v).all() and fl.tolist() == [1] and (r2 == r).all()


def test_hand_made_rings_set_the_flags():
    from wesup_amd import contour as C
    r, v = S.make_rings([S.SLIVER, S.REVERSED, S.OVERSIZE, S.THREE_MAXIMA])
    assert C.area2_of(r)[1] == 11
    r2, v2, fl = C.simplify_host(r, v, 32)
    e = S.ref_simplify(r, v, 32)
    assert (r2 == e[0]).all() and (v2 == e[1]).all() and (fl == e[2]).all()
    assert fl.tolist() == [1, 1, 2, 0]
    assert S.ref_kept(S.SLIVER, 32) == [0, 3] and S.ref_kept(S.REVERSED, 32) == [0, 2, 3, 4]
    assert S.area2([S.REVERSED[k] for k in (0, 2, 3, 4)]) == -5
    n = [len(S.SLIVER), len(S.REVERSED), len(S.OVERSIZE)]
    assert r2[:3, 3].tolist() == n and (v2[:sum(n)] == v[:sum(n)]).all() and (r2[:3] == r[:3]).all()
    assert r2[3, 3] < len(S.THREE_MAXIMA)
    # a span one below stays in the arithmetic
    under = [(x if x < 32768 else 32767, y) for x, y in S.OVERSIZE]
    assert C.simplify_host(*S.make_rings([under]), 32)[2].tolist() == [1]
    r, v = S.make_rings(S.FOUR_FIVE)
    r2, v2, fl = C.simplify_host(r, v, 32)
    assert r2[:, 3].tolist() == [4, 4] and fl.tolist() == [0, 0] and v2[4:].tolist() == [[10, 0], [10, 4], [16, 4], [16, 0]]


def test_arguments_are_checked():
    from wesup_amd import contour as C
    r, v = S.make_rings([S.SLIVER])
    for tol in (-1, 4097, 1.5):
        with pytest.raises(ValueError):
            C.simplify_host(r, v, tol)
    for px in (-0.1, 256.1):
        with pytest.raises(ValueError):
            C.simplify(r, v, px)
    assert [len(C.simplify(r, v, px)[1]) for px in (0, 256)] == [4, 6]
    bad = r.copy()
    bad[0, 3] += 1                       # a range past V
    with pytest.raises(ValueError):
        C.simplify_host(bad, v, 8)
    bad = r.copy()
    bad[0, 2] = 1                        # does not start where the ring in front ended
    with pytest.raises(ValueError):
        C.simplify_host(bad, v[:5], 8)
    e = C.simplify_host(np.zeros((0, 12), np.int32), np.zeros((0, 2), np.int32), 8)
    assert e[0].shape == (0, 12) and e[1].shape == (0, 2) and e[2].shape == (0,)


def _write_maps(tmp_path):
    from PIL import Image
    d = tmp_path / 'pred'
    d.mkdir()
    Image.fromarray((S.ellipses() > 0).astype(np.uint8) * 255).save(d / 'glands.png')
    Image.fromarray((S.diamond() > 0).astype(np.uint8) * 255).save(d / 'diamond.png')
    return d


def test_exports_without_simplify_are_byte_identical(tmp_path):
    from wesup_amd import contour as C
    d = _write_maps(tmp_path)
    logs = [[], []]
    C.export_directory(d, tmp_path / 'a', log=logs[0].append)
    C.export_directory(d, tmp_path / 'b', log=logs[1].append, simplify=None)
    C.main([str(d), str(tmp_path / 'c')])
    for stem in ('glands', 'diamond'):
        a = (tmp_path / 'a' / f'{stem}.geojson').read_bytes()
        assert a == (tmp_path / 'b' / f'{stem}.geojson').read_bytes() == (tmp_path / 'c' / f'{stem}.geojson').read_bytes()
        assert b'simplif' not in a
        # ... and equal to what the functions underneath give when they are called as before
        polys = C.mask_polygons(np.asarray(__import__('PIL.Image').Image.open(d / f'{stem}.png')))
        assert json.dumps(C.to_geojson(polys)).encode() == a
    assert logs[0] == logs[1] and all('simplify' not in line for line in logs[0])


def test_simplify_1_px_writes_closed_outer_first_rings_and_the_two_properties(tmp_path, capsys):
    from wesup_amd import contour as C
    d = _write_maps(tmp_path)
    C.main([str(d), str(tmp_path / 'out'), '--simplify', '1'])
    printed = capsys.readouterr().out
    assert 'glands.png' in printed and 'simplify 1.0 px' in printed and 'pixels change on fill-back' in printed
    C.export_directory(d, tmp_path / 'raw', log=lambda s: None)
    for stem, lab in (('glands', S.ellipses()), ('diamond', S.diamond())):
        doc = json.loads((tmp_path / 'out' / f'{stem}.geojson').read_text())
        raw = json.loads((tmp_path / 'raw' / f'{stem}.geojson').read_text())
        assert len(doc['features']) == len(raw['features']) > 0
        n_doc = n_raw = 0
        for f, g in zip(doc['features'], raw['features']):
            pr = f['properties']
            assert pr['simplify_px'] == 1.0 and isinstance(pr['simplified_area2'], int) and pr['simplified_area2'] > 0
            assert pr['area_px'] == g['properties']['area_px'] and pr['perimeter_px'] == g['properties']['perimeter_px']
            assert abs(pr['simplified_area2'] - 2 * pr['area_px']) <= 2 * pr['perimeter_px']     # within a pixel of every crack
            rings = f['geometry']['coordinates']
            assert len(rings) == len(g['geometry']['coordinates'])
            for i, ring in enumerate(rings):
                assert ring[0] == ring[-1] and len(ring) >= 4
                assert (S.area2([(int(x), int(y)) for x, y in ring[:-1]]) > 0) == (i == 0)        # the outer ring first, then holes
                assert all(p in g['geometry']['coordinates'][i] for p in ring)
            n_doc += sum(len(ring) for ring in rings)
            n_raw += sum(len(ring) for ring in g['geometry']['coordinates'])
        assert n_doc < n_raw
        from wesup_amd import raster
        changed = int((raster.geojson_to_mask(doc, lab.shape) != (lab > 0)).sum())               # (slanted edges: the general fill)
        assert f'{changed} pixels change' in [line for line in printed.splitlines() if line.startswith(stem)][0]
        assert 0 < changed < (lab > 0).sum() // 10


def test_simplify_change_counts_pixels_per_label():
    from wesup_amd import contour as C
    lab, r, v = S.traced('diamond')
    r2, v2, _ = S.host('diamond', 12)
    total, per = C.simplify_change(lab, r2, v2)
    from wesup_amd import raster
    mask = raster.fill(C.polygons(r2, v2), lab.shape) > 0                                        # (slanted edges: the general fill)
    assert total == int((mask != (lab > 0)).sum()) > 0 and per == {1: total}
    lab, r, v = S.traced('random3_3')
    r2, v2, _ = S.host('random3_3', 16)
    total, per = C.simplify_change(lab, r2, v2)
    assert total > 0 and set(per) <= {1, 2, 3} and total <= sum(per.values()) <= 2 * total


def test_entries_workspace_and_host_refusals():
    import ctypes
    from wesup_amd import _lib
    h = _lib.load()
    assert h.wesup_abi_version() == _lib.ABI_VERSION == 6
    assert 'wesup_contour_simplify' in _lib.EXPORTS and 'wesup_contour_simplify_workspace_bytes' in _lib.EXPORTS
    q = h.wesup_contour_simplify_workspace_bytes
    assert q(0, 0) > 0 and q(-1, 4) == 0 and q(1, -4) == 0 and q(5, 4) == 0 and q(1, 2 ** 28 + 1) == 0
    sizes = [q(R, V) for R, V in ((1, 4), (1, 5), (1, 1024), (8, 1024), (8, 1025), (800, 250104), (800, 2 ** 20))]
    assert sizes == sorted(sizes) and sizes[0] < sizes[2] < sizes[-1]
    assert all(q(R, 4096) <= q(R + 1, 4096) for R in (1, 7, 100))
    # the refusals come before any launch: they need no GPU.  Host buffers stand in for the operands.
    R, V = 2, 12
    buf = {k: (ctypes.c_int32 * n)() for k, n in (('rings', 12 * R), ('verts', 2 * V), ('rings_out', 12 * R), ('verts_out', 2 * V),
                                                  ('flags', R), ('counts', 4))}
    nb = q(R, V)
    ws = (ctypes.c_char * (nb + 64))()
    wsp = (ctypes.addressof(ws) + 15) & ~15
    a = {k: ctypes.addressof(b) for k, b in buf.items()}
    assert all(p % 8 == 0 for p in a.values())

    def call(R=R, V=V, tol=8, ws=wsp, nb=nb, **over):
        p = dict(a, **over)
        return h.wesup_contour_simplify(p['rings'], R, p['verts'], V, tol, p['rings_out'], p['verts_out'], p['flags'], p['counts'],
                                        ws, nb, None)

    for k in a:
        assert call(**{k: None}) == -1, k
    assert call(ws=None) == -1 and call(nb=nb - 1) == -1 and call(ws=wsp + 4) == -1
    assert call(R=-1) == -1 and call(V=-1) == -1 and call(R=V + 1) == -1
    assert call(tol=-1) == -1 and call(tol=4097) == -1
    assert call(rings=a['rings'] + 4) == -1 and call(rings_out=a['rings_out'] + 4) == -1            # misaligned records
    assert call(rings_out=a['rings']) == -1 and call(verts_out=a['verts']) == -1 and call(flags=a['counts']) == -1
    assert call(verts_out=a['verts'] + 8) == -1 and call(counts=wsp) == -1                            # overlapping operands


def test_the_wrapper_refuses_host_tensors():
    import torch
    from wesup_amd import _lib, ops
    with pytest.raises(_lib.WesupHipError):
        ops.contour_simplify(torch.zeros(1, 12, dtype=torch.int32), torch.zeros(4, 2, dtype=torch.int32), 8)


def test_split_and_measure_tools_take_simplify(tmp_path):
    """``split.py --geojson DIR --simplify PX`` and ``measure.py --geojson DIR --simplify PX`` on the host: the files parse, carry
    the two properties and fewer vertices, the fill-back difference is logged; without ``--simplify`` they write what they wrote."""
    from wesup_amd import measure as Ms
    from wesup_amd import split as Sp
    d = _write_maps(tmp_path)
    logs = []
    Sp.split_directory(d, tmp_path / 's0', 3, geojson=tmp_path / 'g0', log=lambda s: None)
    Sp.split_directory(d, tmp_path / 's1', 3, geojson=tmp_path / 'g1', simplify=1.0, log=logs.append)
    Sp.main([str(d), str(tmp_path / 's2'), '--radius', '3', '--geojson', str(tmp_path / 'g2')])
    Ms.measure_directory(d, tmp_path / 'm0.csv', geojson=tmp_path / 'h0', log=lambda s: None)
    Ms.measure_directory(d, tmp_path / 'm1.csv', geojson=tmp_path / 'h1', simplify=1.0, log=logs.append)
    Ms.main([str(d), str(tmp_path / 'm2.csv'), '--geojson', str(tmp_path / 'h2')])
    assert (tmp_path / 'm0.csv').read_bytes() == (tmp_path / 'm1.csv').read_bytes() == (tmp_path / 'm2.csv').read_bytes()
    assert sum('pixels change on fill-back' in line for line in logs) == 4
    for raw, same, simp in (('g0', 'g2', 'g1'), ('h0', 'h2', 'h1')):
        for stem in ('glands', 'diamond'):
            a = (tmp_path / raw / f'{stem}.geojson').read_bytes()
            assert a == (tmp_path / same / f'{stem}.geojson').read_bytes() and b'simplif' not in a
            doc, ref = json.loads((tmp_path / simp / f'{stem}.geojson').read_text()), json.loads(a)
            assert len(doc['features']) == len(ref['features']) > 0
            for f, g in zip(doc['features'], ref['features']):
                assert f['properties']['simplify_px'] == 1.0 and 'simplified_area2' in f['properties']
                assert {k: v for k, v in f['properties'].items() if not k.startswith('simplif')} == g['properties']
                assert len(f['geometry']['coordinates'][0]) < len(g['geometry']['coordinates'][0])
    for fn, kw in ((Sp.split_directory, dict(radius=3)), (Ms.measure_directory, {})):
        with pytest.raises(ValueError):
            fn(d, tmp_path / 'x', simplify=1.0, **kw)
