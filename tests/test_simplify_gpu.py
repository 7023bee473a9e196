"""Ring simplification on the device (csrc/contour.hip, ops.contour_simplify) against the host definition
wesup_amd/contour.py:simplify_host: ring records, vertices, flags and counts are equal word for word -- the work is integer and
its result does not depend on the order of the atomics, so there is no tolerance.  The rings come from ops.contour_trace, so the
chain stays on the device.  Shapes: every case and tolerance of the CPU tests; a batch of two maps; random_map(43, 64, 64), whose
largest ring (1326 vertices) is longer than a block and than the LDS form (896); a diamond ring of 2724 vertices, where every
per-thread loop wraps twice; the comb, 127 levels deep; 1156 plus signs, more rings than the grid has blocks; hand-made rings of 4
and 5 vertices side by side, the flagged rings, the three maxima and the one-point ring; R = 0."""
import functools
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _simplifycases as S      # noqa: E402
from _simplifycases import TOLS      # noqa: E402
from _contourcases import random_map      # noqa: E402

pytestmark = pytest.mark.gpu

DEV = 'cuda:0'
SENTINEL = 0x5a5a5a5a
GUARD = 64


@functools.lru_cache(maxsize=None)
def _maps():
    out = S.label_cases()
    out['batch2'] = np.stack([S.diamond(), np.pad(random_map(4, 13, 13, 3), ((0, 27), (0, 27)))])
    out['random64'] = random_map(43, 64, 64)
    out['big_diamond'] = S.big_diamond()
    out['plus_lattice'] = S.plus_lattice()
    return out


NAMES = list(S.label_cases()) + ['batch2', 'random64', 'big_diamond', 'plus_lattice']


@functools.lru_cache(maxsize=None)
def _traced(name):
    """The rings of a map from the device tracer: (rings, verts) on the device, and their copies."""
    from wesup_amd import ops
    r, v, _ = ops.contour_trace(torch.from_numpy(_maps()[name]).to(DEV))
    return r, v, r.cpu().numpy(), v.cpu().numpy()


def _same(got, want, what):
    got = got.cpu().numpy()
    assert got.shape == want.shape, (what, got.shape, want.shape)
    bad = np.argwhere(got != want)
    assert len(bad) == 0, f'{what}: first differing words {bad[:8].tolist()}'


def _check(r, v, rh, vh, tol):
    from wesup_amd import contour as C
    from wesup_amd import ops
    er, ev, ef = C.simplify_host(rh, vh, tol)
    r2, v2, fl, counts = ops.contour_simplify(r, v, tol)
    assert all(t.is_cuda and t.dtype == torch.int32 for t in (r2, v2, fl, counts))
    _same(r2, er, f'rings at {tol}')
    _same(v2, ev, f'vertices at {tol}')
    _same(fl, ef, f'flags at {tol}')
    assert counts.tolist() == [len(ev), int((ef == 1).sum()), int((ef == 2).sum()), 0]
    return er, ev, ef


def test_the_cases_are_what_they_claim():
    assert _traced('random64')[2][:, 3].max() == 1326
    assert _traced('big_diamond')[2][:, 3].tolist() == [2724]
    assert len(_traced('plus_lattice')[2]) == 34 * 34 > 1024 and set(_traced('plus_lattice')[2][:, 3].tolist()) == {12}
    assert _traced('comb')[2][:, 3].tolist() == [258]
    assert len(set(_traced('batch2')[2][:, 0].tolist())) == 2


@pytest.mark.parametrize('name', NAMES)
def test_simplify_equals_the_host_definition(name):
    r, v, rh, vh = _traced(name)
    for tol in TOLS:
        _check(r, v, rh, vh, tol)


def test_hand_made_rings_flags_and_short_rings():
    lists = [S.SLIVER, S.REVERSED, S.OVERSIZE, S.THREE_MAXIMA, S.ONE_POINT] + S.FOUR_FIVE
    rh, vh = S.make_rings(lists)
    r, v = torch.from_numpy(rh).to(DEV), torch.from_numpy(vh).to(DEV)
    er, ev, ef = _check(r, v, rh, vh, 32)
    assert ef.tolist() == [1, 1, 2, 0, 1, 0, 0] and er[5:, 3].tolist() == [4, 4]
    er, ev, ef = _check(r, v, rh, vh, 8)
    assert ef.tolist()[2] == 2 and er[3, 3] == 4                       # the three maxima: the middle one stays
    for tol in (0, 4096):
        _check(r, v, rh, vh, tol)


def test_no_rings():
    from wesup_amd import _lib, ops
    e = torch.empty(0, 12, dtype=torch.int32, device=DEV)
    r2, v2, fl, counts = ops.contour_simplify(e, torch.empty(0, 2, dtype=torch.int32, device=DEV), 8)
    assert r2.shape == (0, 12) and v2.shape == (0, 2) and fl.shape == (0,) and counts.tolist() == [0, 0, 0, 0]
    r, v, _ = ops.contour_trace(torch.zeros(5, 9, dtype=torch.int32, device=DEV))
    assert ops.contour_simplify(r, v, 8)[1].shape == (0, 2)
    with pytest.raises(_lib.WesupHipError):
        ops.contour_simplify(e, torch.zeros(4, 2, dtype=torch.int32, device=DEV), 8)
    with pytest.raises(_lib.WesupHipError):
        ops.contour_simplify(r, v, 4097)


def _raw(rh, vh, tol):
    """The entry itself with guard bands behind rings_out, verts_out and flags."""
    from wesup_amd import _lib, ops
    R, V = len(rh), len(vh)
    r, v = torch.from_numpy(rh).to(DEV), torch.from_numpy(vh).to(DEV)
    r2 = torch.full((R + GUARD, 12), SENTINEL, dtype=torch.int32, device=DEV)
    v2 = torch.full((V + GUARD, 2), SENTINEL, dtype=torch.int32, device=DEV)
    fl = torch.full((R + GUARD,), SENTINEL, dtype=torch.int32, device=DEV)
    counts = torch.full((4,), SENTINEL, dtype=torch.int32, device=DEV)
    nb = _lib.load().wesup_contour_simplify_workspace_bytes(R, V)
    assert nb > 0
    ws = torch.empty(nb, dtype=torch.uint8, device=DEV)
    _lib.call('wesup_contour_simplify', ops._p(r), R, ops._p(v), V, tol, ops._p(r2), ops._p(v2), ops._p(fl), ops._p(counts),
              ops._p(ws), nb, ops._stream())
    torch.cuda.synchronize()
    return r2.cpu().numpy(), v2.cpu().numpy(), fl.cpu().numpy(), counts.cpu().numpy()


@pytest.mark.parametrize('name', ['random64', 'ellipses'])
def test_guard_bands_stay_and_a_second_run_gives_the_same_words(name):
    from wesup_amd import contour as C
    _, _, rh, vh = _traced(name)
    er, ev, ef = C.simplify_host(rh, vh, 16)
    a, b = _raw(rh, vh, 16), _raw(rh, vh, 16)
    for x, y in zip(a, b):
        assert (x == y).all()
    r2, v2, fl, counts = a
    R, K = len(er), len(ev)
    assert counts.tolist() == [K, 0, 0, 0] and K < len(vh)
    assert (r2[:R] == er).all() and (v2[:K] == ev).all() and (fl[:R] == ef).all()
    assert (r2[R:] == SENTINEL).all() and (v2[K:] == SENTINEL).all() and (fl[R:] == SENTINEL).all()


@pytest.mark.parametrize('what', ['past V', 'a gap', 'an empty ring', 'short of V'])
def test_a_broken_record_sets_the_status_and_writes_no_vertex(what):
    from wesup_amd import _lib, ops
    _, _, rh, vh = _traced('ellipses')
    rh = rh.copy()
    if what == 'past V':
        rh[-1, 3] += 1
    elif what == 'a gap':
        rh[3, 2] += 1
    elif what == 'an empty ring':
        rh[2, 3] = 0
    else:
        vh = np.concatenate([vh, vh[:1]])
    r2, v2, fl, counts = _raw(rh, vh, 16)
    assert counts.tolist() == [0, 0, 0, 1]
    assert (v2 == SENTINEL).all() and (r2 == SENTINEL).all() and (fl == SENTINEL).all()
    with pytest.raises(_lib.WesupHipError, match='status 1'):
        ops.contour_simplify(torch.from_numpy(rh).to(DEV), torch.from_numpy(vh).to(DEV), 16)


@pytest.mark.parametrize('name', ['ellipses', 'random3_3', 'batch2'])
def test_simplify_change_on_the_device_equals_the_host(name):
    from wesup_amd import contour as C
    lab = _maps()[name]
    _, _, rh, vh = _traced(name)
    for tol in (0, 16, 40):
        r2, v2, _ = C.simplify_host(rh, vh, tol)
        host = C.simplify_change(lab, r2, v2)
        assert C.simplify_change(lab, r2, v2, DEV) == host
        assert (host[0] == 0) == (tol == 0)


def test_the_python_layer_on_the_device_equals_the_host_path(tmp_path):
    import json
    from PIL import Image
    from wesup_amd import contour as C
    _, _, rh, vh = _traced('ellipses')
    for a, b in zip(C.simplify(rh, vh, 1.0), C.simplify(rh, vh, 1.0, DEV)):
        assert a.shape == b.shape and (a == b).all()
    mask = (S.ellipses() > 0).astype(np.uint8) * 255
    hs, ds = {}, {}
    host, dev = C.mask_polygons(mask, simplify=1.5, stats=hs), C.mask_polygons(mask, DEV, simplify=1.5, stats=ds)
    assert json.dumps(C.to_geojson(host)) == json.dumps(C.to_geojson(dev)) and hs == ds and hs['kept'] < hs['vertices']
    cmap = (S.ellipses() % 3).astype(np.uint8)
    assert json.dumps(C.to_geojson(C.classmap_polygons(cmap, 3, simplify=1.0))) == \
        json.dumps(C.to_geojson(C.classmap_polygons(cmap, 3, DEV, simplify=1.0)))
    d = tmp_path / 'pred'
    d.mkdir()
    Image.fromarray(mask).save(d / 'glands.png')
    logs = [[], []]
    C.export_directory(d, tmp_path / 'h', simplify=1.0, log=logs[0].append)
    C.export_directory(d, tmp_path / 'g', DEV, simplify=1.0, log=logs[1].append)
    assert (tmp_path / 'h' / 'glands.geojson').read_bytes() == (tmp_path / 'g' / 'glands.geojson').read_bytes()
    assert logs[0] == logs[1] and 'pixels change on fill-back' in logs[0][0]


def test_slide_driver_simplifies_the_outlines_it_writes(tmp_path):
    """``slide.py --geojson DIR --simplify PX``: the combined maps are written as before, the outlines carry the two properties
    and fewer vertices, and the log names what the fill-back changed."""
    import json
    from PIL import Image
    from wesup_amd import slide as Sl
    import test_slide_gpu as TS                       # the synthetic slide and the weights of the slide tests
    root, ckpt = tmp_path / 'val', tmp_path / 'record' / 'checkpoints' / 'ckpt.0001.pth'
    (root / 'images').mkdir(parents=True)
    (root / 'masks').mkdir()
    ckpt.parent.mkdir(parents=True)
    torch.save({'epoch': 0, 'model_state_dict': {k: torch.from_numpy(v) for k, v in TS._weights().items()}}, ckpt)
    H, W = 100, 90
    Image.fromarray(TS._image(20, H, W)).save(root / 'images' / 'positive-a.jpg', quality=95)
    Image.fromarray((np.random.RandomState(4).rand(H, W) < 0.5).astype(np.uint8) * 255).save(root / 'masks' / 'positive-a.png')
    logs = []
    Sl.main(root, ckpt, patch_size=80, device=TS.DEV, batch=2, log=lambda *a: logs.append(' '.join(str(x) for x in a)),
            post_threshold=20, geojson=tmp_path / 'simple', simplify=1.0)
    out = tmp_path / 'record' / 'combined-results-for-ckpt.0001.pth'
    written = np.asarray(Image.open(out / 'positive-a.png'))
    Sl.main(root, ckpt, patch_size=80, device=TS.DEV, batch=2, log=lambda *a: None, post_threshold=20, geojson=tmp_path / 'raw')
    assert (np.asarray(Image.open(out / 'positive-a.png')) == written).all() and written.any()
    doc = json.loads((tmp_path / 'simple' / 'positive-a.geojson').read_text())
    raw = json.loads((tmp_path / 'raw' / 'positive-a.geojson').read_text())
    assert len(doc['features']) == len(raw['features']) > 0 and b'simplif' not in (tmp_path / 'raw' / 'positive-a.geojson').read_bytes()
    count = lambda d: sum(len(r) for f in d['features'] for r in f['geometry']['coordinates'])
    assert count(doc) < count(raw)
    assert all(f['properties']['simplify_px'] == 1.0 and f['properties']['area_px'] == g['properties']['area_px']
               for f, g in zip(doc['features'], raw['features']))
    line = [s for s in logs if 'pixels change on fill-back' in s]
    assert len(line) == 1 and line[0].startswith('positive-a: simplify 1.0 px')
    with pytest.raises(ValueError):
        Sl.main(root, ckpt, patch_size=80, device=TS.DEV, skip_infer=True, simplify=1.0, log=lambda *a: None)
