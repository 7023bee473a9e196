"""Object outlines on the device (csrc/contour.hip) against the sequential tracer wesup_amd/contour.py:trace_host:
the counts, every word of every ring record and every vertex are equal -- the work is integer and its order is defined by the
data, so there is no tolerance.  Shapes: the named cases; random masks and label maps at 16 x 16 (exactly 1024 slots, one scan
block), 17 x 15, 1 x 257 and 257 x 1 (a scan block and one pixel), 33 x 65 and 40 x 40 (several blocks); rings of 1024 and 1026
cracks and maps of 1024 and 1028 cracks, on either side of a power of two in the number of doubling rounds; checkerboards, where
every vertex is a saddle; a serpentine whose one ring is longer than 2048 cracks beside a 4-crack ring.  The refusal path (wrong
totals, a ring capacity one too small) sets the status word and writes nothing."""
import functools
import json
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from _contourcases import checkerboard, isolated_pixels, named_cases, random_map, serpentine      # noqa: E402

pytestmark = pytest.mark.gpu

DEV = 'cuda:0'
SENTINEL = 0x5a5a5a5a
GUARD = 64                 # rows behind rings and verts that no call may touch


def _serpentine_and_a_pixel():
    a = np.zeros((66, 64), np.int32)
    a[:64] = serpentine(64)
    a[65, 63] = 1
    return a


CASES = dict(named_cases())
for _k, (_h, _w) in enumerate([(16, 16), (17, 15), (1, 257), (257, 1), (33, 65), (40, 40)]):
    CASES[f'mask_{_h}x{_w}'] = random_map(10 + _k, _h, _w)
    CASES[f'labels_{_h}x{_w}'] = random_map(20 + _k, _h, _w, n_labels=3)
CASES['batch3'] = np.stack([random_map(31, 19, 23, 2), np.zeros((19, 23), np.int32), np.ones((19, 23), np.int32)])
CASES['checker_16x16'] = checkerboard(16, 16)
CASES['checker_31x33'] = checkerboard(31, 33)
CASES['row512'] = np.ones((1, 512), np.int32)
CASES['isolated_256'] = isolated_pixels(256)
CASES['isolated_257'] = isolated_pixels(257)
CASES['serpentine'] = _serpentine_and_a_pixel()
CASES['empty'] = np.zeros((5, 9), np.int32)
CASES['big_label'] = np.array([[-3, 2 ** 31 - 1, 2 ** 31 - 1], [0, -1, 2 ** 31 - 1], [5, 0, -3]], np.int32)


@functools.lru_cache(maxsize=None)
def _host(name):
    from wesup_amd import contour as C
    out = C.trace_host(CASES[name]) + (C.count_host(CASES[name]),)
    for a in out:
        a.setflags(write=False)
    return out


def test_the_cases_are_what_they_claim():
    r = _host('row511')[0]
    assert r[:, 4].tolist() == [1024]
    assert _host('row512')[0][:, 4].tolist() == [1026]
    assert _host('isolated_256')[3].tolist() == [[1024, 1024]] and _host('isolated_257')[3].tolist() == [[1028, 1028]]
    r = _host('serpentine')[0]
    assert len(r) == 2 and r[0, 4] > 2048 and r[1, 4] == 4
    assert _host('batch3')[2].tolist()[1:] == [0, 1]
    r, v, n, c = _host('checker_16x16')
    assert c[0, 0] == 4 * 128 and len(r) < 128                    # the pixels hang together through their corners


@pytest.mark.parametrize('name', list(CASES))
def test_count_and_trace_equal_the_host_tracer(name):
    from wesup_amd import ops
    lab = CASES[name]
    er, ev, en, ec = _host(name)
    t = torch.from_numpy(lab).to(DEV)
    counts = ops.contour_count(t)
    assert counts.dtype == torch.int32 and counts.is_cuda
    assert counts.cpu().numpy().tolist() == ec.tolist()
    rings, verts, n_rings = ops.contour_trace(t)
    assert rings.is_cuda and verts.is_cuda and n_rings.is_cuda
    assert rings.dtype == verts.dtype == n_rings.dtype == torch.int32
    r, v, n = rings.cpu().numpy(), verts.cpu().numpy(), n_rings.cpu().numpy()
    assert n.tolist() == en.tolist()
    assert r.shape == er.shape and v.shape == ev.shape
    bad = np.argwhere(r != er)
    assert len(bad) == 0, f'first differing record words (ring, word): {bad[:8].tolist()}'
    bad = np.argwhere(v != ev)
    assert len(bad) == 0, f'first differing vertices: {bad[:8].tolist()}'


def _raw_trace(lab, n_cracks, n_corners, ring_cap):
    """The entry itself with a guard band behind rings and verts -> (status, rings incl. band, verts incl. band, n_rings)."""
    from wesup_amd import _lib, ops
    t = torch.from_numpy(lab).to(DEV)
    t3 = t.unsqueeze(0) if t.dim() == 2 else t
    B, H, W = t3.shape
    rings = torch.full((ring_cap + GUARD, 12), SENTINEL, dtype=torch.int32, device=DEV)
    verts = torch.full((n_corners + GUARD, 2), SENTINEL, dtype=torch.int32, device=DEV)
    n_rings = torch.full((B,), SENTINEL, dtype=torch.int32, device=DEV)
    status = torch.zeros(1, dtype=torch.int32, device=DEV)
    nb = _lib.load().wesup_contour_trace_workspace_bytes(B, H, W, n_cracks)
    assert nb > 0
    ws = torch.empty(nb, dtype=torch.uint8, device=DEV)
    _lib.call('wesup_contour_trace', ops._p(t3), ops._p(rings), ops._p(verts), ops._p(n_rings), ops._p(status), B, H, W,
              n_cracks, n_corners, ring_cap, ops._p(ws), nb, ops._stream())
    torch.cuda.synchronize()
    return int(status.item()), rings.cpu().numpy(), verts.cpu().numpy(), n_rings.cpu().numpy()


@pytest.mark.parametrize('name', ['labels_33x65', 'batch3', 'serpentine'])
def test_exact_capacities_are_enough_and_the_band_stays(name):
    er, ev, en, ec = _host(name)
    n_cracks, n_corners = (int(x) for x in ec.sum(0))
    status, r, v, n = _raw_trace(CASES[name], n_cracks, n_corners, len(er))
    assert status == 0 and n.tolist() == en.tolist()
    assert (r[:len(er)] == er).all() and (v[:len(ev)] == ev).all()
    assert (r[len(er):] == SENTINEL).all() and (v[len(ev):] == SENTINEL).all()


@pytest.mark.parametrize('what', ['cracks-4', 'cracks+4', 'corners-2', 'corners+2', 'ring_cap-1', 'ring_cap=0'])
def test_wrong_totals_and_a_short_ring_capacity_set_the_status_and_write_nothing(what):
    name = 'labels_33x65'
    er, ev, en, ec = _host(name)
    n_cracks, n_corners = (int(x) for x in ec.sum(0))
    ring_cap = len(er)
    assert ring_cap > 1 and n_corners > 2
    if what.startswith('cracks'):
        n_cracks += int(what[6:])
    elif what.startswith('corners'):
        n_corners += int(what[7:])
    else:
        ring_cap = 0 if what.endswith('=0') else ring_cap - 1
    status, r, v, n = _raw_trace(CASES[name], n_cracks, n_corners, ring_cap)
    assert status == 1
    assert (r == SENTINEL).all() and (v == SENTINEL).all()
    assert (n == 0).all()


def test_status_raises_in_the_wrapper(monkeypatch):
    from wesup_amd import _lib, ops
    t = torch.from_numpy(CASES['mask_17x15']).to(DEV)
    wrong = torch.tensor([[4, 4]], dtype=torch.int32, device=DEV)
    monkeypatch.setattr(ops, 'contour_count', lambda l3: wrong)
    with pytest.raises(_lib.WesupHipError, match='status 1'):
        ops.contour_trace(t)


def test_mask_polygons_on_the_device_equal_the_host_path():
    from wesup_amd import contour as C
    mask = (random_map(41, 45, 52) * 255).astype(np.uint8)
    mask[10:30, 10:40] = 255
    mask[15:20, 15:20] = 0
    host, dev = C.mask_polygons(mask, min_area=3), C.mask_polygons(mask, DEV, min_area=3)
    assert len(host) == len(dev) > 1 and any(p['holes'] for p in host)
    for a, b in zip(host, dev):
        assert {k: v for k, v in a.items() if k not in ('outer', 'holes')} == {k: v for k, v in b.items() if k not in ('outer', 'holes')}
        assert (a['outer'] == b['outer']).all() and len(a['holes']) == len(b['holes'])
        assert all((x == y).all() for x, y in zip(a['holes'], b['holes']))
    cmap = random_map(42, 23, 31, n_labels=3).astype(np.uint8)
    hc, dc = C.classmap_polygons(cmap, 4), C.classmap_polygons(cmap, 4, DEV)
    assert json.dumps(C.to_geojson(hc)) == json.dumps(C.to_geojson(dc)) and {p['class'] for p in hc} == {1, 2, 3}
    r, v, n = C.trace(cmap.astype(np.int32), DEV)
    er, ev, en = C.trace_host(cmap)
    assert (r == er).all() and (v == ev).all() and (n == en).all()


def test_slide_driver_writes_outlines_of_the_written_maps(tmp_path):
    from PIL import Image
    from wesup_amd import contour as C
    from wesup_amd import slide as S
    import test_slide_gpu as TS                       # the synthetic slide and the weights of the slide tests
    root, ckpt = tmp_path / 'val', tmp_path / 'record' / 'checkpoints' / 'ckpt.0001.pth'
    (root / 'images').mkdir(parents=True)
    (root / 'masks').mkdir()
    ckpt.parent.mkdir(parents=True)
    torch.save({'epoch': 0, 'model_state_dict': {k: torch.from_numpy(v) for k, v in TS._weights().items()}}, ckpt)
    sizes = {'positive-a': (100, 90), 'negative-b': (70, 120)}
    rs = np.random.RandomState(4)
    for seed, (stem, (H, W)) in enumerate(sizes.items()):
        Image.fromarray(TS._image(20 + seed, H, W)).save(root / 'images' / f'{stem}.jpg', quality=95)
        Image.fromarray((rs.rand(H, W) < 0.5).astype(np.uint8) * 255).save(root / 'masks' / f'{stem}.png')
    gj = tmp_path / 'outlines'
    S.main(root, ckpt, patch_size=80, device=TS.DEV, batch=2, log=lambda *a: None, post_threshold=20, geojson=gj)
    out = tmp_path / 'record' / 'combined-results-for-ckpt.0001.pth'
    assert sorted(q.name for q in gj.iterdir()) == ['negative-b.geojson', 'positive-a.geojson']
    for stem, shape in sizes.items():
        written = np.asarray(Image.open(out / f'{stem}.png'))
        doc = json.loads((gj / f'{stem}.geojson').read_text())
        assert written.shape == shape and written.any()
        assert (C.geojson_to_mask_host(doc, shape) == (written != 0)).all()
        assert sum(f['properties']['area_px'] for f in doc['features']) == (written != 0).sum()
