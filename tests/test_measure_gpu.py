"""Object measurements on the device (csrc/measure.hip) against wesup_amd/measure.py:measure_host: every word of the
table and every hull vertex are equal -- the work is integer and independent of the order of the atomics, so there is no
tolerance.  Shapes: the named outline cases, a checkerboard and a serpentine; isolated pixels labelled 1 .. n with L + 1 on both
sides of the LDS-table limit; random maps whose runs cross thread (8 pixels), wave (512) and row boundaries; labels with empty
rows and labels interleaved row by row; one-pixel-wide bars and parabolas whose candidates fill a hull chunk less one, exactly,
plus one and two chunks plus one; a disc of 281 rows; a batch with an empty image; a row, a column and a 4096 x 4096 square of
one label against closed forms (a 32-bit sum or a lost atomic shows there).  A short capacity sets the status and writes
nothing."""
import functools
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from _contourcases import checkerboard, named_cases, random_map, serpentine      # noqa: E402
from _measurecases import bar, disc, empty_rows, full_row, interleaved, isolated_labels, parabola      # noqa: E402

pytestmark = pytest.mark.gpu

DEV = 'cuda:0'
SENTINEL = 0x5a5a5a5a
SENTINEL64 = 0x5a5a5a5a5a5a5a5a
GUARD = 64                 # rows behind table and hull_verts that no call may touch
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _limits():
    from wesup_amd import _lib
    return _lib.MEASURE_LDS_LABELS, _lib.MEASURE_HULL_CHUNK


def _cases():
    lds, chunk = _limits()
    cases = dict(named_cases())
    cases['checker_16x16'] = checkerboard(16, 16)
    cases['serpentine'] = serpentine(64)
    for n in (lds - 2, lds - 1, lds, lds + 1):              # L + 1 = limit - 1, limit (the table in LDS), limit + 1, limit + 2 entries
        cases[f'isolated_{n}'] = isolated_labels(n)
    for k, (h, w) in enumerate([(17, 15), (1, 257), (257, 1), (33, 65), (9, 63), (9, 64), (9, 65)]):
        cases[f'mask_{h}x{w}'] = random_map(10 + k, h, w)
        cases[f'labels_{h}x{w}'] = random_map(20 + k, h, w, n_labels=3)
    cases['dense_19x600'] = (random_map(40, 19, 600) | (np.indices((19, 600))[1] < 560)).astype(np.int32)      # runs longer than a wave's 512 pixels
    cases['empty_rows'] = empty_rows()
    cases['interleaved'] = interleaved()
    for c in (chunk - 1, chunk, chunk + 1, 2 * chunk + 1):  # candidates h + 1
        cases[f'bar_{c}'] = bar(c - 1)
        cases[f'parabola_{c}'] = parabola(c - 1)
    cases['disc_140'] = disc(140)
    cases['batch3'] = np.stack([random_map(31, 19, 23, 2), np.zeros((19, 23), np.int32), np.ones((19, 23), np.int32)])
    cases['empty'] = np.zeros((5, 9), np.int32)
    return cases


CASES = _cases()
NAMES = sorted(CASES)


def _device_d2(lab):
    from wesup_amd import ops
    t = torch.from_numpy(lab).to(DEV)
    return t, ops.edt_sq_full((t > 0).to(torch.uint8))


@functools.lru_cache(maxsize=None)
def _host(name):
    """measure_host of a case with the device's own distance map (checked on its own in tests/test_surface_gpu.py)."""
    from wesup_amd import measure as MS
    lab = CASES[name]
    d2 = _device_d2(lab)[1].cpu().numpy()
    out = MS.measure_host(lab, max(int(lab.max()), 0), d2)
    for a in out:
        a.setflags(write=False)
    return out


def _assert_equal(table, verts, status, want):
    et, ev, es = want
    assert status.tolist() == es.tolist()
    assert table.shape == et.shape and verts.shape == ev.shape
    bad = np.argwhere(table != et)
    assert len(bad) == 0, f'first differing words (image, label, word): {bad[:8].tolist()}: {table[tuple(bad[0])]} for {et[tuple(bad[0])]}'
    bad = np.argwhere(verts != ev)
    assert len(bad) == 0, f'first differing vertices: {bad[:8].tolist()}'


def test_the_cases_are_what_they_claim():
    from wesup_amd import ops
    lds, chunk = _limits()
    assert ops.measure_limits() == (lds, chunk)
    assert int(CASES[f'isolated_{lds - 1}'].max()) + 1 == lds and int(CASES[f'isolated_{lds}'].max()) + 1 == lds + 1
    t = _host(f'parabola_{chunk + 1}')[0][0, 1]
    assert t[8] - t[6] + 2 == chunk + 1 and t[17] == 37      # a vertex per slope of the floor curve, on candidates of all chunks
    assert _host(f'bar_{2 * chunk + 1}')[0][0, 1, 17] == 4
    t = _host('disc_140')[0][0, 1]
    assert t[8] - t[6] + 1 == 281 and t[17] == 96
    assert _host('batch3')[0][1, :, 0].tolist() == [0, 0, 0]
    assert _host('empty_rows')[0][0, 1, 0] == 7


@pytest.mark.parametrize('name', NAMES)
def test_table_and_hulls_equal_the_host_definition(name):
    from wesup_amd import ops
    lab = CASES[name]
    t, d2 = _device_d2(lab)
    table, verts, status = ops.object_measure(t, max(int(lab.max()), 0), d2)
    assert table.is_cuda and verts.is_cuda and status.is_cuda
    assert table.dtype == torch.int64 and verts.dtype == status.dtype == torch.int32
    _assert_equal(table.cpu().numpy(), verts.cpu().numpy(), status.cpu().numpy(), _host(name))


def test_without_a_distance_map_words_21_and_22_are_zero():
    from wesup_amd import measure as MS
    from wesup_amd import ops
    lab = CASES['labels_33x65']
    table, verts, status = ops.object_measure(torch.from_numpy(lab).to(DEV), 3)
    _assert_equal(table.cpu().numpy(), verts.cpu().numpy(), status.cpu().numpy(), MS.measure_host(lab, 3))
    assert (table[:, :, 21:23] == 0).all()


@pytest.mark.parametrize('H,W', [(1, 32768), (32768, 1), (4096, 4096)])
def test_one_label_over_a_large_map_in_closed_form(H, W):
    from wesup_amd import ops
    t = torch.ones(H, W, dtype=torch.int32, device=DEV)
    r = torch.arange(H, device=DEV).view(H, 1)
    c = torch.arange(W, device=DEV).view(1, W)
    d2 = ((r * 7 + c * 13) % 1000).to(torch.int32).contiguous()
    top = int(d2.max())
    first = int((d2.view(-1) == top).nonzero()[0])
    table, verts, status = ops.object_measure(t, 1, d2)
    assert status.tolist() == [0]
    assert table[0, 1].tolist() == full_row(H, W, (top, first)) and (table[0, 0] == 0).all()
    assert verts.tolist() == [[0, 0], [0, H], [W, H], [W, 0]]


def test_an_out_of_range_label_sets_the_status_and_changes_no_other_row():
    from wesup_amd import measure as MS
    from wesup_amd import ops
    lab = random_map(51, 33, 65, 3)
    dirty = lab.copy()
    dirty[5, 7:12] = 9
    dirty[20, 3] = -4
    dirty[32, 64] = 2 ** 31 - 1
    clean = np.where((dirty < 0) | (dirty > 3), 0, dirty).astype(np.int32)
    table, verts, status = ops.object_measure(torch.from_numpy(np.stack([dirty, clean])).to(DEV), 3)
    assert status.tolist() == [1, 0]
    table, verts = table.cpu().numpy(), verts.cpu().numpy()
    _assert_equal(table, verts, np.array([1, 0]), MS.measure_host(np.stack([dirty, clean]), 3))
    assert (table[0, :, :23] == table[1, :, :23]).all()


def _raw(lab, L, n_prof, vert_cap):
    """The entry itself with a guard band behind table and hull_verts -> (status, table incl. band, verts incl. band)."""
    from wesup_amd import _lib, ops
    t = torch.from_numpy(lab).to(DEV)
    t3 = t.unsqueeze(0) if t.dim() == 2 else t
    B, H, W = t3.shape
    table = torch.full((B * (L + 1) + GUARD, 24), SENTINEL64, dtype=torch.int64, device=DEV)
    verts = torch.full((vert_cap + GUARD, 2), SENTINEL, dtype=torch.int32, device=DEV)
    status = torch.full((B,), SENTINEL, dtype=torch.int32, device=DEV)
    nb = _lib.load().wesup_measure_workspace_bytes(B, H, W, L, n_prof)
    assert nb > 0
    ws = torch.empty(nb, dtype=torch.uint8, device=DEV)
    _lib.call('wesup_object_measure', ops._p(t3), None, ops._p(table), ops._p(verts), ops._p(status), B, H, W, L, n_prof, vert_cap,
              ops._p(ws), nb, ops._stream())
    torch.cuda.synchronize()
    return status.cpu().numpy(), table.cpu().numpy(), verts.cpu().numpy()


@pytest.mark.parametrize('name', ['labels_33x65', 'batch3', 'disc_140'])
def test_exact_capacities_are_enough_and_the_band_stays(name):
    from wesup_amd import measure as MS
    from wesup_amd import ops
    lab = CASES[name]
    L = int(lab.max())
    et, ev, es = MS.measure_host(lab, L)
    n_prof = int((et[..., 8] - et[..., 6] + 2)[et[..., 0] > 0].sum())
    assert int(ops.measure_profile_count(torch.from_numpy(lab).to(DEV), L)[0].item()) == n_prof
    status, table, verts = _raw(lab, L, n_prof, len(ev))
    rows = et.reshape(-1, 24)
    assert (status == 0).all()
    assert (table[:len(rows)] == rows).all() and (verts[:len(ev)] == ev).all()
    assert (table[len(rows):] == SENTINEL64).all() and (verts[len(ev):] == SENTINEL).all()


@pytest.mark.parametrize('what', ['n_prof-1', 'vert_cap-1', 'n_prof=0', 'vert_cap=0'])
def test_a_short_capacity_sets_the_status_and_writes_nothing(what):
    from wesup_amd import measure as MS
    name = 'batch3'
    lab = CASES[name]
    L = int(lab.max())
    et, ev, es = MS.measure_host(lab, L)
    n_prof = int((et[..., 8] - et[..., 6] + 2)[et[..., 0] > 0].sum())
    vert_cap = len(ev)
    assert n_prof > 1 and vert_cap > 1
    if what.startswith('n_prof'):
        n_prof = 0 if what.endswith('=0') else n_prof - 1
    else:
        vert_cap = 0 if what.endswith('=0') else vert_cap - 1
    status, table, verts = _raw(lab, L, n_prof, vert_cap)
    assert status.tolist() == [2, 2, 2]
    assert (table == SENTINEL64).all() and (verts == SENTINEL).all()


def test_bad_arguments_are_refused_before_any_launch():
    from wesup_amd import _lib
    h = _lib.load()
    assert h.wesup_object_measure(None, None, None, None, None, 1, 8, 8, 1, 0, 0, None, 0, None) == -1
    assert h.wesup_measure_profile_count(None, None, None, 1, 8, 8, 1, None, 0, None) == -1
    assert h.wesup_measure_workspace_bytes(1, 32769, 8, 1, 0) == 0 and h.wesup_measure_workspace_bytes(1, 8, 8, 2 ** 20, 0) == 0
    assert h.wesup_measure_workspace_bytes(1, 8, 8, 1, -1) == 0 and h.wesup_measure_workspace_bytes(1, 8, 8, 1, 16) > 0
    assert h.wesup_measure_limit(1) == _lib.MEASURE_HULL_CHUNK and h.wesup_measure_limit(2) == _lib.MEASURE_WORDS
    lab = torch.ones(8, 8, dtype=torch.int32, device=DEV)
    out = torch.zeros(64, dtype=torch.int64, device=DEV)
    ws = torch.empty(h.wesup_measure_workspace_bytes(1, 8, 8, 1, 16), dtype=torch.uint8, device=DEV)
    # a workspace one byte short, and a table that overlaps the labels
    assert h.wesup_object_measure(lab.data_ptr(), None, out.data_ptr(), out.data_ptr() + 400, out.data_ptr() + 500, 1, 8, 8, 1, 16, 1,
                                  ws.data_ptr(), ws.numel() - 1, None) == -1
    assert h.wesup_object_measure(lab.data_ptr(), None, lab.data_ptr(), out.data_ptr(), out.data_ptr() + 400, 1, 8, 8, 1, 16, 1,
                                  ws.data_ptr(), ws.numel(), None) == -1


def _mask_with_a_hole():
    mask = (random_map(41, 45, 52) * 255).astype(np.uint8)
    mask[10:30, 10:40] = 255
    mask[15:20, 15:20] = 0
    return mask


def test_measure_on_the_device_equals_the_host_path():
    from wesup_amd import contour as C
    from wesup_amd import measure as MS
    from wesup_amd.utils import metrics as M
    mask = _mask_with_a_hole()
    lab = M.label(mask != 0).astype(np.int32)
    host, dev = MS.measure(lab), MS.measure(lab, device=DEV)
    _assert_equal(dev[0], dev[1], dev[2], host)
    polys = {p['label']: p for p in C.mask_polygons(mask)}
    assert len(polys) == host[0].shape[1] - 1 > 1 and any(p['holes'] for p in polys.values())
    for l, p in polys.items():
        f = MS.features(dev[0][0, l], width=52)
        assert f['area'] == p['area_px'] and f['holes'] == len(p['holes'])
    tens = MS.measure(torch.from_numpy(lab).to(DEV), device=DEV)                # a tensor on the device: L by a read-back
    _assert_equal(tens[0], tens[1], tens[2], host)


def test_command_line_writes_the_same_csv_with_and_without_gpu(tmp_path):
    from PIL import Image
    (tmp_path / 'in').mkdir()
    Image.fromarray(_mask_with_a_hole()).save(tmp_path / 'in' / 'a.png')
    Image.fromarray((random_map(43, 30, 41) * 255).astype(np.uint8)).save(tmp_path / 'in' / 'b.png')
    env = dict(os.environ, PYTHONPATH=ROOT + os.pathsep + os.environ.get('PYTHONPATH', ''))
    for flags, out in ((['--gpu', '-d', DEV], 'gpu.csv'), ([], 'host.csv')):
        subprocess.run([sys.executable, '-m', 'wesup_amd.measure', str(tmp_path / 'in'), str(tmp_path / out), '--min-area', '2',
                        '--scale', '0.5'] + flags, check=True, cwd=tmp_path, env=env, timeout=300)
    text = (tmp_path / 'host.csv').read_text()
    assert text == (tmp_path / 'gpu.csv').read_text() and text.count('\n') > 5


def test_slide_driver_writes_the_table_of_the_written_maps(tmp_path):
    from PIL import Image
    from wesup_amd import slide as S
    from wesup_amd.utils import metrics as M
    import test_slide_gpu as TS                       # the synthetic slide and the weights of the slide tests
    root, ckpt = tmp_path / 'val', tmp_path / 'record' / 'checkpoints' / 'ckpt.0001.pth'
    (root / 'images').mkdir(parents=True)
    (root / 'masks').mkdir()
    ckpt.parent.mkdir(parents=True)
    torch.save({'epoch': 0, 'model_state_dict': {k: torch.from_numpy(v) for k, v in TS._weights().items()}}, ckpt)
    H, W = 100, 90
    Image.fromarray(TS._image(20, H, W)).save(root / 'images' / 'positive-a.jpg', quality=95)
    Image.fromarray((np.random.RandomState(4).rand(H, W) < 0.5).astype(np.uint8) * 255).save(root / 'masks' / 'positive-a.png')
    S.main(root, ckpt, patch_size=80, device=TS.DEV, batch=2, log=lambda *a: None, post_threshold=20, measure=tmp_path / 'tables')
    written = np.asarray(Image.open(tmp_path / 'record' / 'combined-results-for-ckpt.0001.pth' / 'positive-a.png'))
    lines = (tmp_path / 'tables' / 'positive-a.csv').read_text().splitlines()
    inst = M.label(written != 0)
    assert written.any() and len(lines) == 1 + inst.max()
    assert sum(float(l.split(',')[3]) for l in lines[1:]) == (written != 0).sum()
