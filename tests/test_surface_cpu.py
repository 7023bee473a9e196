"""Surface-distance metrics: the numpy definitions of wesup_amd/surface.py against scipy and numpy, their
conventions, the new columns of evaluate.score and its command line, and the host-side checks of the new C entries.  No GPU."""
import math
import os
import re
import subprocess

import numpy as np
import pytest
from scipy import ndimage

from wesup_amd import evaluate, surface
from wesup_amd.utils import metrics as M

from _splitcases import disc_scene, write_scene
from _surfacecases import blob_pairs, border_scipy, directed_scipy, edt_cases, edt_sq_scipy

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CASES = edt_cases()


@pytest.mark.parametrize('name,mask', CASES, ids=[c[0] for c in CASES])
def test_edt_sq_full_host_equals_scipy(name, mask):
    got = surface.edt_sq_full_host(mask)
    assert got.dtype == np.int32 and got.shape == mask.shape
    assert np.array_equal(got, edt_sq_scipy(mask))


def test_edt_sq_full_host_edges():
    assert (surface.edt_sq_full_host(np.ones((9, 13), np.uint8)) == surface.EDT_NONE).all()
    assert surface.EDT_NONE == 2 ** 31 - 1
    assert (surface.edt_sq_full_host(np.zeros((9, 13), np.uint8)) == 0).all()
    row = np.array([[7, 1, 0, 1, 1, 255, 1]], np.uint8)                            # any dtype, non-zero = foreground
    assert surface.edt_sq_full_host(row).tolist() == [[4, 1, 0, 1, 4, 9, 16]]
    assert surface.edt_sq_full_host(row.T.astype(np.float32)).tolist() == [[4], [1], [0], [1], [4], [9], [16]]
    both = surface.edt_sq_full_host(np.stack([row, row == 0]))                      # images of a batch do not see each other
    assert both.tolist() == [[[4, 1, 0, 1, 4, 9, 16]], [[0, 0, 1, 0, 0, 0, 0]]]
    far = np.ones((300, 300), bool)                                                # beyond the cap of split.edt_sq_host
    far[0, 0] = False
    assert surface.edt_sq_full_host(far).max() == 2 * 299 * 299 == 178802
    with pytest.raises(ValueError):
        surface.edt_sq_full_host(np.ones((2, 3, 4, 5)))
    with pytest.raises(ValueError):
        surface.edt_sq_full_host(np.broadcast_to(np.uint8(1), (1, 46342)))          # 46341^2 >= 2^31 - 1
    assert surface.edt_sq_full_host(np.broadcast_to(np.uint8(0), (1, 46341))).max() == 0


@pytest.mark.parametrize('name,mask', CASES, ids=[c[0] for c in CASES])
def test_border_host_equals_scipy(name, mask):
    got = surface.border_host(mask)
    assert got.dtype == bool and np.array_equal(got, border_scipy(mask))


@pytest.mark.parametrize('seed', range(len(blob_pairs())))
def test_scores_equal_their_definitions(seed):
    pred, gt = blob_pairs()[seed]
    d_pg, d_gp = directed_scipy(pred, gt)
    assert d_pg.size and d_gp.size
    for tau in (2.0, 1.0, 0.5, 3.7):
        s = surface.surface_scores_host(pred, gt, tau)
        assert set(s) == {'hd', 'hd95', 'assd', 'nsd'}
        assert s['hd95'] == np.percentile(np.hstack((d_pg, d_gp)), 95)             # MedPy's hd95
        assert s['assd'] == (d_pg.mean() + d_gp.mean()) / 2                        # MedPy's assd
        assert s['nsd'] == ((d_pg <= tau).sum() + (d_gp <= tau).sum()) / (d_pg.size + d_gp.size)
        assert s['hd'] == max(d_pg.max(), d_gp.max())
    assert surface.surface_scores_host(pred, gt) == surface.surface_scores_host(pred, gt, 2.0)      # the interface default
    st = surface.surface_stats_host(pred, gt, 2.0)
    assert tuple(st) == surface.STAT_KEYS
    both = np.sort(np.rint(np.hstack((d_pg, d_gp)) ** 2).astype(np.int64))
    k = int(math.floor((both.size - 1) * (95.0 / 100.0)))
    assert (st['lo'], st['hi']) == (both[k], both[min(k + 1, both.size - 1)])
    assert all(isinstance(st[key], int) for key in surface.STAT_KEYS[:8])
    for q in (0.0, 50.0, 100.0):                                                   # the percentile rule at other ranks
        got = surface.scores_from_stats(surface.surface_stats_host(pred, gt, 2.0, q), q)['hd95']
        assert got == np.percentile(np.hstack((d_pg, d_gp)), q)


@pytest.mark.parametrize('seed', range(len(blob_pairs())))
def test_hausdorff_full_host_equals_metrics_hausdorff(seed):
    pred, gt = blob_pairs()[seed]
    assert surface.hausdorff_full_host(pred, gt) == M.hausdorff(pred, gt)
    assert surface.hausdorff_full_host(gt, pred) == M.hausdorff(gt, pred)


def test_conventions():
    empty = np.zeros((20, 30), bool)
    disc = np.zeros((20, 30), bool)
    yy, xx = np.mgrid[:20, :30]
    disc[(yy - 10) ** 2 + (xx - 12) ** 2 <= 36] = True
    assert surface.surface_scores_host(empty, empty) == {'hd': 0.0, 'hd95': 0.0, 'assd': 0.0, 'nsd': 1.0}
    for a, b in ((empty, disc), (disc, empty)):
        assert surface.surface_scores_host(a, b) == {'hd': math.inf, 'hd95': math.inf, 'assd': math.inf, 'nsd': 0.0}
    assert surface.surface_scores_host(disc, disc) == {'hd': 0.0, 'hd95': 0.0, 'assd': 0.0, 'nsd': 1.0}
    assert surface.hausdorff_full_host(empty, empty) == 0 and surface.hausdorff_full_host(empty, disc) == np.inf
    shifted = np.roll(disc, 1, axis=1)
    assert surface.surface_scores_host(disc, shifted, 1.0)['nsd'] == 1.0
    assert surface.surface_scores_host(disc, shifted, 0.5)['nsd'] < 1.0
    st = surface.surface_stats_host(empty, disc, 2.0)
    assert st['n_p'] == 0 and st['max_pg'] == 0 and st['sum_pg'] == 0.0 and st['lo'] == st['hi'] == st['max_gp'] == surface.EDT_NONE
    st = surface.surface_stats_host(empty, empty, 2.0)
    assert [st[k] for k in surface.STAT_KEYS] == [0] * 10
    for bad in (-1.0, math.inf, math.nan):
        with pytest.raises(ValueError):
            surface.surface_scores_host(disc, disc, bad)
    with pytest.raises(ValueError):
        surface.surface_scores_host(disc, disc[:-1])
    # one full image against a disc: the border of a full image is the image's frame
    full = np.ones((20, 30), bool)
    assert surface.border_host(full).sum() == 2 * 20 + 2 * 30 - 4


def test_classes_host():
    rng = np.random.default_rng(3)
    gt = np.zeros((64, 48), np.uint8)
    gt[10:40, 5:30] = 1
    gt[30:60, 25:45] = 2
    pred = np.roll(gt, (1, -2), (0, 1))
    pred[rng.random(pred.shape) < 0.01] = 0
    rows = surface.surface_scores_classes_host(pred, gt, 3, 2.0)
    assert len(rows) == 3
    for c in range(3):
        assert rows[c] == surface.surface_scores_host(pred == c, gt == c, 2.0)
    assert surface.surface_scores_classes(pred, gt, 3) == rows                     # no device: the host route
    with pytest.raises(ValueError):
        surface.surface_scores_classes_host(pred, gt, 0)


def test_score_rows_without_and_with_surface():
    pred, gt = disc_scene()
    pred = pred.astype(np.float64)
    rows0, means0 = evaluate.score([pred], [gt])
    assert list(rows0[0]) == ['accuracy', 'dice', 'detection_f1', 'object_dice', 'object_hausdorff']
    assert rows0[0] == {'accuracy': float(M.accuracy(pred, gt)), 'dice': float(M.dice(pred, gt)),
                        'detection_f1': float(M.detection_f1(pred, gt)), 'object_dice': float(M.object_dice(pred, gt)),
                        'object_hausdorff': 59.0}
    rows_none, means_none = evaluate.score([pred], [gt], surface=None)
    assert rows_none == rows0 and means_none == means0
    rows1, means1 = evaluate.score([pred, np.zeros_like(pred)], [gt, gt], surface=2.0)
    assert list(rows1[0]) == list(rows0[0]) + ['hd95', 'assd', 'nsd'] and len(rows1[0]) == 8
    assert {k: rows1[0][k] for k in rows0[0]} == rows0[0]
    s = surface.surface_scores_host(pred != 0, gt > 0, 2.0)                        # the ground truth binarised for these columns
    assert [rows1[0][k] for k in ('hd95', 'assd', 'nsd')] == [s['hd95'], s['assd'], s['nsd']]
    assert math.isnan(rows1[1]['hd95']) and math.isnan(rows1[1]['assd']) and rows1[1]['nsd'] == 0.0      # inf is written as nan
    assert means1['hd95'] == s['hd95'] and means1['nsd'] == s['nsd'] / 2


def test_evaluate_command_line(tmp_path):
    pred_dir, gt_dir = write_scene(tmp_path)
    root, gts = tmp_path / 'run', tmp_path / 'data'
    (root / 'testA').mkdir(parents=True)
    (gts / 'testA' / 'masks').mkdir(parents=True)
    for src, dst in ((pred_dir, root / 'testA'), (gt_dir, gts / 'testA' / 'masks')):
        (dst / 'scene.png').write_bytes((src / 'scene.png').read_bytes())
    pred, gt = disc_scene()
    f1, od = float(M.detection_f1(pred.astype(np.float64), gt)), float(M.object_dice(pred.astype(np.float64), gt))
    before = f',detection_f1,object_dice,object_hausdorff\r\nscene.png,{f1},{od},59.0\r\n'.encode()
    lines = []
    evaluate.evaluate_split(pred_dir, gt_dir, None, tmp_path / 'split.csv', 100, lines.append)
    assert (tmp_path / 'split.csv').read_bytes() == before and len(lines) == 5
    evaluate.main([str(root), '--gt-root', str(gts), '--min-size', '100'])          # without the flag: the bytes of before
    assert (root / 'testA.csv').read_bytes() == before
    evaluate.main([str(root), '--gt-root', str(gts), '--min-size', '100', '--surface-metrics'])
    s = surface.surface_scores_host(pred, gt > 0, 2.0)
    after = (f',detection_f1,object_dice,object_hausdorff,hd95,assd,nsd\r\n'
             f'scene.png,{f1},{od},59.0,{s["hd95"]},{s["assd"]},{s["nsd"]}\r\n').encode()
    assert (root / 'testA.csv').read_bytes() == after
    lines = []
    rows, means = evaluate.evaluate_split(pred_dir, gt_dir, None, None, 100, lines.append, surface_tolerance=1.5)
    assert len(lines) == 8 and lines[0].startswith('Accuracy: ') and lines[4] == 'Object Hausdorff: 59.0'
    assert lines[5] == f'HD95: {means["hd95"]}' and lines[6] == f'ASSD: {means["assd"]}' and lines[7] == f'NSD@1.5: {means["nsd"]}'
    _, means_flat, _ = evaluate.evaluate_flat(pred_dir, gt_dir, 100, lambda *a: None, surface_tolerance=1.5)
    assert means_flat == means
    a = evaluate.build_parser().parse_args(['preds', '--dataset', 'crag', '--surface-metrics', '3.5'])
    assert a.surface_metrics == 3.5 and evaluate.build_parser().parse_args(['preds']).surface_metrics is None
    assert evaluate.build_parser().parse_args(['preds', '--surface-metrics']).surface_metrics == 2.0


def test_surface_command_line(tmp_path):
    pred_dir, gt_dir = write_scene(tmp_path)
    lines = []
    rows, means = surface.score_directory(pred_dir, gt_dir, 2.0, log=lines.append)
    pred, gt = disc_scene()
    s = surface.surface_scores_host(pred, gt, 2.0)
    assert rows == [{'name': 'scene.png', 'class': '', **s}] and means == s and len(lines) == 4
    surface.main([str(pred_dir), str(gt_dir), '--tolerance', '1', '--csv', str(tmp_path / 's.csv')])
    s1 = surface.surface_scores_host(pred, gt, 1.0)
    assert (tmp_path / 's.csv').read_bytes() == (',class,hd,hd95,assd,nsd\r\n'
                                                 f'scene.png,,{s1["hd"]},{s1["hd95"]},{s1["assd"]},{s1["nsd"]}\r\n').encode()
    # class-index maps: the ground truth of the scene holds the ids 0, 1, 2
    rows, _ = surface.score_directory(gt_dir, gt_dir, 2.0, n_classes=3, log=lambda *a: None)
    assert [r['class'] for r in rows] == [0, 1, 2] and all(r['hd'] == 0.0 and r['nsd'] == 1.0 for r in rows)
    a = surface.build_parser().parse_args(['p', 'g', '--gpu', '--classes', '4'])
    assert a.gpu and a.classes == 4 and a.tolerance == 2.0 and a.csv is None


@pytest.fixture(scope='module')
def lib():
    from wesup_amd import _lib
    if not os.path.exists(_lib.LIB_PATH):
        _lib.build()
    return _lib


NEW_ENTRIES = ('wesup_edt_full_workspace_bytes', 'wesup_edt_full', 'wesup_mask_border', 'wesup_surface_stats_workspace_bytes',
               'wesup_surface_stats', 'wesup_select_i32_workspace_bytes', 'wesup_select_i32')


def test_header_library_and_binding_agree(lib):
    hdr = open(os.path.join(ROOT, 'include', 'wesup_hip.h')).read()
    nm = subprocess.run(['nm', '-D', '--defined-only', lib.LIB_PATH], check=True, capture_output=True, text=True).stdout
    exported = set(re.findall(r' T (wesup_\w+)', nm))
    handle = lib.load()
    for name in NEW_ENTRIES:
        assert re.search(r'\b%s\s*\(' % name, hdr), name
        assert name in exported and name in lib._SIGS and hasattr(handle, name), name
    assert handle.wesup_abi_version() == lib.ABI_VERSION == 6
    for name, v in (('NONE', 2147483647), ('CHUNK', 64), ('COLS', 256), ('SEG', 64), ('ROWS', 4)):
        assert f'#define WESUP_EDT_{name} {v}' in hdr
    assert (lib.EDT_NONE, lib.EDT_CHUNK, lib.EDT_COLS, lib.EDT_SEG, lib.EDT_ROWS) == (2 ** 31 - 1, 64, 256, 64, 4)
    assert '#define WESUP_SURFACE_STATS 10' in hdr and lib.SURFACE_STATS == 10 == len(surface.STAT_KEYS)
    assert surface.EDT_NONE == lib.EDT_NONE


def test_entries_refuse_bad_arguments_on_the_host(lib):
    import ctypes
    import struct
    h = lib.load()
    assert h.wesup_edt_full_workspace_bytes(1, 1, 46341) > 0
    assert h.wesup_edt_full_workspace_bytes(1, 1, 46342) == 0
    assert h.wesup_edt_full_workspace_bytes(0, 4, 4) == 0
    assert h.wesup_edt_full_workspace_bytes(2, 5, 7) >= 2 * 5 * 7 * 4
    assert h.wesup_surface_stats_workspace_bytes(2, 5, 7) >= 2 * 2 * 5 * 7 * 4
    assert h.wesup_select_i32_workspace_bytes(1000) > 0 and h.wesup_select_i32_workspace_bytes(0) == 0
    buf = ctypes.create_string_buffer(1 << 16)       # non-null addresses; no entry gets as far as using them
    base = (ctypes.cast(buf, ctypes.c_void_p).value + 255) // 256 * 256
    m, d, s, g, e, w = (base + 4096 * k for k in range(6))
    big = 1 << 15
    q = struct.unpack('<q', struct.pack('<d', 0.95))[0]
    for B, H, W in ((0, 5, 7), (1, 0, 7), (1, 5, -1), (65536, 5, 7), (1, 65536, 7), (1, 40000, 40000), (1, 1, 46342),
                    (1, 32769, 32769)):
        assert h.wesup_edt_full_workspace_bytes(B, H, W) == 0 and h.wesup_surface_stats_workspace_bytes(B, H, W) == 0
        assert h.wesup_edt_full(m, d, B, H, W, 0, w, big, None) == -1
        if (B, H, W) != (1, 1, 46342):                  # (a legal shape for the border: only the distances overflow there)
            assert h.wesup_mask_border(m, d, B, H, W, None) == -1
        assert h.wesup_surface_stats(m, s, d, g, e, B, H, W, 4, q, w, big, None) == -1
    # null pointers, before any launch
    assert h.wesup_edt_full(None, d, 1, 5, 7, 0, w, big, None) == -1
    assert h.wesup_edt_full(m, None, 1, 5, 7, 0, w, big, None) == -1
    assert h.wesup_edt_full(m, d, 1, 5, 7, 0, None, big, None) == -1
    assert h.wesup_mask_border(None, d, 1, 5, 7, None) == -1 and h.wesup_mask_border(m, None, 1, 5, 7, None) == -1
    args = [m, s, d, g, e]
    for k in range(5):
        a = list(args)
        a[k] = None
        assert h.wesup_surface_stats(*a, 1, 5, 7, 4, q, w, big, None) == -1
    assert h.wesup_surface_stats(*args, 1, 5, 7, 4, q, None, big, None) == -1
    assert h.wesup_select_i32(None, 10, s, 2, d, w, big, None) == -1
    assert h.wesup_select_i32(m, 10, None, 2, d, w, big, None) == -1
    assert h.wesup_select_i32(m, 10, s, 2, None, w, big, None) == -1
    assert h.wesup_select_i32(m, 10, s, 2, d, None, big, None) == -1
    # ranges, short workspaces, overlapping operands
    assert h.wesup_edt_full(m, d, 1, 5, 7, 2, w, big, None) == -1                   # invert is 0 or 1
    assert h.wesup_edt_full(m, d, 1, 5, 7, 0, w, 16, None) == -1
    assert h.wesup_edt_full(m, m, 1, 5, 7, 0, w, big, None) == -1 and h.wesup_edt_full(m, w, 1, 5, 7, 0, w, big, None) == -1
    assert h.wesup_mask_border(m, m + 34, 1, 5, 7, None) == -1
    assert h.wesup_surface_stats(*args, 1, 5, 7, -1, q, w, big, None) == -1          # a negative squared tolerance
    assert h.wesup_surface_stats(*args, 1, 5, 7, 4, struct.unpack('<q', struct.pack('<d', 1.5))[0], w, big, None) == -1
    assert h.wesup_surface_stats(*args, 1, 5, 7, 4, q, w, 16, None) == -1
    assert h.wesup_surface_stats(m, s, d, g, w, 1, 5, 7, 4, q, w, big, None) == -1
    assert h.wesup_select_i32(m, 0, s, 2, d, w, big, None) == -1 and h.wesup_select_i32(m, 10, s, 5, d, w, big, None) == -1


def test_wrappers_fail_loudly_without_gpu_tensors(lib):
    import torch
    from wesup_amd import ops
    for call in (lambda: ops.edt_sq_full(torch.zeros(4, 4, dtype=torch.uint8)),
                 lambda: ops.mask_border(torch.zeros(4, 4, dtype=torch.uint8)),
                 lambda: ops.select_i32(torch.zeros(4, dtype=torch.int32), torch.zeros(1, dtype=torch.int64)),
                 lambda: ops.surface_stats(torch.zeros(4, 4, dtype=torch.uint8), torch.zeros(4, 4, dtype=torch.uint8), 2.0)):
        with pytest.raises(lib.WesupHipError):
            call()
