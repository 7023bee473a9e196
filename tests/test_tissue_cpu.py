"""Tissue selection for whole-slide evaluation, the parts that need no GPU: the host definitions of
wesup_amd/slide.py, the walk over a patch list with the device calls replaced, and the new entries' host-side refusals.

Otsu.  ``slide.otsu_threshold`` is a statement in six fp64 operations per threshold, made so that a device can repeat it bit for
bit.  It is compared with the exact argmax of the same score in rational arithmetic on 300 seeded histograms (RandomState(0);
five kinds in turn: uniform noise, two Gaussians, counts up to 2^36 per bin, two levels, one level).  Where the two differ on
another input, the fp64 statement is the definition: the test of record is then the device against that statement
(tests/test_tissue_gpu.py), not this one."""
import os
import re
from fractions import Fraction

import numpy as np
import pytest
import torch

from wesup_amd import slide as S

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_ENTRIES = ('wesup_patch_value_hist', 'wesup_tissue_select', 'wesup_tissue_mask_u8', 'wesup_patch_gather_resize_list',
               'wesup_patch_scatter_u8_list', 'wesup_patch_scatter_classes_u8_list')


# ------------------------------------------------------------------------------------------------------------ 1. Otsu
def _otsu_exact(h):
    """The first t with the largest (S w0 - s0 N)^2 / D over t = 0 .. 254 with D > 0, in exact rationals; -1 when there is none."""
    h = [int(v) for v in h]
    N, S_ = sum(h), sum(i * v for i, v in enumerate(h))
    best, bq, w0, s0 = -1, None, 0, 0
    for t in range(255):
        w0 += h[t]
        s0 += t * h[t]
        D = w0 * (N - w0)
        if D == 0:
            continue
        q = Fraction((S_ * w0 - s0 * N) ** 2, D)
        if best < 0 or q > bq:
            best, bq = t, q
    return best


def _seeded_histograms():
    rs = np.random.RandomState(0)
    for trial in range(300):
        kind = trial % 5
        if kind == 0:
            h = rs.randint(0, 1000, 256)
        elif kind == 1:
            x = np.arange(256)
            h = (1e6 * np.exp(-((x - rs.randint(40, 120)) / rs.uniform(5, 25)) ** 2)
                 + 3e6 * np.exp(-((x - rs.randint(180, 250)) / rs.uniform(3, 15)) ** 2)).astype(np.int64)
        elif kind == 2:
            h = rs.randint(0, 2 ** 28, 256).astype(np.int64) * rs.randint(1, 2 ** 8)
        elif kind == 3:
            h = np.zeros(256, np.int64)
            a, b = sorted(rs.choice(256, 2, replace=False))
            h[a], h[b] = rs.randint(1, 10 ** 6), rs.randint(1, 10 ** 6)
        else:
            h = np.zeros(256, np.int64)
            h[rs.randint(0, 256)] = rs.randint(1, 10 ** 9)
        yield kind, h


def test_otsu_fp64_statement_equals_the_exact_argmax_on_300_seeded_histograms():
    differ, kinds = [], set()
    for trial, (kind, h) in enumerate(_seeded_histograms()):
        got = S.otsu_threshold(h)
        kinds.add(kind)
        if got != _otsu_exact(h):
            differ.append((trial, kind, got, _otsu_exact(h)))
        if kind == 3:
            assert got == int(np.nonzero(h)[0][0]), (trial, got)             # two levels: the lower one (the tie rule)
        if kind == 4:
            assert got == -1, (trial, got)                                   # one level: no threshold
    assert kinds == {0, 1, 2, 3, 4}
    assert differ == [], differ


def test_otsu_two_levels_one_level_and_the_needs_of_128_bits():
    h = np.zeros(256, np.int64)
    h[40], h[200] = 7, 9
    assert S.otsu_threshold(h) == 40
    h[200] = 0
    assert S.otsu_threshold(h) == -1
    h[:] = 0
    h[255] = 5
    assert S.otsu_threshold(h) == -1                                         # t stops at 254: w0 = 0 throughout
    h[254] = 5
    assert S.otsu_threshold(h) == 254
    big = np.zeros(256, np.int64)                                            # N = 2^32: S w0 is beyond 64 bits
    big[10], big[250] = 1 << 31, 1 << 31
    assert 250 * (1 << 31) * (1 << 31) > 1 << 64 and S.otsu_threshold(big) == 10
    assert S.otsu_threshold(np.zeros(256, np.int64)) == -1                   # an empty histogram: D = 0 everywhere
    with pytest.raises(ValueError):
        S.otsu_threshold(np.zeros(255, np.int64))


# ------------------------------------------------------------------------------------------ 2. values, histograms, rule
def test_pixel_value_is_the_stated_integer_formula():
    rs = np.random.RandomState(1)
    img = rs.randint(0, 256, (9, 11, 3)).astype(np.uint8)
    img[0, 0], img[0, 1], img[0, 2] = (255, 255, 255), (0, 0, 0), (255, 0, 128)
    luma, chroma = S.pixel_value(img, 'luma'), S.pixel_value(img, 'chroma')
    for y in range(9):
        for x in range(11):
            r, g, b = (int(v) for v in img[y, x])
            assert luma[y, x] == (77 * r + 150 * g + 29 * b + 128) >> 8 and chroma[y, x] == max(r, g, b) - min(r, g, b)
    assert luma[0, 0] == 255 and luma[0, 1] == 0 and chroma[0, 2] == 255 and luma.dtype == chroma.dtype == np.uint8
    with pytest.raises(ValueError):
        S.pixel_value(img, 'hue')


def test_histograms_count_the_slide_never_the_padding():
    rs = np.random.RandomState(2)
    img = rs.randint(0, 256, (37, 53, 3)).astype(np.uint8)
    hist = S.patch_histograms(img, 16)
    areas = S.patch_areas(37, 53, 16)
    assert hist.shape == (12, 256) and list(areas) == [256] * 3 + [80] + [256] * 3 + [80] + [80] * 3 + [25]
    assert np.array_equal(hist.sum(axis=1), areas) and hist.sum() == 37 * 53
    assert np.array_equal(hist[11], np.bincount(S.pixel_value(img)[32:, 48:].ravel(), minlength=256))
    one = S.patch_histograms(img[:20], 128)                                  # p > H and p > W: one padded patch
    assert one.shape == (1, 256) and one.sum() == 20 * 53


def test_a_given_threshold_passes_through_unchanged():
    rs = np.random.RandomState(3)
    img = rs.randint(0, 256, (40, 40, 3)).astype(np.uint8)
    for t in (0, 100, 254):
        for channel in S.TISSUE_CHANNELS:
            r = S.tissue_patches(img, 16, channel=channel, threshold=t)
            v = S.pixel_value(img, channel)
            assert r.t == t and not r.flat
            want = (v <= t) if channel == 'luma' else (v > t)
            assert int(np.asarray(r.counts).sum()) == int(want.sum())
            assert np.array_equal(S.tissue_mask_array(img, t, channel), want * np.uint8(255))
    assert S.tissue_patches(img, 16, threshold='otsu').t == S.otsu_threshold(S.patch_histograms(img, 16).sum(axis=0))
    for bad in (-1, 255, 'median'):
        with pytest.raises(ValueError):
            S.tissue_patches(img, 16, threshold=bad)


def test_select_patches_rule_on_hand_made_counts():
    # the ppm rule at exact equality keeps the patch: 123 * 10^6 == 1230 * 100000
    assert S.select_patches([123, 122], [100000, 100000], 1230) == [0]
    assert S.select_patches([1, 0], [100, 100], 10000) == [0]               # 1 * 10^6 == 10000 * 100
    # count = 0 is never kept, even at min_ppm = 0
    assert S.select_patches([0, 1, 0], [256, 256, 256], 0) == [1]
    # border patches use their in-slide area: 37 x 53 with p 16; the corner patch has 25 pixels, the full ones 256
    areas = S.patch_areas(37, 53, 16)
    counts = [3] * 12                                                        # 3 / 25 = 12 %, 3 / 80 = 3.75 %, 3 / 256 = 1.17 %
    assert S.select_patches(counts, areas, 100000) == [11]
    assert S.select_patches(counts, areas, 37500) == [3, 7, 8, 9, 10, 11]   # 3 * 10^6 == 37500 * 80
    assert S.select_patches(counts, areas, 37501) == [11]
    assert S.select_patches(counts, areas, 11718) == list(range(12)) and S.select_patches(counts, areas, 11719) == [3, 7, 8, 9, 10, 11]
    # a flat slide keeps all, at any bar
    assert S.select_patches([0] * 12, areas, 1000000, flat=True) == list(range(12))
    flat = np.full((37, 53, 3), 200, np.uint8)
    r = S.tissue_patches(flat, 16, min_fraction=1.0)
    assert r.t == -1 and r.flat and r.list == list(range(12)) and np.array_equal(r.counts, areas)
    assert S.min_ppm_of(0.01) == 10000 and S.min_ppm_of(0) == 0 and S.min_ppm_of(1) == 1000000
    for bad in (-0.1, 1.0000006):
        with pytest.raises(ValueError):
            S.min_ppm_of(bad)
    with pytest.raises(ValueError):
        S.select_patches([1], [1, 2], 0)


def test_host_selection_of_a_slide_with_glass():
    rs = np.random.RandomState(4)
    img = np.full((48, 64, 3), 240, np.uint8)
    img[:16, 16:32] = rs.randint(0, 120, (16, 16, 3))                        # patch 1: all tissue
    img[40:42, 50:52] = 10                                                   # patch 11: 4 of 256 pixels
    r = S.tissue_patches(img, 16, min_fraction=0.01)
    assert r.n == 12 and 0 <= r.t < 240 and r.list == [1, 11] and r.n_keep == 2 and r.counts[1] == 256 and r.counts[11] == 4
    assert S.tissue_patches(img, 16, min_fraction=0.02).list == [1]
    chroma = img.copy()
    chroma[:16, 16:32] = (200, 40, 180)
    assert S.tissue_patches(chroma, 16, channel='chroma').list == [1]


# ---------------------------------------------------------------------------------------- 3. the walk over a patch list
class _Calls:
    def __init__(self):
        self.gathers, self.pastes, self.forwards = [], [], 0


def _walk(monkeypatch, n_keep, batch, H=48, W=64, p=16):
    """``_patch_walk`` on CPU tensors: the gather fills slot i with the index of the patch it names, ``forward`` passes that on,
    the paste records what it was given."""
    from wesup_amd import ops
    calls = _Calls()
    n = -(-H // p) * -(-W // p)
    kept = list(range(1, n, 2))[:n_keep]
    sel = S.TissuePatches(100, len(kept), n, torch.tensor(kept, dtype=torch.int32), None, False, 'luma')

    def gather(img, p_, h, w, first, count, align_corners=False, out=None, patch_list=None):
        assert patch_list is sel.list and out.shape == (count, 3, h, w)
        slots = [int(patch_list[min(first + i, len(patch_list) - 1)]) for i in range(count)]
        calls.gathers.append((first, count, slots))
        for i, k in enumerate(slots):
            out[i] = k
        return out

    def forward(x):
        calls.forwards += 1
        return x[:, 0].clone()

    def paste(pred, out, first, patch_list=None):
        assert patch_list is sel.list
        calls.pastes.append((first, [int(v) for v in pred[:, 0, 0]]))

    monkeypatch.setattr(ops, 'patch_gather_resize', gather)
    out = S._patch_walk(torch.zeros(H, W, 3, dtype=torch.uint8), p, (4, 4), batch, False, False, forward, paste, sel)
    return calls, kept, out


def test_walk_with_nothing_kept_never_calls_forward(monkeypatch):
    calls, kept, out = _walk(monkeypatch, 0, 4)
    assert kept == [] and calls.forwards == 0 and calls.gathers == [] and calls.pastes == []
    assert out.shape == (48, 64) and out.dtype == np.uint8 and not out.any()


def test_walk_passes_of_a_ragged_list(monkeypatch):
    calls, kept, out = _walk(monkeypatch, 5, 2)
    assert kept == [1, 3, 5, 7, 9]
    # window_batches(5, 2): passes (0, 2), (2, 2), (4, 1); every gather asks for `batch` slots, the last repeats the last patch
    assert calls.gathers == [(0, 2, [1, 3]), (2, 2, [5, 7]), (4, 2, [9, 9])]
    assert calls.pastes == [(0, [1, 3]), (2, [5, 7]), (4, [9])] and calls.forwards == 3
    assert not out.any()                                                     # the stub pastes nothing: the map starts as zeros
    calls, kept, _ = _walk(monkeypatch, 3, 8)                                # a batch larger than the list: one pass of 3
    assert calls.gathers == [(0, 3, [1, 3, 5])] and calls.pastes == [(0, [1, 3, 5])]


def test_walk_refuses_a_selection_of_another_lattice(monkeypatch):
    sel = S.TissuePatches(1, 1, 5, torch.zeros(1, dtype=torch.int32), None, False, 'luma')
    with pytest.raises(ValueError):
        S._patch_walk(torch.zeros(48, 64, 3, dtype=torch.uint8), 16, (4, 4), 2, False, False, None, None, sel)
    with pytest.raises(ValueError):
        S._selection(torch.zeros(48, 64, 3, dtype=torch.uint8), 16, {'fraction': 0.1})
    assert S._selection(None, 16, None) is None and S._selection(None, 16, False) is None


def test_cli_arguments():
    a = S.parse_args(['root', '-c', 'ckpt'])
    assert a.skip_background is None and a.tissue_masks is None and a.tissue_channel == 'luma' and a.tissue_threshold == 'otsu'
    a = S.parse_args(['root', '-c', 'ckpt', '--skip-background'])
    assert a.skip_background == S.SKIP_MIN_FRACTION == 0.01
    a = S.parse_args(['root', '-c', 'ckpt', '--skip-background', '0.2', '--tissue-channel', 'chroma', '--tissue-threshold', '30',
                      '--tissue-masks', 'm'])
    assert (a.skip_background, a.tissue_channel, a.tissue_threshold, a.tissue_masks) == (0.2, 'chroma', '30', 'm')
    with pytest.raises(ValueError):
        S.main('root', 'ckpt', skip_infer=True, tissue_masks='m')            # masks without --skip-background


# --------------------------------------------------------------------------------------------------- 4. the boundary
def test_new_entries_are_declared_exported_and_bound():
    from wesup_amd import _lib
    hdr = open(os.path.join(ROOT, 'include', 'wesup_hip.h')).read()
    h = _lib.load()
    for name in NEW_ENTRIES:
        assert re.search(r'\bint\s+' + name + r'\s*\(', hdr), name
        assert name in _lib._SIGS and hasattr(h, name), name
    assert h.wesup_abi_version() == _lib.ABI_VERSION == 6
    for macro, value in (('WESUP_TISSUE_MAX_BLOCKS', _lib.TISSUE_MAX_BLOCKS), ('WESUP_TISSUE_ITEM_PIXELS', _lib.TISSUE_ITEM_PIXELS),
                         ('WESUP_TISSUE_LIST_CHUNK', _lib.TISSUE_LIST_CHUNK)):
        assert int(re.search(r'#define\s+' + macro + r'\s+(\d+)', hdr).group(1)) == value


def test_new_entries_refuse_bad_arguments_without_a_launch():
    """Every refusal is made on the host in front of the first launch (no GPU here); 1 stands for a non-null pointer that is
    never followed."""
    from wesup_amd import _lib
    h = _lib.load()
    P = 8                                                                    # (8-byte aligned, for total)
    INVALID = -1
    assert h.wesup_patch_value_hist(None, P, 10, 10, 4, 0, None) == INVALID
    assert h.wesup_patch_value_hist(P, None, 10, 10, 4, 0, None) == INVALID
    for H, W, p, ch in ((0, 10, 4, 0), (10, 0, 4, 0), (10, 10, 0, 0), (10, 10, 65536, 0), (10, 10, 4, 2), (10, 10, 4, -1),
                        ((1 << 30) + 1, 10, 4, 0), (1 << 17, 1 << 16, 4, 0)):  # the last: H * W > 2^32
        assert h.wesup_patch_value_hist(P, P, H, W, p, ch, None) == INVALID, (H, W, p, ch)
    ok = dict(H=10, W=10, p=4, channel=0, threshold=-1, min_ppm=10000)

    def select(ptrs=(P, P, P, P, P), **kw):
        a = dict(ok, **kw)
        return h.wesup_tissue_select(ptrs[0], a['H'], a['W'], a['p'], a['channel'], a['threshold'], a['min_ppm'], ptrs[1], ptrs[2],
                                     ptrs[3], ptrs[4], None)
    for i in range(5):
        assert select(tuple(None if j == i else P for j in range(5))) == INVALID, i
    for kw in (dict(threshold=-2), dict(threshold=255), dict(min_ppm=-1), dict(min_ppm=1000001), dict(channel=2), dict(p=65536),
               dict(p=0), dict(H=0), dict(H=1 << 17, W=1 << 16)):
        assert select(**kw) == INVALID, kw
    for args in ((None, P, P, 10, 10, 0), (P, None, P, 10, 10, 0), (P, P, None, 10, 10, 0), (P, P, P, 0, 10, 0), (P, P, P, 10, 10, 2)):
        assert h.wesup_tissue_mask_u8(*args, None) == INVALID, args
    # the list entries: a null list or an empty one, and everything the plain entries refuse
    assert h.wesup_patch_gather_resize_list(P, P, 10, 10, 4, 8, 8, 0, 0, 1, None, 3, None) == INVALID
    assert h.wesup_patch_gather_resize_list(P, P, 10, 10, 4, 8, 8, 0, 0, 1, P, 0, None) == INVALID
    assert h.wesup_patch_gather_resize_list(P, P, 10, 10, 4, 8, 8, 0, 0, 0, P, 3, None) == INVALID          # count < 1
    assert h.wesup_patch_gather_resize_list(None, P, 10, 10, 4, 8, 8, 0, 0, 1, P, 3, None) == INVALID
    assert h.wesup_patch_scatter_u8_list(P, P, 10, 10, 4, 8, 8, 1, 0, 0, 1, None, 3, None) == INVALID
    assert h.wesup_patch_scatter_u8_list(P, P, 10, 10, 4, 8, 8, 1, 0, 0, 1, P, 0, None) == INVALID
    assert h.wesup_patch_scatter_u8_list(P, P, 10, 10, 4, 8, 8, 1, 2, 0, 1, P, 3, None) == INVALID          # mode
    assert h.wesup_patch_scatter_classes_u8_list(P, P, P, 10, 10, 4, 8, 8, 3, 0, 0, 1, None, 3, None) == INVALID
    assert h.wesup_patch_scatter_classes_u8_list(P, P, P, 10, 10, 4, 8, 8, 3, 0, 0, 1, P, -1, None) == INVALID
    assert h.wesup_patch_scatter_classes_u8_list(P, P, P, 10, 10, 4, 8, 8, 1, 0, 0, 1, P, 3, None) == INVALID  # C


def test_ops_refuse_host_tensors_and_bad_arguments():
    from wesup_amd import _lib, ops
    img = torch.zeros(8, 8, 3, dtype=torch.uint8)
    with pytest.raises(_lib.WesupHipError):
        ops.patch_value_hist(img, 4)                                         # a CPU tensor: no fallback
    with pytest.raises(_lib.WesupHipError):
        ops.patch_value_hist(img, 4, channel='hue')
    with pytest.raises(_lib.WesupHipError):
        ops.tissue_select(torch.zeros(4, 256, dtype=torch.int32), 8, 8, 4)
    with pytest.raises(_lib.WesupHipError):
        ops.tissue_mask(img, torch.zeros(8, dtype=torch.int32))
