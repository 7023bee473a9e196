"""Host side of the device-resident window inference (csrc/tiles.hip, ops.window_gather / window_merge, infer_tile's batched
functions): the entries exist and are bound, every rejected argument class comes back as WESUP_ERR_INVALID before any launch,
the wrappers refuse CPU tensors and wrong lattices, the ragged-batch arithmetic, and the command line.  No GPU here."""
import ctypes
import os
import re
from unittest import mock

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRIES = ('wesup_window_gather', 'wesup_window_merge')
INVALID = -1


@pytest.fixture(scope='module')
def lib():
    from wesup_amd import _lib
    if not os.path.exists(_lib.LIB_PATH):
        _lib.build()
    return _lib


def test_entries_are_declared_exported_and_bound(lib):
    hdr = open(os.path.join(ROOT, 'include', 'wesup_hip.h')).read()
    handle = lib.load()
    for name in ENTRIES:
        assert re.search(r'\bint\s+%s\s*\(' % name, hdr), name
        assert name in lib.EXPORTS and name in lib._SIGS
        assert hasattr(handle, name)
        assert getattr(handle, name).restype is ctypes.c_int
        assert len(getattr(handle, name).argtypes) == 12
    assert lib._SIGS['wesup_window_gather'][1] == 'ppppiiiiiiip' and lib._SIGS['wesup_window_merge'][1] == 'ppppiiiiiiip'
    assert 'tiles.hip' in open(os.path.join(lib.CSRC, 'Makefile')).read()
    assert handle.wesup_abi_version() == lib.ABI_VERSION == 6          # additions do not bump the ABI


def test_gather_rejects_bad_arguments_on_the_host(lib):
    """(img, tops, lefts, out, H, W, n_h, n_w, p, first, count, stream): never a launch -- the pointers are not memory."""
    h = lib.load()
    q = ctypes.c_void_p(4096)
    good = dict(img=q, tops=q, lefts=q, out=q, H=80, W=112, n_h=2, n_w=2, p=64, first=0, count=4)

    def call(**kw):
        a = {**good, **kw}
        return h.wesup_window_gather(a['img'], a['tops'], a['lefts'], a['out'], a['H'], a['W'], a['n_h'], a['n_w'], a['p'],
                                     a['first'], a['count'], None)
    for ptr in ('img', 'tops', 'lefts', 'out'):
        assert call(**{ptr: None}) == INVALID, ptr
    assert call(p=0) == INVALID and call(p=-3) == INVALID
    assert call(p=81) == INVALID                                       # p > H
    assert call(p=113, H=200) == INVALID                               # p > W
    assert call(count=0) == INVALID and call(count=-1) == INVALID
    assert call(n_h=0) == INVALID and call(n_w=0) == INVALID
    assert call(first=-1) == INVALID


def test_merge_rejects_bad_arguments_on_the_host(lib):
    """(pred, tops, lefts, out, H, W, C, n_h, n_w, p, round_first, stream)"""
    h = lib.load()
    q = ctypes.c_void_p(4096)
    good = dict(pred=q, tops=q, lefts=q, out=q, H=80, W=112, C=1, n_h=2, n_w=2, p=64)

    def call(**kw):
        a = {**good, **kw}
        return h.wesup_window_merge(a['pred'], a['tops'], a['lefts'], a['out'], a['H'], a['W'], a['C'], a['n_h'], a['n_w'], a['p'],
                                    1, None)
    for ptr in ('pred', 'tops', 'lefts', 'out'):
        assert call(**{ptr: None}) == INVALID, ptr
    assert call(p=0) == INVALID
    assert call(p=81) == INVALID and call(p=113, H=200) == INVALID
    assert call(C=0) == INVALID
    assert call(n_h=0) == INVALID and call(n_w=0) == INVALID


def test_wrappers_refuse_cpu_tensors(lib):
    from wesup_amd import infer_tile as T
    from wesup_amd import ops
    tops, lefts = T.window_grid(80, 112, 64)
    with pytest.raises(lib.WesupHipError, match='no CPU fallback'):
        ops.window_gather(torch.zeros(80, 112, 3, dtype=torch.uint8), tops, lefts, 64, 0, 4)
    with pytest.raises(lib.WesupHipError, match='no CPU fallback'):
        ops.window_merge(torch.zeros(4, 64, 64, 1), tops, lefts, 80, 112)
    with pytest.raises(lib.WesupHipError):
        ops.window_gather(torch.zeros(80, 112, dtype=torch.uint8), tops, lefts, 64, 0, 4)          # not (H,W,3)
    with pytest.raises(lib.WesupHipError):
        ops.window_gather(torch.zeros(80, 112, 3, dtype=torch.uint8), tops, lefts, 64, 0, 0)       # count < 1


@pytest.mark.parametrize('tops,lefts,what', [
    ([16, 0], [0, 48], 'not sorted'),
    ([0, 16], [0, 24, 12, 48], 'not sorted'),
    ([0, 15], [0, 48], 'size - p'),                  # does not end at H - p
    ([0, 16], [0, 47], 'size - p'),                  # does not end at W - p
    ([1, 16], [0, 48], 'size - p'),                  # does not start at 0
    ([], [0, 48], 'empty'),
    ([0, 16], [0, 112 - 64 - 70, 48], 'not sorted'),
])
def test_wrappers_refuse_a_wrong_lattice(lib, tops, lefts, what):
    """The kernels read the lattice from device memory: its contents are checked in Python, before the tensors are looked at
    (these are CPU tensors -- the message tells which check fired)."""
    from wesup_amd import ops
    with pytest.raises(lib.WesupHipError, match=what):
        ops.window_gather(torch.zeros(80, 112, 3, dtype=torch.uint8), tops, lefts, 64, 0, 4)
    with pytest.raises(lib.WesupHipError, match=what):
        ops.window_merge(torch.zeros(len(tops) * len(lefts), 64, 64, 1), tops, lefts, 80, 112)


def test_wrappers_refuse_a_lattice_with_a_gap_or_a_patch_larger_than_the_image(lib):
    from wesup_amd import ops
    with pytest.raises(lib.WesupHipError, match='uncovered'):
        ops.window_merge(torch.zeros(4, 16, 16, 1), [0, 64], [0, 96], 80, 112)
    with pytest.raises(lib.WesupHipError, match='patch size'):
        ops.window_gather(torch.zeros(80, 112, 3, dtype=torch.uint8), [0], [0], 81, 0, 1)
    with pytest.raises(lib.WesupHipError, match='windows for a lattice'):
        ops.window_merge(torch.zeros(3, 64, 64, 1), [0, 16], [0, 48], 80, 112)


def test_the_lattice_of_window_grid_passes_the_check():
    from wesup_amd import infer_tile as T
    from wesup_amd import ops
    for H, W, p in ((64, 64, 64), (80, 112, 64), (128, 192, 64), (150, 333, 64), (522, 775, 464), (3000, 3000, 464)):
        tops, lefts = T.window_grid(H, W, p)
        t, l = ops._lattice(tops, lefts, H, W, p, 'cpu')
        assert t.dtype == torch.int32 and t.tolist() == [int(v) for v in tops] and l.tolist() == [int(v) for v in lefts]


def test_ragged_batch_arithmetic():
    from wesup_amd import infer_tile as T
    passes, batch = T.window_batches(18, 4)
    assert batch == 4 and passes == [(0, 4), (4, 4), (8, 4), (12, 4), (16, 2)]
    # what the gather reads for every pass: `batch` indices from `first`, those past the lattice clamped to the last window
    read = [[min(first + i, 17) for i in range(batch)] for first, _ in passes]
    assert read[-1] == [16, 17, 17, 17]
    kept = [k for (first, valid), row in zip(passes, read) for k in row[:valid]]
    assert kept == list(range(18))                                     # every window once, in order
    assert T.window_batches(18, 3) == ([(f, 3) for f in range(0, 18, 3)], 3)
    assert T.window_batches(4, 8) == ([(0, 4)], 4)                     # never more than the image has
    assert T.window_batches(1, 1) == ([(0, 1)], 1)
    assert T.window_batches(49, 8)[0][-1] == (48, 1)
    for bad in ((0, 4), (4, 0), (4, -1)):
        with pytest.raises(ValueError):
            T.window_batches(*bad)


def test_command_line_parses_batch_and_pixel():
    from wesup_amd import infer_tile as T
    with mock.patch.object(T, '_load_pixel_model', return_value='model') as load, \
            mock.patch.object(T, 'pixel_infer') as run, mock.patch.object(T, 'initialize_trainer') as init:
        T.main(['d', '--batch', '4', '--pixel'])
    load.assert_called_once_with(None, 'cuda')
    assert not init.called
    (model, data_dir, patch, out), kw = run.call_args
    assert (model, data_dir, patch, out) == ('model', 'd', 464, None) and kw == {'device': 'cuda', 'batch': 4}
    # without the flags: the per-window path, as before
    with mock.patch.object(T, 'initialize_trainer') as init, mock.patch.object(T, 'infer') as run:
        T.main(['d', '--patch-size', '300'])
    assert run.call_args[0][1:] == ('d', 300, None) and run.call_args[1] == {'device': 'cuda', 'batch': None}
    with mock.patch.object(T, 'initialize_trainer') as init, mock.patch.object(T, 'infer') as run:
        T.main(['d', '--batch', '8'])
    assert run.call_args[1]['batch'] == 8


def test_predict_takes_the_per_window_path_by_default(tmp_path):
    from PIL import Image
    from wesup_amd import infer_tile as T
    Image.fromarray(np.zeros((8, 8, 3), dtype=np.uint8)).save(tmp_path / 'a.png')
    with mock.patch.object(T, 'predict_array', return_value='old') as old, \
            mock.patch.object(T, 'predict_array_batched', return_value='new') as new:
        assert T.predict('trainer', tmp_path / 'a.png', 8) == 'old' and not new.called
        assert T.predict('trainer', tmp_path / 'a.png', 8, batch=2) == 'new'
    assert new.call_args[1] == {'batch': 2, 'device': 'cuda'} and old.call_count == 1


class _Stub:
    """A model for the per-window forms: a deterministic function of the window tensor, and the class count the forms read."""
    def __init__(self, fn, n_classes):
        self.fn, self.n_classes = fn, n_classes

    def __call__(self, x):
        return self.fn(x)


@pytest.mark.parametrize('C', [2, 3])
def test_per_window_forms_equal_the_composition_written_out(C):
    """The four per-window forms on the CPU with stub models: each is divide_image_to_patches -> the stub -> its merge.  20 x 27 at
    patch 8 is a 3 x 4 lattice that overlaps on both axes; the stubs add a ramp over the window, so two windows disagree about a
    pixel they share and the order of the merge shows."""
    from types import SimpleNamespace
    from wesup_amd import infer_tile as T
    H, W, p = 20, 27, 8
    assert [len(axis) for axis in T.window_grid(H, W, p)] == [3, 4]
    img = np.random.RandomState(C).randint(0, 256, (H, W, 3)).astype(np.uint8)
    ramp = torch.linspace(0., 1., p * p).view(p, p)

    def probabilities(x):                                              # (1, 3, p, p) -> (p, p, C)
        return torch.softmax(torch.stack([x[0, c] * (c + 1) + ramp * (C - c) for c in range(C)], dim=-1), dim=-1)

    def painted(x):                                                    # what WESUP.forward paints: (1, p, p)
        return probabilities(x)[..., 1][None] if C == 2 else probabilities(x).argmax(dim=-1).float()[None]
    pixel = _Stub(probabilities, C)
    trainer = SimpleNamespace(preprocess=lambda x: (x * 0.5, None), model=_Stub(painted, C), postprocess=torch.round)
    windows = [T._to_tensor(patch, 'cpu') for patch in T.divide_image_to_patches(img, p)]
    assert len(windows) == 12
    with mock.patch.object(T, '_host_windows', wraps=T._host_windows) as walk:
        if C == 2:
            sp = T.predict_array(trainer, img, p, device='cpu')
            px = T.pixel_predict_array(pixel, img, p, device='cpu')
            want_sp = T.combine_patches_to_image(np.stack([torch.round(painted(x * 0.5))[0].numpy()[..., None] for x in windows]), H, W)
            want_px = T.combine_patches_to_image(np.stack([probabilities(x).numpy()[..., 1] for x in windows]), H, W)
        else:
            sp = T.predict_array_classes(trainer, img, p, device='cpu')
            px = T.pixel_predict_array_classes(pixel, img, p, device='cpu')
            want_sp = T.combine_patches_to_classes(np.stack([painted(x * 0.5)[0].numpy() for x in windows]), H, W, C, votes=True)
            want_px = T.combine_patches_to_classes(np.stack([probabilities(x).numpy() for x in windows]), H, W, C)
    assert walk.call_count == 2
    for got, want in ((sp, want_sp), (px, want_px)):
        assert got.shape == (H, W) and got.dtype == want.dtype and np.array_equal(got, want)
    assert len(np.unique(want_sp)) > 1 and len(np.unique(want_px)) > 1          # (not one value everywhere)
