"""Test-time augmentation over the eight views of a square window without a GPU: the host functions of
``infer_tile`` that are the specification of the device path -- ``apply_view`` / ``invert_view``, ``VIEW_SETS``,
``combine_views_to_image`` / ``combine_views_to_classes`` and the order of their sum -- the view lists they refuse, the command
line, and the bindings of the three entries, which refuse a wrong view word on the host."""
import ctypes
import itertools
import os
import re
from unittest import mock

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRIES = {'wesup_window_gather_views': 'pppp' + 'i' * 9 + 'p', 'wesup_window_merge_views': 'pppp' + 'i' * 9 + 'p',
           'wesup_window_merge_classes_views': 'ppppp' + 'i' * 9 + 'p'}
INVALID = -1
D4_WORD = 0x76543210


# ------------------------------------------------------------------------------------------------------------- the views
@pytest.mark.parametrize('tail', [(), (3,)])
@pytest.mark.parametrize('p', [1, 5, 8])
def test_invert_view_undoes_apply_view(p, tail):
    from wesup_amd import infer_tile as T
    a = np.random.RandomState(p).rand(p, p, *tail)
    for v in range(8):
        b = T.apply_view(a, v)
        assert b.shape == a.shape                                      # windows are square: a view keeps the shape
        assert np.array_equal(T.invert_view(b, v), a), v
        assert np.array_equal(T.apply_view(T.invert_view(a, v), v), a), v


def test_the_eight_views_are_pairwise_different():
    from wesup_amd import infer_tile as T
    a = np.arange(25).reshape(5, 5)
    views = [T.apply_view(a, v) for v in range(8)]
    for (i, x), (j, y) in itertools.combinations(enumerate(views), 2):
        assert not np.array_equal(x, y), (i, j)
    b = np.arange(25 * 2).reshape(5, 5, 2)                             # a trailing axis is carried along
    for v in range(8):
        assert np.array_equal(T.apply_view(b, v)[..., 1], T.apply_view(b[..., 1], v))


def test_view_sets_and_the_numbering():
    from wesup_amd import infer_tile as T
    assert T.VIEW_SETS == {'none': (0,), 'flips': (0, 2, 4, 6), 'rot': (0, 1, 2, 3), 'd4': (0, 1, 2, 3, 4, 5, 6, 7)}
    a = np.arange(36).reshape(6, 6)
    assert np.array_equal(T.apply_view(a, 0), a)
    assert np.array_equal(T.apply_view(a, 4), a[:, ::-1])              # the left-right mirror
    assert np.array_equal(T.apply_view(a, 6), a[::-1])                 # the up-down mirror
    assert np.array_equal(T.apply_view(a, 2), a[::-1, ::-1])           # the half turn
    assert np.array_equal(T.apply_view(a, 1), np.rot90(a))             # counter-clockwise
    assert np.array_equal(T.apply_view(a, 5), np.rot90(a[:, ::-1]))    # the mirror comes first


@pytest.mark.parametrize('bad', [(), tuple(range(8)) + (0,), (0, 0), (1, 3, 1), (8,), (-1,), (0, 8), (0.5,), None, 3])
def test_bad_view_lists_raise(bad):
    from wesup_amd import _lib, ops
    from wesup_amd import infer_tile as T
    with pytest.raises(ValueError):
        T.check_views(bad)
    if isinstance(bad, tuple):
        with pytest.raises(ValueError):
            T.combine_views_to_image(np.zeros((1, len(bad), 4, 4)), bad, 4, 4)
        with pytest.raises(ValueError):
            T.combine_views_to_classes(np.zeros((1, len(bad), 4, 4)), bad, 4, 4, 3, votes=True)
    if bad != (0.5,):                                                  # (the wrappers take what int() takes)
        with pytest.raises(_lib.WesupHipError, match='views'):
            ops._view_word(bad, 'test')
    for v in (8, -1):
        with pytest.raises(ValueError):
            T.apply_view(np.zeros((2, 2)), v)
        with pytest.raises(ValueError):
            T.invert_view(np.zeros((2, 2)), v)


def test_check_views_takes_any_order_and_the_view_word():
    from wesup_amd import infer_tile as T
    from wesup_amd import ops
    assert T.check_views([5, 2]) == (5, 2) and T.check_views(np.array([7, 0, 3])) == (7, 0, 3)
    assert ops._view_word((5, 2), 't') == (2, 0x25)
    assert ops._view_word(T.VIEW_SETS['d4'], 't') == (8, D4_WORD)
    assert ops._view_word(T.VIEW_SETS['flips'], 't') == (4, 0x6420)


# ------------------------------------------------------------------------------------------------------------- the merge
@pytest.mark.parametrize('H,W,p', [(8, 8, 8), (10, 14, 8), (13, 11, 5)])
def test_one_upright_view_is_the_merge_without_views(H, W, p):
    from wesup_amd import infer_tile as T
    N = len(T._get_top_left_coordinates(H, W, p))
    rs = np.random.RandomState(H + W)
    x = rs.rand(N, p, p).astype(np.float32)
    assert np.array_equal(T.combine_views_to_image(x[:, None], (0,), H, W), T.combine_patches_to_image(x, H, W))
    x3 = rs.rand(N, p, p, 3).astype(np.float32)
    assert np.array_equal(T.combine_views_to_image(x3[:, None], (0,), H, W), T.combine_patches_to_image(x3, H, W))
    assert np.array_equal(T.combine_views_to_classes(x3[:, None], (0,), H, W, 3), T.combine_patches_to_classes(x3, H, W, 3))
    votes = rs.randint(0, 3, (N, p, p)).astype(np.float32)
    votes[0, 0, 0] = 3.0                                               # an invalid vote counts for nothing in both
    assert np.array_equal(T.combine_views_to_classes(votes[:, None], (0,), H, W, 3, votes=True),
                          T.combine_patches_to_classes(votes, H, W, 3, votes=True))


def test_views_are_turned_back_before_they_are_added():
    """A window whose predictions are the views of one array merges to that array: eight times x over eight."""
    from wesup_amd import infer_tile as T
    x = np.random.RandomState(0).randint(0, 256, (5, 5)).astype(np.float64)
    views = (5, 2, 7, 0)
    stack = np.stack([T.apply_view(x, v) for v in views])[None]
    assert np.array_equal(T.combine_views_to_image(stack, views, 5, 5), x)
    wrong = T.combine_views_to_image(stack, (0, 1, 2, 3), 5, 5)        # the same numbers under another list: not x
    assert not np.array_equal(wrong, x)


TINY = np.float64(np.float32(1e-30))


def order_cases():
    """Planted predictions whose fp64 sum depends on the order -> [(pred, views, H, W, (y, x), the value in the definition's
    order, the value in another order)].  1e-30 is lost when it is added to 1.0 and kept when 1.0 and -1.0 have cancelled first.
    (a) 2 x 3 image, p = 2: windows at columns 0 and 1 both cover column 1; under view 4 offset (y, x) is read at (y, 1 - x).
    Pixel (0, 1) gets, in the definition's order, window 0 view 0, window 0 view 4, window 1 view 0, window 1 view 4:
    ((1.0 + 1e-30) + -1.0) + 0.0 = 0.0; with the views outside and the windows inside it would be (1.0 + -1.0) + 1e-30.
    (b) one 2 x 2 window under the list (0, 4, 2): pixel (0, 0) gets view 0's [0][0], view 4's [0][1] and view 2's [1][1] in
    LIST order, (1e-30 + 1.0) + -1.0 = 0.0; under the list (4, 2, 0) with the predictions reordered alike it is 1e-30 / 3."""
    a = np.zeros((2, 2, 2, 2), dtype=np.float32)                       # (N, V, p, p)
    a[0, 0, 0, 1], a[0, 1, 0, 0], a[1, 0, 0, 0], a[1, 1, 0, 1] = 1.0, 1e-30, -1.0, 0.0
    b = np.zeros((1, 3, 2, 2), dtype=np.float32)
    b[0, 0, 0, 0], b[0, 1, 0, 1], b[0, 2, 1, 1] = 1e-30, 1.0, -1.0
    return [(a, (0, 4), 2, 3, (0, 1), 0.0, TINY / 4.0), (b, (0, 4, 2), 2, 2, (0, 0), 0.0, TINY / 3.0),
            (np.ascontiguousarray(b[:, [1, 2, 0]]), (4, 2, 0), 2, 2, (0, 0), TINY / 3.0, 0.0)]


def test_the_order_of_the_sum_is_pinned():
    """Windows ascending, inside each the views in LIST order, onto 0.0, one division: the hand-computed values."""
    from wesup_amd import infer_tile as T
    assert [l for _, l in T._get_top_left_coordinates(2, 3, 2)] == [0, 1]
    assert ((0.0 + 1.0) + TINY) + -1.0 == 0.0 and ((0.0 + 1.0) + -1.0) + TINY == TINY and TINY > 0
    for pred, views, H, W, at, want, other in order_cases():
        got = T.combine_views_to_image(pred, views, H, W)
        assert got.shape == (H, W) and got[at] == want and got[at] != other, (views, got[at])
    a = order_cases()[0][0]
    assert T.combine_views_to_image(a, (0, 4), 2, 3)[0, 1] == ((((0.0 + 1.0) + TINY) + -1.0) + 0.0) / 4.0
    # the same numbers with the views outside and the windows inside would keep the small value
    assert (((0.0 + np.float64(a[0, 0, 0, 1])) + np.float64(a[1, 0, 0, 0])) + np.float64(a[0, 1, 0, 0])) / 4.0 == TINY / 4.0


def test_votes_over_views_and_ties():
    from wesup_amd import infer_tile as T
    # one 2 x 2 window, views (0, 4): pixel (0, 0) gets votes 2 and 1 -> the lower class; an invalid vote counts for nothing
    v = np.zeros((1, 2, 2, 2), dtype=np.float32)
    v[0, 0, 0, 0], v[0, 1, 0, 1] = 2.0, 1.0                            # pixel (0, 0): a tie of classes 1 and 2
    v[0, 0, 0, 1], v[0, 1, 0, 0] = np.nan, 2.0                         # pixel (0, 1): a NaN and a 2
    v[0, 0, 1, 0], v[0, 1, 1, 1] = 3.0, -1.0                           # pixel (1, 0): nobody votes
    v[0, 0, 1, 1], v[0, 1, 1, 0] = 1.0, 1.0
    got = T.combine_views_to_classes(v, (0, 4), 2, 2, 3, votes=True)
    assert got.dtype == np.uint8 and got.tolist() == [[1, 2], [0, 1]]
    with pytest.raises(ValueError):
        T.combine_views_to_classes(np.zeros((1, 2, 2, 2, 3)), (0, 4), 2, 2, 3, votes=True)
    with pytest.raises(ValueError):
        T.combine_views_to_classes(np.zeros((1, 2, 2, 2)), (0, 4), 2, 2, 3)
    with pytest.raises(ValueError):
        T.combine_views_to_image(np.zeros((1, 3, 2, 2)), (0, 4), 2, 2)            # three predictions for two views


# ----------------------------------------------------------------------------------------------- the walk and the command line
class _Stub:
    def __init__(self, fn, n_classes):
        self.fn, self.n_classes = fn, n_classes

    def __call__(self, x):
        return self.fn(x)


@pytest.mark.parametrize('C', [2, 3])
def test_per_window_forms_under_views_equal_the_composition_written_out(C):
    """The four per-window forms on the CPU with stub models whose output depends on where a pixel lies in the window: each is
    divide_image_to_patches -> apply_view -> the stub -> combine_views_*."""
    from types import SimpleNamespace
    from wesup_amd import infer_tile as T
    H, W, p, views = 13, 11, 5, (5, 0, 2)
    img = np.random.RandomState(C).randint(0, 256, (H, W, 3)).astype(np.uint8)
    ramp = torch.linspace(0., 1., p * p).view(p, p)

    def probabilities(x):                                              # (1, 3, p, p) -> (p, p, C)
        return torch.softmax(torch.stack([x[0, c] * (c + 1) + ramp * (C - c) for c in range(C)], dim=-1), dim=-1)

    def painted(x):
        return probabilities(x)[..., 1][None] if C == 2 else probabilities(x).argmax(dim=-1).float()[None]
    pixel = _Stub(probabilities, C)
    trainer = SimpleNamespace(preprocess=lambda x: (x * 0.5, None), model=_Stub(painted, C), postprocess=torch.round)
    seen = [[T._to_tensor(T.apply_view(patch, v), 'cpu') for v in views] for patch in T.divide_image_to_patches(img, p)]
    assert len(seen) == 9
    if C == 2:
        sp = T.predict_array(trainer, img, p, device='cpu', views=views)
        px = T.pixel_predict_array(pixel, img, p, device='cpu', views=views)
        want_sp = T.combine_views_to_image(np.stack([[painted(x * 0.5)[0].numpy() for x in w] for w in seen]), views, H, W)
        want_px = T.combine_views_to_image(np.stack([[probabilities(x).numpy()[..., 1] for x in w] for w in seen]), views, H, W)
        assert len(np.unique(sp)) > 2                                  # un-rounded values were merged
    else:
        sp = T.predict_array_classes(trainer, img, p, device='cpu', views=views)
        px = T.pixel_predict_array_classes(pixel, img, p, device='cpu', views=views)
        want_sp = T.combine_views_to_classes(np.stack([[painted(x * 0.5)[0].numpy() for x in w] for w in seen]), views, H, W, C,
                                             votes=True)
        want_px = T.combine_views_to_classes(np.stack([[probabilities(x).numpy() for x in w] for w in seen]), views, H, W, C)
    for got, want in ((sp, want_sp), (px, want_px)):
        assert got.shape == (H, W) and got.dtype == want.dtype and np.array_equal(got, want)
    assert len(np.unique(want_sp)) > 1 and len(np.unique(want_px)) > 1
    # and the views are not ignored
    none = (T.predict_array if C == 2 else T.predict_array_classes)(trainer, img, p, device='cpu')
    assert not np.array_equal(none, sp)


def test_command_line_tta():
    from wesup_amd import infer_tile as T
    assert T.parse_args(['d']).tta == 'none'
    for name in ('none', 'flips', 'rot', 'd4'):
        assert T.parse_args(['d', '--tta', name]).tta == name
    with pytest.raises(SystemExit):
        T.parse_args(['d', '--tta', 'all'])
    with mock.patch.object(T, 'initialize_trainer'), mock.patch.object(T, 'infer') as run:
        T.main(['d'])
        assert run.call_args[1] == {'device': 'cuda', 'batch': None}              # the default: no keyword at all
        T.main(['d', '--tta', 'none', '--batch', '2'])
        assert run.call_args[1] == {'device': 'cuda', 'batch': 2}
        T.main(['d', '--tta', 'd4', '--batch', '2'])
        assert run.call_args[1] == {'device': 'cuda', 'batch': 2, 'views': (0, 1, 2, 3, 4, 5, 6, 7)}
    with mock.patch.object(T, '_load_pixel_model', return_value='model'), mock.patch.object(T, 'pixel_infer') as run:
        T.main(['d', '--pixel', '--tta', 'flips'])
        assert run.call_args[1] == {'device': 'cuda', 'batch': None, 'views': (0, 2, 4, 6)}


def test_drivers_pass_views_through_and_round_a_two_class_map_once(tmp_path):
    from types import SimpleNamespace
    from PIL import Image
    from wesup_amd import infer_tile as T
    (tmp_path / 'images').mkdir()
    Image.fromarray(np.zeros((8, 8, 3), dtype=np.uint8)).save(tmp_path / 'images' / 'a.png')
    merged = np.array([[0.5, 0.5000001], [0.49, 1.0]])
    trainer = SimpleNamespace(model=SimpleNamespace(n_classes=2, eval=lambda: None))
    with mock.patch.object(T, 'predict_array', return_value=merged) as old, \
            mock.patch.object(T, 'predict_array_batched', return_value=merged) as new:
        got = T.infer(trainer, tmp_path, 8, views=(0, 4))
        assert old.call_args[1] == {'device': 'cuda', 'views': (0, 4)} and not new.called
        assert got[0].tolist() == [[0.0, 1.0], [0.0, 1.0]]             # np.round: the tie at 0.5 goes to 0
        got = T.infer(trainer, tmp_path, 8, batch=2, views=[0, 4])
        assert new.call_args[1] == {'batch': 2, 'device': 'cuda', 'views': (0, 4)}
        assert T.infer(trainer, tmp_path, 8)[0] is merged              # without views: what the form returns, as before
        assert old.call_args[1] == {'device': 'cuda'}
    model = SimpleNamespace(n_classes=2, eval=lambda: None)
    with mock.patch.object(T, 'pixel_predict_array', return_value=merged) as old:
        got = T.pixel_infer(model, tmp_path, 8, views=(0, 1))
        assert old.call_args[1] == {'device': 'cuda', 'views': (0, 1)} and got[0].tolist() == [[0.0, 1.0], [0.0, 1.0]]


# ------------------------------------------------------------------------------------------------------------- bindings
@pytest.fixture(scope='module')
def lib():
    from wesup_amd import _lib
    if not os.path.exists(_lib.LIB_PATH):
        _lib.build()
    return _lib


def test_entries_are_declared_exported_and_bound(lib):
    hdr = open(os.path.join(ROOT, 'include', 'wesup_hip.h')).read()
    hdr = re.sub(r'/\*.*?\*/', '', hdr, flags=re.S)
    handle = lib.load()
    for name, sig in ENTRIES.items():
        m = re.search(r'\bint\s+%s\s*\(([^;]*?)\)\s*;' % name, hdr, flags=re.S)
        assert m, name
        args = [a.strip() for a in m.group(1).replace('\n', ' ').split(',')]
        assert ''.join('p' if '*' in a else 'i' for a in args) == sig == lib._SIGS[name][1], name
        assert 'int n_views' in args and 'uint32_t views' in args       # the view list comes by value
        assert name in lib.EXPORTS and hasattr(handle, name)
        assert getattr(handle, name).restype is ctypes.c_int and len(getattr(handle, name).argtypes) == len(sig)
    assert handle.wesup_abi_version() == lib.ABI_VERSION == 6          # additions do not bump the ABI


BAD_WORDS = [(0, 0), (-1, 0), (9, D4_WORD), (2, 0x00), (2, 0x33), (3, 0x151), (1, 0x8), (2, 0x90), (8, 0x76543211),
             (8, 0xF6543210)]


def test_entries_refuse_a_wrong_view_word_on_the_host(lib):
    """Never a launch: the pointers are not memory.  With a good word every other argument check still fires; a good call is not
    made here (it would launch)."""
    h = lib.load()
    q = ctypes.c_void_p(4096)

    def gather(n_views, word, p=64):
        return h.wesup_window_gather_views(q, q, q, q, 80, 112, 2, 2, p, n_views, word, 0, 4, None)

    def merge(n_views, word, p=64):
        return h.wesup_window_merge_views(q, q, q, q, 80, 112, 1, 2, 2, p, n_views, word, 0, None)

    def classes(n_views, word, p=64, votes=0):
        return h.wesup_window_merge_classes_views(q, q, q, q, q, 80, 112, 3, 2, 2, p, n_views, word, votes, None)
    for entry in (gather, merge, classes):
        for n_views, word in BAD_WORDS:
            assert entry(n_views, word) == INVALID, (entry.__name__, n_views, hex(word))
        assert entry(8, D4_WORD, p=81) == INVALID and entry(1, 0, p=0) == INVALID          # p > H, p < 1 under a good word
    assert classes(2, 0x40, votes=2) == INVALID
    assert h.wesup_window_gather_views(None, q, q, q, 80, 112, 2, 2, 64, 1, 0, 0, 4, None) == INVALID
    assert h.wesup_window_gather_views(q, q, q, q, 80, 112, 2, 2, 64, 1, 0, 0, 0, None) == INVALID            # count < 1
    assert h.wesup_window_merge_views(q, q, q, None, 80, 112, 1, 2, 2, 64, 1, 0, 0, None) == INVALID
    assert h.wesup_window_merge_views(q, q, q, q, 80, 112, 0, 2, 2, 64, 1, 0, 0, None) == INVALID             # C < 1
    assert h.wesup_window_merge_classes_views(q, q, q, q, None, 80, 112, 3, 2, 2, 64, 1, 0, 0, None) == INVALID
    for C in (1, 17):
        assert h.wesup_window_merge_classes_views(q, q, q, q, q, 80, 112, C, 2, 2, 64, 1, 0, 0, None) == INVALID


def test_wrappers_check_their_arguments_and_have_no_cpu_fallback(lib):
    from wesup_amd import infer_tile as T
    from wesup_amd import ops
    tops, lefts = T.window_grid(80, 112, 64)
    img = torch.zeros(80, 112, 3, dtype=torch.uint8)
    with pytest.raises(lib.WesupHipError, match='no CPU fallback'):
        ops.window_gather(img, tops, lefts, 64, 0, 4, views=(0, 4))
    with pytest.raises(lib.WesupHipError, match='no CPU fallback'):
        ops.window_merge(torch.zeros(4, 2, 64, 64, 1), tops, lefts, 80, 112, views=(0, 4))
    with pytest.raises(lib.WesupHipError, match='no CPU fallback'):
        ops.window_merge_classes(torch.zeros(4, 2, 64, 64, 3), tops, lefts, 80, 112, views=(0, 4))
    with pytest.raises(lib.WesupHipError, match='views'):
        ops.window_gather(img, tops, lefts, 64, 0, 4, views=(0, 0))
    with pytest.raises(lib.WesupHipError, match='slots'):
        ops.window_gather(img, tops, lefts, 64, 0, 0, views=(0, 4))
    with pytest.raises(lib.WesupHipError, match='for 2 views'):
        ops.window_merge(torch.zeros(4, 3, 64, 64, 1), tops, lefts, 80, 112, views=(0, 4))
    with pytest.raises(lib.WesupHipError, match='windows for a lattice'):
        ops.window_merge(torch.zeros(3, 2, 64, 64), tops, lefts, 80, 112, views=(0, 4))
    with pytest.raises(lib.WesupHipError, match='not sorted'):
        ops.window_merge_classes(torch.zeros(4, 2, 64, 64, 3), [16, 0], lefts, 80, 112, views=(0, 4))
    with pytest.raises(lib.WesupHipError, match='n_classes'):
        ops.window_merge_classes(torch.zeros(4, 2, 64, 64), tops, lefts, 80, 112, votes=True, views=(0, 4))
    with pytest.raises(lib.WesupHipError, match='for 2 views'):
        ops.window_merge_classes(torch.zeros(4, 8, 64, 64), tops, lefts, 80, 112, n_classes=3, votes=True, views=(0, 4))
    with pytest.raises(lib.WesupHipError):
        ops.window_merge_classes(torch.zeros(4, 2, 64, 64, 3), tops, lefts, 80, 112, votes=True, views=(0, 4))
    # the earlier positional spelling is forwarded to the keyword form: the same checks
    with pytest.raises(lib.WesupHipError, match='no CPU fallback'):
        ops.window_gather_views(img, tops, lefts, 64, (0, 4), 0, 4)
    with pytest.raises(lib.WesupHipError, match='for 2 views'):
        ops.window_merge_views(torch.zeros(4, 3, 64, 64, 1), (0, 4), tops, lefts, 80, 112)
    with pytest.raises(lib.WesupHipError, match='n_classes'):
        ops.window_merge_classes_views(torch.zeros(4, 2, 64, 64), (0, 4), tops, lefts, 80, 112, votes=True)
