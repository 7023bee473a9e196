"""Test-time augmentation over the eight views of a window on the device (csrc/tiles.hip, csrc/classmap.hip,
csrc/lattice.hpp, infer_tile.py).

Kernels.  The host functions of ``infer_tile`` are the specification and every comparison is bit for bit: ``window_gather`` under
``views=`` against ``_to_tensor(apply_view(window, v))`` slot by slot, ``window_merge`` against ``combine_views_to_image``,
``window_merge_classes`` against ``combine_views_to_classes``; under the one upright view each equals the plain entry, the call
without views.  A round trip without a model -- the device-resident walk under all eight views with a pointwise ``forward``, merged
through the inverse index -- equals the walk without views: a forward / inverse mismatch of the index functions shows there.

End to end.  The models, weights and image of tests/test_tiles_gpu.py (two classes) and tests/test_classmaps_gpu.py (three
classes, biases shifted so that every class covers at least 10 % of the map, asserted).  Batch 1 of every batched form equals
its per-window form under the same views bit for bit; two runs at batch 4 are equal; batch 4 is compared with batch 1 outside
AMBIGUOUS pixels by those files' rule -- the top-two gap of the batch-1 run below 1e-5 (two classes: the merged value within
1e-5 of 0.5) -- which may be at most 1 % of the image."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import test_classmaps_gpu as CM          # noqa: E402
import test_tiles_gpu as TL              # noqa: E402
from test_tta_cpu import order_cases     # noqa: E402

pytestmark = pytest.mark.gpu

DEV = 'cuda:0'
SENTINEL = 77
D4 = (0, 1, 2, 3, 4, 5, 6, 7)
VIEW_LISTS = [(0,), (0, 4), (0, 1, 2, 3), D4, (5, 2)]
AMBIGUOUS, MAX_AMBIGUOUS_SHARE = CM.AMBIGUOUS, CM.MAX_AMBIGUOUS_SHARE
_d = CM._d


def _lattice(H, W, p):
    from wesup_amd import infer_tile as T
    tops, lefts = T.window_grid(H, W, p)
    return tops, lefts, len(tops) * len(lefts)


# ------------------------------------------------------------------------------------------------------------ 1. gather
def _view_slots(img, p, views):
    """What the gather is held to: ``_to_tensor(apply_view(window, v))`` for every window (row-major) and inside it every view."""
    from wesup_amd import infer_tile as T
    return torch.cat([T._to_tensor(T.apply_view(patch, v), DEV).contiguous() for patch in T.divide_image_to_patches(img, p)
                      for v in views])


@pytest.mark.parametrize('views', [D4, (5, 2), (3,)])
@pytest.mark.parametrize('H,W,p', [(13, 11, 5), (5, 5, 5), (13, 11, 8), (8, 8, 8)])      # p = 5: one pixel per thread, the centre
def test_window_gather_views_equals_to_tensor_of_the_views(H, W, p, views):                # pixel; p = 8: float4 stores
    from wesup_amd import ops
    img = TL._all_bytes_image(H * 100 + W + p, H, W) if H * W * 3 >= 256 else \
        np.random.RandomState(p).randint(0, 256, (H, W, 3)).astype(np.uint8)
    tops, lefts, N = _lattice(H, W, p)
    assert N == {(13, 5): 9, (13, 8): 4}.get((H, p), 1)                # ragged overlaps on both axes, or one window
    V, S = len(views), N * len(views)
    want = _view_slots(img, p, views)
    img_d = _d(img)
    got = ops.window_gather(img_d, tops, lefts, p, 0, S, views=views)
    assert got.shape == (S, 3, p, p) and got.dtype == torch.float32
    assert torch.equal(got, want)
    if V > 1:                                                          # the views differ: a view ignored would show
        assert not torch.equal(got[0], got[1])
    # a pass that starts inside a window and runs past the end: the tail repeats the LAST SLOT
    first = max(S - V - 1, 0) if N > 1 else S // 2
    assert V == 1 or first % V != 0
    out = torch.full((S - first + 3, 3, p, p), float('nan'), device=DEV)
    tail = ops.window_gather(img_d, tops, lefts, p, first, S - first + 3, out=out, views=views)
    assert tail is out
    for i in range(S - first + 3):
        assert torch.equal(tail[i], want[min(first + i, S - 1)]), i
    # the upright view alone is window_gather
    assert torch.equal(ops.window_gather(img_d, tops, lefts, p, 0, N + 1, views=(0,)), ops.window_gather(img_d, tops, lefts, p, 0, N + 1))


def test_window_gather_views_where_the_grid_stride_loop_wraps():
    """700 x 700 at p = 128 under all eight views: 36 windows, 288 slots, 1 179 648 threads' worth of float4 stores for a grid of
    at most 4096 blocks of 256 -- every thread of the first 131 072 makes a second round."""
    from wesup_amd import ops
    H = W = 700
    p = 128
    img = TL._all_bytes_image(11, H, W)
    tops, lefts, N = _lattice(H, W, p)
    S = N * 8
    assert S * p * (p // 4) > 4096 * 256
    got = ops.window_gather(_d(img), tops, lefts, p, 0, S, views=D4)
    assert torch.equal(got, _view_slots(img, p, D4))


# ------------------------------------------------------------------------------------------------------------- 2. merge
def _planted(rs, shape):
    """fp32 predictions with 1/16 of the values at x.5 (ties of the rounding: half to even) and 1/16 at 1.0."""
    pred = (rs.rand(*shape) * 3).astype(np.float32)
    flat = pred.reshape(-1)
    flat[rs.permutation(flat.size)[:flat.size // 16]] = rs.choice(np.array([0.5, 1.5, 2.5], dtype=np.float32), flat.size // 16)
    flat[rs.permutation(flat.size)[:flat.size // 16]] = np.float32(1.0)
    return pred


@pytest.mark.parametrize('C', [1, 2, 3, 16])
@pytest.mark.parametrize('H,W,p', CM.MERGE_SIZES)
def test_window_merge_views_equals_the_host_merge(H, W, p, C):
    from wesup_amd import infer_tile as T
    from wesup_amd import ops
    tops, lefts, N = _lattice(H, W, p)
    all_views = _planted(np.random.RandomState(H + W + C), (N, 8, p, p, C))
    for views in VIEW_LISTS:
        pred = np.ascontiguousarray(all_views[:, :len(views)])
        pred_d = _d(pred)
        for round_first in (False, True):
            host = T.combine_views_to_image(np.round(pred) if round_first else pred, views, H, W).reshape(H, W, C)
            out = torch.full((H, W, C), float('nan'), dtype=torch.float64, device=DEV)
            got = ops.window_merge(pred_d, tops, lefts, H, W, round_first=round_first, out=out, views=views)
            assert got is out and np.array_equal(got.cpu().numpy(), host), (views, round_first)
        if views == (0,):                                              # the upright view alone is window_merge
            assert torch.equal(ops.window_merge(pred_d, tops, lefts, H, W, views=views), ops.window_merge(pred_d[:, 0], tops, lefts, H, W))
        elif views == (5, 2):                                          # and the list is not ignored
            assert not np.array_equal(T.combine_views_to_image(pred, (2, 5), H, W).reshape(H, W, C), host)
        if C == 1:                                                     # the (N,V,p,p) form
            got = ops.window_merge(pred_d[..., 0].contiguous(), tops, lefts, H, W, views=views)
            assert got.shape == (H, W) and np.array_equal(got.cpu().numpy(), T.combine_views_to_image(pred[..., 0], views, H, W))


def test_window_merge_views_adds_in_the_order_of_the_definition():
    """tests/test_tta_cpu.py::order_cases: sums that depend on the order, at their hand-computed values."""
    from wesup_amd import infer_tile as T
    from wesup_amd import ops
    for pred, views, H, W, at, want, other in order_cases():
        tops, lefts, N = _lattice(H, W, pred.shape[2])
        got = ops.window_merge(_d(pred), tops, lefts, H, W, views=views).cpu().numpy()
        assert got[at] == want and got[at] != other, (views, got[at])
        assert np.array_equal(got, T.combine_views_to_image(pred, views, H, W))


# ------------------------------------------------------------------------------------------------------- 3. class merge
def _corners(p):
    """The four 4 x 4 corner blocks of a window: a set of pixels that every view maps onto itself."""
    mask = np.zeros((p, p), dtype=bool)
    mask[:4, :4] = mask[:4, -4:] = mask[-4:, :4] = mask[-4:, -4:] = True
    return mask


def _view_votes(rs, H, W, p, C, views):
    """(N,V,p,p) fp32 class indices in view space: all windows and views agree on a random map, then 1/16 of the entries get a
    random class -- a split vote between the views of one window, and between windows in an overlap.  Where there are two
    views or more, the first half of window 0's views vote for class C - 1 in the corner blocks and the other half for class 0:
    a tie between the views of one window that goes to the lowest class wherever window 0 alone covers a pixel."""
    from wesup_amd import infer_tile as T
    base = rs.randint(0, C, (H, W))
    votes = np.stack([[T.apply_view(base[t:t + p, l:l + p], v) for v in views]
                      for t, l in T._get_top_left_coordinates(H, W, p)]).astype(np.float32)
    flat = votes.reshape(-1)
    pick = rs.permutation(flat.size)[:flat.size // 16]
    flat[pick] = rs.randint(0, C, len(pick)).astype(np.float32)
    V = len(views)
    if V >= 2:
        votes[0, :V // 2, _corners(p)] = C - 1
        votes[0, V // 2:, _corners(p)] = 0
    return votes


def _view_probabilities(rs, N, V, p, C):
    """(N,V,p,p,C) fp32: 1/16 of the vectors with two equal largest entries; and where there are two views or more, window 0
    holds in its corner blocks 0.5 for class C - 1 and 0.125 for class 0 under its first view, the other way round under its
    second and zeros under the others: the SUMS of the two classes tie exactly, 0.625 -- a tie between the views of one window,
    which the first maximum decides wherever window 0 alone covers a pixel."""
    pred = CM._probabilities(rs, N * V, p, C).reshape(N, V, p, p, C)
    if V >= 2:
        corners = _corners(p)
        pred[0, :, corners] = 0.0
        pred[0, 0, corners, C - 1], pred[0, 0, corners, 0] = 0.5, 0.125
        pred[0, 1, corners, C - 1], pred[0, 1, corners, 0] = 0.125, 0.5
    return pred


@pytest.mark.parametrize('votes', [False, True])
@pytest.mark.parametrize('C', [2, 3, 5, 9, 16])
@pytest.mark.parametrize('H,W,p', CM.MERGE_SIZES)
def test_window_merge_classes_views_equals_the_host_function(H, W, p, C, votes):
    from wesup_amd import infer_tile as T
    from wesup_amd import ops
    tops, lefts, N = _lattice(H, W, p)
    out = torch.full((H, W), SENTINEL, dtype=torch.uint8, device=DEV)
    status = torch.full((1,), 5, dtype=torch.int32, device=DEV)                # zeroed by the entry
    for views in VIEW_LISTS:
        V = len(views)
        rs = np.random.RandomState(H + W + 17 * C + votes + V)
        pred = _view_votes(rs, H, W, p, C, views) if votes else _view_probabilities(rs, N, V, p, C)
        want = T.combine_views_to_classes(pred, views, H, W, C, votes=votes)
        out.fill_(SENTINEL)
        status.fill_(5)
        got, st = ops.window_merge_classes(_d(pred), tops, lefts, H, W, n_classes=C, votes=votes, out=out, status=status, views=views)
        assert got is out and st is status and int(status) == 0
        assert np.array_equal(got.cpu().numpy(), want), (views, int((got.cpu().numpy() != want).sum()))
        assert len(np.unique(want)) == C, views                                # every class is somewhere
        if V > 1:                                                              # ties are among the pixels: the first maximum decides
            onehot = (pred[..., None] == np.arange(C)).astype(np.float64) if votes else pred
            top = np.sort(T.combine_views_to_image(onehot, views, H, W).reshape(H, W, C), axis=-1)
            assert (top[..., -1] == top[..., -2]).any(), views
        if V > 1:
            assert want[0, 0] == 0                                             # window 0's planted tie of classes C - 1 and 0
        if views == (0,):                                                      # the upright view alone is window_merge_classes
            sibling, _ = ops.window_merge_classes(_d(pred[:, 0]), tops, lefts, H, W, n_classes=C, votes=votes)
            assert torch.equal(got, sibling)
        if votes:                                  # -1, C and a NaN: the status is set, the votes are not counted, no fault
            bad = pred.copy()
            bad[0, 0, 0, 0], bad[0, V - 1, 1, 1], bad[N - 1, V - 1, p - 1, p - 1] = -1.0, float(C), np.nan
            want = T.combine_views_to_classes(bad, views, H, W, C, votes=True)
            got, st = ops.window_merge_classes(_d(bad), tops, lefts, H, W, n_classes=C, votes=True, out=out, status=status, views=views)
            assert int(st) != 0 and np.array_equal(got.cpu().numpy(), want), views
            if N == 1 and V == 1:
                assert want[0, 0] == 0 and want[1, 1] == 0 and want[H - 1, W - 1] == 0      # nobody voted there


WRAP = (1100, 1000, 550, (5, 2))         # 2 x 2 windows that overlap along x; 1 100 000 pixels, more than the merges' 4096 x 256 threads


@pytest.mark.parametrize('what', ['mean', 'votes', 'probabilities'])
def test_merges_under_views_where_the_grid_stride_loop_wraps(what):
    """Every other size here fits the grid once; the end-to-end cases wrap it, but without views."""
    from wesup_amd import infer_tile as T
    from wesup_amd import ops
    H, W, p, views = WRAP
    tops, lefts, N = _lattice(H, W, p)
    assert N == 4 and list(lefts) == [0, 450] and H * W > 4096 * 256
    rs = np.random.RandomState(len(what))
    if what == 'mean':
        pred = _planted(rs, (N, 2, p, p, 1))
        got = ops.window_merge(_d(pred), tops, lefts, H, W, views=views)
        want = T.combine_views_to_image(pred, views, H, W).reshape(H, W, 1)
    else:
        votes = what == 'votes'
        pred = _view_votes(rs, H, W, p, 3, views) if votes else _view_probabilities(rs, N, 2, p, 3)
        got, status = ops.window_merge_classes(_d(pred), tops, lefts, H, W, n_classes=3, votes=votes, views=views)
        assert int(status) == 0
        want = T.combine_views_to_classes(pred, views, H, W, 3, votes=votes)
    assert np.array_equal(got.cpu().numpy(), want)


# ---------------------------------------------------------------------------------------- 4. round trip without a model
@pytest.mark.parametrize('H,W,p,batch', [(150, 333, 64, 5), (13, 11, 5, 3), (64, 64, 64, 8)])
def test_round_trip_through_the_walk_equals_the_walk_without_views(H, W, p, batch):
    """A pointwise forward (channel 0 of the input) commutes with every view, so gathering all eight views, keeping them and
    merging them through the inverse index must give the merge without views.  Bit for bit: the inputs are bytes / 255 in fp32,
    so the sum of the 8 x cnt equal values of a window is exact in fp64, and 8 S / (8 cnt) is S / cnt (a power of two)."""
    from wesup_amd import infer_tile as T
    from wesup_amd import ops
    img = TL._all_bytes_image(H + W, H, W)

    def forward(x):
        return x[:, 0, :, :, None].contiguous()
    kept, tops, lefts, h, w = T._resident_windows(img, p, batch, None, DEV, forward, (1,))
    plain = ops.window_merge(kept, tops, lefts, H, W)
    N = kept.shape[0]
    for views in (D4, (6, 3, 1)):
        kept_v, tops_v, lefts_v, h, w = T._resident_windows(img, p, batch, None, DEV, forward, (1,), views=views)
        assert kept_v.shape == (N, len(views), p, p, 1) and (h, w) == (H, W)
        assert list(tops_v) == list(tops) and list(lefts_v) == list(lefts)
        if views == D4:
            turned = ops.window_merge(kept_v, tops, lefts, H, W, views=views)
            assert torch.equal(turned, plain)
            assert p == 1 or not torch.equal(kept_v[:, 1], kept_v[:, 0])       # (the views were really made)
        # ... and every kept slot is its view of the window's plain prediction (any list, any batch: the slot arithmetic)
        host = kept.cpu().numpy()
        for t, v in enumerate(views):
            assert np.array_equal(kept_v[:, t].cpu().numpy(), np.stack([T.apply_view(k, v) for k in host])), v
    assert np.array_equal(plain.cpu().numpy()[..., 0], T.combine_patches_to_image(host[..., 0], H, W))


# ------------------------------------------------------------------------------------------------------- 5. end to end
H_, W_, P_ = 150, 333, 64                            # 18 windows, ragged overlaps on both axes
VIEW_SETS_TESTED = ['flips', 'd4']


@pytest.fixture(scope='module')
def image():
    return TL._image(TL.IMAGE_SEED, H_, W_)


@pytest.fixture(scope='module')
def trainer2():
    return TL._trainer(TL._weights(), sp_area=64)


@pytest.fixture(scope='module')
def pixel2():
    from wesup_amd.models.wesup import WESUPPixelInference
    model = WESUPPixelInference().to(DEV)
    CM._load(model, TL._weights())
    return model


@pytest.fixture(scope='module')
def trainer3():
    return CM._trainer3()


@pytest.fixture(scope='module')
def pixel3():
    return CM._pixel3()


def _recorded(monkeypatch, name):
    """Record the prediction buffer a form hands to ``ops.<name>`` (the merge of the batched forms)."""
    from wesup_amd import ops
    seen, real = [], getattr(ops, name)

    def recording(pred, *args, **kw):
        seen.append(pred)
        return real(pred, *args, **kw)
    monkeypatch.setattr(ops, name, recording)
    return seen


def _few_ambiguous(name, amb):
    share = float(amb.mean())
    print(f'{name}: ambiguous pixels {share:.5f} of the image')
    assert share <= MAX_AMBIGUOUS_SHARE, (name, share)


def _two_class_paths(name, host_form, batched_form, model, img, views):
    """Two classes, both models: the merged map is a mean of un-rounded probabilities, the tools round it once."""
    single = host_form(model, img, P_, device=DEV, views=views)
    assert single.shape == (H_, W_) and single.dtype == np.float64 and 0.0 <= single.min() and single.max() <= 1.0
    assert len(np.unique(single)) > 2                                          # un-rounded values were merged
    one = batched_form(model, img, P_, batch=1, device=DEV, views=views)
    assert one.dtype == np.float64 and np.array_equal(one, single)
    zeros, ones = float((np.round(single) == 0).mean()), float((np.round(single) == 1).mean())
    print(f'{name}: {zeros:.3f} of the rounded batch-1 map at 0, {ones:.3f} at 1')
    amb = np.abs(single - 0.5) < AMBIGUOUS
    _few_ambiguous(name, amb)
    a = batched_form(model, img, P_, batch=4, device=DEV, views=views)
    b = batched_form(model, img, P_, batch=4, device=DEV, views=views)
    assert np.array_equal(a, b)                                                # run to run
    differ = np.round(a) != np.round(single)
    print(f'{name}: batch 4 max |p - p_batch1| = {float(np.abs(a - single).max()):.3e}, {int(differ.sum())} rounded pixels differ, '
          f'{int((differ & ~amb).sum())} of them outside ambiguous pixels')
    assert np.array_equal(np.round(a)[~amb], np.round(single)[~amb])
    return single


@pytest.mark.parametrize('tta', VIEW_SETS_TESTED)
def test_two_class_superpixel_forms_under_views(trainer2, image, tta):
    from wesup_amd import infer_tile as T
    views = T.VIEW_SETS[tta]
    single = _two_class_paths(f'superpixels, two classes, {tta}', T.predict_array, T.predict_array_batched, trainer2, image, views)
    zeros, ones = float((np.round(single) == 0).mean()), float((np.round(single) == 1).mean())
    assert zeros >= 0.10 and ones >= 0.10, (zeros, ones)                       # not vacuous (test_tiles_gpu.py's bar)
    none = T.predict_array_batched(trainer2, image, P_, batch=1, device=DEV)
    differ = int((np.round(single) != np.round(none)).sum())
    print(f'superpixels, two classes, {tta}: {differ} pixels differ from the rounded map without views')
    assert differ > 0                                                          # the views are not ignored


@pytest.mark.parametrize('tta', VIEW_SETS_TESTED)
def test_two_class_pixel_forms_under_views(pixel2, image, tta):
    from wesup_amd import infer_tile as T
    single = _two_class_paths(f'pixel-wise, two classes, {tta}', T.pixel_predict_array, T.pixel_predict_array_batched, pixel2, image,
                              T.VIEW_SETS[tta])
    assert not np.array_equal(single, T.pixel_predict_array_batched(pixel2, image, P_, batch=1, device=DEV))


@pytest.mark.parametrize('tta', VIEW_SETS_TESTED)
def test_three_class_superpixel_forms_under_views(trainer3, image, tta):
    from wesup_amd import infer_tile as T
    views = T.VIEW_SETS[tta]
    name = f'superpixels, three classes, {tta}'
    single = T.predict_array_classes(trainer3, image, P_, device=DEV, views=views)
    assert single.shape == (H_, W_) and single.dtype == np.uint8
    CM._assert_not_vacuous(name, single)
    # the top-two gap of every pixel's superpixel, per (window, view) slot of the batch-1 run, in view space
    gaps = []

    def hook(model, inputs, output):
        sp = model._padded[1][0]
        rows = model._last_meta.new_row[0].long()
        top = torch.topk(sp, 2, dim=-1).values
        gaps.append((top[:, 0] - top[:, 1])[rows].view(output.shape[-2:]).cpu().numpy())
    handle = trainer3.model.register_forward_hook(hook)
    try:
        one = T.predict_array_classes_batched(trainer3, image, P_, batch=1, device=DEV, views=views)
    finally:
        handle.remove()
    assert np.array_equal(one, single)
    N = 18
    assert len(gaps) == N * len(views)
    near = (np.stack(gaps).reshape(N, len(views), P_, P_) < AMBIGUOUS).astype(np.float64)
    amb = T.combine_views_to_image(near, views, H_, W_) > 0
    _few_ambiguous(name, amb)
    a = T.predict_array_classes_batched(trainer3, image, P_, batch=4, device=DEV, views=views)
    assert np.array_equal(T.predict_array_classes_batched(trainer3, image, P_, batch=4, device=DEV, views=views), a)
    CM._compare_outside_ambiguous(f'{name}, batch 4', a, single, amb)
    none = T.predict_array_classes_batched(trainer3, image, P_, batch=1, device=DEV)
    differ = int((none != single).sum())
    print(f'{name}: {differ} pixels differ from the map without views')
    assert differ > 0                                                          # the views are not ignored


@pytest.mark.parametrize('tta', VIEW_SETS_TESTED)
def test_three_class_pixel_forms_under_views(pixel3, image, tta, monkeypatch):
    from wesup_amd import infer_tile as T
    from wesup_amd import ops
    views = T.VIEW_SETS[tta]
    name = f'pixel-wise, three classes, {tta}'
    single = T.pixel_predict_array_classes(pixel3, image, P_, device=DEV, views=views)
    assert single.shape == (H_, W_) and single.dtype == np.uint8
    CM._assert_not_vacuous(name, single)
    seen = _recorded(monkeypatch, 'window_merge_classes')
    one = T.pixel_predict_array_classes_batched(pixel3, image, P_, batch=1, device=DEV, views=views)
    assert np.array_equal(one, single) and len(seen) == 1 and seen[0].shape == (18, len(views), P_, P_, 3)
    tops, lefts, N = _lattice(H_, W_, P_)
    merged = ops.window_merge(seen[0], tops, lefts, H_, W_, views=views).cpu().numpy()      # the means behind the batch-1 map
    assert np.array_equal(single, merged.argmax(axis=-1))
    amb = CM._top_two_gap(merged) < AMBIGUOUS
    _few_ambiguous(name, amb)
    a = T.pixel_predict_array_classes_batched(pixel3, image, P_, batch=4, device=DEV, views=views)
    assert np.array_equal(T.pixel_predict_array_classes_batched(pixel3, image, P_, batch=4, device=DEV, views=views), a)
    CM._compare_outside_ambiguous(f'{name}, batch 4', a, single, amb)
    assert not np.array_equal(single, T.pixel_predict_array_classes_batched(pixel3, image, P_, batch=1, device=DEV))


# ------------------------------------------------------------------------------------------------------------- 6. the tool
def test_command_line_writes_what_the_function_returns(tmp_path):
    from PIL import Image
    from wesup_amd import infer_tile as T
    from wesup_amd.models import initialize_trainer
    data = tmp_path / 'd'
    (data / 'images').mkdir(parents=True)
    imgs = {'one.png': TL._image(TL.IMAGE_SEED, 80, 112), 'two.png': TL._image(TL.IMAGE_SEED + 1, 64, 100)}
    for name, img in imgs.items():
        Image.fromarray(img).save(data / 'images' / name)
    weights = TL._weights()
    ckpt = tmp_path / 'run' / 'checkpoints' / 'ckpt.0001.pth'
    ckpt.parent.mkdir(parents=True)
    torch.save({'epoch': 0, 'model_state_dict': {k: torch.from_numpy(v) for k, v in weights.items()}}, ckpt)
    T.main([str(data), '--tta', 'd4', '--batch', '2', '--patch-size', '64', '--checkpoint', str(ckpt), '--output-dir',
            str(tmp_path / 'out'), '--device', DEV])
    assert sorted(q.name for q in (tmp_path / 'out').iterdir()) == ['one.png', 'two.png']
    trainer = initialize_trainer('wesup', device=DEV)                          # the tool's trainer: the default sp_area
    CM._load(trainer.model, weights)
    plain_differs = False
    for name, img in imgs.items():
        merged = T.predict_array_batched(trainer, img, 64, batch=2, device=DEV, views=T.VIEW_SETS['d4'])
        saved = np.asarray(Image.open(tmp_path / 'out' / name))
        assert saved.shape == img.shape[:2] and np.array_equal(saved, np.round(merged).astype('uint8') * 255)
        plain_differs |= not np.array_equal(np.round(merged), np.round(T.predict_array_batched(trainer, img, 64, batch=2, device=DEV)))
    assert plain_differs                                                       # (--tta was not ignored)
