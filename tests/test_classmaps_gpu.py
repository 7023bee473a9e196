"""Class maps for more than two classes on the device (csrc/classmap.hip, infer_tile.py, pixel_infer.py,
slide.py).

Kernels.  The reference has no class maps, so the host functions are the specification and every comparison is bit for bit:
``window_merge_classes`` against ``infer_tile.combine_patches_to_classes``; every plane of ``planes_resize_acc`` against the
one-plane ``plane_resize_acc``; ``class_argmax_u8`` against ``np.argmax``; ``patch_scatter_classes_u8`` against nearest
``F.interpolate`` of the index map (mode 0) and against ``class_argmax_u8(planes_resize_acc(...))`` (mode 1), pasted and cropped;
``label_confusion`` against ``np.bincount``.

End to end.  A three-class model: ``oracle.make_weights(3, feat_scale=1.0)`` with the seeded classifier of
tests/test_multiclass_gpu.py::weights_c.  Random weights put nearly every superpixel into one class, which would make a
comparison of class maps vacuous, so the classifier's biases are shifted: per class the median, over the rows of window 0, of
log(p_c / p_0) -- the logit difference z_c - z_0 -- is taken off bias c (derived when the module's fixtures are made, once for
the superpixel model and once for the pixel-wise one, and once more for the pixel-wise slide path, which sees its patches at
another scale), and every test asserts that each class covers at least 10 % of its batch-1 map.  Batch 1 of every batched path
equals its per-window / per-patch path bit for bit; at another batch size the convolutions tile differently and a probability moves by ~2e-6 (tests/test_tiles_gpu.py), so the maps are compared outside
AMBIGUOUS pixels -- the top two probabilities of the batch-1 run less than 1e-5 apart -- which may be at most 1 % of the image."""
import ctypes
import os
import sys

import numpy as np
import pytest
import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from test_pixel_resolution_gpu import RESIZE_CASES          # noqa: E402
from test_slide_gpu import LATTICES                         # noqa: E402

pytestmark = pytest.mark.gpu

DEV = 'cuda:0'
SENTINEL = 77
AMBIGUOUS = 1e-5           # top-two gap below this: the class may differ between two batch sizes (tests/test_tiles_gpu.py's bar)
MAX_AMBIGUOUS_SHARE = 0.01
MIN_CLASS_SHARE = 0.10
WEIGHT_SEED, FEAT_SCALE, IMAGE_SEED, C3 = 3, 1.0, 5, 3
ENTRIES = ['wesup_window_merge_classes', 'wesup_planes_resize_acc', 'wesup_class_argmax_u8', 'wesup_patch_scatter_classes_u8',
           'wesup_label_confusion']


def _d(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


# ====================================================================================================== kernels
# ------------------------------------------------------------------------------------------------ 1. window_merge_classes
MERGE_SIZES = [(64, 64, 64), (80, 112, 64), (150, 333, 64)]           # one window, even overlaps, ragged overlaps


def _probabilities(rs, N, p, C):
    """(N,p,p,C) fp32; 1/16 of the vectors with two equal largest entries."""
    pred = rs.rand(N, p, p, C).astype(np.float32)
    rows = pred.reshape(-1, C)
    pick = rs.permutation(len(rows))[:len(rows) // 16]
    a = rs.randint(0, C, len(pick))
    b = (a + 1 + rs.randint(0, C - 1, len(pick))) % C                  # another class
    rows[pick, a] = rows[pick, b] = np.float32(1.5)
    return pred


def _votes(rs, H, W, p, C):
    """(N,p,p) fp32 class indices: the windows agree on a random map, then 1/16 of the entries get a random class -- in an overlap
    of two windows that is a split vote."""
    from wesup_amd import infer_tile as T
    base = rs.randint(0, C, (H, W))
    votes = np.stack([base[t:t + p, l:l + p] for t, l in T._get_top_left_coordinates(H, W, p)]).astype(np.float32)
    flat = votes.reshape(-1)
    pick = rs.permutation(flat.size)[:flat.size // 16]
    flat[pick] = rs.randint(0, C, len(pick)).astype(np.float32)
    return votes


@pytest.mark.parametrize('votes', [False, True])
@pytest.mark.parametrize('C', [2, 3, 5, 9, 16])
@pytest.mark.parametrize('H,W,p', MERGE_SIZES)
def test_window_merge_classes_equals_the_host_function(H, W, p, C, votes):
    from wesup_amd import infer_tile as T
    from wesup_amd import ops
    tops, lefts = T.window_grid(H, W, p)
    N = len(tops) * len(lefts)
    rs = np.random.RandomState(H + W + 17 * C + votes)
    pred = _votes(rs, H, W, p, C) if votes else _probabilities(rs, N, p, C)
    want = T.combine_patches_to_classes(pred, H, W, C, votes=votes)
    out = torch.full((H, W), SENTINEL, dtype=torch.uint8, device=DEV)
    status = torch.full((1,), 5, dtype=torch.int32, device=DEV)                # zeroed by the entry
    got, st = ops.window_merge_classes(_d(pred), tops, lefts, H, W, n_classes=C, votes=votes, out=out, status=status)
    assert got is out and st is status and int(status) == 0
    assert np.array_equal(got.cpu().numpy(), want), int((got.cpu().numpy() != want).sum())
    assert len(np.unique(want)) == C                                           # every class is somewhere
    if votes and N > 1:
        merged = T.combine_patches_to_image((pred[..., None] == np.arange(C)).astype(np.float64), H, W)
        top = np.sort(merged, axis=-1)
        assert (top[..., -1] == top[..., -2]).any()                            # and split votes are among them
    if votes:                                      # -1, C and a NaN: the status is set, the votes are not counted
        bad = pred.copy()
        bad[0, 0, 0], bad[0, 1, 1], bad[N - 1, p - 1, p - 1] = -1.0, float(C), np.nan
        want = T.combine_patches_to_classes(bad, H, W, C, votes=True)
        got, st = ops.window_merge_classes(_d(bad), tops, lefts, H, W, n_classes=C, votes=True, out=out, status=status)
        assert int(st) != 0 and np.array_equal(got.cpu().numpy(), want)
        if N == 1:
            assert want[0, 0] == 0 and want[1, 1] == 0 and want[H - 1, W - 1] == 0       # nobody voted there


# ---------------------------------------------------------------------------------------------------- 2. planes_resize_acc
@pytest.mark.parametrize('C', [2, 3, 16])
@pytest.mark.parametrize('src,dst', RESIZE_CASES)
def test_planes_resize_acc_equals_plane_resize_acc_plane_by_plane(src, dst, C):
    from wesup_amd import ops
    rs = np.random.RandomState(src[0] * 100 + dst[0] + C)
    a, b = _d(rs.rand(*src, C).astype(np.float32)), _d(rs.rand(*src, C).astype(np.float32))
    out = torch.full((*dst, C), float('nan'), device=DEV)
    assert ops.planes_resize_acc(a, out, alpha=1.0) is out                     # overwrites the NaNs
    for c in range(C):
        one = torch.full(dst, float('nan'), device=DEV)
        ops.plane_resize_acc(a[..., c], one, alpha=1.0)
        assert torch.equal(out[..., c], one), c
    ops.planes_resize_acc(a, out, alpha=0.5)                                   # the running mean of two scales
    ops.planes_resize_acc(b, out, alpha=0.5, accumulate=True)
    assert not bool(torch.isnan(out).any())
    for c in range(C):
        one = torch.full(dst, float('nan'), device=DEV)
        ops.plane_resize_acc(a[..., c], one, alpha=0.5)
        ops.plane_resize_acc(b[..., c], one, alpha=0.5, accumulate=True)
        assert torch.equal(out[..., c], one), c
    thirds = [a, b, _d(rs.rand(*src, C).astype(np.float32))]                   # alpha = 1/3: the product is not exact, so an fma of
    for i, t in enumerate(thirds):                                             # it with the add would show (C = 16: the float4 form)
        ops.planes_resize_acc(t, out, alpha=1.0 / 3, accumulate=i > 0)
    for c in range(C):
        one = torch.full(dst, float('nan'), device=DEV)
        for i, t in enumerate(thirds):
            ops.plane_resize_acc(t[..., c], one, alpha=1.0 / 3, accumulate=i > 0)
        assert torch.equal(out[..., c], one), c
    same = torch.full((*src, C), float('nan'), device=DEV)                     # a resize that is none
    ops.planes_resize_acc(a, same)
    assert torch.equal(same, a)


# ------------------------------------------------------------------------------------------------------ 3. class_argmax_u8
@pytest.mark.parametrize('C', [2, 3, 8, 16])
@pytest.mark.parametrize('n', [1, 63, 65, 4099, 1200000])                      # the last one wraps the grid-stride loop
def test_class_argmax_takes_the_first_maximum(n, C):
    from wesup_amd import ops
    rs = np.random.RandomState(n % 9973 + C)
    x = rs.rand(n, C).astype(np.float32)
    pick = rs.permutation(n)[:max(n // 8, 1)]                                  # planted ties, a tie of all classes among them
    a = rs.randint(0, C, len(pick))
    b = (a + 1 + rs.randint(0, C - 1, len(pick))) % C
    x[pick, a] = x[pick, b] = np.float32(2.0)
    x[pick[0]] = np.float32(0.25)
    got = ops.class_argmax_u8(_d(x))
    assert got.shape == (n,) and got.dtype == torch.uint8
    assert np.array_equal(got.cpu().numpy(), x.argmax(axis=1).astype(np.uint8))
    if n == 4099:                                                              # leading dimensions are kept
        assert ops.class_argmax_u8(_d(x).view(1, n, C)).shape == (1, n)


def test_class_argmax_with_a_nan():
    """No comparison with a NaN is true: one behind the first entry is never the maximum, one in the first entry gives class 0."""
    from wesup_amd import ops
    nan = float('nan')
    x = np.array([[0.5, nan, 1.0], [1.0, nan, 0.5], [nan, 1.0, 2.0], [0.1, 0.2, nan]], dtype=np.float32)
    assert ops.class_argmax_u8(_d(x)).cpu().tolist() == [2, 0, 0, 1]


# --------------------------------------------------------------------------------------------- 4. patch_scatter_classes_u8
def _paste_reference(patch_maps, H, W, p, first, n_total):
    """(count,p,p) uint8 -> the (H,W) map with SENTINEL where nothing is written."""
    n_w = -(-W // p)
    n_h = -(-H // p)
    out = np.full((n_h * p, n_w * p), SENTINEL, dtype=np.uint8)
    for n, m in enumerate(patch_maps):
        k = first + n
        if k >= n_total:
            continue
        y, x = k // n_w * p, k % n_w * p
        out[y:y + p, x:x + p] = m
    return out[:H, :W]


@pytest.mark.parametrize('C', [3, 16])
@pytest.mark.parametrize('H,W,p,size', LATTICES[:5])
def test_patch_scatter_classes_pastes_class_indices(H, W, p, size, C):
    from wesup_amd import ops
    from wesup_amd import slide as S
    n_h, n_w = S.patch_grid(H, W, p)
    N = n_h * n_w
    rs = np.random.RandomState(H + W + p + C)
    # ---- mode 0: nearest resize of the index map
    idx = rs.randint(0, C, (N, *size)).astype(np.float32)
    near = F.interpolate(torch.from_numpy(idx)[:, None], size=(p, p), mode='nearest')[:, 0].numpy().astype(np.uint8)
    out = torch.full((H, W), SENTINEL, dtype=torch.uint8, device=DEV)
    got, status = ops.patch_scatter_classes_u8(_d(idx), out, p, 0, n_classes=C, mode=0)
    assert got is out and int(status) == 0
    want = _paste_reference(near, H, W, p, 0, N)
    assert np.array_equal(out.cpu().numpy(), want) and SENTINEL not in np.unique(want)
    # ---- mode 1: every plane resized back, then the first maximum
    prob = rs.rand(N, *size, C).astype(np.float32)
    rows = prob.reshape(-1, C)
    pick = rs.permutation(len(rows))[:len(rows) // 16]
    rows[pick, 0] = rows[pick, C - 1] = np.float32(1.5)                        # ties that survive where a texel is hit exactly
    prob_d = _d(prob)
    resized = []
    for k in range(N):
        full = torch.empty(p, p, C, device=DEV)
        ops.planes_resize_acc(prob_d[k], full, alpha=1.0)
        resized.append(ops.class_argmax_u8(full).cpu().numpy())
    out.fill_(SENTINEL)
    ops.patch_scatter_classes_u8(prob_d, out, p, 0, mode=1, status=status)
    want1 = _paste_reference(resized, H, W, p, 0, N)
    assert np.array_equal(out.cpu().numpy(), want1), int((out.cpu().numpy() != want1).sum())
    assert int(status) == 0
    # ---- a pass in the middle and a ragged last pass (more predictions than patches are left): only their patches are written
    for mode, src, maps in ((0, _d(idx), near), (1, prob_d, resized)):
        for first, count in ((N // 2, 1), (N - 1, 2)):
            if first + count > N:
                pred = torch.cat([src[first:], src[:first + count - N]])       # the tail of a padded pass: never pasted
            else:
                pred = src[first:first + count]
            out.fill_(SENTINEL)
            ops.patch_scatter_classes_u8(pred.contiguous(), out, p, first, n_classes=C, mode=mode)
            want = _paste_reference(maps[first:first + count], H, W, p, first, N)
            assert np.array_equal(out.cpu().numpy(), want), (mode, first, count)
            assert N == 1 or (want == SENTINEL).any()                          # the sentinel survives outside them
    # ---- an index >= C: pasted as 0, and the status says so (it is OR-ed into: a later clean pass does not clear it)
    bad = idx.copy()
    bad[0, 0, 0] = float(C)
    status.zero_()
    out.fill_(SENTINEL)
    ops.patch_scatter_classes_u8(_d(bad), out, p, 0, n_classes=C, mode=0, status=status)
    assert int(status) != 0 and int(out[0, 0]) == 0
    ops.patch_scatter_classes_u8(_d(idx), out, p, 0, n_classes=C, mode=0, status=status)
    assert int(status) != 0 and np.array_equal(out.cpu().numpy(), _paste_reference(near, H, W, p, 0, N))


# ------------------------------------------------------------------------------------------------------ 5. label_confusion
@pytest.mark.parametrize('C', [3, 16])
@pytest.mark.parametrize('n', [1, 15, 16, 63, 65, 4099, 150 * 131, 4096 * 256 * 16 + 4099])
def test_label_confusion_equals_bincount(n, C):
    from wesup_amd import ops
    rs = np.random.RandomState(n % 65521 + C)
    S, G = rs.randint(0, C, n).astype(np.uint8), rs.randint(0, C, n).astype(np.uint8)
    want = np.bincount(G.astype(np.int64) * C + S, minlength=C * C).reshape(C, C)
    S_d, G_d = _d(S), _d(G)
    conf = torch.full((C, C), -7, dtype=torch.int64, device=DEV)               # a dirty buffer: zeroed by the entry
    status = torch.full((1,), 5, dtype=torch.int32, device=DEV)
    got, st = ops.label_confusion(S_d, G_d, C, out=conf, status=status)
    assert got is conf and st is status and int(status) == 0
    assert np.array_equal(conf.cpu().numpy(), want) and int(conf.sum()) == n
    ops.label_confusion(S_d, G_d, C, out=conf, status=status)                  # a second call starts from zero
    assert np.array_equal(conf.cpu().numpy(), want)
    if n > 1:                                                                  # maps that do not start on a 16-byte boundary
        got, st = ops.label_confusion(S_d[1:], G_d[1:], C)
        assert np.array_equal(got.cpu().numpy(), np.bincount(G[1:].astype(np.int64) * C + S[1:], minlength=C * C).reshape(C, C))
        assert int(st) == 0
    bad = S.copy()
    bad[n // 2] = C                                                            # a byte >= C: not counted, the status is set
    got, st = ops.label_confusion(_d(bad), G_d, C, out=conf, status=status)
    assert int(st) != 0 and int(conf.sum()) == n - 1
    lost = want.copy()
    lost[G[n // 2], S[n // 2]] -= 1
    assert np.array_equal(conf.cpu().numpy(), lost)
    bad_g = G.copy()
    bad_g[0] = 255
    got, st = ops.label_confusion(S_d, _d(bad_g), C)
    assert int(st) != 0 and int(got.sum()) == n - 1


# ---------------------------------------------------------------------------------------------------- 6. class-count range
def test_class_count_outside_the_range_is_invalid():
    from wesup_amd import _lib
    lib = _lib.load()
    p = lambda t: ctypes.c_void_p(t.data_ptr())
    f = torch.zeros(64 * 64 * 17, device=DEV)
    u8 = torch.zeros(64 * 64, dtype=torch.uint8, device=DEV)
    i32 = torch.zeros(4, dtype=torch.int32, device=DEV)
    i64 = torch.zeros(17 * 17, dtype=torch.int64, device=DEV)
    for C in (1, 17):
        for votes in (0, 1):
            assert lib.wesup_window_merge_classes(p(f), p(i32), p(i32), p(u8), p(i32), 8, 8, C, 1, 1, 8, votes, None) == -1
        assert lib.wesup_planes_resize_acc(p(f), p(f), 4, 4, 8, 8, C, 1.0, 0, None) == -1
        assert lib.wesup_class_argmax_u8(p(f), p(u8), 64, C, None) == -1
        for mode in (0, 1):
            assert lib.wesup_patch_scatter_classes_u8(p(f), p(u8), p(i32), 8, 8, 4, 4, 4, C, mode, 0, 1, None) == -1
        assert lib.wesup_label_confusion(p(u8), p(u8), p(i64), p(i32), 64, C, None) == -1
    torch.cuda.synchronize()
    assert int(u8.sum()) == 0 and int(i64.sum()) == 0                          # nothing was launched


# =================================================================================================== end to end
def _image(seed, H, W):
    from wesup_amd import synth
    return np.ascontiguousarray((synth.synth_image(seed, H, W).transpose(1, 2, 0) * 255).astype(np.uint8))


def _weights3():
    """oracle.make_weights(3, feat_scale=1.0) with the three-row classifier of tests/test_multiclass_gpu.py::weights_c."""
    from oracle import wesup_oracle as orc
    w = orc.make_weights(WEIGHT_SEED, feat_scale=FEAT_SCALE)
    rs = np.random.RandomState(1000 + WEIGHT_SEED)
    w['classifier.0.weight'] = (rs.randn(C3, 32) * np.sqrt(1.0 / 32)).astype(np.float32)
    w['classifier.0.bias'] = (rs.randn(C3) * 0.05).astype(np.float32)
    return w


def _shifted(weights, probs):
    """The weights with bias c lowered by the median over the rows of ``probs`` (n, C) of log(p_c / p_0) = z_c - z_0."""
    q = np.clip(np.asarray(probs, dtype=np.float64).reshape(-1, C3), 1e-300, None)
    shift = np.median(np.log(q) - np.log(q[:, :1]), axis=0)
    w = dict(weights)
    w['classifier.0.bias'] = (weights['classifier.0.bias'].astype(np.float64) - shift).astype(np.float32)
    return w, shift


def _load(model, weights):
    model.load_state_dict({k: torch.from_numpy(v) for k, v in weights.items()})
    model.eval()


def _shares(cls_map):
    return [float((np.asarray(cls_map) == c).mean()) for c in range(C3)]


def _assert_not_vacuous(name, cls_map):
    shares = _shares(cls_map)
    print(f'{name}: class shares of the batch-1 map {", ".join(f"{s:.3f}" for s in shares)}')
    assert min(shares) >= MIN_CLASS_SHARE, (name, shares)


def _compare_outside_ambiguous(name, got, single, amb):
    differ = got != single
    print(f'{name}: {int(differ.sum())} pixels differ from the batch-1 map, {int((differ & ~amb).sum())} of them outside ambiguous pixels')
    assert got.shape == single.shape and got.dtype == np.uint8
    assert np.array_equal(got[~amb], single[~amb]), (name, int((differ & ~amb).sum()))


def _assert_few_ambiguous(name, amb):
    share = float(amb.mean())
    print(f'{name}: ambiguous pixels {share:.5f} of the image')
    assert share <= MAX_AMBIGUOUS_SHARE, (name, share)


def _top_two_gap(p):
    top = torch.topk(torch.as_tensor(p), 2, dim=-1).values
    return (top[..., 0] - top[..., 1]).cpu().numpy()


def _trainer3():
    """The three-class superpixel trainer (sp_area 64), biases shifted by the medians over the superpixels of window 0 of the
    150 x 333 image."""
    from wesup_amd import infer_tile as T
    from wesup_amd.models import initialize_trainer
    trainer = initialize_trainer('wesup', device=DEV, n_classes=C3, sp_area=64)
    _load(trainer.model, _weights3())
    window = T.divide_image_to_patches(_image(IMAGE_SEED, 150, 333), 64)[0]
    with torch.no_grad():
        inp, _ = trainer.preprocess(T._to_tensor(window, DEV))
        trainer.model(inp)
        n = int(trainer.model._last_meta.n_sp[0])                              # (model.sp_pred without its padding rows)
        probs = trainer.model._padded[1][0, :n].detach().cpu().numpy()
    weights, shift = _shifted(_weights3(), probs)
    print(f'superpixel model: {len(probs)} superpixels in window 0, bias shifts {shift.tolist()}')
    _load(trainer.model, weights)
    trainer.shifted_weights = weights
    return trainer


@pytest.fixture(scope='module')
def trainer3():
    return _trainer3()


def _pixel_model(x0):
    """The three-class pixel-wise model, biases shifted by the medians over the pixels of the network input ``x0`` (1,3,h,w)."""
    from wesup_amd.models.wesup import WESUPPixelInference
    model = WESUPPixelInference(n_classes=C3).to(DEV)
    _load(model, _weights3())
    probs = model(x0).cpu().numpy()
    weights, shift = _shifted(_weights3(), probs)
    print(f'pixel model: bias shifts {shift.tolist()}')
    _load(model, weights)
    model.shifted_weights = weights
    return model


def _pixel3():
    """The pixel-wise model whose shifts come from window 0 of the 150 x 333 image."""
    from wesup_amd import infer_tile as T
    return _pixel_model(T._to_tensor(T.divide_image_to_patches(_image(IMAGE_SEED, 150, 333), 64)[0], DEV))


@pytest.fixture(scope='module')
def pixel3():
    return _pixel3()


def _sp_window_run(trainer, x):
    """One input through the superpixel model: (painted class map (h,w) fp32, top-two gap of every pixel's superpixel (h,w))."""
    with torch.no_grad():
        inp, _ = trainer.preprocess(x)
        pred = trainer.model(inp)[0].clone()
        sp = trainer.model._padded[1][0]                                       # (Kmax, C): model.sp_pred with its padding rows
        rows = trainer.model._last_meta.new_row[0].long()
        top = torch.topk(sp, 2, dim=-1).values
        gap = (top[:, 0] - top[:, 1])[rows].view(pred.shape)
    return pred.cpu().numpy(), gap.cpu().numpy()


# ----------------------------------------------------------------------------------------- 7. window inference, superpixels
def test_superpixel_window_paths(trainer3):
    from wesup_amd import infer_tile as T
    H, W, p = 150, 333, 64
    img = _image(IMAGE_SEED, H, W)
    single = T.predict_array_classes(trainer3, img, p, device=DEV)
    runs = [_sp_window_run(trainer3, T._to_tensor(patch, DEV)) for patch in T.divide_image_to_patches(img, p)]
    assert len(runs) == 18
    assert single.shape == (H, W) and single.dtype == np.uint8
    assert np.array_equal(single, T.combine_patches_to_classes(np.stack([r[0] for r in runs]), H, W, C3, votes=True))
    _assert_not_vacuous('superpixel windows 150x333', single)
    near = np.stack([r[1] < AMBIGUOUS for r in runs]).astype(np.float64)
    amb = T.combine_patches_to_image(near, H, W) > 0
    _assert_few_ambiguous('superpixel windows 150x333', amb)
    assert np.array_equal(T.predict_array_classes_batched(trainer3, img, p, batch=1, device=DEV), single)
    for batch in (2, 4):                                                       # 18 windows: batch 4 has a ragged tail
        got = T.predict_array_classes_batched(trainer3, img, p, batch=batch, device=DEV)
        _compare_outside_ambiguous(f'superpixel windows, batch {batch}', got, single, amb)
    again = T.predict_array_classes_batched(trainer3, img, p, batch=4, device=DEV)
    assert np.array_equal(again, got)                                          # run to run


# ------------------------------------------------------------------------------------------ 8. window inference, pixel-wise
def test_pixel_window_paths(pixel3):
    from wesup_amd import infer_tile as T
    H, W, p = 150, 333, 64
    img = _image(IMAGE_SEED, H, W)
    single = T.pixel_predict_array_classes(pixel3, img, p, device=DEV)
    with torch.no_grad():
        probs = np.stack([pixel3(T._to_tensor(patch, DEV)).cpu().numpy() for patch in T.divide_image_to_patches(img, p)])
    merged = T.combine_patches_to_image(probs, H, W)                           # the host composition: merge, then argmax
    assert single.dtype == np.uint8 and np.array_equal(single, merged.argmax(axis=-1))
    _assert_not_vacuous('pixel windows 150x333', single)
    amb = _top_two_gap(merged) < AMBIGUOUS
    _assert_few_ambiguous('pixel windows 150x333', amb)
    assert np.array_equal(T.pixel_predict_array_classes_batched(pixel3, img, p, batch=1, device=DEV), single)
    for batch in (2, 4):
        got = T.pixel_predict_array_classes_batched(pixel3, img, p, batch=batch, device=DEV)
        _compare_outside_ambiguous(f'pixel windows, batch {batch}', got, single, amb)
    again = T.pixel_predict_array_classes_batched(pixel3, img, p, batch=4, device=DEV)
    assert np.array_equal(again, got)


# ------------------------------------------------------------------------------------------- 9. whole image, several scales
@pytest.mark.parametrize('full_maps', [False, True])
def test_multi_scale_pixel_classes_equal_the_composition(pixel3, full_maps):
    from wesup_amd import ops
    from wesup_amd import pixel_infer as PI
    H, W, scales = 80, 112, (0.5, 0.75, 1.0)
    img = _image(IMAGE_SEED, H, W)
    got = PI.pixel_predict_classes(pixel3, img, scales, device=DEV, full_maps=full_maps)
    assert got.shape == (H, W) and got.dtype == np.uint8
    img_d = _d(img)
    mean = torch.full((C3, H, W), float('nan'), device=DEV)
    for i, scale in enumerate(scales):                                         # the two-class driver's steps, once per class
        h, w = PI.target_size(H, W, scale)
        x = ops.image_resize_u8(img_d, h, w)
        pred = (pixel3(x) if full_maps else pixel3.forward_per_resolution(x)[0]).clone()
        for c in range(C3):
            ops.plane_resize_acc(pred[..., c], mean[c], alpha=1.0 / len(scales), accumulate=i > 0)
    mean = mean.permute(1, 2, 0).cpu().numpy()
    assert np.array_equal(got, mean.argmax(axis=-1))
    _assert_not_vacuous(f'multi-scale 80x112 full_maps={full_maps}', got)
    assert np.array_equal(PI.pixel_predict_classes(pixel3, img, scales, device=DEV, full_maps=full_maps), got)


# ----------------------------------------------------------------------------------------------------- 10. whole slides
def test_superpixel_slide_path(trainer3):
    from wesup_amd import ops
    from wesup_amd import slide as S
    H, W, p, size = 80, 112, 64, (48, 40)
    img = _image(IMAGE_SEED, H, W)
    img_d = _d(img)
    n_h, n_w = S.patch_grid(H, W, p)
    assert (n_h, n_w) == (2, 2)
    maps, gaps = [], []
    for k in range(n_h * n_w):                                                 # the witness: one patch at a time
        pred, gap = _sp_window_run(trainer3, ops.patch_gather_resize(img_d, p, *size, k, 1).clone())
        up = lambda a: F.interpolate(torch.from_numpy(a)[None, None], size=(p, p), mode='nearest')[0, 0].numpy()
        maps.append(up(pred))
        gaps.append(up(gap))
    witness = S.combine_single_array(np.stack(maps), (H, W)).astype(np.uint8)
    amb = S.combine_single_array(np.stack(gaps), (H, W)) < AMBIGUOUS
    _assert_not_vacuous('superpixel slide 80x112', witness)
    _assert_few_ambiguous('superpixel slide 80x112', amb)
    one = S.slide_predict(trainer3, img, p, size, batch=1, device=DEV)
    assert one.shape == (H, W) and one.dtype == np.uint8 and np.array_equal(one, witness)
    for batch in (2, 4):
        got = S.slide_predict(trainer3, img, p, size, batch=batch, device=DEV)
        _compare_outside_ambiguous(f'superpixel slide, batch {batch}', got, witness, amb)
    kept = S.slide_predict(trainer3, img_d, p, size, batch=4, device=DEV, keep_on_device=True)
    assert kept.is_cuda and kept.dtype == torch.uint8 and np.array_equal(kept.cpu().numpy(), got)


def test_pixel_slide_path():
    """The network sees the patches at scale 0.6, where the logits lie elsewhere than at scale 1 (with the shifts of window 0 of
    the 150 x 333 image class 2 covers 3 % of this map): the shifts are derived from patch 0 of this slide as the network sees it."""
    from wesup_amd import ops
    from wesup_amd import pixel_infer as PI
    from wesup_amd import slide as S
    H, W, p, scale = 80, 112, 64, 0.6
    img = _image(IMAGE_SEED, H, W)
    patches = S.split_patches_array(img, p)
    pixel3 = _pixel_model(ops.image_resize_u8(_d(patches[0]), *PI.target_size(p, p, scale)))
    maps = [PI.pixel_predict_classes(pixel3, patch, (scale,), device=DEV) for patch in patches]
    witness = S.combine_single_array(np.stack(maps), (H, W)).astype(np.uint8)
    gaps = []
    for patch in patches:                                                      # the probabilities behind the witness
        x = ops.image_resize_u8(_d(patch), *PI.target_size(p, p, scale))
        full = torch.empty(p, p, C3, device=DEV)
        ops.planes_resize_acc(pixel3.forward_per_resolution(x)[0].contiguous(), full)
        assert np.array_equal(ops.class_argmax_u8(full).cpu().numpy(), maps[len(gaps)])
        gaps.append(_top_two_gap(full))
    amb = S.combine_single_array(np.stack(gaps), (H, W)) < AMBIGUOUS
    _assert_not_vacuous('pixel slide 80x112', witness)
    _assert_few_ambiguous('pixel slide 80x112', amb)
    one = S.slide_pixel_predict(pixel3, img, p, scale, batch=1, device=DEV)
    assert one.shape == (H, W) and one.dtype == np.uint8 and np.array_equal(one, witness)
    for batch in (2, 4):
        got = S.slide_pixel_predict(pixel3, img, p, scale, batch=batch, device=DEV)
        _compare_outside_ambiguous(f'pixel slide, batch {batch}', got, witness, amb)
    assert np.array_equal(S.slide_pixel_predict(pixel3, img, p, scale, batch=4, device=DEV), got)


# ------------------------------------------------------------------------------------------------------------ 11. drivers
def test_drivers_write_and_score_index_pngs(tmp_path, trainer3, pixel3):
    from PIL import Image
    from wesup_amd import infer_tile as T
    from wesup_amd import slide as S
    root = tmp_path / 'val'
    (root / 'images').mkdir(parents=True)
    (root / 'masks').mkdir()
    rs = np.random.RandomState(4)
    sizes = {'positive-a': (80, 112), 'negative-b': (70, 100)}
    for seed, (stem, (H, W)) in enumerate(sizes.items()):
        Image.fromarray(_image(IMAGE_SEED + seed, H, W)).save(root / 'images' / f'{stem}.jpg', quality=95)
        Image.fromarray(rs.randint(0, C3, (H, W)).astype(np.uint8)).save(root / 'masks' / f'{stem}.png')
    for pixel, weights, name in ((False, trainer3.shifted_weights, 'combined-results-for-ckpt.0001.pth'),
                                 (True, pixel3.shifted_weights, 'combined-results-pixel-for-ckpt.0001.pth')):
        ckpt = tmp_path / ('pixel' if pixel else 'sp') / 'checkpoints' / 'ckpt.0001.pth'
        ckpt.parent.mkdir(parents=True)
        torch.save({'epoch': 0, 'model_state_dict': {k: torch.from_numpy(v) for k, v in weights.items()}}, ckpt)
        lines = []
        got = S.main(root, ckpt, pixel=pixel, patch_size=64, device=DEV, batch=2, log=lambda *a: lines.append(' '.join(str(v) for v in a)))
        out = ckpt.parent.parent / name
        assert sorted(q.name for q in out.iterdir()) == ['negative-b.png', 'positive-a.png']
        scores = []
        for stem in sorted(sizes):
            written = np.asarray(Image.open(out / f'{stem}.png'))
            assert written.shape == sizes[stem] and written.dtype == np.uint8 and int(written.max()) < C3
            gt = np.asarray(Image.open(root / 'masks' / f'{stem}.png'))
            scores.append(S.slide_class_scores(written, gt, C3))                # the host, of what was written
            assert S.slide_class_scores(written, gt, C3, device=DEV) == scores[-1]
        want = {'all': (float(np.mean([s[0] for s in scores])), float(np.mean([s[1] for s in scores])))}
        assert got == want
        assert S.score_directory(out, root / 'masks', log=lambda *a: None, n_classes=C3) == want
        assert S.score_directory(out, root / 'masks', log=lambda *a: None, device=DEV, n_classes=C3) == want
        assert f'Accuracy: {want["all"][0]}' in lines and f'Dice: {want["all"][1]}' in lines
        assert S.main(root, ckpt, pixel=pixel, skip_infer=True, log=lambda *a: None) == want       # re-scores what is on disk
    # infer_tile --pixel --batch 2 on a JPEG and a PNG input: index PNGs under the inputs' stems, whatever the input's format
    data = tmp_path / 'tiles'
    (data / 'images').mkdir(parents=True)
    Image.fromarray(_image(IMAGE_SEED, 80, 112)).save(data / 'images' / 'one.jpg', quality=95)
    Image.fromarray(_image(IMAGE_SEED + 1, 64, 100)).save(data / 'images' / 'two.png')
    decoded = np.asarray(Image.open(data / 'images' / 'one.jpg').convert('RGB'))
    T.main([str(data), '--pixel', '--batch', '2', '--patch-size', '64', '--checkpoint', str(ckpt), '--output-dir',
            str(tmp_path / 'tiles-out'), '--device', DEV])
    assert sorted(q.name for q in (tmp_path / 'tiles-out').iterdir()) == ['one.png', 'two.png']
    with Image.open(tmp_path / 'tiles-out' / 'one.png') as im:
        assert im.format == 'PNG'
        first = np.asarray(im)
    assert first.shape == (80, 112) and first.dtype == np.uint8 and int(first.max()) < C3
    assert np.array_equal(first, T.pixel_predict_array_classes_batched(pixel3, decoded, 64, batch=2, device=DEV))      # the indices round-trip
    # and the superpixel tool with the three-class checkpoint of the trainer
    sp_ckpt = tmp_path / 'sp' / 'checkpoints' / 'ckpt.0001.pth'
    T.main([str(data), '--batch', '2', '--patch-size', '64', '--checkpoint', str(sp_ckpt), '--output-dir', str(tmp_path / 'tiles-sp'),
            '--device', DEV])
    assert sorted(q.name for q in (tmp_path / 'tiles-sp').iterdir()) == ['one.png', 'two.png']
    second = np.asarray(Image.open(tmp_path / 'tiles-sp' / 'two.png'))
    assert second.shape == (64, 100) and second.dtype == np.uint8 and int(second.max()) < C3


# -------------------------------------------------------------------------------------------- 12. two classes are untouched
def test_two_class_paths_call_none_of_the_new_entries(monkeypatch):
    from oracle import wesup_oracle as orc
    from wesup_amd import _lib
    from wesup_amd import infer_tile as T
    from wesup_amd import pixel_infer as PI
    from wesup_amd import slide as S
    from wesup_amd.models import initialize_trainer
    from wesup_amd.models.wesup import WESUPPixelInference
    weights = orc.make_weights(WEIGHT_SEED, feat_scale=FEAT_SCALE)
    trainer = initialize_trainer('wesup', device=DEV, sp_area=64)
    _load(trainer.model, weights)
    model = WESUPPixelInference().to(DEV)
    _load(model, weights)
    names, real = [], _lib.call

    def recording(name, *args):
        names.append(name)
        return real(name, *args)
    monkeypatch.setattr(_lib, 'call', recording)
    img = _image(IMAGE_SEED, 80, 112)
    a = T.predict_array_batched(trainer, img, 64, batch=2, device=DEV)
    b = T.pixel_predict_array_batched(model, img, 64, batch=2, device=DEV)
    c = PI.pixel_predict(model, img, (0.5, 1.0), device=DEV)
    d = S.slide_predict(trainer, img, 64, (48, 40), batch=2, device=DEV)
    e = S.slide_pixel_predict(model, img, 64, 0.6, batch=2, device=DEV)
    assert a.dtype == np.float64 and b.dtype == np.float64 and c.dtype == np.float32
    assert set(np.unique(d)) <= {0, 255} and set(np.unique(e)) <= {0, 255}
    assert 'wesup_window_merge' in names and 'wesup_plane_resize_acc' in names and 'wesup_patch_scatter_u8' in names
    assert not set(names) & set(ENTRIES), sorted(set(names) & set(ENTRIES))


# -------------------------------------------------------------------- 13. the launch sequence around the network is the recorded one
# the entries of tiles.hip, pixel.hip, slide.hip and classmap.hip, and the device copy that keeps a pass
INFERENCE_ENTRIES = ['wesup_window_gather', 'wesup_window_merge', 'wesup_image_resize_u8', 'wesup_plane_resize_acc',
                     'wesup_pixel_gather_fwd', 'wesup_patch_gather_resize', 'wesup_patch_scatter_u8', 'wesup_mask_scores',
                     'wesup_copy'] + ENTRIES
INFERENCE_CALLS = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'inference_calls.json')


def _inference_calls(trainer3, pixel3):
    """driver -> the ordered names of its ``_lib.call``s among INFERENCE_ENTRIES, for the nine device-resident drivers on test 12's
    image, patch, batch, input size and scales (tools/make_inference_calls_golden.py writes them to INFERENCE_CALLS)."""
    from oracle import wesup_oracle as orc
    from wesup_amd import _lib
    from wesup_amd import infer_tile as T
    from wesup_amd import pixel_infer as PI
    from wesup_amd import slide as S
    from wesup_amd.models import initialize_trainer
    from wesup_amd.models.wesup import WESUPPixelInference
    weights = orc.make_weights(WEIGHT_SEED, feat_scale=FEAT_SCALE)
    trainer = initialize_trainer('wesup', device=DEV, sp_area=64)
    _load(trainer.model, weights)
    model = WESUPPixelInference().to(DEV)
    _load(model, weights)
    img = _image(IMAGE_SEED, 80, 112)
    drivers = {
        'predict_array_batched': lambda: T.predict_array_batched(trainer, img, 64, batch=2, device=DEV),
        'pixel_predict_array_batched': lambda: T.pixel_predict_array_batched(model, img, 64, batch=2, device=DEV),
        'predict_array_classes_batched': lambda: T.predict_array_classes_batched(trainer3, img, 64, batch=2, device=DEV),
        'pixel_predict_array_classes_batched': lambda: T.pixel_predict_array_classes_batched(pixel3, img, 64, batch=2, device=DEV),
        'pixel_predict': lambda: PI.pixel_predict(model, img, (0.5, 1.0), device=DEV),
        'pixel_predict_classes': lambda: PI.pixel_predict_classes(pixel3, img, (0.5, 1.0), device=DEV),
        'slide_predict, C = 2': lambda: S.slide_predict(trainer, img, 64, (48, 40), batch=2, device=DEV),
        'slide_predict, C = 3': lambda: S.slide_predict(trainer3, img, 64, (48, 40), batch=2, device=DEV),
        'slide_pixel_predict': lambda: S.slide_pixel_predict(model, img, 64, 0.6, batch=2, device=DEV),
    }
    names, real = [], _lib.call

    def recording(name, *args):
        names.append(name)
        return real(name, *args)
    calls = {}
    _lib.call = recording
    try:
        for driver, run in drivers.items():
            del names[:]
            run()
            calls[driver] = [n for n in names if n in INFERENCE_ENTRIES]
    finally:
        _lib.call = real
    return calls


def test_inference_launch_sequences_are_the_recorded_ones(trainer3, pixel3):
    import json
    with open(INFERENCE_CALLS) as f:
        want = json.load(f)
    got = _inference_calls(trainer3, pixel3)
    assert sorted(got) == sorted(want) and len(got) == 9
    for driver, names in got.items():
        assert names and names == want[driver], (driver, names, want[driver])
