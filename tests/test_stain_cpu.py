"""Stain normalisation without a GPU: the restatement (tests/_stainref.py) against numpy's own functions and against itself in
float32, the host path of wesup_amd.stain against the restatement, the identity, degenerate images, the argument checks of the
entries through ctypes, the prefetcher's random streams and the tools' flags."""
import contextlib
import ctypes
import os

import numpy as np
import pytest
import torch

import _staincases as C
import _stainref as R
from _tol import within

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _img(shape, vectors=C.VEC_A):
    return C.he_image(shape[0] * shape[1], shape[0], shape[1], vectors)


# ---------------------------------------------------------------- the restatement
def test_percentile_and_covariance_restate_numpys():
    rs = np.random.RandomState(0)
    for n in (1, 2, 21, 100, 101, 1320):
        a = rs.standard_normal(n)
        for q in (0.0, 1.0, 37.0, 99.0, 100.0):
            assert abs(R.percentile(a, q) - np.percentile(a, q)) <= 1e-13 * max(1.0, np.abs(a).max()), (n, q)
    od = R.od_table()[_img((33, 65)).reshape(-1, 3)]
    assert np.abs(R.cov_from_moments(R.moments(od)) - np.cov(od.T)).max() <= 1e-13
    assert R.ranks(1.0, 21) == (0, 1, pytest.approx(0.2)) and R.ranks(99.0, 2)[:2] == (0, 1) and R.ranks(50.0, 1) == (0, 0, 0.0)


@pytest.mark.parametrize('shape', C.SHAPES)
def test_fits_are_valid_and_float32_agrees(shape):
    """What single precision costs, recorded: HE and maxC, the grey level in front of the rounding, no output value differs."""
    img = _img(shape)
    f, g = R.fit(img), R.fit(img, dtype=np.float32)
    assert f['valid'] and g['valid'] and f['n_tissue'] == g['n_tissue'] >= R.MIN_TISSUE
    assert f['HE'][0, 0] > f['HE'][0, 1] and np.allclose(np.linalg.norm(f['HE'], axis=0), 1.0, atol=1e-12)
    assert np.allclose(f['pinv'] @ f['HE'], np.eye(2), atol=1e-12)
    case = f'{shape[0]}x{shape[1]}'
    assert within(case, 'stain restatement fp32 vs fp64 HE', np.abs(f['HE'] - g['HE']).max(), 2e-6)
    assert within(case, 'stain restatement fp32 vs fp64 maxC', np.abs(f['maxC'] - g['maxC']).max() / f['maxC'].max(), 2e-6)
    pre64 = R.apply_pre(img, f, R.target())
    pre32 = R.apply_pre(img, g, R.target(np.float32), dtype=np.float32)
    assert within(case, 'stain restatement fp32 vs fp64 grey level before rint', np.abs(pre64 - pre32).max(), 1e-3)
    assert np.array_equal(R.apply(img, f, R.target()), R.apply(img, g, R.target(np.float32), dtype=np.float32))


def test_seven_by_five_has_few_tissue_pixels():
    assert R.fit(_img((7, 5)))['n_tissue'] == 27                      # of 35: a fit barely over min_tissue = 16


def test_stride_samples_the_lattice():
    img = _img((33, 65))
    assert R.sample(img, 3).shape == (11 * 22, 3) and np.array_equal(R.sample(img, 3)[23], img[3, 3])
    f = R.fit(img, stride=3)
    assert f['valid'] and f['n_tissue'] == int(R.tissue_mask(R.od_table()[img[::3, ::3].reshape(-1, 3)]).sum())


# ---------------------------------------------------------------- the host path of the public surface
@pytest.mark.parametrize('shape', C.SHAPES)
def test_host_path_equals_the_restatement(shape):
    from wesup_amd import stain as S
    img = _img(shape)
    f = R.fit(img)
    blk = S.host_fit(img)
    assert np.array_equal(blk.astype(np.float32), R.to_block(f)) and np.abs(blk[0:6] - f['HE'].reshape(-1)).max() <= 1e-14
    norm = S.StainNormalizer(host=True)
    assert np.array_equal(norm.target_host.astype(np.float32), R.to_block(R.target()))
    assert np.array_equal(norm(img), R.normalize(img))
    assert np.array_equal(norm(np.stack([img, img]))[1], R.normalize(img))
    par = (1.07, -0.03, 0.94, 0.05)
    assert np.array_equal(S.stain_jitter(img, par, host=True), R.jitter(img, par))
    # a target fitted from an image
    other = _img(shape, C.VEC_B)
    assert np.array_equal(S.StainNormalizer(other, host=True)(img), R.normalize(img, R.fit(other)))


def test_host_identity_jitter_returns_random_images_bit_for_bit():
    from wesup_amd import stain as S
    for seed in (1, 2):
        img = C.random_u8(seed)
        assert np.array_equal(S.stain_jitter(img, (1.0, 0.0, 1.0, 0.0), host=True), img)
        f = R.fit(img)
        assert f['valid'] and np.array_equal(R.apply(img, f, f, keep_residual=1.0), img)


def test_normalisation_brings_two_stainings_together():
    from wesup_amd import stain as S
    a, b = C.he_image(5, 96, 80, C.VEC_A), C.he_image(5, 96, 80, C.VEC_B)
    norm = S.StainNormalizer(host=True)
    before = np.abs(a.astype(np.float64) - b).mean()
    after = np.abs(norm(a).astype(np.float64) - norm(b)).mean()
    within('96x80', 'stain normalisation: mean |a - b| after / before', after / before, 1.0)       # (recorded; the bar is "smaller")
    assert after < before


@pytest.mark.parametrize('name', ['white', 'single', 'few'])
def test_degenerate_images_have_no_fit_and_stay_as_they_are(name):
    from wesup_amd import stain as S
    img = C.degenerate()[name]
    f = R.fit(img)
    assert not f['valid'] and not S.host_fit(img)[15] and S.host_fit(img)[14] == f['n_tissue']
    assert (f['n_tissue'] < R.MIN_TISSUE) == (name != 'single')
    assert np.array_equal(S.StainNormalizer(host=True)(img), img)
    assert np.array_equal(S.stain_jitter(img, (1.2, 0.1, 0.8, -0.1), host=True), img)
    with pytest.raises(ValueError):
        S.StainNormalizer(img, host=True)                               # no target to be had from it


def test_default_target():
    from wesup_amd import stain as S
    t = S.default_target()
    assert t.shape == (16,) and t[15] == 1 and np.array_equal(t[0:6].reshape(3, 2), R.TARGET_HE) and np.array_equal(t[12:14], R.TARGET_MAXC)
    assert np.allclose(t[6:12].reshape(2, 3), np.linalg.pinv(R.TARGET_HE), atol=1e-12)
    assert (S.IO, S.ALPHA, S.BETA, S.MIN_TISSUE) == (R.IO, R.ALPHA, R.BETA, R.MIN_TISSUE) == (240.0, 1.0, 0.15, 16)


# ---------------------------------------------------------------- the entries through ctypes
def test_entries_refuse_bad_arguments_on_the_host():
    from wesup_amd import _lib
    h = _lib.load()
    assert h.wesup_abi_version() == 6
    hdr = open(os.path.join(ROOT, 'include', 'wesup_hip.h')).read()
    for name, val in (('WESUP_STAIN_BLOCK', _lib.STAIN_BLOCK), ('WESUP_SELECT_BLOCK', _lib.SELECT_BLOCK),
                      ('WESUP_SELECT_MAX_BLOCKS', _lib.SELECT_MAX_BLOCKS), ('WESUP_SELECT_MAX_RANKS', _lib.SELECT_MAX_RANKS)):
        assert f'#define {name} {val}\n' in hdr
    one = ctypes.c_void_p(256)                                          # non-null, never dereferenced: every call is refused first
    sel = h.wesup_select_f32_workspace_bytes
    assert sel(0) == 0 and sel(-1) == 0
    for n in (1, 255, 256, 257, 65536, 65537, 1 << 24):
        blocks = min(_lib.SELECT_MAX_BLOCKS, -(-n // _lib.SELECT_BLOCK))
        assert sel(n) == 256 + blocks * _lib.SELECT_MAX_RANKS * 256 * 4
    assert h.wesup_select_f32(None, 8, None, 1, None, None, 0, None) == -1
    for n, r in ((0, 1), (-1, 1), (8, 0), (8, 5)):
        assert h.wesup_select_f32(one, n, one, r, one, one, 1 << 30, None) == -1
    assert h.wesup_select_f32(one, 8, one, 2, one, one, sel(8) - 1, None) == -3

    fit, off = h.wesup_stain_fit_workspace_bytes, h.wesup_stain_fit_stage_offset
    for shape in ((0, 8, 8, 1), (1, 0, 8, 1), (1, 8, 0, 1), (1, 8, 8, 0), (1, 8, 8, -1), (1, 4097, 4097, 1)):
        assert fit(*shape) == 0
    assert fit(1, 4097, 4097, 2) > 0                                    # 2049^2 samples: under 2^24

    def up(x):
        return -(-x // 256) * 256
    for B, H, W, s in ((1, 7, 5, 1), (3, 64, 48, 1), (1, 33, 65, 3), (4, 480, 480, 1)):
        n = -(-H // s) * -(-W // s)
        mb = min(256, -(-n // 256))
        sizes = [up(B * mb * 80), up(B * 80), B * 256, up(B * n * 4), up(B * 2 * n * 4), B * sel(n)]
        assert fit(B, H, W, s) == sum(sizes)
        assert [off(B, H, W, s, k) for k in range(4)] == [sum(sizes[:1]), sum(sizes[:2]), sum(sizes[:3]), sum(sizes[:4])]
    ok = dict(B=1, H=8, W=8, s=1, io=240.0, alpha=1.0, beta=0.15, mt=16)
    assert h.wesup_stain_fit(None, None, 1, 8, 8, 1, 240.0, 1.0, 0.15, 16, None, 0, None) == -1
    for bad in (dict(B=0), dict(H=0), dict(W=-1), dict(s=0), dict(io=1.0), dict(io=float('nan')), dict(alpha=-1.0), dict(alpha=51.0),
                dict(beta=-0.1), dict(mt=1)):
        a = dict(ok, **bad)
        assert h.wesup_stain_fit(one, one, a['B'], a['H'], a['W'], a['s'], a['io'], a['alpha'], a['beta'], a['mt'], one, 1 << 30,
                                 None) == -1, bad
    assert h.wesup_stain_fit(one, one, 1, 8, 8, 1, 240.0, 1.0, 0.15, 16, one, fit(1, 8, 8, 1) - 1, None) == -3

    assert h.wesup_stain_apply(None, None, None, None, 0, None, 0.0, 1, 8, 8, 240.0, None) == -1
    far = ctypes.c_void_p(1 << 20)
    for bad in (dict(B=0), dict(H=0), dict(W=0), dict(ds=8), dict(io=0.5), dict(keep=float('nan'))):
        a = dict(dict(B=1, H=8, W=8, ds=0, io=240.0, keep=0.0), **bad)
        assert h.wesup_stain_apply(one, far, one, one, a['ds'], None, a['keep'], a['B'], a['H'], a['W'], a['io'], None) == -1, bad
    assert h.wesup_stain_apply(one, ctypes.c_void_p(256 + 3), one, one, 0, None, 0.0, 1, 8, 8, 240.0, None) == -1     # overlapping, not in place


def test_ops_refuse_before_any_device_work():
    from wesup_amd import _lib, ops
    assert ops.stain_stride(480, 480) == 1 and ops.stain_stride(4096, 4096) == 1 and ops.stain_stride(8192, 8192) == 2
    assert ops.stain_stride(100000, 80000) == 22 and -(-100000 // 22) * -(-80000 // 22) <= 1 << 24 < -(-100000 // 21) * -(-80000 // 21)
    img = torch.zeros(8, 8, 3, dtype=torch.uint8)
    for call in (lambda: ops.stain_fit(img), lambda: ops.stain_apply(img, torch.zeros(1, 16), torch.zeros(16)),
                 lambda: ops.select_f32(torch.zeros(4), torch.zeros(1, dtype=torch.int64))):
        with pytest.raises(_lib.WesupHipError):                           # host tensors: there is no CPU path behind ops
            call()


# ---------------------------------------------------------------- the prefetcher's random streams
class _Recorder:
    def __init__(self):
        self.calls = []

    def __call__(self, img, out=None):
        self.calls.append(tuple(img.shape))
        return img


def _staged_states(monkeypatch, **kw):
    """Stages two synthetic batches with every device call replaced; returns the state of ``rs`` after each and the prefetcher."""
    from wesup_amd import ops, stain as S
    from wesup_amd.utils import data as D
    monkeypatch.setattr(torch.cuda, 'Stream', lambda device=None: None)
    monkeypatch.setattr(torch.cuda, 'stream', lambda s: contextlib.nullcontext())
    monkeypatch.setattr(torch.cuda, 'Event', lambda: type('E', (), {'record': lambda self: None})())
    monkeypatch.setattr(torch.Tensor, 'pin_memory', lambda self: self)
    monkeypatch.setattr(ops, 'appearance', lambda img, par: img)
    monkeypatch.setattr(ops, 'augment', lambda img, mask, par, C, elastic=None: (
        torch.zeros(img.shape[0], 3, *img.shape[1:3]), None if mask is None else torch.zeros(img.shape[0], C, *img.shape[1:3], dtype=torch.uint8)))
    jit = []
    monkeypatch.setattr(S, 'stain_jitter', lambda img, par, out=None: (jit.append(par.numpy().copy()), img)[1])
    ds = C.RawItems(4, 48, 40)
    loader = torch.utils.data.DataLoader(ds, batch_size=2)
    pf = D.DevicePrefetcher(loader, 'cpu', train=True, with_points=True, has_masks=True, seed=3, **kw)
    states = []
    for raw in loader:
        pf._stage(raw)
        states.append(pf.rs.get_state())
    return states, pf, jit


def test_prefetcher_draws_the_same_stream_with_the_feature_on_and_off(monkeypatch):
    from wesup_amd.utils import data as D
    off, pf_off, jit_off = _staged_states(monkeypatch)
    rec = _Recorder()
    on, pf_on, jit_on = _staged_states(monkeypatch, stain=rec, stain_jitter=0.1)
    assert len(off) == len(on) == 2
    for a, b in zip(off, on):
        assert a[0] == b[0] and np.array_equal(a[1], b[1]) and a[2:] == b[2:]
    assert jit_off == [] and pf_off.stain is None and pf_off.stain_jitter == 0.0
    assert rec.calls == [(2, 48, 40, 3)] * 2
    gen = D.stain_jitter_generator(3)
    for rows in jit_on:
        want = D.sample_stain_jitter(gen, 0.1, 2)
        assert rows.dtype == np.float32 and np.array_equal(rows, want)
        assert (np.abs(want[:, [0, 2]] - 1) <= 0.1).all() and (np.abs(want[:, [1, 3]]) <= 0.1).all()
    # the second generator is the stated one: RandomState(seed + 0x57A1), a then b for H, then for E
    g = np.random.RandomState(3 + 0x57A1)
    first = [g.uniform(0.9, 1.1), g.uniform(-0.1, 0.1), g.uniform(0.9, 1.1), g.uniform(-0.1, 0.1)]
    assert np.array_equal(jit_on[0][0], np.array(first, dtype=np.float32))
    with pytest.raises(ValueError):
        _staged_states(monkeypatch, stain_jitter=-0.5)


# ---------------------------------------------------------------- the tools' flags
def test_tools_accept_the_flag_and_default_it_to_off():
    from wesup_amd import infer, infer_tile, pixel_infer, slide, stain as S, train
    parsers = [(infer.parse_args, ['d']), (infer_tile.parse_args, ['d']), (infer_tile.parse_args, ['d', '--batch', '4', '--pixel']),
               (pixel_infer.parse_args, ['d', '-c', 'r/checkpoints/c.pth']), (slide.parse_args, ['d', '-c', 'r/checkpoints/c.pth'])]
    for parse, argv in parsers:
        assert parse(argv).stain_normalize is None
        assert parse(argv + ['--stain-normalize']).stain_normalize is True
        assert parse(argv + ['--stain-normalize', 'ref.png']).stain_normalize == 'ref.png'
    assert train.parse_cli_kwargs([]) == {}
    assert train.parse_cli_kwargs(['--stain-normalize', '--stain-jitter', '0.1']) == {'stain_normalize': True, 'stain_jitter': 0.1}
    assert train.parse_cli_kwargs(['--stain-normalize', 'ref.png'])['stain_normalize'] == 'ref.png'
    assert S.make_normalizer(None, 'cpu') is None and S.make_normalizer(False, 'cpu') is None
    a = S.parse_args(['src', 'out'])
    assert (a.src_dir, a.out_dir, a.target, a.host) == ('src', 'out', None, False)
    a = S.parse_args(['src', 'out', '--target', 't.png', '--host'])
    assert (a.target, a.host) == ('t.png', True)


def test_program_writes_normalised_pngs_on_the_host_path(tmp_path):
    from PIL import Image
    from wesup_amd import stain as S
    src, out = tmp_path / 'src', tmp_path / 'out'
    src.mkdir()
    imgs = {'a': _img((33, 65)), 'b': _img((64, 48), C.VEC_B), 'glass': C.degenerate()['white']}
    for k, v in imgs.items():
        Image.fromarray(v).save(src / f'{k}.png')
    Image.fromarray(_img((96, 80), C.VEC_B)).save(tmp_path / 'target.png')
    (src / 'notes.txt').write_text('not an image')
    assert S.run(S.parse_args([str(src), str(out), '--host'])) == 3
    for k, v in imgs.items():
        assert np.array_equal(np.asarray(Image.open(out / f'{k}.png')), R.normalize(v))
    S.main([str(src), str(out), '--host', '--target', str(tmp_path / 'target.png')])
    assert np.array_equal(np.asarray(Image.open(out / 'a.png')), R.normalize(imgs['a'], R.fit(_img((96, 80), C.VEC_B))))
