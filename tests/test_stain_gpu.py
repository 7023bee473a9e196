"""Stain normalisation and stain jitter on the device (csrc/stain.hip) against the fp64 restatement (tests/_stainref.py).

Every stage of a fit is held to the device's own result of the stage before, so that one stage's rounding is not charged to the
next: the bar of a stage is four times the error of the float32 restatement of that stage on the same input (the project's
convention for "the same thing in another order of operations"); counts and order statistics are exact.  The apply pass is held
to its own rule (``_check_apply``)."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _staincases as C     # noqa: E402
import _stainref as R       # noqa: E402
from _tol import within     # noqa: E402

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
U = 2.0 ** -24              # unit roundoff of float32
L = float(np.log(240.0))    # the largest OD of a channel
T32 = R.od_table(dtype=np.float32)          # the kernels' table: float64 log, rounded once


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def _batch(shape, B=1):
    H, W = shape
    return np.stack([C.he_image(H * W + b, H, W, C.VEC_B if b % 2 else C.VEC_A) for b in range(B)])


# ------------------------------------------------------------------------------------------------------------ 1. select
def _select_arrays(n):
    rs = np.random.RandomState(n)
    normal = rs.standard_normal(n).astype(np.float32)
    two = np.where(rs.rand(n) < 0.4, np.float32(-1.5), np.float32(2.25)).astype(np.float32)
    signs = rs.standard_normal(n).astype(np.float32)
    signs[rs.rand(n) < 0.2] = np.float32(0.0)
    signs[rs.rand(n) < 0.2] = np.float32(-0.0)                               # both zeros are in there
    tail = (rs.rand(n).astype(np.float32) * np.float32(2 * np.pi) - np.float32(np.pi))
    tail[rs.rand(n) < 0.3] = np.inf                                           # the "not tissue" key
    return {'normal': normal, 'equal': np.full(n, 0.37, np.float32), 'two values': two, 'signs and zeros': signs, 'inf tail': tail}


def _rank_sets(keys):
    n = len(keys)
    sets = [sorted({0, n - 1, n // 2})]
    srt = np.sort(keys)
    run = np.flatnonzero(srt[1:] == srt[:-1])                               # inside a run of duplicates
    if len(run):
        sets.append([int(run[0]), int(run[0]) + 1] + ([int(run[len(run) // 2])] if len(run) > 2 else []))
    nt = max(int(np.isfinite(keys).sum()), 1)                               # the four ranks of a fit at once
    lo, hi = R.ranks(1.0, nt), R.ranks(99.0, nt)
    sets.append([lo[0], lo[1], hi[0], hi[1]])
    return sets


@pytest.mark.parametrize('n', [1, 2, 255, 256, 257, 65537, 2 * 256 * 256 + 3, 2 * 4 * 256 * 256 + 3])
def test_select_is_np_sort_bit_for_bit(n):
    """The histogram kernel's grid is capped at 256 blocks of 256 threads and its main loop takes four keys per thread and trip,
    4 * 65536 keys per trip of the grid; what is left goes one key per thread and trip.  The last size is three more than two
    whole trips of the main loop; the one before it, three more than two trips of the remainder loop, never enters the main one."""
    from wesup_amd import _lib, ops
    assert (_lib.SELECT_BLOCK, _lib.SELECT_MAX_BLOCKS) == (256, 256)
    for name, keys in _select_arrays(n).items():
        srt = np.sort(keys)
        d_keys = _dev(keys)
        for ranks in _rank_sets(keys):
            got = ops.select_f32(d_keys, _dev(np.asarray(ranks, dtype=np.int64))).cpu().numpy()
            want = srt[ranks]
            same = (got.view(np.int32) == want.view(np.int32)) | ((got == 0) & (want == 0))      # (+-0 meet: by value)
            assert same.all(), (n, name, ranks, got, want)
    # a rank outside the array is taken to its end
    keys = _select_arrays(n)['normal']
    got = ops.select_f32(_dev(keys), _dev(np.array([-5, n + 7], dtype=np.int64))).cpu().numpy()
    assert got[0] == keys.min() and got[1] == keys.max()


# ------------------------------------------------------------------------------------------------------------ 2 - 4. the fit
# shape, B, stride.  The last: 529 920 samples -- past the 4 * 65536 of one trip of the moments kernel's four-in-flight loop, 256
# partial rows for the 64 lanes of the fold, and past the 2048 * 256 threads of the key and concentration kernels' capped grids
FIT_CASES = [((7, 5), 1, 1), ((33, 65), 1, 1), ((64, 48), 3, 1), ((33, 65), 1, 3), ((96, 80), 2, 2), ((736, 720), 1, 1)]


def _fit(imgs, stride):
    from wesup_amd import ops
    blocks, st = ops.stain_fit(_dev(imgs), stride=stride, return_stages=True)
    return blocks.cpu().numpy(), {k: v.cpu().numpy().copy() for k, v in st.items()}


def _rel(a, b):
    return float(np.abs(np.asarray(a, dtype=np.float64) - b).max() / np.abs(b).max())


@pytest.mark.parametrize('shape,B,stride', FIT_CASES)
def test_fit_stage_by_stage(shape, B, stride):
    imgs = _batch(shape, B)
    blocks, st = _fit(imgs, stride)
    for b in range(B):
        case = f'{shape[0]}x{shape[1]} image {b} stride {stride}'
        px = R.sample(imgs[b], stride)
        od32 = T32[px]
        od = od32.astype(np.float64)                                        # the same table OD, in double
        tis = R.tissue_mask(od32)
        blk = R.from_block(blocks[b])
        assert blk['valid'] and blocks[b][14] == tis.sum() >= R.MIN_TISSUE
        # moments: another summation order of the same numbers; the count exact
        m64, m32 = R.moments(od[tis]), R.moments(od32[tis])
        assert st['moments'][b][0] == tis.sum()
        assert within(case, 'stain moments', _rel(st['moments'][b], m64), 4 * _rel(m32, m64), 'max |m - m64| / max |m64|')
        # eigenvectors of the device's moments
        mom = st['moments'][b]
        v64 = R.eigvecs(R.cov_from_moments(mom))
        v32 = R.eigvecs(R.cov_from_moments(mom.astype(np.float32)))
        assert within(case, 'stain eigenvectors', np.abs(st['eig'][b] - v64).max(), 4 * np.abs(v32 - v64).max())
        # phi of the device's eigenvectors; +inf exactly where a sample is not tissue
        v = st['eig'][b]
        phi = st['phi'][b]
        assert phi.shape == (len(px),) and np.array_equal(np.isposinf(phi), ~tis) and np.isfinite(phi[tis]).all()
        p64, p32 = R.phi(od[tis], v), R.phi(od32[tis], v.astype(np.float32))
        assert within(case, 'stain phi', np.abs(phi[tis] - p64).max(), 4 * np.abs(p32 - p64).max())
        # stain vectors from the device's keys, after the H / E ordering
        k64, k32 = phi[tis].astype(np.float64), phi[tis]
        he64 = R.stain_vectors(R.percentile(k64, 1.0), R.percentile(k64, 99.0), v)
        he32 = R.stain_vectors(R.percentile(k32, 1.0), R.percentile(k32, 99.0), v.astype(np.float32))
        assert within(case, 'stain vectors', np.abs(blk['HE'] - he64).max(), 4 * np.abs(he32 - he64).max())
        assert blk['HE'][0, 0] > blk['HE'][0, 1]
        # the pseudo-inverse of the block's vectors
        pv64, pv32 = R.pinv(blk['HE']), R.pinv(blk['HE'].astype(np.float32))
        assert within(case, 'stain pinv', np.abs(blk['pinv'] - pv64).max(), 4 * np.abs(pv32 - pv64).max())
        # concentrations of ALL samples with the block's pinv
        conc = st['conc'][b].T
        c64, c32 = R.concentrations(od, blk['pinv']), R.concentrations(od32, blk['pinv'].astype(np.float32))
        assert conc.shape == c64.shape
        assert within(case, 'stain concentrations', np.abs(conc - c64).max(), 4 * np.abs(c32 - c64).max())
        # maxC from the device's concentrations
        mx64 = np.array([R.percentile(conc[:, k].astype(np.float64), 99.0) for k in range(2)])
        mx32 = np.array([R.percentile(conc[:, k], 99.0) for k in range(2)])
        assert within(case, 'stain maxC', np.abs(blk['maxC'] - mx64).max(), 4 * np.abs(mx32 - mx64).max())


@pytest.mark.parametrize('shape,B,stride', FIT_CASES)
def test_fit_end_to_end(shape, B, stride):
    """The same image through the fp64 restatement alone (its own table, np.cov, eigh)."""
    imgs = _batch(shape, B)
    blocks, _ = _fit(imgs, stride)
    for b in range(B):
        case = f'{shape[0]}x{shape[1]} image {b} stride {stride}'
        f, g = R.fit(imgs[b], stride=stride), R.fit(imgs[b], stride=stride, dtype=np.float32)
        blk = R.from_block(blocks[b])
        assert f['valid'] and blk['valid'] and blk['n_tissue'] == f['n_tissue']
        assert within(case, 'stain fit end to end HE', np.abs(blk['HE'] - f['HE']).max(), 4 * np.abs(g['HE'] - f['HE']).max())
        assert within(case, 'stain fit end to end maxC', np.abs(blk['maxC'] - f['maxC']).max(), 4 * np.abs(g['maxC'] - f['maxC']).max())


def test_stride_three_samples_the_restatements_lattice():
    img = _batch((33, 65))
    blocks, st = _fit(img, 3)
    od32 = T32[img[0][::3, ::3].reshape(-1, 3)]
    assert st['phi'].shape == (1, 11 * 22) and np.array_equal(np.isposinf(st['phi'][0]), ~R.tissue_mask(od32))
    assert blocks[0][14] == R.fit(img[0], stride=3)['n_tissue']


# ------------------------------------------------------------------------------------------------------------ 5 - 7. apply
def apply_error_bound(src, dst, jitter, keep):
    """E: how far the kernel's float32 chain can be from the fp64 value in front of rint, in grey levels.

    u = 2^-24 per rounding, relative to the rounded quantity; every OD <= L = ln 240.  With A_k = L sum_c |pinv_kc| >= |c_k|:
      table entry + the 3-term dot (a multiply and two fmas)       e(c_k)  = 4 u A_k
      the scale (one division, one multiply) and fma(c, sa, b)      e(c'_k) = |sa_k| e(c_k) + 2 u |sa_k| A_k + u D_k,  D_k = |sa_k| A_k + |b_k|
      the 2-term dots (a multiply and an fma)                       e(dst)  = sum_k |HEd_ck| (2 u D_k + e(c'_k)),  e(fit) likewise with A_k, e(c_k)
      the residual (a subtraction) and fma(keep, r, dst)            e(r)    = u R + u L + e(fit),  R = L + |fit|;
                                                                    e(OD')  = u (|dst| + keep R) + keep e(r) + e(dst)
      expf within 1 ulp (2 u, the HIP math API's bound), fma(Io, e, -1) with Io e <= 256
                                                                    E       = 256 (e(OD') + 2 u) + 255 u"""
    ps, hs, hd = np.abs(src['pinv']), np.abs(src['HE']), np.abs(dst['HE'])
    j = np.abs(np.asarray(jitter, dtype=np.float64))
    sa = dst['maxC'] / src['maxC'] * j[[0, 2]]
    A = L * ps.sum(1)
    ec = 4 * U * A
    D = sa * A + j[[1, 3]]
    ed = sa * ec + 2 * U * sa * A + U * D
    edst = (hd @ (2 * U * D + ed)).max()
    fit = (hs @ A).max()
    efit = (hs @ (2 * U * A + ec)).max()
    Rm = L + fit
    er = U * Rm + U * L + efit
    eod = U * ((hd @ D).max() + keep * Rm) + keep * er + edst
    return 256 * (eod + 2 * U) + 255 * U


def _check_apply(case, got, img, src_block, dst_block, jitter=(1.0, 0.0, 1.0, 0.0), keep=0.0):
    """A device value may differ from rint of the fp64 value only where that value lies within E of a half-integer, and then by
    exactly one level.  The largest distance to a half-integer at a differing value is recorded."""
    src, dst = R.from_block(src_block), R.from_block(dst_block)
    if not (src['valid'] and dst['valid']):
        assert np.array_equal(got, img), case
        return 0
    pre = np.clip(R.apply_pre(img, src, dst, jitter, keep), 0, 255)
    want = np.rint(pre).astype(np.int64)
    differ = got.astype(np.int64) != want
    E = apply_error_bound(src, dst, jitter, keep)
    assert 0 < E < 0.05, E
    if differ.any():
        assert (np.abs(got.astype(np.int64) - want)[differ] == 1).all(), case
        dist = np.abs(pre[differ] - np.floor(pre[differ]) - 0.5)
        assert within(case, 'stain apply: distance to a half-integer where the device rounds the other way', dist.max(), E,
                      'grey levels; the bar is the float32 chain\'s error bound for the case\'s blocks'), (case, dist.max(), E)
    else:
        within(case, 'stain apply: distance to a half-integer where the device rounds the other way', 0.0, E)
    return int(differ.sum())


def _target_block():
    return R.to_block(R.target())


@pytest.mark.parametrize('shape,B', [((7, 5), 1), ((33, 65), 1), ((64, 48), 3)])
def test_normalisation_follows_the_rounding_rule(shape, B):
    from wesup_amd import ops
    imgs = _batch(shape, B)
    d_img = _dev(imgs)
    blocks = ops.stain_fit(d_img)
    tgt = _dev(_target_block())
    out = ops.stain_apply(d_img, blocks, tgt)
    got, blk = out.cpu().numpy(), blocks.cpu().numpy()
    assert torch.equal(d_img.cpu(), torch.from_numpy(imgs))                  # the input is left alone
    for b in range(B):
        _check_apply(f'normalise {shape[0]}x{shape[1]} image {b}', got[b], imgs[b], blk[b], _target_block())
    # in place equals out of place
    same = d_img.clone()
    assert ops.stain_apply(same, blocks, tgt, out=same).data_ptr() == same.data_ptr() and torch.equal(same, out)


def test_apply_past_one_trip_of_its_capped_grid():
    """1456 x 1448 = 2 108 288 pixels: more than the 2048 * 256 * 4 one trip of the dword path's capped grid takes, and four
    trips of the byte path's.  The dword path against the fp64 restatement under the rounding rule, the byte path (output at
    another phase of the dword grid) equal to it."""
    from wesup_amd import ops
    img = np.tile(C.he_image(7, 364, 362), (4, 4, 1))
    assert img.shape == (1456, 1448, 3) and img.shape[0] * img.shape[1] > 2048 * 256 * 4
    d_img = _dev(img)
    blocks = ops.stain_fit(d_img)
    tgt = _dev(_target_block())
    want = ops.stain_apply(d_img, blocks, tgt)
    assert want.data_ptr() % 4 == d_img.data_ptr() % 4 == 0
    _check_apply('1456x1448', want.cpu().numpy(), img, blocks.cpu().numpy()[0], _target_block())
    flat = torch.full((img.size + 8,), 77, dtype=torch.uint8, device=DEV)
    dst = flat[1:1 + img.size].view(1456, 1448, 3)
    ops.stain_apply(d_img, blocks, tgt, out=dst)
    assert torch.equal(dst, want) and flat[0] == 77 and (flat[1 + img.size:] == 77).all()


@pytest.mark.parametrize('offset', [1, 2, 3])
def test_vector_head_and_tail_at_an_odd_base(offset):
    """2 x 9 x 7: 189 bytes per image (no multiple of 4), the buffer a slice that starts ``offset`` bytes into an allocation, so
    the two images sit at different phases of the dword grid.  The same phase in and out takes the dword path with a scalar head
    and tail, a fresh (aligned) output the byte path; both equal the result on an aligned copy."""
    from wesup_amd import ops
    imgs = _batch((9, 7), 2)
    n = imgs.size
    aligned = _dev(imgs)
    blocks = ops.stain_fit(aligned)
    tgt = _dev(_target_block())
    want = ops.stain_apply(aligned, blocks, tgt)
    blk = blocks.cpu().numpy()
    for b in range(2):
        _check_apply(f'9x7 image {b}', want[b].cpu().numpy(), imgs[b], blk[b], _target_block())
    flat_in = torch.zeros(n + 8, dtype=torch.uint8, device=DEV)
    flat_out = torch.full((n + 8,), 77, dtype=torch.uint8, device=DEV)
    src = flat_in[offset:offset + n].view(2, 9, 7, 3)
    src.copy_(aligned)
    assert src.data_ptr() % 4 == offset
    assert torch.equal(ops.stain_fit(src), blocks)                             # the fit reads bytes: any base
    assert torch.equal(ops.stain_apply(src, blocks, tgt), want)                # other phase out: byte path
    dst = flat_out[offset:offset + n].view(2, 9, 7, 3)
    ops.stain_apply(src, blocks, tgt, out=dst)                                 # same phase: dword path
    assert torch.equal(dst, want)
    assert (flat_out[:offset] == 77).all() and (flat_out[offset + n:] == 77).all()      # nothing outside the images is written
    ops.stain_apply(src, blocks, tgt, out=src)
    assert torch.equal(src, want) and (flat_in[:offset] == 0).all() and (flat_in[offset + n:] == 0).all()


def test_batch_of_three_sources_one_invalid():
    """Three different source blocks, the middle one invalid (empty glass): a bitwise copy there, the rule elsewhere -- block
    stride and flag handling; then one destination block per image."""
    from wesup_amd import ops
    imgs = np.stack([C.he_image(1, 33, 65, C.VEC_A), C.degenerate()['white'], C.he_image(2, 33, 65, C.VEC_B)])
    d_img = _dev(imgs)
    blocks = ops.stain_fit(d_img)
    blk = blocks.cpu().numpy()
    assert blk[:, 15].tolist() == [1.0, 0.0, 1.0] and blk[1, 14] == 0 and (blk[1, :14] == 0).all()
    got = ops.stain_apply(d_img, blocks, _dev(_target_block())).cpu().numpy()
    assert np.array_equal(got[1], imgs[1])
    for b in (0, 2):
        _check_apply(f'three sources, image {b}', got[b], imgs[b], blk[b], _target_block())
    # one destination each: image 0 to image 2's stains, image 1 stays, image 2 to an invalid destination stays
    dst = np.stack([blk[2], blk[0], blk[1]])
    got = ops.stain_apply(d_img, blocks, _dev(dst)).cpu().numpy()
    _check_apply('three destinations, image 0', got[0], imgs[0], blk[0], dst[0])
    assert np.array_equal(got[1], imgs[1]) and np.array_equal(got[2], imgs[2])


def test_identity_jitter_returns_random_images_bit_for_bit():
    from wesup_amd import stain as S
    imgs = np.stack([C.random_u8(1), C.random_u8(2)])
    d_img = _dev(imgs)
    assert torch.equal(S.stain_jitter(d_img, (1.0, 0.0, 1.0, 0.0)), d_img)
    assert torch.equal(S.stain_jitter(d_img[0], torch.tensor([[1.0, 0.0, 1.0, 0.0]], device=DEV)), d_img[0])
    he = _dev(_batch((33, 65), 2))
    assert torch.equal(S.stain_jitter(he, (1.0, 0.0, 1.0, 0.0)), he)


def test_jitter_follows_the_rounding_rule():
    from wesup_amd import ops
    imgs = _batch((64, 48), 3)
    par = np.array([[1.08, -0.04, 0.93, 0.06], [0.9, 0.1, 1.1, -0.1], [1.0, 0.0, 1.0, 0.0]], dtype=np.float32)
    d_img = _dev(imgs)
    blocks = ops.stain_fit(d_img)
    got = ops.stain_apply(d_img, blocks, blocks, jitter=_dev(par), keep_residual=1.0).cpu().numpy()
    blk = blocks.cpu().numpy()
    moved = 0
    for b in range(3):
        _check_apply(f'jitter image {b}', got[b], imgs[b], blk[b], blk[b], jitter=par[b].astype(np.float64), keep=1.0)
        moved += int((got[b] != imgs[b]).sum())
    assert np.array_equal(got[2], imgs[2]) and moved > imgs[0].size                      # (the jitter does something)


# ------------------------------------------------------------------------------------------------------------ 8 - 9.
@pytest.mark.parametrize('name', ['white', 'single', 'few'])
def test_degenerate_images_are_invalid_and_copied(name):
    from wesup_amd import ops, stain as S
    img = C.degenerate()[name]
    d_img = _dev(img)
    blocks = ops.stain_fit(d_img)
    blk = blocks.cpu().numpy()[0]
    assert blk[15] == 0 and (blk[:14] == 0).all() and blk[14] == R.fit(img)['n_tissue']
    assert torch.equal(S.StainNormalizer(device=DEV)(d_img), d_img)
    assert torch.equal(S.stain_jitter(d_img, (1.2, 0.1, 0.8, -0.1)), d_img)


def test_two_runs_give_the_same_bits():
    from wesup_amd import ops
    d_img = _dev(_batch((64, 48), 3))
    tgt = _dev(_target_block())
    runs = []
    for _ in range(2):
        blocks, st = ops.stain_fit(d_img, return_stages=True)
        st = {k: v.clone() for k, v in st.items()}
        runs.append((blocks.clone(), st, ops.stain_apply(d_img, blocks, tgt)))
    (b0, s0, o0), (b1, s1, o1) = runs
    assert torch.equal(b0.view(torch.int32), b1.view(torch.int32)) and torch.equal(o0, o1)
    for k in s0:
        assert torch.equal(s0[k].view(torch.int64 if s0[k].dtype == torch.float64 else torch.int32),
                           s1[k].view(torch.int64 if s1[k].dtype == torch.float64 else torch.int32)), k


# ------------------------------------------------------------------------------------------------------------ 10. wiring
def test_normalizer_equals_ops_by_hand():
    from wesup_amd import ops, stain as S
    img = _batch((96, 80))[0]
    d_img = _dev(img)
    norm = S.StainNormalizer(device=DEV)
    assert norm.target.shape == (16,) and np.array_equal(norm.target.cpu().numpy(), _target_block())
    blocks = ops.stain_fit(d_img)
    assert torch.equal(norm.fit(d_img), blocks)
    want = ops.stain_apply(d_img, blocks, _dev(_target_block()))
    assert want.shape == (96, 80, 3) and torch.equal(norm(d_img), want)
    assert torch.equal(norm(d_img[None]), want[None])
    # a target fitted from an image, on the device and on the host: the same stains to float32
    other = C.he_image(9, 64, 48, C.VEC_B)
    fitted = S.StainNormalizer(other, device=DEV)
    assert np.abs(fitted.target_host - S.StainNormalizer(other, host=True).target_host)[:14].max() < 1e-5
    _check_apply('fitted target', fitted(d_img).cpu().numpy(), img, blocks.cpu().numpy()[0], fitted.target.cpu().numpy())
    # the device result against the host path of the same surface: the rounding rule again, so all but a few values agree
    host = S.StainNormalizer(host=True)(img)
    assert (host != want.cpu().numpy()).mean() < 0.01


def test_window_inference_with_the_normaliser_equals_normalising_first():
    from oracle import wesup_oracle as orc
    from wesup_amd import infer_tile as T, stain as S
    from wesup_amd.models import initialize_trainer
    trainer = initialize_trainer('wesup', device=DEV, sp_area=64)
    trainer.model.load_state_dict({k: torch.from_numpy(v) for k, v in orc.make_weights(3, feat_scale=1.0).items()})
    trainer.model.eval()
    img = C.he_image(4, 96, 80, C.VEC_B)
    norm = S.StainNormalizer(device=DEV)
    first = norm(_dev(img)).cpu().numpy()
    assert (first != img).mean() > 0.1
    want = T.predict_array_batched(trainer, first, 64, batch=2, device=DEV)
    got = T.predict_array_batched(trainer, img, 64, batch=2, device=DEV, stain=norm)
    assert got.shape == (96, 80) and np.array_equal(got, want)


def test_trainer_refuses_the_flags_where_nothing_would_apply_them():
    """The prefetcher applies them; a dataset it does not wrap ('synthetic:' hands out float items) must not train on silently."""
    from wesup_amd import train
    with pytest.raises(ValueError, match='stain_normalize / stain_jitter'):
        train.fit('synthetic:64:64:6:2', device=DEV, epochs=1, batch_size=1, smoke=True, stain_jitter=0.1)


def test_prefetcher_equals_the_plain_one_on_prepared_images():
    """DevicePrefetcher(stain=..., stain_jitter=0.1) yields what the plain prefetcher yields on images that were normalised and
    jittered beforehand with the rows of the stated second generator."""
    from wesup_amd import stain as S
    from wesup_amd.utils import data as D
    ds = C.RawItems(4, 48, 40)
    norm = S.StainNormalizer(device=DEV)
    gen = D.stain_jitter_generator(5)
    prepared = []
    for first in (0, 2):
        batch = _dev(np.stack(ds.images[first:first + 2]))
        rows = D.sample_stain_jitter(gen, 0.1, 2)
        prepared += list(S.stain_jitter(norm(batch), _dev(rows)).cpu().numpy())
    assert any((p != i).any() for p, i in zip(prepared, ds.images))

    def items(dataset, **kw):
        loader = torch.utils.data.DataLoader(dataset, batch_size=2, shuffle=False, num_workers=0)
        out = list(D.DevicePrefetcher(loader, DEV, train=True, with_points=True, has_masks=True, seed=5, **kw))
        torch.cuda.synchronize()
        return out
    got = items(ds, stain=norm, stain_jitter=0.1)
    want = items(C.RawItems(4, 48, 40, images=prepared))
    assert len(got) == len(want) == 2
    for g, w in zip(got, want):
        assert len(g) == len(w) == 3
        for a, b in zip(g, w):
            assert torch.equal(a, b)
