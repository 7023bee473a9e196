"""Exact t-SNE on the GPU (csrc/tsne.hip, ops.tsne_*, wesup_amd/tsne.py) against the fp64 restatement tests/_tsneref.py.

Where a bar is "the float32 restatement's own error", that is the same numpy code run in float32 on the same case, against fp64;
the device gets four times it (another summation order).  Each stage is held to the inputs it was given -- the search to the
device's own distances, the iteration to the device's own P and to the float32 state -- so that one stage's rounding is not
charged to the next.  Scalars that are sums of same-signed terms (Z, the three parts of the KL divergence) get a bar from the
format instead, ULPS roundings of 2^-24 per term and along the longest chain of additions: one number against one number has no
"own error" to borrow that luck could not make 0."""
import os

import numpy as np
import pytest
import torch

import _tsneref as R
from _tol import within
from _tsnecases import DIMS, SIZES, STATE_ITERS, WHOLE_RUN_PERPLEXITY, WHOLE_RUN_SIZES, clusters, perplexity_for, phase_of, start

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
U = 2.0 ** -24
ULPS = 64          # <= 5 roundings in a term (squares, their sum, + 1, the quotient, the product), <= 32 sequential additions per
#                    lane at N = 2049, 6 shuffle steps, 8 slabs, 9 per thread and 8 across the block in the update kernel


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32)).to(DEV)


def _np(t):
    return t.detach().cpu().numpy().astype(np.float64)


def _rel(a, ref):
    m = np.abs(ref).max()
    return float(np.abs(a - ref).max() / m) if m > 0 else float(np.abs(a).max())


@pytest.fixture(scope='module')
def gold(golden_dir):
    return np.load(os.path.join(golden_dir, 'tsne.npz'))


# ---------------------------------------------------------------- squared distances
def _check_sqdist(case, x):
    from wesup_amd import ops
    d2 = ops.tsne_sqdist(_dev(x))
    assert torch.equal(d2, d2.T) and float(d2.diagonal().abs().max()) == 0.0
    ref = R.sqdist(x)
    own = _rel(R.sqdist(x, np.float32).astype(np.float64), ref)
    assert within(case, 'tsne sqdist vs fp64', _rel(_np(d2), ref), 4 * own, 'max error / max distance; 4 x float32 numpy')
    return d2


@pytest.mark.parametrize('n', SIZES)
def test_sqdist_sizes(n):
    _check_sqdist(f'n{n}', clusters(n, n, 32)[0])


@pytest.mark.parametrize('d', DIMS)
def test_sqdist_feature_counts(d):
    _check_sqdist(f'd{d}', clusters(d, 130, d)[0])


# ---------------------------------------------------------------- search and joint probabilities
def _check_affinities(case, x, perp):
    """The search is held to the distances it was given (the device's, read as fp64): what float32 costs the distances is
    test_sqdist's."""
    from wesup_amd import ops
    n = x.shape[0]
    d2_dev = ops.tsne_sqdist(_dev(x))
    P_dev, beta_dev = ops.tsne_affinities(d2_dev, perp)
    assert torch.equal(P_dev, P_dev.T) and float(P_dev.diagonal().abs().max()) == 0.0
    d2, P, beta = _np(d2_dev), _np(P_dev), _np(beta_dev)
    assert np.isfinite(P).all() and np.isfinite(beta).all() and (beta > 0).all()
    off = ~np.eye(n, dtype=bool)
    assert P[off].min() >= np.float32(R.EPS)
    target = np.log(perp)
    beta32 = R.search(d2, perp, np.float32).astype(np.float64)
    beta64 = R.search(d2, perp)
    # rows no beta brings to the target (more than `perplexity` neighbours at the smallest distance) run all 100 steps everywhere
    reach = beta64 < 2.0 ** 90
    assert np.array_equal(reach, beta < 2.0 ** 90) and np.array_equal(reach, beta32 < 2.0 ** 90)
    if reach.any():
        # the rule stops on the float32 entropy: the fp64 entropy is within 1e-5 plus what float32 misses the entropy by, and that
        # is measured on the same rows at the same betas with the restatement in float32 (3e-7 - 5e-7: H is 3 - 5, half an ulp
        # of its logarithm alone is 1.2e-7 - 2.4e-7)
        own_miss = float(np.abs(R.row_entropy(d2, beta, np.float32).astype(np.float64) - R.row_entropy(d2, beta))[reach].max())
        miss = float(np.abs(R.row_entropy(d2, beta) - target)[reach].max())
        print(f'{case}: entropy miss device {miss:.4e}, float32 numpy misses the fp64 entropy by {own_miss:.3e}')
        assert within(case, 'tsne row entropy at the device beta', miss, R.SEARCH_TOL + own_miss, '1e-5 + float32 numpy\'s miss')
        # two stopping points within the tolerance of one target: |d beta| = |dH| / (beta Var d) with |dH| <= 2e-5, and 1e-5 more for
        # what float32 does to H itself
        dd, _ = R._shifted(d2, np.float64)
        e = np.where(off, np.exp(-beta64[:, None] * dd), 0)
        C = e / e.sum(1, keepdims=True)
        var = (C * (dd - (C * dd).sum(1, keepdims=True)) ** 2).sum(1)
        ratio = (np.abs(beta - beta64)[reach] / (3e-5 / (beta64 * var)[reach])).max()
        rel = (np.abs(beta - beta64) / beta64)[reach].max()
        print(f'{case}: beta vs fp64 search, relative {rel:.3e}, of what the tolerance allows {ratio:.3f}')
        assert within(case, 'tsne beta vs fp64 search / allowed by the tolerance', ratio, 1.0, f'relative distance {rel:.3e}')
    ref = R.joint(d2, beta)
    own = _rel(R.joint(d2, beta, np.float32).astype(np.float64), ref)
    assert within(case, 'tsne P vs fp64 at the device beta', _rel(P, ref), 4 * own, 'max error / max P; 4 x float32 numpy')
    # <= 3 roundings in an entry, <= 2 + log2(256 n) along the total: under 32
    assert within(case, 'tsne sum of P - 1', abs(P.sum() - 1.0), 32 * U)
    return P_dev, beta_dev


@pytest.mark.parametrize('n', SIZES)
def test_affinities_sizes(n):
    _check_affinities(f'n{n}', clusters(n, n, 32)[0], perplexity_for(n))


@pytest.mark.parametrize('d', DIMS)
def test_affinities_feature_counts(d):
    _check_affinities(f'd{d}', clusters(d, 130, d)[0], 30.0)


def test_affinities_ten_identical_rows_and_a_far_row():
    _check_affinities('same10', clusters(11, 200, 32, same=10)[0], 30.0)
    x = clusters(12, 200, 32, far=True)[0]
    P, _ = _check_affinities('far', x, 30.0)
    # no all-zero row: the far row's own conditional row sums to 1, so its row of P holds 1 / 2N of the mass whoever else picks
    # it (nobody does), less the roundings of the sum
    assert _np(P)[0].sum() >= (1 - 32 * U) / (2 * 200)


def test_all_rows_identical_uniform_p_and_zero_gradient():
    from wesup_amd import ops
    n = 70
    x = np.full((n, 32), 1.5, np.float32)
    d2 = ops.tsne_sqdist(_dev(x))
    assert float(d2.abs().max()) == 0.0
    P, beta = ops.tsne_affinities(d2, perplexity_for(n))
    Pn = _np(P)
    off = ~np.eye(n, dtype=bool)
    assert len(np.unique(Pn[off])) == 1 and abs(Pn[0, 1] * n * (n - 1) - 1) <= 32 * U and torch.isfinite(beta).all()
    y0 = np.full((n, 2), 0.25, np.float32)
    y, upd, gains, stats = _dev(y0), _dev(np.zeros((n, 2))), _dev(np.ones((n, 2))), torch.zeros(4, device=DEV)
    ops.tsne_iterate(P, y, upd, gains, stats, 3, 12.0, 0.5, 50.0, 0.01)
    assert float(upd.abs().max()) == 0.0 and np.array_equal(y.cpu().numpy(), y0) and float(stats[1]) == 0.0
    assert float(stats[2]) == n * (n - 1)


# ---------------------------------------------------------------- one iteration
def _one_iteration(case, P_dev, y0, upd0, gains0, ex, mom, lr):
    """One device iteration from a float32 state against fp64 from the same state and the same P."""
    from wesup_amd import ops
    n = y0.shape[0]
    y0, upd0, gains0 = (np.asarray(a, np.float32) for a in (y0, upd0, gains0))
    y, upd, gains, stats = _dev(y0), _dev(upd0), _dev(gains0), torch.zeros(4, device=DEV)
    ops.tsne_iterate(P_dev, y, upd, gains, stats, 1, ex, mom, lr, R.MIN_GAIN)
    y, upd, gains, stats = _np(y), _np(upd), _np(gains), _np(stats)
    P = _np(P_dev)
    s64 = [a.astype(np.float64) for a in (y0, upd0, gains0)]
    g64, kl64, Z64 = R.gradient(P, s64[0], ex)
    y64, upd64, gains64 = R.update(g64, *s64, mom, lr)
    g32, kl32, Z32 = R.gradient(P, y0, ex, np.float32)
    y32, upd32, gains32 = R.update(g32, y0, upd0, gains0, mom, lr, dtype=np.float32)
    gmax, extent = np.abs(g64).max(), max(np.ptp(y64, axis=0).max(), 1e-30)

    def rebuilt(upd_new, gains_new):                                   # g as the update saw it
        return (mom * s64[1] - upd_new.astype(np.float64)) / (lr * gains_new.astype(np.float64))
    own_g = np.abs(rebuilt(upd32, gains32) - g64).max() / gmax
    err_g = np.abs(rebuilt(upd, gains) - g64).max() / gmax
    assert within(case, 'tsne gradient rebuilt from upd vs fp64', err_g, 4 * own_g, 'max error / max |g|; 4 x float32 numpy')
    # the gain rule's branch: may differ only where upd g is within the gradient's bar of 0; counted, not compared
    flip = (gains != gains64.astype(np.float32)) & (np.abs(gains - gains64) > 1e-6)
    assert (np.abs(s64[1] * g64)[flip] <= np.abs(s64[1][flip]) * 4 * own_g * gmax).all()
    assert within(case, 'tsne gain branches taken differently / 2N', flip.mean(), 0.005)
    keep = ~flip
    assert within(case, 'tsne gains vs fp64', np.abs(gains - gains64)[keep].max(), 2 * U * max(gains64.max(), 1.0))
    own_y = np.abs(y32 - y64)[keep].max() / extent
    assert within(case, 'tsne y after one iteration vs fp64', np.abs(y - y64)[keep].max() / extent, 4 * own_y + U,
                  'max error / extent; 4 x float32 numpy + the rounding of y')
    assert within(case, 'tsne Z vs fp64', abs(stats[2] - Z64) / Z64, ULPS * U)
    pc = np.maximum(P, R.EPS)
    offd = ~np.eye(n, dtype=bool)
    df = s64[0][:, None] - s64[0][None]
    parts = abs((pc * np.log(pc))[offd].sum()) + abs((pc * np.log1p((df * df).sum(-1)))[offd].sum()) + abs(np.log(Z64))
    assert within(case, 'tsne KL vs fp64 / its three sums', abs(stats[0] - kl64) / parts, ULPS * U)
    gn64 = np.sqrt((g64 ** 2).sum())
    assert within(case, 'tsne |g| vs fp64', abs(stats[1] - gn64) / gn64 if gn64 > 0 else abs(stats[1]),
                  np.sqrt(2 * n) * 4 * own_g * gmax / max(gn64, 1e-300) + 4 * U, 'sqrt(2N) x the gradient bar')


@pytest.mark.parametrize('n', WHOLE_RUN_SIZES)
@pytest.mark.parametrize('it', STATE_ITERS)
def test_one_iteration_from_the_trajectory(gold, n, it):
    """The fp64 trajectory's state at iterations 1, 50 and 300: tiny, exaggerated, spread."""
    from wesup_amd import tsne as T
    x, _ = clusters(7, n, 32)
    assert float(x.astype(np.float64).sum()) == float(gold[f'xsum_{n}'])
    P_dev, _ = T.affinities(_dev(x), WHOLE_RUN_PERPLEXITY[n])
    ex, mom = phase_of(it)
    _one_iteration(f'n{n}it{it}', P_dev, gold[f'y_{n}_{it}'], gold[f'upd_{n}_{it}'], gold[f'gains_{n}_{it}'], ex, mom,
                   max(n / 12.0 / 4.0, 50.0))


@pytest.mark.parametrize('n', SIZES)
def test_one_iteration_sizes(n):
    """Every size the kernels branch on, from made-up states of the three kinds (a trajectory in fp64 is out of reach at 2049)."""
    from wesup_amd import tsne as T
    x, _ = clusters(n, n, 32)
    P_dev, _ = T.affinities(_dev(x), perplexity_for(n))
    rs = np.random.RandomState(n)
    # (two points have p = q = 1/2 whatever y is: without exaggeration their gradient is exactly 0 and every sign in the gain
    #  rule is rounding -- N = 2 keeps the two exaggerated states)
    for scale, ex, mom in ((1e-4, 12.0, 0.5), (1.0, 12.0, 0.5), (30.0, 1.0, 0.8))[:1 if n > 300 else 2 if n == 2 else 3]:
        y0 = scale * rs.standard_normal((n, 2))
        upd0 = 0.02 * scale * rs.standard_normal((n, 2))
        gains0 = rs.uniform(0.01, 3.0, (n, 2))
        _one_iteration(f'n{n}s{scale}', P_dev, y0, upd0, gains0, ex, mom, max(n / 48.0, 50.0))


def test_iters_zero_moves_nothing_and_two_calls_equal_one():
    from wesup_amd import ops, tsne as T
    n = 257
    P, _ = T.affinities(_dev(clusters(7, n, 32)[0]), 30.0)

    def state():
        return _dev(start(n)), _dev(np.zeros((n, 2))), _dev(np.ones((n, 2))), torch.zeros(4, device=DEV)
    a, b = state(), state()
    ops.tsne_iterate(P, *a, 7, 12.0, 0.5, 50.0, 0.01)
    ops.tsne_iterate(P, *b, 3, 12.0, 0.5, 50.0, 0.01)
    ops.tsne_iterate(P, *b, 4, 12.0, 0.5, 50.0, 0.01)
    assert all(torch.equal(s, t) for s, t in zip(a, b))                # the stats too: both are the 7th iteration's
    before = [t.clone() for t in a[:3]]
    ops.tsne_iterate(P, *a, 0, 1.0, 0.8, 50.0, 0.01)
    assert all(torch.equal(s, t) for s, t in zip(before, a[:3]))
    g, kl, Z = R.gradient(_np(P), _np(a[0]), 1.0)
    assert abs(float(a[3][2]) - Z) / Z <= ULPS * U and abs(float(a[3][1]) - np.sqrt((g ** 2).sum())) <= 1e-4 * np.sqrt((g ** 2).sum())


# ---------------------------------------------------------------- ten iterations, the whole run
@pytest.mark.parametrize('n', WHOLE_RUN_SIZES)
def test_ten_iterations_from_the_start(n):
    """The whole pipeline in float32 against the whole pipeline in fp64; nothing positional is compared beyond ten iterations
    (float32 and fp64 trajectories are O(1) apart by iteration 50)."""
    from wesup_amd import ops, tsne as T
    x, _ = clusters(7, n, 32)
    perp, lr, y0 = WHOLE_RUN_PERPLEXITY[n], max(n / 48.0, 50.0), start(n)
    zero, one = np.zeros((n, 2)), np.ones((n, 2))
    ref = R.iterate(R.affinities(x, perp)[0], y0, zero, one, 10, 12.0, 0.5, lr)[0]
    own = R.iterate(R.affinities(x, perp, np.float32)[0], y0, zero, one, 10, 12.0, 0.5, lr, dtype=np.float32)[0]
    extent = np.ptp(ref, axis=0).max()
    own = np.abs(own - ref).max() / extent
    P, _ = T.affinities(_dev(x), perp)
    y = _dev(y0)
    ops.tsne_iterate(P, y, _dev(zero), _dev(one), torch.zeros(4, device=DEV), 10, 12.0, 0.5, lr, 0.01)
    print(f'n{n}: ten iterations, float32 numpy {own:.3e} of the extent')
    assert within(f'n{n}', 'tsne y after ten iterations vs fp64', np.abs(_np(y) - ref).max() / extent, 4 * own,
                  'max error / extent; 4 x float32 numpy')


@pytest.mark.parametrize('n', WHOLE_RUN_SIZES)
def test_whole_default_run(gold, n):
    from wesup_amd import tsne as T
    x, lab = clusters(7, n, 32)
    assert float(x.astype(np.float64).sum()) == float(gold[f'xsum_{n}'])
    X = _dev(x)
    perp = WHOLE_RUN_PERPLEXITY[n]
    t = T.TSNE(perplexity=perp, init='random', random_state=0).fit(X)
    t2 = T.TSNE(perplexity=perp, init='random', random_state=0).fit(X)
    assert torch.equal(t.embedding_, t2.embedding_) and t.kl_divergence_ == t2.kl_divergence_ and t.n_iter_ == t2.n_iter_
    assert t.stats_history_ == t2.stats_history_ and t.learning_rate_ == 50.0
    y = _np(t.embedding_)
    assert y.shape == (n, 2) and np.isfinite(y).all()
    # the reported KL is the returned embedding's
    P = _np(T.affinities(X, perp)[0])
    _, kl64, Z64 = R.gradient(P, y, 1.0)
    pc = np.maximum(P, R.EPS)
    offd = ~np.eye(n, dtype=bool)
    df = y[:, None] - y[None]
    parts = abs((pc * np.log(pc))[offd].sum()) + abs((pc * np.log1p((df * df).sum(-1)))[offd].sum()) + abs(np.log(Z64))
    assert within(f'n{n}', 'tsne reported KL vs fp64 KL of the embedding / its three sums', abs(t.kl_divergence_ - kl64) / parts,
                  ULPS * U)
    # n_iter_ is the stopping rules on the device's own checks
    hist = list(t.stats_history_)
    assert [h[0] for h in hist] == list(range(49, hist[-1][0] + 1, 50))
    todo, it = list(hist), -1
    for end, _, _, patience in T.phases(t.max_iter, t.early_exaggeration, t.n_iter_without_progress):
        if it + 1 < end:
            it = T.descend(lambda k: todo.pop(0)[1:], it + 1, end, patience, t.min_grad_norm)
    assert it == t.n_iter_ and not todo
    # as good an embedding as fp64 finds from five starts
    lo, hi = float(gold[f'kl_{n}'].min()), float(gold[f'kl_{n}'].max())
    print(f'n{n}: KL {t.kl_divergence_:.5f} (fp64, five starts: {lo:.5f} .. {hi:.5f}), n_iter {t.n_iter_}')
    assert within(f'n{n}', 'tsne final KL vs five fp64 runs', t.kl_divergence_, hi + (hi - lo))
    purity = R.knn_purity(y, lab)
    assert within(f'n{n}', 'tsne 1 - neighbour purity', 1.0 - purity, 1.0 - (float(gold[f'purity_{n}'].min()) - 1.0 / n))


def test_init_pca_and_given_run():
    from wesup_amd import tsne as T
    x, lab = clusters(7, 65, 32)
    t = T.TSNE(perplexity=20.0, init='pca', max_iter=250).fit(_dev(x))
    assert t.n_iter_ == 249 and np.isfinite(t.kl_divergence_) and R.knn_purity(_np(t.embedding_), lab) >= 0.9
    y0 = start(65, 3)
    a = T.TSNE(perplexity=20.0, init=y0, max_iter=250).fit_transform(_dev(x))
    b = T.TSNE(perplexity=20.0, init='random', random_state=3, max_iter=250).fit_transform(_dev(x))
    assert torch.equal(a, b)


# ---------------------------------------------------------------- the program
def _write_dataset(root, n=2, H=96, W=80):
    from PIL import Image
    os.makedirs(root / 'images')
    os.makedirs(root / 'masks')
    for i in range(n):
        rs = np.random.RandomState(40 + i)
        yy, xx = np.mgrid[:H, :W]
        blob = ((yy - H * (0.4 + 0.2 * i)) ** 2 + (xx - W * 0.5) ** 2) < (0.3 * W) ** 2
        img = np.where(blob[..., None], (200, 90, 160), (120, 170, 220)) + rs.randint(-40, 40, (H, W, 3))
        Image.fromarray(np.clip(img, 0, 255).astype(np.uint8)).save(root / 'images' / f'im{i}.png')
        Image.fromarray(blob.astype(np.uint8)).save(root / 'masks' / f'im{i}.png')


def _weights(seed):
    from oracle import wesup_oracle as orc
    return {k: torch.from_numpy(v) for k, v in orc.make_weights(seed, feat_scale=0.03).items()}


def test_collect_sp_features_and_the_program(tmp_path):
    from wesup_amd import tsne as T
    from wesup_amd.models import initialize_trainer
    from wesup_amd.utils.data import SegmentationDataset
    _write_dataset(tmp_path / 'data')
    ds = SegmentationDataset(tmp_path / 'data', train=False)
    trainer = initialize_trainer('wesup', device=DEV)
    trainer.model.load_state_dict(_weights(3))
    feats, labels = T.collect_sp_features(trainer, ds, 2)
    rows = []
    for i in range(2):
        img, mask = ds.to_reference_item(ds[i])
        (x, sp_maps), _ = trainer.preprocess(img.unsqueeze(0), mask.unsqueeze(0))
        with torch.no_grad():
            trainer.model((x, sp_maps))
        n = int(sp_maps.meta.n_sp[0])
        f = trainer.model.sp_features
        rows.append((f[0] if f.dim() == 3 else f)[:n].clone())
    assert feats.shape == (sum(r.shape[0] for r in rows), trainer.model.D) and feats.dtype == torch.float32 and feats.is_cuda
    assert torch.equal(feats, torch.cat(rows))
    assert labels.shape == (feats.shape[0],) and set(labels.unique().tolist()) == {0, 1}
    assert all(r.shape[0] > 10 for r in rows)
    assert T.collect_sp_features(trainer, ds, 1)[0].shape[0] == rows[0].shape[0]
    # the program: two checkpoints in, the reference's keys out
    for name, seed in (('before', 3), ('after', 4)):
        torch.save({'epoch': 0, 'model_state_dict': _weights(seed)}, tmp_path / f'{name}.pth')
    out = tmp_path / 'tsne.npz'
    T.main([str(tmp_path / 'data'), '-c', str(tmp_path / 'after.pth'), '--before', str(tmp_path / 'before.pth'), '--rescale-factor',
            '1.0', '--images', '2', '--init', 'random', '--max-iter', '250', '--device', DEV, '-o', str(out)])
    z = np.load(out)
    assert sorted(z.files) == ['after_x2d', 'before_x2d', 'kl_after', 'kl_before', 'n_iter', 'sp_labels']
    N = feats.shape[0]
    assert z['before_x2d'].shape == z['after_x2d'].shape == (N, 2) and z['sp_labels'].shape == (N,)
    assert np.array_equal(z['sp_labels'], labels.cpu().numpy())
    assert all(np.isfinite(z[k]).all() for k in z.files) and z['n_iter'].tolist() == [249, 249]
    assert not np.array_equal(z['before_x2d'], z['after_x2d'])
