"""t-SNE without a GPU: the fp64 restatement (tests/_tsneref.py) against scikit-learn's own functions, the host logic of
wesup_amd/tsne.py (learning rate, schedule, stopping rules, initial embeddings, refusals), the argument checks of the three
entries through ctypes, the kernels' machine code, and the program's argument parsing and output keys."""
import ctypes
import os
import re
import shutil
import subprocess
import types

import numpy as np
import pytest
import torch

import _tsneref as R
from _tol import within
from _tsnecases import clusters, perplexity_for

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ---------------------------------------------------------------- the restatement against scikit-learn
def _sk():
    pytest.importorskip('sklearn')
    from sklearn.manifold import _t_sne
    for name in ('_joint_probabilities', '_kl_divergence', '_gradient_descent', 'MACHINE_EPSILON'):
        if not hasattr(_t_sne, name):
            pytest.skip(f'sklearn.manifold._t_sne.{name} is gone')
    return _t_sne


@pytest.mark.parametrize('n,d', [(65, 32), (257, 32), (64, 1)])
def test_joint_probabilities_equal_sklearns(n, d):
    """No underflow in these cases, so the shift changes nothing but rounding.  scikit-learn rounds the distances to float32 and
    searches in double: the restatement gets the same float32 distances.  Both searches stop anywhere within 1e-5 of the target
    entropy, so where a rounding takes one of them a step further the rows differ by what that tolerance allows: to first order
    |dC_ij| = C_ij |<d>_i - d_ij| |dH| / (beta_i Var_i d) (from dC/dbeta = C (<d> - d), dH/dbeta = -beta Var d) with |dH| <= 2e-5
    between two stopping points; P = (C + C^T) / 2n carries the mean of the two.  The bar is twice the largest such entry."""
    sk = _sk()
    from scipy.spatial.distance import squareform
    x, _ = clusters(n, n, d)
    d2 = R.sqdist(x).astype(np.float32)
    perp = perplexity_for(n)
    beta = R.search(d2, perp)
    P = R.joint(d2, beta)
    Psk = squareform(sk._joint_probabilities(d2, perp, 0))
    off = ~np.eye(n, dtype=bool)
    dd, _ = R._shifted(d2, np.float64)
    e = np.where(off, np.exp(-beta[:, None] * dd), 0)
    C = e / e.sum(1, keepdims=True)
    mean = (C * dd).sum(1, keepdims=True)
    var = (C * (dd - mean) ** 2).sum(1, keepdims=True)
    with np.errstate(invalid='ignore', divide='ignore'):           # a row of equal distances has one entropy whatever beta is
        dC = np.where(var > 0, C * np.abs(mean - dd) * 2e-5 / (beta[:, None] * var), 0)
    bar = 2 * ((dC + dC.T) / (2 * n)).max()
    assert within(f'n{n}d{d}', 'tsne restatement P vs sklearn', np.abs(P - Psk)[off].max(), bar)
    reach = beta < 2.0 ** 90                                       # (more than `perplexity` neighbours at distance 0: no beta reaches it)
    assert reach.sum() >= n // 4 and np.abs(R.row_entropy(d2, beta) - np.log(perp))[reach].max() <= 1e-5


@pytest.mark.parametrize('n', [65, 257])
def test_gradient_and_kl_equal_sklearns(n):
    sk = _sk()
    from scipy.spatial.distance import squareform
    x, _ = clusters(n, n, 32)
    P, _ = R.affinities(x, perplexity_for(n))
    rs = np.random.RandomState(n)
    for scale in (1e-4, 1.0, 30.0):
        y = scale * rs.standard_normal((n, 2))
        g, kl, _ = R.gradient(P, y)
        kl_sk, g_sk = sk._kl_divergence(y.ravel(), squareform(P, checks=False), 1, n, 2)
        assert within(f'n{n}s{scale}', 'tsne restatement KL vs sklearn', abs(kl - kl_sk) / abs(kl_sk), 1e-10)
        assert within(f'n{n}s{scale}', 'tsne restatement gradient vs sklearn', np.abs(g.ravel() - g_sk).max() / np.abs(g_sk).max(), 1e-10)


@pytest.mark.parametrize('n', [65, 257])
def test_twenty_iterations_equal_sklearns_descent(n):
    sk = _sk()
    from scipy.spatial.distance import squareform
    x, _ = clusters(n, n, 32)
    P, _ = R.affinities(x, perplexity_for(n))
    y0 = 1e-4 * np.random.RandomState(0).standard_normal((n, 2))
    lr = max(n / 12.0 / 4.0, 50.0)
    y, _, _, _ = R.iterate(12.0 * P, y0, np.zeros_like(y0), np.ones_like(y0), 20, 1.0, 0.5, lr)
    y_sk, _, it = sk._gradient_descent(sk._kl_divergence, y0.ravel().copy(), 0, 20, n_iter_check=50, momentum=0.5, learning_rate=lr,
                                       min_gain=0.01, min_grad_norm=0, args=[squareform(12.0 * P, checks=False), 1, n, 2],
                                       kwargs=dict(skip_num_points=0))
    assert it == 19
    extent = np.ptp(y_sk.reshape(n, 2), axis=0).max()
    assert within(f'n{n}', 'tsne restatement 20 iterations vs sklearn', np.abs(y - y_sk.reshape(n, 2)).max() / extent, 1e-8)


def test_exaggeration_scales_p_in_the_gradient_only():
    x, _ = clusters(3, 40, 8)
    P, _ = R.affinities(x, 10.0)
    y = np.random.RandomState(1).standard_normal((40, 2))
    g12, kl12, _ = R.gradient(P, y, 12.0)
    g1, kl1, _ = R.gradient(12.0 * P, y, 1.0)
    assert np.allclose(g12, g1, rtol=1e-13, atol=0) and kl12 == R.gradient(P, y, 1.0)[1] and kl12 != kl1


def test_shift_rescues_a_far_row_and_float32_runs_the_same_code():
    x, _ = clusters(5, 64, 32, far=True)
    d2 = R.sqdist(x)
    assert d2[0, 1:].min() > 5e7                                       # exp(-1 * 5e7) is 0 in any format
    # float32 sees the far row's distances (1e8) on a grid of 8: its search is held to the distances it was given, with 1e-5 more
    # for its own arithmetic
    for dt, tol in ((np.float64, 1e-5), (np.float32, 2e-5)):
        beta = R.search(d2, 20.0, dt)
        assert beta.dtype == dt
        assert np.abs(R.row_entropy(d2.astype(dt).astype(np.float64), beta.astype(np.float64)) - np.log(20.0)).max() <= tol
        P = R.joint(d2, beta, dt)
        assert P.dtype == dt and np.isfinite(P).all() and abs(P.sum() - 1) < 1e-5 and (P == P.T).all()


def test_identical_rows_give_uniform_p_and_zero_gradient():
    x = np.ones((20, 5), np.float32)
    P, beta = R.affinities(x, 20 / 3.0)
    off = ~np.eye(20, dtype=bool)
    assert np.allclose(P[off], 1.0 / (20 * 19), rtol=1e-14) and np.isfinite(beta).all()
    g, _, _ = R.gradient(P, np.zeros((20, 2)))
    assert (g == 0).all()


# ---------------------------------------------------------------- host logic
def test_auto_learning_rate_and_phases():
    from wesup_amd import tsne as T
    assert T.auto_learning_rate(6000, 12.0) == pytest.approx(6000 / 12.0 / 4.0) == 125.0
    assert T.auto_learning_rate(100, 12.0) == 50.0
    assert T.phases(1000, 12.0, 300) == [(250, 12.0, 0.5, 250), (1000, 1.0, 0.8, 300)]
    assert (T.EXPLORATION_ITERS, T.N_ITER_CHECK, T.MIN_GAIN) == (R.EXPLORATION_ITERS, R.N_ITER_CHECK, R.MIN_GAIN) == (250, 50, 0.01)


def _drive(stats, it, max_iter, patience, min_grad_norm):
    """wesup_amd.tsne.descend and the restatement's one-iteration-at-a-time loop over the same KL / |g| per iteration."""
    from wesup_amd import tsne as T
    pos = {'i': it}
    calls, hist = [], []

    def step(k):
        calls.append(k)
        pos['i'] += k
        return stats[pos['i'] - 1]
    got = T.descend(step, it, max_iter, patience, min_grad_norm, history=hist)
    one = {'i': it}

    def step1(check):
        one['i'] += 1
        return stats[one['i'] - 1]
    assert got == R.descend(step1, it, max_iter, patience, min_grad_norm)
    assert sum(calls) == got - it + 1                                  # the device ran exactly the iterations the rule allows
    return got, calls, hist


def test_stopping_rules_on_stubbed_stats():
    flat = {i: (1.0, 1.0) for i in range(2000)}
    # KL improves until iteration 399, then never: 300 iterations without progress are over at the check of iteration 749
    stats = {i: (1.0 / (1 + min(i, 399)), 1.0) for i in range(2000)}
    got, calls, hist = _drive(stats, 250, 1000, 300, 1e-7)
    assert got == 749 and calls == [50] * 10 and [h[0] for h in hist] == list(range(299, 750, 50))
    # |g| under the bar at the check of iteration 449 (and at iteration 430, where nobody looks)
    stats = {i: (1.0 / (1 + i), 1e-8 if i in (430, 449) else 1.0) for i in range(2000)}
    assert _drive(stats, 250, 1000, 300, 1e-7)[0] == 449
    # nothing triggers: the last index, with a short last call when max_iter is no multiple of 50, and a start between checks
    assert _drive({i: (1.0 / (1 + i), 1.0) for i in range(2000)}, 250, 1000, 300, 1e-7)[0] == 999
    got, calls, _ = _drive(flat, 201, 260, 300, 1e-7)
    assert got == 259 and calls == [49, 10]
    # the first phase cannot run out of patience: 250 iterations, patience 250
    assert _drive(flat, 0, 250, 250, 1e-7)[0] == 249


def test_fit_runs_the_schedule_on_a_stubbed_device(monkeypatch):
    """TSNE.fit with the three device calls replaced: what it enqueues, with which exaggeration and momentum, and that update and
    gains start again at the switch."""
    from wesup_amd import ops, tsne as T
    log = []

    def iterate(P, y, upd, gains, stats, iters, ex, mom, lr, min_gain):
        log.append((iters, ex, mom, lr, min_gain, float(upd.abs().max()), float(gains.min())))
        upd += 1.0
        gains *= 0.5
        stats[0] = 1.0 / (1 + len(log))
        stats[1] = 1.0
    monkeypatch.setattr(ops, 'tsne_iterate', iterate)
    monkeypatch.setattr(T, 'affinities', lambda X, perp: (torch.zeros(X.shape[0], X.shape[0]), None))
    t = T.TSNE(max_iter=500, init='random', random_state=0).fit(torch.zeros(100, 3))
    assert t.n_iter_ == 499 and t.learning_rate_ == 50.0 and len(t.stats_history_) == 10
    assert [e[:5] for e in log[:5]] == [(50, 12.0, 0.5, 50.0, 0.01)] * 5 and [e[:3] for e in log[5:10]] == [(50, 1.0, 0.8)] * 5
    assert log[0][5:] == (0.0, 1.0) and log[5][5:] == (0.0, 1.0) and log[6][5:] == (1.0, 0.5)
    assert log[10][:2] == (0, 1.0) and len(log) == 11               # the closing evaluation of the returned embedding
    assert t.kl_divergence_ == pytest.approx(1.0 / 12)


def test_initial_embeddings():
    from wesup_amd import tsne as T
    y = T.random_init(57, 3)
    want = 1e-4 * np.random.RandomState(3).standard_normal(size=(57, 2)).astype(np.float32)
    assert y.dtype == np.float32 and np.array_equal(y, want)
    x, _ = clusters(1, 200, 32)
    y = T.pca_init(x)
    assert y.dtype == np.float32 and y.shape == (200, 2) and y[:, 0].std() == pytest.approx(1e-4, rel=1e-5)
    # the principal axes: uncorrelated, the first carries the most variance, and they span what the SVD's first two do
    xc = x.astype(np.float64) - x.astype(np.float64).mean(0)
    u, s, _ = np.linalg.svd(xc, full_matrices=False)
    assert abs(np.corrcoef(y.T)[0, 1]) < 1e-4 and y[:, 1].std() / y[:, 0].std() == pytest.approx(s[1] / s[0], rel=1e-4)
    assert np.abs(np.abs(np.corrcoef(y[:, 0], u[:, 0])[0, 1]) - 1) < 1e-6
    assert T.pca_init(x[:, :1]).shape == (200, 2)
    given = np.arange(20, dtype=np.float64).reshape(10, 2)
    t = T.TSNE(init=given)
    assert np.array_equal(t._initial(torch.zeros(10, 4)), given.astype(np.float32))
    with pytest.raises(ValueError):
        T.TSNE(init=given)._initial(torch.zeros(11, 4))


def test_refusals_before_any_device_work():
    from wesup_amd import ops, tsne as T
    for shape, perp in (((1, 4), 0.5), ((32769, 1), 30.0), ((10, 4), 10.0), ((10, 4), 0.0), ((10, 4097), 3.0)):
        with pytest.raises(ValueError):
            T.TSNE(perplexity=perp).fit(torch.empty(shape))
        with pytest.raises(ValueError):
            T.affinities(torch.empty(shape), perp)
    with pytest.raises(ValueError):
        T.TSNE(n_components=3)
    for kw in (dict(init='spectral'), dict(max_iter=249), dict(learning_rate=0.0), dict(early_exaggeration=0.5)):
        with pytest.raises(ValueError):
            T.TSNE(**kw)
    with pytest.raises(ValueError):
        T.TSNE().fit(torch.empty(10))
    from wesup_amd import _lib
    with pytest.raises(_lib.WesupHipError):                            # in range, but a host tensor: there is no CPU path
        T.TSNE(perplexity=3.0).fit(torch.zeros(10, 4))
    with pytest.raises(ValueError):
        ops.tsne_sqdist(torch.empty(1, 3))


# ---------------------------------------------------------------- the entries through ctypes, the machine code
def test_entries_refuse_bad_arguments_on_the_host():
    from wesup_amd import _lib
    h = _lib.load()
    assert h.wesup_abi_version() == 6 and (_lib.TSNE_MAX_N, _lib.TSNE_MAX_D, _lib.TSNE_STATS) == (32768, 4096, 4)
    hdr = open(os.path.join(ROOT, 'include', 'wesup_hip.h')).read()
    assert '#define WESUP_TSNE_MAX_N 32768' in hdr and '#define WESUP_TSNE_MAX_D 4096' in hdr and '#define WESUP_TSNE_STATS 4' in hdr
    aff, itb = h.wesup_tsne_affinities_workspace_bytes, h.wesup_tsne_iterate_workspace_bytes
    for n in (-1, 0, 1, 32769):
        assert aff(n) == 0 and itb(n) == 0
    assert aff(2) >= 12 and aff(32768) >= 4 * 32769
    # pair-pass partials: 7 floats per row and column slab; one slab from 16384 rows on, 64-column slabs at 1000
    assert itb(32768) == 7 * 32768 * 4 and itb(16384) == 7 * 16384 * 4 and itb(1000) == 16 * 7 * 1000 * 4 and itb(2) >= 7 * 2 * 4
    one = ctypes.c_void_p(256)                                         # non-null, never dereferenced: every call is refused first
    assert h.wesup_tsne_sqdist(None, 8, 4, None, None) == -1
    for n, d in ((1, 4), (32769, 4), (8, 0), (8, 4097)):
        assert h.wesup_tsne_sqdist(one, n, d, one, None) == -1
    assert h.wesup_tsne_affinities(None, 8, 2.0, None, None, None, 0, None) == -1
    for n, perp in ((1, 0.5), (32769, 30.0), (8, 8.0), (8, 0.0), (8, -1.0), (8, float('nan'))):
        assert h.wesup_tsne_affinities(one, n, perp, one, one, one, 1 << 20, None) == -1
    assert h.wesup_tsne_affinities(one, 8, 2.0, one, one, one, aff(8) - 1, None) == -3
    assert h.wesup_tsne_iterate(None, None, None, None, None, 8, 1, 1.0, 0.5, 50.0, 0.01, None, 0, None) == -1
    ok = dict(n=8, iters=1, ex=1.0, mom=0.5, lr=50.0, mg=0.01)
    for bad in (dict(n=1), dict(n=32769), dict(iters=-1), dict(iters=65537), dict(ex=0.0), dict(mom=-0.1), dict(lr=0.0),
                dict(mg=-1.0), dict(lr=float('nan'))):
        a = dict(ok, **bad)
        assert h.wesup_tsne_iterate(one, one, one, one, one, a['n'], a['iters'], a['ex'], a['mom'], a['lr'], a['mg'], one, 1 << 30,
                                    None) == -1, bad
    assert h.wesup_tsne_iterate(one, one, one, one, one, 8, 1, 1.0, 0.5, 50.0, 0.01, one, itb(8) - 1, None) == -3


def test_kernels_use_fp32_valu_only_and_no_scratch(tmp_path):
    from wesup_amd import _lib
    objdump = '/opt/rocm/lib/llvm/bin/llvm-objdump'
    if not os.path.exists(objdump):
        pytest.skip('llvm-objdump not found')
    so = shutil.copy(_lib.LIB_PATH, tmp_path / 'lib.so')
    subprocess.run([objdump, '--offloading', str(so)], cwd=tmp_path, check=True, capture_output=True)
    found = {}
    for co in sorted(tmp_path.glob('lib.so.*gfx950')):
        name = None
        for line in subprocess.run([objdump, '-d', str(co)], check=True, capture_output=True, text=True).stdout.splitlines():
            m = re.match(r'^[0-9a-f]+ <(\S+)>:', line)
            if m:
                name = m.group(1) if re.search(r'ts_(sqdist|search|total|symmetrise|pair|update)_kernel', m.group(1)) else None
                if name:
                    found[name] = []
            elif name and line.startswith('\t'):
                found[name].append(line.strip().split()[0])
    assert len(found) == 8, sorted(found)                              # pair and update in two instantiations each
    for name, ops_ in found.items():
        assert ops_, name
        for op in ops_:
            assert not op.startswith(('scratch_', 'v_mfma', 'v_smfmac')) and 'atomic' not in op and 'f64' not in op, (name, op)


# ---------------------------------------------------------------- the program
def test_program_arguments():
    from wesup_amd import tsne as T
    a = T.parse_args(['data/test', '-c', 'ckpt.pth'])
    assert (a.data_dir, a.checkpoint, a.before, a.rescale_factor, a.images, a.perplexity, a.init, a.seed, a.output, a.plot) == (
        'data/test', 'ckpt.pth', None, 0.4, 1, 30.0, 'pca', 0, 'tsne.npz', None)
    a = T.parse_args(['d', '-c', 'c', '--before', 'b', '--rescale-factor', '0.5', '--images', '3', '--perplexity', '12', '--init',
                      'random', '--seed', '4', '-o', 'x.npz', '--plot', 'p.png'])
    assert (a.before, a.rescale_factor, a.images, a.perplexity, a.init, a.seed, a.output, a.plot) == ('b', 0.5, 3, 12.0, 'random', 4,
                                                                                                      'x.npz', 'p.png')
    with pytest.raises(SystemExit):
        T.parse_args(['d'])                                            # no checkpoint
    with pytest.raises(SystemExit):
        T.parse_args(['d', '-c', 'c', '--init', 'spectral'])


def test_program_writes_the_references_keys_with_a_stubbed_trainer(tmp_path, monkeypatch):
    from wesup_amd import tsne as T
    n = 40
    labels = torch.arange(n) % 2
    made = []

    def collect(trainer, dataset, k):
        made.append((trainer, k))
        return torch.full((n, 32), float(len(made))), labels

    class Stub(T.TSNE):
        def fit(self, X):
            self.embedding_ = X[:, :2] * 2
            self.kl_divergence_, self.n_iter_ = 0.25 * float(X[0, 0]), 999
            return self
    monkeypatch.setattr(T, 'collect_sp_features', collect)
    monkeypatch.setattr(T, 'TSNE', Stub)
    out = tmp_path / 't.npz'
    a = T.parse_args(['unused', '-c', 'after.pth', '--images', '2', '-o', str(out), '--plot', str(tmp_path / 'p.png')])
    T.run(a, make_trainer=lambda ckpt: ckpt, dataset=object())
    assert made == [(None, 2), ('after.pth', 2)]
    z = np.load(out)
    assert sorted(z.files) == ['after_x2d', 'before_x2d', 'kl_after', 'kl_before', 'n_iter', 'sp_labels']
    assert z['before_x2d'].shape == z['after_x2d'].shape == (n, 2) and (z['before_x2d'] == 2).all() and (z['after_x2d'] == 4).all()
    assert np.array_equal(z['sp_labels'], labels.numpy()) and z['kl_before'] == 0.25 and z['kl_after'] == 0.5
    assert z['n_iter'].tolist() == [999, 999]
    try:
        import matplotlib  # noqa: F401
        assert (tmp_path / 'p.png').stat().st_size > 0
    except ImportError:
        assert not (tmp_path / 'p.png').exists()
    # more rows than an exact embedding holds: refused with the count
    monkeypatch.setattr(T, 'collect_sp_features', lambda *a: (torch.zeros(T.MAX_ROWS + 1, 1), torch.zeros(T.MAX_ROWS + 1)))
    with pytest.raises(SystemExit, match=str(T.MAX_ROWS + 1)):
        T.run(a, make_trainer=lambda ckpt: ckpt, dataset=object())
