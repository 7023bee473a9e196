"""Exact t-SNE of superpixel features on the device (the reference's plot_tsne.py).

``TSNE`` follows ``sklearn.manifold.TSNE(method='exact')`` -- its perplexity search, its gradient, its delta-bar-delta update
and its schedule (250 iterations at exaggeration 12 and momentum 0.5, the rest at 1 and 0.8, a check every 50) -- with the
N x N work in csrc/tsne.hip: nothing falls back to the host.  The program embeds ``model.sp_features`` of the first K test
images before and after training and writes ``before_x2d``, ``after_x2d`` and ``sp_labels`` (the reference's keys):

    python -m wesup_amd.tsne DATA -c CKPT [--before CKPT0] [--rescale-factor 0.4] [--images K] [--perplexity P]
                                  [--init pca|random] [--seed S] [-o tsne.npz] [--plot PNG]
"""
import argparse
import sys

import numpy as np
import torch

from . import ops

EXPLORATION_ITERS = 250      # scikit-learn's _EXPLORATION_MAX_ITER: iterations under early exaggeration
N_ITER_CHECK = 50            # _N_ITER_CHECK: the stopping rules look at the KL divergence and |g| this often
MIN_GAIN = 0.01
MAX_ROWS = ops.TSNE_MAX_N


def auto_learning_rate(n, early_exaggeration):
    return max(n / early_exaggeration / 4.0, 50.0)


def descend(step, it, max_iter, n_iter_without_progress, min_grad_norm, n_iter_check=N_ITER_CHECK, history=None):
    """scikit-learn's ``_gradient_descent`` loop around ``step(k)``, which runs k iterations and returns (KL, |g|) as the last of
    them found them.  Iterations ``it .. max_iter - 1``; a check after every iteration i with (i + 1) % n_iter_check == 0: stop
    when the KL has not improved for more than ``n_iter_without_progress`` iterations or |g| <= ``min_grad_norm``.  Returns the
    index of the last iteration run.  ``history`` collects (i, KL, |g|) of every check."""
    best_error, best_iter, i = np.finfo(float).max, it, it
    while i < max_iter:
        last = min((i // n_iter_check + 1) * n_iter_check, max_iter) - 1      # the next check, or the end
        error, grad_norm = step(last - i + 1)
        i = last
        if (i + 1) % n_iter_check == 0:
            if history is not None:
                history.append((i, float(error), float(grad_norm)))
            if error < best_error:
                best_error, best_iter = error, i
            elif i - best_iter > n_iter_without_progress:
                break
            if grad_norm <= min_grad_norm:
                break
        i += 1
    return min(i, max_iter - 1)


def phases(max_iter, early_exaggeration, n_iter_without_progress):
    """scikit-learn's two calls of its descent: (last iteration + 1, exaggeration, momentum, patience)."""
    return [(EXPLORATION_ITERS, float(early_exaggeration), 0.5, EXPLORATION_ITERS),
            (int(max_iter), 1.0, 0.8, int(n_iter_without_progress))]


def random_init(n, random_state):
    """scikit-learn's draw: 1e-4 * standard_normal((n, 2)) as float32."""
    rs = random_state if isinstance(random_state, np.random.RandomState) else (
        np.random.mtrand._rand if random_state is None else np.random.RandomState(random_state))
    return 1e-4 * rs.standard_normal(size=(n, 2)).astype(np.float32)


def pca_init(x):
    """The first two principal components from the D x D covariance (host, float64), scaled so that the first has standard
    deviation 1e-4; each component's sign makes its largest entry of the axis positive."""
    x = np.asarray(x, dtype=np.float64)
    xc = x - x.mean(0)
    w, v = np.linalg.eigh(xc.T @ xc)
    axes = v[:, np.argsort(w)[::-1][:2]]
    if axes.shape[1] < 2:                                    # one feature: the second component is empty
        axes = np.concatenate([axes, np.zeros((axes.shape[0], 1))], 1)
    axes = axes * np.where(axes[np.abs(axes).argmax(0), np.arange(2)] < 0, -1.0, 1.0)
    y = xc @ axes
    sd = y[:, 0].std()
    return (y / (sd if sd > 0 else 1.0) * 1e-4).astype(np.float32)


def affinities(X, perplexity):
    """X (N, D) on the device -> (P (N, N), beta (N,))."""
    if not isinstance(X, torch.Tensor) or X.dim() != 2:
        raise ValueError('affinities: expected an (N, D) tensor')
    ops.tsne_check_shape(X.shape[0], X.shape[1], perplexity)
    d2 = ops.tsne_sqdist(X.detach().float().contiguous())
    return ops.tsne_affinities(d2, perplexity)


class TSNE:
    """``sklearn.manifold.TSNE(method='exact')`` on a device tensor.  ``init``: 'pca', 'random' or an (N, 2) array."""

    def __init__(self, perplexity=30.0, early_exaggeration=12.0, learning_rate='auto', max_iter=1000, n_iter_without_progress=300,
                 min_grad_norm=1e-7, init='pca', random_state=None, n_components=2):
        if n_components != 2:
            raise ValueError(f'n_components must be 2 (the kernels embed into the plane), got {n_components}')
        if isinstance(init, str) and init not in ('pca', 'random'):
            raise ValueError(f"init must be 'pca', 'random' or an (N, 2) array, got {init!r}")
        if learning_rate != 'auto' and not float(learning_rate) > 0:
            raise ValueError(f"learning_rate must be 'auto' or positive, got {learning_rate!r}")
        if int(max_iter) < EXPLORATION_ITERS:
            raise ValueError(f'max_iter must be at least {EXPLORATION_ITERS}, got {max_iter}')
        if not float(early_exaggeration) >= 1:
            raise ValueError(f'early_exaggeration must be at least 1, got {early_exaggeration}')
        self.perplexity, self.early_exaggeration = float(perplexity), float(early_exaggeration)
        self.learning_rate, self.max_iter = learning_rate, int(max_iter)
        self.n_iter_without_progress, self.min_grad_norm = int(n_iter_without_progress), float(min_grad_norm)
        self.init, self.random_state, self.n_components = init, random_state, 2
        self.embedding_ = self.kl_divergence_ = self.n_iter_ = self.learning_rate_ = None
        self.stats_history_ = []

    def _initial(self, X):
        n = X.shape[0]
        if isinstance(self.init, str):
            return random_init(n, self.random_state) if self.init == 'random' else pca_init(X.cpu().numpy())
        y = self.init.detach().cpu().numpy() if isinstance(self.init, torch.Tensor) else np.asarray(self.init)
        if y.shape != (n, 2):
            raise ValueError(f'init must be ({n}, 2), got {y.shape}')
        return y.astype(np.float32)

    def fit(self, X):
        if not isinstance(X, torch.Tensor) or X.dim() != 2:
            raise ValueError('TSNE.fit: expected an (N, D) tensor')
        n, d = X.shape
        ops.tsne_check_shape(n, d, self.perplexity)
        X = X.detach().float().contiguous()
        P, _ = affinities(X, self.perplexity)
        dev = X.device
        y = torch.from_numpy(np.ascontiguousarray(self._initial(X))).to(dev)
        upd, gains = torch.zeros_like(y), torch.ones_like(y)
        stats = torch.zeros(ops.TSNE_STATS, dtype=torch.float32, device=dev)
        self.learning_rate_ = auto_learning_rate(n, self.early_exaggeration) if self.learning_rate == 'auto' else float(self.learning_rate)
        self.stats_history_ = []
        it = -1
        for end, exaggeration, momentum, patience in phases(self.max_iter, self.early_exaggeration, self.n_iter_without_progress):
            if it + 1 >= end:
                continue
            upd.zero_(); gains.fill_(1.0)                   # scikit-learn starts each of its two descents from these

            def step(k, exaggeration=exaggeration, momentum=momentum):
                ops.tsne_iterate(P, y, upd, gains, stats, k, exaggeration, momentum, self.learning_rate_, MIN_GAIN)
                s = stats.cpu()                              # the one synchronisation of a check
                return float(s[0]), float(s[1])
            it = descend(step, it + 1, end, patience, self.min_grad_norm, history=self.stats_history_)
        ops.tsne_iterate(P, y, upd, gains, stats, 0, 1.0, 0.8, self.learning_rate_, MIN_GAIN)
        self.kl_divergence_ = float(stats.cpu()[0])          # of the embedding returned (scikit-learn's is one update older)
        self.n_iter_ = it
        self.embedding_ = y
        return self

    def fit_transform(self, X):
        return self.fit(X).embedding_


def collect_sp_features(trainer, dataset, k):
    """``model.sp_features`` and ``sp_labels.argmax(1)`` of the first ``k`` images of ``dataset`` under their full masks (every
    superpixel labelled), concatenated on the device: ((sum N, D) float32, (sum N,) int64)."""
    if dataset.mask_paths is None:
        raise ValueError('collect_sp_features: the dataset has no masks to label the superpixels with')
    feats, labels = [], []
    trainer.model.eval()
    for i in range(min(int(k), len(dataset))):
        img, mask = dataset.to_reference_item(dataset[i])
        (x, sp_maps), (_, sp_labels) = trainer.preprocess(img.unsqueeze(0), mask.unsqueeze(0))
        with torch.no_grad():
            trainer.model((x, sp_maps))
        meta = sp_maps.meta
        n, n_l = int(meta.n_sp[0]), int(meta.n_l[0])
        if n_l != n:
            raise RuntimeError(f'image {i}: {n - n_l} of {n} superpixels without a label under the full mask')
        f = trainer.model.sp_features
        f = f[0] if f.dim() == 3 else f
        feats.append(f[:n].detach().clone())
        labels.append(meta.sp_labels[0, :n].argmax(1))
    return torch.cat(feats), torch.cat(labels)


def parse_args(argv=None):
    ap = argparse.ArgumentParser(prog='python -m wesup_amd.tsne', description=__doc__.split('\n')[0])
    ap.add_argument('data_dir', metavar='DATA')
    ap.add_argument('-c', '--checkpoint', required=True, help='the trained model')
    ap.add_argument('--before', help='checkpoint of the model before training (default: the model as constructed)')
    ap.add_argument('--rescale-factor', type=float, default=0.4)
    ap.add_argument('--images', type=int, default=1, help='embed the superpixels of the first K images')
    ap.add_argument('--perplexity', type=float, default=30.0)
    ap.add_argument('--init', choices=('pca', 'random'), default='pca')
    ap.add_argument('--seed', type=int, default=0)
    ap.add_argument('--max-iter', type=int, default=1000)
    ap.add_argument('--device', default='cuda')
    ap.add_argument('-o', '--output', default='tsne.npz')
    ap.add_argument('--plot', metavar='PNG')
    return ap.parse_args(argv)


def plot(path, before, after, labels):
    try:
        import matplotlib
        matplotlib.use('Agg')
        import matplotlib.pyplot as plt
    except ImportError:
        print(f'cannot draw {path}: matplotlib is not installed', file=sys.stderr)
        return False
    fig, (ax1, ax2) = plt.subplots(1, 2, figsize=(10, 5))
    ax1.scatter(before[:, 0], before[:, 1], c=labels, alpha=0.3)
    ax1.set_title('before training')
    ax2.scatter(after[:, 0], after[:, 1], c=labels, alpha=0.3)
    ax2.set_title('after training')
    fig.savefig(path)
    plt.close(fig)
    return True


def run(a, make_trainer=None, dataset=None):
    """The program behind ``main``: ``make_trainer(checkpoint or None)`` and ``dataset`` can be handed in (tests)."""
    if make_trainer is None:
        def make_trainer(ckpt):
            from .models import initialize_trainer
            trainer = initialize_trainer('wesup', device=a.device)
            if ckpt:
                trainer.load_checkpoint(ckpt)
            return trainer
    if dataset is None:
        from .utils.data import SegmentationDataset
        dataset = SegmentationDataset(a.data_dir, rescale_factor=a.rescale_factor, train=False)
    out, labels = {}, None
    for name, ckpt in (('before', a.before), ('after', a.checkpoint)):
        feats, lab = collect_sp_features(make_trainer(ckpt), dataset, a.images)
        if feats.shape[0] > MAX_ROWS:
            raise SystemExit(f'{feats.shape[0]} superpixels in {a.images} image(s): an exact embedding holds at most {MAX_ROWS} '
                             '(fewer --images, or a smaller --rescale-factor)')
        if labels is not None and not torch.equal(lab, labels):
            raise RuntimeError('the two models saw different superpixels')
        labels = lab
        t = TSNE(perplexity=a.perplexity, init=a.init, random_state=a.seed, max_iter=a.max_iter)
        out[name] = (t.fit_transform(feats).cpu().numpy(), t.kl_divergence_, t.n_iter_)
    res = dict(before_x2d=out['before'][0], after_x2d=out['after'][0], sp_labels=labels.cpu().numpy(),
               kl_before=np.float64(out['before'][1]), kl_after=np.float64(out['after'][1]),
               n_iter=np.array([out['before'][2], out['after'][2]], dtype=np.int64))
    np.savez(a.output, **res)
    print(f"{a.output}: {len(res['sp_labels'])} superpixels; KL before {res['kl_before']:.4f}, after {res['kl_after']:.4f}")
    if a.plot:
        plot(a.plot, res['before_x2d'], res['after_x2d'], res['sp_labels'])
    return res


def main(argv=None):
    run(parse_args(argv))


if __name__ == '__main__':
    main()
