"""Times of the exact t-SNE (csrc/tsne.hip, wesup_amd/tsne.py) at N = 1000, 4096 and 16384 superpixels of D = 32 features:
``sqdist``, ``affinities``, one gradient iteration (pair pass + update, from a run of 100 enqueued at once), the pair pass's
rate on the bytes it must read (4 N^2 per iteration: P once), and a whole default run (1000 iterations, checks included).  For
N = 1000 also the host: ``sklearn.manifold.TSNE(method='exact')`` when scikit-learn can be imported, otherwise the fp64
restatement of tests/_tsneref.py.

  python tools/tsne_micro.py [--sizes 1000 4096 16384] [--out profiles/tsne_micro.txt]

Every stage warm, host clock around work that ends in a device synchronise; iterations are timed mid-schedule (a spread
embedding, exaggeration 1) as well as at the start, since nothing in the kernels depends on the values."""
import argparse
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tests'))
D = 32


def _cpu_model():
    try:
        for line in open('/proc/cpuinfo'):
            if line.startswith('model name'):
                return line.split(':', 1)[1].strip()
    except OSError:
        pass
    return 'unknown'


def _features(n):
    rs = np.random.RandomState(7)
    c = 2.0 * rs.standard_normal((3, D))
    return np.maximum(c[rs.randint(0, 3, n)] + 0.5 * rs.standard_normal((n, D)), 0).astype(np.float32)


def _timed(fn, sync, reps):
    fn()
    times = []
    for _ in range(reps):
        sync()
        t0 = time.perf_counter()
        fn()
        sync()
        times.append(time.perf_counter() - t0)
    return statistics.median(times), min(times), max(times)


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.split('\n')[0])
    ap.add_argument('--sizes', type=int, nargs='+', default=[1000, 4096, 16384])
    ap.add_argument('--out')
    a = ap.parse_args(argv)
    import torch
    if not torch.cuda.is_available():
        raise SystemExit('tsne_micro.py measures the device path: it needs a GPU')
    from wesup_amd import ops, tsne as T
    dev = torch.device('cuda:0')
    sync = torch.cuda.synchronize
    lines = ['exact t-SNE on the device, seconds: median (min .. max)',
             f'host: {_cpu_model()}, {len(os.sched_getaffinity(0))} CPUs available to the process',
             f'device: {torch.cuda.get_device_name(0)}', f'features: three ReLU clusters, D = {D}, perplexity 30', '']
    for n in a.sizes:
        x = torch.from_numpy(_features(n)).to(dev)
        d2 = ops.tsne_sqdist(x)
        t_sq = _timed(lambda: ops.tsne_sqdist(x, out=d2), sync, 5)
        P, beta = ops.tsne_affinities(d2, 30.0)
        t_aff = _timed(lambda: ops.tsne_affinities(d2, 30.0, p=P, beta=beta), sync, 3)
        y = torch.from_numpy(T.random_init(n, 0)).to(dev)
        upd, gains, stats = torch.zeros_like(y), torch.ones_like(y), torch.zeros(ops.TSNE_STATS, device=dev)
        lr = T.auto_learning_rate(n, 12.0)
        K = 100
        t_early = _timed(lambda: ops.tsne_iterate(P, y, upd, gains, stats, K, 12.0, 0.5, lr, 0.01), sync, 3)
        t_late = _timed(lambda: ops.tsne_iterate(P, y, upd, gains, stats, K, 1.0, 0.8, lr, 0.01), sync, 3)
        t_eval = _timed(lambda: ops.tsne_iterate(P, y, upd, gains, stats, 0, 1.0, 0.8, lr, 0.01), sync, 5)
        run = T.TSNE(init='random', random_state=0)
        t0 = time.perf_counter()
        run.fit(x)
        sync()
        t_run = time.perf_counter() - t0
        per = t_late[0] / K
        lines += [f'N = {n}',
                  f'  sqdist                        {t_sq[0]:.6f} ({t_sq[1]:.6f} .. {t_sq[2]:.6f})',
                  f'  affinities (search + joint P) {t_aff[0]:.6f} ({t_aff[1]:.6f} .. {t_aff[2]:.6f})',
                  f'  iteration, exaggerated start  {t_early[0] / K:.7f} ({t_early[1] / K:.7f} .. {t_early[2] / K:.7f})  [{K} per call]',
                  f'  iteration, spread embedding   {per:.7f} ({t_late[1] / K:.7f} .. {t_late[2] / K:.7f})  [{K} per call]',
                  f'  pair pass + update on 4 N^2 = {4 * n * n / 1e6:.1f} MB of P: {4 * n * n / per / 1e9:.0f} GB/s, '
                  f'{n * (n - 1) / per / 1e9:.1f} G pairs/s',
                  f'  evaluation (iters = 0: KL, |g|, Z; logs in the pair pass) {t_eval[0]:.6f}',
                  f'  whole default run             {t_run:.3f}  (n_iter_ {run.n_iter_}, KL {run.kl_divergence_:.4f}, '
                  f'{len(run.stats_history_)} checks)', '']
        if n == 1000:
            xh = x.cpu().numpy()
            try:
                from sklearn.manifold import TSNE as SK
                t0 = time.perf_counter()
                sk = SK(method='exact', init='random', random_state=0).fit(xh)
                t_host = time.perf_counter() - t0
                lines += [f'  host, sklearn.manifold.TSNE(method=\'exact\'): {t_host:.2f} s (n_iter_ {sk.n_iter_}, KL '
                          f'{sk.kl_divergence_:.4f}); host / device: {t_host / t_run:.0f}', '']
            except ImportError:
                import _tsneref as R
                t0 = time.perf_counter()
                Ph, _ = R.affinities(xh, 30.0)
                _, kl, it, _ = R.run(Ph, T.random_init(n, 0), n)
                lines += [f'  host, fp64 numpy restatement (scikit-learn is not installed): {time.perf_counter() - t0:.2f} s (n_iter {it}, '
                          f'KL {kl:.4f})', '']
        del d2, P, x
        torch.cuda.empty_cache()
    text = '\n'.join(lines)
    print(text)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, 'w') as f:
            f.write(text + '\n')


if __name__ == '__main__':
    main()
