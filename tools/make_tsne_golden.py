"""Writes tests/golden/tsne.npz: recorded results of the fp64 restatement (tests/_tsneref.py) on the whole-run cases of
tests/test_tsne_gpu.py, which take too long to recompute in the suite (N = 257: 8 s per run).  For N = 65 (perplexity 20) and
N = 257 (perplexity 30), clusters of RandomState(7) at D = 32:
  kl_N, purity_N      final KL divergence and 5-neighbour label purity of the default schedule from the random starts of seeds 0 - 4
  y_N_I, upd_N_I, gains_N_I   the seed-0 trajectory's state at the start of iterations I = 1, 50, 300
  xsum_N              sum of the inputs in float64 (the generator must not drift)

    python tools/make_tsne_golden.py
"""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, 'tests'))

import _tsneref as R  # noqa: E402
from _tsnecases import STATE_ITERS, WHOLE_RUN_PERPLEXITY, WHOLE_RUN_SIZES, clusters  # noqa: E402


def main():
    out = {}
    for n in WHOLE_RUN_SIZES:
        x, lab = clusters(7, n, 32)
        P, _ = R.affinities(x, WHOLE_RUN_PERPLEXITY[n])
        kls, pur = [], []
        for seed in range(5):
            y0 = 1e-4 * np.random.RandomState(seed).standard_normal((n, 2)).astype(np.float32)
            y, kl, it, kept = R.run(P, y0, n, keep=STATE_ITERS if seed == 0 else ())
            kls.append(kl)
            pur.append(R.knn_purity(y, lab))
            if seed == 0:
                for i, (yy, uu, gg) in kept.items():
                    out[f'y_{n}_{i}'], out[f'upd_{n}_{i}'], out[f'gains_{n}_{i}'] = yy, uu, gg
            print(f'N = {n} seed {seed}: KL {kl:.6f}, purity {pur[-1]:.4f}, n_iter {it}')
        out[f'kl_{n}'], out[f'purity_{n}'] = np.array(kls), np.array(pur)
        out[f'xsum_{n}'] = np.float64(x.astype(np.float64).sum())
    path = os.path.join(ROOT, 'tests', 'golden', 'tsne.npz')
    np.savez_compressed(path, **out)
    print(path, os.path.getsize(path), 'bytes')


if __name__ == '__main__':
    main()
