"""Inputs shared by tests/test_tsne_cpu.py and tests/test_tsne_gpu.py."""
import numpy as np

import _tsneref as R

# the kernels' tile sizes (csrc/tsne.hip): rows per block of the pair pass, columns per LDS chunk, tile of sqdist / symmetrise,
# slab alignment.  A slab is wider than one chunk from N = 2049 on (8 slabs of 320 columns).
ROWS, CHUNK, TILE, SLAB = 16, 256, 64, 64
SIZES = sorted({2, 4, 63, 64, 65, 257, 1000, 2049, ROWS - 1, ROWS, ROWS + 1, CHUNK - 1, CHUNK, CHUNK + 1, 2 * SLAB - 1, 2 * SLAB,
                2 * SLAB + 1})
DIMS = (1, 32, 33, 257)


def perplexity_for(n):
    return min(30.0, n / 3.0)


def clusters(seed, n, d, far=False, same=0):
    """X = relu(c[label] + 0.5 randn) around three centres c = 2 randn(3, d): centres, then labels, then noise from one stream.
    ``far``: row 0 at distance ~1e4 from all others; ``same``: the first ``same`` rows identical."""
    rs = np.random.RandomState(seed)
    c = 2.0 * rs.standard_normal((3, d))
    lab = rs.randint(0, 3, n)
    x = np.maximum(c[lab] + 0.5 * rs.standard_normal((n, d)), 0).astype(np.float32)
    if far:
        x[0] = x[0] + np.float32(1e4 / np.sqrt(d))
    if same:
        x[:same] = x[0]
    return x, lab


WHOLE_RUN_PERPLEXITY = {65: 20.0, 257: 30.0}
WHOLE_RUN_SIZES = (65, 257)       # the default schedule from start to end (tests/golden/tsne.npz, tools/make_tsne_golden.py)
STATE_ITERS = (1, 50, 300)        # the seed-0 trajectory's states kept there: tiny, exaggerated, spread


def start(n, seed=0):
    """scikit-learn's random start."""
    return 1e-4 * np.random.RandomState(seed).standard_normal((n, 2)).astype(np.float32)


def phase_of(it):
    """(exaggeration, momentum) of iteration ``it`` under the default schedule."""
    return (12.0, 0.5) if it < R.EXPLORATION_ITERS else (1.0, 0.8)
