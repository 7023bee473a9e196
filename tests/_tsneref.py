"""numpy restatement of csrc/tsne.hip and of the schedule in wesup_amd/tsne.py: squared distances from differences, the shifted
perplexity search and the joint P, the one-pass gradient and KL divergence, the delta-bar-delta update, the two-phase schedule
with its stopping rules.  ``dtype=np.float64`` is the reference the device is held to; the same code under ``np.float32`` is the
yardstick for what single precision costs (tests/test_tsne_gpu.py takes its bars from it)."""
import numpy as np

EPS = 2.220446049250313e-16
SEARCH_STEPS = 100
SEARCH_TOL = 1e-5
EXPLORATION_ITERS = 250
N_ITER_CHECK = 50
MIN_GAIN = 0.01


def sqdist(x, dtype=np.float64):
    x = np.asarray(x, dtype=dtype)
    n, d = x.shape
    out = np.zeros((n, n), dtype=dtype)
    for k in range(d):                                        # ascending k, as the kernel adds them
        df = x[:, k, None] - x[None, :, k]
        out += df * df
    np.fill_diagonal(out, 0)
    return out


def _shifted(d2, dtype):
    d2 = np.asarray(d2, dtype=dtype)
    n = d2.shape[0]
    off = ~np.eye(n, dtype=bool)
    m = np.where(off, d2, np.inf).min(1)
    dd = d2 - m[:, None]
    np.fill_diagonal(dd, 0)                                   # (never used; keeps exp(-beta dd) finite there)
    return dd, off


def row_entropy(d2, beta, dtype=np.float64):
    """H_i of the conditional row built with beta_i (invariant under the shift)."""
    dd, off = _shifted(d2, dtype)
    e = np.where(off, np.exp(-np.asarray(beta, dtype=dtype)[:, None] * dd), 0).astype(dtype)
    s = e.sum(1)
    return np.log(s) + np.asarray(beta, dtype=dtype) * (dd * e).sum(1) / s


def search(d2, perplexity, dtype=np.float64):
    """scikit-learn's _binary_search_perplexity on the shifted rows, all rows at once -> beta (the value each row's C uses)."""
    dd, off = _shifted(d2, dtype)
    n = dd.shape[0]
    target = dtype(np.log(dtype(perplexity)))
    beta = np.ones(n, dtype=dtype)
    lo, hi = np.full(n, -np.inf, dtype=dtype), np.full(n, np.inf, dtype=dtype)
    used = beta.copy()
    live = np.ones(n, dtype=bool)
    for _ in range(SEARCH_STEPS):
        idx = np.nonzero(live)[0]
        if idx.size == 0:
            break
        b = beta[idx]
        e = np.where(off[idx], np.exp(-b[:, None] * dd[idx]), 0).astype(dtype)
        s = e.sum(1)
        diff = np.log(s) + b * (dd[idx] * e).sum(1) / s - target
        used[idx] = b
        done = np.abs(diff) <= dtype(SEARCH_TOL)
        live[idx[done]] = False
        up = diff > 0
        for sel, bound, other, grow in ((up & ~done, lo, hi, dtype(2)), (~up & ~done, hi, lo, dtype(0.5))):
            j = idx[sel]
            bound[j] = beta[j]
            free = np.isinf(other[j])
            beta[j] = np.where(free, beta[j] * grow, (beta[j] + np.where(free, 0, other[j])) * dtype(0.5))
    return used


def joint(d2, beta, dtype=np.float64):
    """P = max((C + C^T) / max(sum, eps), eps) with the diagonal 0, C the conditional rows under ``beta``."""
    dd, off = _shifted(d2, dtype)
    e = np.where(off, np.exp(-np.asarray(beta, dtype=dtype)[:, None] * dd), 0).astype(dtype)
    c = e / e.sum(1, keepdims=True)
    p = c + c.T
    p = np.maximum(p / max(p.sum(), dtype(EPS)), dtype(EPS))
    np.fill_diagonal(p, 0)
    return p.astype(dtype)


def affinities(x, perplexity, dtype=np.float64):
    d2 = sqdist(x, dtype)
    beta = search(d2, perplexity, dtype)
    return joint(d2, beta, dtype), beta


def gradient(p, y, exaggeration=1.0, dtype=np.float64):
    """One pass over the pairs -> (g (n, 2), KL of the UNexaggerated p, Z).  g = 4 (att - rep / Z)."""
    p, y = np.asarray(p, dtype=dtype), np.asarray(y, dtype=dtype)
    n = y.shape[0]
    off = ~np.eye(n, dtype=bool)
    df = y[:, None, :] - y[None, :, :]
    num = (dtype(1) / (dtype(1) + (df * df).sum(-1))).astype(dtype)
    att = ((dtype(exaggeration) * p * num)[..., None] * df).sum(1)
    rep = ((num * num)[..., None] * df).sum(1)
    Z = np.where(off, num, 0).sum(dtype=dtype)
    g = dtype(4) * (att - rep / Z)
    pc = np.maximum(p, dtype(EPS))
    kl = np.where(off, pc * np.log(pc), 0).sum(dtype=dtype) - np.where(off, pc * np.log(num), 0).sum(dtype=dtype) + np.log(Z)
    return g.astype(dtype), dtype(kl), dtype(Z)


def update(g, y, upd, gains, momentum, lr, min_gain=MIN_GAIN, dtype=np.float64):
    """scikit-learn's delta-bar-delta step -> (y, upd, gains), new arrays."""
    g, y, upd, gains = (np.asarray(a, dtype=dtype) for a in (g, y, upd, gains))
    inc = upd * g < 0
    gains = np.maximum(np.where(inc, gains + dtype(0.2), gains * dtype(0.8)), dtype(min_gain)).astype(dtype)
    upd = (dtype(momentum) * upd - dtype(lr) * (g * gains)).astype(dtype)
    return (y + upd).astype(dtype), upd, gains


def iterate(p, y, upd, gains, iters, exaggeration, momentum, lr, min_gain=MIN_GAIN, dtype=np.float64):
    """``iters`` iterations -> (y, upd, gains, (KL, |g|, Z) of the last iteration's starting point)."""
    y, upd, gains = (np.asarray(a, dtype=dtype).copy() for a in (y, upd, gains))
    stats = None
    for _ in range(iters):
        g, kl, Z = gradient(p, y, exaggeration, dtype)
        stats = (float(kl), float(np.sqrt((g.astype(np.float64) ** 2).sum())), float(Z))
        y, upd, gains = update(g, y, upd, gains, momentum, lr, min_gain, dtype)
    return y, upd, gains, stats


def descend(step, it, max_iter, n_iter_without_progress, min_grad_norm, n_iter_check=N_ITER_CHECK):
    """scikit-learn's _gradient_descent control flow, one iteration at a time: ``step(check)`` runs one iteration and returns
    (KL, |g|) -- the KL only means something when ``check`` is set.  Returns the index of the last iteration run."""
    best_error, best_iter, i = np.finfo(float).max, it, it
    for i in range(it, max_iter):
        check = (i + 1) % n_iter_check == 0
        error, grad_norm = step(check)
        if check:
            if error < best_error:
                best_error, best_iter = error, i
            elif i - best_iter > n_iter_without_progress:
                break
            if grad_norm <= min_grad_norm:
                break
    return i


def run(p, y0, n, early_exaggeration=12.0, learning_rate='auto', max_iter=1000, n_iter_without_progress=300, min_grad_norm=1e-7,
        dtype=np.float64, keep=()):
    """The whole schedule -> (y, KL of y, n_iter, {iteration: (y, upd, gains) at its start for the iterations in ``keep``})."""
    lr = max(n / early_exaggeration / 4.0, 50.0) if learning_rate == 'auto' else float(learning_rate)
    state = {'y': np.asarray(y0, dtype=dtype).copy(), 'i': 0}
    kept = {}
    it = -1
    for end, ex, mom, patience in ((EXPLORATION_ITERS, early_exaggeration, 0.5, EXPLORATION_ITERS),
                                   (max_iter, 1.0, 0.8, n_iter_without_progress)):
        if it + 1 >= end:
            continue
        state['upd'], state['gains'] = np.zeros_like(state['y']), np.ones_like(state['y'])
        state['i'] = it + 1

        def step(check, ex=ex, mom=mom):
            if state['i'] in keep:
                kept[state['i']] = (state['y'].copy(), state['upd'].copy(), state['gains'].copy())
            g, kl, _ = gradient(p, state['y'], ex, dtype)
            state['y'], state['upd'], state['gains'] = update(g, state['y'], state['upd'], state['gains'], mom, lr, MIN_GAIN, dtype)
            state['i'] += 1
            return float(kl), float(np.sqrt((g.astype(np.float64) ** 2).sum()))
        it = descend(step, it + 1, end, patience, min_grad_norm)
    _, kl, _ = gradient(p, state['y'], 1.0, dtype)
    return state['y'], float(kl), it, kept


def knn_purity(y, labels, k=5):
    """Share of the points whose k nearest embedded neighbours all carry the point's own label."""
    y = np.asarray(y, dtype=np.float64)
    d = ((y[:, None] - y[None]) ** 2).sum(-1)
    np.fill_diagonal(d, np.inf)
    nn = np.argsort(d, 1, kind='stable')[:, :k]
    lab = np.asarray(labels)
    return float((lab[nn] == lab[:, None]).all(1).mean())
