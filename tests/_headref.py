"""fp64 statements of what the head kernels of csrc/loss.hip compute -- label propagation, the semi-supervised loss and its
gradient, the generic cross entropy, the SGD step and the accuracy / dice sums -- the anchor tests/test_head_branches_gpu.py holds
them to.  Plain numpy float64 (int64 for the metric sums); nothing here calls the library, wesup_amd.ops or the oracle
(tests/test_headref_cpu.py ties every function to oracle/wesup_oracle.py at small sizes).  Inputs are the float32 arrays the kernels
get; every scalar a kernel receives as a float (threshold, eps, lr, ...) enters as float64(float32(x)).

    propagate()      d_ij = sum_k (f_j,k - f_i,k)^2, W = exp(-d); src = FIRST labelled index of the row maximum; propagated iff
                     W > threshold (strict).  Defaults of every other row: own labels (labelled), zeros, src -1, max_sim 0.
    loss_terms()     terms[b] = {sup, #sup, prop, #prop, sum of pseudo labels, loss_b, 0, 0} and their mean over B
    loss_grad()      dloss * d mean_b(loss_b) / d pred, non-zero on the closed clamp interval [eps32, 1 - eps32] only
    cross_entropy()  {sum, #rows, loss, 0} of (n, C) with optional class weights, and its gradient
    sgd()            g' = g gs + wd p;  v = g' on the first step (v is not read), else mu v + g';  p -= lr v
    seg_sums()       {#(P == G), sum P G, sum P, sum G}, P = round-half-to-even(pred), G = first maximum over the mask planes

The "plain fp32 on the CPU" evaluations whose distance from fp64 sets the bars (4 x, capped) are here as well: *_fp32."""
import numpy as np
import torch

CAP_LOSS = 1e-5         # what test_propagate_and_loss / test_cross_entropy_generic demand of a loss, relative
CAP_SIM = 1e-5          # ... of max_sim
CAP_GRAD = 1e-4         # TOL of tests/test_kernels_gpu.py (dpred, dy_hat)
CAP_SGD = 1e-6          # test_sgd_and_metrics
PROP_TILE, PROP_ROWS = 256, 16      # csrc/loss.hip: labelled rows per LDS tile, rows per block (4 per wave, 64 lanes over j)
HEAD_LDS_MAX = 160 * 1024


def head_lds_bytes(D):
    """Dynamic LDS of the propagation kernel for a feature width D (prop_lds_bytes of csrc/loss.hip)."""
    return (PROP_TILE * (D + 1) + PROP_ROWS * D) * 4


def f32(x):
    return float(np.float32(x))


def clamp_bounds(eps):
    """(lo, hi) of the clamp as the kernels form them: float32(eps) and float32(1) - float32(eps), the difference rounded to float32."""
    e = np.float32(eps)
    return float(e), float(np.float32(1.0) - e)


def bar_from(cpu_figure, cap):
    return min(4.0 * float(cpu_figure), cap)


def rel_elem(got, ref):
    """max over the elements with ref != 0 of |got - ref| / |ref|; inf if an element with ref == 0 is not exactly 0, or a NaN of
    ref is not a NaN of got (0.0 for an empty tensor)."""
    got, ref = np.asarray(got, dtype=np.float64), np.asarray(ref, dtype=np.float64)
    if got.size == 0:
        return 0.0
    nan = np.isnan(ref)
    if not np.array_equal(nan, np.isnan(got)):
        return float('inf')
    z = (ref == 0) & ~nan
    if np.any(got[z] != 0):
        return float('inf')
    nz = ~z & ~nan
    return float((np.abs(got[nz] - ref[nz]) / np.abs(ref[nz])).max()) if nz.any() else 0.0


def rel_whole(got, ref):
    """The suite's whole-tensor norm: max |got - ref| / max |ref|."""
    got, ref = np.asarray(got, dtype=np.float64), np.asarray(ref, dtype=np.float64)
    if got.size == 0:
        return 0.0
    if np.isnan(got).any():
        return float('inf')
    return float(np.abs(got - ref).max() / max(np.abs(ref).max(), 1e-300))


# ---------------------------------------------------------------- propagation
def sqdist(feat_b, n_sp, n_l, dtype=np.float64):
    """d (n_sp - n_l, n_l): d_ij = sum_k (f_j,k - f_i,k)^2 in ascending k, unlabelled row i against labelled row j."""
    f = np.asarray(feat_b, dtype=dtype)
    d = np.zeros((n_sp - n_l, n_l), dtype=dtype)
    for k in range(f.shape[1]):
        t = f[None, :n_l, k] - f[n_l:n_sp, None, k]
        d += t * t
    return d


def propagate(feat, labels, n_sp, n_l, threshold, enable=True):
    """feat (B, Kmax, D), labels (B, Kmax, C) float32 -> y_all (B, Kmax, C) float64, src (B, Kmax) int64, max_sim (B, Kmax) float64."""
    feat, labels = np.asarray(feat), np.asarray(labels)
    B, Kmax, _ = feat.shape
    C = labels.shape[2]
    thr = float(np.float32(threshold))
    y = np.zeros((B, Kmax, C))
    src = np.full((B, Kmax), -1, dtype=np.int64)
    sim = np.zeros((B, Kmax))
    for b in range(B):
        ns, nl = int(n_sp[b]), int(n_l[b])
        y[b, :nl] = labels[b, :nl]
        if not enable or nl <= 0 or ns <= nl:
            continue
        W = np.exp(-sqdist(feat[b], ns, nl))
        j = np.argmax(W, axis=1)                                  # the first maximum
        w = W[np.arange(ns - nl), j]
        assert np.all(W[np.arange(ns - nl), j][:, None] >= W) and all(np.all(W[i, :j[i]] < w[i]) for i in range(ns - nl))
        src[b, nl:ns], sim[b, nl:ns] = j, w
        take = w > thr
        y[b, nl:ns][take] = labels[b, j[take]]
    return y, src, sim


def max_sim_fp32(feat, n_sp, n_l):
    """max_sim of the present unlabelled rows in numpy float32 (zeros elsewhere): direct differences, np.exp of float32."""
    feat = np.asarray(feat, dtype=np.float32)
    B, Kmax, _ = feat.shape
    sim = np.zeros((B, Kmax), dtype=np.float32)
    for b in range(B):
        ns, nl = int(n_sp[b]), int(n_l[b])
        if nl > 0 and ns > nl:
            sim[b, nl:ns] = np.exp(-sqdist(feat[b], ns, nl, np.float32)).max(axis=1)
    return sim


# ---------------------------------------------------------------- loss
def _ce_terms(p, y, eps, cw=None):
    """-y log(clamp(p)) [* cw] per element, float64; a NaN of p stays a NaN (torch.clamp keeps it)."""
    lo, hi = clamp_bounds(eps)
    p = np.asarray(p, dtype=np.float64)
    pc = np.where(np.isnan(p), p, np.minimum(np.maximum(p, lo), hi))
    ce = -np.asarray(y, dtype=np.float64) * np.log(pc)
    return ce if cw is None else ce * np.asarray(cw, dtype=np.float64)[None, :]


def loss_terms(pred, y_all, n_sp, n_l, eps, prop_weight):
    """pred, y_all (B, Kmax, C) float32 -> (terms (B, 8) float64, loss = mean_b terms[b][5])."""
    B = pred.shape[0]
    pw = f32(prop_weight)
    terms = np.zeros((B, 8))
    for b in range(B):
        ns, nl = int(n_sp[b]), int(n_l[b])
        ce = _ce_terms(pred[b, :ns], y_all[b, :ns], eps).sum(axis=1)
        ys = np.asarray(y_all[b, :ns], dtype=np.float64).sum(axis=1)
        sup, supc = ce[:nl].sum(), float((ys[:nl] > 0).sum())
        pro, proc, plab = ce[nl:].sum(), float((ys[nl:] > 0).sum()), ys[nl:].sum()
        l = sup / supc if supc > 0 else 0.0
        if nl < ns and proc > 0:
            l = l + pw * (pro / proc)
        terms[b, :6] = sup, supc, pro, proc, plab, l
    return terms, terms[:, 5].sum() / B


def loss_grad(pred, y_all, n_sp, n_l, eps, prop_weight, dloss):
    """dloss * d loss / d pred (B, Kmax, C) float64: -y / p on the closed interval [lo, hi], 0 outside it, for a NaN and beyond n_sp."""
    lo, hi = clamp_bounds(eps)
    B = pred.shape[0]
    pw, dl = f32(prop_weight), f32(dloss)
    terms, _ = loss_terms(pred, y_all, n_sp, n_l, eps, prop_weight)
    p = np.asarray(pred, dtype=np.float64)
    y = np.asarray(y_all, dtype=np.float64)
    g = np.zeros_like(p)
    for b in range(B):
        ns, nl = int(n_sp[b]), int(n_l[b])
        coef = np.zeros(p.shape[1])
        coef[:nl] = 1.0 / terms[b, 1] if terms[b, 1] > 0 else 0.0
        coef[nl:ns] = pw / terms[b, 3] if (nl < ns and terms[b, 3] > 0) else 0.0
        with np.errstate(divide='ignore', invalid='ignore'):
            inside = (p[b] >= lo) & (p[b] <= hi)
            g[b] = np.where(inside, dl / B * coef[:, None] * (-y[b] / p[b]), 0.0)
        g[b, ns:] = 0.0
    return g


def loss_fp32(pred, y_all, n_sp, n_l, eps, prop_weight, dloss):
    """The same in torch float32 on the CPU, the gradient by autograd: (terms (B, 8) float32 as numpy, loss, dpred)."""
    lo, hi = clamp_bounds(eps)
    p = torch.from_numpy(np.ascontiguousarray(pred)).clone().requires_grad_(True)
    y = torch.from_numpy(np.ascontiguousarray(y_all))
    B = p.shape[0]
    terms = np.zeros((B, 8), dtype=np.float32)
    losses = []
    for b in range(B):
        ns, nl = int(n_sp[b]), int(n_l[b])
        ce = (-y[b, :ns] * torch.log(torch.clamp(p[b, :ns], min=lo, max=hi))).sum(dim=1)
        ys = y[b, :ns].sum(dim=1)
        sup, supc = ce[:nl].sum(), (ys[:nl] > 0).sum().float()
        pro, proc = ce[nl:].sum(), (ys[nl:] > 0).sum().float()
        l = sup / supc if float(supc) > 0 else sup * 0.0
        if nl < ns and float(proc) > 0:
            l = l + f32(prop_weight) * (pro / proc)
        losses.append(l)
        terms[b, :6] = [float(x.detach()) for x in (sup, supc, pro, proc, ys[nl:].sum(), l)]
    loss = torch.stack(losses).mean()
    (loss * f32(dloss)).backward()
    return terms, float(loss.detach()), p.grad.numpy()


def terms_figure(got, ref):
    """Relative error of the three floating sums of every image (sup, prop, loss_b), the worst of them; inf if a count or the sum of
    the pseudo labels (small integers and halves: exact in float32) differs at all."""
    got, ref = np.asarray(got, dtype=np.float64), np.asarray(ref, dtype=np.float64)
    if not (np.array_equal(got[:, [1, 3, 4]], ref[:, [1, 3, 4]]) and np.array_equal(got[:, 6:], ref[:, 6:])):
        return float('inf')
    return rel_elem(got[:, [0, 2, 5]], ref[:, [0, 2, 5]])


# ---------------------------------------------------------------- generic cross entropy
def cross_entropy(y_hat, y_true, eps, cw=None, dloss=1.0):
    """(out (4,) float64 = {sum, #rows with sum(y) > 0, loss, 0}, dy (n, C) float64)."""
    lo, hi = clamp_bounds(eps)
    p = np.asarray(y_hat, dtype=np.float64)
    y = np.asarray(y_true, dtype=np.float64)
    s = _ce_terms(p, y, eps, cw).sum()
    cnt = float((y.sum(axis=1) > 0).sum())
    out = np.array([s, cnt, s / cnt if cnt > 0 else 0.0, 0.0])
    dy = np.zeros_like(p)
    if cnt > 0:
        with np.errstate(divide='ignore', invalid='ignore'):
            dy = np.where((p >= lo) & (p <= hi), f32(dloss) * (-y / p) / cnt, 0.0)
        if cw is not None:
            dy = dy * np.asarray(cw, dtype=np.float64)[None, :]
    return out, dy


def cross_entropy_fp32(y_hat, y_true, eps, cw=None, dloss=1.0):
    """torch float32 on the CPU: (sum, loss, dy)."""
    lo, hi = clamp_bounds(eps)
    p = torch.from_numpy(np.ascontiguousarray(y_hat)).clone().requires_grad_(True)
    y = torch.from_numpy(np.ascontiguousarray(y_true))
    ce = -y * torch.log(torch.clamp(p, min=lo, max=hi))
    if cw is not None:
        ce = ce * torch.from_numpy(np.ascontiguousarray(cw))[None, :]
    s = ce.sum()
    cnt = (y.sum(dim=1) > 0).sum().float()
    if float(cnt) == 0:
        return float(s.detach()), 0.0, np.zeros(p.shape, dtype=np.float32)
    loss = s / cnt
    (loss * f32(dloss)).backward()
    return float(s.detach()), float(loss.detach()), p.grad.numpy()


# ---------------------------------------------------------------- SGD
def sgd(p, g, v, lr, mu, wd, gs, first, dtype=np.float64):
    """One step on copies: (p, v) in ``dtype`` (float64: the reference; float32: the plain evaluation on the CPU, every product and
    sum rounded).  On the first step v is replaced, never read."""
    lr, mu, wd, gs = (dtype(np.float32(x)) for x in (lr, mu, wd, gs))
    p, g = np.asarray(p, dtype=dtype), np.asarray(g, dtype=dtype)
    gp = g * gs + wd * p
    v = gp.copy() if first else mu * np.asarray(v, dtype=dtype) + gp
    return p - lr * v, v


# ---------------------------------------------------------------- metric sums
def seg_sums(pred, mask):
    """pred (B, H, W) float32, mask (B, C, H, W) uint8 -> (B, 4) int64."""
    P = np.rint(np.asarray(pred, dtype=np.float64)).astype(np.int64)           # numpy rounds half to even
    m = np.asarray(mask)
    G = np.zeros(P.shape, dtype=np.int64)
    best = m[:, 0].astype(np.int64)
    for c in range(1, m.shape[1]):                                               # the FIRST maximum: a later plane must be larger
        up = m[:, c].astype(np.int64) > best
        G[up], best[up] = c, m[:, c].astype(np.int64)[up]
    B = P.shape[0]
    return np.stack([(P == G).reshape(B, -1).sum(1), (P * G).reshape(B, -1).sum(1), P.reshape(B, -1).sum(1), G.reshape(B, -1).sum(1)], axis=1)
