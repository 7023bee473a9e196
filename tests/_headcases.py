"""Case lists and seeded builders of tests/test_head_branches_gpu.py (reference: tests/_headref.py).  Every builder asserts, on the
CPU, the conditions that make its case decidable; tests/test_headref_cpu.py runs every one of them.

Propagation features are multiples of 1/8 in [0, 1] ([0, 1/2] above D = 64): a squared difference is a multiple of 1/64 and at most
1, a sum of D of them at most 64 -- d is EXACT in float32 as in float64, both agree on every ordering and on every tie, distinct d
differ by >= 1/64 (exp(-d) by 1.5 %: no two distinct d share an expf value, and exp(-64) = 1.6e-28 is a normal float32), and no
exp(-d) lies within 1e-4 of the threshold 0.8 (the nearest are d = 14/64 and 15/64: 0.8035 and 0.7911).  So src_idx and y_all are
compared exactly, every row of them."""
import functools

import numpy as np

import _headref as hr

SENTINEL = -777.25
ABSENT = 7.0                 # what sp_labels holds in rows at and beyond n_l (the kernels never read them)

# ---------------------------------------------------------------- propagation
N_L = (0, 1, 15, 16, 17, 63, 64, 65, 255, 256, 257, 513)          # 513: three tiles, the last holding one row
N_U = (0, 1, 5, 16, 40)                                            # n_sp - n_l
THR = 0.8
# (id, D, C, Kmax, fused): Kmax 553 = the largest n_sp (513 + 40), 563 and 571 beyond every n_sp and no multiple of 16; the fused
# entries need Kmax % 64 == 0 for the classifier's backward only, they are compared where the step runs them (576, 640)
PROP = [('D1-C2-K563', 1, 2, 563, False), ('D7-C3-K553', 7, 3, 553, False), ('D32-C2-K553', 32, 2, 553, False),
        ('D32-C16-K571', 32, 16, 571, False), ('D33-C3-K563', 33, 3, 563, False), ('D64-C2-K563', 64, 2, 563, False),
        ('D128-C16-K553', 128, 16, 553, False), ('D149-C3-K563', 149, 3, 563, False),
        ('fused-D32-C2-K576', 32, 2, 576, True), ('fused-D7-C3-K640', 7, 3, 640, True), ('fused-D64-C16-K576', 64, 16, 576, True),
        ('fused-D128-C2-K576', 128, 2, 576, True)]
D_REFUSED = 150             # 164 224 bytes of LDS: beyond the CU's 160 KiB, refused on the host
TIE_NL, TIE_NU = 513, 8     # the image of planted ties (every D >= 32)


def _grid(D):
    """Number of eighths the features of width D are drawn from: 0 ... 8 (values in [0, 1]), 0 ... 4 above D = 64 (d <= D / 4)."""
    return 8 if D <= 64 else 4


def _labels(rng, n, C):
    """(n, C) one-hot rows, every seventh a soft 0.5 / 0.5 row."""
    y = np.zeros((n, C), dtype=np.float32)
    c = rng.integers(0, C, n)
    y[np.arange(n), c] = 1.0
    soft = np.arange(n) % 7 == 3
    y[soft] = 0.0
    y[soft, c[soft]] = 0.5
    y[soft, (c[soft] + 1) % C] = 0.5
    return y


def _features(rng, nl, nu, D, pooled):
    """(nl + nu, D) in eighths.  Labelled rows: random, or (pooled) copies of 37 prototypes -- rows j and j + 37 k are then equal and
    ties are everywhere.  Unlabelled rows: a labelled row with a row-specific share of its entries moved by 1/8 or 2/8 (near and
    far neighbours: both sides of the threshold), every fifth one random."""
    q = _grid(D)
    ql = q if D >= 8 else 2             # (narrow features: labelled rows from the low end, or no random row would be far from all)
    lab = rng.integers(0, ql + 1, (nl, D))
    if pooled and nl:
        lab = rng.integers(0, ql + 1, (37, D))[np.arange(nl) % 37]
    un = rng.integers(0, q + 1, (nu, D))
    for i in range(nu):
        if nl and i % 5 != 4:
            base = lab[rng.integers(0, nl)]
            move = rng.random(D) < rng.random() ** 3 * 0.6
            step = rng.integers(1, 3, D) * rng.choice([-1, 1], D)
            cand = base + np.where(move, step, 0)
            un[i] = np.where((cand < 0) | (cand > q), base - np.where(move, step, 0), cand)
    return (np.concatenate([lab, un]) / 8.0).astype(np.float32)


def _tie_image(rng, D, C):
    """513 labelled + 8 unlabelled rows with the planted ties; returns (feat, labels, winners {unlabelled row: labelled index})."""
    q = _grid(D)
    nl, nu = TIE_NL, TIE_NU
    lab = rng.integers(0, q + 1, (nl, D))
    un = np.zeros((nu, D), dtype=np.int64)

    def near(j):                        # labelled row j with entry 0 moved by one eighth: d = 1/64
        r = lab[j].copy()
        r[0] += 1 if r[0] < q else -1
        return r
    lab[69] = lab[5];   un[0] = near(5)          # j and j + 64: the same lane, a later trip
    lab[11] = lab[10];  un[1] = near(10)         # j and j + 1: neighbouring lanes
    lab[276] = lab[20]; un[2] = near(20)         # j and j + 256: the next tile
    un[3] = near(512)                            # the winner sits alone in the ragged last tile
    lab[64] = lab[63];  un[4] = near(63)         # lane 63 and lane 0 of the next trip
    un[5] = lab[30]                              # a duplicate of a labelled row: W = 1.0 exactly
    lab[300] = lab[44]; lab[500] = lab[44]; un[6] = near(44)     # three equal rows over two tiles
    un[7] = near(200)                            # a plain unique winner
    winners = {0: 5, 1: 10, 2: 20, 3: 512, 4: 63, 5: 30, 6: 44, 7: 200}
    y = _labels(rng, nl, C)
    for a, b in ((5, 69), (10, 11), (20, 276), (63, 64), (44, 300), (44, 500)):   # the loser of a tie carries another label
        y[a], y[b] = 0.0, 0.0
        y[a, a % C], y[b, (a + 1) % C] = 1.0, 1.0
    return (np.concatenate([lab, un]) / 8.0).astype(np.float32), y, winners


@functools.lru_cache(maxsize=None)
def prop_case(i):
    """The batch of case PROP[i]: one image per (n_l, n_sp - n_l) of N_L x N_U (60), plus the tie image from D = 32 on.  Returns a
    dict: feat (B, Kmax, D), labels (B, Kmax, C), n_sp, n_l (B,) int32, tie (index of the tie image or None), winners."""
    name, D, C, Kmax, fused = PROP[i]
    rng = np.random.default_rng(1000 + i)
    shapes = [(nl, nu) for nl in N_L for nu in N_U]
    tie = len(shapes) if D >= 32 else None
    B = len(shapes) + (tie is not None)
    feat = (rng.integers(0, _grid(D) + 1, (B, Kmax, D)) / 8.0).astype(np.float32)      # rows beyond n_sp: plausible features
    labels = np.full((B, Kmax, C), ABSENT, dtype=np.float32)
    n_sp, n_l = np.zeros(B, dtype=np.int32), np.zeros(B, dtype=np.int32)
    for b, (nl, nu) in enumerate(shapes):
        feat[b, :nl + nu] = _features(rng, nl, nu, D, pooled=(b % 2 == 1))
        labels[b, :nl] = _labels(rng, nl, C)
        n_sp[b], n_l[b] = nl + nu, nl
    winners = None
    if tie is not None:
        f, y, winners = _tie_image(rng, D, C)
        feat[tie, :TIE_NL + TIE_NU], labels[tie, :TIE_NL] = f, y
        n_sp[tie], n_l[tie] = TIE_NL + TIE_NU, TIE_NL
    case = dict(name=name, D=D, C=C, Kmax=Kmax, fused=fused, feat=feat, labels=labels, n_sp=n_sp, n_l=n_l, tie=tie, winners=winners)
    check_prop_case(case)
    return case


def check_prop_case(c):
    """The conditions under which src_idx and y_all are decidable exactly (module docstring), asserted image by image."""
    assert hr.head_lds_bytes(c['D']) <= hr.HEAD_LDS_MAX
    assert c['Kmax'] >= int(c['n_sp'].max()) and (c['Kmax'] % 64 == 0 if c['fused'] else c['Kmax'] % 16 != 0) and c['Kmax'] <= 640
    lo_thr, hi_thr = hr.f32(THR) * (1 - 1e-4), hr.f32(THR) * (1 + 1e-4)
    n_prop = n_not = n_tied = 0
    for b in range(len(c['n_sp'])):
        ns, nl = int(c['n_sp'][b]), int(c['n_l'][b])
        assert 0 <= nl <= ns <= c['Kmax']
        if nl == 0 or ns == nl:
            continue
        d = hr.sqdist(c['feat'][b], ns, nl)
        d32 = hr.sqdist(c['feat'][b], ns, nl, np.float32)
        assert d.max() <= 64.0 and np.array_equal(d * 64, np.round(d * 64)) and np.array_equal(d32.astype(np.float64), d)
        w = np.exp(-d.min(axis=1))
        assert not np.any((w > lo_thr) & (w < hi_thr))
        n_prop += int((w > hr.f32(THR)).sum())
        n_not += int((w <= hr.f32(THR)).sum())
        n_tied += int(((d == d.min(axis=1, keepdims=True)).sum(axis=1) > 1).sum())
    assert n_prop >= 20 and n_not >= 20 and n_tied >= 20, (c['name'], n_prop, n_not, n_tied)
    if c['tie'] is not None:
        b = c['tie']
        d = hr.sqdist(c['feat'][b], TIE_NL + TIE_NU, TIE_NL)
        mates = {0: (5, 69), 1: (10, 11), 2: (20, 276), 3: (512,), 4: (63, 64), 5: (30,), 6: (44, 300, 500), 7: (200,)}
        for i, js in mates.items():
            best = d[i].min()
            assert best == (0.0 if i == 5 else 1.0 / 64)
            assert tuple(np.flatnonzero(d[i] == best)) == js and c['winners'][i] == js[0]          # a tie in fp64, and only these
            for a in js[1:]:
                assert not np.array_equal(c['labels'][b, a], c['labels'][b, js[0]])


# ---------------------------------------------------------------- loss
EPS = 1e-7
LOSS_B, LOSS_KMAX, LOSS_D = 6, 640, 32
LOSS_NSP = (0, 1, 255, 256, 257, 600)
LOSS_NL = {'A': (0, 1, 100, 0, 257, 300), 'B': (0, 0, 255, 17, 64, 600)}     # 0, a part of n_sp, n_sp itself
# (id, C, n_l pattern, prop_weight, dloss)
LOSS = [('C2-A-w0.5', 2, 'A', 0.5, 1.7), ('C2-B-w0.25', 2, 'B', 0.25, 0.3), ('C3-A-w0.25', 3, 'A', 0.25, 1.7),
        ('C3-B-w0.5', 3, 'B', 0.5, 0.3), ('C16-A-w0.5', 16, 'A', 0.5, 0.3), ('C16-B-w0.25', 16, 'B', 0.25, 1.7)]


def planted_values():
    """name -> (float32 prediction, whether the gradient passes): the two clamp bounds, their outer neighbours, 0 and 1."""
    lo, hi = (np.float32(x) for x in hr.clamp_bounds(EPS))
    return {'eps': (lo, True), 'below_eps': (np.nextafter(lo, np.float32(0)), False), 'one_minus_eps': (hi, True),
            'above_one_minus_eps': (np.nextafter(hi, np.float32(2)), False), 'zero': (np.float32(0), False), 'one': (np.float32(1), False)}


@functools.lru_cache(maxsize=None)
def loss_case(i, nan=False):
    """pred, y_all (6, 640, C) float32 with garbage beyond n_sp, n_sp / n_l, feat / Wc for the fused backward, and ``planted``:
    name -> (b, r, c, gradient passes).  Labelled rows: one-hot, soft, every ninth all-zero (not counted); pseudo labels: one-hot,
    soft or zero; image 2 of pattern A has no pseudo label at all (#prop = 0)."""
    name, C, pat, pw, dloss = LOSS[i]
    rng = np.random.default_rng(2000 + i)
    B, Kmax = LOSS_B, LOSS_KMAX
    n_sp, n_l = np.array(LOSS_NSP, dtype=np.int32), np.array(LOSS_NL[pat], dtype=np.int32)
    z = rng.standard_normal((B, Kmax, C)) * 2.0
    pred = (np.exp(z) / np.exp(z).sum(axis=2, keepdims=True)).astype(np.float32)
    y = np.full((B, Kmax, C), 3.0, dtype=np.float32)                   # beyond n_sp: nothing of it may arrive anywhere
    for b in range(B):
        ns, nl = int(n_sp[b]), int(n_l[b])
        y[b, :ns] = _labels(rng, ns, C)
        y[b, :nl][np.arange(nl) % 9 == 4] = 0.0
        un = np.arange(ns - nl)
        y[b, nl:ns][un % 3 == 1] = 0.0
        if pat == 'A' and b == 2:
            y[b, nl:ns] = 0.0
    # the planted predictions: image 5 (n_sp = 600), a labelled and -- pattern A -- an unlabelled row each, at a class whose label is
    # not zero in a counted row, so that the gradient there is zero for one reason only: the clamp
    planted = {}
    b = 5
    nl = int(n_l[b])
    rows = [r for r in range(nl) if y[b, r].sum() > 0][:6] + [r for r in range(nl, int(n_sp[b])) if y[b, r].sum() > 0][:6]
    vals = planted_values()
    for k, r in enumerate(rows):
        nm = list(vals)[k % 6]
        c = int(np.argmax(y[b, r]))
        pred[b, r, c] = vals[nm][0]
        planted[(nm, 'labelled' if r < nl else 'unlabelled')] = (b, r, c, vals[nm][1])
    if nan:
        pred[4, 3, 0] = np.nan                                          # present row of image 4 (n_sp = 257)
    feat = np.maximum(rng.standard_normal((B * Kmax, LOSS_D)), 0).astype(np.float32)
    Wc = (rng.standard_normal((C, LOSS_D)) * 0.3).astype(np.float32)
    case = dict(name=name, C=C, pw=pw, dloss=dloss, pred=pred, y_all=y, n_sp=n_sp, n_l=n_l, planted=planted, feat=feat, Wc=Wc)
    check_loss_case(case, pat)
    return case


def check_loss_case(c, pat):
    assert len(c['planted']) == (12 if pat == 'A' else 6)              # pattern B: image 5 is fully labelled
    terms, loss = hr.loss_terms(np.nan_to_num(c['pred'], nan=0.5), c['y_all'], c['n_sp'], c['n_l'], EPS, c['pw'])
    for (nm, where), (b, r, cc, passes) in c['planted'].items():
        assert c['y_all'][b, r, cc] > 0 and terms[b, 1 if where == 'labelled' else 3] > 0
    assert any(terms[b, 1] < c['n_l'][b] for b in range(LOSS_B))       # all-zero labelled rows are there and not counted
    if pat == 'A':
        assert terms[2, 3] == 0 and c['n_l'][2] < c['n_sp'][2]          # unlabelled rows, none with a pseudo label
    assert c['dloss'] != 1.0 and np.isfinite(loss)


# ---------------------------------------------------------------- generic cross entropy
CE_N = (0, 1, 255, 256, 257, 1000)                                      # 0: forward only
# (id, C, class weights, all rows unlabelled)
CE = [('C2', 2, False, False), ('C2-w', 2, True, False), ('C5', 5, False, False), ('C5-w', 5, True, False), ('C16', 16, False, False),
      ('C16-w', 16, True, False), ('C5-none', 5, False, True)]


@functools.lru_cache(maxsize=None)
def ce_case(i, n):
    name, C, weighted, none = CE[i]
    rng = np.random.default_rng(3000 + 10 * i + n)
    z = rng.standard_normal((n, C)) * 2.0
    y_hat = (np.exp(z) / np.exp(z).sum(axis=1, keepdims=True)).astype(np.float32)
    y = _labels(rng, n, C)
    y[np.arange(n) % 4 == 2] = 0.0
    if none:
        y[:] = 0.0
    vals = planted_values()
    for k, nm in enumerate(vals):                                       # the clamp edges again, where there are rows for them
        r = 4 * k + 1
        if r < n and not none:
            y_hat[r, int(np.argmax(y[r]))] = vals[nm][0]
    cw = (0.5 + rng.random(C)).astype(np.float32) if weighted else None
    assert none == (float((y.sum(axis=1) > 0).sum()) == 0) or n < 2
    return dict(y_hat=y_hat, y_true=y, cw=cw, dloss=0.6)


# ---------------------------------------------------------------- SGD
SGD_SMALL = (1, 2, 3, 4, 5, 7, 1023, 1024, 1025)
SGD_WRAP = 2048 * 256 * 4 + 1200          # floats: the capped grid (2048 x 256 threads, a float4 each) takes a second trip
SGD_LARGE = tuple(SGD_WRAP + k for k in range(4))                      # tails of 0, 1, 2, 3 floats
# (id, lr, momentum, weight_decay, grad_scale)
SGD_HYPER = {'plain': (5e-2, 0.9, 1e-3, 0.5), 'wd0': (5e-2, 0.9, 0.0, 0.5), 'mu0': (5e-2, 0.0, 1e-3, 1.0)}


def sgd_inputs(n, seed):
    """p and the three steps' gradients, float32.  (lr is 5e-2, a thousand times the step's: at 5e-5 an error in v would hide
    below the rounding of p.)"""
    rng = np.random.default_rng(4000 + seed)
    return rng.standard_normal(n).astype(np.float32), [rng.standard_normal(n).astype(np.float32) for _ in range(3)]


def sgd_reference(p0, gs3, hyper, dtype=np.float64):
    """Three steps from p0; v enters the first step as NaN and must leave no trace.  Returns [(p, v) after each step]."""
    lr, mu, wd, gs = hyper
    p, v = np.asarray(p0, dtype=dtype), np.full(len(p0), np.nan, dtype=dtype)
    out = []
    for step, g in enumerate(gs3):
        p, v = hr.sgd(p, g, v, lr, mu, wd, gs, step == 0, dtype)
        out.append((p, v))
    assert all(np.isfinite(a).all() and np.isfinite(b).all() for a, b in out)
    return out


# ---------------------------------------------------------------- metric sums
SEG_HW = (1, 255, 256, 257, 16383, 16384, 16385, 2 * 16384 + 3)         # 64 blocks x 256 threads = 16384 pixels per trip
SEG = [(hw, C, B) for hw in SEG_HW for C, B in ((2, 1), (3, 3), (16, 1))] + [(2 * 16384 + 3, 16, 3), (257, 2, 3)]


@functools.lru_cache(maxsize=None)
def seg_case(i):
    """pred (B, 1, HW) float32 with halves (0.5 -> 0, 1.5 -> 2, 2.5 -> 2), mask (B, C, 1, HW) uint8 in 0 ... 3: ties between planes
    in most pixels, the first plane of the maximum wins."""
    HW, C, B = SEG[i]
    rng = np.random.default_rng(5000 + i)
    pred = (rng.random((B, 1, HW)) * (C - 0.51)).astype(np.float32)
    halves = np.array([0.5, 1.5, 2.5], dtype=np.float32)
    pos = np.arange(HW) % 5 == 0
    pred[:, 0, pos] = halves[np.arange(int(pos.sum())) % 3][None, :]
    mask = rng.integers(0, 4, (B, C, 1, HW)).astype(np.uint8)
    mask[:, :, 0, np.arange(HW) % 11 == 0] = 2                            # every plane equal: class 0
    ref = hr.seg_sums(pred, mask)
    assert ref.max() < 2 ** 24                                            # the float sums of the kernel are exact integers
    m = mask[:, :, 0].astype(np.int64)
    assert HW < 8 or np.any((m == m.max(axis=1, keepdims=True)).sum(axis=1) > 1)
    return pred, mask, ref
