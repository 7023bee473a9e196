"""Label propagation, the semi-supervised loss and its gradient, the generic cross entropy, SGD and the accuracy / dice sums
(csrc/loss.hip) where their loops wrap, each against an fp64 statement of the same operation (tests/_headref.py), never against
another kernel or the fp32 oracle.  The case lists and their seeded builders are tests/_headcases.py; tests/test_headref_cpu.py
holds the reference to oracle/wesup_oracle.py and runs every builder without a GPU.  (The classifier kernels have their own fp64
checks in tests/test_multiclass_gpu.py.)

Measure and bar.  Integer and label outputs (src_idx, y_all, the counts and the pseudo-label sum of terms, the four metric sums)
are compared for equality, every element: the propagation features are eighths, so d is exact in float32 and float64 alike and no
row is a near-tie (tests/_headcases.py states and asserts the conditions).  Every element of every floating-point output is
compared as well: where the reference is exactly zero (padded rows, absent images, clamped predictions) the output must be exactly
zero, elsewhere the figure is the largest relative error of an element (max_sim, dpred, dy_hat, the three floating sums of every
image's terms, the losses) or, for SGD, the suite's whole-tensor norm max |gpu - ref| / max |ref|.  The bar of a figure is 4 x the
same figure of a plain fp32 evaluation on the CPU of exactly these inputs (numpy float32 for max_sim and SGD, torch float32 with
autograd for the losses and gradients) and never above what the existing tests use: 1e-5 for a loss and for max_sim, 1e-4 (TOL) for
dpred / dy_hat, 1e-6 for SGD.  The factor 4 allows another legitimate order of the same sums (256 threads striding over the rows and
a tree, against torch's vectorised sum) and a contracted multiply-add.  A figure belongs to one launch, or to the launches of one
list where a single launch is too small to have a stable fp32 figure: the n of one cross-entropy configuration, the small n of one
SGD configuration (their outputs count as one tensor).  Both figures go through tests/_tol.within.

Every case's HIP figure beside its fp32-CPU figure and bar: profiles/tolerances_head_branches.json; the worst of each class is at the end
of this docstring.

Which case reaches which branch (ids as pytest prints them):

  prop_kernel / prop_c_kernel, one body (wesup_propagate: C = 2, 3, 16 through prop_kernel; ops.head_fwd calls wesup_head_fwd_c:
  prop_kernel with the two-class tail at C = 2, prop_c_kernel with cls_row beyond).  Every case is a batch of 60 images, one per
  (n_l, n_sp - n_l) of
  {0, 1, 15, 16, 17, 63, 64, 65, 255, 256, 257, 513} x {0, 1, 5, 16, 40}, plus the image of planted ties from D = 32 on:
    no labelled row (nl <= 0: early return)          n_l = 0, every n_sp - n_l
    no unlabelled row / block wholly labelled        n_sp - n_l = 0; every block below n_l - 16
    block straddling labelled | unlabelled           n_l = 1, 15, 17, 63, 65, 255, 257, 513 (n_l % 16 != 0); on the boundary: 16, 64, 256
    block straddling present | absent, wholly absent n_sp % 16 != 0 (most); i_blk >= n_sp: every image, Kmax = 553 ... 640 > n_sp
    last block cut by Kmax (r < Kmax)                Kmax = 553, 563, 571 (not a multiple of 16); Kmax == n_sp: the 513 + 40 image at 553
    lanes with no j (nj < 64), one trip, several     n_l = 1, 15, 16, 17, 63 | 64 | 65, 255, 256
    second and third LDS tile, ragged last tile      n_l = 257 (1 row), 513 (256 + 256 + 1)
    in-lane tie, later trip (j, j + 64)              tie image row 0; the pooled images (odd index: labelled rows repeat every 37)
    neighbouring lanes (j, j + 1)                    tie image row 1
    next tile (j, j + 256), three-way over two tiles tie image rows 2 and 6
    winner alone in the ragged last tile             tie image row 3 (j = 512)
    lane 63 and lane 0 of the next trip              tie image row 4
    W = 1.0 exactly, threshold 1.0 / below 1.0       tie image row 5 (test_threshold_is_strict_at_w_equal_one)
    D = 1, 7, 32, 33 (default LDS), 64, 128, 149     the -D<n>- part of the id; from D = 60 the raised LDS limit, 149 is the last that fits
    D = 150                                          test_too_wide_features_are_refused_on_the_host: return code only, nothing launched
    the raised limit inside a whole training step    test_a_model_of_64_features_trains_a_step_like_the_oracle (WESUP(D=64) against the oracle)
    enable = 0                                       every case (second half of test_propagation_against_fp64)
  loss_fwd_kernel / loss_bwd_kernel / head_bwd_kernel / head_bwd_c_kernel (head_bwd_body<2> at C = 2, <0> beyond): B = 6,
    Kmax = 640, n_sp = 0, 1, 255, 256, 257, 600 (no trip,
    part of one, one less than / exactly / one more than a trip of 256 threads, three trips), n_l = 0 | part | n_sp (patterns A, B),
    all-zero labelled rows, an image without any pseudo label, the six clamp-edge predictions in a labelled and an unlabelled row,
    garbage beyond n_sp; the fused launches bit for bit against the unfused ones on the same inputs; one NaN (test_nan_...)
  ce_fwd_kernel / ce_bwd_kernel: n = 0 (forward only), 1, 255, 256, 257, 1000; C = 2, 5, 16; with and without weights; no labelled row
  sgd_kernel: n = 1, 2, 3 (tail only, n4 = 0), 4 (no tail), 5, 7, 1023, 1024, 1025; 2048 * 256 * 4 + 1200 + k: the capped grid's second
    trip (300 float4) with tails of k = 0 ... 3; v = NaN before the first step; weight_decay = 0; momentum = 0; a misaligned view
  seg_metrics_kernel: HW = 1, 255, 256, 257 (one block, part / all / one more), 16383, 16384, 16385 (all 64 blocks: one trip less one,
    exactly, one more), 2 * 16384 + 3 (third trip); C = 2, 3, 16 with ties between planes; B = 1, 3; halves

Measured on the MI355X, worst case of each class, HIP | fp32 on the CPU (every bar is 4 x the CPU figure of its own case; no cap binds):
  max_sim             6.9e-8 | 1.6e-7      (expf against numpy's float32 exp)
  loss terms          1.2e-7 | 1.5e-7      loss (mean over B)  4.4e-8 | 4.4e-8
  dpred               2.3e-7 | 1.2e-7      (dloss * (1 / B) * coef * (-y / p): four roundings against autograd's three)
  cross entropy       1.5e-7 | 1.4e-7      dy_hat              1.6e-7 | 1.3e-7
  SGD p               1.3e-7 | 1.3e-7      SGD v               7.7e-8 | 1.1e-7   (g gs + wd p contracted to one rounding on the GPU)
  src_idx, y_all, counts, pseudo-label sums, metric sums: equal.
"""
from types import SimpleNamespace

import numpy as np
import pytest
import torch

import _headcases as hc
import _headref as hr
from _tol import within

pytestmark = pytest.mark.gpu

S = hc.SENTINEL
S_INT = -777
WESUP_ERR_INVALID = -1


def dev():
    assert torch.cuda.is_available(), 'GPU tests need a GPU'
    return torch.device('cuda:0')


@pytest.fixture(scope='module')
def ops():
    from wesup_amd import ops as o
    return o


def t(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(dev())


def meta_of(labels, n_sp, n_l):
    """What the wrappers read of a preprocessing result: B, Kmax, C, sp_labels, n_sp, n_l."""
    B, Kmax, C = labels.shape
    return SimpleNamespace(B=B, Kmax=Kmax, C=C, sp_labels=t(labels), n_sp=t(n_sp.astype(np.int32)), n_l=t(n_l.astype(np.int32)))


def sentinels(B, Kmax, C):
    d = dev()
    return (torch.full((B, Kmax, C), S, device=d), torch.full((B, Kmax), S_INT, dtype=torch.int32, device=d), torch.full((B, Kmax), S, device=d))


def figure(case, what, got, ref, cpu, cap, measure=hr.rel_elem):
    """Records the HIP figure beside the fp32-CPU figure of the same inputs (printed before anything is asserted) and returns
    (ok, text)."""
    f_cpu, f_hip = measure(cpu, ref), measure(got, ref)
    bar = hr.bar_from(f_cpu, cap)
    text = f'{case}: {what} HIP {f_hip:.3e}, fp32 CPU {f_cpu:.3e}, bar {bar:.3e}'
    print(text)
    within(case, f'{what}, fp32 on the CPU vs fp64', f_cpu, cap)
    return within(case, f'{what}, HIP vs fp64', f_hip, bar, 'bar = min(4 x the fp32-CPU figure of the case, cap)'), text


_PROP_REF = {}


def prop_reference(i):
    if i not in _PROP_REF:
        c = hc.prop_case(i)
        _PROP_REF[i] = hr.propagate(c['feat'], c['labels'], c['n_sp'], c['n_l'], hc.THR) + (hr.max_sim_fp32(c['feat'], c['n_sp'], c['n_l']),)
    return _PROP_REF[i]


def assert_prop_outputs(c, out, ref, case):
    """y_all and src_idx exactly, every row; max_sim exactly zero outside the present unlabelled rows, within the bar inside."""
    y, src, sim, sim32 = ref
    gy, gs, gm = (o.cpu().numpy() for o in out)
    bad = np.flatnonzero((gs != src).any(axis=1))
    assert bad.size == 0, (case, 'src_idx', [(int(b), int(c['n_l'][b]), int(c['n_sp'][b])) for b in bad[:5]])
    assert np.array_equal(gy.astype(np.float64), y), (case, 'y_all', np.argwhere(gy != y)[:5].tolist())
    ok, text = figure(case, 'max_sim', gm, sim, sim32, hr.CAP_SIM)
    assert ok, text


# ---------------------------------------------------------------- propagation
@pytest.mark.parametrize('i', range(len(hc.PROP)), ids=[c[0] for c in hc.PROP])
def test_propagation_against_fp64(ops, i):
    c = hc.prop_case(i)
    ref = prop_reference(i)
    d = dev()
    B, Kmax, C, D = len(c['n_sp']), c['Kmax'], c['C'], c['D']
    m = meta_of(c['labels'], c['n_sp'], c['n_l'])
    feat = t(c['feat'])
    out = sentinels(B, Kmax, C)
    ops.propagate(feat, m, hc.THR, out=out)
    assert_prop_outputs(c, out, ref, c['name'])
    if c['tie'] is not None:                                             # the planted ties, by name
        src = out[1][c['tie'], hc.TIE_NL:hc.TIE_NL + hc.TIE_NU].cpu().tolist()
        assert src == [c['winners'][k] for k in range(hc.TIE_NU)], src
    again = sentinels(B, Kmax, C)
    ops.propagate(feat, m, hc.THR, out=again)
    assert all(torch.equal(a, b) for a, b in zip(out, again))            # two calls, bit-equal
    if c['fused']:
        # classifier + propagation in one launch: against fp64 like the unfused entry, and bit for bit the two entries
        rng = np.random.default_rng(i)
        Wc, bc = t((rng.standard_normal((C, D)) * 0.3).astype(np.float32)), t(rng.standard_normal(C).astype(np.float32))
        pred = torch.full((B * Kmax, C), S, device=d)
        fused = sentinels(B, Kmax, C)
        ops.head_fwd(feat, Wc, bc, pred, m, hc.THR, out=fused)
        assert_prop_outputs(c, fused, ref, c['name'] + '/head_fwd')
        assert all(torch.equal(a, b) for a, b in zip(out, fused))
        assert torch.equal(pred, ops.classifier_fwd(feat.view(B * Kmax, D), Wc, bc)) and bool(torch.isfinite(pred).all())
    # enable = 0: the defaults and nothing else
    off = sentinels(B, Kmax, C)
    ops.propagate(feat, m, hc.THR, enable=False, out=off)
    y0, src0, sim0 = hr.propagate(c['feat'], c['labels'], c['n_sp'], c['n_l'], hc.THR, enable=False)
    assert np.array_equal(off[0].cpu().numpy(), y0) and np.array_equal(off[1].cpu().numpy(), src0) and np.array_equal(off[2].cpu().numpy(), sim0)


@pytest.mark.parametrize('i', [2, 5], ids=[hc.PROP[2][0], hc.PROP[5][0]])
def test_threshold_is_strict_at_w_equal_one(ops, i):
    """An unlabelled row that duplicates a labelled one has W = exp(-0) = 1.0 exactly: not propagated under threshold 1.0, propagated
    under the largest float below 1.0; every other row of the image is below both."""
    c = hc.prop_case(i)
    b = c['tie']
    sl = slice(b, b + 1)
    m = meta_of(c['labels'][sl], c['n_sp'][sl], c['n_l'][sl])
    below = np.nextafter(np.float32(1), np.float32(0))
    for thr in (1.0, float(below)):
        out = sentinels(1, c['Kmax'], c['C'])
        ops.propagate(t(c['feat'][sl]), m, thr, out=out)
        y, src, sim = hr.propagate(c['feat'][sl], c['labels'][sl], c['n_sp'][sl], c['n_l'][sl], thr)
        assert np.array_equal(out[0].cpu().numpy(), y) and np.array_equal(out[1].cpu().numpy(), src)
        assert float(out[2][0, hc.TIE_NL + 5]) == 1.0
        assert int(np.count_nonzero(y[0, hc.TIE_NL:].sum(axis=1))) == (0 if thr == 1.0 else 1)


def test_too_wide_features_are_refused_on_the_host(ops):
    """D = 150 needs 164 224 bytes of LDS, more than a CU has: the three entries return WESUP_ERR_INVALID and launch nothing."""
    from wesup_amd import _lib
    from wesup_amd.ops import _p, _stream
    D, B, Kmax, C = hc.D_REFUSED, 1, 32, 2
    assert hr.head_lds_bytes(D) > hr.HEAD_LDS_MAX >= hr.head_lds_bytes(D - 1) and D == ops.HEAD_MAX_D + 1
    d = dev()
    feat = torch.zeros(B, Kmax, D, device=d)
    m = meta_of(np.zeros((B, Kmax, C), dtype=np.float32), np.array([20]), np.array([10]))
    Wc, bc, pred = torch.zeros(C, D, device=d), torch.zeros(C, device=d), torch.full((B * Kmax, C), S, device=d)
    out = sentinels(B, Kmax, C)
    lib = _lib.load()
    tail = (_p(m.sp_labels), _p(m.n_sp), _p(m.n_l), 0.8, 1, _p(out[0]), _p(out[1]), _p(out[2]), B, Kmax, D, C, _stream())
    assert lib.wesup_propagate(_p(feat), *tail) == WESUP_ERR_INVALID
    assert lib.wesup_head_fwd(_p(feat), _p(Wc), _p(bc), _p(pred), *tail) == WESUP_ERR_INVALID
    assert lib.wesup_head_fwd_c(_p(feat), _p(Wc), _p(bc), _p(pred), *tail) == WESUP_ERR_INVALID
    with pytest.raises(_lib.WesupHipError):
        ops.propagate(feat, m, 0.8, out=out)
    torch.cuda.synchronize()
    fresh = sentinels(B, Kmax, C)
    assert all(torch.equal(a, b) for a, b in zip(out, fresh)) and torch.equal(pred, torch.full_like(pred, S))


def test_a_model_of_64_features_trains_a_step_like_the_oracle():
    """WESUP(D=64): the head of the whole step runs through the raised LDS limit (the step of __graft_entry__.smoke at D = 64, its bar)."""
    from oracle import wesup_oracle as orc
    from wesup_amd import synth
    from wesup_amd.models import initialize_trainer
    from wesup_amd.utils.metrics import accuracy, dice
    dev()
    D = 64
    assert hr.head_lds_bytes(D) > 64 * 1024
    weights = orc.make_weights(3, D=D, feat_scale=0.03)
    imgs, labs, pts, pix = synth.make_batch(9, 2, 64, 64, 6)
    ref_loss, _, ref_new, _, _, _ = orc.train_step(weights, imgs, labs.astype(np.int64), pts.astype(np.int64))
    trainer = initialize_trainer('wesup', device='cuda:0', D=D)
    trainer.model.load_state_dict({k: torch.from_numpy(v) for k, v in weights.items()})
    trainer.optimizer, trainer.scheduler = trainer.get_default_optimizer()
    trainer.metric_funcs = [accuracy, dice]
    trainer.tracker.train()
    trainer.train_one_iteration('train', torch.from_numpy(imgs), torch.from_numpy(pix).long(), torch.from_numpy(pts).long(), torch.from_numpy(labs))
    loss = trainer.tracker.history['loss'][0]
    print(f'D = 64: loss {loss!r}, oracle {ref_loss!r}')
    assert within('model-D64', 'loss of a step at D = 64 vs the oracle', abs(loss - ref_loss) / abs(ref_loss), 1e-4, 'the bar of smoke()')


# ---------------------------------------------------------------- loss
def _run_loss(ops, c):
    m = meta_of(np.zeros((hc.LOSS_B, hc.LOSS_KMAX, c['C']), dtype=np.float32), c['n_sp'], c['n_l'])
    d = dev()
    pred, y_all = t(c['pred']), t(c['y_all'])
    terms, loss = torch.full((hc.LOSS_B, 8), S, device=d), torch.full((1,), S, device=d)
    ops.loss_fwd(pred, y_all, m, hc.EPS, c['pw'], out=(loss, terms))
    dloss = torch.tensor([c['dloss']], device=d)
    dpred = torch.full_like(pred, S)
    ops.loss_bwd(pred, y_all, m, terms, dloss, hc.EPS, c['pw'], out=dpred)
    return m, pred, y_all, terms, loss, dloss, dpred


def _same_bits(a, b):
    """torch.equal with a NaN equal to a NaN (the NaN case: its payload is nobody's promise)."""
    return torch.equal(a.isnan(), b.isnan()) and torch.equal(a.nan_to_num(nan=0.0), b.nan_to_num(nan=0.0))


def _fused_equals_unfused(ops, c, m, pred, y_all, terms, dloss, dpred):
    """wesup_head_bwd_c (+ the finish; head_bwd_kernel at C = 2, head_bwd_c_kernel beyond) on the same inputs: terms, dpred, dfeat,
    dWc, dbc bit for bit what loss_fwd,
    loss_bwd and classifier_bwd give -- the fp64 result of the unfused entries covers the fused ones."""
    d = dev()
    B, Kmax, C, D = hc.LOSS_B, hc.LOSS_KMAX, c['C'], hc.LOSS_D
    R = B * Kmax
    feat, Wc = t(c['feat']), t(c['Wc'])
    dfeat, dWc, dbc = ops.classifier_bwd(feat, Wc, pred.view(R, C), dpred.view(R, C))
    terms2, dpred2 = torch.full((B, 8), S, device=d), torch.full((B, Kmax, C), S, device=d)
    dfeat2, dWc2, dbc2 = torch.full((R, D), S, device=d), torch.full((C, D), S, device=d), torch.full((C,), S, device=d)
    part = ops.head_bwd_partials(R, D, d, C)
    ops.head_bwd(feat, Wc, pred.view(R, C), y_all, m, dloss, hc.EPS, c['pw'], terms2, dpred2, dfeat2, part)
    ops.classifier_bwd_finish(part, R, D, dWc2, dbc2)
    assert _same_bits(terms2, terms) and _same_bits(dpred2, dpred)
    assert _same_bits(dfeat2, dfeat) and _same_bits(dWc2, dWc) and _same_bits(dbc2, dbc)
    assert float(dfeat.abs().nan_to_num().max()) > 0


@pytest.mark.parametrize('i', range(len(hc.LOSS)), ids=[c[0] for c in hc.LOSS])
def test_loss_and_its_gradient_against_fp64(ops, i):
    c = hc.loss_case(i)
    m, pred, y_all, terms, loss, dloss, dpred = _run_loss(ops, c)
    ref_t, ref_l = hr.loss_terms(c['pred'], c['y_all'], c['n_sp'], c['n_l'], hc.EPS, c['pw'])
    ref_g = hr.loss_grad(c['pred'], c['y_all'], c['n_sp'], c['n_l'], hc.EPS, c['pw'], c['dloss'])
    t32, l32, g32 = hr.loss_fp32(c['pred'], c['y_all'], c['n_sp'], c['n_l'], hc.EPS, c['pw'], c['dloss'])
    case = 'loss-' + c['name']
    gt, gl, gg = terms.cpu().numpy(), float(loss), dpred.cpu().numpy()
    checks = [figure(case, 'loss terms', gt, ref_t, t32, hr.CAP_LOSS, hr.terms_figure),
              figure(case, 'loss', np.array([gl]), np.array([ref_l]), np.array([l32]), hr.CAP_LOSS),
              figure(case, 'dpred', gg, ref_g, g32, hr.CAP_GRAD)]
    # counts, the pseudo-label sum and the two pad words exactly (terms_figure is inf otherwise); an absent image is all zeros
    assert np.array_equal(gt[:, [1, 3, 4, 6, 7]], ref_t[:, [1, 3, 4, 6, 7]]) and not gt[0].any()
    # the planted clamp edges: the gradient passes on the closed interval and nowhere else
    for (nm, where), (b, r, cc, passes) in c['planted'].items():
        assert (gg[b, r, cc] != 0) == passes == (ref_g[b, r, cc] != 0), (nm, where, gg[b, r, cc])
    for b in range(hc.LOSS_B):                                           # beyond n_sp: exactly zero, whatever pred and y_all hold there
        assert not gg[b, int(c['n_sp'][b]):].any()
    assert all(ok for ok, _ in checks), [text for ok, text in checks if not ok]
    _fused_equals_unfused(ops, c, m, pred, y_all, terms, dloss, dpred)


def test_nan_prediction_is_a_nan_loss_and_a_zero_gradient(ops):
    c = hc.loss_case(0, True)
    m, pred, y_all, terms, loss, dloss, dpred = _run_loss(ops, c)
    ref_t, ref_l = hr.loss_terms(c['pred'], c['y_all'], c['n_sp'], c['n_l'], hc.EPS, c['pw'])
    ref_g = hr.loss_grad(c['pred'], c['y_all'], c['n_sp'], c['n_l'], hc.EPS, c['pw'], c['dloss'])
    t32, l32, g32 = hr.loss_fp32(c['pred'], c['y_all'], c['n_sp'], c['n_l'], hc.EPS, c['pw'], c['dloss'])
    gt, gg = terms.cpu().numpy(), dpred.cpu().numpy()
    assert np.isnan(ref_l) and np.isnan(float(loss))
    assert np.array_equal(np.isnan(gt), np.isnan(ref_t)) and np.isnan(gt[4, [0, 5]]).all() and int(np.isnan(gt).sum()) == 2
    assert np.isfinite(gg).all() and gg[4, 3, 0] == 0.0
    checks = [figure('loss-nan', 'loss terms', gt, ref_t, t32, hr.CAP_LOSS, hr.terms_figure), figure('loss-nan', 'dpred', gg, ref_g, g32, hr.CAP_GRAD)]
    assert all(ok for ok, _ in checks), [text for ok, text in checks if not ok]
    _fused_equals_unfused(ops, c, m, pred, y_all, terms, dloss, dpred)


# ---------------------------------------------------------------- generic cross entropy
@pytest.mark.parametrize('i', range(len(hc.CE)), ids=[c[0] for c in hc.CE])
def test_cross_entropy_against_fp64(ops, i):
    """One figure per configuration over its n = 1 ... 1000 (a single row has no stable fp32 figure of its own): the sums and losses
    of all n as one vector, the gradients of all n as one tensor."""
    name, C, weighted, none = hc.CE[i]
    d = dev()
    got_l, ref_l, cpu_l, got_g, ref_g, cpu_g = [], [], [], [], [], []
    for n in hc.CE_N:
        c = hc.ce_case(i, n)
        cw = None if c['cw'] is None else t(c['cw'])
        if n:
            y_hat, y_true = t(c['y_hat']), t(c['y_true'])
            out2 = ops.cross_entropy_fwd(y_hat, y_true, hc.EPS, cw)
        else:                                                            # (an empty tensor has no address: the entry itself, n = 0)
            from wesup_amd import _lib
            from wesup_amd.ops import _p, _stream
            buf, out2 = torch.full((1, C), S, device=d), torch.full((4,), S, device=d)
            _lib.call('wesup_cross_entropy_fwd', _p(buf), _p(buf), _p(cw), hc.EPS, _p(out2), 0, C, _stream())
        out, dy = hr.cross_entropy(c['y_hat'], c['y_true'], hc.EPS, c['cw'], c['dloss'])
        s32, l32, g32 = hr.cross_entropy_fp32(c['y_hat'], c['y_true'], hc.EPS, c['cw'], c['dloss'])
        o = out2.cpu().numpy()
        assert o[1] == out[1] and o[3] == 0.0                            # the row count exactly
        if out[1] == 0:
            assert o[2] == 0.0 and (n == 0 or none) and (o[0] == 0.0) == (out[0] == 0.0)
        got_l += [o[0], o[2]]; ref_l += [out[0], out[2]]; cpu_l += [s32, l32]
        if n:
            g = ops.cross_entropy_bwd(y_hat, y_true, out2, torch.tensor([c['dloss']], device=d), hc.EPS, cw).cpu().numpy()
            got_g.append(g.ravel()); ref_g.append(dy.ravel()); cpu_g.append(g32.ravel())
            if none:
                assert not g.any()
    checks = [figure('ce-' + name, 'cross entropy', np.array(got_l), np.array(ref_l), np.array(cpu_l), hr.CAP_LOSS),
              figure('ce-' + name, 'dy_hat', np.concatenate(got_g), np.concatenate(ref_g), np.concatenate(cpu_g), hr.CAP_GRAD)]
    assert all(ok for ok, _ in checks), [text for ok, text in checks if not ok]


# ---------------------------------------------------------------- SGD
def _sgd_run(ops, n, seed, hyper):
    """Three steps on the device from v = NaN; returns per step (p, v) of the GPU, the fp64 reference and numpy float32."""
    lr, mu, wd, gs = hyper
    p0, g3 = hc.sgd_inputs(n, seed)
    ref, cpu = hc.sgd_reference(p0, g3, hyper), hc.sgd_reference(p0, g3, hyper, np.float32)
    d = dev()
    p, v = t(p0), torch.full((n,), float('nan'), device=d)
    got = []
    for step in range(3):
        ops.sgd_step(p, t(g3[step]), v, lr, mu, wd, gs, step == 0)
        got.append((p.cpu().numpy(), v.cpu().numpy()))
    return got, ref, cpu


@pytest.mark.parametrize('hyper', list(hc.SGD_HYPER))
def test_sgd_small_sizes_against_fp64(ops, hyper):
    """n = 1 ... 1025: the float4 body, the scalar tail of block 0, both, and neither half; the outputs of all n as one tensor per
    step (a tensor of one element has no stable fp32 figure of its own)."""
    runs = [_sgd_run(ops, n, n, hc.SGD_HYPER[hyper]) for n in hc.SGD_SMALL]
    checks = []
    for step in range(3):
        for k, what in ((0, 'p'), (1, 'v')):
            got, ref, cpu = (np.concatenate([r[j][step][k] for r in runs]) for j in range(3))
            assert np.isfinite(got).all(), (hyper, step, what, 'a NaN of v before the first step came through')
            checks.append(figure(f'sgd-small-{hyper}-step{step}', f'SGD {what}', got, ref, cpu, hr.CAP_SGD, hr.rel_whole))
    assert all(ok for ok, _ in checks), [text for ok, text in checks if not ok]


@pytest.mark.parametrize('n', hc.SGD_LARGE, ids=[f'wrap+{k}' for k in range(4)])
def test_sgd_where_the_capped_grid_takes_a_second_trip(ops, n):
    """2048 blocks x 256 threads x 4 floats + 1200 + k: 300 threads take a second trip, block 0 a tail of k floats."""
    assert n // 4 == 2048 * 256 + 300 and n % 4 == n - hc.SGD_WRAP
    got, ref, cpu = _sgd_run(ops, n, 77, hc.SGD_HYPER['plain'])
    checks = []
    for step in range(3):
        for k, what in ((0, 'p'), (1, 'v')):
            assert np.isfinite(got[step][k]).all(), (step, what)
            checks.append(figure(f'sgd-wrap+{n - hc.SGD_WRAP}-step{step}', f'SGD {what}', got[step][k], ref[step][k], cpu[step][k], hr.CAP_SGD,
                                 hr.rel_whole))
    assert all(ok for ok, _ in checks), [text for ok, text in checks if not ok]


def test_sgd_refuses_a_view_that_is_not_16_byte_aligned(ops):
    from wesup_amd import _lib
    d = dev()
    n = 1024
    base_p, base_v, g = torch.randn(n + 4, device=d), torch.randn(n + 4, device=d), torch.randn(n, device=d)
    for p, v in ((base_p[1:n + 1], base_v[:n]), (base_p[:n], base_v[3:n + 3])):
        assert p.is_contiguous() and v.is_contiguous() and (p.data_ptr() | v.data_ptr()) % 16 != 0
        keep_p, keep_v = base_p.clone(), base_v.clone()
        with pytest.raises(_lib.WesupHipError):
            ops.sgd_step(p, g, v, 5e-2, 0.9, 1e-3, 1.0, False)
        torch.cuda.synchronize()
        assert torch.equal(base_p, keep_p) and torch.equal(base_v, keep_v)
    with pytest.raises(_lib.WesupHipError):
        ops.sgd_step(base_p[:n], torch.randn(n + 4, device=d)[2:n + 2], base_v[:n], 5e-2, 0.9, 1e-3, 1.0, False)


# ---------------------------------------------------------------- metric sums
@pytest.mark.parametrize('i', range(len(hc.SEG)), ids=[f'HW{c[0]}-C{c[1]}-B{c[2]}' for c in hc.SEG])
def test_metric_sums_are_exact(ops, i):
    """Every sum is an integer below 2^24 (asserted by the builder): the float outputs are those integers, compared for equality."""
    pred, mask, ref = hc.seg_case(i)
    B = pred.shape[0]
    out = torch.full((B, 4), S, device=dev())
    ops.seg_metrics(t(pred), t(mask), out=out)
    got = out.cpu().numpy().astype(np.float64)
    assert np.array_equal(got, ref.astype(np.float64)), (hc.SEG[i], got.tolist(), ref.tolist())
