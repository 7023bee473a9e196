"""tests/_headref.py -- the fp64 reference tests/test_head_branches_gpu.py holds the propagation, loss, cross-entropy, SGD and
metric kernels to -- against oracle/wesup_oracle.py at small sizes (fp32 noise apart), every builder of tests/_headcases.py with
the conditions it asserts, and the plain-fp32 figures of the whole case list: each is recorded (tests/_tol.py) and must lie below
the cap of its class -- a case whose honest fp32 evaluation already breaks the cap has unsuitable inputs.  No GPU."""
import os
import re

import numpy as np
import pytest
import torch

import _headcases as hc
import _headref as hr
from _tol import within

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ---------------------------------------------------------------- the bound on D
def test_lds_bound_is_arithmetic_and_stated_in_the_header_and_the_package():
    from wesup_amd import _lib, ops
    with open(os.path.join(ROOT, 'include', 'wesup_hip.h')) as f:
        stated = int(re.search(r'#define\s+WESUP_HEAD_MAX_D\s+(\d+)', f.read()).group(1))
    fits = [D for D in range(1, 300) if hr.head_lds_bytes(D) <= hr.HEAD_LDS_MAX]
    assert fits == list(range(1, stated + 1)) and stated == 149 == _lib.HEAD_MAX_D == ops.HEAD_MAX_D and hc.D_REFUSED == stated + 1
    assert hr.head_lds_bytes(32) == 35840 and hr.head_lds_bytes(59) <= 65536 < hr.head_lds_bytes(60)
    assert {c[1] for c in hc.PROP} >= {1, 7, 32, 33, 64, 128, stated}


def test_model_refuses_a_feature_width_the_head_cannot_take():
    from wesup_amd.models.wesup import WESUP
    for D in (150, 256):
        with pytest.raises(ValueError):
            WESUP(D=D)
    with pytest.raises(ValueError):
        WESUP(n_classes=17)
    assert WESUP(D=64).classifier[0].in_features == 64


# ---------------------------------------------------------------- propagation
@pytest.mark.parametrize('i', range(len(hc.PROP)), ids=[c[0] for c in hc.PROP])
def test_propagation_reference_is_the_oracles_label_propagate(i):
    """Every builder runs (its asserts with it); on a sample of its images the fp64 reference names the oracle's sources and pseudo
    labels exactly -- d is exact in float32 on these features -- and its max_sim to fp32 rounding."""
    from oracle import wesup_oracle as orc
    c = hc.prop_case(i)
    y, src, sim = hr.propagate(c['feat'], c['labels'], c['n_sp'], c['n_l'], hc.THR)
    sim32 = hr.max_sim_fp32(c['feat'], c['n_sp'], c['n_l'])
    assert within(f'prop-{c["name"]}', 'max_sim, fp32 on the CPU vs fp64', hr.rel_elem(sim32, sim), hr.CAP_SIM)
    B = len(c['n_sp'])
    for b in list(range(0, B, 7)) + [B - 1]:
        ns, nl = int(c['n_sp'][b]), int(c['n_l'][b])
        assert np.array_equal(y[b, :nl], c['labels'][b, :nl]) and not y[b, ns:].any()
        assert np.all(src[b, :nl] == -1) and np.all(src[b, ns:] == -1) and not sim[b, :nl].any() and not sim[b, ns:].any()
        if nl == 0 or ns == nl:
            assert np.all(src[b] == -1) and not sim[b].any() and not y[b, nl:].any()
            continue
        y_u, _, max_sim, s = orc.label_propagate(torch.from_numpy(c['feat'][b, :ns]), torch.from_numpy(c['labels'][b, :nl]), hc.THR,
                                                 return_aux=True)
        assert np.array_equal(src[b, nl:ns], s.numpy()) and np.array_equal(y[b, nl:ns], y_u.numpy())
        assert hr.rel_elem(max_sim.numpy(), sim[b, nl:ns]) < 1e-6
    if c['tie'] is not None:
        b = c['tie']
        for i_u, j in c['winners'].items():
            assert src[b, hc.TIE_NL + i_u] == j
        # the duplicate row: W = 1.0 exactly -- propagated under the largest float below 1, not under 1.0 (strict)
        r = hc.TIE_NL + 5
        below = np.nextafter(np.float32(1), np.float32(0))
        y1 = hr.propagate(c['feat'][b:b + 1], c['labels'][b:b + 1], c['n_sp'][b:b + 1], c['n_l'][b:b + 1], 1.0)[0]
        yb = hr.propagate(c['feat'][b:b + 1], c['labels'][b:b + 1], c['n_sp'][b:b + 1], c['n_l'][b:b + 1], below)[0]
        assert sim[b, r] == 1.0 and not y1[0, hc.TIE_NL:].any() and np.array_equal(yb[0, r], c['labels'][b, 30])
        assert np.count_nonzero(yb[0, hc.TIE_NL:].sum(axis=1)) == 1
    y0, src0, sim0 = hr.propagate(c['feat'], c['labels'], c['n_sp'], c['n_l'], hc.THR, enable=False)
    assert np.all(src0 == -1) and not sim0.any() and all(not y0[b, int(c['n_l'][b]):].any() for b in range(B))


# ---------------------------------------------------------------- loss
@pytest.mark.parametrize('C,pw', [(2, 0.5), (3, 0.25), (16, 0.5)])
def test_loss_reference_is_the_oracles_compute_loss(C, pw):
    """Small images through propagate -> loss_terms -> loss_grad against compute_loss and its autograd gradient."""
    from oracle import wesup_oracle as orc
    rng = np.random.default_rng(C)
    shapes = [(40, 12), (40, 40), (9, 0), (33, 1), (17, 16)]
    B, Kmax, D = len(shapes), 40, 8
    n_sp, n_l = np.array([s[0] for s in shapes], dtype=np.int32), np.array([s[1] for s in shapes], dtype=np.int32)
    feat = np.zeros((B, Kmax, D), dtype=np.float32)
    labels = np.full((B, Kmax, C), hc.ABSENT, dtype=np.float32)
    for b, (ns, nl) in enumerate(shapes):
        feat[b, :ns] = hc._features(rng, nl, ns - nl, D, pooled=False)
        labels[b, :nl] = hc._labels(rng, nl, C)
        labels[b, :nl][np.arange(nl) % 9 == 4] = 0.0
    z = rng.standard_normal((B, Kmax, C))
    pred = (np.exp(z) / np.exp(z).sum(axis=2, keepdims=True)).astype(np.float32)
    pred[0, 0, int(np.argmax(labels[0, 0]))] = 0.0                        # a clamped prediction under a label
    y_all, _, _ = hr.propagate(feat, labels, n_sp, n_l, hc.THR)
    y_all = y_all.astype(np.float32)
    terms, loss = hr.loss_terms(pred, y_all, n_sp, n_l, hc.EPS, pw)
    grad = hr.loss_grad(pred, y_all, n_sp, n_l, hc.EPS, pw, 1.7)
    p = torch.from_numpy(pred).clone().requires_grad_(True)
    ref = []
    for b, (ns, nl) in enumerate(shapes):
        mets = {}
        ref.append(orc.compute_loss(p[b, :ns], torch.from_numpy(feat[b, :ns]), torch.from_numpy(labels[b, :nl]), propagate_threshold=hc.THR,
                                    propagate_weight=pw, metrics=mets))
        assert abs(float(ref[-1].detach()) - terms[b, 5]) <= 2e-6 * max(1.0, abs(terms[b, 5]))
        if nl < ns:
            assert mets['propagated_labels'] == terms[b, 4]
            assert abs(mets['propagate_loss'] - terms[b, 2] / max(terms[b, 3], 1.0)) <= 2e-6 * max(1.0, mets['propagate_loss'])
    total = torch.stack([r.reshape(()) for r in ref]).mean()
    assert abs(float(total.detach()) - loss) <= 2e-6 * abs(loss)
    (total * 1.7).backward()
    assert hr.rel_whole(p.grad.numpy(), grad) < 1e-6 and not grad[0, 0].any() and np.abs(grad).max() > 0
    t32, l32, g32 = hr.loss_fp32(pred, y_all, n_sp, n_l, hc.EPS, pw, 1.7)
    assert hr.terms_figure(t32, terms) < 1e-6 and abs(l32 - loss) < 1e-6 * abs(loss) and hr.rel_elem(g32, grad) < 1e-6


@pytest.mark.parametrize('i', range(len(hc.LOSS)), ids=[c[0] for c in hc.LOSS])
def test_loss_cases_and_their_fp32_figures(i):
    c = hc.loss_case(i)
    terms, loss = hr.loss_terms(c['pred'], c['y_all'], c['n_sp'], c['n_l'], hc.EPS, c['pw'])
    grad = hr.loss_grad(c['pred'], c['y_all'], c['n_sp'], c['n_l'], hc.EPS, c['pw'], c['dloss'])
    for (nm, where), (b, r, cc, passes) in c['planted'].items():
        assert (grad[b, r, cc] != 0) == passes, (nm, where)
    for b in range(hc.LOSS_B):
        assert not grad[b, int(c['n_sp'][b]):].any()
    t32, l32, g32 = hr.loss_fp32(c['pred'], c['y_all'], c['n_sp'], c['n_l'], hc.EPS, c['pw'], c['dloss'])
    assert within(f'loss-{c["name"]}', 'loss terms, fp32 on the CPU vs fp64', hr.terms_figure(t32, terms), hr.CAP_LOSS)
    assert within(f'loss-{c["name"]}', 'loss, fp32 on the CPU vs fp64', abs(l32 - loss) / abs(loss), hr.CAP_LOSS)
    assert within(f'loss-{c["name"]}', 'dpred, fp32 on the CPU vs fp64', hr.rel_elem(g32, grad), hr.CAP_GRAD)


def test_a_nan_prediction_is_a_nan_loss():
    c = hc.loss_case(0, True)
    terms, loss = hr.loss_terms(c['pred'], c['y_all'], c['n_sp'], c['n_l'], hc.EPS, c['pw'])
    assert np.isnan(loss) and np.isnan(terms[4, [0, 5]]).all() and np.isfinite(np.delete(terms, 4, axis=0)).all()
    grad = hr.loss_grad(c['pred'], c['y_all'], c['n_sp'], c['n_l'], hc.EPS, c['pw'], c['dloss'])
    assert np.isfinite(grad).all() and grad[4, 3, 0] == 0
    t32, l32, g32 = hr.loss_fp32(c['pred'], c['y_all'], c['n_sp'], c['n_l'], hc.EPS, c['pw'], c['dloss'])
    assert np.isnan(l32) and np.array_equal(np.isnan(t32), np.isnan(terms))


# ---------------------------------------------------------------- generic cross entropy
@pytest.mark.parametrize('i', range(len(hc.CE)), ids=[c[0] for c in hc.CE])
def test_cross_entropy_reference_and_figures(i):
    from oracle import wesup_oracle as orc
    name, C, weighted, none = hc.CE[i]
    worst_l = worst_g = 0.0
    for n in hc.CE_N:
        c = hc.ce_case(i, n)
        out, dy = hr.cross_entropy(c['y_hat'], c['y_true'], hc.EPS, c['cw'], c['dloss'])
        assert out[1] == (0 if none else (c['y_true'].sum(axis=1) > 0).sum()) and out[3] == 0 and (out[1] > 0 or out[2] == 0)
        p = torch.from_numpy(c['y_hat']).clone().requires_grad_(True)
        if not weighted:                                                   # the oracle has no class weights
            ref = orc.cross_entropy(p, torch.from_numpy(c['y_true']))
            assert abs(float(ref) - out[2]) <= 2e-6 * max(1.0, out[2])
            if ref.requires_grad:
                (ref * c['dloss']).backward()
                assert hr.rel_whole(p.grad.numpy(), dy) < 1e-6
        else:                                                              # models/wesup.py:93-94: ce * class_weights, in float64
            lo, hi = hr.clamp_bounds(hc.EPS)
            pd = torch.from_numpy(c['y_hat']).double().requires_grad_(True)
            ce = -torch.from_numpy(c['y_true']).double() * torch.log(torch.clamp(pd, min=lo, max=hi)) * torch.from_numpy(c['cw']).double()
            if out[1] > 0:
                l = ce.sum() / out[1]
                (l * hr.f32(c['dloss'])).backward()
                assert abs(float(l) - out[2]) <= 1e-12 * out[2] and hr.rel_whole(dy, pd.grad.numpy()) < 1e-12
        s32, l32, g32 = hr.cross_entropy_fp32(c['y_hat'], c['y_true'], hc.EPS, c['cw'], c['dloss'])
        if out[1] > 0:
            worst_l = max(worst_l, abs(s32 - out[0]) / out[0], abs(l32 - out[2]) / out[2])
            worst_g = max(worst_g, hr.rel_elem(g32, dy))
    assert within(f'ce-{name}', 'cross entropy, fp32 on the CPU vs fp64', worst_l, hr.CAP_LOSS)
    assert within(f'ce-{name}', 'dy_hat, fp32 on the CPU vs fp64', worst_g, hr.CAP_GRAD)


# ---------------------------------------------------------------- SGD
@pytest.mark.parametrize('hyper', list(hc.SGD_HYPER))
def test_sgd_reference_is_the_oracles_step(hyper):
    from oracle import wesup_oracle as orc
    lr, mu, wd, gs = hc.SGD_HYPER[hyper]
    p0, g3 = hc.sgd_inputs(1025, 1)
    ref = hc.sgd_reference(p0, g3, hc.SGD_HYPER[hyper])
    f32 = hc.sgd_reference(p0, g3, hc.SGD_HYPER[hyper], np.float32)
    params, bufs = {'w': torch.from_numpy(p0).double()}, {}
    for step in range(3):
        params, bufs = orc.sgd_step(params, {'w': torch.from_numpy(g3[step]).double() * hr.f32(gs)}, bufs, hr.f32(lr), hr.f32(mu), hr.f32(wd))
        assert hr.rel_whole(ref[step][0], params['w'].numpy()) < 1e-12 and hr.rel_whole(ref[step][1], bufs['w'].numpy()) < 1e-12
        assert f32[step][0].dtype == np.float32 and hr.rel_whole(f32[step][0], ref[step][0]) < hr.CAP_SGD
        assert hr.rel_whole(f32[step][1], ref[step][1]) < hr.CAP_SGD
    # a step that read v on the first step would end in NaN: the reference never does
    p1, v1 = hr.sgd(p0, g3[0], np.full(1025, np.nan), lr, mu, wd, gs, True)
    assert np.isfinite(p1).all() and np.isfinite(v1).all()
    assert hc.SGD_WRAP // 4 > 2048 * 256 and (hc.SGD_WRAP // 4 - 2048 * 256) == 300 and [n % 4 for n in hc.SGD_LARGE] == [0, 1, 2, 3]


# ---------------------------------------------------------------- metric sums
@pytest.mark.parametrize('i', range(len(hc.SEG)), ids=[f'HW{c[0]}-C{c[1]}-B{c[2]}' for c in hc.SEG])
def test_metric_sums_are_the_oracles_accuracy_and_dice(i):
    from oracle import wesup_oracle as orc
    pred, mask, ref = hc.seg_case(i)
    HW, C, B = hc.SEG[i]
    P = torch.from_numpy(pred).round().long()
    G = torch.from_numpy(mask.astype(np.int64)).argmax(dim=1)             # torch: the first maximum
    for b in range(B):
        assert abs(ref[b, 0] / HW - orc.accuracy(P[b], G[b])) < 1e-6
        assert abs(2 * ref[b, 1] / (ref[b, 3] + ref[b, 2] + 1e-7) - orc.dice(P[b], G[b])) < 1e-5 * max(1.0, orc.dice(P[b], G[b]))
    assert np.array_equal(ref[:, 2], P.reshape(B, -1).sum(1).numpy()) and np.array_equal(ref[:, 3], G.reshape(B, -1).sum(1).numpy())
    assert hr.seg_sums(np.array([[[0.5, 1.5, 2.5, 3.5]]], dtype=np.float32), np.zeros((1, 2, 1, 4), dtype=np.uint8))[0, 2] == 0 + 2 + 2 + 4
