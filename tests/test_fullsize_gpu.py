"""Parity of the HIP training step AT THE SIZES OF THE BASELINE CONFIGS, on a real MI355X.

  * against outputs of the REAL reference at full size (tests/golden/c480_g14.npz = BASELINE configs[0]: 480x480, 196
    superpixels; c480_g24.npz = one image of configs[1]: 576 superpixels; c800_g39.npz = one image of configs[3]:
    800x800, 1521 superpixels; made by oracle/make_golden.py full / crag from
    /root/reference/models/wesup.py:18-139,263-304,492-531 + autograd backward);
  * one image of configs[4] (1024x1024, 3025 superpixels) against the CPU oracle (the reference itself needs > 60 GB
    there: 12.7 GB of dense sp_maps, a 8.9 GB feature map and their gradients);
  * against the CPU oracle at configs[1] EXACTLY (B = 4, 480x480, 576 superpixels, 20 % point-labelled): loss, metrics,
    every integer output bit-exact, every parameter gradient against an fp64 evaluation (tests/_gradcheck.py);
  * size-independent properties at the per-GPU shards of configs[3] (B = 4, 800x800, 1521 SP) and configs[4]
    (B = 8, 1024x1024, 3025 SP).
Bars: integer outputs bit-exact; fp32 tensors within 1e-4 relative (north_star)."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from conftest import load_full_size_case          # noqa: E402
import _gradcheck
import _parity                              # noqa: E402
import _tol                                 # noqa: E402

pytestmark = pytest.mark.gpu
TOL = 1e-4
# rows per image that the src / y_u comparison at configs[1] may leave out as near-ties (threshold or runner-up within 1e-5): 10 x the
# worst count observed on round 6's green run (profiles/r06_tolerances.json), floor 4
MASKED_ROWS_BUDGET = 10        # observed: 0 - 1 per image at configs[1], 4 of 2 420 at 1024^2 (budget there: 5 x this)


def rel_err(a, b):
    a = torch.as_tensor(a).detach().double().cpu()
    b = torch.as_tensor(b).detach().double().cpu()
    return float((a - b).abs().max() / (b.abs().max() + 1e-30))


def make_trainer(weights, **kw):
    from wesup_amd.models import initialize_trainer
    from wesup_amd.utils.metrics import accuracy, dice
    trainer = initialize_trainer('wesup', device='cuda:0', **kw)
    trainer.model.load_state_dict({k: torch.from_numpy(v) for k, v in weights.items()})
    trainer.optimizer, trainer.scheduler = trainer.get_default_optimizer()
    trainer.metric_funcs = [accuracy, dice]
    trainer.model.train()
    trainer.tracker.train()
    return trainer


def loss_under_gpu_decisions(orc, out, y_all_b, threshold=0.8, weight=0.5, tol=1e-5):
    """The oracle's per-image loss with the pseudo labels the GPU propagated, after checking that the two only disagree
    on rows whose best similarity is within fp32 rounding of the threshold or of the runner-up (the propagation is a
    discrete decision: ``max_sim > threshold``, first arg-max; one such row moves the loss by ~1/n_propagated)."""
    pp = out['pp']
    n, n_l = pp['K'], pp['n_l']
    feats = out['sp_features'].detach()
    y_u, W_ul, max_sim, src = orc.label_propagate(feats, pp['sp_labels'], threshold, return_aux=True)
    got = y_all_b[n_l:n].cpu()
    differ = (got != y_u).any(dim=1)
    if bool(differ.any()):
        top2 = W_ul.topk(min(2, W_ul.shape[1]), dim=1).values
        close = ((max_sim - threshold).abs() < tol) | ((top2[:, 0] - top2[:, -1]).abs() < tol)
        assert bool(close[differ].all()), f'{int(differ.sum())} pseudo labels differ, not all of them near-ties'
    loss = orc.cross_entropy(out['sp_pred'].detach()[:n_l], pp['sp_labels'])
    loss = loss + weight * orc.cross_entropy(out['sp_pred'].detach()[n_l:], got)
    return float(loss), int(differ.sum())


@pytest.mark.parametrize('name', ['c480_g14', 'c480_g24', 'c800_g39'])
def test_step_matches_the_reference_at_full_size(golden_dir, name):
    """The trainer's own path (preprocess -> forward -> compute_loss -> backward) on the reference's full-size inputs."""
    from oracle import wesup_oracle as orc
    from wesup_amd import ops
    torch.set_num_threads(min(16, os.cpu_count() or 1))
    fx = load_full_size_case(golden_dir, name)
    d = torch.device('cuda:0')
    H, W = int(fx['H']), int(fx['W'])
    weights = orc.make_weights(int(fx['seed']), feat_scale=float(fx['feat_scale']))
    trainer = make_trainer(weights)
    model = trainer.model
    img = torch.from_numpy(fx['img'])[None]
    mask = torch.from_numpy(fx['mask'].astype(np.int64))[None]
    (x, sp_maps), (pixel_mask, sp_labels) = trainer.preprocess(img, mask, mask, torch.from_numpy(fx['seg'])[None])
    meta = sp_maps.meta
    meta.check()
    K = int(fx['seg'].max()) + 1
    n_l = fx['sp_labels'].shape[0]
    # integer outputs of _preprocess_superpixels: bit-exact (models/wesup.py:18-63)
    assert int(meta.n_sp[0]) == K and int(meta.n_l[0]) == n_l
    assert sp_labels.size(0) == n_l and tuple(sp_labels.shape) == fx['sp_labels'].shape      # behaves like the (N_l, C) tensor
    assert np.array_equal(sp_labels.cpu().numpy(), fx['sp_labels'])
    assert np.array_equal(meta.new_row[0].cpu().numpy().reshape(H, W).astype(np.int16), fx['new_row'])
    assert rel_err(1.0 / meta.area_new[0, :K].float(), fx['sp_maps_max']) < 1e-6

    pred = model((x, sp_maps))
    assert tuple(pred.shape) == (1, H, W)
    ref = 'max |a - b| / max |b| against the real reference (tests/golden)'
    assert _tol.within(name, 'sp_features vs reference', rel_err(model.sp_features, fx['sp_features']), TOL, ref)
    assert _tol.within(name, 'sp_pred vs reference', rel_err(model.sp_pred, fx['sp_pred']), TOL, ref)
    assert _tol.within(name, 'pred (painted) vs reference', rel_err(pred[0, ::7, ::11], fx['pred_sample']), TOL, ref)
    assert np.array_equal(trainer.postprocess(pred).cpu().numpy().astype(np.int8), fx['post_pred'])
    fm = model.feature_maps
    assert tuple(fm.shape) == (2112, H, W)
    assert _tol.within(name, 'feature map channel means vs reference', rel_err(fm.mean(dim=(1, 2)), fx['fm_chan_mean']), TOL, ref)
    # ... and slice by slice: the 13 side outputs differ in magnitude, one max over 2112 channels would hide a small slice
    ok, errs = _parity.check_sp_slices(name, 'feature map channel means per slice vs reference', fm.mean(dim=(1, 2)),
                                       fx['fm_chan_mean'], TOL, 'the reference\'s per-channel means of the 2112-channel feature map')
    assert ok, errs
    assert _tol.within(name, 'feature map samples vs reference', rel_err(fm[::97, ::23, ::29], fx['fm_sample']), TOL, ref)
    del fm

    feats_padded = model._padded[0].detach().clone()
    metrics = {}
    loss = trainer.compute_loss(pred, (pixel_mask, sp_labels), metrics=metrics)
    host = trainer._read_back(loss, metrics, None)
    assert _tol.within(name, 'loss vs reference', abs(host['loss'] - float(fx['loss'])) / abs(float(fx['loss'])), TOL, 'relative')
    assert metrics['propagated_labels'] == float(fx['propagated_labels'])
    assert _tol.within(name, 'propagate_loss vs reference',
                       abs(metrics['propagate_loss'] - float(fx['propagate_loss'])) / abs(float(fx['propagate_loss'])), TOL, 'relative')
    assert abs(metrics['labeled_sp_ratio'] - float(fx['labeled_sp_ratio'])) < 1e-7
    y_all, src, sim = ops.propagate(feats_padded, meta, 0.8)
    assert np.array_equal(src[0, n_l:K].cpu().numpy(), fx['src'])                 # argmax indices bit-exact
    assert np.array_equal(y_all[0, n_l:K].cpu().numpy(), fx['y_u'])
    assert _tol.within(name, 'max_sim vs reference', rel_err(sim[0, n_l:K], fx['max_sim']), TOL, ref)

    loss.backward()
    # every parameter gradient against fp64 under the same ReLU / pooling decisions: 1e-4 of each tensor's max (fixed bar) ...
    worst, n_named = _gradcheck.check_gradients(model, weights, fx['img'][None], fx['seg'][None], fx['mask'][None], case=name)
    g64 = _gradcheck.check_gradients.last_g64
    # the superpixel input of the fc layers, slice by slice, against the fp64 evaluation (the reference keeps no copy of it)
    ok, errs = _parity.check_sp_slices(name, 'sp_in per slice vs oracle', model.engine._last.sp_in[0, :K],
                                       _gradcheck.check_gradients.last_sp_in[0], TOL, 'GPU superpixel input of the fc layers against fp64')
    assert ok, errs
    # ... and against the reference itself: the norm of every tensor, and 64 elements per tensor at north_star's 1e-4 of the
    # tensor's max -- PER TENSOR, with one named reason for anything above it: the reference's own fp32 CPU gradient is that far
    # from the fp64 evaluation at the very same elements (its sums carry summation-order noise -- conv1_1's dW adds 230 400
    # mixed-sign products per element -- and it takes near-tie decisions its own way).  bar_k = min(1e-4 + (the reference's own
    # distance), 1e-3), and that distance itself at most 1e-3 (worst observed 7.25e-4, profiles/r06_tolerances.json): a bug the
    # oracle and the GPU shared would otherwise be absorbed into the reference's own distance.
    exceptions = []
    for k in [k[6:] for k in fx if k.startswith('gnorm.')]:
        g = model._grad_views[k]
        ref_norm = float(fx['gnorm.' + k])
        assert _tol.within(name, 'gradient norms vs reference (fp32 CPU)', abs(g.double().norm().item() - ref_norm) / ref_norm, 2e-4,
                           '| ||g|| - ||g_ref|| | / ||g_ref||, every parameter tensor'), k
        step = max(1, g.numel() // 64)
        samp = g.flatten()[::step][:64].cpu().numpy()
        s64 = g64[k].flatten()[::step][:64].numpy()
        gmax = float(fx['gmax.' + k])
        ref_own = float(np.abs(fx['gsamp.' + k].astype(np.float64) - s64).max() / gmax)
        err = float(np.abs(samp - fx['gsamp.' + k]).max() / gmax)
        assert _tol.within(name, 'reference fp32 gradient samples vs fp64 (the reference\'s own distance)', ref_own, 1e-3,
                           'the same 64 elements: |g_ref - g64| / max |g_ref|, fp64 under the GPU\'s decisions'), (k, ref_own)
        if err > 1e-4:
            exceptions.append((k, err, ref_own))
        assert _tol.within(name, 'gradient samples vs reference (fp32 CPU), per-tensor bar', err, min(1e-4 + ref_own, 1e-3),
                           '64 elements per tensor, error / max |g_ref|; bar = min(1e-4 + the reference\'s own distance from fp64 at '
                           'the same elements (the one named reason for exceeding 1e-4), 1e-3)'), (k, err, ref_own)
    _tol.within(name, 'gradient tensors above 1e-4 vs reference (count; each named with the reference\'s own fp64 distance)',
                len(exceptions), len(exceptions), '; '.join(f'{k}: {e:.1e} (reference vs fp64 {r:.1e})' for k, e, r in exceptions) or 'none')
    print(f'{name}: worst gradient error vs fp64 {worst:.2e}, {n_named} near-tie decisions differ; tensors above 1e-4 of the '
          f'reference\'s samples: {[(k, f"{e:.1e}", f"ref own {r:.1e}") for k, e, r in exceptions]}')


def test_config_c2_exactly_matches_the_oracle():
    """BASELINE configs[1] as bench.py runs it: B = 4, 480x480, 576 superpixels, 20 % point-labelled, one full
    train_one_iteration; against the CPU oracle's training step on the same inputs."""
    from oracle import wesup_oracle as orc
    from wesup_amd import synth, ops
    torch.set_num_threads(min(16, os.cpu_count() or 1))
    d = torch.device('cuda:0')
    B, H, W, g = 4, 480, 480, 24
    weights = orc.make_weights(0, feat_scale=1.0)                  # features spread enough that only some rows propagate
    imgs, labs, pts, pix = synth.make_batch(5, B, H, W, g)
    ref_loss, ref_grads, ref_new, _, outs, mets = orc.train_step(weights, imgs, labs.astype(np.int64), pts.astype(np.int64))

    trainer = make_trainer(weights, max_superpixels=g * g)
    data = (torch.from_numpy(imgs).to(d), torch.from_numpy(pix).to(d), torch.from_numpy(pts).to(d), torch.from_numpy(labs).to(d))
    trainer.train_one_iteration('train', *data)
    model = trainer.model
    meta = model._last_meta
    hist = trainer.tracker.history
    assert 0 < hist['propagated_labels'][0] < 0.8 * g * g            # some rows propagate, some do not
    assert abs(hist['labeled_sp_ratio'][0] - np.mean([m['labeled_sp_ratio'] for m in mets])) < 1e-7
    bufs = model.engine._last
    feats = bufs.feats.view(B, meta.Kmax, -1)
    y_all, src, sim = ops.propagate(feats.contiguous(), meta, 0.8)
    per_image = [loss_under_gpu_decisions(orc, outs[b], y_all[b]) for b in range(B)]
    n_near = sum(k for _, k in per_image)
    assert _tol.within('c2_exact', 'loss vs oracle', abs(hist['loss'][0] - np.mean([l for l, _ in per_image])) / abs(ref_loss), TOL, 'relative')
    if n_near == 0:                                                   # no near-tie row: the oracle's own numbers
        assert abs(hist['loss'][0] - ref_loss) <= TOL * abs(ref_loss)
        assert hist['propagated_labels'][0] == np.mean([m['propagated_labels'] for m in mets])
        assert abs(hist['propagate_loss'][0] - np.mean([m['propagate_loss'] for m in mets])) < 1e-5
    P = torch.stack([o['pred'].detach().round().long() for o in outs])
    G = torch.from_numpy(pix).long().argmax(dim=1)
    assert abs(hist['accuracy'][0] - np.mean([orc.accuracy(P[b], G[b]) for b in range(B)])) < 1e-6
    assert abs(hist['dice'][0] - np.mean([orc.dice(P[b], G[b]) for b in range(B)])) < 1e-6
    # integer outputs, per image: row order, labels, propagation sources and pseudo labels
    for b in range(B):
        pp = outs[b]['pp']
        n, n_l = pp['K'], pp['n_l']
        assert int(meta.n_sp[b]) == n and int(meta.n_l[b]) == n_l
        assert torch.equal(meta.perm[b, :n].cpu().long(), pp['perm'])
        assert torch.equal(meta.sp_labels[b, :n_l].cpu(), pp['sp_labels'])
        y_u, W_ul, max_sim, src_ref = orc.label_propagate(outs[b]['sp_features'], pp['sp_labels'], 0.8, return_aux=True)
        top2 = W_ul.topk(2, dim=1).values
        near = ((max_sim - 0.8).abs() < 1e-5) | ((top2[:, 0] - top2[:, 1]).abs() < 1e-5)   # threshold / runner-up within rounding
        assert _tol.within('c2_exact', 'sp_features vs oracle', rel_err(feats[b, :n], outs[b]['sp_features']), TOL)
        ok, errs = _parity.check_sp_slices(f'c2_exact image {b}', 'sp_in per slice vs oracle', bufs.sp_in[b, :n],
                                           outs[b]['sp_in'].detach(), TOL, 'GPU superpixel input of the fc layers against the oracle\'s fp32')
        assert ok, (b, errs)
        # (how many rows the comparison below leaves out: recorded, and bounded -- a kernel whose arg-max drifted would mask many)
        assert _tol.within(f'c2_exact image {b}', 'propagation rows masked as near-ties before src / y_u are compared (count)',
                           int(near.sum()), MASKED_ROWS_BUDGET, f'of {n - n_l} unlabelled rows; near = max_sim within 1e-5 of the threshold '
                           'or of the runner-up'), (int(near.sum()), n - n_l)
        assert torch.equal(src[b, n_l:n].cpu().long()[~near], src_ref[~near])
        assert torch.equal(y_all[b, n_l:n].cpu()[~near], y_u[~near])
        assert torch.equal(bufs.pred[b].round().long().cpu(), outs[b]['pred'].detach().round().long())
    # every parameter gradient against fp64 (same decisions), and the SGD update against the oracle's
    worst, n_named = _gradcheck.check_gradients(model, weights, imgs, labs, pts, case='c2_exact')
    new = {k: v.detach().cpu() for k, v in model.state_dict().items()}
    for k, v in ref_new.items():
        assert _tol.within('c2_exact', 'updated parameters (SGD) vs oracle', rel_err(new[k], v), 1e-5), k
    print(f'c2: loss {hist["loss"][0]:.6f} (oracle {ref_loss:.6f}), worst gradient error vs fp64 {worst:.2e}, '
          f'{n_named} near-tie decisions differ')
    # ---- what bench.py TIMES is this shape replayed from a recorded step plan (wesup_amd/runner.py): six more iterations, over
    # two further batches, beside a twin that walks every iteration in Python (step_plan=False) and has taken the same first
    # step: loss, metrics, every parameter and every gradient bit for bit, with the plan replaying by the end.
    del outs, ref_grads
    twin = make_trainer(weights, max_superpixels=g * g, step_plan=False)
    twin.train_one_iteration('train', *data)
    assert torch.equal(twin.model._flat, model._flat) and twin.tracker.history['loss'][0] == hist['loss'][0]
    more = []
    for s in (6, 7):
        im2, lb2, pt2, px2 = synth.make_batch(s, B, H, W, g)
        more.append(tuple(torch.from_numpy(a).to(d) for a in (im2, px2, pt2, lb2)))
    for i in range(6):
        trainer.train_one_iteration('train', *more[i % 2])
        twin.train_one_iteration('train', *more[i % 2])
        for k in ('loss', 'labeled_sp_ratio', 'propagated_labels', 'propagate_loss', 'accuracy', 'dice'):
            assert twin.tracker.history[k][-1] == trainer.tracker.history[k][-1], (i, k)
        assert torch.equal(twin.model._flat, model._flat), f'parameters differ after replayed step {i}'
        assert torch.equal(twin.model._flat_grad, model._flat_grad), f'gradients differ after replayed step {i}'
    st = trainer.step_runner().stats
    assert st['replayed'] >= 3 and st['dropped'] == 0 and twin.step_runner().stats['replayed'] == 0, st


def _host_memory_gb():
    try:
        lim = int(open('/sys/fs/cgroup/memory.max').read())
    except Exception:
        lim = 1 << 62
    try:
        avail = int(next(l for l in open('/proc/meminfo') if l.startswith('MemAvailable')).split()[1]) * 1024
    except Exception:
        avail = 0
    return min(lim, avail) / 2 ** 30


def test_one_image_of_config_c5_matches_the_oracle():
    """BASELINE configs[4] shape: 1024x1024, 3025 superpixels, one image through train_one_iteration against the CPU
    oracle's training step: loss, metrics, integer outputs bit-exact, every parameter gradient against fp64 under the
    GPU's ReLU / pooling decisions.  (The fp64 evaluation holds ~90 GB on the host.)"""
    if _host_memory_gb() < 160:
        pytest.skip('needs ~90 GB of host memory for the fp64 evaluation at 1024x1024')
    from oracle import wesup_oracle as orc
    from wesup_amd import synth, ops
    torch.set_num_threads(min(16, os.cpu_count() or 1))
    d = torch.device('cuda:0')
    B, H, W, g = 1, 1024, 1024, 55
    weights = orc.make_weights(0, feat_scale=1.0)
    imgs, labs, pts, pix = synth.make_batch(7, B, H, W, g)
    ref_loss, ref_grads, ref_new, _, outs, mets = orc.train_step(weights, imgs, labs.astype(np.int64), pts.astype(np.int64))
    trainer = make_trainer(weights, max_superpixels=g * g)
    trainer.train_one_iteration('train', torch.from_numpy(imgs).to(d), torch.from_numpy(pix).to(d), torch.from_numpy(pts).to(d),
                                torch.from_numpy(labs).to(d))
    model, hist = trainer.model, trainer.tracker.history
    meta = model._last_meta
    assert 0 < hist['propagated_labels'][0] < 0.8 * g * g
    bufs = model.engine._last
    y_all0, _, _ = ops.propagate(bufs.feats.view(1, meta.Kmax, -1).contiguous(), meta, 0.8)
    loss_ref, n_near = loss_under_gpu_decisions(orc, outs[0], y_all0[0])
    assert abs(hist['loss'][0] - loss_ref) <= TOL * abs(ref_loss)
    if n_near == 0:
        assert abs(hist['loss'][0] - ref_loss) <= TOL * abs(ref_loss)
        assert hist['propagated_labels'][0] == mets[0]['propagated_labels']
        assert abs(hist['propagate_loss'][0] - mets[0]['propagate_loss']) < 1e-5
    pp = outs[0]['pp']
    n, n_l = pp['K'], pp['n_l']
    assert n == g * g == int(meta.n_sp[0]) and int(meta.n_l[0]) == n_l
    assert torch.equal(meta.perm[0, :n].cpu().long(), pp['perm']) and torch.equal(meta.sp_labels[0, :n_l].cpu(), pp['sp_labels'])
    feats = bufs.feats.view(1, meta.Kmax, -1)
    assert rel_err(feats[0, :n], outs[0]['sp_features']) < TOL
    ok, errs = _parity.check_sp_slices('c5_one_image', 'sp_in per slice vs oracle', bufs.sp_in[0, :n], outs[0]['sp_in'].detach(), TOL,
                                       'GPU superpixel input of the fc layers against the oracle\'s fp32')
    assert ok, errs
    y_all, src, sim = ops.propagate(feats.contiguous(), meta, 0.8)
    y_u, W_ul, max_sim, src_ref = orc.label_propagate(outs[0]['sp_features'], pp['sp_labels'], 0.8, return_aux=True)
    top2 = W_ul.topk(2, dim=1).values
    near = ((max_sim - 0.8).abs() < 1e-5) | ((top2[:, 0] - top2[:, 1]).abs() < 1e-5)     # threshold or runner-up within rounding
    assert _tol.within('c5_one_image', 'propagation rows masked as near-ties before src / y_u are compared (count)', int(near.sum()),
                       MASKED_ROWS_BUDGET * 5, f'of {n - n_l} unlabelled rows'), int(near.sum())
    assert torch.equal(src[0, n_l:n].cpu().long()[~near], src_ref[~near]) and torch.equal(y_all[0, n_l:n].cpu()[~near], y_u[~near])
    assert torch.equal(bufs.pred[0].round().long().cpu(), outs[0]['pred'].detach().round().long())
    del outs, ref_grads
    worst, n_named = _gradcheck.check_gradients(model, weights, imgs, labs, pts, case='c5_one_image')
    new = {k: v.detach().cpu() for k, v in model.state_dict().items()}
    for k, v in ref_new.items():
        assert _tol.within('c5_one_image', 'updated parameters (SGD) vs oracle', rel_err(new[k], v), 1e-5), k
    print(f'c5 (one image): loss {hist["loss"][0]:.6f} (oracle {ref_loss:.6f}; {n_near} pseudo labels decided by a '
          f'near-tie), worst gradient error vs fp64 {worst:.2e}, {n_named} near-tie decisions differ')
    model.engine.release_buffers()
    torch.cuda.empty_cache()


@pytest.mark.parametrize('H,W,g,B', [(800, 800, 39, 4), (1024, 1024, 55, 8)])
def test_per_gpu_shards_of_c4_and_c5(H, W, g, B):
    """Per-GPU shards of BASELINE configs[3] (CRAG 800x800, 1521 SP, 16 images over 4 GPUs) and configs[4]
    (1024x1024, 3025 SP, 64 images over 8 GPUs) at their real batch: size-independent properties of one full training
    iteration -- finite loss in range, label ratio, conservation of pixels, gradients finite, non-zero and LINEAR in
    the upstream gradient, SGD moves the weights, and the whole step is bitwise reproducible."""
    from oracle import wesup_oracle as orc
    from wesup_amd import synth
    d = torch.device('cuda:0')
    trainer = make_trainer(orc.make_weights(0, feat_scale=0.05), max_superpixels=g * g)
    imgs, labs, pts, pix = synth.make_batch(2, B, H, W, g)
    data = (torch.from_numpy(imgs).to(d), torch.from_numpy(pix).to(d), torch.from_numpy(pts).to(d), torch.from_numpy(labs).to(d))
    del imgs, pix
    before = trainer.model._flat.clone()
    trainer.train_one_iteration('train', *data)
    h = trainer.tracker.history
    assert np.isfinite(h['loss'][0]) and 0.0 < h['loss'][0] < 10.0
    assert 0.15 < h['labeled_sp_ratio'][0] < 0.25            # 20 % point-labelled superpixels
    assert 0.0 <= h['accuracy'][0] <= 1.0 and 0.0 <= h['dice'][0] <= 1.0
    meta = trainer.model._last_meta
    meta.check()
    assert int(meta.n_sp.min()) == g * g and int(meta.area_new.sum()) == B * H * W
    gflat = trainer.model._flat_grad.clone()
    assert bool(torch.isfinite(gflat).all()) and float(gflat.abs().sum()) > 0
    assert not torch.equal(before, trainer.model._flat)     # SGD moved the weights
    loss0 = h['loss'][0]
    # bitwise reproducible: restore the weights, same batch again -> identical loss and gradient bits
    trainer.model._flat.copy_(before)
    trainer.optimizer._first = True
    trainer.train_one_iteration('train', *data)
    assert trainer.tracker.history['loss'][1] == loss0
    assert torch.equal(trainer.model._flat_grad, gflat)
    # linearity of backward in the upstream gradient
    trainer.model._flat.copy_(before)
    (x, sp_maps), target = trainer.preprocess(*data)
    pred = trainer.model((x, sp_maps))
    loss = trainer.compute_loss(pred, target, metrics={})
    (2.0 * loss).backward()
    assert rel_err(trainer.model._flat_grad, 2.0 * gflat) < 1e-5
    trainer.model.engine.release_buffers()
    torch.cuda.empty_cache()
