"""The per-GPU shards of BASELINE configs[3] (B = 4, 800x800, 1521 superpixels) and configs[4] (B = 8, 1024x1024, 3025
superpixels) at their real batch, IMAGE BY IMAGE: one training iteration of the batch against each image's own iteration at
B = 1 (same weights, fresh optimiser state, same Kmax), and every conv layer of every batched image against fp64.

What changes with the number of images and tiles -- the Winograd route chosen by tile count, the product tilings chosen by M,
the weight-gradient split-K slabs across images, the per-image interpolation-matrix transposes -- is invisible to properties
(finite, reproducible, linear): an image dropped, duplicated or misaddressed keeps all of them.  Here every image of the batch
is tied to its single run (integers bit-exact, floats at 1e-5 of their own scale, gradients to the mean of the single-image
gradients) and, through fp64 convolutions on corner and centre windows, to a high-precision reference directly; image 0 of
the 800x800 batch is the c800_g39 golden's input and is checked against the real reference, image 0 of the 1024x1024 batch
is the input of test_one_image_of_config_c5_matches_the_oracle."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from conftest import load_full_size_case          # noqa: E402
import _gradcheck          # noqa: E402
import _parity             # noqa: E402
import _tol                # noqa: E402
from test_fullsize_gpu import MASKED_ROWS_BUDGET, TOL, make_trainer, rel_err    # noqa: E402

pytestmark = pytest.mark.gpu
# batched vs single, and conv pre-activations vs fp64 of the GPU's own input: 1e-5 of the layer's (slice's) max; gradients: 2e-5
# when no discrete decision differs (the reordering bar of test_round3_schedule_and_fusions_against_the_plain_order), 5e-3 when
# only named near-ties do (_gradcheck's docstring).  Worst observed on the first green run of these tests
# (profiles/tolerances_shards_multiscale.json): conv vs single 2.2e-6 (c4; c5's batch is bit-identical to its single runs), conv vs
# fp64 2.4e-6, sp_in slices 1.1e-6, loss terms 1.1e-7; gradients 1.3e-6 (c5, no decision differs) and 4.6e-4 (c4, 27 near-ties)
BAR = 1e-5
GRAD_REORDER, GRAD_NEAR_TIE = 2e-5, 5e-3


def _run(weights, arrays, g):
    """One training iteration; everything the comparison needs, cloned on the device; the trainer's buffers released."""
    from wesup_amd import ops
    d = torch.device('cuda:0')
    B = arrays[0].shape[0]
    trainer = make_trainer(weights, max_superpixels=g * g)
    trainer.train_one_iteration('train', *(torch.from_numpy(a).to(d) for a in arrays))
    m, hist = trainer.model, trainer.tracker.history
    meta, bufs = m._last_meta, m.engine._last
    K = meta.Kmax
    feats, sp_pred = (t.detach().contiguous() for t in m._padded)
    y_all, src, sim = ops.propagate(feats, meta, 0.8)
    _, terms = ops.loss_fwd(sp_pred, y_all, meta, float(trainer.kwargs.get('epsilon')), float(trainer.kwargs.get('propagate_weight')))
    out = dict(loss=hist['loss'][0], accuracy=hist['accuracy'][0], dice=hist['dice'][0], Kmax=K,
               n_sp=meta.n_sp.clone(), n_l=meta.n_l.clone(), perm=meta.perm.clone(), new_row=meta.new_row.clone(),
               sp_labels=meta.sp_labels.clone(), y=[y.clone() for y in bufs.y], sp_in=bufs.sp_in.clone(),
               fc=[t.view(B, K, -1).clone() for t in (bufs.h1, bufs.h2, bufs.feats)], feats=feats.clone(), sp_pred=sp_pred.clone(),
               pred=bufs.pred.clone(), y_all=y_all.clone(), src=src.clone(), sim=sim.clone(), terms=terms.clone(),
               grads={k: v.detach().clone() for k, v in m._grad_views.items()})
    m.engine.release_buffers()
    del trainer, m, bufs
    torch.cuda.empty_cache()
    return out


def _compare_image(case, bat, b, one, img, weights, rows_budget):
    """Image b of the batched run against its single run (image 0 of ``one``); its conv layers against fp64.
    Returns (decisions that differ, units of the image whose decisions were compared, loss-bar widening masked / propagated)."""
    n, n_l = int(one['n_sp'][0]), int(one['n_l'][0])
    # integers bit-exact
    assert int(bat['n_sp'][b]) == n and int(bat['n_l'][b]) == n_l and bat['Kmax'] == one['Kmax']
    assert torch.equal(bat['perm'][b, :n], one['perm'][0, :n]) and torch.equal(bat['new_row'][b], one['new_row'][0])
    assert torch.equal(bat['sp_labels'][b, :n_l], one['sp_labels'][0, :n_l])
    # every conv layer's pre-activation against the single run, and against fp64 from the batched run's own input
    ys = [y[b].permute(2, 0, 1) for y in bat['y']]
    ys1 = [y[0].permute(2, 0, 1) for y in one['y']]
    same = 0
    for l in range(13):
        e = float((ys[l] - ys1[l]).abs().max()) / float(ys1[l].abs().max())
        same += int(e == 0.0)
        assert _tol.within(case, 'conv pre-activation, batched vs single (per layer)', e, BAR,
                           'max |y_batch - y_single| / max |y_single| per layer and image'), (b, l, e)
    _tol.within(case, 'conv layers bit-identical, batched vs single (count of 13; no bar)', same, 13, 'recorded only')
    _parity.check_conv_layers(case, img, ys, weights, BAR)
    # the 2112-wide superpixel input slice by slice; features and superpixel predictions
    ok, errs = _parity.check_sp_slices(case, 'sp_in per slice, batched vs single', bat['sp_in'][b, :n], one['sp_in'][0, :n], BAR,
                                       'superpixel input of the fc layers, image b of the batch against its single run')
    assert ok, (b, errs)
    assert _tol.within(case, 'sp_features, batched vs single', rel_err(bat['feats'][b, :n], one['feats'][0, :n]), BAR), b
    assert _tol.within(case, 'sp_pred, batched vs single', rel_err(bat['sp_pred'][b, :n], one['sp_pred'][0, :n]), BAR), b
    # propagation: src and y_u equal except rows decided within rounding (their count bounded)
    near = _parity.near_tie_rows(one['feats'][0, :n], one['sp_labels'][0, :n_l]).to(bat['src'].device)
    assert _tol.within(case, 'propagation rows masked as near-ties, batched vs single (count)', int(near.sum()), rows_budget,
                       f'of {n - n_l} unlabelled rows, per image'), (b, int(near.sum()))
    differ = (bat['src'][b, n_l:n] != one['src'][0, n_l:n]) | (bat['y_all'][b, n_l:n] != one['y_all'][0, n_l:n]).any(dim=1)
    assert not bool((differ & ~near).any()), (b, int((differ & ~near).sum()))
    # painted prediction: rounded labels equal except pixels within 1e-5 of 0.5
    pb, p1 = bat['pred'][b], one['pred'][0]
    amb = ((pb - 0.5).abs() < 1e-5) | ((p1 - 0.5).abs() < 1e-5)
    assert torch.equal(pb.round()[~amb], p1.round()[~amb]), b
    # this image's row of the per-image loss terms (sup, sup count, propagated, propagated count, labels, loss)
    t, t1 = bat['terms'][b, :6].double().cpu(), one['terms'][0, :6].double().cpu()
    widen = int(near.sum()) / max(float(t1[4]), 1.0)
    e = float(((t - t1).abs() / t1.abs().clamp_min(1e-30)).max())
    assert _tol.within(case, 'per-image loss terms, batched vs single', e, BAR + widen,
                       'max over the row of |t_batch - t_single| / |t_single|; bar 1e-5 + masked / propagated rows'), (b, t, t1)
    # discrete decisions the batched forward takes differently from the single one
    count, bad = _parity.decision_diffs(ys, ys1, [h[b, :n] for h in bat['fc']], [h[0, :n] for h in one['fc']])
    assert not bad, (b, bad)
    return count + int(differ.sum()), sum(int(y.numel()) for y in ys) + sum(int(h[b, :n].numel()) for h in bat['fc']), widen


def _compare_batch(case, bat, singles, imgs, weights, rows_budget):
    d = torch.device('cuda:0')
    B = len(singles)
    total, widen_sum = 0, 0.0
    for b, one in enumerate(singles):
        k, n_units, widen = _compare_image(f'{case} image {b}', bat, b, one, torch.from_numpy(imgs[b]).to(d), weights, rows_budget)
        budget = max(_gradcheck.NEAR_TIE_FLOOR, int(np.ceil(_gradcheck.NEAR_TIE_BUDGET_PER_M * n_units / 1e6)))
        assert _tol.within(f'{case} image {b}', 'near-tie decisions differing, batched vs single (count)', k, budget,
                           'ReLU signs of conv and fc units, pooling arg-max, propagation rows; every one a near-tie'), (b, k, budget)
        total += k
        widen_sum += widen
    # the batch's loss and metrics against the mean of the single runs
    mean = lambda key: float(np.mean([s[key] for s in singles]))
    assert _tol.within(case, 'loss, batched vs mean of singles', abs(bat['loss'] - mean('loss')) / abs(mean('loss')),
                       BAR + widen_sum / B, 'relative'), (bat['loss'], mean('loss'))
    assert abs(bat['accuracy'] - mean('accuracy')) < 1e-6 and abs(bat['dice'] - mean('dice')) < 1e-6
    # gradients: the batch's against the mean of the single-image gradients, per parameter tensor
    bar = GRAD_REORDER if total == 0 else GRAD_NEAR_TIE
    for k, g in bat['grads'].items():
        ref = sum(s['grads'][k].double() for s in singles) / B
        scale = float(ref.abs().max())
        e = float((g.double() - ref).abs().max()) / scale if scale > 0 else float(g.abs().max())
        assert _tol.within(case, 'gradients, batched vs mean of singles', e, bar,
                           f'max |g - mean_b g_b| / max |mean_b g_b| per tensor; {GRAD_REORDER} when no decision differs, '
                           f'{GRAD_NEAR_TIE} when only named near-ties do'), (k, e, total)
    return total


def _singles(weights, arrays, g):
    B = arrays[0].shape[0]
    return [_run(weights, tuple(np.ascontiguousarray(a[b:b + 1]) for a in arrays), g) for b in range(B)]


def test_c4_shard_image_by_image_and_image_0_against_the_reference(golden_dir):
    """B = 4 at 800x800, 1521 superpixels: image 0 is the c800_g39 golden's input (its point mask also serves as the
    pixel mask, as in test_step_matches_the_reference_at_full_size) with the golden's weights, images 1-3 synthetic."""
    from oracle import wesup_oracle as orc
    from wesup_amd import synth
    torch.set_num_threads(min(16, os.cpu_count() or 1))
    fx = load_full_size_case(golden_dir, 'c800_g39')
    B, H, W, g = 4, 800, 800, 39
    assert (int(fx['H']), int(fx['W']), int(fx['g'])) == (H, W, g)
    weights = orc.make_weights(int(fx['seed']), feat_scale=float(fx['feat_scale']))
    imgs, labs, pts, pix = synth.make_batch(3, B, H, W, g)
    imgs[0], labs[0] = fx['img'], fx['seg']
    pts[0] = fx['mask']
    pix[0] = fx['mask']
    arrays = (imgs, pix, pts, labs)
    bat = _run(weights, arrays, g)
    singles = _singles(weights, arrays, g)
    n_dec = _compare_batch('c4_shard', bat, singles, imgs, weights, MASKED_ROWS_BUDGET)

    # image 0 of the batch against the real reference, with the bars of test_step_matches_the_reference_at_full_size
    name = 'c4_shard image 0 (c800_g39)'
    ref = 'max |a - b| / max |b| against the real reference (tests/golden)'
    K, n_l = int(fx['seg'].max()) + 1, fx['sp_labels'].shape[0]
    assert int(bat['n_sp'][0]) == K and int(bat['n_l'][0]) == n_l
    assert np.array_equal(bat['sp_labels'][0, :n_l].cpu().numpy(), fx['sp_labels'])
    assert np.array_equal(bat['new_row'][0].cpu().numpy().reshape(H, W).astype(np.int16), fx['new_row'])
    assert _tol.within(name, 'sp_features vs reference', rel_err(bat['feats'][0, :K], fx['sp_features']), TOL, ref)
    assert _tol.within(name, 'sp_pred vs reference', rel_err(bat['sp_pred'][0, :K], fx['sp_pred']), TOL, ref)
    assert _tol.within(name, 'pred (painted) vs reference', rel_err(bat['pred'][0, ::7, ::11], fx['pred_sample']), TOL, ref)
    assert np.array_equal(bat['pred'][0:1].round().long().cpu().numpy().astype(np.int8), fx['post_pred'])
    assert np.array_equal(bat['src'][0, n_l:K].cpu().numpy(), fx['src'])
    assert np.array_equal(bat['y_all'][0, n_l:K].cpu().numpy(), fx['y_u'])
    assert _tol.within(name, 'max_sim vs reference', rel_err(bat['sim'][0, n_l:K], fx['max_sim']), TOL, ref)
    t = bat['terms'][0].double().cpu().numpy()
    assert _tol.within(name, 'loss vs reference', abs(t[5] - float(fx['loss'])) / abs(float(fx['loss'])), TOL, 'relative')
    assert t[4] == float(fx['propagated_labels'])
    assert _tol.within(name, 'propagate_loss vs reference', abs(t[2] / t[3] - float(fx['propagate_loss'])) / abs(float(fx['propagate_loss'])),
                       TOL, 'relative')
    assert abs(n_l / K - float(fx['labeled_sp_ratio'])) < 1e-7
    print(f'c4 shard: loss {bat["loss"]:.6f} (mean of singles {np.mean([s["loss"] for s in singles]):.6f}), '
          f'{n_dec} decisions differ between the batch and its single runs')


def test_c5_shard_image_by_image():
    """B = 8 at 1024x1024, 3025 superpixels.  Image 0 is exactly the input of test_one_image_of_config_c5_matches_the_oracle
    (same seed, same weights): batched -> single -> oracle is one chain."""
    from oracle import wesup_oracle as orc
    from wesup_amd import synth
    torch.set_num_threads(min(16, os.cpu_count() or 1))
    B, H, W, g = 8, 1024, 1024, 55
    weights = orc.make_weights(0, feat_scale=1.0)
    arrays = synth.make_batch(7, B, H, W, g)
    for a, a1 in zip(arrays, synth.make_batch(7, 1, H, W, g)):
        assert np.array_equal(a[:1], a1)
    imgs, labs, pts, pix = arrays
    arrays = (imgs, pix, pts, labs)
    bat = _run(weights, arrays, g)
    singles = _singles(weights, arrays, g)
    n_dec = _compare_batch('c5_shard', bat, singles, imgs, weights, MASKED_ROWS_BUDGET * 5)
    print(f'c5 shard: loss {bat["loss"]:.6f} (mean of singles {np.mean([s["loss"] for s in singles]):.6f}), '
          f'{n_dec} decisions differ between the batch and its single runs')
