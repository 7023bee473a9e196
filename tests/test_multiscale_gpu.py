"""Parity of the training step at the multi-scale operating point that ``bench.py --multiscale`` times: batch 1 at
int(522 f) x int(775 f), Voronoi label maps at sp_area 200 handed over as ``LabelMaps`` with their counts, Kmax the count
rounded up to 64 (``max_superpixels=None``), against the CPU oracle's training step.

At these sizes most deep levels have a cell count that is not a multiple of 4 and take the GATHER form of the superpixel
pooling (engine rule: matrix form only for coarse grids of at most 4096 cells, ``cells % 4 == 0``), on odd grids such as
39x58 or 13x19 with 128- and 256-channel side outputs, and the Winograd tiles are ragged at almost every level.  The four
factors cover odd and 2-mod-4 sizes, both pooling forms and padded and unpadded Kmax.  Every conv layer is checked over its
WHOLE output against an fp64 conv of the GPU's own input, the 2112-wide superpixel input slice by slice, the loss, the
propagation, the painted prediction and metrics, every parameter gradient against fp64 under the GPU's decisions and the
SGD update."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _gradcheck          # noqa: E402
import _parity             # noqa: E402
import _tol                # noqa: E402
from test_fullsize_gpu import MASKED_ROWS_BUDGET, TOL, loss_under_gpu_decisions, make_trainer, rel_err    # noqa: E402

pytestmark = pytest.mark.gpu

# f -> (H, W, superpixels, Kmax, {deep-level grid: matrix form?})
SHAPES = {
    0.30: (156, 232, 169, 192, {(39, 58): False, (19, 29): False, (9, 14): False}),
    0.35: (182, 271, 256, 256, {(45, 67): False, (22, 33): False, (11, 16): True}),
    0.3787: (197, 293, 289, 320, {(49, 73): False, (24, 36): True, (12, 18): True}),
    0.40: (208, 310, 324, 384, {(52, 77): True, (26, 38): True, (13, 19): False}),
}
# pre-activation against fp64 conv of the GPU's own input, whole layer: 1e-5 of the layer's max (worst observed 1.8e-6 on the first
# green run of these tests, profiles/tolerances_shards_multiscale.json; sp_in slices vs the oracle 1.7e-6, gradients vs fp64 3.1e-6)
CONV_BAR = 1e-5


@pytest.mark.parametrize('f', sorted(SHAPES))
def test_multiscale_step_matches_the_oracle(f):
    from oracle import wesup_oracle as orc
    from wesup_amd import synth, ops
    from wesup_amd.utils.data import LabelMaps
    torch.set_num_threads(min(16, os.cpu_count() or 1))
    d = torch.device('cuda:0')
    H, W, n_sp, kmax, forms = SHAPES[f]
    assert (H, W) == (int(522 * f), int(775 * f))
    gi = max(2, int(round((H * W / 200.0) ** 0.5)))                     # sp_area 200, as bench.py --multiscale
    assert gi * gi == n_sp
    case = f'multiscale f={f} {H}x{W}'
    weights = orc.make_weights(0, feat_scale=1.0)                       # only some rows propagate at these sizes
    imgs, labs, pts, pix = synth.make_batch(41, 1, H, W, gi)
    ref_loss, ref_grads, ref_new, _, outs, mets = orc.train_step(weights, imgs, labs.astype(np.int64), pts.astype(np.int64))

    trainer = make_trainer(weights)
    trainer.kwargs['max_superpixels'] = None                            # rows = the label map's own count
    trainer.train_one_iteration('train', torch.from_numpy(imgs).to(d), torch.from_numpy(pix).to(d), torch.from_numpy(pts).to(d),
                                LabelMaps(torch.from_numpy(labs).to(d), [int(labs.max()) + 1]))
    model, hist = trainer.model, trainer.tracker.history
    meta = model._last_meta
    bufs = model.engine._last
    assert meta.Kmax == kmax and (meta.B, meta.H, meta.W) == (1, H, W)
    # the pooling form of every deep level is the one this case is here for
    for l in range(13):
        if bufs.dims[l] in forms:
            assert (bufs.group_of[l] is not None) == forms[bufs.dims[l]], (l, bufs.dims[l])
    # integer outputs bit-exact
    pp = outs[0]['pp']
    n, n_l = pp['K'], pp['n_l']
    assert n == n_sp == int(meta.n_sp[0]) and int(meta.n_l[0]) == n_l and 0 < n_l < n
    assert torch.equal(meta.perm[0, :n].cpu().long(), pp['perm']) and torch.equal(meta.sp_labels[0, :n_l].cpu(), pp['sp_labels'])
    assert torch.equal(meta.new_row[0].cpu().long().reshape(-1), pp['inv_perm'][torch.from_numpy(labs[0]).long().view(-1)])
    # every conv layer over its whole output against fp64 from the GPU's own input
    img = torch.from_numpy(imgs[0]).to(d)
    ys = [y[0].permute(2, 0, 1) for y in bufs.y]
    _parity.check_conv_layers(case, img, ys, weights, CONV_BAR, full=True)
    # the superpixel input of the fc layers, slice by slice, and the features against the oracle
    ok, errs = _parity.check_sp_slices(case, 'sp_in per slice vs oracle', bufs.sp_in[0, :n], outs[0]['sp_in'].detach(), TOL,
                                       'GPU superpixel input of the fc layers against the oracle\'s fp32')
    assert ok, errs
    feats = bufs.feats.view(1, meta.Kmax, -1)
    assert _tol.within(case, 'sp_features vs oracle', rel_err(feats[0, :n], outs[0]['sp_features']), TOL)
    # the loss under the GPU's propagation decisions; the propagation itself except near-tie rows
    y_all, src, _ = ops.propagate(feats.contiguous(), meta, 0.8)
    loss_ref, n_near = loss_under_gpu_decisions(orc, outs[0], y_all[0])
    assert _tol.within(case, 'loss vs oracle', abs(hist['loss'][0] - loss_ref) / abs(ref_loss), TOL, 'relative')
    if n_near == 0:
        assert abs(hist['loss'][0] - ref_loss) <= TOL * abs(ref_loss)
        assert hist['propagated_labels'][0] == mets[0]['propagated_labels']
        assert abs(hist['propagate_loss'][0] - mets[0]['propagate_loss']) < 1e-5
    assert 0 < mets[0]['propagated_labels'] < n - n_l                   # some rows propagate, some do not
    assert abs(hist['labeled_sp_ratio'][0] - mets[0]['labeled_sp_ratio']) < 1e-7
    y_u, _, _, src_ref = orc.label_propagate(outs[0]['sp_features'], pp['sp_labels'], 0.8, return_aux=True)
    near = _parity.near_tie_rows(outs[0]['sp_features'], pp['sp_labels'])
    assert _tol.within(case, 'propagation rows masked as near-ties before src / y_u are compared (count)', int(near.sum()),
                       MASKED_ROWS_BUDGET, f'of {n - n_l} unlabelled rows'), int(near.sum())
    assert torch.equal(src[0, n_l:n].cpu().long()[~near], src_ref[~near]) and torch.equal(y_all[0, n_l:n].cpu()[~near], y_u[~near])
    # painted prediction and metrics
    P = bufs.pred[0].round().long().cpu()
    assert torch.equal(P, outs[0]['pred'].detach().round().long())
    G = torch.from_numpy(pix[0]).long().argmax(dim=0)
    assert abs(hist['accuracy'][0] - orc.accuracy(P, G)) < 1e-6 and abs(hist['dice'][0] - orc.dice(P, G)) < 1e-6
    del outs, ref_grads
    # every parameter gradient against fp64 under the GPU's decisions, and the SGD update against the oracle's
    worst, n_named = _gradcheck.check_gradients(model, weights, imgs, labs, pts, case=case)
    new = {k: v.detach().cpu() for k, v in model.state_dict().items()}
    for k, v in ref_new.items():
        assert _tol.within(case, 'updated parameters (SGD) vs oracle', rel_err(new[k], v), 1e-5), k
    print(f'{case}: Kmax {meta.Kmax}, loss {hist["loss"][0]:.6f} (oracle {ref_loss:.6f}), worst sp_in slice {max(errs):.2e}, '
          f'worst gradient error vs fp64 {worst:.2e}, {n_named} near-tie decisions differ')
    model.engine.release_buffers()
    torch.cuda.empty_cache()
