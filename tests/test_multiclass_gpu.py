"""The C-way head (2 <= C <= 16): classifier, fused head launches, class-map painting, confusion table, the training step,
record / replay and pixel inference for more than two classes -- and the two-class step's launch list, which must not move.

Bars: those the two-class entries are held to (tests/test_kernels_gpu.py, tests/test_step_gpu.py); bit equality wherever two
routes run the same arithmetic (fused / unfused, C = 2 old / new entries, walk / replay, run to run)."""
import ctypes
import json
import os
import sys

import numpy as np
import pytest
import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _gradcheck          # noqa: E402

pytestmark = pytest.mark.gpu

TOL = 1e-4                 # tests/test_kernels_gpu.py's and tests/test_step_gpu.py's


def dev():
    return torch.device('cuda:0')


@pytest.fixture(scope='module')
def ops():
    from wesup_amd import ops as o
    return o


def rnd(*shape, seed=0, scale=1.0):
    return torch.from_numpy((np.random.RandomState(seed).randn(*shape) * scale).astype(np.float32))


def rel_err(a, b):
    a = torch.as_tensor(a).detach().double().cpu()
    b = torch.as_tensor(b).detach().double().cpu()
    return float((a - b).abs().max() / (b.abs().max() + 1e-30))


def weights_c(seed, C, feat_scale=0.03):
    """orc.make_weights with a seeded C-way classifier made the same way (std = sqrt(1/32), bias * 0.05)."""
    from oracle import wesup_oracle as orc
    w = orc.make_weights(seed, feat_scale=feat_scale)
    rs = np.random.RandomState(1000 + seed)
    w['classifier.0.weight'] = (rs.randn(C, 32) * np.sqrt(1.0 / 32)).astype(np.float32)
    w['classifier.0.bias'] = (rs.randn(C) * 0.05).astype(np.float32)
    return w


def make_trainer(weights, **kw):
    from wesup_amd.models import initialize_trainer
    from wesup_amd.utils.metrics import accuracy, dice
    C = weights['classifier.0.weight'].shape[0]
    t = initialize_trainer('wesup', device='cuda:0', n_classes=C, **kw)
    t.model.load_state_dict({k: torch.from_numpy(v) for k, v in weights.items()})
    t.optimizer, t.scheduler = t.get_default_optimizer()
    t.metric_funcs = [accuracy, dice]
    t.model.train()
    t.tracker.train()
    return t


def batch_c(seed, B, H, W, gs, C, frac=0.3, tie_every=4):
    from wesup_amd import synth
    imgs = np.stack([synth.synth_image(seed + 100 + b, H, W) for b in range(B)])
    segs = np.stack([synth.voronoi_labels(seed + 200 + b, H, W, gs[b]) for b in range(B)])
    pts = np.stack([synth.point_mask(seed + 300 + b, segs[b], frac, C, tie_every=tie_every) for b in range(B)])
    pix = np.stack([synth.pixel_mask(seed + 400 + b, H, W, C) for b in range(B)])
    return imgs, segs, pts, pix


# ---------------------------------------------------------------- 1. classifier forward and backward
@pytest.mark.parametrize('D', [32, 7])
@pytest.mark.parametrize('C', [2, 3, 5, 16])
def test_classifier_c_against_fp64_and_the_two_class_entries(ops, C, D):
    from wesup_amd import _lib
    lib, p, st = _lib.load(), ops._p, ops._stream()
    d = dev()
    for R in (1, 63, 64, 65, 300):
        pre = rnd(R, D, seed=R + 6).double().requires_grad_(True)           # feat = relu(pre): the ReLU mask
        Wc = rnd(C, D, seed=C + 2, scale=0.3).double().requires_grad_(True)
        bc = rnd(C, seed=C + 3).double().requires_grad_(True)
        featr = F.relu(pre)
        pred = F.softmax(F.linear(featr, Wc, bc), dim=1)
        dpred, extra = rnd(R, C, seed=R + 4), rnd(R, D, seed=R + 5)
        dp = dpred.to(d)
        (pred * dpred.double()).sum().backward(retain_graph=True)
        g_plain = {k: v.grad.clone() for k, v in (('pre', pre), ('Wc', Wc), ('bc', bc))}
        (featr * extra.double()).sum().backward()
        f32 = featr.detach().float().to(d)
        W32, b32 = Wc.detach().float().to(d), bc.detach().float().to(d)
        pg = ops.classifier_fwd(f32, W32, b32)
        assert tuple(pg.shape) == (R, C)
        assert rel_err(pg, pred) < 1e-5, (R, rel_err(pg, pred))
        if C == 2:                                                        # the two-class ABI entry, bit for bit
            old_p = torch.full_like(pg, 9.0)
            assert lib.wesup_classifier_fwd(p(f32), p(W32), p(b32), p(old_p), R, D, st) == 0
            assert torch.equal(old_p, pg), R
        for ex, ref_pre in ((extra.to(d), pre.grad), (None, g_plain['pre'])):                 # with and without dfeat_extra
            dfeat, dWc, dbc = ops.classifier_bwd(f32, W32, pg, dp, ex)
            assert rel_err(dfeat, ref_pre) < TOL, (R, rel_err(dfeat, ref_pre))
            assert float(dfeat[f32 <= 0].abs().sum()) == 0.0                                  # masked where feat <= 0
            assert rel_err(dWc, Wc.grad) < TOL and rel_err(dbc, bc.grad) < TOL, R
            if C == 2:                                                                         # the two-class ABI entries, bit for bit
                old = [torch.full_like(x, 9.0) for x in (dfeat, dWc, dbc)]
                nb = lib.wesup_classifier_bwd_workspace_bytes(R, D)
                assert nb == lib.wesup_classifier_bwd_c_workspace_bytes(R, D, 2)
                ws = torch.zeros(nb, dtype=torch.uint8, device=d)
                assert lib.wesup_classifier_bwd(p(f32), p(W32), p(pg), p(dp), p(ex), p(old[0]),
                                                p(old[1]), p(old[2]), R, D, p(ws), nb, st) == 0
                assert torch.equal(old[0], dfeat) and torch.equal(old[1], dWc) and torch.equal(old[2], dbc), R


def test_class_count_outside_the_range_is_invalid(ops):
    from wesup_amd import _lib
    lib = _lib.load()
    d = dev()
    R, D = 8, 32
    p = lambda t: ctypes.c_void_p(t.data_ptr())
    for C in (1, 17):
        f, W, b, o = (torch.zeros(R, D, device=d), torch.zeros(C, D, device=d), torch.zeros(C, device=d), torch.zeros(R, C, device=d))
        ws = torch.zeros(1 << 16, dtype=torch.uint8, device=d)
        assert lib.wesup_classifier_fwd_c(p(f), p(W), p(b), p(o), R, D, C, None) == -1
        assert lib.wesup_classifier_bwd_c_workspace_bytes(R, D, C) == 0
        assert lib.wesup_classifier_bwd_c(p(f), p(W), p(o), p(o), None, p(f), p(W), p(b), R, D, C, p(ws), ws.numel(), None) == -1
        assert lib.wesup_classifier_bwd_c_finish(p(ws), ws.numel(), p(W), p(b), R, D, C, None) == -1
    assert ops.MAX_CLASSES == 16


# ---------------------------------------------------------------- 2. fused equals unfused
def _head_meta(ops, B, Kmax, C, n_sp, n_l, seed):
    """A hand-made superpixel description for the head entries: labelled rows first (one-hot, every fourth a two-class tie)."""
    rs = np.random.RandomState(seed)
    lab = np.zeros((B, Kmax, C), dtype=np.float32)
    for b in range(B):
        for r in range(n_l[b]):
            lab[b, r, rs.randint(C)] = 1.0
            if r % 4 == 3:
                lab[b, r] = 0.0
                lab[b, r, rs.choice(C, 2, replace=False)] = 0.5
    m = ops.SuperpixelMeta()
    m.B, m.Kmax, m.C = B, Kmax, C
    m.sp_labels = torch.from_numpy(lab).to(dev())
    m.n_sp = torch.tensor(n_sp, dtype=torch.int32, device=dev())
    m.n_l = torch.tensor(n_l, dtype=torch.int32, device=dev())
    return m


@pytest.mark.parametrize('Kmax', [64, 128])
@pytest.mark.parametrize('C', [3, 5])
def test_fused_head_c_equals_the_separate_entries_bit_for_bit(ops, C, Kmax):
    d = dev()
    B, D = 3, 32
    n_sp = [Kmax - 14, Kmax, Kmax // 2 + 5]                    # ragged
    n_l = [0, Kmax, 20]                                        # none labelled, fully labelled, mixed
    m = _head_meta(ops, B, Kmax, C, n_sp, n_l, seed=C + Kmax)
    feat = F.relu(rnd(B, Kmax, D, seed=C, scale=0.1)).to(d)
    Wc, bc = rnd(C, D, seed=C + 7).to(d), rnd(C, seed=C + 8).to(d)
    R = B * Kmax
    pred = ops.classifier_fwd(feat.view(R, D), Wc, bc)
    y_all, src, sim = ops.propagate(feat, m, 0.8)
    _, terms = ops.loss_fwd(pred.view(B, Kmax, C), y_all, m, 1e-7, 0.5)
    dloss = torch.tensor([1.0], device=d)
    dpred = ops.loss_bwd(pred.view(B, Kmax, C), y_all, m, terms, dloss, 1e-7, 0.5)
    dfeat, dWc, dbc = ops.classifier_bwd(feat.view(R, D), Wc, pred, dpred.view(R, C))
    assert ops.head_supported(Kmax, C)
    pred2 = torch.full((R, C), 9.0, device=d)
    out2 = (torch.full((B, Kmax, C), 9.0, device=d), torch.full((B, Kmax), 9, dtype=torch.int32, device=d),
            torch.full((B, Kmax), 9.0, device=d))
    ops.head_fwd(feat, Wc, bc, pred2, m, 0.8, out=out2)
    assert torch.equal(pred2, pred) and torch.equal(out2[0], y_all) and torch.equal(out2[1], src) and torch.equal(out2[2], sim)
    terms2, dpred2 = torch.full((B, 8), 9.0, device=d), torch.full((B, Kmax, C), 9.0, device=d)
    dfeat2, dWc2, dbc2 = torch.full((R, D), 9.0, device=d), torch.full((C, D), 9.0, device=d), torch.full((C,), 9.0, device=d)
    part = ops.head_bwd_partials(R, D, d, C=C)
    ops.head_bwd(feat.view(R, D), Wc, pred2, out2[0], m, dloss, 1e-7, 0.5, terms2, dpred2, dfeat2, part)
    ops.classifier_bwd_finish(part, R, D, dWc2, dbc2)
    assert torch.equal(terms2, terms) and torch.equal(dpred2, dpred) and torch.equal(dfeat2, dfeat)
    assert torch.equal(dWc2, dWc) and torch.equal(dbc2, dbc)
    assert float(dpred.abs().max()) > 0 and float(dfeat.abs().max()) > 0
    assert int((src[2] >= 0).sum()) > 0 and float(y_all[2, 20:n_sp[2]].sum()) > 0          # the mixed image propagates
    assert not ops.head_supported(100, 3) and not ops.head_supported(64, 1) and not ops.head_supported(64, 17)


# ---------------------------------------------------------------- 3. class-map painting
def test_paint_argmax_takes_the_first_maximum(ops):
    d = dev()
    B, H, W, C, Kmax = 2, 37, 29, 3, 20
    rs = np.random.RandomState(5)
    sp = F.softmax(torch.from_numpy(rs.randn(B, Kmax, C).astype(np.float32)), dim=2).numpy()
    sp[0, 0] = [0.4, 0.4, 0.2]
    sp[0, 1] = [0.2, 0.4, 0.4]
    sp[0, 2] = [0.4, 0.2, 0.4]
    sp[1, 3] = [0.25, 0.25, 0.25]                              # three-way tie
    sp[1, 4] = [0.0, 0.5, 0.5]
    new_row = rs.randint(0, Kmax, size=(B, H * W)).astype(np.int32)
    new_row[:, :8] = np.arange(8)                              # every tie row is painted somewhere
    m = ops.SuperpixelMeta()
    m.B, m.H, m.W, m.Kmax, m.C = B, H, W, Kmax, C
    m.new_row = torch.from_numpy(new_row).to(d)
    out = torch.full((B, H, W), 9.0, device=d)
    ops.paint_argmax(torch.from_numpy(sp).to(d), m, out=out)
    cls = sp.argmax(axis=2)                                    # numpy: the first maximum
    ref = np.stack([cls[b][new_row[b]] for b in range(B)]).reshape(B, H, W).astype(np.float32)
    assert torch.equal(out.cpu(), torch.from_numpy(ref))
    assert ref[0].reshape(-1)[:3].tolist() == [0.0, 1.0, 0.0] and ref[1].reshape(-1)[3:5].tolist() == [0.0, 1.0]
    assert torch.equal(ops.paint(torch.from_numpy(sp).to(d), m), out)


# ---------------------------------------------------------------- 4. confusion table
@pytest.mark.parametrize('HW', [1, 255, 64 * 256 + 3])
@pytest.mark.parametrize('C', [3, 16])
def test_seg_confusion_is_exact_and_starts_from_zero(ops, C, HW):
    d = dev()
    B = 2
    rs = np.random.RandomState(C + HW)
    P = rs.randint(0, C, size=(B, HW))
    G = rs.randint(0, C, size=(B, HW))
    mask = np.zeros((B, C, HW), dtype=np.uint8)
    for b in range(B):
        mask[b, G[b], np.arange(HW)] = 1
    # every 7th pixel: a second, equal maximum in a higher plane -- the lower class stays the ground truth; every 11th: no plane set
    # (class 0, the first maximum of all-equal planes)
    for b in range(B):
        for p in range(0, HW, 7):
            mask[b, min(G[b, p] + 1, C - 1), p] = 1
        for p in range(5, HW, 11):
            mask[b, :, p] = 0
            G[b, p] = 0
    ref = np.zeros((B, C, C), dtype=np.int64)
    for b in range(B):
        np.add.at(ref[b], (G[b], P[b]), 1)
    pred = torch.from_numpy(P.astype(np.float32)).view(B, 1, HW).to(d)
    mk = torch.from_numpy(mask).view(B, C, 1, HW).to(d)
    conf = torch.full((B, C, C), 77, dtype=torch.int32, device=d)          # a dirty buffer
    status = torch.full((1,), 5, dtype=torch.int32, device=d)
    ops.seg_confusion(pred, mk, out=conf, status=status)
    assert np.array_equal(conf.cpu().numpy().astype(np.int64), ref) and int(status) == 0
    ops.seg_confusion(pred, mk, out=conf, status=status)                   # again into the same buffer: the same table
    assert np.array_equal(conf.cpu().numpy().astype(np.int64), ref) and int(status) == 0
    assert int(conf.sum()) == B * HW
    bad = pred.clone()
    bad[1, 0, 0] = float(C)
    ops.seg_confusion(bad, mk, out=conf, status=status)
    assert int(status) != 0 and int(conf.sum()) == B * HW - 1


# ---------------------------------------------------------------- 5. the training step against the oracle
@pytest.mark.parametrize('B,H,W,gs,C', [(3, 64, 48, [5, 6, 4], 3), (1, 32, 32, [4], 5)])
def test_multiclass_step_matches_oracle(B, H, W, gs, C):
    from oracle import wesup_oracle as orc
    from wesup_amd.utils import metrics as M
    d = dev()
    weights = weights_c(11, C)
    imgs, segs, pts, pix = batch_c(0, B, H, W, gs, C)
    ref_loss, ref_grads, ref_new, _, outs, mets = orc.train_step(weights, imgs, segs.astype(np.int64), pts.astype(np.int64))
    # accuracy / dice by their definitions, on the oracle's class map sp_pred[seg_new].argmax(1)
    G = pix.argmax(axis=1)
    conf = []
    for b in range(B):
        seg_new = outs[b]['pp']['inv_perm'][torch.from_numpy(segs[b].reshape(-1)).long()]
        Pb = outs[b]['sp_pred'].detach().numpy()[seg_new.numpy()].argmax(axis=1)
        t = np.zeros((C, C), dtype=np.int64)
        np.add.at(t, (G[b].reshape(-1), Pb), 1)
        conf.append(t)
    acc = np.mean([np.trace(t) / t.sum() for t in conf])
    dices = []
    for t in conf:
        present = (t.sum(0) + t.sum(1)) > 0
        dices.append(np.mean(2 * np.diag(t)[present] / (t.sum(1)[present] + t.sum(0)[present] + 1e-7)))
    results = []
    for rep in range(2):
        trainer = make_trainer(weights)
        assert trainer.model.classifier[0].weight.shape == (C, 32)
        data = (torch.from_numpy(imgs).to(d), torch.from_numpy(pix).long().to(d), torch.from_numpy(pts).long().to(d),
                torch.from_numpy(segs))
        trainer.train_one_iteration('train', *data)
        hist = trainer.tracker.history
        print(f'C={C} rep={rep} loss {hist["loss"][0]!r} oracle {ref_loss!r}; accuracy {hist["accuracy"][0]!r} / {acc!r}; '
              f'dice {hist["dice"][0]!r} / {np.mean(dices)!r}')
        assert abs(hist['loss'][0] - ref_loss) <= TOL * abs(ref_loss)
        assert abs(hist['propagated_labels'][0] - np.mean([m['propagated_labels'] for m in mets])) < 1e-6
        assert abs(hist['labeled_sp_ratio'][0] - np.mean([m['labeled_sp_ratio'] for m in mets])) < 1e-6
        assert abs(hist['accuracy'][0] - acc) < 1e-6
        assert abs(hist['dice'][0] - np.mean(dices)) < 1e-6
        assert abs(M.accuracy_from_confusion(np.stack(conf)) - acc) < 1e-12 and abs(M.dice_from_confusion(np.stack(conf)) - np.mean(dices)) < 1e-12
        grads = {k: trainer.model._grad_views[k].clone() for k in ref_grads}
        assert grads['classifier.0.weight'].shape == (C, 32)
        if rep == 0:
            worst, _ = _gradcheck.check_gradients(trainer.model, weights, imgs, segs, pts)
            assert worst < 1e-4, worst
        new = {k: v.detach().cpu() for k, v in trainer.model.state_dict().items()}
        for k, v in ref_new.items():
            assert rel_err(new[k], v) < 1e-5, k
        results.append((hist['loss'][0], {k: v.cpu() for k, v in grads.items()}))
    assert results[0][0] == results[1][0]
    for k in results[0][1]:
        assert torch.equal(results[0][1][k], results[1][1][k]), k


# ---------------------------------------------------------------- 6. record / replay
def test_multiclass_step_replays_bit_for_bit():
    d = dev()
    C, B, H, W, g = 3, 2, 64, 64, 4
    weights = weights_c(5, C, feat_scale=0.05)
    data = []
    for i in range(3):
        imgs, segs, pts, pix = batch_c(1000 * i, B, H, W, [g] * B, C, frac=0.2, tie_every=0)
        data.append(tuple(torch.from_numpy(a).to(d) for a in (imgs, pix, pts, segs)))
    a = make_trainer(weights, max_superpixels=g * g, step_plan=False)
    b = make_trainer(weights, max_superpixels=g * g)
    for i in range(6):
        a.train_one_iteration('train', *data[i % 3])
        b.train_one_iteration('train', *data[i % 3])
        for k in ('loss', 'labeled_sp_ratio', 'propagated_labels', 'propagate_loss', 'accuracy', 'dice'):
            assert a.tracker.history[k][-1] == b.tracker.history[k][-1], (i, k)
        assert torch.equal(a.model._flat, b.model._flat), f'parameters differ after step {i}'
        assert torch.equal(a.model._flat_grad, b.model._flat_grad), f'gradients differ after step {i}'
    st = b.step_runner().stats
    assert st['replayed'] > 0 and st['dropped'] == 0, st
    assert a.step_runner().stats['replayed'] == 0
    names = _plan_names(b)[1]
    assert any('head_bwd_c_kernel' in n for n in names) and any('prop_c_kernel' in n for n in names)
    assert any('seg_confusion_kernel' in n for n in names) and any('row_argmax_kernel' in n for n in names)


# ---------------------------------------------------------------- 7. pixel inference
def test_multiclass_pixel_inference_matches_oracle():
    from oracle import wesup_oracle as orc
    from wesup_amd import synth
    from wesup_amd.models.wesup import WESUPPixelInference
    d = dev()
    C, H, W = 3, 40, 24
    weights = weights_c(4, C, feat_scale=0.3)
    model = WESUPPixelInference(n_classes=C).to(d)
    model.load_state_dict({k: torch.from_numpy(v) for k, v in weights.items()})
    model.eval()
    imgs = torch.from_numpy(np.stack([synth.synth_image(8 + b, H, W) for b in range(2)]))
    refs = [orc.pixel_inference(orc.to_torch(weights), imgs[b:b + 1]) for b in range(2)]

    def check(out, ref):
        assert tuple(out.shape) == (H, W, C)
        assert rel_err(out, ref) < TOL
        assert float((out.sum(dim=-1) - 1).abs().max()) < 1e-6
        flips = (out.argmax(dim=-1).cpu() != ref.argmax(dim=-1))
        assert int(flips.sum()) == 0 or float((out.cpu() - ref)[flips].abs().max()) < 1e-5      # only exact-tie pixels

    check(model(imgs[:1].to(d)), refs[0])
    out = model.forward_batch(imgs.to(d))
    assert tuple(out.shape) == (2, H, W, C)
    for b in range(2):
        check(out[b], refs[b])
    out = model.forward_per_resolution(imgs.to(d))
    assert tuple(out.shape) == (2, H, W, C)
    for b in range(2):
        check(out[b], refs[b])


# ---------------------------------------------------------------- 8. the two-class step is untouched
def _plan_names(trainer):
    from wesup_amd import _lib
    lib = _lib.load()
    plan = next(iter(trainer.step_runner().states.values())).plan
    assert plan is not None
    return lib.wesup_plan_kernels(plan.h), [lib.wesup_plan_node_name(plan.h, i).decode() for i in range(plan.size())]


def test_two_class_step_keeps_its_launch_list(golden_dir):
    """The recorded plan of a two-class step on the 64x48 case of tests/test_step_gpu.py: the kernel count and every node's name as
    the commit before the C-way head recorded them (tests/golden/plan_nodes_c2_64x48.json)."""
    from oracle import wesup_oracle as orc
    d = dev()
    weights = orc.make_weights(11, feat_scale=0.03)
    imgs, segs, pts, pix = batch_c(0, 3, 64, 48, [5, 6, 4], 2)
    trainer = make_trainer(weights)
    data = (torch.from_numpy(imgs).to(d), torch.from_numpy(pix).long().to(d), torch.from_numpy(pts).long().to(d), torch.from_numpy(segs))
    for _ in range(3):                                          # walked, recorded, recorded again and confirmed
        trainer.train_one_iteration('train', *data)
    kernels, names = _plan_names(trainer)
    want = json.load(open(os.path.join(golden_dir, 'plan_nodes_c2_64x48.json')))
    assert kernels == want['kernels']
    assert names == want['names']


def test_two_class_entries_write_the_bits_of_the_commit_before_the_fold(golden_dir):
    """The two-class kernels are instantiations of the C-class bodies (csrc/loss.hip); a comparison of the two-class entries with
    the _c entries at C = 2 therefore compares a kernel with itself.  What pins their bits is the library of the last commit that had
    two-class kernels of its own: tests/golden/head_two_class_bits.json holds a SHA-256 of every output tensor it wrote on the cases
    of tests/_headbits.py (tools/make_head_bits_golden.py, run with WESUP_HIP_LIB on that commit's build; the file names the commit
    and the ROCm version).  Among them the shapes where the fold could newly go wrong: a second trip of the streaming forward
    kernel's capped grid, Wc | bc filling the LDS exactly and one row beyond it, a view that cannot be read as float4.  A compiler
    upgrade that moves expf regenerates the file at a commit where the other head tests pass."""
    import _headbits
    from wesup_amd import _lib
    want = json.load(open(os.path.join(golden_dir, 'head_two_class_bits.json')))['digests']
    got = _headbits.digests(_lib.load())
    assert sorted(got) == sorted(want)
    moved = [(k, name) for k in sorted(want) for name in want[k] if got[k].get(name) != want[k][name]]
    assert not moved, moved
