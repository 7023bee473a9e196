"""The fused Adam / AdamW step (csrc/optim.hip, wesup_amd/optim.py) on the device: the kernel against the float64 reference of
tests/_adamref.py on every branch it has, and the optimisers on the model -- against torch.optim on a float64 copy, walked against
replayed bit for bit (a new learning rate included, without a plan being dropped), through a checkpoint, and past a NaN loss.

Bars: a figure is the suite's whole-tensor norm max |gpu - ref| / max |ref| (_headref.rel_whole); its bar is
min(4 x the same figure of the plain float32 evaluation on the CPU of exactly these inputs, CAP_ADAM = 1e-6) (_headref.bar_from).
The factor 4 allows another legitimate rounding of the same expression (the GPU contracts a b + c to one rounding, its sqrt and
division are correctly rounded like numpy's).  Outputs of one configuration's small sizes count as one tensor, so that no bar is
zero.  The three factors of a step, read back from the device block, are held to 2^-23 of torch's Python-float values: one
rounding to float32 (2^-24) and the rounding of the complement 1 - beta the tick gets as a float (2^-24 of 1 - beta^t at most).
Everything "bit-equal" is torch.equal.

Measured on an MI355X (HIP | float32 on the CPU, worst over the steps and configurations; the smallest bar any of them had):
  small sizes  p 1.4e-7 | 1.4e-7 (1.3e-7 .. )   m 8.0e-8 | 8.7e-8 (2.1e-7 .. )   v 1.6e-7 | 1.6e-7 (3.3e-7 .. )
  wrap sizes   p 1.2e-7 | 1.2e-7 (3.0e-7 .. )   m 1.0e-7 | 1.1e-7 (3.1e-7 .. )   v 2.0e-7 | 2.0e-7 (5.8e-7 .. )
  the model    p 1.0e-7 | 1.7e-7 (1.6e-7 .. )   m 9.6e-8 | 1.1e-7 (1.8e-7 .. )   v 1.1e-7 | 1.1e-7 (2.7e-7 .. )
  the model, every parameter on its own: p 1.8e-7, m 2.4e-7, v 2.7e-7 (cap 1e-6)
(each figure was below the bar of its own step and configuration; most HIP figures equal the CPU's to all printed digits.)"""
import copy

import numpy as np
import pytest
import torch

import _adamcases as ac
import _adamref as ar
import _headref as hr
from _tol import within

pytestmark = pytest.mark.gpu

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


def figure(case, what, got, ref, cpu):
    """Records the HIP figure beside the fp32-CPU figure of the same inputs (printed before anything is asserted): (ok, text)."""
    f_cpu, f_hip = hr.rel_whole(cpu, ref), hr.rel_whole(got, ref)
    bar = hr.bar_from(f_cpu, ar.CAP_ADAM)
    text = f'{case}: {what} HIP {f_hip:.3e}, fp32 CPU {f_cpu:.3e}, bar {bar:.3e}'
    print(text)
    within(case, f'{what}, fp32 on the CPU vs fp64', f_cpu, ar.CAP_ADAM)
    return within(case, f'{what}, HIP vs fp64', f_hip, bar, 'bar = min(4 x the fp32-CPU figure of the case, cap)'), text


def _factors_ok(ops, state, t_, lr, betas, wd):
    got = ops.adam_state_read(state)
    want = ar.factors(t_, lr, betas, wd)
    assert got['t'] == t_ and got['lr'] == lr
    for k, w in zip(('step_size', 'inv_sqrt_bc2', 'decay'), want):
        assert abs(got[k] - w) <= 2.0 ** -23 * abs(w), (k, t_, got[k], w)


def _run(ops, n, seed, name, decoupled):
    """Three steps on the device from m = v = 0: per step (p, m, v) of the GPU, the fp64 reference, numpy float32; the state block."""
    lr, betas, eps, wd, gs = ac.HYPER[name]
    p0, g3, ref, cpu = ac.case(n, seed, name, decoupled)
    p, m, v = t(p0), torch.zeros(n, device=dev()), torch.zeros(n, device=dev())
    state = ops.adam_state(lr, dev())
    got = []
    for step in range(ac.STEPS):
        ops.adam_tick(state, betas, wd)
        ops.adam_step(p, t(g3[step]), m, v, state, betas, eps, wd, gs, decoupled)
        got.append((p.cpu().numpy(), m.cpu().numpy(), v.cpu().numpy()))
    return got, ref, cpu, state


# ---------------------------------------------------------------- 1. small sizes
@pytest.mark.parametrize('name,decoupled', ac.CONFIGS, ids=ac.IDS)
def test_small_sizes_against_fp64(ops, name, decoupled):
    """n = 1 ... 1025: the float4 body, the scalar tail of block 0, both, and neither half; the outputs of all n as one tensor per
    step.  The count read back is 3 and the factors are torch's."""
    lr, betas, eps, wd, gs = ac.HYPER[name]
    runs = [_run(ops, n, n, name, decoupled) for n in ac.SMALL]
    checks = []
    for step in range(ac.STEPS):
        for k, what in enumerate('pmv'):
            got, ref, cpu = (np.concatenate([r[j][step][k] for r in runs]) for j in range(3))
            assert np.isfinite(got).all(), (name, step, what)
            checks.append(figure(f'adam-small-{name}-{int(decoupled)}-step{step}', f'Adam {what}', got, ref, cpu))
    for r in runs:
        _factors_ok(ops, r[3], 3, lr, betas, wd)
    assert all(ok for ok, _ in checks), [text for ok, text in checks if not ok]


def test_tick_forms_torchs_factors_at_every_count(ops):
    """The block after 1 ... 12 ticks, and from a count a checkpoint set (1000, 100000: 1 - beta^t near 1)."""
    lr, betas, wd = 1e-4, (0.9, 0.999), 1e-2
    state = ops.adam_state(lr, dev())
    for k in range(1, 13):
        ops.adam_tick(state, betas, wd)
        _factors_ok(ops, state, k, lr, betas, wd)
    for t0 in (999, 99999):
        state = ops.adam_state(lr, dev(), t=t0)
        ops.adam_tick(state, betas, wd)
        _factors_ok(ops, state, t0 + 1, lr, betas, wd)


# ---------------------------------------------------------------- 2. the wrap
@pytest.mark.parametrize('n', ac.LARGE, ids=[f'wrap+{k}' for k in range(4)])
def test_where_the_capped_grid_takes_a_second_trip(ops, n):
    """2048 blocks x 256 threads x 4 floats + 1200 + k: 300 threads take a second trip, block 0 a tail of k floats."""
    assert n // 4 == 2048 * 256 + 300 and n % 4 == n - ac.WRAP
    got, ref, cpu, state = _run(ops, n, ac.WRAP_SEED, 'adam', False)
    checks = []
    for step in range(ac.STEPS):
        for k, what in enumerate('pmv'):
            assert np.isfinite(got[step][k]).all(), (step, what)
            checks.append(figure(f'adam-wrap+{n - ac.WRAP}-step{step}', f'Adam {what}', got[step][k], ref[step][k], cpu[step][k]))
    assert ops.adam_state_read(state)['t'] == 3
    assert all(ok for ok, _ in checks), [text for ok, text in checks if not ok]


# ---------------------------------------------------------------- 3. refusals
def test_refuses_misaligned_views_null_pointers_and_no_elements(ops):
    from wesup_amd import _lib
    d = dev()
    n = 1024
    betas, eps = (0.9, 0.999), 1e-8
    base = [torch.randn(n + 4, device=d) for _ in range(4)]          # p, g, m, v
    state = ops.adam_state(5e-2, d)
    ops.adam_tick(state, betas, 0.0)
    keep = [b.clone() for b in base]
    for bad in range(4):                              # each of the four in turn one, two or three floats off a 16-byte boundary
        views = [b[bad % 3 + 1 if k == bad else 0:][:n] for k, b in enumerate(base)]
        assert all(x.is_contiguous() for x in views) and views[bad].data_ptr() % 16 != 0
        with pytest.raises(_lib.WesupHipError):
            ops.adam_step(*views, state, betas, eps, 1e-3, 1.0, False)
    wide = torch.zeros(64, dtype=torch.uint8, device=d)
    wide[4:36].copy_(state)
    with pytest.raises(_lib.WesupHipError):           # the block itself off its boundary
        ops.adam_step(*[b[:n] for b in base], wide[4:36], betas, eps, 1e-3, 1.0, False)
    with pytest.raises(_lib.WesupHipError):
        ops.adam_tick(wide[4:36], betas, 0.0)
    h = _lib.load()
    P = [b.data_ptr() for b in base]
    args = (0.9, 0.1, 0.999, 0.001, 1e-8, 0.0, 1.0, 0, None)
    assert h.wesup_adam_step(P[0], P[1], P[2], P[3], 0, state.data_ptr(), *args) == WESUP_ERR_INVALID
    for k in range(5):
        ptrs = [None if j == k else x for j, x in enumerate(P + [state.data_ptr()])]
        assert h.wesup_adam_step(ptrs[0], ptrs[1], ptrs[2], ptrs[3], n, ptrs[4], *args) == WESUP_ERR_INVALID
    assert h.wesup_adam_tick(None, 0.1, 0.001, 0.0, None) == WESUP_ERR_INVALID
    torch.cuda.synchronize()
    assert all(torch.equal(a, b) for a, b in zip(base, keep)) and ops.adam_state_read(state)['t'] == 1


# ---------------------------------------------------------------- 4. two launches equal one
@pytest.mark.parametrize('decoupled', [False, True], ids=['adam', 'adamw'])
@pytest.mark.parametrize('cuts', [(4096,), (1024, 8192)], ids=['two', 'three'])
def test_ranges_behind_one_tick_equal_one_launch(ops, decoupled, cuts):
    """What step_early / step_late and the per-range launches of a frozen backbone rely on: the buffer in two or three 16-byte
    aligned ranges behind ONE tick is the one launch, bit for bit (the last range ends in a tail of three)."""
    n = 10003
    lr, betas, eps, wd, gs = ac.HYPER['adam']
    p0, g3 = ac.inputs(n, 5)
    runs = []
    for split in (False, True):
        p, m, v = t(p0), torch.zeros(n, device=dev()), torch.zeros(n, device=dev())
        state = ops.adam_state(lr, dev())
        edges = [0, *cuts, n] if split else [0, n]
        for step in range(ac.STEPS):
            g = t(g3[step])
            ops.adam_tick(state, betas, wd)
            for lo, hi in zip(edges[:-1], edges[1:]):
                ops.adam_step(p[lo:hi], g[lo:hi], m[lo:hi], v[lo:hi], state, betas, eps, wd, gs, decoupled)
        runs.append((p, m, v, ops.adam_state_read(state)))
    for a, b, what in zip(runs[0][:3], runs[1][:3], 'pmv'):
        assert torch.equal(a, b), what
    assert runs[0][3] == runs[1][3] and runs[0][3]['t'] == 3
    assert not torch.equal(runs[0][0], t(p0))


# ---------------------------------------------------------------- on the model: the 64 x 48, batch-3 case of tests/test_step_gpu.py
B, H, W = 3, 64, 48
_DATA = {}


def _case():
    """(oracle weights, the batch on the device); made once."""
    if not _DATA:
        from oracle import wesup_oracle as orc
        from wesup_amd import synth
        imgs = np.stack([synth.synth_image(100 + b, H, W) for b in range(B)])
        gs = [5, 6, 4]
        segs = np.stack([synth.voronoi_labels(200 + b, H, W, gs[b]) for b in range(B)])
        pts = np.stack([synth.point_mask(300 + b, segs[b], 0.3, 2, tie_every=4) for b in range(B)])
        pix = np.stack([synth.pixel_mask(400 + b, H, W) for b in range(B)])
        d = dev()
        _DATA['weights'] = orc.make_weights(11, feat_scale=0.03)
        _DATA['batch'] = (torch.from_numpy(imgs).to(d), torch.from_numpy(pix).long().to(d), torch.from_numpy(pts).long().to(d),
                          torch.from_numpy(segs))
    return _DATA['weights'], _DATA['batch']


def _trainer(**kw):
    from wesup_amd.models import initialize_trainer
    from wesup_amd.utils.metrics import accuracy, dice
    weights, _ = _case()
    tr = initialize_trainer('wesup', device='cuda:0', **kw)
    tr.model.load_state_dict({k: torch.from_numpy(v) for k, v in weights.items()})
    tr.optimizer, tr.scheduler = tr.get_default_optimizer()
    tr.metric_funcs = [accuracy, dice]
    tr.model.train()
    tr.tracker.train()
    return tr


def _pmv(tr):
    o = tr.optimizer
    return tr.model._flat.detach().clone(), o._mflat.clone(), o._vflat.clone()


def _same(a, b, where):
    for x, y, what in zip(_pmv(a), _pmv(b), 'pmv'):
        assert torch.equal(x, y), (where, what)
    keys = set(a.tracker.history)
    assert keys == set(b.tracker.history) and {'loss', 'labeled_sp_ratio', 'propagated_labels', 'accuracy', 'dice'} <= keys
    for k in keys:
        assert a.tracker.history[k][-1] == b.tracker.history[k][-1], (where, k)


# ---------------------------------------------------------------- 5. against torch.optim on a float64 copy
@pytest.mark.parametrize('name', ['adam', 'adamw'])
def test_training_iterations_against_torch_optim_in_float64(name):
    """Three iterations without a plan.  After each: torch.optim.Adam / AdamW steps a float64 CPU copy of the flat parameter buffer
    with the gradient read from the GPU's flat buffer, numpy float32 (tests/_adamref.py) steps its own copy with the same
    gradient; p, m and v of the GPU against float64 -- all parameters as one tensor at the bar of the module docstring, and every
    parameter on its own at CAP_ADAM (of a two-element bias the float32 figure is luck, not a bar)."""
    _, batch = _case()
    tr = _trainer(optimizer=name, step_plan=False)
    o, model = tr.optimizer, tr.model
    g = o.param_groups[0]
    lr, betas, eps, wd = g['lr'], tuple(g['betas']), g['eps'], g['weight_decay']
    assert (lr, betas, eps, wd) == (5e-5, (0.9, 0.999), 1e-8, 1e-3) and o.DECOUPLED == (name == 'adamw')
    w64 = torch.nn.Parameter(model._flat.detach().double().cpu())
    ref = (torch.optim.AdamW if name == 'adamw' else torch.optim.Adam)([w64], lr=lr, betas=betas, eps=eps, weight_decay=wd)
    p32 = model._flat.detach().cpu().numpy().copy()
    m32, v32 = np.zeros_like(p32), np.zeros_like(p32)
    spans = [(n_, model._offs[n_], p.numel()) for n_, p in model._named]
    checks = []
    for step in range(3):
        tr.train_one_iteration('train', *batch)
        grad = model._flat_grad.detach().cpu()
        w64.grad = grad.double()
        ref.step()
        p32, m32, v32 = ar.adam(p32, grad.numpy(), m32, v32, step + 1, (lr, betas, eps, wd, 1.0), o.DECOUPLED, np.float32)
        st = ref.state[w64]
        for what, got, want, cpu in (('p', model._flat, w64.detach(), p32), ('m', o._mflat, st['exp_avg'], m32),
                                     ('v', o._vflat, st['exp_avg_sq'], v32)):
            got, want = got.detach().cpu().numpy(), want.numpy()
            checks.append(figure(f'adam-model-{name}-step{step}', f'Adam {what} on the model', got, want, cpu))
            worst = max((hr.rel_whole(got[o_:o_ + k], want[o_:o_ + k]), n_) for n_, o_, k in spans)
            print(f'  step {step} {what}: worst single parameter {worst[0]:.3e} ({worst[1]})')
            checks.append((within(f'adam-model-{name}-step{step}', f'Adam {what}, each parameter', worst[0], ar.CAP_ADAM), str(worst)))
        assert o.step_count() == step + 1
    assert all(ok for ok, _ in checks), [text for ok, text in checks if not ok]
    sd = o.state_dict()
    assert len(sd['state']) == len(spans) and all(float(s['step']) == 3.0 for s in sd['state'].values())


@pytest.mark.parametrize('name', ['adam', 'adamw'])
def test_frozen_backbone_is_untouched_and_has_no_state(name):
    _, batch = _case()
    tr = _trainer(optimizer=name, freeze_backbone=True, step_plan=False)
    model, o = tr.model, tr.optimizer
    before = {n_: p.detach().clone() for n_, p in model._named}
    for _ in range(2):
        tr.train_one_iteration('train', *batch)
    torch.cuda.synchronize()
    frozen = [n_ for n_, p in model._named if not p.requires_grad]
    assert frozen and all(n_.startswith('backbone.') for n_ in frozen)
    for n_, p in model._named:
        if n_ in frozen:
            assert torch.equal(p.detach(), before[n_]) and p not in o.state, n_
            mv, vv = o._views[p]
            assert not mv.any() and not vv.any(), n_
        else:
            assert not torch.equal(p.detach(), before[n_]) and set(o.state[p]) == {'step', 'exp_avg', 'exp_avg_sq'}, n_
    assert o.step_count() == 2 and len(o.state_dict()['state']) == len(model._named) - len(frozen)


# ---------------------------------------------------------------- 6. replay
@pytest.mark.parametrize('name', ['adam', 'adamw'])
def test_replayed_steps_equal_walked_ones_and_a_new_lr_reaches_them(name):
    """Six iterations beside a twin that never replays: loss, metrics, p, m, v bit-equal after each, and some were replayed (the
    tick is a node of the plan: a replay that did not advance the count, or advanced it twice, would show in p at once).  Then
    both halve lr: still bit-equal, NO plan dropped -- lr is not in a plan --, and p differs from a third trainer that kept
    the old lr (a plan with lr baked in would go on with it)."""
    _, batch = _case()
    a = _trainer(optimizer=name, step_plan=False)
    b = _trainer(optimizer=name)
    c = _trainer(optimizer=name, step_plan=False)
    for i in range(6):
        for tr in (a, b, c):
            tr.train_one_iteration('train', *batch)
        _same(a, b, i)
    st = b.step_runner().stats
    assert st['replayed'] > 0 and st['dropped'] == 0 and a.step_runner().stats['replayed'] == 0, st
    assert a.optimizer.step_count() == b.optimizer.step_count() == 6
    dropped, replayed = st['dropped'], st['replayed']
    for tr in (a, b):
        tr.optimizer.param_groups[0]['lr'] *= 0.5
    for i in range(6, 8):
        for tr in (a, b, c):
            tr.train_one_iteration('train', *batch)
        _same(a, b, i)
        assert not torch.equal(b.model._flat, c.model._flat), i
    st = b.step_runner().stats
    assert st['dropped'] == dropped and st['replayed'] == replayed + 2, st
    assert b.optimizer.step_count() == 8
    assert b.optimizer.state_dict()['param_groups'][0]['lr'] == 2.5e-5


# ---------------------------------------------------------------- 7. checkpoint
def test_checkpoint_round_trip_through_torch_optim_adam():
    _, batch = _case()
    a = _trainer(optimizer='adam')
    for _ in range(2):
        a.train_one_iteration('train', *batch)
    sd = a.optimizer.state_dict()
    shapes = [p.shape for _, p in a.model._named]
    # a plain torch.optim.Adam over same-shaped parameters takes it
    plain = torch.optim.Adam([torch.nn.Parameter(torch.zeros(s)) for s in shapes], lr=1e-3)
    plain.load_state_dict(sd)
    assert plain.param_groups[0]['lr'] == 5e-5
    for (_, p), q in zip(a.model._named, plain.param_groups[0]['params']):
        assert float(plain.state[q]['step']) == 2.0
        assert torch.equal(plain.state[q]['exp_avg'], a.optimizer._views[p][0].cpu())
        assert torch.equal(plain.state[q]['exp_avg_sq'], a.optimizer._views[p][1].cpu())
    # a fresh FusedAdam adopts the count and the moments (from torch's own copy of the state) ...
    b = _trainer(optimizer='adam')
    with torch.no_grad():
        b.model._flat.copy_(a.model._flat)
    b.optimizer.load_state_dict(plain.state_dict())
    assert b.optimizer.step_count() == 2
    assert torch.equal(b.optimizer._mflat, a.optimizer._mflat) and torch.equal(b.optimizer._vflat, a.optimizer._vflat)
    for _, p in b.model._named:
        assert b.optimizer.state[p]['exp_avg'].data_ptr() == b.optimizer._views[p][0].data_ptr()
    # ... and its third iteration is the uninterrupted run's
    a.train_one_iteration('train', *batch)
    b.train_one_iteration('train', *batch)
    _same(a, b, 'third iteration')
    assert a.optimizer.step_count() == b.optimizer.step_count() == 3
    # per-parameter counts that differ cannot be represented: refused, nothing changed
    bad = copy.deepcopy(plain.state_dict())
    bad['state'][3]['step'] = torch.tensor(7.0)
    keep = _pmv(b)
    with pytest.raises(ValueError, match='differ'):
        b.optimizer.load_state_dict(bad)
    assert b.optimizer.step_count() == 3 and all(torch.equal(x, y) for x, y in zip(keep, _pmv(b)))


# ---------------------------------------------------------------- 8. NaN
@pytest.mark.parametrize('step_plan', [True, False], ids=['replayed', 'walked'])
def test_nan_loss_leaves_parameters_moments_and_count_untouched(step_plan):
    _, batch = _case()
    tr = _trainer(optimizer='adam', step_plan=step_plan)
    for _ in range(3):
        tr.train_one_iteration('train', *batch)
    if step_plan:
        assert tr.step_runner().stats['replayed'] >= 1
    torch.cuda.synchronize()
    before, block = _pmv(tr), tr.optimizer._state.clone()
    bad = (torch.full_like(batch[0], float('nan')),) + tuple(batch[1:])
    with pytest.raises(ValueError, match='Loss is nan'):
        tr.train_one_iteration('train', *bad)
    torch.cuda.synchronize()
    assert all(torch.equal(x, y) for x, y in zip(before, _pmv(tr)))
    assert torch.equal(block, tr.optimizer._state) and tr.optimizer.step_count() == 3
    tr.train_one_iteration('train', *batch)                   # and the next clean iteration goes through
    assert np.isfinite(tr.tracker.history['loss'][-1]) and tr.optimizer.step_count() == 4
