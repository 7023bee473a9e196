"""The Adam / AdamW reference of tests/_adamref.py against torch.optim, its float32 evaluation against the cap the GPU tests use,
and the wiring of the fused optimisers that needs no launch: the C ABI entries, ``WESUPTrainer.get_default_optimizer``,
``plan_fields()`` and the refusal of a checkpoint one count cannot represent (a stub model with flat buffers on the CPU).

Measured on the CPU (rel_whole = max |a - ref| / max |ref|):
  float64 reference vs torch.optim.Adam / AdamW on float64 tensors, three steps, all configurations: <= 2.3e-16  (bar 1e-14)
  float32 evaluation vs the float64 reference, p / m / v: <= 2.4e-7 at n >= 1023 and at the four wrap sizes (_adamcases.WRAP_SEED
  says why their seed matters); at n <= 7, where one or two elements are the tensor, <= 3.1e-7 except m of the 'adam' set at
  n = 2, 6.7e-7                                                                                                   (CAP_ADAM 1e-6)"""
import os
import re

import numpy as np
import pytest
import torch

import _adamcases as ac
import _adamref as ar
import _headref as hr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ---------------------------------------------------------------- 1. the reference is torch's Adam / AdamW
@pytest.mark.parametrize('name,decoupled', ac.CONFIGS, ids=ac.IDS)
def test_float64_reference_is_torch_optim(name, decoupled):
    lr, betas, eps, wd, gs = ac.HYPER[name]
    p0, g3, ref, _ = ac.case(1025, 1, name, decoupled)
    w = torch.nn.Parameter(torch.from_numpy(p0).double())
    cls = torch.optim.AdamW if decoupled else torch.optim.Adam
    opt = cls([w], lr=lr, betas=betas, eps=eps, weight_decay=wd)
    worst = 0.0
    for step in range(ac.STEPS):
        w.grad = torch.from_numpy(g3[step]).double() * gs
        opt.step()
        st = opt.state[w]
        assert float(st['step']) == step + 1
        for got, want in zip((w.detach(), st['exp_avg'], st['exp_avg_sq']), ref[step]):
            worst = max(worst, hr.rel_whole(got.numpy(), want))
    print(f'{name} decoupled={decoupled}: float64 reference vs torch {worst:.2e}')
    assert worst <= 1e-14


# ---------------------------------------------------------------- 2. the float32 evaluation stays under the cap
@pytest.mark.parametrize('name,decoupled', ac.CONFIGS, ids=ac.IDS)
def test_float32_evaluation_stays_under_the_cap(name, decoupled):
    worst = {}
    # every case tests/test_optim_gpu.py runs: the small sizes under every configuration, the wrap sizes under the first
    cases = [(n, n) for n in ac.SMALL] + [(n, ac.WRAP_SEED) for n in (ac.LARGE if (name, decoupled) == ('adam', False) else ac.LARGE[3:])]
    for n, seed in cases:
        _, _, ref, cpu = ac.case(n, seed, name, decoupled)
        for step in range(ac.STEPS):
            for k, what in enumerate('pmv'):
                assert cpu[step][k].dtype == np.float32
                f = hr.rel_whole(cpu[step][k], ref[step][k])
                worst[what] = max(worst.get(what, 0.0), f)
                assert f < ar.CAP_ADAM, (n, seed, step, what, f)
    print(f'{name} decoupled={decoupled}: float32 vs float64 ' + ', '.join(f'{k} {v:.2e}' for k, v in worst.items()))


def test_complements_are_rounded_from_doubles():
    """What the kernel gets as 1 - beta2 must be float32(1 - 0.999): float32(1) - float32(0.999) is off in the fifth digit, and v with it."""
    good, bad = np.float32(1.0 - 0.999), np.float32(1.0) - np.float32(0.999)
    assert abs(float(good) - 1e-3) / 1e-3 < 6e-8 and abs(float(bad) - 1e-3) / 1e-3 > 1e-5


def test_factors_are_torchs():
    """step_size, the inverse root of the second bias correction and AdamW's decay as torch.optim forms them from Python floats."""
    for t in (1, 2, 3, 10, 1000, 100000):
        ss, ib, dc = ar.factors(t, 1e-4, (0.9, 0.999), 1e-2)
        assert ss == 1e-4 / (1 - 0.9 ** t) and ib == 1.0 / (1 - 0.999 ** t) ** 0.5 and dc == 1 - 1e-4 * 1e-2


# ---------------------------------------------------------------- 3. wiring
def _header_decls():
    hdr = open(os.path.join(ROOT, 'include', 'wesup_hip.h')).read()
    hdr = re.sub(r'/\*.*?\*/', '', hdr, flags=re.S)
    return dict(re.findall(r'\n\s*int\s+(wesup_adam_\w+)\s*\(([^;]*?)\)\s*;', hdr, flags=re.S))


def test_entries_are_declared_bound_and_exported():
    from wesup_amd import _lib
    decls = _header_decls()
    assert sorted(decls) == ['wesup_adam_step', 'wesup_adam_tick']
    assert _lib._SIGS['wesup_adam_tick'][1] == 'pfffp' and _lib._SIGS['wesup_adam_step'][1] == 'ppppzp' + 'f' * 7 + 'ip'
    assert _lib.ABI_VERSION == 6
    if not os.path.exists(_lib.LIB_PATH):
        _lib.build()
    h = _lib.load()
    assert h.wesup_abi_version() == 6
    # refused on the host, before any launch: null pointers, n = 0, a state block that is not 16-byte aligned
    assert h.wesup_adam_tick(None, 0.1, 0.001, 0.0, None) == -1 and h.wesup_adam_tick(8, 0.1, 0.001, 0.0, None) == -1
    assert h.wesup_adam_step(None, None, None, None, 4, None, 0.9, 0.1, 0.999, 0.001, 1e-8, 0.0, 1.0, 0, None) == -1
    assert h.wesup_adam_step(16, 16, 16, 16, 0, 16, 0.9, 0.1, 0.999, 0.001, 1e-8, 0.0, 1.0, 0, None) == -1
    assert h.wesup_adam_step(16, 16, 16, 20, 4, 16, 0.9, 0.1, 0.999, 0.001, 1e-8, 0.0, 1.0, 0, None) == -1


class _Stub(torch.nn.Module):
    """A model with what the fused optimisers read of WESUP: flat parameter / gradient buffers (64-float slots), offsets, the
    (name, parameter) list and gradient views -- on the CPU, no engine."""

    def __init__(self):
        super().__init__()
        self.backbone = torch.nn.Linear(3, 5)
        self.head = torch.nn.Linear(5, 2)
        self._flat = None

    def _ensure_engine(self):
        if self._flat is not None:
            return
        params = dict(self.named_parameters())
        self._offs, total = {}, 0
        for name, p in params.items():
            self._offs[name] = total
            total += (p.numel() + 63) // 64 * 64
        self._flat, self._flat_grad = torch.zeros(total), torch.zeros(total)
        self._grad_views = {}
        for name, p in params.items():
            o, n = self._offs[name], p.numel()
            self._flat[o:o + n].copy_(p.detach().reshape(-1))
            p.data = self._flat[o:o + n].view(p.shape)
            self._grad_views[name] = self._flat_grad[o:o + n].view(p.shape)
        self._named = list(params.items())


def _trainer(**kwargs):
    from wesup_amd.models.wesup import WESUPConfig, WESUPTrainer
    t = object.__new__(WESUPTrainer)                  # (the constructor moves the model to a GPU; none of that is needed here)
    t.model, t.kwargs = _Stub(), {**WESUPConfig().to_dict(), **kwargs}
    return t


def test_default_optimizer_is_unchanged():
    from wesup_amd.optim import FusedSGD
    opt, sched = _trainer().get_default_optimizer()
    g = opt.param_groups[0]
    assert type(opt) is FusedSGD and sched is None
    assert g['lr'] == 5e-5 and g['momentum'] == 0.9 and g['weight_decay'] == 1e-3 and opt.grad_scale == 1.0


@pytest.mark.parametrize('name', ['adam', 'adamw'])
def test_adam_kwargs_reach_the_optimizer(name):
    from wesup_amd import optim
    opt, sched = _trainer(optimizer=name, lr=1e-4, betas=(0.8, 0.99), adam_eps=1e-6, lr_scheduler='plateau').get_default_optimizer()
    assert type(opt) is (optim.FusedAdam if name == 'adam' else optim.FusedAdamW)
    assert isinstance(opt, torch.optim.AdamW if name == 'adamw' else torch.optim.Adam)
    g = opt.param_groups[0]
    assert (g['lr'], tuple(g['betas']), g['eps'], g['weight_decay']) == (1e-4, (0.8, 0.99), 1e-6, 1e-3)
    assert opt.DECOUPLED == (name == 'adamw')
    # the scheduler the reference constructs (models/wesup.py:452-455): min mode, patience 10, factor 0.5, min_lr 1e-5
    assert isinstance(sched, torch.optim.lr_scheduler.ReduceLROnPlateau) and sched.optimizer is opt
    assert (sched.mode, sched.patience, sched.factor, list(sched.min_lrs)) == ('min', 10, 0.5, [1e-5])
    d, _ = _trainer(optimizer=name).get_default_optimizer()
    g = d.param_groups[0]
    assert (g['lr'], tuple(g['betas']), g['eps']) == (5e-5, (0.9, 0.999), 1e-8)


def test_plateau_scheduler_on_the_default_optimizer():
    from wesup_amd.optim import FusedSGD
    opt, sched = _trainer(lr_scheduler='plateau', lr=1e-3).get_default_optimizer()
    assert type(opt) is FusedSGD and opt.param_groups[0]['lr'] == 1e-3
    assert isinstance(sched, torch.optim.lr_scheduler.ReduceLROnPlateau)
    for _ in range(12):                               # eleven epochs without improvement: the scheduler halves the optimiser's lr
        sched.step(1.0)
    assert opt.param_groups[0]['lr'] == 5e-4


def test_unknown_names_raise_with_the_choices():
    with pytest.raises(ValueError, match='sgd.*adam.*adamw'):
        _trainer(optimizer='rmsprop').get_default_optimizer()
    with pytest.raises(ValueError, match='plateau'):
        _trainer(lr_scheduler='cosine').get_default_optimizer()


def test_config_mirror_has_no_new_attributes():
    from wesup_amd.models.wesup import WESUPConfig
    assert not {'optimizer', 'lr', 'betas', 'adam_eps', 'lr_scheduler'} & set(WESUPConfig().to_dict())


# ---------------------------------------------------------------- 4. what a recorded plan depends on
def test_plan_fields_hold_lr_for_sgd_only():
    from wesup_amd import optim
    m = _Stub()
    sgd = optim.FusedSGD(m, lr=5e-5, momentum=0.9, weight_decay=1e-3)
    f0 = sgd.plan_fields()
    assert f0 == (5e-5, 0.9, 1e-3, 1.0, True, sgd._vflat.data_ptr())
    sgd.param_groups[0]['lr'] = 2.5e-5
    assert sgd.plan_fields() != f0 and 2.5e-5 in sgd.plan_fields()
    for cls in (optim.FusedAdam, optim.FusedAdamW):
        o = cls(m, lr=1e-4, weight_decay=1e-3, grad_scale=0.5)
        f0 = o.plan_fields()
        assert f0 == ((0.9, 0.999), 1e-8, 1e-3, 0.5, cls is optim.FusedAdamW, o._mflat.data_ptr(), o._vflat.data_ptr(), o._state.data_ptr())
        o.param_groups[0]['lr'] = 5e-5
        assert o.plan_fields() == f0                  # lr lives in the device block
        o.grad_scale = 0.25
        assert o.plan_fields() != f0
        for a in ('step_early', 'step_late', 'plan_fields', 'push_hyper'):
            assert callable(getattr(o, a))
    assert not hasattr(sgd, 'push_hyper')


def test_state_block_layout_and_checkpoint_refusal():
    """The host's view of the 32-byte block (double lr at 0, int32 count at 8), and load_state_dict(): the count and the moments of a
    torch.optim.Adam state are adopted; per-parameter 'step' values that differ are refused before anything changes."""
    import struct
    from wesup_amd import optim
    m = _Stub()
    o = optim.FusedAdam(m, lr=1e-4)
    assert o._state.numel() == 32 and o._state.data_ptr() % 16 == 0
    raw = bytes(o._state.numpy().tobytes())
    assert struct.unpack('<d', raw[:8])[0] == 1e-4 and o.step_count() == 0 and not any(raw[8:])
    assert o.state_dict()['state'] == {}              # never stepped: no state, as in torch
    o.param_groups[0]['lr'] = 5e-5
    o.push_hyper()
    assert struct.unpack('<d', bytes(o._state.numpy().tobytes())[:8])[0] == 5e-5
    # a plain torch.optim.Adam over same-shaped parameters, stepped twice
    twin = [torch.nn.Parameter(p.detach().clone()) for p in m.parameters()]
    ref = torch.optim.Adam(twin, lr=1e-4)
    for _ in range(2):
        for p in twin:
            p.grad = torch.ones_like(p)
        ref.step()
    sd = ref.state_dict()
    o.load_state_dict(sd)
    assert o.step_count() == 2 and o.param_groups[0]['lr'] == 1e-4
    assert struct.unpack('<d', bytes(o._state.numpy().tobytes())[:8])[0] == 1e-4
    for p, q in zip(m.parameters(), twin):
        mv, vv = o._views[p]
        assert o.state[p]['exp_avg'].data_ptr() == mv.data_ptr() and o.state[p]['exp_avg_sq'].data_ptr() == vv.data_ptr()
        assert torch.equal(mv, ref.state[q]['exp_avg']) and torch.equal(vv, ref.state[q]['exp_avg_sq'])
    back = o.state_dict()
    assert all(float(s['step']) == 2.0 for s in back['state'].values()) and len(back['state']) == 4
    keep_m, keep_v = o._mflat.clone(), o._vflat.clone()
    sd['state'][1]['step'] = torch.tensor(3.0)
    with pytest.raises(ValueError, match='differ'):
        o.load_state_dict(sd)
    assert o.step_count() == 2 and torch.equal(o._mflat, keep_m) and torch.equal(o._vflat, keep_v)
