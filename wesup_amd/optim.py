"""Fused optimisers over the model's flat parameter buffer.

``FusedSGD`` replaces torch.optim.SGD.step (models/wesup.py:445-451; semantics of SURVEY.md Appendix A: g += wd*p;
buf = mu*buf + g (first step buf = g); p -= lr*buf).  It IS a torch.optim.SGD (same param_groups and state_dict layout, momentum
buffers under 'momentum_buffer'), only ``step`` is replaced by one launch of the ``wesup_sgd_step`` kernel; ``grad_scale`` folds
the 1/world_size of data-parallel gradient averaging into the same pass.

``FusedAdam`` / ``FusedAdamW`` relate to torch.optim.Adam / AdamW (no amsgrad) in the same way: same param_groups, state under
'exp_avg', 'exp_avg_sq' and 'step', the moments views of two flat buffers, ``step`` one launch of ``wesup_adam_step`` per
contiguous trainable range.  What moves from step to step -- the count behind the bias corrections, and the learning rate a
scheduler changes -- lives in a 32-byte device block that a launch of its own advances (``wesup_adam_tick``, once per step, in
front of the step's first update launch): the step runner records and replays both like every other launch of the iteration,
and a new learning rate reaches the recorded plans through one small copy (``push_hyper``) instead of dropping them.

All three share ``_FlatStep``: which ranges of the flat buffers a step covers (frozen parameters, parameters without a
gradient, a gradient set by hand), the step in one part or in two (``step_early`` / ``step_late``, runner.py), and
``plan_fields()``, what a recorded plan of the step depends on."""
import struct

import torch

from . import ops


class _FlatStep:
    """The range logic of a step over the flat buffers.  A subclass is a torch optimiser as well and provides ``_sync_state_in``
    (adopt what load_state_dict() left in self.state), ``_launch(ranges)``, ``_finish()`` and ``plan_fields()``; ``_begin()`` is
    called once per step in front of its first ``_launch``."""

    def _trainable_ranges(self, with_grad):
        """Contiguous [lo, hi) element ranges of the flat buffers that hold parameters that are stepped (padding
        included, adjacent parameters merged): one range = the whole buffer when nothing is frozen, the tail behind the
        backbone with freeze_backbone (models/wesup.py:427-429,447).  with_grad: one flag per parameter -- like
        torch.optim.SGD, a parameter whose ``grad`` is None (no backward since zero_grad(): a raised or partial backward,
        step() called twice) is skipped, not updated with whatever the flat gradient buffer still holds."""
        m = self.model
        ranges = []
        for (name, p), has in zip(m._named, with_grad):
            if not has:
                continue
            lo, hi = m._offs[name], m._offs[name] + (p.numel() + 63) // 64 * 64
            if ranges and ranges[-1][1] == lo:
                ranges[-1][1] = hi
            else:
                ranges.append([lo, hi])
        return ranges

    def _prepare(self):
        m = self.model
        self._sync_state_in()
        m._ensure_engine()
        for name, p in m._named:                      # a gradient that is not the flat view (set by hand): adopt it
            if p.requires_grad and p.grad is not None and p.grad.data_ptr() != m._grad_views[name].data_ptr():
                m._grad_views[name].copy_(p.grad)
        sig = tuple(p.requires_grad and p.grad is not None for _, p in m._named)
        if getattr(self, '_ranges_sig', None) != sig:
            self._ranges, self._ranges_sig = self._trainable_ranges(sig), sig

    def _begin(self):
        pass

    @torch.no_grad()
    def step(self, closure=None):
        self._prepare()
        self._begin()
        self._launch(self._ranges)
        self._finish()
        return None

    # The step in two launches (the step runner, one rank): every parameter but those named in ``late`` as soon as their gradients
    # are complete -- beside the end of the backward pass, on the stream the caller has made current -- and the rest behind it.
    # The update is elementwise: the two parts together are step(), bit for bit.
    @torch.no_grad()
    def step_early(self, late):
        m = self.model
        self._prepare()
        cut = sorted((m._offs[n], m._offs[n] + (dict(m._named)[n].numel() + 63) // 64 * 64) for n in late)
        early, held = [], []
        for lo, hi in self._ranges:
            pos = lo
            for a, b in cut:
                a, b = max(a, lo), min(b, hi)
                if a >= b:
                    continue
                if a > pos:
                    early.append([pos, a])
                if held and held[-1][1] == a:             # (weight and bias of a layer are neighbours: one launch)
                    held[-1][1] = b
                else:
                    held.append([a, b])
                pos = b
            if pos < hi:
                early.append([pos, hi])
        self._late = held
        self._begin()
        self._launch(early)

    @torch.no_grad()
    def step_late(self):
        self._launch(self._late)
        self._late = None
        self._finish()


class FusedSGD(_FlatStep, torch.optim.SGD):
    def __init__(self, model, lr=5e-5, momentum=0.9, weight_decay=0.0, grad_scale=1.0):
        model._ensure_engine()
        self.model = model
        params = [p for p in model.parameters() if p.requires_grad]
        torch.optim.SGD.__init__(self, params, lr=lr, momentum=momentum or 0.0, weight_decay=weight_decay or 0.0)
        self.grad_scale = grad_scale
        self._vflat = torch.zeros_like(model._flat)
        self._first = True
        self._views = {}
        for name, p in model.named_parameters():
            o, n = model._offs[name], p.numel()
            self._views[p] = self._vflat[o:o + n].view(p.shape)

    def _sync_state_in(self):
        """Adopt momentum buffers that load_state_dict() put into self.state."""
        for p, view in self._views.items():
            st = self.state.get(p)
            if st and st.get('momentum_buffer') is not None and st['momentum_buffer'].data_ptr() != view.data_ptr():
                view.copy_(st['momentum_buffer'])
                st['momentum_buffer'] = view
                self._first = False

    def _launch(self, ranges):
        m = self.model
        g = self.param_groups[0]
        lr, mu, wd = g['lr'], g['momentum'], g['weight_decay']
        for lo, hi in ranges:                         # one launch per contiguous trainable range
            ops.sgd_step(m._flat[lo:hi], m._flat_grad[lo:hi], self._vflat[lo:hi], lr, mu, wd, self.grad_scale, self._first)

    def _finish(self):
        if self.param_groups[0]['momentum'] != 0:
            for p, view in self._views.items():
                if p.requires_grad and p.grad is not None:
                    self.state[p]['momentum_buffer'] = view
        self._first = False

    def plan_fields(self):
        """What a recorded plan of this step holds as launch arguments: every scalar of the kernel, lr among them (its signature
        is pinned by the recorded node list: a new lr drops the plans), and the momentum buffer's address."""
        g = self.param_groups[0]
        return (g['lr'], g['momentum'], g['weight_decay'], self.grad_scale, self._first, self._vflat.data_ptr())


class _FusedAdamBase(_FlatStep):
    DECOUPLED = False
    # the device block (AdamState, csrc/optim.hip): byte offsets of what the host writes or reads
    _LR, _T = (0, 'd'), (8, 'i')

    def _init_flat(self, model, grad_scale):
        self.model = model
        self.grad_scale = grad_scale
        g = self.param_groups[0]
        if len(self.param_groups) != 1 or g.get('amsgrad') or g.get('maximize') or torch.is_tensor(g['lr']):
            raise ValueError('the fused Adam family has one parameter group, a float lr, no amsgrad and no maximize')
        self._mflat = torch.zeros_like(model._flat)
        self._vflat = torch.zeros_like(model._flat)
        self._views = {}
        for name, p in model.named_parameters():
            o, n = model._offs[name], p.numel()
            self._views[p] = (self._mflat[o:o + n].view(p.shape), self._vflat[o:o + n].view(p.shape))
        dev = model._flat.device
        self._lr_pushed = float(g['lr'])
        self._state = ops.adam_state(self._lr_pushed, dev)        # (allocations are 512-byte aligned: the block needs 16)
        # host mirror of the block (pinned where the block is on a GPU: the copies below are queued, not waited for)
        self._host = self._state.to('cpu', copy=True)
        if dev.type == 'cuda':
            self._host = self._host.pin_memory()
        self._copied = None

    # ------------------------------------------------------------------ the device block
    def _push(self, field, value):
        """Queue the copy of one field of the block on the current stream."""
        off, fmt = field
        n = struct.calcsize(fmt)
        if self._copied is not None:                  # the mirror is the source of a queued copy until that copy has run
            self._copied.synchronize()
        self._host[off:off + n] = torch.frombuffer(bytearray(struct.pack('<' + fmt, value)), dtype=torch.uint8)
        self._state[off:off + n].copy_(self._host[off:off + n], non_blocking=True)
        if self._state.is_cuda:
            self._copied = torch.cuda.Event()
            self._copied.record()

    def push_hyper(self):
        """A learning rate that changed since the last push (a scheduler, a caller writing param_groups[0]['lr']) goes to the
        device block -- one 8-byte copy on the caller's stream; the next tick forms the step's factors from it.  The block
        holds the double itself.  Called by step() and, before it walks, replays or audits, by the step runner."""
        lr = float(self.param_groups[0]['lr'])
        if lr != self._lr_pushed:
            self._push(self._LR, lr)
            self._lr_pushed = lr

    def step_count(self):
        """Optimiser steps so far, read back from the device (waits for the device)."""
        return ops.adam_state_read(self._state)['t']

    # ------------------------------------------------------------------ the step
    def _hyper(self):
        g = self.param_groups[0]
        return tuple(float(b) for b in g['betas']), float(g['eps']), float(g['weight_decay'])

    def _begin(self):
        """The step's one tick, in front of its first update launch (none when nothing is stepped, as torch counts)."""
        if self._ranges:
            self.push_hyper()
            betas, _, wd = self._hyper()
            ops.adam_tick(self._state, betas, wd)

    def _launch(self, ranges):
        m = self.model
        betas, eps, wd = self._hyper()
        for lo, hi in ranges:                         # one launch per contiguous trainable range
            ops.adam_step(m._flat[lo:hi], m._flat_grad[lo:hi], self._mflat[lo:hi], self._vflat[lo:hi], self._state, betas, eps, wd,
                          self.grad_scale, self.DECOUPLED)

    def _finish(self):
        for p, (mv, vv) in self._views.items():
            if p.requires_grad and p.grad is not None:
                st = self.state[p]
                if 'exp_avg' not in st:               # ('step' is the one count of the device block: state_dict() fills it in)
                    st['step'], st['exp_avg'], st['exp_avg_sq'] = torch.tensor(0.0), mv, vv

    def plan_fields(self):
        """What a recorded plan of this step holds as launch arguments.  NOT lr and not the count: they are in the device block
        the launches read, whose address is here with the moment buffers'."""
        betas, eps, wd = self._hyper()
        return (betas, eps, wd, self.grad_scale, self.DECOUPLED, self._mflat.data_ptr(), self._vflat.data_ptr(), self._state.data_ptr())

    # ------------------------------------------------------------------ checkpoints
    def _sync_state_in(self):
        pass                                          # (load_state_dict() adopts at once)

    def state_dict(self):
        """torch.optim.Adam's layout.  Reads the count back from the device: every stepped parameter's 'step' is that count."""
        t = float(self.step_count())
        for st in self.state.values():
            if 'exp_avg' in st:
                st['step'] = torch.tensor(t)
        return super().state_dict()

    def load_state_dict(self, state_dict):
        """Adopts the moments into the flat buffers and pushes the count.  One count serves every stepped parameter: a state
        whose per-parameter 'step' values differ cannot be represented and is refused before anything is changed."""
        steps = sorted({float(st['step']) for st in state_dict['state'].values() if 'step' in st})
        if len(steps) > 1:
            raise ValueError(f"the fused Adam family keeps ONE step count for all parameters; this state holds per-parameter 'step' "
                             f'values that differ: {steps[:8]}')
        if steps and steps[0] != int(steps[0]):
            raise ValueError(f"'step' is not a whole number: {steps[0]}")
        super().load_state_dict(state_dict)
        with torch.no_grad():
            for p, (mv, vv) in self._views.items():
                st = self.state.get(p)
                if not st or 'exp_avg' not in st:     # never stepped: no state, zero moments
                    self.state.pop(p, None)
                    mv.zero_()
                    vv.zero_()
                    continue
                for key, view in (('exp_avg', mv), ('exp_avg_sq', vv)):
                    if st[key].data_ptr() != view.data_ptr():
                        view.copy_(st[key])
                        st[key] = view
        self._push(self._T, int(steps[0]) if steps else 0)
        self._lr_pushed = None                        # (the loaded group's lr goes to the block before the next tick)
        self.push_hyper()


class FusedAdam(_FusedAdamBase, torch.optim.Adam):
    def __init__(self, model, lr=5e-5, betas=(0.9, 0.999), eps=1e-8, weight_decay=0.0, grad_scale=1.0):
        model._ensure_engine()
        params = [p for p in model.parameters() if p.requires_grad]
        torch.optim.Adam.__init__(self, params, lr=lr, betas=tuple(betas), eps=eps, weight_decay=weight_decay or 0.0)
        self._init_flat(model, grad_scale)


class FusedAdamW(_FusedAdamBase, torch.optim.AdamW):
    DECOUPLED = True

    def __init__(self, model, lr=5e-5, betas=(0.9, 0.999), eps=1e-8, weight_decay=0.0, grad_scale=1.0):
        model._ensure_engine()
        params = [p for p in model.parameters() if p.requires_grad]
        torch.optim.AdamW.__init__(self, params, lr=lr, betas=tuple(betas), eps=eps, weight_decay=weight_decay or 0.0)
        self._init_flat(model, grad_scale)
