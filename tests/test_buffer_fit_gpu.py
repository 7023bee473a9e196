"""A shape's buffer set is complete before the first launch of its first walk: WesupEngine._fit creates what layer_plan.buffers
lists for the plan, and nothing in forward / backward allocates afterwards."""
import math

import pytest
import torch

pytestmark = pytest.mark.gpu


def set_bytes(b):
    """Device bytes a buffer set holds right now (every tensor reachable from it, storages counted once)."""
    from wesup_amd.engine import _Bufs
    seen, total, todo = set(), 0, [b]
    while todo:
        o = todo.pop()
        if torch.is_tensor(o):
            st = o.untyped_storage()
            if st.data_ptr() not in seen:
                seen.add(st.data_ptr())
                total += st.nbytes()
        elif isinstance(o, (list, tuple)):
            todo.extend(o)
        elif isinstance(o, _Bufs):
            todo.extend(vars(o).values())
    return total


def storages(b):
    from wesup_amd.engine import _Bufs
    out, todo = set(), [b]
    while todo:
        o = todo.pop()
        if torch.is_tensor(o):
            out.add(o.untyped_storage().data_ptr())
        elif isinstance(o, (list, tuple)):
            todo.extend(o)
        elif isinstance(o, _Bufs):
            todo.extend(vars(o).values())
    return out


@pytest.mark.parametrize('plain, shape', [(False, (2, 64, 64, 36)), (True, (2, 64, 64, 36)), (False, (1, 75, 53, 36))],
                         ids=['default', 'plain', 'odd_75x53'])
def test_a_set_is_complete_when_its_first_forward_returns_and_no_walk_allocates(plain, shape):
    from wesup_amd import layer_plan as lp, ops
    from wesup_amd.models import initialize_trainer
    dev = torch.device('cuda:0')
    B, H, W, Kmax = shape
    model = initialize_trainer('wesup', device='cuda:0').model
    model._ensure_engine()
    eng = model.engine
    eng.plain = plain
    g = math.isqrt(Kmax)
    lab = ((torch.arange(H, device=dev) * g // H).view(H, 1) * g + (torch.arange(W, device=dev) * g // W).view(1, W))
    meta = ops.sp_preprocess(lab.to(torch.int32).expand(B, H, W).contiguous(), None, Kmax)
    gen = torch.Generator(device=dev).manual_seed(3)
    img = torch.rand(B, 3, H, W, device=dev, generator=gen)
    dpred = torch.randn(B, Kmax, 2, device=dev, generator=gen) * 0.01
    allocated = lambda: torch.cuda.memory_stats()['allocation.all.allocated']

    def step():
        eng.forward(img, meta, train=True)
        eng.backward(None, dpred)
        torch.cuda.synchronize()

    def check(want):
        """want: table bytes.  The first training forward after a (re)fit leaves the set at exactly that, and it stays."""
        eng.forward(img, meta, train=True)
        b = eng._last
        print(f'set bytes after the first forward {set_bytes(b)}, table {want}')
        assert set_bytes(b) == want
        eng.backward(None, dpred)
        torch.cuda.synchronize()
        assert set_bytes(b) == want
        held, n0 = storages(b), allocated()
        step()
        print(f'allocations across the second step: {allocated() - n0}')
        assert allocated() == n0
        assert set_bytes(b) == want and storages(b) == held
        return b, held

    table = lambda b: {(e.name, e.layer): e for e in eng._table(b, eng._plan(b, True))}
    b0 = eng._get_bufs(B, H, W, Kmax, True)          # (the bare record: no tensor yet)
    assert set_bytes(b0) == 0
    first = table(b0)
    b, held = check(lp.nbytes(first.values()))
    assert b is b0
    # a switch flipped on the live engine: the next step tops the set up to the union of the two tables and frees nothing
    eng.plain = not plain
    second = table(b)
    assert second != first and all(first[k].shape == e.shape for k, e in second.items() if k in first)
    union = {**first, **second}
    assert lp.nbytes(union.values()) > lp.nbytes(first.values())
    b2, held2 = check(lp.nbytes(union.values()))
    assert b2 is b and held <= held2
    eng.release_buffers()
