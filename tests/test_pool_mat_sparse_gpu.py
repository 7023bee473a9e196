"""The two products of the interpolation-pooling matrix (ops.sp_pool_mat_fwd / sp_pool_mat_bwd) on both of their routes: the
dense batched GEMM below the size rule, the walk over Wm's non-zeros above it.  WESUP_POOL_MAT_SPARSE_MIN forces a route
(1: sparse, 0: GEMM) at sizes the rule would not pick; the entries read it at every call.

1. exact: small-integer matrices, mostly zero, against an int64 host product -- every loop edge of the two kernels (list chunk of
   2048 cells / 512 rows, passes of 256 cells / 64 rows, channel slabs of 1024), a strided slice, batch 3, full / empty / first-cell
   / last-cell rows and a full column.  The GEMM route runs where wesup_gemm_tn_batched accepts the shape (Kmax a multiple of 4
   for the forward, hw for the backward) and must refuse the others as it always did.
2. real label maps against Wm (as the device built it) applied in float64.  Bar: 1e-5 of the tensor's largest value, what
   tests/test_pooling_branches_gpu.py asks of Wm's products (_poolref.CAP_FUSED); and the sparse route may not be worse than the
   GEMM route on the same inputs by more than one fp32 ulp (2^-23) of that scale -- it adds in the GEMM's own order, and where
   both exist the bits are the same (test_sparse_route_writes_the_dense_products_bits).  39 x 58 = 2262
   cells is no multiple of 4: the GEMM backward does not exist there, only its forward is compared.
3. determinism: run to run, and across batch positions.
4. the training step at 2 x 96 x 96 on the sparse route: replay equals walk bit for bit; loss and gradients agree with the GEMM
   route's step within tests/test_step_gpu.py's 1e-4."""
import contextlib
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _poolref as pr          # noqa: E402

pytestmark = pytest.mark.gpu

ENV = 'WESUP_POOL_MAT_SPARSE_MIN'
SENTINEL = -777.25
ULP = 2.0 ** -23
TOL = 1e-4                     # tests/test_step_gpu.py's


def dev():
    assert torch.cuda.is_available(), 'GPU tests need a GPU'
    return torch.device('cuda:0')


@pytest.fixture(scope='module')
def ops():
    from wesup_amd import ops as o
    return o


@contextlib.contextmanager
def route(kind):
    old = os.environ.get(ENV)
    os.environ[ENV] = {'sparse': '1', 'gemm': '0'}[kind]
    try:
        yield
    finally:
        if old is None:
            del os.environ[ENV]
        else:
            os.environ[ENV] = old


def gemm_accepts(direction, Kmax, hw):
    """wesup_gemm_tn_batched wants M and A's row stride to be multiples of 4: Kmax for Wm . s (A = WmT), hw for Wm^T . g (A = Wm)."""
    return (Kmax if direction == 'fwd' else hw) % 4 == 0


def run_fwd(ops, Wm, WmT, s, ld, off):
    B, Kmax, _ = Wm.shape
    sp = torch.full((B, Kmax, ld), SENTINEL, device=Wm.device)
    ops.sp_pool_mat_fwd(Wm, WmT, s, sp, off, ws_tag='test')
    return sp


def run_bwd(ops, Wm, WmT, gsp, off, C):
    B, _, hw = Wm.shape
    ds = torch.full((B, hw, C), SENTINEL, device=Wm.device)
    ops.sp_pool_mat_bwd(Wm, WmT, gsp, off, ds, ws_tag='test')
    return ds


# ---------------------------------------------------------------- 1. exact
# (B, Kmax, hw, C, ld, off)
EXACT = [
    (3, 1, 1, 4, 8, 4),
    (3, 64, 64, 256, 2112, 576),             # GEMM-able: the step's stride, a non-zero offset
    (3, 65, 63, 260, 2112, 1344),
    (3, 130, 65, 768, 2112, 1344),
    (2, 64, 2052, 256, 2112, 64),            # GEMM-able: one list chunk of the forward and four cells
    (3, 65, 2049, 4, 2112, 2108),            # one cell beyond the chunk, the slice at the very end of its row
    (1, 132, 64, 768, 2112, 576),            # GEMM-able: three row passes of the backward
    (3, 516, 64, 260, 264, 4),               # GEMM-able: one list chunk of the backward and four rows
    (2, 1, 65, 1028, 2112, 1084),            # a second channel slab of one quad
    (3, 130, 1, 256, 256, 0),
    (1, 64, 4100, 4, 4, 0),                  # GEMM-able: two full chunks and four cells
    (2, 4, 257, 4, 12, 8),                   # one cell beyond a pass of 256
]


def exact_matrix(B, Kmax, hw, seed):
    rs = np.random.RandomState(seed)
    Wm = rs.randint(-4, 5, size=(B, Kmax, hw)) * (rs.rand(B, Kmax, hw) < 0.04)

    def pattern(b, r, kind):
        Wm[b, r] = 0
        if kind == 0:
            Wm[b, r] = rs.randint(1, 5, size=hw) * rs.choice([-1, 1], size=hw)      # every cell
        elif kind == 2:
            Wm[b, r, 0] = 3                                                          # the first cell only
        elif kind == 3:
            Wm[b, r, hw - 1] = -2                                                    # the last cell only
    if Kmax >= 4:
        for kind in range(4):
            pattern(0, kind, kind)
        Wm[B - 1, :, hw // 2] = rs.randint(1, 5, size=Kmax)                          # a column with every row (image 0 where B = 1:
        if B == 1:                                                                   # its rows 1 - 3 give way to the column)
            assert np.all(Wm[0, :, hw // 2] != 0)
    else:
        for b in range(B):
            pattern(b, 0, b % 4)
    return Wm.astype(np.int64)


@pytest.mark.parametrize('case', EXACT, ids=lambda c: 'B{}-K{}-hw{}-C{}-ld{}-off{}'.format(*c))
def test_integer_products_are_exact_on_both_routes(ops, case):
    from wesup_amd import _lib
    B, Kmax, hw, C, ld, off = case
    d = dev()
    rs = np.random.RandomState(hw + Kmax)
    Wi = exact_matrix(B, Kmax, hw, 7 * hw + Kmax)
    si = rs.randint(-8, 9, size=(B, hw, C)).astype(np.int64)
    gi = rs.randint(-8, 9, size=(B, Kmax, ld)).astype(np.int64)
    Wt, st, gt = torch.from_numpy(Wi), torch.from_numpy(si), torch.from_numpy(gi)
    want_f = torch.bmm(Wt, st)                                        # int64 on the host
    want_b = torch.bmm(Wt.transpose(1, 2), gt[:, :, off:off + C].contiguous())
    assert int(want_f.abs().max()) < 2 ** 24 and int(want_b.abs().max()) < 2 ** 24
    Wm = Wt.float().to(d)
    WmT = Wm.transpose(1, 2).contiguous()
    s, gsp = st.float().to(d), gt.float().to(d)
    for kind in ('sparse', 'gemm'):
        with route(kind):
            assert ops.sp_pool_mat_sparse(Kmax, hw) == (kind == 'sparse')
            sp = ds = None
            if kind == 'sparse' or gemm_accepts('fwd', Kmax, hw):
                sp = run_fwd(ops, Wm, WmT, s, ld, off).cpu()
            else:
                with pytest.raises(_lib.WesupHipError):
                    run_fwd(ops, Wm, WmT, s, ld, off)
            if kind == 'sparse' or gemm_accepts('bwd', Kmax, hw):
                ds = run_bwd(ops, Wm, WmT, gsp, off, C).cpu()
            else:
                with pytest.raises(_lib.WesupHipError):
                    run_bwd(ops, Wm, WmT, gsp, off, C)
        if sp is not None:
            assert torch.equal(sp[:, :, off:off + C].long(), want_f) and torch.equal(sp[:, :, off:off + C], want_f.float()), kind
            keep = torch.ones(ld, dtype=torch.bool)
            keep[off:off + C] = False
            assert torch.equal(sp[:, :, keep], torch.full((B, Kmax, ld - C), SENTINEL)), kind      # nothing outside the slice
        if ds is not None:
            assert torch.equal(ds, want_b.float()), kind


def test_entries_refuse_what_they_cannot_walk(ops):
    from wesup_amd import _lib
    lib, p, st = _lib.load(), ops._p, ops._stream()
    d = dev()
    B, Kmax, hw, C, ld = 1, 4, 8, 8, 16
    Wm, WmT = torch.zeros(B, Kmax, hw, device=d), torch.zeros(B, hw, Kmax, device=d)
    s, sp = torch.zeros(B, hw, C, device=d), torch.zeros(B, Kmax, ld, device=d)
    with route('sparse'):
        ok = lambda *a: lib.wesup_sp_pool_mat_fwd(*a, None, 0, st)
        assert ok(p(Wm), p(WmT), p(s), p(sp), ld, 8, B, Kmax, hw, C) == 0
        assert ok(None, p(WmT), p(s), p(sp), ld, 8, B, Kmax, hw, C) == -1
        assert ok(p(Wm), p(WmT), None, p(sp), ld, 8, B, Kmax, hw, C) == -1
        assert ok(p(Wm), p(WmT), p(s), p(sp), ld, 12, B, Kmax, hw, C) == -1           # 12 + 8 > 16: the slice leaves its row
        assert ok(p(Wm), p(WmT), p(s), p(sp), ld, 8, B, Kmax, 8196, C) == -1          # more than 8192 cells
        assert ok(p(Wm), p(WmT), p(s), p(sp), ld, 6, B, Kmax, hw, C) == -1            # an offset that is no multiple of 4
        assert lib.wesup_sp_pool_mat_bwd(p(Wm), p(WmT), p(sp), ld, 12, p(s), B, Kmax, hw, C, None, 0, st) == -1
        assert lib.wesup_sp_pool_mat_bwd(p(Wm), p(WmT), p(sp), ld, 8, None, B, Kmax, hw, C, None, 0, st) == -1
        assert lib.wesup_sp_pool_mat_bwd(p(Wm), p(WmT), p(sp), ld, 8, p(s), B, Kmax, hw, C, None, 0, st) == 0
    torch.cuda.synchronize()


def test_the_size_rule(ops):
    """The default bound: not below 16 384 entries, and the pinned 3 x 64 x 48 step (Kmax = 64 rows over 32 x 24 cells) stays dense;
    the benchmark's matrices are sparse."""
    old = os.environ.pop(ENV, None)
    try:
        assert not ops.sp_pool_mat_sparse(64, 255) and not ops.sp_pool_mat_sparse(64, 32 * 24)
        assert not ops.sp_pool_mat_sparse(6, 768) and not ops.sp_pool_mat_sparse(64, 16 * 12)
        assert ops.sp_pool_mat_sparse(576, 3600) and ops.sp_pool_mat_sparse(576, 900) and ops.sp_pool_mat_sparse(1536, 2500)
    finally:
        if old is not None:
            os.environ[ENV] = old
    with route('gemm'):
        assert not ops.sp_pool_mat_sparse(576, 3600)
    with route('sparse'):
        assert ops.sp_pool_mat_sparse(1, 1)


# ---------------------------------------------------------------- 2. real label maps against fp64
_REAL = {}


def real_case(ops, H, W):
    """B = 2 Voronoi maps: 36 superpixels plus one of a single pixel, and 25 (fewer than Kmax = 40)."""
    if (H, W) not in _REAL:
        from wesup_amd import synth
        labs = np.stack([synth.voronoi_labels(21, H, W, 6), synth.voronoi_labels(22, H, W, 5)]).astype(np.int32)
        labs[0, H // 3, W // 2] = 36
        masks = np.stack([synth.point_mask(70 + b, labs[b], 0.3, 2) for b in range(2)])
        d = dev()
        meta = ops.sp_preprocess(torch.from_numpy(labs).to(d), torch.from_numpy(masks).to(d), 40)
        assert meta.n_sp.tolist() == [37, 25] and 1 in meta.area_new[0].tolist()
        _REAL[(H, W)] = meta
    return _REAL[(H, W)]


@pytest.mark.parametrize('H,W,h,w', [(96, 80, 24, 20), (96, 80, 12, 10), (156, 232, 39, 58)])
def test_both_routes_against_the_fp64_product(ops, H, W, h, w):
    meta = real_case(ops, H, W)
    B, Kmax, hw, C, ld, off = 2, meta.Kmax, h * w, 768, 2112, 576
    d = dev()
    Wm = ops.sp_interp_matrix(meta, h, w)
    WmT = Wm.transpose(1, 2).contiguous()
    assert float(Wm[1, 25:].abs().max()) == 0.0
    s = pr.relu_like(h + w, (B, hw, C)).to(d)
    gsp = pr.relu_like(h * w, (B, Kmax, ld), zero_mean=True).to(d)
    W64 = Wm.double().cpu()
    ref_f = torch.bmm(W64, s.double().cpu())
    ref_b = torch.bmm(W64.transpose(1, 2), gsp[:, :, off:off + C].double().cpu())
    err = {}
    for kind in ('gemm', 'sparse'):
        with route(kind):
            sp = run_fwd(ops, Wm, WmT, s, ld, off)[:, :, off:off + C].double().cpu()
            err[kind, 'fwd'] = float((sp - ref_f).abs().max() / ref_f.abs().max())
            if kind == 'sparse':
                assert float(sp[1, 25:].abs().max()) == 0.0                 # rows beyond n_sp: exact zeros
            if kind == 'sparse' or gemm_accepts('bwd', Kmax, hw):
                ds = run_bwd(ops, Wm, WmT, gsp, off, C).double().cpu()
                err[kind, 'bwd'] = float((ds - ref_b).abs().max() / ref_b.abs().max())
    print(f'{H}x{W} -> {h}x{w}: ' + ', '.join(f'{k[0]} {k[1]} {v:.3e}' for k, v in sorted(err.items())))
    for k, v in err.items():
        assert v <= pr.CAP_FUSED, (k, v)
    for direction in ('fwd', 'bwd'):
        if ('gemm', direction) in err:
            assert err['sparse', direction] <= err['gemm', direction] + ULP, (direction, err)


def test_sparse_route_writes_the_dense_products_bits(ops):
    """The sparse kernels add in the order of wesup_gemm_tn_batched's own additions (its K ranges, one fused multiply-add per k,
    the ranges' sums in ascending order), so a step computes the same bits on either route: real matrices (several K ranges
    under 480 cells) and a random one whose rows cross the forward's list chunk; batch > 1 (a single product of 128 x 128 tiles
    has weighted ranges, which the sparse route does not follow)."""
    d = dev()
    meta = real_case(ops, 96, 80)
    cases = [(ops.sp_interp_matrix(meta, 24, 20), 768, 2112, 576), (ops.sp_interp_matrix(meta, 12, 10), 260, 2112, 64)]
    g = torch.Generator().manual_seed(3)
    Wr = torch.randn(3, 64, 2052, generator=g) * (torch.rand(3, 64, 2052, generator=g) < 0.03)
    cases.append((Wr.to(d), 256, 2112, 1344))
    for Wm, C, ld, off in cases:
        B, Kmax, hw = Wm.shape
        WmT = Wm.transpose(1, 2).contiguous()
        s = pr.relu_like(hw, (B, hw, C), zero_mean=True).to(d)
        gsp = pr.relu_like(hw + 1, (B, Kmax, ld), zero_mean=True).to(d)
        out = {}
        for kind in ('gemm', 'sparse'):
            with route(kind):
                out[kind] = (run_fwd(ops, Wm, WmT, s, ld, off), run_bwd(ops, Wm, WmT, gsp, off, C))
        assert torch.equal(out['sparse'][0], out['gemm'][0]), (hw, 'fwd', float((out['sparse'][0] - out['gemm'][0]).abs().max()))
        assert torch.equal(out['sparse'][1], out['gemm'][1]), (hw, 'bwd', float((out['sparse'][1] - out['gemm'][1]).abs().max()))


# ---------------------------------------------------------------- 3. determinism
def test_sparse_route_is_reproducible_and_blind_to_the_batch_position(ops):
    meta = real_case(ops, 96, 80)
    d = dev()
    h, w, C, ld, off = 24, 20, 260, 2112, 64
    Wm2 = ops.sp_interp_matrix(meta, h, w)
    Wm = torch.stack([Wm2[0], Wm2[1], Wm2[0]]).contiguous()                  # images 0 and 2 are the same image
    WmT = Wm.transpose(1, 2).contiguous()
    s2 = pr.relu_like(5, (2, h * w, C), zero_mean=True)
    g2 = pr.relu_like(6, (2, meta.Kmax, ld), zero_mean=True)
    s, gsp = torch.stack([s2[0], s2[1], s2[0]]).to(d), torch.stack([g2[0], g2[1], g2[0]]).to(d)
    with route('sparse'):
        sp_a, sp_b = run_fwd(ops, Wm, WmT, s, ld, off), run_fwd(ops, Wm, WmT, s, ld, off)
        ds_a, ds_b = run_bwd(ops, Wm, WmT, gsp, off, C), run_bwd(ops, Wm, WmT, gsp, off, C)
    assert torch.equal(sp_a, sp_b) and torch.equal(ds_a, ds_b)
    assert torch.equal(sp_a[0], sp_a[2]) and torch.equal(ds_a[0], ds_a[2])
    assert not torch.equal(sp_a[0], sp_a[1]) and float(ds_a.abs().max()) > 0


# ---------------------------------------------------------------- 4. the training step
def make_trainer(weights, **kw):
    from wesup_amd.models import initialize_trainer
    from wesup_amd.utils.metrics import accuracy, dice
    t = initialize_trainer('wesup', device='cuda:0', **kw)
    t.model.load_state_dict({k: torch.from_numpy(v) for k, v in weights.items()})
    t.optimizer, t.scheduler = t.get_default_optimizer()
    t.metric_funcs = [accuracy, dice]
    t.model.train()
    t.tracker.train()
    return t


def test_step_on_the_sparse_route_replays_and_agrees_with_the_gemm_route():
    from oracle import wesup_oracle as orc
    from wesup_amd import synth
    d = dev()
    B, H, W, g = 2, 96, 96, 6
    weights = orc.make_weights(7, feat_scale=0.05)
    data = []
    for i in range(2):
        imgs, labs, pts, pix = synth.make_batch(40 + i, B, H, W, g)
        data.append((torch.from_numpy(imgs).to(d), torch.from_numpy(pix).long().to(d), torch.from_numpy(pts).long().to(d),
                     torch.from_numpy(labs).to(d)))
    first = {}
    with route('sparse'):
        a = make_trainer(weights, max_superpixels=g * g, step_plan=False)
        b = make_trainer(weights, max_superpixels=g * g)
        for i in range(6):
            a.train_one_iteration('train', *data[i % 2])
            b.train_one_iteration('train', *data[i % 2])
            assert a.tracker.history['loss'][-1] == b.tracker.history['loss'][-1], i
            assert torch.equal(a.model._flat, b.model._flat), f'parameters differ after step {i}'
            assert torch.equal(a.model._flat_grad, b.model._flat_grad), f'gradients differ after step {i}'
            if i == 0:
                first['sparse'] = (a.tracker.history['loss'][-1], {k: v.clone() for k, v in a.model._grad_views.items()})
        st = b.step_runner().stats
        assert st['replayed'] > 0 and st['dropped'] == 0, st
        from wesup_amd import _lib
        lib = _lib.load()
        plan = next(iter(b.step_runner().states.values())).plan
        names = [lib.wesup_plan_node_name(plan.h, i).decode() for i in range(plan.size())]
        assert any('sp_pool_mat_fwd_kernel' in n for n in names) and any('sp_pool_mat_bwd_kernel' in n for n in names)
    with route('gemm'):
        c = make_trainer(weights, max_superpixels=g * g, step_plan=False)
        c.train_one_iteration('train', *data[0])
        first['gemm'] = (c.tracker.history['loss'][-1], {k: v.clone() for k, v in c.model._grad_views.items()})
    ls, lg = first['sparse'][0], first['gemm'][0]
    worst = 0.0
    for k, ref in first['gemm'][1].items():
        e = float((first['sparse'][1][k] - ref).abs().max() / (ref.abs().max() + 1e-30))
        worst = max(worst, e)
    print(f'loss sparse {ls!r} gemm {lg!r}; worst gradient difference {worst:.3e} of its tensor\'s max')
    assert abs(ls - lg) <= TOL * abs(lg)
    assert worst <= TOL, worst
