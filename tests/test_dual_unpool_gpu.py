"""ops.winograd_dual_transform_unpool -- the dual transform of the gradient of a pooled layer that is never written (side-branch
gradient + max-pool backward of the gradient at pooled resolution, formed while loading) -- against the dual transform of that
tensor built from existing entries, and a training step with the engine's unpool_on_load on against the same step with it off.
Tolerance zero throughout: the same arithmetic on the same values."""
import pytest
import torch

pytestmark = pytest.mark.gpu


def dev():
    assert torch.cuda.is_available(), 'GPU tests need a GPU'
    return torch.device('cuda:0')


def rnd(*shape, seed=0, scale=1.0):
    g = torch.Generator().manual_seed(seed)
    return (torch.randn(*shape, generator=g) * scale).float()


class _every_shape_on_the_one_kernel_route:
    """Grids this small take the two-kernel product route by default, and the pooling codes exist on the one-kernel route only."""

    def __enter__(self):
        from wesup_amd import _lib
        self.lib = _lib.load()
        self.was = self.lib.wesup_winograd_set_fused_min_blocks(0)

    def __exit__(self, *exc):
        self.lib.wesup_winograd_set_fused_min_blocks(self.was)


# B = 2 throughout: the batch stride matters
KERNEL_CASES = [
    # form, (Hu, Wu), C
    ('dense', (10, 14), 128),     # partial last tile row and column; windows cut by the 6 x 6 patch halo
    ('dense', (8, 8), 512),       # Q = 128
    ('dense', (12, 20), 256),
    ('gather', (10, 14), 64),     # Kmax = 8, random new_row; T * C / 4 = 384, a block and a half: inactive threads meet the block column sum
]


@pytest.mark.parametrize('form,hw,C', KERNEL_CASES)
def test_dual_transform_unpool_equals_the_dual_transform_of_the_materialised_gradient(form, hw, C):
    from wesup_amd import ops
    d = dev()
    B, (Hu, Wu), Kmax = 2, hw, 8
    # the pooling's codes from the library's own forward, on a pre-pool tensor with windows (whole channels, and one corner of
    # every channel's map) whose maximum is not positive: code 0
    x = rnd(B, Hu, Wu, 64, seed=1).to(d)
    x[:, :4, :4] = 0.0
    w = rnd(C, 64, 3, 3, seed=2, scale=(2.0 / (9 * 64)) ** 0.5)
    bias = rnd(C, seed=3, scale=0.1)
    bias[5::16] = -50.0
    bias[2] = -1e-3           # (corner windows: conv of zeros + a negative bias)
    with _every_shape_on_the_one_kernel_route():
        uf, _ = ops.winograd_pack_weight(w.to(d), m=4)
        code = torch.full((B, Hu // 2, Wu // 2, C // 4), -1, dtype=torch.int16, device=d)
        yp = torch.empty(B, Hu // 2, Wu // 2, C, device=d)
        y = ops.conv3x3_fwd_winograd(x, uf, bias.to(d), relu_in=False, out_pool=yp, m=4, pool_code_out=code)
    torch.cuda.synchronize()
    seen = set()
    for sh in (0, 3, 6, 9):
        seen |= set(((code.int() >> sh) & 7).unique().tolist())
    assert seen == {0, 1, 2, 3, 4}
    dp = rnd(B, Hu // 2, Wu // 2, C, seed=4).to(d)
    if form == 'dense':
        side, new_row = rnd(B, Hu, Wu, C, seed=5).to(d), None
        g_ref = side.clone()
    else:
        side = rnd(B, Kmax, C, seed=5).to(d)
        new_row = torch.randint(0, Kmax, (B, Hu * Wu), generator=torch.Generator().manual_seed(6), dtype=torch.int32).to(d)
        g_ref = torch.stack([side[b][new_row[b].long()] for b in range(B)]).view(B, Hu, Wu, C).contiguous()
    ops.maxpool2_bwd(y, dp, g_ref, accumulate=True)
    T = ops.winograd_tiles(B, Hu, Wu, 4)
    rows = ops.winograd_bias_rows(B, Hu, Wu, C)
    assert rows > 0
    want = [torch.full((36, T, C), float('nan'), device=d), torch.full((36, T, C), float('nan'), device=d),
            torch.full((rows, C), float('nan'), device=d)]
    got = [t.clone() for t in want]
    ops.winograd_dual_transform(g_ref, *want)
    ops.winograd_dual_transform_unpool(side, dp, code, *got, new_row=new_row)
    torch.cuda.synchronize()
    for name, a, b in zip(('V', 'dM', 'bias_part'), got, want):
        assert torch.equal(a, b), name
    # (without the bias rows: the launch is the same, nothing is written there)
    v2, dm2 = torch.empty_like(got[0]), torch.empty_like(got[1])
    ops.winograd_dual_transform_unpool(side, dp, code, v2, dm2, new_row=new_row)
    assert torch.equal(v2, want[0]) and torch.equal(dm2, want[1])


def _step_grads(data, weights, on_load):
    from wesup_amd.models import initialize_trainer
    tr = initialize_trainer('wesup', device='cuda:0')
    tr.model.load_state_dict({k: torch.from_numpy(v) for k, v in weights.items()})
    tr.optimizer, tr.scheduler = tr.get_default_optimizer()
    tr.model.train(); tr.tracker.train()
    tr.model._ensure_engine()
    eng = tr.model.engine
    eng.unpool_on_load = on_load
    tr.train_one_iteration('train', *data)
    torch.cuda.synchronize()
    plan = next(iter(eng._bufs.values())).plans[True][1]
    grads = {k: v.detach().clone() for k, v in tr.model._grad_views.items()}
    eng.release_buffers()
    return grads, plan.dp_on_load


@pytest.mark.parametrize('one_kernel', [False, True])
@pytest.mark.parametrize('B,H,W', [(1, 96, 80), (2, 64, 64)])
def test_step_with_unpool_on_load_equals_the_step_without(B, H, W, one_kernel):
    """One training step, same weights and inputs, unpool_on_load 1 and 0: every parameter gradient equal.  At these sizes the
    default routing leaves no pooling codes, so the walk is the same one either way; one_kernel puts every supported product on
    the one-kernel route, as at the training shapes, and then both forms (dP in G's head under conv2_1, in dV's tail under
    conv3_1) are in the step."""
    import contextlib
    from oracle import wesup_oracle as orc
    from wesup_amd import synth
    d = dev()
    imgs, labs, pts, pix = synth.make_batch(41, B, H, W, 4)
    data = (torch.from_numpy(imgs).to(d), torch.from_numpy(pix).long().to(d), torch.from_numpy(pts).long().to(d),
            torch.from_numpy(labs).to(d))
    weights = orc.make_weights(5, feat_scale=0.03)
    with (_every_shape_on_the_one_kernel_route() if one_kernel else contextlib.nullcontext()):
        g1, at1 = _step_grads(data, weights, 1)
        g0, at0 = _step_grads(data, weights, 0)
    assert all(a is None for a in at0)
    if one_kernel:
        assert {a[0] for a in at1 if a is not None} == {'G', 'dV'}
    else:
        assert all(a is None for a in at1)
    assert g1.keys() == g0.keys() and len(g1) > 30
    for k in g0:
        assert torch.equal(g1[k], g0[k]), k
