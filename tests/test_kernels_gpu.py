"""Per-kernel parity on a real MI355X, through the C ABI (wesup_amd.ops -> libwesup_hip.so).

Integer / index outputs must be bit-exact; fp32 outputs within 1e-4 relative
(BASELINE.json north_star).  References: the CPU oracle (oracle/wesup_oracle.py)
where it restates the op, plain torch fp32 CPU ops for generic conv/GEMM kernels.
"""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

TOL = 1e-4


def dev():
    assert torch.cuda.is_available(), 'GPU tests need a GPU'
    return torch.device('cuda:0')


def rel_err(a, b):
    a = a.detach().double().cpu()
    b = b.detach().double().cpu()
    return float((a - b).abs().max() / (b.abs().max() + 1e-30))


def nhwc(t):
    return t.permute(0, 2, 3, 1).contiguous()


def nchw(t):
    return t.permute(0, 3, 1, 2).contiguous()


@pytest.fixture(scope='module')
def ops():
    from wesup_amd import ops as o
    return o


@pytest.fixture(scope='module')
def lib():
    from wesup_amd import _lib as l
    return l


def rnd(*shape, seed=0, scale=1.0):
    g = torch.Generator().manual_seed(seed)
    return (torch.randn(*shape, generator=g) * scale).float()


# ---------------------------------------------------------------- conv 3x3
CONV_CASES = [
    # B, H, W, Cin, Cout
    (2, 12, 10, 64, 64),
    (1, 6, 6, 128, 256),
    (3, 5, 7, 256, 128),
    (1, 2, 2, 512, 512),
    (2, 16, 12, 3, 64),
    (1, 224, 224, 64, 64),      # 128x64 tiles
    (1, 224, 224, 64, 128),     # 128x128 tiles
    (1, 230, 218, 3, 64),       # image layer, 128x64 tiles, ragged M
]


@pytest.mark.parametrize('B,H,W,Cin,Cout', CONV_CASES)
@pytest.mark.parametrize('relu_in', [False, True])
def test_conv3x3_fwd(ops, B, H, W, Cin, Cout, relu_in):
    d = dev()
    x = rnd(B, Cin, H, W, seed=1)
    w = rnd(Cout, Cin, 3, 3, seed=2, scale=(2.0 / (9 * Cin)) ** 0.5)
    b = rnd(Cout, seed=3, scale=0.1)
    ref = F.conv2d(F.relu(x) if relu_in else x, w, b, padding=1)
    if Cin == 3:
        xg = ops.pack_input(x.to(d))
    else:
        xg = nhwc(x).to(d)
    wf, _ = ops.pack_conv3x3_weight(w.to(d), need_dgrad=False)
    y = ops.conv3x3_fwd(xg, wf, b.to(d), Cout, relu_in)
    assert rel_err(nchw(y), ref) < TOL
    # the optional second output is exactly max(y, 0) -- also on the tiles that go through the stream-K fix-up
    y2, yr = torch.empty_like(y), torch.empty_like(y)
    ops.conv3x3_fwd(xg, wf, b.to(d), Cout, relu_in, out=y2, out_relu=yr)
    assert torch.equal(y2, y) and torch.equal(yr, torch.relu(y))


@pytest.mark.parametrize('B,H,W,Cin,Cout', [(1, 40, 36, 3, 64), (2, 33, 29, 64, 64), (1, 37, 41, 64, 128),
                                            (2, 24, 24, 128, 128), (1, 11, 7, 32, 64)])
@pytest.mark.parametrize('relu_in', [False, True])
@pytest.mark.parametrize('into_slice', [False, True])
def test_conv3x3_fwd_with_fused_side_conv(ops, B, H, W, Cin, Cout, relu_in, into_slice):
    """The side conv computed in the conv's epilogue (models/wesup.py:256-266) equals Conv2d(Cout, Cout/2, 1) on the
    conv output; the conv output and its ReLU'd copy are bit-identical to the unfused launch's; ragged last pixel tile,
    and the side output written into a channel slice of a wider buffer (row stride > Cout/2) leaves the rest alone."""
    d = dev()
    x = rnd(B, Cin, H, W, seed=1)
    w = rnd(Cout, Cin, 3, 3, seed=2, scale=(2.0 / (9 * Cin)) ** 0.5)
    b = rnd(Cout, seed=3, scale=0.1)
    sw = rnd(Cout // 2, Cout, seed=4, scale=(1.0 / Cout) ** 0.5)
    sb = rnd(Cout // 2, seed=5, scale=0.1)
    y_ref = F.conv2d(F.relu(x) if relu_in else x, w, b, padding=1)
    s_ref = F.conv2d(y_ref.double(), sw.double().view(Cout // 2, Cout, 1, 1), sb.double()).float()
    xg = ops.pack_input(x.to(d)) if Cin == 3 else nhwc(x).to(d)
    wf, _ = ops.pack_conv3x3_weight(w.to(d), need_dgrad=False)
    y0 = ops.conv3x3_fwd(xg, wf, b.to(d), Cout, relu_in)
    P = B * H * W
    if into_slice:
        wide = torch.full((P, Cout // 2 + 24), 7.0, device=d)
        sout = wide[:, 8:8 + Cout // 2]
    else:
        wide = None
        sout = torch.empty(P, Cout // 2, device=d)
    y, yr = torch.empty_like(y0), torch.empty_like(y0)
    ops.conv3x3_fwd(xg, wf, b.to(d), Cout, relu_in, out=y, out_relu=yr, side=(sw.to(d), sb.to(d), sout))
    assert rel_err(nchw(y), y_ref) < TOL
    assert torch.equal(yr, torch.relu(y))
    assert (y - y0).abs().max().item() <= 2e-6 * y0.abs().max().item()      # bias added before / after the LDS image
    s = sout.view(B, H, W, Cout // 2)
    assert rel_err(nchw(s), s_ref) < TOL
    if wide is not None:
        assert (wide[:, :8] == 7.0).all() and (wide[:, 8 + Cout // 2:] == 7.0).all()
    # no bias on either conv
    sout2 = torch.empty(P, Cout // 2, device=d)
    ops.conv3x3_fwd(xg, wf, None, Cout, relu_in, out=y, side=(sw.to(d), None, sout2))
    y_nb = F.conv2d(F.relu(x) if relu_in else x, w, None, padding=1)
    s_nb = F.conv2d(y_nb.double(), sw.double().view(Cout // 2, Cout, 1, 1)).float()
    assert rel_err(nchw(sout2.view(B, H, W, Cout // 2)), s_nb) < TOL


def test_relu_on_load_nan_semantics(ops):
    """ReLU-on-load in the GEMM loops (relu_in / relu_b; off the step's default path, csrc/common.hpp vmax1) is a signed
    integer max of the float's bits: a NaN with the sign bit clear survives like in torch.relu, a NaN with the sign bit
    set is swallowed (read as +0).  The epilogue ReLU (relu1: the step's default, relu_on_store) keeps both."""
    d = dev()
    B, H, W, C = 1, 8, 8, 64
    x = rnd(B, C, H, W, seed=1)
    w = rnd(C, C, 3, 3, seed=2, scale=0.05)
    wf, _ = ops.pack_conv3x3_weight(w.to(d), need_dgrad=False)
    pos_nan = torch.tensor([0x7fc00000], dtype=torch.int32).view(torch.float32)
    neg_nan = torch.tensor([-0x400000], dtype=torch.int32).view(torch.float32)          # 0xffc00000
    for nan, survives in ((pos_nan, True), (neg_nan, False)):
        xn = nhwc(x).clone()
        xn[0, 3, 4, 5] = nan
        y = ops.conv3x3_fwd(xn.to(d), wf, None, C, True)
        hit = torch.isnan(y[0, 2:5, 3:6]).any(dim=-1)                # the 3x3 neighbourhood of the poisoned pixel
        assert bool(hit.all()) == survives and bool(hit.any()) == survives
        x0 = nhwc(x).clone()
        x0[0, 3, 4, 5] = 0.0
        if not survives:                                            # ... and then it reads exactly as a zero
            assert torch.equal(y, ops.conv3x3_fwd(x0.to(d), wf, None, C, True))
        # the producer-side ReLU (second output of the conv kernel) keeps a NaN of either sign
        y1, yr = torch.empty_like(y), torch.empty_like(y)
        wn = wf.clone()
        ops.conv3x3_fwd(xn.to(d), wn, None, C, False, out=y1, out_relu=yr)
        assert torch.isnan(y1).any() and torch.equal(torch.isnan(yr), torch.isnan(y1))


def test_fused_side_conv_rejects_other_widths(ops, lib):
    d = dev()
    x = torch.zeros(1, 8, 8, 128, device=d)
    wf = torch.zeros(256, 9 * 128, device=d)
    y = torch.empty(1, 8, 8, 256, device=d)
    with pytest.raises(lib.WesupHipError):
        ops.conv3x3_fwd(x, wf, None, 256, False, out=y, side=(torch.zeros(128, 256, device=d), None, torch.empty(64, 128, device=d)))


@pytest.mark.parametrize('B,H,W,Cin,Cout', [(1, 12, 10, 32, 32), (2, 37, 41, 64, 128), (1, 30, 30, 256, 256),
                                            (2, 60, 60, 128, 256), (3, 15, 15, 512, 512), (1, 7, 9, 256, 512), (1, 1, 1, 32, 64)])
@pytest.mark.parametrize('relu_in', [False, True])
@pytest.mark.parametrize('m', [2, 4])
def test_conv3x3_wgrad_winograd(ops, B, H, W, Cin, Cout, relu_in, m):
    """The Winograd-domain weight gradient equals autograd's (fp64) to fp32 noise -- odd heights / widths (tiles that
    hang over the border), one-pixel images, K not a multiple of the GEMM step -- and sits next to the direct kernel.
    F(2x2,3x3): within 4x the direct kernel's own error; F(4x4,3x3): <= 2e-5 of the tensor's maximum (its transforms
    multiply by up to 8 and 1/24; the path's tolerance is 1e-4)."""
    d = dev()
    x = rnd(B, Cin, H, W, seed=1)
    dy = rnd(B, Cout, H, W, seed=4)
    w = torch.zeros(Cout, Cin, 3, 3, dtype=torch.float64, requires_grad=True)
    xin = (F.relu(x) if relu_in else x).double()
    F.conv2d(xin, w, torch.zeros(Cout, dtype=torch.float64), padding=1).backward(dy.double())
    ref = w.grad
    xg, dyg = nhwc(x).to(d), nhwc(dy).to(d)
    dw, db = ops.conv3x3_wgrad_winograd(xg, dyg, relu_in, m=m)
    dw0, db0 = ops.conv3x3_wgrad(xg, dyg, Cin, relu_in)
    e_w, e_0 = rel_err(dw, ref), rel_err(dw0, ref)
    assert e_w < wino_bar(m, e_0), (e_w, e_0)
    assert rel_err(db, dy.double().sum(dim=(0, 2, 3))) < TOL / 10
    dw2, db2 = ops.conv3x3_wgrad_winograd(xg, dyg, relu_in, m=m)            # deterministic (fixed split-K order)
    assert torch.equal(dw, dw2) and torch.equal(db, db2)


def _lib_mod():
    from wesup_amd import _lib
    return _lib


def _composite(ops, entry, B, H, W, k_in, k_out, m, *args):
    """A C composite of the Winograd-domain conv (input transform, products, output transform issued from C: the form a C
    caller uses) called directly: args are the entry's arguments up to its workspace, tensors as themselves.  The ops
    wrappers issue the same passes one by one from Python and must leave the same bits."""
    lib = _lib_mod()
    nb = lib.load().wesup_conv3x3_winograd_workspace_bytes(B, H, W, k_in, k_out, m)
    assert nb > 0
    ws = ops.workspace(nb, dev(), 'composite')
    lib.call(entry, *[ops._p(a) if a is None or isinstance(a, torch.Tensor) else a for a in args], ops._p(ws), nb, ops._stream())


class _Tags:
    """A timer like engine.KernelTimer that records the class tags in the order the passes are bracketed."""
    def __init__(self):
        self.tags = []

    def begin(self, tag):
        self.tags.append(tag)
        return tag

    def end(self, tok, work):
        assert tok == self.tags[-1] and work > 0      # the brackets do not nest; every pass states its work


def _wino_tags(ops, k_in, k_out, tiles, v_pre=False):
    """The timer classes of a dgrad-like pass per route: one kernel for products + output transform, or three passes."""
    one_kernel = ops.winograd_fused_supported(k_in, k_out, 4, tiles) == 2
    tags = ['winograd_transform', 'winograd_gemm'] + ([] if one_kernel else ['winograd_transform'])
    return tags[1:] if v_pre else tags


def wino_bar(m, e_direct):
    """Error bar of a Winograd-domain conv pass against fp64, as a fraction of the tensor's maximum."""
    return max(TOL / 10, 4 * e_direct) if m == 2 else 2e-5


WINO_CASES = [(1, 12, 10, 32, 32), (2, 37, 41, 64, 128), (1, 30, 30, 256, 256), (2, 60, 60, 256, 512), (3, 15, 15, 512, 512),
              (1, 7, 9, 512, 256), (1, 1, 1, 32, 64), (4, 30, 30, 512, 512)]


@pytest.mark.parametrize('B,H,W,Cin,Cout', WINO_CASES)
@pytest.mark.parametrize('relu_in', [False, True])
@pytest.mark.parametrize('m', [2, 4])
def test_conv3x3_fwd_winograd(ops, B, H, W, Cin, Cout, relu_in, m):
    """Forward through the Winograd domain = Conv2d(k=3, pad=1) to fp32 noise (odd sizes, one-pixel image, one full
    round of tiles), second ReLU'd output exact, the kept transformed input serves the Winograd weight gradient."""
    d = dev()
    x = rnd(B, Cin, H, W, seed=1)
    w = rnd(Cout, Cin, 3, 3, seed=2, scale=(2.0 / (9 * Cin)) ** 0.5)
    b = rnd(Cout, seed=3, scale=0.1)
    ref = F.conv2d((F.relu(x) if relu_in else x).double(), w.double(), b.double(), padding=1)
    xg = nhwc(x).to(d)
    uf, ud = ops.winograd_pack_weight(w.to(d), m=m)
    P = (m + 2) ** 2
    assert ud.shape == (P, Cin, Cout)
    T = ops.winograd_tiles(B, H, W, m)
    assert T == B * -(-H // m) * -(-W // m)
    v_keep = torch.empty(P, T, Cin, device=d)
    y = torch.empty(B, H, W, Cout, device=d)
    yr = torch.empty_like(y)
    ops.conv3x3_fwd_winograd(xg, uf, b.to(d), relu_in, out=y, out_relu=yr, v_keep=v_keep, m=m)
    wf, _ = ops.pack_conv3x3_weight(w.to(d), need_dgrad=False)
    y0 = ops.conv3x3_fwd(xg, wf, b.to(d), Cout, relu_in)
    e_w, e_0 = rel_err(nchw(y), ref), rel_err(nchw(y0), ref)
    assert e_w < wino_bar(m, e_0), (e_w, e_0)
    assert torch.equal(yr, torch.relu(y))
    # the C composite (the same passes issued from C) leaves the same bits in every output
    yc, yrc, vc = torch.empty_like(y), torch.empty_like(y), torch.empty_like(v_keep)
    _composite(ops, 'wesup_conv3x3_fwd_winograd', B, H, W, Cin, Cout, m, xg, uf, b.to(d), yc, yrc, None, 0, vc, B, H, W, Cin, Cout,
               int(relu_in), m)
    assert torch.equal(yc, y) and torch.equal(yrc, yr) and torch.equal(vc, v_keep)
    if H >= 2 and W >= 2:      # the pooled third output = the max-pool kernel on y, bit for bit (odd borders: floor mode)
        for pool_relu in (False, True):
            yp = torch.full((B, H // 2, W // 2, Cout), 7.0, device=d)
            y3 = torch.empty_like(y)
            ops.conv3x3_fwd_winograd(xg, uf, b.to(d), relu_in, out=y3, out_pool=yp, pool_relu=pool_relu, m=m)
            ypc, y3c = torch.full_like(yp, 7.0), torch.empty_like(y)
            _composite(ops, 'wesup_conv3x3_fwd_winograd', B, H, W, Cin, Cout, m, xg, uf, b.to(d), y3c, None, ypc, int(pool_relu), None,
                       B, H, W, Cin, Cout, int(relu_in), m)
            assert torch.equal(y3c, y3) and torch.equal(ypc, yp)
            if _lib_mod().load().wesup_winograd_fused_supported(Cin, Cout, m):
                # without a second (ReLU'd) output, short products take the one-kernel route: the same sums in another order
                assert float((y3 - y).abs().max()) < 4e-6 * float(y.abs().max()) * 25
                assert torch.equal(yp, ops.maxpool2_fwd(y3, torch.empty_like(yp), relu=pool_relu))
            else:
                assert torch.equal(y3, y)
                assert torch.equal(yp, ops.maxpool2_fwd(y, torch.empty_like(yp), relu=pool_relu))
    y2 = ops.conv3x3_fwd_winograd(xg, uf, None, relu_in, m=m)                  # no bias, workspace V
    assert rel_err(nchw(y2), ref - b.double().view(1, -1, 1, 1)) < wino_bar(m, e_0)
    dy = rnd(B, Cout, H, W, seed=4)
    dyg = nhwc(dy).to(d)
    dw1, db1 = ops.conv3x3_wgrad_winograd(xg, dyg, relu_in, v_pre=v_keep, m=m)
    dw2, db2 = ops.conv3x3_wgrad_winograd(xg, dyg, relu_in, m=m)
    assert torch.equal(dw1, dw2) and torch.equal(db1, db2)


@pytest.mark.parametrize('B,H,W,Ci,Co', [(2, 7, 9, 32, 64), (1, 12, 12, 64, 32), (3, 5, 4, 128, 128), (1, 16, 24, 32, 32)])
@pytest.mark.parametrize('m', [2, 4])
def test_winograd_building_blocks_match_the_numpy_oracle(ops, B, H, W, Ci, Co, m):
    """Every stage entry on its own against oracle/winograd_oracle.py (itself checked against torch's Conv2d and autograd
    in tests/test_winograd_oracle_cpu.py): the two activation transforms, the filter transforms, the batched product,
    the output transform with each epilogue option, and the way back from split-K slabs to (dw, db)."""
    from oracle import winograd_oracle as wo
    d = dev()
    f32 = np.float32
    x = nhwc(rnd(B, Ci, H, W, seed=1))
    dy = nhwc(rnd(B, Co, H, W, seed=2))
    w = rnd(Co, Ci, 3, 3, seed=3, scale=0.1)
    bias = rnd(Co, seed=4)
    xg, dyg = x.to(d), dy.to(d)
    T, P = wo.tiles(B, H, W, m), (m + 2) ** 2
    # transforms (m = 2: adds and halves only; m = 4: small integer / 1/6-multiple factors): fp32 results equal the fp64
    # oracle to rounding of differently ordered sums
    def close(got, want, rel=3e-6):
        return np.abs(got.cpu().numpy() - want).max() < (1e-5 if m == 2 else rel * np.abs(want).max())
    for relu in (False, True):
        V = ops.winograd_input_transform(xg, relu=relu, m=m)
        assert V.shape == (P, T, Ci)
        assert close(V, wo.input_transform(x.numpy(), relu, m=m))
    dM = ops.winograd_outgrad_transform(dyg, m=m)
    assert close(dM, wo.outgrad_transform(dy.numpy(), m=m))
    if m == 4:       # the bias gradient rides in the outgrad transform (F(2x2): in the filter-gradient reduce, below)
        dbo = torch.empty(Co, device=d)
        dM2 = ops.winograd_outgrad_transform(dyg, m=m, db=dbo)
        assert torch.equal(dM2, dM)
        want = dy.double().sum(dim=(0, 1, 2))
        assert float((dbo.cpu().double() - want).abs().max()) < 1e-5 * float(want.abs().max() + 1)
    uf, ud = ops.winograd_pack_weight(w.to(d), m=m)
    uf_o, ud_o = wo.pack_weight(w.numpy(), m=m)
    assert np.abs(uf.cpu().numpy() - uf_o).max() < 1e-6 and np.abs(ud.cpu().numpy() - ud_o).max() < 1e-6
    # batched product
    V = ops.winograd_input_transform(xg, m=m)
    M = ops.gemm_nt_batched(V, uf)
    M_o = wo.products_nt(V.cpu().numpy().astype(np.float64), uf.cpu().numpy().astype(np.float64))
    assert np.abs(M.cpu().numpy() - M_o).max() < 1e-4 * np.abs(M_o).max()
    # output transform: plain + bias + second (ReLU'd) output + pooled output; then mask + accumulate
    y_o = wo.output_transform(M.cpu().numpy(), B, H, W, bias.numpy(), m=m)
    yr = torch.empty(B, H, W, Co, device=d)
    yp = torch.empty(B, H // 2, W // 2, Co, device=d)
    y = ops.winograd_output_transform(M, B, H, W, bias=bias.to(d), out_relu=yr, out_pool=yp, pool_relu=True, m=m)
    # (m = 4: the outputs are small differences of transformed values up to ~100x larger)
    out_tol = 1e-5 * max(1.0, np.abs(y_o).max()) if m == 2 else 3e-6 * np.abs(M.cpu().numpy()).max()
    assert np.abs(y.cpu().numpy() - y_o).max() < out_tol
    assert torch.equal(yr, torch.relu(y))
    assert torch.equal(yp, torch.relu(F.max_pool2d(y.permute(0, 3, 1, 2), 2).permute(0, 2, 3, 1)))
    base = rnd(B, H, W, Co, seed=6).to(d)
    mask = rnd(B, H, W, Co, seed=7).to(d)
    acc = base.clone()
    ops.winograd_output_transform(M, B, H, W, mask_src=mask, out=acc, accumulate=True, m=m)
    y_nb = wo.output_transform(M.cpu().numpy(), B, H, W, m=m)
    expect = base.cpu().numpy() + np.where(mask.cpu().numpy() > 0, y_nb, 0.0)
    assert np.abs(acc.cpu().numpy() - expect).max() < (1e-5 * max(1.0, np.abs(expect).max()) if m == 2 else out_tol)
    # filter gradient from split-K slabs: two splits whose sum is dU, column sums behind each slab
    dU = np.einsum('pto,pti->poi', wo.outgrad_transform(dy.numpy(), m=m), wo.input_transform(x.numpy(), m=m))
    half = np.random.default_rng(0).standard_normal(dU.shape)
    cs = wo.outgrad_transform(dy.numpy(), m=m).sum(axis=1)                     # (P, Co)
    slabs = np.zeros((P, 2, Co * Ci + Co), dtype=f32)
    slabs[:, 0, :Co * Ci] = (dU - half).reshape(P, -1); slabs[:, 1, :Co * Ci] = half.reshape(P, -1)
    slabs[:, 0, Co * Ci:] = cs * 0.25; slabs[:, 1, Co * Ci:] = cs * 0.75
    dw = torch.empty(Co, Ci, 3, 3, device=d); db = torch.empty(Co, device=d) if m == 2 else None
    ops.winograd_filter_grad(torch.from_numpy(slabs).to(d), dw, db, m=m)
    dw_o, db_o = wo.conv_wgrad(x.numpy(), dy.numpy(), m=m)
    assert np.abs(dw.cpu().numpy() - dw_o).max() < 1e-4 * np.abs(dw_o).max()
    if m == 2:
        assert np.abs(db.cpu().numpy() - db_o).max() < 1e-4 * np.abs(db_o).max()


@pytest.mark.parametrize('B,H,W,Cin,Cout', WINO_CASES)
@pytest.mark.parametrize('m', [2, 4])
def test_conv3x3_dgrad_winograd(ops, B, H, W, Cin, Cout, m):
    d = dev()
    x = rnd(B, Cin, H, W, seed=1).requires_grad_(True)
    w = rnd(Cout, Cin, 3, 3, seed=2, scale=(2.0 / (9 * Cin)) ** 0.5)
    dy = rnd(B, Cout, H, W, seed=4)
    F.conv2d(F.relu(x).double(), w.double(), None, padding=1).backward(dy.double())
    ref = x.grad.double()                                  # includes the ReLU mask (x > 0)
    _, ud = ops.winograd_pack_weight(w.to(d), need_fwd=False, m=m)
    _, wd = ops.pack_conv3x3_weight(w.to(d))
    base = rnd(B, H, W, Cin, seed=5)
    out = base.clone().to(d)
    mask = nhwc(x.detach()).to(d)
    ops.conv3x3_dgrad_winograd(nhwc(dy).to(d), ud, mask_src=mask, out=out, accumulate=True, m=m)
    outc = base.clone().to(d)                              # the C composite: the same bits
    _composite(ops, 'wesup_conv3x3_dgrad_winograd', B, H, W, Cout, Cin, m, nhwc(dy).to(d), ud, mask, outc, B, H, W, Cin, Cout, 1, m)
    assert torch.equal(outc, out)
    out0 = base.clone().to(d)
    ops.conv3x3_dgrad(nhwc(dy).to(d), wd, Cin, mask_src=mask, out=out0, accumulate=True)
    e_w, e_0 = rel_err(nchw(out.cpu() - base), ref), rel_err(nchw(out0.cpu() - base), ref)
    assert e_w < wino_bar(m, e_0), (e_w, e_0)
    # plain (no mask, no accumulate)
    x2 = rnd(B, Cin, H, W, seed=1).requires_grad_(True)
    F.conv2d(x2.double(), w.double(), None, padding=1).backward(dy.double())
    out2 = ops.conv3x3_dgrad_winograd(nhwc(dy).to(d), ud, m=m)
    assert rel_err(nchw(out2), x2.grad) < wino_bar(m, TOL / 40)
    out2c = torch.empty_like(out2)
    _composite(ops, 'wesup_conv3x3_dgrad_winograd', B, H, W, Cout, Cin, m, nhwc(dy).to(d), ud, None, out2c, B, H, W, Cin, Cout, 0, m)
    assert torch.equal(out2c, out2)


@pytest.mark.parametrize('B,H,W,K,N', [(2, 24, 16, 64, 64), (1, 37, 41, 64, 128), (3, 9, 8, 128, 64), (1, 2, 2, 64, 64),
                                       (1, 120, 120, 128, 128), (2, 30, 30, 128, 256), (1, 60, 60, 256, 128), (2, 15, 15, 256, 256)])
def test_winograd_products_and_output_transform_in_one_kernel(ops, B, H, W, K, N):
    """wesup_winograd_gemm_output_transform (short products: the batched GEMM and the output transform in one kernel, the
    transformed output never written) against the two separate entries on the same transformed input, for every epilogue
    the conv passes use: bias + pooled output (forward), mask + accumulate (input gradient), the max-pool backward; ragged
    tile grids, fewer than 32 tiles, several blocks along both grid axes.  Also against the fp64 oracle."""
    from oracle import winograd_oracle as wo
    d = dev()
    x = nhwc(rnd(B, K, H, W, seed=1))
    w = rnd(N, K, 3, 3, seed=2, scale=(2.0 / (9 * K)) ** 0.5)
    bias = rnd(N, seed=3, scale=0.1)
    xg = x.to(d)
    uf, _ = ops.winograd_pack_weight(w.to(d), need_dgrad=False, m=4)
    V = ops.winograd_input_transform(xg, m=4)
    Mt = ops.gemm_nt_batched(V, uf)
    scale = float(Mt.abs().max())
    # forward epilogue: bias (+ pooled output)
    yp2 = torch.full((B, H // 2, W // 2, N), 7.0, device=d) if H >= 2 and W >= 2 else None
    yp1 = None if yp2 is None else torch.full_like(yp2, 7.0)
    y2 = ops.winograd_output_transform(Mt, B, H, W, bias=bias.to(d), out_pool=yp2, pool_relu=True, m=4)
    y1 = ops.winograd_gemm_output_transform(V, uf, B, H, W, bias=bias.to(d), out_pool=yp1, pool_relu=True)
    tol = 4e-6 * scale                       # the same sums in another order, outputs ~100x below the transformed values
    assert float((y1 - y2).abs().max()) < tol
    if yp1 is not None:
        assert float((yp1 - yp2).abs().max()) < tol and torch.equal(yp1, torch.relu(F.max_pool2d(y1.permute(0, 3, 1, 2), 2).permute(0, 2, 3, 1)))
    ref = wo.conv_fwd(x.numpy(), w.numpy(), bias.numpy(), m=4)
    assert np.abs(y1.cpu().numpy() - ref).max() < 2e-5 * np.abs(ref).max()
    # input-gradient epilogue: ReLU mask of the layer below + accumulation
    base, mask = rnd(B, H, W, N, seed=6).to(d), rnd(B, H, W, N, seed=7).to(d)
    a1, a2 = base.clone(), base.clone()
    ops.winograd_gemm_output_transform(V, uf, B, H, W, mask_src=mask, out=a1, accumulate=True)
    ops.winograd_output_transform(Mt, B, H, W, mask_src=mask, out=a2, accumulate=True, m=4)
    assert float((a1 - a2).abs().max()) < tol and torch.equal(a1[mask <= 0], base[mask <= 0])
    # max-pool backward epilogue (ties and dead windows included)
    Hu, Wu = 2 * H + 1, 2 * W
    ypre = rnd(B, Hu, Wu, N, seed=8)
    ypre[0, 0:2, 0:2, :8] = 0.37
    ypre[0, 0:2, 2:4, :8] = -1.0
    ypre = ypre.to(d)
    g0 = rnd(B, Hu, Wu, N, seed=9).to(d)
    u1, u2 = g0.clone(), g0.clone()
    ops.winograd_gemm_output_transform(V, uf, B, H, W, unpool=(ypre, u1))
    dxp = ops.winograd_output_transform(Mt, B, H, W, m=4)
    ops.maxpool2_bwd(ypre, dxp, u2, accumulate=True)
    assert float((u1 - u2).abs().max()) < tol
    assert torch.equal((u1 != g0), (u2 != g0)) or float(((u1 != g0) != (u2 != g0)).float().mean()) < 1e-4      # same positions touched


@pytest.mark.parametrize('B,Hu,Wu,Cin,Cout', [(2, 24, 16, 64, 128), (1, 37, 41, 128, 64), (3, 9, 8, 256, 256), (1, 2, 2, 32, 32),
                                              (1, 120, 120, 128, 256)])
def test_conv3x3_dgrad_winograd_through_the_maxpool_backward(ops, B, Hu, Wu, Cin, Cout):
    """The input gradient of a layer behind a 2x2 max-pool with the pooling's backward as its epilogue equals the two
    separate launches (Winograd input gradient at pooled resolution, then wesup_maxpool2_bwd accumulating into the side-
    branch gradient): odd pre-pool sizes (the trailing row / column belongs to no window), ties (first maximum), windows
    whose maximum is not positive (ReLU: no gradient)."""
    d = dev()
    H, W = Hu // 2, Wu // 2
    ypre = rnd(B, Hu, Wu, Cin, seed=1)
    ypre[0, 0:2, 0:2, :8] = 0.37                              # a four-way tie: the first position wins
    if Wu >= 4:
        ypre[0, 0:2, 2:4, :8] = -1.0                          # a dead window
    w = rnd(Cout, Cin, 3, 3, seed=2, scale=(2.0 / (9 * Cin)) ** 0.5)
    dy = nhwc(rnd(B, Cout, H, W, seed=4)).to(d)
    base = rnd(B, Hu, Wu, Cin, seed=5)
    _, ud = ops.winograd_pack_weight(w.to(d), need_fwd=False, m=4)
    ypre_g = ypre.to(d)
    fused = base.clone().to(d)
    ops.conv3x3_dgrad_winograd_unpool(dy, ud, ypre_g, fused)
    dxp = ops.conv3x3_dgrad_winograd(dy, ud, m=4)
    two = base.clone().to(d)
    ops.maxpool2_bwd(ypre_g, dxp, two, accumulate=True)
    if _lib_mod().load().wesup_winograd_fused_supported(Cout, Cin, 4) == 1:
        # forward-only fusion: the plain input gradient of a short product takes the one-kernel route, the unpooling one
        # the two-kernel route -- the same sums in another order
        assert float((fused - two).abs().max()) < 1e-4 * float((two - base.to(d)).abs().max())
    else:
        assert torch.equal(fused, two)       # the same product kernel on both sides
    # and against autograd of relu -> max_pool2d -> conv on the CPU
    yp = nchw(ypre).double().requires_grad_(True)
    out = F.conv2d(F.max_pool2d(F.relu(yp), 2), w.double(), None, padding=1)
    out.backward(nchw(dy.cpu()).double())
    assert rel_err(nchw(fused.cpu() - base), yp.grad) < 2e-5
    # the C composite (the passes issued from C) is the same computation as the passes of the wrapper ...
    again = base.clone().to(d)
    _composite(ops, 'wesup_conv3x3_dgrad_winograd_unpool', B, H, W, Cout, Cin, 4, dy, ud, ypre_g, again, B, H, W, Hu, Wu, Cin, Cout, 4)
    assert torch.equal(again, fused)
    # ... which a timer sees bracketed as classes of their own, per route
    timed, rec = base.clone().to(d), _Tags()
    ops.conv3x3_dgrad_winograd_unpool(dy, ud, ypre_g, timed, timer=rec)
    assert torch.equal(timed, fused)
    assert rec.tags == _wino_tags(ops, Cout, Cin, ops.winograd_tiles(B, H, W, 4))


@pytest.mark.parametrize('B,Hd,Wd,g,Cin,Cout,pooled', [(2, 32, 32, 4, 64, 64, False), (1, 44, 36, 5, 64, 128, True), (2, 24, 40, 4, 64, 64, True),
                                                      (1, 30, 26, 3, 128, 64, False)])
def test_conv3x3_dgrad_winograd_with_the_side_gradient_gathered_in_the_epilogue(ops, B, Hd, Wd, g, Cin, Cout, pooled):
    """conv3x3_dgrad_winograd_gather: the destination's old content (the side-branch gradient of a native-resolution layer of
    the commuted side branch: one row per superpixel over its area) is gathered by the epilogue instead of being materialised by
    wesup_upsample_bwd and accumulated into.  Against exactly that pair of launches -- masked accumulate form and max-pool
    backward form (destination (Hd, Wd), dy at half of it) -- to the rounding of one multiply-add."""
    d = dev()
    labs, masks = _sp_case(3, B, Hd, Wd, g)
    Kmax = int(labs.max()) + 3
    m = ops.sp_preprocess(torch.from_numpy(labs).to(d), torch.from_numpy(masks).to(d), Kmax)
    side = rnd(B, Kmax, Cin, seed=7).to(d)
    H, W = (Hd // 2, Wd // 2) if pooled else (Hd, Wd)
    w = rnd(Cout, Cin, 3, 3, seed=2, scale=(2.0 / (9 * Cin)) ** 0.5)
    _, ud = ops.winograd_pack_weight(w.to(d), need_fwd=False, m=4)
    dy = nhwc(rnd(B, Cout, H, W, seed=4)).to(d)
    ypre = rnd(B, Hd, Wd, Cin, seed=1).to(d)
    want = ops.upsample_bwd_fused(side, m.new_row, m.area_new, Hd, Wd, 0, Hd, Wd, Cin)
    base = want.clone()
    if pooled:
        ops.conv3x3_dgrad_winograd_unpool(dy, ud, ypre, want)
    else:
        ops.conv3x3_dgrad_winograd(dy, ud, mask_src=ypre, out=want, accumulate=True, m=4)
    got = torch.full((B, Hd, Wd, Cin), float('nan'), device=d)
    ops.conv3x3_dgrad_winograd_gather(dy, ud, side, m.new_row, m.area_new, out=got, mask_src=None if pooled else ypre,
                                      unpool_src=ypre if pooled else None)
    scale = float(want.abs().max())
    # (a grid this small sends the plain entries through the batched GEMM + output transform -- other summation order -- while
    # the gather form always is the one-kernel route: then to the rounding of the products instead of one multiply-add)
    same_route = ops.winograd_fused_supported(Cout, Cin, 4, ops.winograd_tiles(B, H, W, 4)) == 2
    assert float((got - want).abs().max()) <= (2e-7 if same_route else 4e-6) * scale
    assert float((want - base).abs().max()) > 0.05 * scale         # the conv part is not negligible beside the gathered part
    # the C composite (the passes issued from C) is the same computation as the passes of the wrapper ...
    again = torch.empty_like(got)
    _composite(ops, 'wesup_conv3x3_dgrad_winograd_gather', B, H, W, Cout, Cin, 4, dy, ud, None if pooled else ypre,
               ypre if pooled else None, again, side, m.new_row, m.area_new, Kmax, B, H, W, Hd if pooled else 0, Wd if pooled else 0,
               Cin, Cout)
    assert torch.equal(again, got)
    # ... which a timer sees bracketed as classes of their own: always the one-kernel route; no transform when dy's is handed in
    timed, rec = torch.empty_like(got), _Tags()
    ops.conv3x3_dgrad_winograd_gather(dy, ud, side, m.new_row, m.area_new, out=timed, mask_src=None if pooled else ypre,
                                      unpool_src=ypre if pooled else None, timer=rec)
    assert torch.equal(timed, got) and rec.tags == ['winograd_transform', 'winograd_gemm']
    timed, rec = torch.empty_like(got), _Tags()
    ops.conv3x3_dgrad_winograd_gather(dy, ud, side, m.new_row, m.area_new, out=timed, mask_src=None if pooled else ypre,
                                      unpool_src=ypre if pooled else None, timer=rec, v_pre=ops.winograd_input_transform(dy, m=4))
    assert torch.equal(timed, got) and rec.tags == ['winograd_gemm']
    # the side rows divided by their areas beforehand (scale_rows_by_area; area_new = None): the same coefficient applied once
    # per row instead of once per pixel -- one rounding more per element (the product is no longer fused into the sum)
    scaled = ops.scale_rows_by_area(side.clone(), m.area_new)
    ref_rows = side / m.area_new.clamp(min=1).unsqueeze(-1).float()
    live = (m.area_new > 0).unsqueeze(-1)
    assert torch.equal(scaled[live.expand_as(scaled)], (side * (1.0 / m.area_new.clamp(min=1).float()).unsqueeze(-1))[live.expand_as(scaled)])
    assert float((scaled - torch.where(live, ref_rows, torch.zeros_like(ref_rows))).abs().max()) <= 1e-6 * float(ref_rows.abs().max())
    pre = torch.full_like(got, float('nan'))
    ops.conv3x3_dgrad_winograd_gather(dy, ud, scaled, m.new_row, None, out=pre, mask_src=None if pooled else ypre,
                                      unpool_src=ypre if pooled else None)
    assert float((pre - got).abs().max()) <= 2e-6 * float(got.abs().max())


@pytest.mark.parametrize('B,H,W,Cin,Cout', [(2, 24, 16, 64, 64), (1, 37, 41, 64, 128), (1, 13, 9, 256, 512), (3, 8, 8, 512, 512)])
def test_winograd_dual_transform_and_weight_gradient_from_it(ops, B, H, W, Cin, Cout):
    """winograd_dual_transform: one pass over a gradient tensor leaves exactly what the two separate F(4x4) transforms leave (input
    transform for the input gradient, outgrad transform for the weight gradient), and conv3x3_wgrad_winograd_pre on those operands
    gives the weight and bias gradient of conv3x3_wgrad_winograd bit for bit."""
    d = dev()
    x = torch.relu(rnd(B, H, W, Cin, seed=1)).to(d)
    dy = rnd(B, H, W, Cout, seed=2).to(d)
    T = ops.winograd_tiles(B, H, W, 4)
    V = torch.full((36, T, Cout), float('nan'), device=d)
    dM = torch.full((36, T, Cout), float('nan'), device=d)
    rows = ops.winograd_bias_rows(B, H, W, Cout)
    assert rows > 0
    bp = torch.empty(rows, Cout, device=d)
    ops.winograd_dual_transform(dy, V, dM, bp)
    assert torch.equal(V, ops.winograd_input_transform(dy, m=4))
    assert torch.equal(dM, ops.winograd_outgrad_transform(dy, m=4))
    assert rel_err(bp.sum(0), dy.sum((0, 1, 2))) < 1e-5
    Vx = ops.winograd_input_transform(x, m=4)
    dw, db = ops.conv3x3_wgrad_winograd(x, dy, relu_in=False, v_pre=Vx, m=4)
    dw2 = torch.empty_like(dw); db2 = torch.empty_like(db)
    ops.conv3x3_wgrad_winograd_pre(Vx, dM, bp, B, H, W, dw2, db2)
    assert torch.equal(dw, dw2) and torch.equal(db, db2)
    # the input gradient from the transformed operand: same bits as from dy itself
    w = rnd(Cout, Cin, 3, 3, seed=3, scale=(2.0 / (9 * Cin)) ** 0.5)
    _, ud = ops.winograd_pack_weight(w.to(d), need_fwd=False, m=4)
    assert torch.equal(ops.conv3x3_dgrad_winograd(dy, ud, m=4), ops.conv3x3_dgrad_winograd(dy, ud, m=4, v_pre=V))
    # ... also through a max-pool backward (one-kernel route or batched products + unpooling output transform)
    ypre = rnd(B, 2 * H, 2 * W, Cin, seed=4).to(d)
    base = rnd(B, 2 * H, 2 * W, Cin, seed=5).to(d)
    a, b_ = base.clone(), base.clone()
    ops.conv3x3_dgrad_winograd_unpool(dy, ud, ypre, a)
    ops.conv3x3_dgrad_winograd_unpool(dy, ud, ypre, b_, v_pre=V)
    assert torch.equal(a, b_)
    timed, rec = base.clone(), _Tags()          # a timer sees no input transform then
    ops.conv3x3_dgrad_winograd_unpool(dy, ud, ypre, timed, v_pre=V, timer=rec)
    assert torch.equal(a, timed) and rec.tags == _wino_tags(ops, Cout, Cin, T, v_pre=True)


def _pool_codes(y):
    """(B,H,W,C) -> (B,H//2,W//2,C) codes of the 2x2 max-pool's decisions: 0 = the window's maximum is not positive, k + 1 =
    first maximum at window position k (row-major)."""
    B, H, W, C = y.shape
    Hp, Wp = H // 2, W // 2
    win = torch.stack([y[:, 0:2 * Hp:2, 0:2 * Wp:2], y[:, 0:2 * Hp:2, 1:2 * Wp:2], y[:, 1:2 * Hp:2, 0:2 * Wp:2], y[:, 1:2 * Hp:2, 1:2 * Wp:2]], 0)
    mx, idx = win.max(0)                       # torch.max returns the first maximal index along the dim? not guaranteed: do it by hand
    first = torch.full_like(idx, 3)
    for k in (2, 1, 0):
        first = torch.where(win[k] == mx, torch.full_like(idx, k), first)
    return torch.where(mx > 0, first + 1, torch.zeros_like(first))


@pytest.mark.parametrize('B,H,W,Cin,Cout', [(2, 24, 16, 64, 64), (1, 38, 42, 64, 128), (1, 17, 13, 128, 128), (2, 8, 8, 256, 256)])
def test_winograd_compact_masks_and_pool_codes(ops, B, H, W, Cin, Cout):
    """The compact forms the forward leaves for the backward (F(4x4), one-kernel route): sign bits of the input from the input
    transform, pooling codes from the pooling epilogue -- checked against the tensors they stand for -- and the dgrad
    epilogues that read them (masked accumulate, max-pool backward, both gather forms): the same bits as with the float
    tensors."""
    d = dev()
    # (grids this small take the two-kernel route by default; the float-tensor twins of this test must run the same product
    # kernel as the compact forms, which only exist on the one-kernel route)
    was = _lib_mod().load().wesup_winograd_set_fused_min_blocks(0)
    try:
        _compact_masks_body(ops, d, B, H, W, Cin, Cout)
    finally:
        _lib_mod().load().wesup_winograd_set_fused_min_blocks(was)


def _compact_masks_body(ops, d, B, H, W, Cin, Cout):
    x = rnd(B, H, W, Cin, seed=1).to(d)
    x[0, :2, :2, :8] = 0.0                                    # exact zeros: not positive
    w = rnd(Cout, Cin, 3, 3, seed=2, scale=(2.0 / (9 * Cin)) ** 0.5)
    uf, ud = ops.winograd_pack_weight(w.to(d), m=4)
    bias = rnd(Cout, seed=3).to(d)
    bits = torch.zeros(B, H, W, Cin // 4, dtype=torch.uint8, device=d)
    codes = torch.full((B, H // 2, W // 2, Cout // 4), -1, dtype=torch.int16, device=d)
    yp = torch.empty(B, H // 2, W // 2, Cout, device=d)
    y = ops.conv3x3_fwd_winograd(x, uf, bias, relu_in=True, out_pool=yp, m=4, relu_bits_out=bits, pool_code_out=codes)
    y_ref = ops.conv3x3_fwd_winograd(x, uf, bias, relu_in=True, out_pool=torch.empty_like(yp), m=4)
    assert torch.equal(y, y_ref)
    xb = (x > 0).view(B, H, W, Cin // 4, 4).to(torch.uint8)
    assert torch.equal(bits, xb[..., 0] | (xb[..., 1] << 1) | (xb[..., 2] << 2) | (xb[..., 3] << 3))
    c4 = _pool_codes(y).view(B, H // 2, W // 2, Cout // 4, 4).to(torch.int16)
    assert torch.equal(codes, c4[..., 0] | (c4[..., 1] << 3) | (c4[..., 2] << 6) | (c4[..., 3] << 9))
    assert torch.equal(yp, F.max_pool2d(nchw(y), 2).permute(0, 2, 3, 1))
    # consumers.  dy of the layer (Cout channels) -> gradient w.r.t. x (pre-ReLU values: mask x > 0)
    dy = rnd(B, H, W, Cout, seed=5).to(d)
    base = rnd(B, H, W, Cin, seed=6).to(d)
    a, b_ = base.clone(), base.clone()
    ops.conv3x3_dgrad_winograd(dy, ud, mask_src=x, out=a, accumulate=True, m=4)
    ops.conv3x3_dgrad_winograd(dy, ud, out=b_, accumulate=True, m=4, mask_bits=bits)
    assert torch.equal(a, b_)
    # ... and through a max-pool: x2 (B,2H,2W,Cin) pre-pool activations with their codes
    x2 = rnd(B, 2 * H, 2 * W, Cin, seed=7).to(d)
    c2 = _pool_codes(x2).view(B, H, W, Cin // 4, 4).to(torch.int16)
    code2 = (c2[..., 0] | (c2[..., 1] << 3) | (c2[..., 2] << 6) | (c2[..., 3] << 9)).contiguous()
    base2 = rnd(B, 2 * H, 2 * W, Cin, seed=8).to(d)
    a, b_ = base2.clone(), base2.clone()
    ops.conv3x3_dgrad_winograd_unpool(dy, ud, x2, a)
    ops.conv3x3_dgrad_winograd_unpool(dy, ud, None, b_, unpool_code=code2)
    assert torch.equal(a, b_)
    # gather forms
    labs, masks = _sp_case(3, B, 2 * H, 2 * W, 3)
    Kmax = int(labs.max()) + 2
    m2 = ops.sp_preprocess(torch.from_numpy(labs).to(d), torch.from_numpy(masks).to(d), Kmax)
    side = rnd(B, Kmax, Cin, seed=9).to(d)
    a, b_ = torch.empty_like(base2), torch.empty_like(base2)
    ops.conv3x3_dgrad_winograd_gather(dy, ud, side, m2.new_row, m2.area_new, out=a, unpool_src=x2)
    ops.conv3x3_dgrad_winograd_gather(dy, ud, side, m2.new_row, m2.area_new, out=b_, unpool_code=code2)
    assert torch.equal(a, b_)
    labs, masks = _sp_case(4, B, H, W, 3)
    Kmax = int(labs.max()) + 2
    m1 = ops.sp_preprocess(torch.from_numpy(labs).to(d), torch.from_numpy(masks).to(d), Kmax)
    side = rnd(B, Kmax, Cin, seed=10).to(d)
    a, b_ = torch.empty_like(base), torch.empty_like(base)
    ops.conv3x3_dgrad_winograd_gather(dy, ud, side, m1.new_row, m1.area_new, out=a, mask_src=x)
    ops.conv3x3_dgrad_winograd_gather(dy, ud, side, m1.new_row, m1.area_new, out=b_, mask_bits=bits)
    assert torch.equal(a, b_)


@pytest.mark.parametrize('B,H,W,Cin,Cout', [c for c in CONV_CASES if c[3] != 3])
def test_conv3x3_dgrad(ops, B, H, W, Cin, Cout):
    d = dev()
    x = rnd(B, Cin, H, W, seed=1).requires_grad_(True)
    w = rnd(Cout, Cin, 3, 3, seed=2, scale=(2.0 / (9 * Cin)) ** 0.5)
    dy = rnd(B, Cout, H, W, seed=4)
    y = F.conv2d(F.relu(x), w, None, padding=1)
    y.backward(dy)
    ref = x.grad                                   # includes the ReLU mask (x > 0)
    _, wd = ops.pack_conv3x3_weight(w.to(d))
    base = rnd(B, H, W, Cin, seed=5)
    out = base.clone().to(d)
    ops.conv3x3_dgrad(nhwc(dy).to(d), wd, Cin, mask_src=nhwc(x.detach()).to(d), out=out, accumulate=True)
    assert rel_err(nchw(out.cpu() - base), ref) < TOL
    # plain (no mask, no accumulate)
    x2 = rnd(B, Cin, H, W, seed=1).requires_grad_(True)
    F.conv2d(x2, w, None, padding=1).backward(dy)
    out2 = ops.conv3x3_dgrad(nhwc(dy).to(d), wd, Cin)
    assert rel_err(nchw(out2), x2.grad) < TOL


@pytest.mark.parametrize('B,H,W,Cin,Cout', CONV_CASES[:5] + [(1, 120, 96, 64, 64), (2, 60, 60, 128, 128), (1, 100, 90, 3, 64),
                                                 (3, 35, 17, 64, 64), (2, 33, 40, 32, 160), (1, 70, 50, 128, 64)])
@pytest.mark.parametrize('relu_in', [False, True])
def test_conv3x3_wgrad(ops, B, H, W, Cin, Cout, relu_in):
    d = dev()
    x = rnd(B, Cin, H, W, seed=1)
    w = rnd(Cout, Cin, 3, 3, seed=2, scale=0.05).requires_grad_(True)
    b = torch.zeros(Cout, requires_grad=True)
    dy = rnd(B, Cout, H, W, seed=4)
    F.conv2d(F.relu(x) if relu_in else x, w, b, padding=1).backward(dy)
    xg = ops.pack_input(x.to(d)) if Cin == 3 else nhwc(x).to(d)
    dw, db = ops.conv3x3_wgrad(xg, nhwc(dy).to(d), Cin, relu_in)
    assert rel_err(dw, w.grad) < TOL
    assert rel_err(db, b.grad) < TOL
    dw2, db2 = ops.conv3x3_wgrad(xg, nhwc(dy).to(d), Cin, relu_in)      # deterministic split-K
    assert torch.equal(dw, dw2) and torch.equal(db, db2)


# ---------------------------------------------------------------- GEMMs
@pytest.mark.parametrize('M,N,K', [(100, 32, 64), (2400, 1024, 2112), (600, 2112, 1024), (57600, 64, 128),
                                   (50000, 256, 64), (37, 32, 1024), (49160, 32, 64)])
def test_gemm_nt(ops, M, N, K):
    d = dev()
    A = rnd(M, K, seed=1)
    Bw = rnd(N, K, seed=2, scale=K ** -0.5)
    bias = rnd(N, seed=3)
    ref = A @ Bw.t() + bias
    out = ops.gemm_nt(A.to(d), Bw.to(d), bias.to(d))
    assert rel_err(out, ref) < TOL
    out = ops.gemm_nt(A.to(d), Bw.to(d), bias.to(d), flags=ops.RELU_OUT | ops.RELU_IN)
    assert rel_err(out, F.relu(F.relu(A) @ Bw.t() + bias)) < TOL
    # mask + accumulate into a strided (column-slice) output
    big = rnd(M, N + 64, seed=4).to(d)
    base = big.clone()
    mask = rnd(M, N, seed=5)
    ops.gemm_nt(A.to(d), Bw.to(d), None, out=big[:, 32:32 + N], mask=mask.to(d), flags=ops.ACCUM)
    ref2 = base.cpu()
    ref2[:, 32:32 + N] += torch.where(mask > 0, A @ Bw.t(), torch.zeros(()))
    assert rel_err(big, ref2) < TOL


@pytest.mark.parametrize('M,N,K', [(32, 1024, 2400), (1024, 2112, 600), (64, 128, 57600), (256, 512, 3601), (32, 64, 230400)])
def test_gemm_tn_colsum(ops, M, N, K):
    d = dev()
    A = rnd(K, M, seed=1)
    Bm = rnd(K, N, seed=2)
    out = ops.gemm_tn(A.to(d), Bm.to(d))
    ref = (A.double().t() @ Bm.double()).float()
    assert rel_err(out, ref) < TOL
    out_r = ops.gemm_tn(A.to(d), Bm.to(d), relu_b=True)
    assert rel_err(out_r, (A.double().t() @ F.relu(Bm).double()).float()) < TOL
    assert torch.equal(out, ops.gemm_tn(A.to(d), Bm.to(d)))
    cs = ops.colsum(A.to(d))
    assert rel_err(cs, A.double().sum(0).float()) < TOL
    cs2 = torch.empty(M, device=d)                                     # the same sums as a by-product of the GEMM
    out2 = ops.gemm_tn(A.to(d), Bm.to(d), colsum=cs2)
    assert torch.equal(out2, out) and rel_err(cs2, A.double().sum(0).float()) < TOL
    cs3 = torch.empty(M, device=d)
    ops.gemm_tn(A.to(d), Bm.to(d), colsum=cs3)
    assert torch.equal(cs2, cs3)
    assert rel_err(ops.transpose(Bm.to(d)), Bm.t()) == 0.0


def test_gemm_tn_batched(ops):
    d = dev()
    nb, K, M, N = 3, 900, 584, 768
    A = rnd(nb, K, M, seed=1).to(d)
    big = rnd(nb, K, N + 128, seed=2).to(d)
    Bm = big[:, :, 64:64 + N]                                              # row-strided operand
    outbig = torch.zeros(nb, M, N + 32, device=d)
    out = outbig[:, :, 32:]
    ops.gemm_tn_batched(A, Bm, out)
    ref = torch.einsum('bkm,bkn->bmn', A.double().cpu(), Bm.double().cpu()).float()
    assert rel_err(out, ref) < TOL
    assert float(outbig[:, :, :32].abs().max()) == 0.0
    for i in range(nb):                                                    # same numbers as the single-product entry?
        assert rel_err(ops.gemm_tn(A[i], Bm[i]), ref[i]) < TOL


@pytest.mark.parametrize('nb,M,N,K', [(36, 900, 512, 512), (36, 900, 256, 512), (36, 256, 512, 512), (9, 3604, 384, 64)])
def test_gemm_nt_batched_shapes_of_the_k512_products(ops, nb, M, N, K):
    """wesup_gemm_nt_batched on the shapes of the step's K = 512 Winograd products: the 36 products of conv4_x at 4 x 480^2 take the
    128 x 64 tile three to a CU (2304 = 9 x 256 blocks, csrc/gemm.hip), conv5_x the 64 x 64 tile; ragged M."""
    d = dev()
    A = rnd(nb, M, K, seed=11).to(d)
    Bw = rnd(nb, N, K, seed=12).to(d)
    out = ops.gemm_nt_batched(A, Bw)
    ref = torch.einsum('bmk,bnk->bmn', A.double().cpu(), Bw.double().cpu()).float()
    assert rel_err(out, ref) < TOL
    assert torch.equal(out, ops.gemm_nt_batched(A, Bw))


def test_gemm_tn_one_split_stores_straight_into_a_strided_output(ops):
    """Grids that fill the chip without a split (>= 600 tiles: the step's Wm^T g at 60 x 60, four images) run one split and the
    kernel's epilogue stores into C itself -- no slab, no reduce launch (csrc/gemm.hip: tn_direct).  Row-strided outputs with
    untouched neighbours, batched and single, M not a multiple of the tile."""
    d = dev()
    nb, K, M, N = 4, 640, 3600, 768
    A = rnd(nb, K, M, seed=3).to(d)
    Bm = rnd(nb, K, N, seed=4).to(d)
    outbig = torch.full((nb, M, N + 64), 7.0, device=d)
    out = outbig[:, :, 32:32 + N]
    ops.gemm_tn_batched(A, Bm, out)
    ref = torch.einsum('bkm,bkn->bmn', A.double().cpu(), Bm.double().cpu()).float()
    assert rel_err(out, ref) < TOL
    assert float((outbig[:, :, :32] - 7.0).abs().max()) == 0.0 and float((outbig[:, :, 32 + N:] - 7.0).abs().max()) == 0.0
    K, M, N = 330, 4036, 2556                        # 32 x 20 tiles of 128 x 128, ragged edges in both directions
    A1, B1 = rnd(K, M, seed=5).to(d), rnd(K, N, seed=6).to(d)
    big = torch.full((M, N + 8), -3.0, device=d)
    ops.gemm_tn(A1, B1, out=big[:, 4:4 + N])
    assert rel_err(big[:, 4:4 + N], (A1.double().cpu().t() @ B1.double().cpu()).float()) < TOL
    assert float((big[:, :4] + 3.0).abs().max()) == 0.0 and float((big[:, 4 + N:] + 3.0).abs().max()) == 0.0
    cs = torch.empty(M, device=d)                    # with column sums the slab path stays (they sit behind the slabs)
    out_cs = ops.gemm_tn(A1, B1, colsum=cs)
    assert torch.equal(out_cs, big[:, 4:4 + N].contiguous()) and rel_err(cs, A1.double().cpu().sum(0).float()) < TOL


def test_gemm_nt_group_one_launch_with_per_product_bias(ops):
    """wesup_gemm_nt_batched_bias through ops.gemm_nt_group: three side convs of one resolution (weights and biases views of
    one flat parameter buffer, outputs column slices of the side-feature matrix) in one launch -- the numbers of three
    single launches, bit for bit; unequally spaced operands launch nothing and return False."""
    d = dev()
    P, co, cs = 900, 512, 256
    y = rnd(3, P, co, seed=1).to(d)
    flat = (rnd(3 * (cs * co + cs), seed=2) * 0.05).to(d)
    step = cs * co + cs
    ws = [flat[i * step:i * step + cs * co].view(cs, co) for i in range(3)]
    bs = [flat[i * step + cs * co:(i + 1) * step] for i in range(3)]
    s = torch.zeros(P, 3 * cs + 64, device=d)
    outs = [s[:, cs * i:cs * (i + 1)] for i in range(3)]
    assert ops.gemm_nt_group([y[i] for i in range(3)], ws, bs, outs) is True
    assert float(s[:, 3 * cs:].abs().max()) == 0.0
    for i in range(3):
        ref = y[i].double().cpu() @ ws[i].double().cpu().t() + bs[i].double().cpu()
        assert rel_err(outs[i], ref.float()) < TOL
        assert torch.equal(ops.gemm_nt(y[i], ws[i], bs[i]), outs[i])
    before = s.clone()
    assert ops.gemm_nt_group([y[0], y[2], y[1]], ws, bs, outs) is False and torch.equal(before, s)


# ---------------------------------------------------------------- maxpool / upsample
@pytest.mark.parametrize('B,H,W,C', [(2, 8, 6, 64), (1, 30, 30, 512), (1, 10, 14, 128)])
def test_maxpool(ops, B, H, W, C):
    d = dev()
    y = rnd(B, C, H, W, seed=1)
    y[:, :, 0:2, 0:2] = 0.5                       # exact ties -> first max takes the gradient
    yr = y.clone().requires_grad_(True)
    p = F.max_pool2d(F.relu(yr), 2, 2)
    dyp = rnd(*p.shape, seed=2)
    p.backward(dyp)
    yp = ops.maxpool2_fwd(nhwc(y).to(d))
    assert torch.equal(F.relu(nchw(yp)).cpu(), p.detach())
    assert torch.equal(nchw(ops.maxpool2_fwd(nhwc(y).to(d), relu=True)).cpu(), p.detach())       # ReLU applied as it stores
    base = rnd(B, H, W, C, seed=3)
    out = base.clone().to(d)
    ops.maxpool2_bwd(nhwc(y).to(d), nhwc(dyp).to(d), out, accumulate=True)
    assert torch.equal(out.cpu(), base + nhwc(yr.grad))           # every value is a copy or one fp32 add (tests/test_pooling_branches_gpu.py)


@pytest.mark.parametrize('B,h,w,H,W,C', [(2, 4, 4, 8, 8, 32), (1, 2, 2, 32, 32, 256), (1, 15, 15, 240, 240, 64),
                                          (2, 6, 5, 96, 80, 64), (1, 8, 8, 8, 8, 32), (1, 1, 1, 16, 16, 32)])
def test_upsample(ops, B, h, w, H, W, C):
    d = dev()
    s = rnd(B, C, h, w, seed=1).requires_grad_(True)
    up = F.interpolate(s, (H, W), mode='bilinear', align_corners=True)
    ldf, coff = C + 64, 32
    fm = torch.zeros(B, H, W, ldf, device=d)
    ops.upsample_fwd(nhwc(s.detach()).to(d), fm, coff)
    assert rel_err(nchw(fm[..., coff:coff + C]), up) < 1e-5
    assert float(fm[..., :coff].abs().max()) == 0.0 and float(fm[..., coff + C:].abs().max()) == 0.0
    dfm = rnd(B, H, W, ldf, seed=2)
    up.backward(nchw(dfm[..., coff:coff + C]))
    ds = ops.upsample_bwd(dfm.to(d), coff, h, w, C)
    assert rel_err(nchw(ds), s.grad) < 1e-5


# ---------------------------------------------------------------- superpixel preprocessing + pooling
def _sp_case(seed, B, H, W, g, mode='point'):
    from wesup_amd import synth
    labs = np.stack([synth.voronoi_labels(seed + b, H, W, g) for b in range(B)])
    if mode == 'point':
        masks = np.stack([synth.point_mask(seed + b, labs[b], 0.25, 2, tie_every=3) for b in range(B)])
    elif mode == 'full':
        masks = np.stack([synth.pixel_mask(seed + b, H, W) for b in range(B)])
    else:
        masks = None
    return labs, masks


@pytest.mark.parametrize('B,H,W,g,mode,Kpad', [(2, 32, 32, 4, 'point', 0), (1, 96, 80, 7, 'point', 11), (2, 64, 64, 6, 'full', 0),
                                                 (1, 64, 64, 6, 'none', 3), (1, 480, 480, 24, 'point', 0)])
def test_sp_preprocess(ops, B, H, W, g, mode, Kpad):
    from oracle import wesup_oracle as orc
    d = dev()
    labs, masks = _sp_case(7, B, H, W, g, mode)
    Kmax = g * g + Kpad
    m = ops.sp_preprocess(torch.from_numpy(labs).to(d), None if masks is None else torch.from_numpy(masks).to(d), Kmax)
    m.check()
    for b in range(B):
        pp = orc.preprocess_superpixels(torch.from_numpy(labs[b]).long(),
                                        None if masks is None else torch.from_numpy(masks[b]).long())
        K, n_l = pp['K'], pp['n_l']
        assert int(m.n_sp[b]) == K and int(m.n_l[b]) == n_l
        assert torch.equal(m.perm[b, :K].cpu().long(), pp['perm'])
        assert torch.equal(m.inv_perm[b, :K].cpu().long(), pp['inv_perm'])
        assert torch.equal(m.area_new[b, :K].cpu().long(), pp['area'][pp['perm']])
        assert int(m.area_new[b, K:].abs().sum()) == 0
        assert torch.equal(m.sp_labels[b, :n_l].cpu(), pp['sp_labels'][:, :2] if n_l else m.sp_labels[b, :0].cpu())
        assert float(m.sp_labels[b, n_l:].abs().sum()) == 0.0
        new_row = pp['inv_perm'][torch.from_numpy(labs[b]).long().reshape(-1)]
        assert torch.equal(m.new_row[b].cpu().long(), new_row)
        # stable counting sort: pixels grouped by row, ascending inside a row
        order = torch.argsort(new_row, stable=True)
        assert torch.equal(m.pix_sorted[b].cpu().long(), order)
        rs = torch.zeros(Kmax + 1, dtype=torch.long)
        rs[1:K + 1] = torch.cumsum(pp['area'][pp['perm']], 0)
        rs[K + 1:] = H * W
        assert torch.equal(m.row_start[b].cpu().long(), rs)


def test_sp_preprocess_rejects_bad_maps(ops):
    d = dev()
    lab = torch.zeros(1, 8, 8, dtype=torch.int32)
    lab[0, 4:] = 2                                    # id 1 is empty
    m = ops.sp_preprocess(lab.to(d), None, 4)
    with pytest.raises(ValueError):
        m.check()
    lab[0, 0, 0] = 9                                  # id >= Kmax
    m = ops.sp_preprocess(lab.to(d), None, 4)
    with pytest.raises(ValueError):
        m.check()


@pytest.mark.parametrize('B,H,W,g,C', [(2, 32, 32, 4, 2112), (1, 96, 80, 7, 2112), (1, 64, 64, 6, 256), (1, 120, 120, 12, 2112)])
def test_sp_pool(ops, B, H, W, g, C):
    from oracle import wesup_oracle as orc
    d = dev()
    labs, masks = _sp_case(11, B, H, W, g)
    Kmax = g * g + 5
    m = ops.sp_preprocess(torch.from_numpy(labs).to(d), torch.from_numpy(masks).to(d), Kmax)
    fm = rnd(B, H, W, C, seed=3)
    out = ops.sp_pool_fwd(fm.to(d), m)
    gup = rnd(B, Kmax, C, seed=4)
    dfm = ops.sp_pool_bwd(gup.to(d), m)
    for b in range(B):
        pp = orc.preprocess_superpixels(torch.from_numpy(labs[b]).long(), torch.from_numpy(masks[b]).long())
        K = pp['K']
        seg_new = pp['inv_perm'][torch.from_numpy(labs[b]).long().reshape(-1)]
        area_new = pp['area'][pp['perm']]
        fmc = fm[b].reshape(H * W, C).t().contiguous().requires_grad_(True)        # (C, HW) as the reference holds it
        ref = orc.pool_labelmap(fmc, seg_new, area_new, K)
        assert rel_err(out[b, :K], ref) < TOL
        assert float(out[b, K:].abs().max()) == 0.0
        ref.backward(gup[b, :K])
        assert rel_err(dfm[b].reshape(H * W, C), fmc.grad.t()) < TOL
    assert torch.equal(out, ops.sp_pool_fwd(fm.to(d), m))          # bitwise reproducible
    # fused upsample + scatter-mean forward == upsample_fwd followed by sp_pool_fwd
    for (h, w, Cs, coff) in [(H, W, 32, 0), (H, W, 64, 32), (H // 2, W // 2, 64, 64), (H // 2, W // 2, 128, 128), (H // 4, W // 4, 128, 128),
                             (H // 4, W // 4, 256, 0), (max(1, H // 8), max(1, W // 8), 512, 256), (max(1, H // 16), max(1, W // 16), 256, 512)]:
        if coff + Cs > C:
            continue
        sl = rnd(B, h, w, Cs, seed=9).to(d)
        fm2 = torch.zeros(B, H, W, C, device=d)
        ops.upsample_fwd(sl, fm2, coff)
        ref2 = ops.sp_pool_fwd(fm2, m)
        got = torch.zeros(B, Kmax, C, device=d)
        ops.sp_pool_upsample_fwd(sl, m, got, coff)
        assert rel_err(got[..., coff:coff + Cs], ref2[..., coff:coff + Cs]) < 1e-5
        assert float(got[..., :coff].abs().max() if coff else 0.0) == 0.0
        got2 = torch.zeros(B, Kmax, C, device=d)
        ops.sp_pool_upsample_fwd(sl, m, got2, coff)
        assert torch.equal(got, got2)
    # fused pool-backward + upsample-backward == unfused
    for (h, w, Cs, coff) in [(H, W, 32, 0), (H, W, 64, 32), (H // 2, W // 2, 64, 64), (H // 4, W // 4, 256, 0), (max(1, H // 8), max(1, W // 8), 512, 0), (max(1, H // 16), max(1, W // 16), 64, 128)]:
        if coff + Cs > C:
            continue
        a = ops.upsample_bwd(dfm, coff, h, w, Cs)
        f = ops.upsample_bwd_fused(gup.to(d), m.new_row, m.area_new, H, W, coff, h, w, Cs)
        assert rel_err(f, a) < 1e-5
    # ... and the layers of one coarse resolution in one launch (shared window scan): the per-layer values, bit for bit
    for (h, w, Cl) in [(H // 2, W // 2, (128, 128)), (H // 4, W // 4, (256, 256, 256)), (H // 2, W // 4, (64,)), (H // 4, W // 4, (32, 256)), (H // 4, W // 4, (512,))]:
        gs = [rnd(B, Kmax, c, seed=20 + i).to(d) for i, c in enumerate(Cl)]
        outs = [torch.full((B, h, w, c), 7.0, device=d) for c in Cl]
        ops.upsample_bwd_fused_group(gs, m.new_row, m.area_new, H, W, h, w, outs)
        for gi, oi in zip(gs, outs):
            if gi.shape[2] <= 256:
                assert torch.equal(oi, ops.upsample_bwd_fused(gi, m.new_row, m.area_new, H, W, 0, h, w, gi.shape[2]))
            else:          # wide dense rows take the group kernel inside wesup_upsample_bwd too: compare with a strided call
                wide = torch.zeros(B, Kmax, gi.shape[2] + 64, device=d)
                wide[..., 32:32 + gi.shape[2]] = gi
                assert rel_err(oi, ops.upsample_bwd_fused(wide, m.new_row, m.area_new, H, W, 32, h, w, gi.shape[2])) < 1e-6
                assert torch.equal(oi, ops.upsample_bwd_fused(gi, m.new_row, m.area_new, H, W, 0, h, w, gi.shape[2]))


def test_paint_and_dense_compat(ops):
    from oracle import wesup_oracle as orc
    d = dev()
    H = W = 32
    labs, masks = _sp_case(5, 1, H, W, 4)
    seg = torch.from_numpy(labs[0]).long()
    sp_maps, sp_labels = orc.preprocess_superpixels_dense(seg, torch.from_numpy(masks[0]).long())
    new_lab = ops.spmaps_to_labels(sp_maps.to(d))
    assert torch.equal(new_lab[0].cpu().long(), sp_maps.argmax(dim=0))
    m = ops.sp_preprocess(torch.from_numpy(labs).to(d), torch.from_numpy(masks).to(d), 16)
    sp_pred = torch.rand(1, 16, 2)
    pred = ops.paint_fwd(sp_pred.to(d), m)
    ref = sp_pred[0][sp_maps.argmax(dim=0).reshape(-1), 1].reshape(H, W)
    assert torch.equal(pred[0].cpu(), ref)


# ---------------------------------------------------------------- head, propagation, loss
def test_classifier(ops):
    d = dev()
    R, D = 700, 32
    feat = F.relu(rnd(R, D, seed=1)).requires_grad_(True)
    Wc = rnd(2, D, seed=2, scale=0.3).requires_grad_(True)
    bc = rnd(2, seed=3).requires_grad_(True)
    pre = rnd(R, D, seed=6).requires_grad_(True)              # feat = relu(pre) to check the ReLU mask
    featr = F.relu(pre)
    pred = F.softmax(F.linear(featr, Wc, bc), dim=1)
    dpred = rnd(R, 2, seed=4)
    extra = rnd(R, D, seed=5)
    (pred * dpred).sum().backward(retain_graph=True)
    (featr * extra).sum().backward()
    pg = ops.classifier_fwd(featr.detach().to(d), Wc.detach().to(d), bc.detach().to(d))
    assert rel_err(pg, pred) < 1e-5
    dfeat, dWc, dbc = ops.classifier_bwd(featr.detach().to(d), Wc.detach().to(d), pg, dpred.to(d), extra.to(d))
    assert rel_err(dfeat, pre.grad) < TOL
    assert rel_err(dWc, Wc.grad) < TOL and rel_err(dbc, bc.grad) < TOL


@pytest.mark.parametrize('seed,scale,ident', [(1, 0.08, False), (2, 0.5, False), (3, 0.12, False), (4, 0.0, True)])
def test_propagate_and_loss(ops, seed, scale, ident):
    from oracle import wesup_oracle as orc
    d = dev()
    B, H, W, g, D = 3, 64, 64, 6, 32
    labs, masks = _sp_case(20 + seed, B, H, W, g)
    Kmax = g * g + 4
    m = ops.sp_preprocess(torch.from_numpy(labs).to(d), torch.from_numpy(masks).to(d), Kmax)
    feat = F.relu(rnd(B, Kmax, D, seed=seed, scale=scale))
    if ident:
        feat = torch.zeros(B, Kmax, D) + 0.25                 # identical features: W = 1 everywhere -> first index
    pred = F.softmax(rnd(B, Kmax, 2, seed=seed + 50, scale=2.0), dim=2)
    pred[0, 0, 0], pred[0, 0, 1] = 1.0, 0.0                   # clamp edge: zero gradient outside [eps, 1-eps]
    y_all, src, sim = ops.propagate(feat.to(d), m, 0.8)
    loss, terms = ops.loss_fwd(pred.to(d), y_all, m, 1e-7, 0.5)
    dloss = torch.tensor([1.7], device=d)
    dpred = ops.loss_bwd(pred.to(d), y_all, m, terms, dloss, 1e-7, 0.5)
    ref_losses = []
    pr = pred.clone().requires_grad_(True)
    for b in range(B):
        pp = orc.preprocess_superpixels(torch.from_numpy(labs[b]).long(), torch.from_numpy(masks[b]).long())
        K, n_l = pp['K'], pp['n_l']
        y_u, W_ul, max_sim, s = orc.label_propagate(feat[b, :K], pp['sp_labels'], 0.8, return_aux=True)
        assert torch.equal(src[b, n_l:K].cpu().long(), s)                      # argmax indices bit-exact
        assert torch.equal(y_all[b, n_l:K].cpu(), y_u)
        assert torch.equal(y_all[b, :n_l].cpu(), pp['sp_labels'])
        assert rel_err(sim[b, n_l:K], max_sim) < 1e-5
        mets = {}
        ref_losses.append(orc.compute_loss(pr[b, :K], feat[b, :K], pp['sp_labels'], metrics=mets))
        assert abs(float(terms[b, 4]) - mets['propagated_labels']) == 0.0
        assert abs(float(terms[b, 2] / max(float(terms[b, 3]), 1.0)) - mets['propagate_loss']) < 1e-5
    ref = torch.stack(ref_losses).mean()
    assert abs(float(loss) - float(ref)) < 1e-5 * max(1.0, abs(float(ref)))
    (ref * 1.7).backward()
    assert rel_err(dpred, pr.grad) < TOL
    # propagation disabled -> no pseudo labels
    y_off, _, _ = ops.propagate(feat.to(d), m, 0.8, enable=False)
    for b in range(B):
        assert float(y_off[b, int(m.n_l[b]):].abs().sum()) == 0.0


@pytest.mark.parametrize('seed,scale', [(1, 0.1), (2, 0.35)])
def test_head_in_two_launches_equals_the_six_it_replaces_bit_for_bit(ops, seed, scale):
    """wesup_head_fwd = classifier_fwd + propagate, wesup_head_bwd (+ classifier_bwd_finish) = loss_fwd + loss_bwd + classifier_bwd
    (ABI 5, csrc/loss.hip): what the step runner launches between the fc layers' forward and backward.  Same numbers, bit for bit;
    the oracle checks of the separate entries (test_propagate_and_loss, test_classifier) then hold for these too."""
    d = dev()
    B, H, W, g, D = 3, 64, 64, 6, 32
    labs, masks = _sp_case(40 + seed, B, H, W, g)
    Kmax = 64
    m = ops.sp_preprocess(torch.from_numpy(labs).to(d), torch.from_numpy(masks).to(d), Kmax)
    feat = F.relu(rnd(B, Kmax, D, seed=seed, scale=scale)).to(d)
    Wc, bc = rnd(2, D, seed=seed + 7).to(d), rnd(2, seed=seed + 8).to(d)
    R = B * Kmax
    # the six launches
    pred = ops.classifier_fwd(feat.view(R, D), Wc, bc)
    y_all, src, sim = ops.propagate(feat, m, 0.8)
    _, terms = ops.loss_fwd(pred.view(B, Kmax, 2), y_all, m, 1e-7, 0.5)
    dloss = torch.tensor([1.0], device=d)
    dpred = ops.loss_bwd(pred.view(B, Kmax, 2), y_all, m, terms, dloss, 1e-7, 0.5)
    dfeat, dWc, dbc = ops.classifier_bwd(feat.view(R, D), Wc, pred, dpred.view(R, 2))
    # the two (+ the reduce off the chain)
    pred2 = torch.full((R, 2), 9.0, device=d)
    out2 = (torch.full((B, Kmax, 2), 9.0, device=d), torch.full((B, Kmax), 9, dtype=torch.int32, device=d), torch.full((B, Kmax), 9.0, device=d))
    ops.head_fwd(feat, Wc, bc, pred2, m, 0.8, out=out2)
    assert torch.equal(pred2, pred) and torch.equal(out2[0], y_all) and torch.equal(out2[1], src) and torch.equal(out2[2], sim)
    terms2, dpred2 = torch.full((B, 8), 9.0, device=d), torch.full((B, Kmax, 2), 9.0, device=d)
    dfeat2, dWc2, dbc2 = torch.full((R, D), 9.0, device=d), torch.full((2, D), 9.0, device=d), torch.full((2,), 9.0, device=d)
    part = ops.head_bwd_partials(R, D, d)
    ops.head_bwd(feat.view(R, D), Wc, pred2, out2[0], m, dloss, 1e-7, 0.5, terms2, dpred2, dfeat2, part)
    ops.classifier_bwd_finish(part, R, D, dWc2, dbc2)
    assert torch.equal(terms2, terms) and torch.equal(dpred2, dpred) and torch.equal(dfeat2, dfeat)
    assert torch.equal(dWc2, dWc) and torch.equal(dbc2, dbc)
    assert float(dpred.abs().max()) > 0 and float(dfeat.abs().max()) > 0
    assert ops.head_supported(64, 2) and not ops.head_supported(100, 2) and not ops.head_supported(64, 1)


def test_cross_entropy_generic(ops):
    from oracle import wesup_oracle as orc
    d = dev()
    y_hat = F.softmax(rnd(50, 2, seed=1), dim=1).requires_grad_(True)
    y_true = torch.zeros(50, 2)
    y_true[::3, 0] = 1
    y_true[1::7, 1] = 1
    ref = orc.cross_entropy(y_hat, y_true)
    ref.backward()
    out2 = ops.cross_entropy_fwd(y_hat.detach().to(d), y_true.to(d), 1e-7)
    assert abs(float(out2[0] / out2[1]) - float(ref)) < 1e-5
    dy = ops.cross_entropy_bwd(y_hat.detach().to(d), y_true.to(d), out2, torch.ones(1, device=d), 1e-7)
    assert rel_err(dy, y_hat.grad) < TOL
    out0 = ops.cross_entropy_fwd(y_hat.detach().to(d), torch.zeros(50, 2, device=d), 1e-7)
    assert float(out0[1]) == 0.0                                               # no labelled rows -> loss 0


def test_sgd_and_metrics(ops):
    from oracle import wesup_oracle as orc
    d = dev()
    n = 100003
    p = rnd(n + 1, seed=1)[:n]
    g = rnd(n + 1, seed=2)[:n]
    pd, gd = p.to(d).contiguous(), g.to(d).contiguous()
    vd = torch.zeros(n, device=d)
    params, bufs = {'w': p.clone()}, {}
    for step in range(3):
        params, bufs = orc.sgd_step(params, {'w': g * 0.5}, bufs, 5e-5, 0.9, 1e-3)
        ops.sgd_step(pd, gd, vd, 5e-5, 0.9, 1e-3, 0.5, step == 0)
    assert rel_err(pd, params['w']) < 1e-6 and rel_err(vd, bufs['w']) < 1e-6
    from wesup_amd import synth
    B, H, W = 2, 40, 36
    pred = torch.rand(B, H, W)
    pred[0, 0, :4] = torch.tensor([0.5, 1.5, 0.4999, 0.5001])                 # round half to even
    mask = np.stack([synth.pixel_mask(b, H, W) for b in range(B)])
    out = ops.seg_metrics(pred.to(d), torch.from_numpy(mask).to(d)).cpu()
    P = pred.round().long()
    G = torch.from_numpy(mask).long().argmax(dim=1)
    for b in range(B):
        acc = float(out[b, 0]) / (H * W)
        dice = 2 * float(out[b, 1]) / (float(out[b, 3]) + float(out[b, 2]) + 1e-7)
        assert abs(acc - orc.accuracy(P[b], G[b])) < 1e-6
        assert abs(dice - orc.dice(P[b], G[b])) < 1e-6


@pytest.mark.parametrize('H,W,g', [(128, 128, 16), (240, 200, 20)])
def test_sp_pool_skewed_maps_multi_segment_rows(ops, H, W, g):
    """Adversarial label maps (a few superpixels ~50x the median): rows longer than one 512-pixel
    segment go through the partial-sum + ordered combine path of both pooling kernels."""
    from oracle import wesup_oracle as orc
    from wesup_amd import synth
    d = dev()
    B, C = 2, 2112
    labs = np.stack([synth.skewed_labels(31 + b, H, W, g) for b in range(B)])
    Kmax = int(labs.max()) + 3
    m = ops.sp_preprocess(torch.from_numpy(labs).to(d), None, Kmax)
    m.check()
    areas = m.area_new.cpu()
    assert int(areas.max()) > 4 * 512                      # really multi-segment
    seg = m.seg_start.cpu()
    for b in range(B):
        nseg = torch.clamp((areas[b] + 511) // 512, min=1)
        assert torch.equal(seg[b, 1:] - seg[b, :-1], nseg.int())
        ur = m.unit_row[b, :int(seg[b, -1])].cpu()
        assert torch.equal(ur, torch.repeat_interleave(torch.arange(Kmax, dtype=torch.int32), nseg))
    fm = rnd(B, H, W, C, seed=3)
    out = ops.sp_pool_fwd(fm.to(d), m)
    for b in range(B):
        pp = orc.preprocess_superpixels(torch.from_numpy(labs[b]).long(), None)
        K = pp['K']
        seg_new = pp['inv_perm'][torch.from_numpy(labs[b]).long().reshape(-1)]
        ref = orc.pool_labelmap(fm[b].reshape(H * W, C).t().contiguous(), seg_new, pp['area'][pp['perm']], K)
        assert rel_err(out[b, :K], ref) < TOL
        assert float(out[b, K:].abs().max()) == 0.0
    assert torch.equal(out, ops.sp_pool_fwd(fm.to(d), m))
    for (h, w, Cs, coff) in [(H, W, 32, 0), (H // 2, W // 2, 64, 64), (H // 8, W // 8, 256, 512)]:
        sl = rnd(B, h, w, Cs, seed=9).to(d)
        fm2 = torch.zeros(B, H, W, C, device=d)
        ops.upsample_fwd(sl, fm2, coff)
        ref2 = ops.sp_pool_fwd(fm2, m)
        got = torch.zeros(B, Kmax, C, device=d)
        ops.sp_pool_upsample_fwd(sl, m, got, coff)
        assert rel_err(got[..., coff:coff + Cs], ref2[..., coff:coff + Cs]) < 1e-5


@pytest.mark.parametrize('Kmax,C,ok', [(16384, 2, True), (16384, 3, True), (16384, 4, False), (13312, 4, True), (20000, 2, False)])
def test_sp_preprocess_limits(ops, Kmax, C, ok):
    """The limits wesup_hip.h states: Kmax <= 16384 and Kmax * (2 + C) <= 81920 (round 4's form refused Kmax > 13312 with a 2-class
    mask); a map with ids up to Kmax - 1 goes through and counts right."""
    d = dev()
    H = W = 128
    rs = np.random.RandomState(3)
    labs = rs.randint(0, min(Kmax, 16384), (1, H, W)).astype(np.int32)
    labs[0, 0, 0] = min(Kmax, 16384) - 1
    mask = (rs.random_sample((1, C, H, W)) > 0.7).astype(np.uint8)
    if not ok:
        with pytest.raises(Exception):
            ops.sp_preprocess(torch.from_numpy(labs).to(d), torch.from_numpy(mask).to(d), Kmax, n_classes=C)
        return
    m = ops.sp_preprocess(torch.from_numpy(labs).to(d), torch.from_numpy(mask).to(d), Kmax, n_classes=C)
    assert int(m.n_sp[0]) == Kmax
    area = np.bincount(labs.reshape(-1), minlength=Kmax)
    perm = m.perm[0].cpu().numpy()
    assert np.array_equal(m.area_new[0].cpu().numpy(), area[perm]) and int(m.area_new.sum()) == H * W
    cnt = np.stack([np.bincount(labs.reshape(-1), weights=mask[0, c].reshape(-1), minlength=Kmax) for c in range(C)], 1)
    lab_rows = cnt.sum(1) > 0
    assert int(m.n_l[0]) == int((lab_rows & (area > 0)).sum())
    n_l = int(m.n_l[0])
    assert np.array_equal(perm[:n_l], np.nonzero(lab_rows)[0])                       # labelled ids ascending first
    want_lab = (cnt[perm[:n_l]] == cnt[perm[:n_l]].max(1, keepdims=True)).astype(np.float32)
    assert np.array_equal(m.sp_labels[0, :n_l].cpu().numpy(), want_lab)
    # the stable counting sort: pixels of a row in ascending order, rows in the reference's order
    ps, rs_ = m.pix_sorted[0].cpu().numpy(), m.row_start[0].cpu().numpy()
    flat = labs.reshape(-1)
    for r in (0, n_l, Kmax - 1):
        seg = ps[rs_[r]:rs_[r + 1]]
        assert np.array_equal(seg, np.nonzero(flat == perm[r])[0])


# ---------------------------------------------------------------- interpolation-pooling matrix (deep layers)
@pytest.mark.parametrize('B,H,W,g,h,w', [(2, 64, 64, 6, 8, 8), (1, 96, 80, 7, 12, 10), (1, 120, 120, 12, 30, 30),
                                         (1, 96, 96, 5, 96, 96 // 2)])
def test_sp_interp_matrix_equals_fused_upsample_pool(ops, B, H, W, g, h, w):
    """Wm . s == fused upsample + scatter-mean, Wm^T . g == fused pool-backward + upsample-backward, rows sum to 1."""
    d = dev()
    labs, masks = _sp_case(13, B, H, W, g)
    Kmax = (g * g + 7) // 4 * 4
    m = ops.sp_preprocess(torch.from_numpy(labs).to(d), torch.from_numpy(masks).to(d), Kmax)
    Wm = ops.sp_interp_matrix(m, h, w)
    assert torch.equal(Wm, ops.sp_interp_matrix(m, h, w))                   # order-independent accumulation
    n_sp = m.n_sp.cpu().tolist()
    C = 64
    s = rnd(B, h, w, C, seed=5).to(d)
    want = torch.zeros(B, Kmax, C, device=d)
    ops.sp_pool_upsample_fwd(s, m, want, 0)
    gup = rnd(B, Kmax, C, seed=6).to(d)
    for b in range(B):
        rows = Wm[b].sum(1).cpu()
        assert float((rows[:n_sp[b]] - 1).abs().max()) < 1e-5 and float(rows[n_sp[b]:].abs().max()) == 0.0
        got = ops.gemm_tn(ops.transpose(Wm[b]), s[b].view(h * w, C))         # (Kmax, C)
        assert rel_err(got, want[b]) < 1e-5
    want_ds = ops.upsample_bwd_fused(gup, m.new_row, m.area_new, H, W, 0, h, w, C)
    for b in range(B):
        gb = gup[b].clone()
        gb[n_sp[b]:] = 0                                                       # padded rows carry no gradient
        ds = ops.gemm_tn(Wm[b], gb)                                            # (hw, C)
        want_b = ops.upsample_bwd_fused(gb.unsqueeze(0).expand(B, -1, -1).contiguous(), m.new_row, m.area_new, H, W, 0, h, w, C)[b]
        assert rel_err(ds, want_b.view(h * w, C)) < 1e-5
    del want_ds


# ---------------------------------------------------------------- stream-K shapes of the NT family
@pytest.fixture
def streamk_on(ops):
    """The training step runs plain tiling (wesup_amd/ops.py); these tests cover the stream-K path of the kernels."""
    ops.set_streamk(True)
    yield
    ops.set_streamk(False)


@pytest.mark.parametrize('M,N,K', [(2336, 1024, 2112), (3600, 512, 4608), (14400, 512, 2304), (57600, 256, 1152),
                                   (130, 128, 1024), (66000, 128, 512)])
def test_gemm_nt_streamk(ops, lib, M, N, K, streamk_on):
    """Shapes whose last round of 128x128 tiles is partial go through the stream-K blocks + fix-up kernel."""
    d = dev()
    assert lib.load().wesup_gemm_nt_workspace_bytes(M, N, K) > 0
    A = rnd(M, K, seed=1)
    Bw = rnd(N, K, seed=2, scale=K ** -0.5)
    bias = rnd(N, seed=3)
    ref = (A.double() @ Bw.double().t() + bias.double()).float()
    out = ops.gemm_nt(A.to(d), Bw.to(d), bias.to(d))
    assert rel_err(out, ref) < TOL
    assert torch.equal(out, ops.gemm_nt(A.to(d), Bw.to(d), bias.to(d)))        # fixed summation order
    big = rnd(M, N + 64, seed=4).to(d)
    base = big.clone()
    mask = rnd(M, N, seed=5)
    ops.gemm_nt(A.to(d), Bw.to(d), None, out=big[:, 32:32 + N], mask=mask.to(d), flags=ops.ACCUM | ops.RELU_IN)
    ref2 = base.cpu()
    ref2[:, 32:32 + N] += torch.where(mask > 0, (F.relu(A).double() @ Bw.double().t()).float(), torch.zeros(()))
    assert rel_err(big, ref2) < TOL


@pytest.mark.parametrize('M,N,K', [(130, 128, 512), (14400, 256, 512), (3600, 256, 512)])
def test_gemm_nt_short_k_under_one_round_is_plain(ops, lib, M, N, K):
    """Short-K problems with fewer tiles than block slots (side convs of the deep layers) take plain smaller tiles: no
    workspace, same result."""
    d = dev()
    assert lib.load().wesup_gemm_nt_workspace_bytes(M, N, K) == 0
    A = rnd(M, K, seed=1)
    Bw = rnd(N, K, seed=2, scale=K ** -0.5)
    bias = rnd(N, seed=3)
    ref = (A.double() @ Bw.double().t() + bias.double()).float()
    out = ops.gemm_nt(A.to(d), Bw.to(d), bias.to(d))
    assert rel_err(out, ref) < TOL
    assert torch.equal(out, ops.gemm_nt(A.to(d), Bw.to(d), bias.to(d)))


@pytest.mark.parametrize('B,H,W,Cin,Cout', [(4, 30, 30, 512, 512), (2, 60, 60, 256, 512), (1, 120, 120, 128, 256)])
def test_conv3x3_streamk(ops, lib, B, H, W, Cin, Cout, streamk_on):
    d = dev()
    assert lib.load().wesup_conv3x3_workspace_bytes(B, H, W, Cin, Cout) > 0
    x = rnd(B, Cin, H, W, seed=1)
    w = rnd(Cout, Cin, 3, 3, seed=2, scale=(9 * Cin) ** -0.5)
    bias = rnd(Cout, seed=3)
    ref = F.conv2d(F.relu(x).double(), w.double(), bias.double(), padding=1).float()
    wf, wd = ops.pack_conv3x3_weight(w.to(d))
    y = ops.conv3x3_fwd(nhwc(x).to(d), wf, bias.to(d), Cout, True)
    assert rel_err(y, nhwc(ref)) < TOL
    yr = torch.empty_like(y)                        # the ReLU'd second output through the fix-up kernel
    y2 = ops.conv3x3_fwd(torch.relu(nhwc(x)).to(d), wf, bias.to(d), Cout, False, out_relu=yr)
    assert torch.equal(y2, y) and torch.equal(yr, torch.relu(y))
    dy = rnd(B, Cout, H, W, seed=4)
    refdx = F.conv_transpose2d(dy.double(), w.double(), padding=1).float()
    msk = rnd(B, Cin, H, W, seed=5)
    acc0 = rnd(B, H, W, Cin, seed=6)
    dx = acc0.clone().to(d)
    ops.conv3x3_dgrad(nhwc(dy).to(d), wd, Cin, mask_src=nhwc(msk).to(d), out=dx, accumulate=True)
    assert rel_err(dx, acc0 + nhwc(torch.where(msk > 0, refdx, torch.zeros(())))) < TOL
