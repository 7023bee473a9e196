"""Whole-image multi-scale pixel inference on the GPU: the two resize kernels and the per-resolution gather of
csrc/pixel.hip against torch's fp32 F.interpolate on the CPU, ``WESUPPixelInference.forward_per_resolution`` against the
oracle and against the shipped ``forward``, and the driver ``wesup_amd.pixel_infer`` against the same composition done on the
CPU.  Weights ``orc.make_weights(4, feat_scale=0.3)``, images ``synth.synth_image(seed, H, W)``; the CPU references are
computed once per shape and shared.  Every bar is recorded through tests/_tol.within."""
import functools

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import _tol

pytestmark = pytest.mark.gpu

TOL = 1e-4                  # the project's bar for this output (tests/test_step_gpu.py)
RESIZE_BAR = 1e-6           # absolute, data in [0, 1]: fewer than eight fp32 roundings of values <= 1 give < 5e-7; twice that
GATHER_BAR = 5e-6           # of the reference's maximum: six terms of at most eight roundings each
RESIZE_CASES = [((37, 53), (14, 21)), ((14, 21), (37, 53)), ((5, 7), (1, 1)), ((9, 1), (20, 3))]


def dev():
    return torch.device('cuda:0')


def rel_err(a, b):
    a = torch.as_tensor(a).detach().double().cpu()
    b = torch.as_tensor(b).detach().double().cpu()
    return float((a - b).abs().max() / (b.abs().max() + 1e-30))


def interp(x, size):
    return F.interpolate(x, size=tuple(size), mode='bilinear', align_corners=True)


@functools.lru_cache(maxsize=None)
def weights():
    from oracle import wesup_oracle as orc
    return orc.make_weights(4, feat_scale=0.3)


@functools.lru_cache(maxsize=None)
def torch_weights():
    from oracle import wesup_oracle as orc
    return orc.to_torch(weights())


@functools.lru_cache(maxsize=None)
def image(seed, H, W):
    from wesup_amd import synth
    return torch.from_numpy(synth.synth_image(seed, H, W))[None]              # (1,3,H,W) fp32


@functools.lru_cache(maxsize=None)
def image_u8(seed, H, W):
    from wesup_amd import synth
    return np.ascontiguousarray(np.round(synth.synth_image(seed, H, W) * 255).astype(np.uint8).transpose(1, 2, 0))


@functools.lru_cache(maxsize=None)
def oracle_pred(seed, H, W):
    """orc.pixel_inference of synth image ``seed`` at (H, W): (H,W,2) on the CPU, computed once and never written to."""
    from oracle import wesup_oracle as orc
    with torch.no_grad():
        return orc.pixel_inference(torch_weights(), image(seed, H, W))


def make_model():
    from wesup_amd.models.wesup import WESUPPixelInference
    m = WESUPPixelInference().to(dev())
    m.load_state_dict({k: torch.from_numpy(v) for k, v in weights().items()})
    m.eval()
    return m


@pytest.fixture(scope='module')
def model():
    return make_model()


def check_probabilities(case, out, ref):
    """out, ref (H,W,2): the 1e-4 bar, and argmax flips only where the two probabilities are within 1e-5 of each other."""
    out = out.detach().cpu()
    assert out.shape == ref.shape
    assert _tol.within(case, 'pixel_per_resolution', rel_err(out, ref), TOL, 'class probabilities, rel. to max')
    flips = out.argmax(dim=-1) != ref.argmax(dim=-1)
    assert int(flips.sum()) == 0 or float((out - ref)[flips].abs().max()) < 1e-5


# ---------------------------------------------------------------- 1. resize kernels
@pytest.mark.parametrize('src,dst', RESIZE_CASES)
def test_image_resize_matches_interpolate(src, dst):
    from wesup_amd import ops
    rs = np.random.RandomState(src[0] * 100 + dst[0])
    u8 = rs.randint(0, 256, size=(*src, 3)).astype(np.uint8)
    unit = u8.astype(np.float32) / np.float32(255)                            # u8 / 255.f
    ref = interp(torch.from_numpy(unit).permute(2, 0, 1)[None], dst)
    out = ops.image_resize_u8(torch.from_numpy(u8).to(dev()), *dst).cpu()
    assert out.shape == ref.shape == (1, 3, *dst)
    assert _tol.within(f'image {src}->{dst}', 'pixel_resize', float((out - ref).abs().max()), RESIZE_BAR, 'abs, data in [0,1]')


def test_image_resize_same_size_is_bit_equal():
    from wesup_amd import ops
    u8 = np.arange(256, dtype=np.uint8).repeat(3).reshape(16, 16, 3)          # every byte value
    u8 = np.ascontiguousarray(np.concatenate([u8, u8[::-1, :, ::-1]], axis=1))
    unit = torch.from_numpy(u8.astype(np.float32) / np.float32(255)).permute(2, 0, 1)[None]
    out = ops.image_resize_u8(torch.from_numpy(u8).to(dev()), *u8.shape[:2]).cpu()
    assert torch.equal(out, unit)                                             # ratio exactly 1, every weight 0 or 1


@pytest.mark.parametrize('src,dst', RESIZE_CASES)
def test_plane_resize_matches_interpolate(src, dst):
    from wesup_amd import ops
    rs = np.random.RandomState(src[1] * 100 + dst[1])
    a, b = (torch.from_numpy(rs.rand(*src).astype(np.float32)) for _ in range(2))
    ra, rb = interp(a[None, None], dst)[0, 0], interp(b[None, None], dst)[0, 0]
    out = torch.full(dst, float('nan'), device=dev())                         # accumulate=0 overwrites whatever is there
    ops.plane_resize_acc(a.to(dev()), out, alpha=1.0, accumulate=False)
    assert _tol.within(f'plane {src}->{dst}', 'pixel_resize', float((out.cpu() - ra).abs().max()), RESIZE_BAR, 'abs, data in [0,1]')
    out.fill_(float('nan'))
    ops.plane_resize_acc(a.to(dev()), out, alpha=0.5, accumulate=False)
    ops.plane_resize_acc(b.to(dev()), out, alpha=0.5, accumulate=True)
    mean = (ra + rb) / 2
    assert _tol.within(f'plane mean {src}->{dst}', 'pixel_resize', float((out.cpu() - mean).abs().max()), RESIZE_BAR, 'abs, data in [0,1]')


def test_plane_resize_same_size_is_bit_equal():
    from wesup_amd import ops
    a = torch.rand(13, 22, device=dev())
    out = torch.full((13, 22), float('nan'), device=dev())
    ops.plane_resize_acc(a, out)
    assert torch.equal(out, a)


def test_plane_resize_reads_class_one_in_place():
    from wesup_amd import ops
    pred = torch.rand(14, 21, 2, device=dev())
    strided, packed = (torch.empty(37, 53, device=dev()) for _ in range(2))
    ops.plane_resize_acc(pred[..., 1], strided, alpha=0.5)
    ops.plane_resize_acc(pred[..., 1].contiguous(), packed, alpha=0.5)
    assert torch.equal(strided, packed)
    assert not torch.equal(strided, ops.plane_resize_acc(pred[..., 0], torch.empty_like(packed), alpha=0.5))


def test_resizes_keep_their_recorded_bits():
    """tests/golden/resize_bits.npz (tools/make_resize_golden.py): 19 x 23 -> 11 x 29, down on one axis and up on the other.  The
    blends are written with their roundings (bilinear.hpp) and slide.hip's kernels are bit-equal to these: the bits are pinned."""
    import os
    from wesup_amd import ops
    gold = np.load(os.path.join(os.path.dirname(__file__), 'golden', 'resize_bits.npz'))
    image_out = ops.image_resize_u8(torch.from_numpy(gold['img']).to(dev()), *gold['image_out'].shape[2:])
    assert torch.equal(image_out.cpu(), torch.from_numpy(gold['image_out']))
    plane_out = torch.from_numpy(gold['base']).to(dev())
    ops.plane_resize_acc(torch.from_numpy(gold['pred']).to(dev())[..., 1], plane_out, alpha=1 / 3, accumulate=True)
    assert torch.equal(plane_out.cpu(), torch.from_numpy(gold['plane_out']))


# ---------------------------------------------------------------- 2. the per-resolution gather
GATHER_CASES = {
    'four_levels': dict(B=2, H=19, W=27, N=64, coarse=[(9, 13), (4, 6), (2, 3), (1, 1)]),
    'one_row_deep_map': dict(B=2, H=24, W=40, N=64, coarse=[(12, 20), (1, 2)]),          # what a 24-row image produces
}


@functools.lru_cache(maxsize=None)
def gather_case(name):
    c = GATHER_CASES[name]
    g = torch.Generator().manual_seed(len(name))
    p0 = torch.randn(c['B'], c['H'], c['W'], c['N'], generator=g)
    bias = torch.randn(c['N'], generator=g)
    coarse = [torch.randn(c['B'], h, w, c['N'], generator=g) for h, w in c['coarse']]
    ref = bias.double() + p0.double()
    for m in coarse:                      # every level straight to (H, W), in fp32 as torch does it, summed in fp64
        ref = ref + interp(m.permute(0, 3, 1, 2), (c['H'], c['W'])).permute(0, 2, 3, 1).double()
    return p0, bias, coarse, ref.clamp_min(0)


@pytest.mark.parametrize('name', sorted(GATHER_CASES))
def test_gather_matches_fp64_sum(name):
    from wesup_amd import ops
    p0, bias, coarse, ref = gather_case(name)
    d = dev()
    p0_d, bias_d, coarse_d = p0.to(d), bias.to(d), [m.to(d) for m in coarse]
    out = ops.pixel_gather_fwd(p0_d, bias_d, coarse_d, out=torch.full_like(p0_d, float('nan')))
    assert torch.equal(p0_d.cpu(), p0)                                        # out of place: p0 untouched
    err = float((out.cpu().double() - ref).abs().max() / ref.max())
    assert _tol.within(name, 'pixel_gather', err, GATHER_BAR, 'h1, rel. to max')
    assert float(out.min()) == 0.0 and float(ref.min()) == 0.0                # the ReLU is there
    inplace = p0_d.clone()
    assert ops.pixel_gather_fwd(inplace, bias_d, coarse_d) is inplace
    assert torch.equal(inplace, out)                                          # in place and out of place: bit-equal
    alone = ops.pixel_gather_fwd(p0_d[1:].contiguous(), bias_d, [m[1:].contiguous() for m in coarse_d])
    assert torch.equal(alone[0], out[1])                                      # image 1 of the batch = the same image alone


def test_gather_without_levels_is_relu_of_sum():
    from wesup_amd import ops
    p0, bias, _, _ = gather_case('four_levels')
    out = ops.pixel_gather_fwd(p0.to(dev()), bias.to(dev()), [], out=torch.empty_like(p0, device=dev()))
    assert torch.equal(out.cpu(), torch.relu(p0 + bias))


def test_gather_level_by_level_is_another_function():
    """Why the kernel interpolates every level straight to (H, W): under align_corners=True, upsampling the coarsest map into
    the next finer one and so on is not the same map.  (CPU arithmetic; it pins the reference the kernel is held to.)"""
    _, _, coarse, _ = gather_case('four_levels')
    H, W = GATHER_CASES['four_levels']['H'], GATHER_CASES['four_levels']['W']
    nchw = [m.permute(0, 3, 1, 2) for m in coarse]
    direct = sum(interp(m, (H, W)) for m in nchw)
    chain = nchw[-1]
    for m in reversed(nchw[:-1]):
        chain = m + interp(chain, m.shape[-2:])
    chain = interp(chain, (H, W))
    assert float((chain - direct).abs().max() / direct.abs().max()) > 1e-2


# ---------------------------------------------------------------- 3. forward_per_resolution
@pytest.mark.parametrize('H,W', [(48, 80), (70, 50)])
def test_forward_per_resolution_matches_oracle_and_forward(model, H, W):
    x = image(8, H, W).to(dev())
    out = model.forward_per_resolution(x)
    assert tuple(out.shape) == (1, H, W, 2)
    out = out[0].clone()
    check_probabilities(f'{H}x{W} vs oracle', out, oracle_pred(8, H, W))
    check_probabilities(f'{H}x{W} vs forward', out, model(x).cpu())
    assert torch.equal(model.forward_per_resolution(x)[0], out)               # the reused buffers give the same numbers


def test_forward_per_resolution_batch_matches_single_images(model):
    H, W = 32, 48
    xs = torch.cat([image(8, H, W), image(9, H, W)]).to(dev())
    both = model.forward_per_resolution(xs).clone()
    assert tuple(both.shape) == (2, H, W, 2)
    assert not torch.equal(both[0], both[1])
    for i, seed in enumerate((8, 9)):
        single = model.forward_per_resolution(xs[i:i + 1])[0]
        check_probabilities(f'batch image {i} vs B=1', both[i], single.cpu())
        check_probabilities(f'batch image {i} vs oracle', both[i], oracle_pred(seed, H, W))


def test_forward_per_resolution_leaves_the_engine_alone(model):
    x = image(8, 48, 80).to(dev())
    before = model(x).clone()
    eng = model.engine
    sets, last, ctx = dict(eng._bufs), eng._last, eng.ctx
    model.forward_per_resolution(x)
    model.forward_per_resolution(image(9, 32, 48).to(dev()))
    assert dict(eng._bufs) == sets and eng._last is last and eng.ctx is ctx   # no buffer set, plan or context of forward() moved
    assert torch.equal(model(x), before)


# ---------------------------------------------------------------- 4. backbone() is the conv chain of forward()
@pytest.mark.parametrize('switches', [{}, {'conv_winograd': False}, {'plain': True}], ids=['default', 'direct', 'plain'])
def test_backbone_taps_equal_forward_taps(switches):
    """The thirteen taps of ``engine.backbone`` against those an evaluation ``engine.forward`` leaves, bit for bit: default
    switches (Winograd layers, their pooling in the output transform), every layer in the direct form (max-pool launches), and
    the plain walk.  70 x 50 pools to odd sizes (35 -> 17, 25 -> 12)."""
    from wesup_amd import ops
    m = make_model()
    m._ensure_engine()
    eng = m.engine
    for name, value in switches.items():
        assert hasattr(eng, name)
        setattr(eng, name, value)
    for B, H, W in ((2, 48, 80), (1, 70, 50)):
        x = torch.cat([image(8 + i, H, W) for i in range(B)]).to(dev())
        labels = torch.zeros(B, H, W, dtype=torch.int32, device=dev())        # one dummy superpixel per image (forward_batch)
        meta = ops.sp_preprocess(labels, None, 1, n_sp_host=[1] * B)
        with torch.no_grad():
            eng.forward(x, meta, train=False, need_paint=False)
            ys = eng.backbone(x)
        taps = eng._last.y
        assert len(ys) == len(taps) == 13
        if 'conv_winograd' in switches:
            assert not any(eng.route(B, H, W))
        for l in range(13):
            assert ys[l] is not taps[l] and ys[l].data_ptr() != taps[l].data_ptr()
            assert torch.equal(ys[l], taps[l]), f'{switches} {(B, H, W)}: tap {l} differs'


# ---------------------------------------------------------------- 5. the driver
DRIVER_CASES = {'64x96': (64, 96, (0.5, 1.0), 0.72), '80x116': (80, 116, (0.4, 0.6), 0.46)}


@functools.lru_cache(maxsize=None)
def driver_reference(name):
    """pixel_infer.py:40-53 on the CPU: fp32 F.interpolate down, orc.pixel_inference, F.interpolate of class 1 up, the mean."""
    from oracle import wesup_oracle as orc
    H, W, scales, _ = DRIVER_CASES[name]
    x = torch.from_numpy(image_u8(8, H, W).astype(np.float32) / np.float32(255)).permute(2, 0, 1)[None]
    preds = []
    with torch.no_grad():
        for s in scales:
            pred = orc.pixel_inference(torch_weights(), interp(x, (int(H * s), int(W * s))))[..., 1]
            preds.append(interp(pred[None, None], (H, W))[0, 0])
    return sum(preds) / len(preds)


@pytest.mark.parametrize('full_maps', [False, True])
@pytest.mark.parametrize('name', sorted(DRIVER_CASES))
def test_pixel_predict_matches_cpu_composition(model, name, full_maps):
    from wesup_amd import pixel_infer
    H, W, scales, mask_mean = DRIVER_CASES[name]
    ref = driver_reference(name)
    ref_mask = ref.round()
    assert 0 < float(ref_mask.mean()) < 1 and round(float(ref_mask.mean()), 2) == mask_mean      # both classes present
    prob = pixel_infer.pixel_predict(model, image_u8(8, H, W), scales, device=dev(), full_maps=full_maps)
    assert prob.shape == (H, W) and prob.dtype == np.float32
    prob = torch.from_numpy(prob)
    case = f'{name} {"full maps" if full_maps else "per resolution"}'
    assert _tol.within(case, 'pixel_predict', rel_err(prob, ref), TOL, 'mean class-1 probability, rel. to max')
    decided = (ref - 0.5).abs() >= 1e-4
    assert torch.equal(prob.round()[decided], ref_mask[decided])
    assert _tol.within(case, 'pixel_predict_undecided', float((~decided).float().mean()), 0.01, 'share of pixels within 1e-4 of 0.5')


def test_main_writes_one_png_per_image(tmp_path):
    from PIL import Image
    from wesup_amd import pixel_infer
    (tmp_path / 'data' / 'images').mkdir(parents=True)
    sizes = {'a.jpg': (40, 56), 'b.png': (33, 47)}
    for seed, (name, (H, W)) in enumerate(sizes.items()):
        Image.fromarray(image_u8(seed, H, W)).save(tmp_path / 'data' / 'images' / name)
    written = pixel_infer.main(str(tmp_path / 'data'), output_dir=tmp_path / 'out', scales=(0.5, 1.0), device='cuda:0')
    assert sorted(p.name for p in (tmp_path / 'out').iterdir()) == ['a.png', 'b.png'] == sorted(p.name for p in written)
    for name, (H, W) in sizes.items():
        with Image.open(tmp_path / 'out' / name.replace('.jpg', '.png')) as im:
            assert im.format == 'PNG'
            arr = np.asarray(im)
        assert arr.shape == (H, W) and arr.dtype == np.uint8 and set(np.unique(arr)) <= {0, 255}
