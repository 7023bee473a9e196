"""Host side of whole-image multi-scale pixel inference (wesup_amd/pixel_infer.py, the mirror of the reference's
pixel_infer.py): command-line parsing, output directories, target sizes, file naming, str / Path roots, and the argument
checks of the three new library entries (csrc/pixel.hip), which answer on the host before any launch.  No GPU here."""
import ctypes
import os
from pathlib import Path

import pytest


@pytest.fixture(scope='module')
def lib():
    from wesup_amd import _lib
    if not os.path.exists(_lib.LIB_PATH):
        _lib.build()
    return _lib


def test_scales_parsing():
    from wesup_amd import pixel_infer as pi
    assert pi.parse_scales('0.5,0.75') == (0.5, 0.75)
    assert pi.parse_scales('0.5') == (0.5,)
    assert pi.parse_scales(' 0.4 , 1 ') == (0.4, 1.0)
    a = pi.parse_args(['data', '-c', 'runs/x/checkpoints/ckpt.pth', '-s', '0.5,0.75'])
    assert a.scale_values == (0.5, 0.75) and a.scales == '0.5,0.75' and not a.full_maps and a.device is None
    assert pi.parse_args(['data', '-c', 'c.pth']).scale_values == (0.5,)          # pixel_infer.py:63
    assert pi.parse_args(['data', '-c', 'c.pth', '--full-maps', '--device', 'cuda:0']).full_maps
    for bad in ('', ',', '0', '-0.5', '0.5,abc'):
        with pytest.raises(ValueError):
            pi.parse_scales(bad)


def test_default_output_directories():
    from wesup_amd import pixel_infer as pi
    ckpt = 'records/20190701/checkpoints/ckpt.0100.pth'
    # main() without output_dir: pixel_infer.py:26-28
    assert pi.default_output_dir(ckpt) == Path('records/20190701/results')
    assert pi.default_output_dir(Path(ckpt)) == Path('records/20190701/results')
    # the command line without -o: pixel_infer.py:75-76 (the scales as typed, the data root's name)
    a = pi.parse_args(['data/GlaS/testA', '-c', ckpt, '-s', '0.5,0.75'])
    assert a.output_dir == Path('records/20190701/results-pixel-0.5,0.75/testA')
    assert pi.parse_args(['data/GlaS/testA/', '-c', ckpt]).output_dir == Path('records/20190701/results-pixel-0.5/testA')
    assert pi.parse_args(['data', '-c', ckpt, '-o', 'out/dir']).output_dir == Path('out/dir')
    assert pi.cli_output_dir('~/r/ckpts/c.pth', '0.4', '~/d/val') == Path.home() / 'r' / 'results-pixel-0.4' / 'val'


def test_target_sizes_truncate():
    from wesup_amd import pixel_infer as pi
    assert pi.target_size(522, 775, 0.5) == (261, 387)            # GlaS at 0.5
    assert pi.target_size(1000, 1000, 0.4) == (400, 400)          # DP2019 patches at 0.4
    assert pi.target_size(80, 116, 0.4) == (32, 46) and pi.target_size(80, 116, 0.6) == (48, 69)
    assert pi.target_size(64, 96, 1.0) == (64, 96)
    assert pi.target_size(37, 53, 0.75) == (int(37 * 0.75), int(53 * 0.75)) == (27, 39)


def test_output_naming():
    from wesup_amd import pixel_infer as pi
    assert pi.output_name('testA_1.jpg') == 'testA_1.png'
    assert pi.output_name('train_12.png') == 'train_12.png'
    assert pi.output_name('a.jpg.jpg') == 'a.png.png'             # str.replace, as the reference (pixel_infer.py:54)
    assert pi.output_name('b.bmp') == 'b.bmp'


def test_roots_as_str_and_path(tmp_path):
    from wesup_amd import pixel_infer as pi
    (tmp_path / 'images').mkdir()
    for name in ('b.jpg', 'a.jpg', 'c.png'):
        (tmp_path / 'images' / name).write_bytes(b'')
    want = [tmp_path / 'images' / n for n in ('a.jpg', 'b.jpg', 'c.png')]
    assert pi.image_paths(tmp_path) == want                       # sorted
    assert pi.image_paths(str(tmp_path)) == want                  # the reference's __main__ hands main() a str and fails on `/`
    assert pi.default_output_dir(str(tmp_path / 'ckpts' / 'c.pth')) == tmp_path / 'results'
    with pytest.raises(ValueError):
        pi.main(tmp_path)                                         # neither output_dir nor checkpoint: nowhere to write


def test_new_entries_reject_bad_arguments_on_the_host(lib):
    """Null pointers, non-positive sizes and a channel count that is no multiple of 4: WESUP_ERR_INVALID without a launch.
    The pointers are 16-byte aligned host addresses that are never dereferenced: every call below fails its check first."""
    h = lib.load()
    buf = ctypes.create_string_buffer(256)
    ok = ctypes.c_void_p((ctypes.addressof(buf) + 15) // 16 * 16)
    INVALID = -1
    # (a) wesup_image_resize_u8(img, out, H, W, h, w, stream)
    assert h.wesup_image_resize_u8(None, ok, 8, 8, 4, 4, None) == INVALID
    assert h.wesup_image_resize_u8(ok, None, 8, 8, 4, 4, None) == INVALID
    for sizes in ((0, 8, 4, 4), (8, 0, 4, 4), (8, 8, 0, 4), (8, 8, 4, 0), (-1, 8, 4, 4)):
        assert h.wesup_image_resize_u8(ok, ok, *sizes, None) == INVALID
    # (b) wesup_plane_resize_acc(in, out, h, w, H, W, stride, alpha, accumulate, stream)
    assert h.wesup_plane_resize_acc(None, ok, 4, 4, 8, 8, 1, 1.0, 0, None) == INVALID
    assert h.wesup_plane_resize_acc(ok, None, 4, 4, 8, 8, 1, 1.0, 0, None) == INVALID
    for sizes in ((0, 4, 8, 8, 1), (4, 0, 8, 8, 1), (4, 4, 0, 8, 1), (4, 4, 8, 0, 1), (4, 4, 8, 8, 0)):
        assert h.wesup_plane_resize_acc(ok, ok, *sizes, 1.0, 0, None) == INVALID
    # (c) wesup_pixel_gather_fwd(p0, bias, out, levels, n_levels, B, H, W, N, stream)
    lv = (lib.CoarseMap * 4)()
    for r in range(4):
        lv[r].p, lv[r].h, lv[r].w = ok.value, 2, 2
    assert h.wesup_pixel_gather_fwd(None, ok, ok, lv, 1, 1, 8, 8, 64, None) == INVALID
    assert h.wesup_pixel_gather_fwd(ok, None, ok, lv, 1, 1, 8, 8, 64, None) == INVALID
    assert h.wesup_pixel_gather_fwd(ok, ok, None, lv, 1, 1, 8, 8, 64, None) == INVALID
    assert h.wesup_pixel_gather_fwd(ok, ok, ok, None, 1, 1, 8, 8, 64, None) == INVALID          # levels announced, none given
    for sizes in ((0, 8, 8, 64), (1, 0, 8, 64), (1, 8, 0, 64), (1, 8, 8, 0), (1, 8, 8, 62), (1, 8, 8, 1022)):
        assert h.wesup_pixel_gather_fwd(ok, ok, ok, lv, 1, *sizes, None) == INVALID
    assert h.wesup_pixel_gather_fwd(ok, ok, ok, lv, 5, 1, 8, 8, 64, None) == INVALID             # at most four coarse maps
    assert h.wesup_pixel_gather_fwd(ok, ok, ok, lv, -1, 1, 8, 8, 64, None) == INVALID
    lv[1].p = None
    assert h.wesup_pixel_gather_fwd(ok, ok, ok, lv, 2, 1, 8, 8, 64, None) == INVALID             # a null coarse map
    lv[1].p, lv[1].h = ok.value, 0
    assert h.wesup_pixel_gather_fwd(ok, ok, ok, lv, 2, 1, 8, 8, 64, None) == INVALID             # an empty one
    assert h.wesup_abi_version() == 6                                                           # additions only


def test_wrappers_fail_loudly_without_gpu_tensors(lib):
    import torch
    from wesup_amd import ops
    with pytest.raises(lib.WesupHipError):
        ops.image_resize_u8(torch.zeros(4, 4, 3, dtype=torch.uint8), 2, 2)
    with pytest.raises(lib.WesupHipError):
        ops.plane_resize_acc(torch.zeros(2, 2), torch.zeros(4, 4))
    with pytest.raises(lib.WesupHipError):
        ops.pixel_gather_fwd(torch.zeros(1, 4, 4, 8), torch.zeros(8))
