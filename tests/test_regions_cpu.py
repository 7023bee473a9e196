"""CPU-side checks of the mask post-processing / challenge scoring entries (csrc/regions.hip) and of the host half of the GPU
metrics: the C ABI rejects bad arguments before any launch, the workspace queries scale, the kernels hold no scratch
instruction, and the factored float formulas of utils/metrics.py -- fed contingency tables and squared directed Hausdorff
distances computed here with numpy -- give the reference's values (tests/golden/metrics.npz) and exactly the values of the
mask-based functions.  No kernel runs."""
import ctypes
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OBJDUMP = '/opt/rocm/lib/llvm/bin/llvm-objdump'
ENTRIES = ['wesup_cc_label_workspace_bytes', 'wesup_cc_label', 'wesup_remove_small_regions_workspace_bytes',
           'wesup_remove_small_regions', 'wesup_binary_morph_workspace_bytes', 'wesup_binary_morph', 'wesup_contingency',
           'wesup_label_sort_workspace_bytes', 'wesup_label_sort', 'wesup_directed_hausdorff_sq']
KERNELS = ['rg_tile_kernel', 'rg_border_kernel', 'rg_flatten_kernel', 'rg_scan_block_sums', 'rg_scan_small', 'rg_scan_apply',
           'rg_relabel_kernel', 'rg_small_apply_kernel', 'rg_morph_kernel', 'rg_contingency_kernel', 'rg_boundary_key_kernel',
           'rg_hist_kernel', 'rg_chunk_scan_kernel', 'rg_place_kernel', 'rg_hausdorff_kernel']


@pytest.fixture(scope='module')
def lib():
    from wesup_amd import _lib
    if not os.path.exists(_lib.LIB_PATH):
        _lib.build()
    return _lib


def test_entries_are_declared_exported_and_bound(lib):
    hdr = open(os.path.join(ROOT, 'include', 'wesup_hip.h')).read()
    h = lib.load()
    nm = subprocess.run(['nm', '-D', '--defined-only', lib.LIB_PATH], capture_output=True, text=True, check=True).stdout
    exported = {line.split()[-1] for line in nm.splitlines() if line.strip()}
    for name in ENTRIES:
        assert re.search(r'\b%s\s*\(' % name, hdr), name
        assert name in lib._SIGS and hasattr(h, name) and name in exported, name
    assert h.wesup_abi_version() == 6                     # entries were only added


def test_bad_arguments_are_rejected_before_any_launch(lib):
    h = lib.load()
    buf = (ctypes.c_int32 * 64)()                         # stands in for every pointer: no entry gets as far as using it
    p = ctypes.cast(buf, ctypes.c_void_p)
    big = 1 << 30
    # null pointers
    assert h.wesup_cc_label(None, None, None, 1, 8, 8, 8, 1, None, 0, None) == -1
    assert h.wesup_remove_small_regions(None, None, 1, 8, 8, 10, None, 0, None) == -1
    assert h.wesup_binary_morph(None, None, None, 1, 8, 8, 3, 3, 2, None, 0, None) == -1
    assert h.wesup_contingency(None, None, None, None, 1, 64, 1, 1, None) == -1
    assert h.wesup_label_sort(None, None, None, None, None, None, 1, 8, 8, 1, None, 0, None) == -1
    assert h.wesup_directed_hausdorff_sq(None, None, None, None, None, None, None, 1, 8, 8, 1, 1, None) == -1
    # bad values with every pointer set
    for conn in (5, 0, 6, -8):
        assert h.wesup_cc_label(p, p, p, 1, 8, 8, conn, 1, p, big, None) == -1
    assert h.wesup_cc_label(p, p, p, 0, 8, 8, 8, 1, p, big, None) == -1
    assert h.wesup_cc_label(p, p, p, 1, 8, -8, 8, 1, p, big, None) == -1
    assert h.wesup_cc_label(p, p, p, 1, 8, 8, 8, 1, p, 16, None) == -3          # workspace too small
    assert h.wesup_remove_small_regions(p, p, 1, 0, 8, 10, p, big, None) == -1
    assert h.wesup_remove_small_regions(p, p, 1, 8, 8, -1, p, big, None) == -1
    assert h.wesup_remove_small_regions(p, p, 1, 8, 8, 10, p, 16, None) == -3
    for fh, fw in ((0, 3), (3, 0), (0, 0), (-1, 3), (40, 40)):
        assert h.wesup_binary_morph(p, ctypes.cast(ctypes.byref(buf, 128), ctypes.c_void_p), p, 1, 8, 8, fh, fw, 2, p, big, None) == -1
    q = ctypes.cast(ctypes.byref(buf, 128), ctypes.c_void_p)
    assert h.wesup_binary_morph(p, q, p, 1, 8, 8, 3, 3, 3, p, big, None) == -1                 # unknown op
    assert h.wesup_binary_morph(p, p, p, 1, 8, 8, 3, 3, 0, p, big, None) == -1                 # in place
    assert h.wesup_contingency(p, p, p, p, 1, 64, -1, 1, None) == -1
    assert h.wesup_contingency(p, p, p, p, 1, 64, 8191, 8192, None) == -1                      # more than 2^26 cells
    assert h.wesup_contingency(p, p, p, p, 0, 64, 1, 1, None) == -1
    assert h.wesup_label_sort(p, p, p, p, p, p, 1, 8, 8, -1, p, big, None) == -1
    assert h.wesup_label_sort(p, p, p, p, p, p, 1, 8, 8, 16384, p, big, None) == -1
    assert h.wesup_label_sort(p, p, p, p, p, p, 1, 8, 8, 4, p, 16, None) == -3
    assert h.wesup_directed_hausdorff_sq(p, p, p, p, p, p, p, -1, 8, 8, 1, 1, None) == -1      # P < 0
    assert h.wesup_directed_hausdorff_sq(p, p, p, p, p, p, p, 1, 8, 40000, 1, 1, None) == -1   # coordinates beyond 16 bits
    assert h.wesup_directed_hausdorff_sq(p, p, p, p, p, p, p, 1, 8, 8, -1, 1, None) == -1
    assert h.wesup_directed_hausdorff_sq(p, p, p, p, p, p, p, 0, 8, 8, 1, 1, None) == 0        # nothing to do: no launch


def test_workspace_queries_are_positive_and_grow(lib):
    h = lib.load()
    shapes = [(1, 7, 9), (1, 522, 775), (1, 1024, 1024), (3, 522, 775), (2, 2048, 2048)]        # ascending B * H * W
    for query in (lambda b, hh, w: h.wesup_cc_label_workspace_bytes(b, hh, w),
                  lambda b, hh, w: h.wesup_remove_small_regions_workspace_bytes(b, hh, w),
                  lambda b, hh, w: h.wesup_binary_morph_workspace_bytes(b, hh, w, 2),
                  lambda b, hh, w: h.wesup_label_sort_workspace_bytes(b, hh, w, 30)):
        sizes = [query(*s) for s in shapes]
        assert all(v > 0 for v in sizes) and sizes == sorted(sizes) and len(set(sizes)) == len(sizes), sizes
    assert h.wesup_cc_label_workspace_bytes(1, 522, 775) >= 2 * 522 * 775 * 4
    assert h.wesup_label_sort_workspace_bytes(1, 522, 775, 3000) > h.wesup_label_sort_workspace_bytes(1, 522, 775, 30)
    assert h.wesup_cc_label_workspace_bytes(0, 8, 8) == 0 and h.wesup_label_sort_workspace_bytes(1, 8, 8, 16384) == 0
    assert h.wesup_binary_morph_workspace_bytes(1, 8, 8, 5) == 0


def test_ops_wrappers_refuse_cpu_tensors_and_oversized_tables(lib):
    import torch
    from wesup_amd import ops
    with pytest.raises(lib.WesupHipError):
        ops.cc_label(torch.zeros(4, 4, dtype=torch.uint8))
    with pytest.raises(lib.WesupHipError):
        ops.remove_small_regions(torch.zeros(4, 4, dtype=torch.uint8))
    with pytest.raises(lib.WesupHipError):
        ops.binary_opening(torch.zeros(4, 4, dtype=torch.uint8), np.ones((3, 3)))
    assert ops.CONTINGENCY_MAX_CELLS == 1 << 26


# ------------------------------------------------------------------------------------------------ host formulas
def _table(S, G):
    nS, nG = int(S.max()), int(G.max())
    C = np.bincount((S.astype(np.int64) * (nG + 1) + G).ravel(), minlength=(nS + 1) * (nG + 1))
    return C.reshape(nS + 1, nG + 1)


def _d2(A, B):
    """max over the pixels of mask A of min over the pixels of mask B of the squared distance, in integers."""
    a, b = np.argwhere(A).astype(np.int64), np.argwhere(B).astype(np.int64)
    worst = 0
    for i in range(0, len(a), 512):
        d = ((a[i:i + 512, None, :] - b[None, :, :]) ** 2).sum(-1)
        worst = max(worst, int(d.min(1).max()))
    return worst


def _host_scores(S, G):
    """detection_f1, object_dice, object_hausdorff from the table and integer squared distances only."""
    from wesup_amd.utils import metrics as M
    Sl, Gl = M.label(S), M.label(G)
    C = _table(Sl, Gl)
    pairs = M.hausdorff_pairs(C)
    d_sg = {(s, g): _d2(Sl == s, Gl == g) for s, g in pairs}
    d_gs = {(s, g): _d2(Gl == g, Sl == s) for s, g in pairs}
    oh = M.object_hausdorff_from_table(C, d_sg, d_gs) if C.shape[0] > 1 and C.shape[1] > 1 else np.nan
    return M.detection_f1_from_table(C), M.object_dice_from_table(C), oh


def test_factored_formulas_match_the_reference_fixture(golden_dir):
    from wesup_amd.utils import metrics as M
    fx = np.load(os.path.join(golden_dir, 'metrics.npz'))
    checked = 0
    for i in range(int(fx['n'])):
        S, G, want = fx[f'S{i}'], fx[f'G{i}'], fx[f'v{i}']
        got = list(_host_scores(S, G))
        if S.any() and G.any():
            got.append(M.hausdorff_from_sq(_d2(S > 0, G > 0), _d2(G > 0, S > 0)))
        for g, w in zip(got, want):
            if np.isnan(w):
                continue
            assert abs(g - w) <= 1e-9 * max(1.0, abs(w)), (i, got, want)
            checked += 1
    assert checked >= 20


def _blobs(rs, H, W, k, rmin, rmax):
    yy, xx = np.mgrid[0:H, 0:W]
    m = np.zeros((H, W), dtype=np.uint8)
    for _ in range(k):
        cy, cx = rs.randint(0, H), rs.randint(0, W)
        ry, rx = rs.randint(rmin, rmax), rs.randint(rmin, rmax)
        m[((yy - cy) / ry) ** 2 + ((xx - cx) / rx) ** 2 <= 1.0] = 1
    return m


def test_factored_formulas_equal_the_mask_functions_on_twenty_blob_pairs():
    from wesup_amd.utils import metrics as M
    fallback = 0
    for seed in range(20):
        rs = np.random.RandomState(100 + seed)
        S = _blobs(rs, 96, 128, rs.randint(2, 7), 5, 16)
        G = np.roll(S, rs.randint(-6, 7), axis=rs.randint(0, 2)) if seed % 2 else _blobs(rs, 96, 128, rs.randint(2, 7), 5, 16)
        if seed % 5 == 0:
            G[2:8, 2:8] = 1                                  # an object that most likely overlaps nothing
        f1, od, oh = _host_scores(S, G)
        assert f1 == M.detection_f1(S, G) and od == M.object_dice(S, G), seed
        assert oh == M.object_hausdorff(S, G), seed
        C = _table(M.label(S), M.label(G))
        fallback += int((M._partner(C)[1:] == 0).any() or (M._partner(C.T)[1:] == 0).any())
    assert fallback >= 3                                     # the nearest-object branch was taken


def test_hausdorff_from_sq_is_scipys_value():
    from scipy.spatial.distance import directed_hausdorff
    from wesup_amd.utils import metrics as M
    rs = np.random.RandomState(5)
    for _ in range(10):
        A, B = rs.rand(40, 50) < 0.05, rs.rand(40, 50) < 0.05
        want = max(directed_hausdorff(np.argwhere(A), np.argwhere(B))[0], directed_hausdorff(np.argwhere(B), np.argwhere(A))[0])
        assert M.hausdorff_from_sq(_d2(A, B), _d2(B, A)) == want == M.hausdorff(A, B)


# ------------------------------------------------------------------------------------------------ machine code
@pytest.fixture(scope='module')
def region_kernels(tmp_path_factory, lib):
    """{mangled kernel name: [instruction lines]} of the kernels of csrc/regions.hip in the built library."""
    if not os.path.exists(OBJDUMP):
        pytest.skip('llvm-objdump not found')
    work = tmp_path_factory.mktemp('isa_regions')
    so = shutil.copy(lib.LIB_PATH, work / 'lib.so')
    subprocess.run([OBJDUMP, '--offloading', str(so)], cwd=work, check=True, capture_output=True)
    out = {}
    for co in sorted(work.glob('lib.so.*gfx950')):
        text = subprocess.run([OBJDUMP, '-d', str(co)], check=True, capture_output=True, text=True).stdout
        name = None
        for line in text.splitlines():
            m = re.match(r'^[0-9a-f]+ <(\S+)>:', line)
            if m:
                name = m.group(1) if any(k in m.group(1) for k in KERNELS) else None
                if name:
                    out[name] = []
            elif name and line.startswith('\t'):
                out[name].append(line.strip().split('//')[0].strip())
    return out


def test_region_kernels_hold_no_scratch(region_kernels):
    for k in KERNELS:
        assert any(k in name for name in region_kernels), f'{k} not found in the code object'
    for name, code in region_kernels.items():
        assert len(code) > 4, name
        for ins in code:
            assert not ins.split()[0].startswith('scratch_'), (name, ins)
