"""Golden bits of the two resize kernels of csrc/pixel.hip (needs the GPU and the built library).

Records what ``ops.image_resize_u8`` and ``ops.plane_resize_acc`` give for one seeded case each -> ``tests/golden/resize_bits.npz``
(about 10 KB, inputs included).  The blends of these kernels are stated with their roundings (csrc/bilinear.hpp: ``blend_image``,
``blend_plane``) and slide.hip's kernels are held to them bit for bit; tests/test_pixel_resolution_gpu.py holds the kernels to this
recording, so a change of the blend's arithmetic -- in the source or by a compiler -- shows.  Recorded on the library of the commit
before the blends moved into bilinear.hpp; record again only when a change of the bits is intended.

    python tools/make_resize_golden.py [--out tests/golden/resize_bits.npz]
"""
import argparse
import os
import sys
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parent.parent
SRC, DST = (19, 23), (11, 29)          # down on one axis, up on the other


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.split('\n')[0])
    ap.add_argument('--out', default=str(ROOT / 'tests' / 'golden' / 'resize_bits.npz'))
    a = ap.parse_args(argv)
    sys.path.insert(0, str(ROOT))
    import torch
    from wesup_amd import ops
    dev = torch.device('cuda:0')
    rs = np.random.RandomState(1923)
    img = rs.randint(0, 256, size=(*SRC, 3)).astype(np.uint8)
    pred = rs.rand(*DST, 2).astype(np.float32)
    base = rs.rand(*SRC).astype(np.float32)
    image_out = ops.image_resize_u8(torch.from_numpy(img).to(dev), *DST)
    plane_out = torch.from_numpy(base).to(dev)
    ops.plane_resize_acc(torch.from_numpy(pred).to(dev)[..., 1], plane_out, alpha=1 / 3, accumulate=True)
    np.savez_compressed(a.out, img=img, pred=pred, base=base, image_out=image_out.cpu().numpy(), plane_out=plane_out.cpu().numpy())
    print(f'{a.out}: {os.path.getsize(a.out)} bytes')


if __name__ == '__main__':
    main()
