"""Writes tests/golden/head_two_class_bits.json: a SHA-256 of every output tensor of the two-class head entries
(wesup_classifier_fwd, wesup_classifier_bwd, wesup_propagate, wesup_head_fwd, wesup_head_bwd + wesup_classifier_bwd_finish) on the
cases of tests/_headbits.py.  tests/test_multiclass_gpu.py recomputes the digests from the library under test and asserts equality.

The golden pins "the two-class bits did not move" against a commit that still had two-class kernels of its own: generate it with
THAT commit's library, never with the code under test --

  mkdir -p build/parent && git archive <commit> wesup_amd/csrc include | tar -x -C build/parent && make -C build/parent/wesup_amd/csrc
  WESUP_HIP_LIB=build/parent/wesup_amd/csrc/libwesup_hip.so python tools/make_head_bits_golden.py --commit <commit>

(the C ABI is the same, and only wesup_amd._lib is used, not the ops wrappers).  The header names the commit, the ROCm version and
the device.  A compiler upgrade that moves expf -- every digest of a prediction or a similarity changes at once, with the fp64
checks of tests/test_head_branches_gpu.py and tests/test_multiclass_gpu.py still passing -- regenerates the file at a commit where
those other head tests pass."""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tests'))
import torch

import _headbits
from wesup_amd import _lib

ap = argparse.ArgumentParser()
ap.add_argument('--commit', required=True, help='the commit whose library is loaded (named in the header)')
ap.add_argument('--out', default=os.path.join(ROOT, 'tests', 'golden', 'head_two_class_bits.json'))
a = ap.parse_args()

doc = {'commit': a.commit, 'rocm': torch.version.hip, 'device': torch.cuda.get_device_name(0), 'digests': _headbits.digests(_lib.load())}
os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
with open(a.out, 'w') as f:
    json.dump(doc, f, indent=1, sort_keys=True)
    f.write('\n')
print(f'{a.out}: {len(doc["digests"])} cases from {_lib.LIB_PATH} ({a.commit}), ROCm {doc["rocm"]}')
