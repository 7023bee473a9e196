"""The launch sequence around the network of the nine device-resident inference drivers (needs the GPU and the built library).

Records, per driver, the ordered names of the library entries of csrc/tiles.hip, pixel.hip, slide.hip and classmap.hip plus
``wesup_copy`` that it calls -> ``tests/golden/inference_calls.json`` (a few KB).  The drivers, their models and the filter are those
of tests/test_classmaps_gpu.py (``_inference_calls``), which holds the drivers to this recording: a refactor of infer_tile.py,
pixel_infer.py or slide.py that adds, drops or reorders a launch shows.  Recorded on the library of the commit before the drivers
were folded onto shared walkers; record again only when a change of the sequence is intended.

    python tools/make_inference_calls_golden.py [--out tests/golden/inference_calls.json]
"""
import argparse
import json
import os
import sys
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.split('\n')[0])
    ap.add_argument('--out', default=str(ROOT / 'tests' / 'golden' / 'inference_calls.json'))
    a = ap.parse_args(argv)
    sys.path.insert(0, str(ROOT))
    sys.path.insert(0, str(ROOT / 'tests'))
    import test_classmaps_gpu as cases
    calls = cases._inference_calls(cases._trainer3(), cases._pixel3())
    with open(a.out, 'w') as f:
        json.dump(calls, f, indent=1)
        f.write('\n')
    print(f'{a.out}: {os.path.getsize(a.out)} bytes, ' + ', '.join(f'{k}: {len(v)}' for k, v in calls.items()))


if __name__ == '__main__':
    main()
