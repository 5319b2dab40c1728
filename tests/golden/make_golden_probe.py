#!/usr/bin/env python3
"""The recorded bytes of the attribute probe's kernels: probe_parent_bytes.json next to this script (or at the path given).

Runs on an MI355X, with the library of the commit whose bytes are to be pinned checked out and built -- the file in the tree was
written from the commit before csrc/attack.hip and csrc/adv.hip shared csrc/probe.h.  tests/probe_cases.py says what a case is and
what of it is hashed; the file holds sha256 digests only, and the torch.version.hip it was recorded under.

usage: python tests/golden/make_golden_probe.py [OUT.json]
"""
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path[:0] = [os.path.dirname(os.path.dirname(HERE)), os.path.dirname(HERE)]

if __name__ == '__main__':
    import torch

    import probe_cases as PC
    from test_gpu_attack import _train_raw
    from ultrare_amd import _native as nv
    out = {'torch_version_hip': torch.version.hip, 'device': torch.cuda.get_device_name(0),
           'cases': {PC.name(case): PC.digests(nv, _train_raw, case) for case in PC.CASES}}
    path = sys.argv[1] if len(sys.argv) > 1 else os.path.join(HERE, 'probe_parent_bytes.json')
    with open(path, 'w') as f:
        json.dump(out, f, indent=1, sort_keys=True)
        f.write('\n')
    print(f"{len(out['cases'])} cases under HIP {out['torch_version_hip']} -> {path}")
