"""What the cycle path's parameter augmentation costs per call, eager torch against smirk_amd.augment, in ONE process on one device.

    python tools/augment_times.py [windows] [calls per window]          (default 10 x 20 = 200 timed calls of each path and shape)

The comparator is the reference's block restated in eager torch (tests/augment_law.py reference_law: draws on the host, one small copy per draw and per
template row, ~150 launches); the HIP path is smirk_amd.augment_flame_params (two launches).  The two alternate window by window, so clock and load drift hit
both alike.  Two numbers per path, reported separately:
    host   time until the call returns (what the Python thread cannot spend enqueueing the next kernels), one sample per call
    wall   time per call of a window of back-to-back calls with ONE device synchronise at its end, one sample per window
Medians with the 10th-90th percentile range.
"""
import os
import sys
import time

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.join(REPO, "tests"))
import numpy as np
import torch

from augment_law import reference_law, synth_inputs, synth_templates
from smirk_amd import TemplateBank, augment_flame_params

windows = int(sys.argv[1]) if len(sys.argv) > 1 else 10
calls = int(sys.argv[2]) if len(sys.argv) > 2 else 20
WARMUP = 20
dev = torch.device("cuda", 0)
templates = synth_templates(sizes=(6, 9, 4, 12, 7, 5, 8, 10, 3, 11, 6, 9))                     # 12 classes, as many as the trainer loads per subject
bank = TemplateBank(templates).to(dev)


def window(fn):
    host = []
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(calls):
        t = time.perf_counter()
        fn()
        host.append(time.perf_counter() - t)
    torch.cuda.synchronize()
    return host, (time.perf_counter() - t0) / calls


def stats(x):
    x = np.asarray(x) * 1e6
    return f"{np.median(x):9.1f} us  [{np.percentile(x, 10):8.1f} .. {np.percentile(x, 90):8.1f}]"


print(f"# {torch.cuda.get_device_name(0)}; {windows} windows x {calls} calls per path and shape after {WARMUP} warm-up calls; median [p10 .. p90]")
for B, Ke in ((64, 1), (32, 4)):
    enc = {k: torch.from_numpy(v).to(dev) for k, v in synth_inputs(B, seed=B).items()}
    paths = {"eager torch": lambda: reference_law(enc, Ke, templates, device=dev),
             "smirk_amd  ": lambda: augment_flame_params(enc, bank, Ke=Ke)}
    for fn in paths.values():
        for _ in range(WARMUP):
            fn()
    host = {n: [] for n in paths}
    wall = {n: [] for n in paths}
    for _ in range(windows):
        for n, fn in paths.items():
            h, w = window(fn)
            host[n] += h
            wall[n].append(w)
    print(f"B = {B}, Ke = {Ke}  ({Ke * B} rows x 50 expression columns)")
    for n in paths:
        print(f"  {n}  host {stats(host[n])}   wall {stats(wall[n])}")
    print(f"  ratio of medians eager / smirk_amd: host {np.median(host['eager torch']) / np.median(host['smirk_amd  ']):.1f}x, "
          f"wall {np.median(wall['eager torch']) / np.median(wall['smirk_amd  ']):.1f}x")
