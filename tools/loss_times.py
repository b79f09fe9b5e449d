"""What the first path's loss head costs per call, eager torch against smirk_amd.FirstPathLoss, forward plus backward, in ONE process on one device.

    python tools/loss_times.py [windows] [calls per window]          (default 10 x 20 = 200 timed calls of each path and shape)

The comparator is the trainer's own block restated in eager torch (tests/loss_law.py first_path_law: smirk_trainer.py:56-154) followed by `backward()` and by
the trainer's one `.item()` per entry of `losses` (:156-157); the HIP path is FirstPathLoss, `backward()` and ONE `LossTerms.as_dict()`.  Both see the same
inputs — the tensors the modules would hand over at batch B, 224 x 224, weights of configs/config_train.yaml with the perceptual term entering through
`extra` as a ready scalar — and alternate window by window, so clock and load drift hit both alike.  Two numbers per path, reported separately:
    host   time until the call returns (what the Python thread cannot spend enqueueing the next kernels), one sample per call
    wall   time per call of a window of back-to-back calls with ONE device synchronise at its end, one sample per window
After the windows, the three kernels of the HIP path are timed on their own by the library's launch profiler (HIP events around each launch, `calls` calls).
Both paths end in a device-to-host read of the terms, so `host` includes waiting for the device in both; the eager path additionally waits at its two
data-dependent branches.  Medians with the 10th-90th percentile range.
"""
import os
import sys
import time

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.join(REPO, "tests"))
import numpy as np
import torch

from loss_law import WEIGHTS_TRAIN, first_path_law, synth_first_path_inputs
from smirk_amd import FirstPathLoss
from smirk_amd import _lib as L

windows = int(sys.argv[1]) if len(sys.argv) > 1 else 10
calls = int(sys.argv[2]) if len(sys.argv) > 2 else 20
WARMUP = 20
dev = torch.device("cuda", 0)


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


print(f"# {torch.cuda.get_device_name(0)}; forward + backward + terms to the host; {windows} windows x {calls} calls per path and shape after {WARMUP} warm-up "
      f"calls; median [p10 .. p90]")
for B in (32, 64):
    enc, lf, lm, batch, recon, _ = synth_first_path_inputs(B, seed=B, device=dev)
    leaves = [lf, lm, recon, enc["expression_params"], enc["shape_params"], enc["jaw_params"]]
    for t in leaves:
        t.requires_grad_(True)
    extra = {"perceptual_vgg_loss": torch.tensor(0.5, device=dev)}
    first = FirstPathLoss(WEIGHTS_TRAIN, optimize_shape=False, optimize_expression=True, enable_fuse_generator=True)      # configs/config_train.yaml

    def clear():
        for t in leaves:
            t.grad = None

    def eager():
        clear()
        loss, losses, _ = first_path_law(enc, lf, lm, batch, WEIGHTS_TRAIN, reconstructed_img=recon, extra=extra, optimize_shape=False)
        loss.backward()
        return {k: v.item() if isinstance(v, torch.Tensor) else v for k, v in losses.items()}                             # smirk_trainer.py:156-157

    def fused():
        clear()
        loss, terms = first(enc, lf, lm, batch, reconstructed_img=recon, extra=extra)
        loss.backward()
        return terms.as_dict()

    paths = {"eager torch": eager, "smirk_amd  ": fused}
    for fn in paths.values():
        for _ in range(WARMUP):
            fn()
    a, b = eager(), fused()
    assert list(a) == list(b) and all(abs(a[k] - b[k]) <= 1e-5 * abs(a[k]) for k in a), (a, b)      # the two paths really compute the same terms
    host = {n: [] for n in paths}
    wall = {n: [] for n in paths}
    for _ in range(windows):
        for n, fn in paths.items():
            h, w = window(fn)
            host[n] += h
            wall[n].append(w)
    print(f"B = {B}  (landmarks [B, 68, 2] / [B, 105, 2], parameters [B, 50] / [B, 300] / [B, 3], images [B, 3, 224, 224])")
    for n in paths:
        print(f"  {n}  host {stats(host[n])}   wall {stats(wall[n])}")
    L.profile_start()                                                                          # the library's launch profiler: HIP events around each launch
    for _ in range(calls):
        fused()
    torch.cuda.synchronize()
    per = {}
    for name, _, nbytes, ms in L.profile_stop():
        per.setdefault(name, []).append((ms * 1e3, nbytes))
    for name, v in per.items():
        us = np.asarray([t for t, _ in v])
        print(f"  {name:22s} {np.median(us):7.1f} us  [{np.percentile(us, 10):6.1f} .. {np.percentile(us, 90):6.1f}] per launch between its two events, "
              f"{v[0][1] / 1e6:.1f} MB algorithmic traffic, {len(v)} launches")
    print(f"  ratio of medians eager / smirk_amd: host {np.median(host['eager torch']) / np.median(host['smirk_amd  ']):.2f}x, "
          f"wall {np.median(wall['eager torch']) / np.median(wall['smirk_amd  ']):.2f}x")
