"""What the first path's perceptual term costs per call, eager torch against smirk_amd.VGGPerceptualLoss, forward plus backward, in ONE process on one device.

    python tools/vgg_loss_times.py [windows] [calls per window]          (default 5 x 4 = 20 timed calls of each path and shape)

The comparator is the reference module's forward restated in eager fp32 torch (tests/vgg_law.py vgg_law: src/losses/VGGPerceptualLoss.py:23-47, NCHW fp32
on the device's own convolution library) followed by `backward()`; the HIP path is the module and its `backward()`.  Both see the same two image batches at
B = 32 and 64, 224 x 224, with the same seeded synthetic weights (tests/vgg_law.py synth_weights), the first image requiring grad, and alternate window by
window, so clock and load drift hit both alike.  Two numbers per path, reported separately:
    host   time until the call returns (what the Python thread cannot spend enqueueing the next kernels), one sample per call
    wall   time per call of a window of back-to-back calls with ONE device synchronise at its end, one sample per window
After the windows, the kernels of the HIP path are timed on their own by the library's launch profiler (HIP events around each launch).  No threshold is
attached to any number.  Medians with the 10th-90th percentile range.  Writes profiles/vgg_loss_times.txt as well as standard output.
"""
import os
import sys
import time

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.join(REPO, "tests"))
import numpy as np
import torch

from vgg_law import synth_images, synth_weights, vgg_law
from smirk_amd import VGGPerceptualLoss
from smirk_amd import _lib as L

windows = int(sys.argv[1]) if len(sys.argv) > 1 else 5
calls = int(sys.argv[2]) if len(sys.argv) > 2 else 4
WARMUP = 3
dev = torch.device("cuda", 0)
lines = []


def say(s):
    print(s, flush=True)
    lines.append(s)


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
    x = np.asarray(x) * 1e3
    return f"{np.median(x):9.2f} ms  [{np.percentile(x, 10):8.2f} .. {np.percentile(x, 90):8.2f}]"


say(f"# {torch.cuda.get_device_name(0)}; VGG perceptual term, forward + backward; {windows} windows x {calls} calls per path and shape after {WARMUP} warm-up "
    f"calls; median [p10 .. p90]")
weights = synth_weights(1, device=dev)
vgg = VGGPerceptualLoss(synth_weights(1)).to(dev)
for B in (32, 64):
    x, y = synth_images(B, 224, 224, seed=B, device=dev)
    x.requires_grad_(True)
    out = {}

    def eager():
        x.grad = None
        loss = vgg_law(x, y, weights, (224, 224))[0]
        loss.backward()
        out["eager"] = loss.detach()

    def fused():
        x.grad = None
        loss = vgg(x, y)
        loss.backward()
        out["fused"] = loss.detach()

    paths = {"eager torch": eager, "smirk_amd  ": fused}
    for fn in paths.values():
        for _ in range(WARMUP):
            fn()
    assert abs(float(out["eager"]) - float(out["fused"])) <= 1e-5 * float(out["eager"]), out        # the two paths really compute the same loss
    host = {n: [] for n in paths}
    wall = {n: [] for n in paths}
    for _ in range(windows):
        for n, fn in paths.items():
            h, w = window(fn)
            host[n] += h
            wall[n].append(w)
    say(f"B = {B}  (two image batches [B, 3, 224, 224]; the network runs over 2B = {2 * B} images forward and B backward)")
    for n in paths:
        say(f"  {n}  host {stats(host[n])}   wall {stats(wall[n])}")
    L.profile_start()                                                                              # the library's launch profiler: HIP events around each launch
    for _ in range(calls):
        fused()
    torch.cuda.synchronize()
    per, order = {}, []
    for name, flop, nbytes, ms in L.profile_stop():
        if name not in per:
            order.append(name)
        per.setdefault(name, []).append((ms, flop, nbytes))
    total = 0.0
    for name in order:
        v = per[name]
        ms = np.asarray([t for t, _, _ in v])
        total += ms.sum() / calls
        say(f"  {name:58s} {len(v) // calls:3d} launches per call, {ms.sum() / calls:8.3f} ms per call (median launch {np.median(ms) * 1e3:8.1f} us), "
            f"{sum(f for _, f, _ in v) / calls / 1e9:8.1f} GFLOP and {sum(b for _, _, b in v) / calls / 1e6:8.1f} MB algorithmic per call")
    say(f"  sum of the kernels between their events: {total:.2f} ms per call")
    say(f"  ratio of medians eager / smirk_amd: host {np.median(host['eager torch']) / np.median(host['smirk_amd  ']):.2f}x, "
        f"wall {np.median(wall['eager torch']) / np.median(wall['smirk_amd  ']):.2f}x")
    del x, y
    torch.cuda.empty_cache()
os.makedirs(os.path.join(REPO, "profiles"), exist_ok=True)
with open(os.path.join(REPO, "profiles", "vgg_loss_times.txt"), "w") as fh:
    fh.write("\n".join(lines) + "\n")
