"""What one forward of smirk_amd.MICA costs at the pre-training stage's batch size, in ONE process on one device.

    python tools/mica_times.py [windows] [calls per window]          (default 5 x 4 = 20 timed calls of each path)

B = 32 (configs/config_pretrain.yaml) at 112 x 112, the full [3, 13, 30, 3] network, the seeded synthetic checkpoint of tests/mica_law.py.  Two paths, alternating
window by window so clock and load drift hit both alike:
    HIP     MICA.forward: libsmirk_hip.so on the caller's stream
    eager   the SAME module's nn layers called by eager PyTorch-ROCm under no_grad on the same inputs: the only route to this result before the module existed
Two numbers per path, reported separately:
    host   time until the call returns, one sample per call
    wall   time per call of a window of back-to-back calls with ONE device synchronise at its end, one sample per window
Then the HIP path's launches timed on their own by the library's launch profiler: the launch count, the kernel-time sum per kernel family, and the achieved
bytes/s of the fully connected kernel from its algorithmic bytes against the 6.29 TB/s a float4 copy reaches on this device.  No threshold is attached to any
number.  Medians with the 10th-90th percentile range.  Writes profiles/mica_times.txt as well as standard output.
"""
import os
import sys
import time

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.join(REPO, "tests"))
import numpy as np
import torch
import torch.nn.functional as F

import mica_law as ML
from smirk_amd import MICA
from smirk_amd import _lib as L

windows = int(sys.argv[1]) if len(sys.argv) > 1 else 5
calls = int(sys.argv[2]) if len(sys.argv) > 2 else 4
WARMUP, B, COPY_TBS = 3, 32, 6.29
lines = []


def say(s):
    print(s, flush=True)
    lines.append(s)
    os.makedirs(os.path.join(REPO, "profiles"), exist_ok=True)
    with open(os.path.join(REPO, "profiles", "mica_times.txt"), "w") as fh:
        fh.write("\n".join(lines) + "\n")


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


def eager(m, img):
    a = m.arcface
    with torch.no_grad():
        x = ((img - 0.5) / 0.5)[:, [2, 1, 0]]
        x = a.prelu(a.bn1(a.conv1(x)))
        for b in a.blocks():
            y = b.bn3(b.conv2(b.prelu(b.bn2(b.conv1(b.bn1(x))))))
            x = y + (x if b.downsample is None else b.downsample(x))
        z = F.normalize(a.features(a.fc(torch.flatten(a.bn2(x), 1))))
        for layer in m.regressor.network:
            z = F.leaky_relu(layer(z), 0.2)
        return m.regressor.output(z)


say(f"# {torch.cuda.get_device_name(0)}; MICA forward, layers {ML.FULL}, B = {B} at 112 x 112; {windows} windows x {calls} calls per path after {WARMUP} warm-up calls; "
    "median [p10 .. p90]")
m = MICA(ML.synth_checkpoint(ML.FULL, 3)).cuda()
img = ML.synth_images(B, 3).cuda()
paths = {"HIP  ": lambda: m(img)["shape_params"], "eager": lambda: eager(m, img)}
for fn in paths.values():
    for _ in range(WARMUP):
        fn()
torch.cuda.synchronize()
d = float((paths["HIP  "]() - paths["eager"]()).abs().max())
say(f"  largest |HIP - eager| over shape_params [{B}, 300]: {d:.3g}")
host = {n: [] for n in paths}
wall = {n: [] for n in paths}
for _ in range(windows):
    for n, fn in paths.items():
        h, w = window(fn)
        host[n] += h
        wall[n].append(w)
for n in paths:
    say(f"  {n}  host {stats(host[n])}   wall {stats(wall[n])}   {B / np.median(wall[n]):8.0f} faces/s")
say(f"  ratio of medians eager / HIP: host {np.median(host['eager']) / np.median(host['HIP  ']):.2f}x, wall {np.median(wall['eager']) / np.median(wall['HIP  ']):.2f}x")

L.profile_start()
for _ in range(calls):
    paths["HIP  "]()
torch.cuda.synchronize()
per, order = {}, []
for name, flop, nbytes, ms in L.profile_stop():
    if name not in per:
        order.append(name)
    per.setdefault(name, []).append((ms, flop, nbytes))
total = sum(sum(t for t, _, _ in v) for v in per.values()) / calls
say(f"HIP: {sum(len(v) for v in per.values()) // calls} library launches per call, sum of the kernels between their events {total:.2f} ms per call")
for name in order:
    v = per[name]
    ms = np.asarray([t for t, _, _ in v])
    flop, nbytes = sum(f for _, f, _ in v), sum(b for _, _, b in v)
    rate = f", {flop / (ms.sum() * 1e-3) / 1e12:6.1f} TFLOP/s algorithmic" if name.startswith("conv") else f", {nbytes / (ms.sum() * 1e-3) / 1e12:5.2f} TB/s algorithmic"
    if name == "mica_fc_kernel":
        rate += f" = {nbytes / (ms.sum() * 1e-3) / 1e12 / COPY_TBS * 100:.0f} % of the {COPY_TBS} TB/s copy figure, over {nbytes / len(v) / 1e6:.1f} MB"
    say(f"  {name:52s} {len(v) // calls:3d} launches per call, {ms.sum() / calls:8.3f} ms per call (median launch {np.median(ms) * 1e3:8.1f} us){rate}")
