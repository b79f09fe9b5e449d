"""What one forward + backward of smirk_amd.ExpressionLoss costs at the trainer's batch size, in ONE process on one device.

    python tools/expression_loss_times.py [windows] [calls per window] [B]          (default 5 x 4 = 20 timed calls of each path, B = 32)

B = 32 at 224 x 224, the full [3, 4, 6, 3] network, the seeded synthetic checkpoint of tests/emotion_law.py, the call of smirk_trainer.py:118-119
(metric 'l2', use_mean=False, .mean()) and its backward into `gen`.  Two paths, alternating window by window so clock and load drift hit both alike:
    HIP     ExpressionLoss.forward / backward: libsmirk_hip.so on the caller's stream
    eager   eager PyTorch-ROCm fp32 on the same parameters and inputs, built here from the module's state dict with torch.nn.functional (conv2d, batch_norm
            with the running statistics, relu, max_pool2d, avg_pool2d) and autograd: the only route to this result before the module existed
Two numbers per path, reported separately:
    host   time until forward + backward return, one sample per call
    wall   time per call of a window of back-to-back calls with ONE device synchronise at its end, one sample per window
and the peak of torch's allocator over one call.  Then the HIP path's launches timed on their own by the library's launch profiler: the launch count and the
kernel-time sum per kernel family.  No threshold is attached to any number.  Medians with the 10th-90th percentile range.  Writes
profiles/expression_loss_times.txt as well as standard output.
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

import emotion_law as EL
from smirk_amd import ExpressionLoss
from smirk_amd import _lib as L
from smirk_amd.expression_loss import launches

windows = int(sys.argv[1]) if len(sys.argv) > 1 else 5
calls = int(sys.argv[2]) if len(sys.argv) > 2 else 4
B = int(sys.argv[3]) if len(sys.argv) > 3 else 32
WARMUP, SIZE = 3, 224
lines = []


def say(s):
    print(s, flush=True)
    lines.append(s)
    os.makedirs(os.path.join(REPO, "profiles"), exist_ok=True)
    with open(os.path.join(REPO, "profiles", "expression_loss_times.txt"), "w") as fh:
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


def eager_features(sd, x):
    bn = lambda p, v: F.batch_norm(v, sd[p + ".running_mean"], sd[p + ".running_var"], sd[p + ".weight"], sd[p + ".bias"], False, 0.0, 1e-5)
    x = F.max_pool2d(F.relu(bn("backbone.bn1", F.conv2d(x, sd["backbone.conv1.weight"], None, 2, 3))), 3, 2, 1)
    for li, n in enumerate(EL.FULL):
        for i in range(n):
            p = f"backbone.layer{li + 1}.{i}"
            stride = 2 if (i == 0 and li > 0) else 1
            y = F.relu(bn(p + ".bn1", F.conv2d(x, sd[p + ".conv1.weight"])))
            y = F.relu(bn(p + ".bn2", F.conv2d(y, sd[p + ".conv2.weight"], None, stride, 1)))
            y = bn(p + ".bn3", F.conv2d(y, sd[p + ".conv3.weight"]))
            r = bn(p + ".downsample.1", F.conv2d(x, sd[p + ".downsample.0.weight"], None, stride)) if i == 0 else x
            x = F.relu(y + r)
    return F.avg_pool2d(x, 7).flatten(1)


say(f"# {torch.cuda.get_device_name(0)}; ExpressionLoss forward + backward, layers {EL.FULL}, B = {B} at {SIZE} x {SIZE}; {windows} windows x {calls} calls per path after "
    f"{WARMUP} warm-up calls; median [p10 .. p90]")
m = ExpressionLoss(EL.synth_checkpoint(EL.FULL, 2)).cuda()
sd = {k: v for k, v in m.state_dict().items()}
gen = EL.synth_images(B, SIZE, SIZE, 2).cuda().requires_grad_(True)
tar = EL.synth_images(B, SIZE, SIZE, 102).cuda()
result = {}


def hip():
    gen.grad = None
    loss = m(gen, tar, metric="l2", use_mean=False).mean()
    loss.backward()
    result["HIP  "] = (loss.detach(), gen.grad)


def eager():
    gen.grad = None
    loss = ((eager_features(sd, gen) - eager_features(sd, tar)) ** 2).mean(dim=1).mean()
    loss.backward()
    result["eager"] = (loss.detach(), gen.grad)


paths = {"HIP  ": hip, "eager": eager}
peak = {}
for n, fn in paths.items():
    for _ in range(WARMUP):
        fn()
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    base = torch.cuda.memory_allocated()
    fn()
    torch.cuda.synchronize()
    peak[n] = (torch.cuda.max_memory_allocated() - base) / 2 ** 20
(lh, gh), (le, ge) = result["HIP  "], result["eager"]
say(f"  loss HIP {float(lh):.6g}, eager {float(le):.6g}; largest |HIP - eager| over d loss / d gen: {float((gh - ge).abs().max()):.3g} of max |grad| {float(ge.abs().max()):.3g}")
host = {n: [] for n in paths}
wall = {n: [] for n in paths}
for _ in range(windows):
    for n, fn in paths.items():
        h, w = window(fn)
        host[n] += h
        wall[n].append(w)
for n in paths:
    say(f"  {n}  host {stats(host[n])}   wall {stats(wall[n])}   {B / np.median(wall[n]):8.0f} images/s   peak memory above the inputs {peak[n]:8.0f} MiB")
say(f"  ratio of medians eager / HIP: host {np.median(host['eager']) / np.median(host['HIP  ']):.2f}x, wall {np.median(wall['eager']) / np.median(wall['HIP  ']):.2f}x")

L.profile_start()
for _ in range(calls):
    hip()
torch.cuda.synchronize()
per, order = {}, []
for name, flop, nbytes, ms in L.profile_stop():
    if name not in per:
        order.append(name)
    per.setdefault(name, []).append((ms, flop, nbytes))
total = sum(sum(t for t, _, _ in v) for v in per.values()) / calls
say(f"HIP: {sum(len(v) for v in per.values()) // calls} library launches per call (documented: {sum(launches(EL.FULL))}), sum of the kernels between their events "
    f"{total:.2f} ms per call")
for name in order:
    v = per[name]
    ms = np.asarray([t for t, _, _ in v])
    flop, nbytes = sum(f for _, f, _ in v), sum(b for _, _, b in v)
    mfma = name.startswith("conv") or name == "emotion_stem_kernel"
    rate = f", {flop / (ms.sum() * 1e-3) / 1e12:6.1f} TFLOP/s algorithmic" if mfma else f", {nbytes / (ms.sum() * 1e-3) / 1e12:5.2f} TB/s algorithmic"
    say(f"  {name:52s} {len(v) // calls:3d} launches per call, {ms.sum() / calls:8.3f} ms per call = {ms.sum() / calls / total * 100:4.1f} % (median launch "
        f"{np.median(ms) * 1e3:8.1f} us){rate}")
