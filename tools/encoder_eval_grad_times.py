"""What the image gradient through the FROZEN encoder costs per call on the even training steps (smirk_amd/encoder_eval_grad.py), in ONE process on one device.

    python tools/encoder_eval_grad_times.py [windows] [calls per window]          (default 5 x 4 = 20 timed calls of each path)

B = 64 at 224 x 224, all three backbones, forward + backward to the image, seeded synthetic weights.  Two paths, alternating window by window so clock and load
drift hit both alike:
    train-mode   the only route to this gradient before the eval-mode path existed: the encoder in .train() with every parameter frozen
                 (batch-statistics BatchNorm, BackboneTrainFunction) — a different function of the image, the same chain of layers
    eval-mode    the sub-encoders frozen and in .eval() as utils.freeze_module leaves them (BackboneEvalGradFunction)
Two numbers per path, reported separately:
    host   time until the call returns, one sample per call
    wall   time per call of a window of back-to-back calls with ONE device synchronise at its end, one sample per window
Then the first eval-mode call after a train-mode step (it rebuilds the folded and transposed weights: the caches are dropped on train() <-> eval()), and the
kernels of the eval-mode path timed on their own by the library's launch profiler, with the achieved bandwidth of the two new kernels from their algorithmic
bytes.  No threshold is attached to any number.  Medians with the 10th-90th percentile range.  Writes profiles/encoder_eval_grad_times.txt as well as
standard output.
"""
import os
import sys
import time

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.join(REPO, "tests"))
import numpy as np
import torch

import enc_eval_law as E
from oracle import assets as A
from oracle import mobilenet_ref as M
from smirk_amd import SmirkEncoder
from smirk_amd import _lib as L

windows = int(sys.argv[1]) if len(sys.argv) > 1 else 5
calls = int(sys.argv[2]) if len(sys.argv) > 2 else 4
WARMUP, B = 3, 64
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


def encoder(mode):
    enc = SmirkEncoder(); enc.load_state_dict(esd); enc = enc.cuda().train()
    for p in enc.parameters():
        p.requires_grad_(False)
    if mode == "eval":
        for n in E.ENCODERS:
            getattr(enc, n).eval()
    return enc


say(f"# {torch.cuda.get_device_name(0)}; SmirkEncoder frozen, forward + backward to the image, B = {B} at 224 x 224; {windows} windows x {calls} calls per path "
    f"after {WARMUP} warm-up calls; median [p10 .. p90]")
esd = M.synth_encoder_state_dict()
img = A.synth_images(B, seed=900).cuda()
tgt = {k: v.cuda() for k, v in E.targets(B).items()}
mods = {"train-mode": encoder("train"), "eval-mode ": encoder("eval")}


def step(enc):
    x = img.detach().requires_grad_(True)
    (E.loss_of(enc(x), tgt) * 2.0 ** -6).backward()               # (the scale keeps every gradient far inside the split-fp16 range; times do not depend on it)
    return x.grad


paths = {n: (lambda m=m: step(m)) for n, m in mods.items()}
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
for n in paths:
    say(f"  {n}  host {stats(host[n])}   wall {stats(wall[n])}")
say(f"  ratio of medians train-mode / eval-mode: host {np.median(host['train-mode']) / np.median(host['eval-mode ']):.2f}x, "
    f"wall {np.median(wall['train-mode']) / np.median(wall['eval-mode ']):.2f}x")

# the first even-step call after a train-mode step: freeze_module's .eval() drops the folded / transposed weight caches, the call rebuilds them
first_h, first_w = [], []
enc = encoder("train")
for _ in range(3):
    for n in E.ENCODERS:
        getattr(enc, n).train()
    step(enc)
    for n in E.ENCODERS:
        getattr(enc, n).eval()
    torch.cuda.synchronize()
    t = time.perf_counter()
    step(enc)
    first_h.append(time.perf_counter() - t)
    torch.cuda.synchronize()
    first_w.append(time.perf_counter() - t)
say(f"  first eval-mode call after a train-mode step (cache rebuild), 3 samples:  host {stats(first_h)}   wall {stats(first_w)}")

for n, fn in paths.items():
    L.profile_start()
    for _ in range(calls):
        fn()
    torch.cuda.synchronize()
    per, order = {}, []
    for name, flop, nbytes, ms in L.profile_stop():
        if name not in per:
            order.append(name)
        per.setdefault(name, []).append((ms, flop, nbytes))
    total = sum(sum(t for t, _, _ in v) for v in per.values()) / calls
    say(f"{n}: {sum(len(v) for v in per.values()) // calls} library launches per call, sum of the kernels between their events {total:.2f} ms per call")
    for name in order:
        v = per[name]
        ms = np.asarray([t for t, _, _ in v])
        nbytes = sum(b for _, _, b in v)
        bw = f", {nbytes / (ms.sum() * 1e-3) / 1e12:5.2f} TB/s over {nbytes / calls / 1e6:8.1f} MB algorithmic" if ("eval_bwd" in name or "relu_scale_bwd" in name) else ""
        say(f"  {name:58s} {len(v) // calls:3d} launches per call, {ms.sum() / calls:8.3f} ms per call (median launch {np.median(ms) * 1e3:8.1f} us){bw}")
os.makedirs(os.path.join(REPO, "profiles"), exist_ok=True)
with open(os.path.join(REPO, "profiles", "encoder_eval_grad_times.txt"), "w") as fh:
    fh.write("\n".join(lines) + "\n")
