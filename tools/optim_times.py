"""What the trainer's optimiser stage costs per step — clip_grad_norm_(generator, 0.1) plus both Adam steps (smirk_trainer.py:379-381) — eager torch against
smirk_amd.optim, in ONE process on one device, on the real parameter sets: the default SmirkGenerator (6, 3, 32, 5) and the SmirkEncoder's expression
encoder, the only trainable one under configs/config_train.yaml (optimize_expression only).  Random fp32 gradients.

    python tools/optim_times.py [steps] > profiles/optim_times.txt            (default 30 timed steps per variant after 5 warm-up steps)

Variants, alternating step by step so that clock and load drift hit all alike:
    (a) torch      torch.nn.utils.clip_grad_norm_ + torch.optim.Adam.step() x 2     the reference; the same code at every commit
    (b) in-place   smirk_amd.clip_grad_norm_ + smirk_amd.Adam.step() x 2
    (c) deferred   smirk_amd.clip_grad_norm_(defer=True) + Adam.step(grad_scale=coef)         = smirk_amd.cycle.optimiser_stage
Before every step each gradient is re-assigned as a fresh tensor, as after zero_grad() (outside the timed region).  Two numbers per variant:
    GPU    between two HIP events on the stream around the stage, one sample per step
    host   perf_counter until the stage's calls have returned (enqueue time; nothing synchronises inside)
Medians with the 10th-90th percentile range.  Launch counts: kernels that torch.profiler sees in one step of each variant.  (d): the bytes per second (c)
achieves on its algorithmic byte count — 4 B per generator gradient element for the norm, 16 B read + 12 B written per element for Adam — and that rate as
a fraction of the 6.3 TB/s this chip streams (reported, not gated).
"""
import collections
import os
import sys
import time

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
import numpy as np
import torch

import smirk_amd
from smirk_amd.cycle import optimiser_stage

steps = int(sys.argv[1]) if len(sys.argv) > 1 else 30
assert steps >= 20
WARMUP, MAX_NORM, STREAM_RATE = 5, 0.1, 6.3e12
dev = torch.device("cuda", 0)
torch.manual_seed(0)


def parameter_sets():
    gen = smirk_amd.SmirkGenerator(in_channels=6, out_channels=3, init_features=32, res_blocks=5).to(dev)
    enc = smirk_amd.SmirkEncoder().to(dev)
    return list(gen.parameters()), list(enc.expression_encoder.parameters())


def build(adam):
    gp, ep = parameter_sets()
    return gp, ep, adam(ep, lr=0.25e-3), adam(gp, lr=1e-3, betas=(0.5, 0.999))   # base_trainer.py:51, 62


def torch_stage(gp, eo, go):
    torch.nn.utils.clip_grad_norm_(gp, MAX_NORM)
    eo.step(); go.step()


def inplace_stage(gp, eo, go):
    smirk_amd.clip_grad_norm_(gp, MAX_NORM)
    eo.step(); go.step()


def deferred_stage(gp, eo, go):
    optimiser_stage(gp, eo, go, max_norm=MAX_NORM)


variants = {}
for name, adam, stage in (("(a) torch   ", torch.optim.Adam, torch_stage), ("(b) in-place", smirk_amd.Adam, inplace_stage),
                          ("(c) deferred", smirk_amd.Adam, deferred_stage)):
    gp, ep, eo, go = build(adam)
    variants[name] = (gp, ep, eo, go, stage)
n_gen, n_enc = sum(p.numel() for p in variants["(a) torch   "][0]), sum(p.numel() for p in variants["(a) torch   "][1])
n_tensors = len(variants["(a) torch   "][0]) + len(variants["(a) torch   "][1])


def fresh_gradients(gp, ep):
    for p in gp + ep:
        p.grad = torch.randn_like(p) * 1e-3


def one_step(v):
    gp, ep, eo, go, stage = v
    fresh_gradients(gp, ep)
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    a.record()
    t = time.perf_counter()
    stage(gp, eo, go)
    host = time.perf_counter() - t
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) * 1e-3, host


def stats(x):
    x = np.asarray(x) * 1e6
    return f"{np.median(x):9.1f} us  [{np.percentile(x, 10):8.1f} .. {np.percentile(x, 90):8.1f}]"


print(f"# {torch.cuda.get_device_name(0)}; torch {torch.__version__}; clip_grad_norm_(generator, {MAX_NORM}) + encoder Adam step + generator Adam step; "
      f"{n_tensors} tensors, generator {n_gen / 1e6:.2f} M + expression encoder {n_enc / 1e6:.2f} M parameters; {steps} timed steps per variant after {WARMUP} warm-up "
      f"steps; median [p10 .. p90]")
gpu, host = {n: [] for n in variants}, {n: [] for n in variants}
for i in range(WARMUP + steps):
    for n, v in variants.items():
        g, h = one_step(v)
        if i >= WARMUP:
            gpu[n].append(g); host[n].append(h)
for n in variants:
    print(f"  {n}  GPU {stats(gpu[n])}   host {stats(host[n])}")
ma, mc = np.median(gpu["(a) torch   "]), np.median(gpu["(c) deferred"])
ha, hc = np.median(host["(a) torch   "]), np.median(host["(c) deferred"])
print(f"  ratio of medians (a) / (c): GPU {ma / mc:.2f}x, host {ha / hc:.2f}x;  (a) / (b): GPU {ma / np.median(gpu['(b) in-place']):.2f}x, "
      f"host {ha / np.median(host['(b) in-place']):.2f}x")
nbytes = 4.0 * n_gen + 28.0 * (n_gen + n_enc)
print(f"  (d) algorithmic bytes of (c): {nbytes / 1e6:.1f} MB -> {nbytes / mc / 1e12:.2f} TB/s over the stage's GPU time, {nbytes / mc / STREAM_RATE:.2f} of {STREAM_RATE / 1e12:.1f} TB/s")

# launch counts: one profiled step per variant, after the timings
try:
    from torch.profiler import ProfilerActivity, profile
    for n, v in variants.items():
        gp, ep, eo, go, stage = v
        fresh_gradients(gp, ep)
        torch.cuda.synchronize()
        with profile(activities=[ProfilerActivity.CPU, ProfilerActivity.CUDA]) as prof:
            stage(gp, eo, go)
            torch.cuda.synchronize()
        ev = [e for e in prof.events() if e.device_type == torch.autograd.DeviceType.CUDA and not e.name.startswith("Optimizer.step")]       # not the step's annotation
        copies = [e for e in ev if any(w in e.name.lower() for w in ("memcpy", "memset", "copybuffer", "fillbuffer"))]       # the runtime's copy kernels included
        names = collections.Counter(e.name.replace("(anonymous namespace)::", "").split("(")[0].split("<")[0].replace("void ", "").split("::")[-1] for e in ev if e not in copies)
        print(f"  {n}  {sum(names.values())} kernel launches, {len(copies)} copy events per step: " + ", ".join(f"{k} x{v}" for k, v in names.most_common()))
except Exception as e:                                                             # the counts are a report; the timings above stand without them
    print(f"  launch counts: not measured ({type(e).__name__}: {e})")
from smirk_amd import _lib as L
gp, ep, eo, go, stage = variants["(c) deferred"]
fresh_gradients(gp, ep)
torch.cuda.synchronize()
L.profile_start()
stage(gp, eo, go)
torch.cuda.synchronize()
recs = L.profile_stop()
for name, _, _, ms in recs:
    print(f"  (c) {name:22s} {ms * 1e3:7.1f} us between its two events")
ksum = sum(r[3] for r in recs) * 1e-3
print(f"  (c) the four launches together {ksum * 1e6:.1f} us -> {nbytes / ksum / 1e12:.2f} TB/s on the algorithmic bytes, {nbytes / ksum / STREAM_RATE:.2f} of {STREAM_RATE / 1e12:.1f} TB/s; "
      f"the stage's GPU time above is bounded by the host's enqueue time, not by the kernels")
