"""What smirk_amd.data.BatchPreparer costs per batch on one device, against the training step it feeds.

    python bench.py --gpus 1 --workload train64 --no-also --no-roofline --cpu-faces 0 > step.json       # the yardstick: same box, same session
    python tools/data_prep_times.py [--step-json step.json] [batches] > profiles/data_prep_times.txt

Two batches of 64 decoded uint8 frames: 64 x 1024 x 1024 (FFHQ's size) and a mixed-size batch (256^2 .. 1024^2, landscape and portrait), each on the training
path (default AugmentConfig) and on the deterministic path.  Frames are seeded random bytes, landmarks are tests/data_law.synth_landmarks.  Per case:
    kernels   per-kernel durations of ONE batch from smirk_profile_start / smirk_profile_stop (events around every launch; a run of its own)
    host      perf_counter of validation + packing into the pinned buffers (numpy; no device work)
    device    HIP events on the stream from before the two H2D copies to after the last kernel, median over the batches
    wall      perf_counter from the call to torch.cuda.synchronize(): host + device, nothing overlapped
    run()     steady-state seconds per batch of prep.run over the same samples, the H2D of batch i + 1 on the copy-in stream
and, with --step-json, each as a fraction of the train64 step measured by bench.py in the same session.  Bytes: the packed frames (H2D) and what the kernels
move at least (frames read once by the crop is an upper bound: only the box is sampled; S^2-sized stages read + written once each).
The reference's CPU chain (cv2 / skimage / albumentations) is not installed and is not timed: no speed-up against it is stated.
"""
import json
import os
import sys
import time

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.join(REPO, "tests"))
import numpy as np
import torch

import data_law as LAW
import synthdata
from smirk_amd import _lib as L, data
from smirk_amd.masking import PhiloxStream

args = sys.argv[1:]
step_ms = None
if "--step-json" in args:
    i = args.index("--step-json")
    for line in open(args[i + 1]):
        line = line.strip()
        if line.startswith("{") and "ms_per_step" in line:
            step_ms = float(json.loads(line)["ms_per_step"])
    del args[i:i + 2]
BATCHES = int(args[0]) if args else 12
N, S, WARMUP = 64, 224, 3
assert torch.cuda.is_available(), "data_prep_times.py measures on the MI355X; there is no CPU path"
dev = torch.device("cuda", 0)
idx = np.asarray(synthdata.load_bundle()["mp_landmark_indices"]).astype(np.int64).ravel()
MIXED = ((256, 256), (480, 640), (720, 1280), (1024, 1024), (640, 480), (512, 384), (1080, 810), (300, 211))


def make_batch(sizes, seed):
    r = np.random.default_rng(seed)
    frames, fans, mps = [], [], []
    for i in range(N):
        H, W = sizes[i % len(sizes)]
        frames.append(r.integers(0, 256, (H, W, 3), dtype=np.uint8))
        fan, mp = LAW.synth_landmarks(H, W, seed + i)
        fans.append(None if i % 16 == 5 else fan)
        mps.append(mp)
    return frames, fans, mps


def fraction(ms):
    return "" if step_ms is None else f"  = {ms / step_ms:6.1%} of the train64 step"


def measure(name, sizes, test):
    frames, fans, mps = make_batch(sizes, 7)
    prep = data.BatchPreparer(image_size=S, scale=1.6 if test else (1.2, 1.8), test=test, mp_indices=idx)
    rng = PhiloxStream(1, 0)
    for _ in range(WARMUP):
        prep(frames, fans, mps, rng=rng)
    torch.cuda.synchronize()
    h2d = sum(f.size for f in frames)
    print(f"\n== {name}, {'deterministic' if test else 'training'} path: N = {N}, S = {S}, packed frames {h2d / 1e6:.1f} MB ==")
    # per-kernel durations (their own run: the profiler brackets every launch with events)
    L.profile_start()
    prep(frames, fans, mps, rng=rng)
    recs = L.profile_stop()
    px = N * S * S
    least = {"data_params_kernel": 0.0, "data_crop_kernel": px * 3 + N * 112 * 112 * 12 + (px * 12 if test else px * 3), "hull_mask_kernel": px * 4,
             "data_stats_kernel": px * 3, "data_colour_kernel": px * 6, "data_blur_noise_kernel": px * 6, "data_resample_kernel": px * (3 + 4 + 12 + 4)}
    total = 0.0
    for kernel, _, _, ms in recs:
        b = least.get(kernel.split("<")[0], 0.0)
        total += ms
        print(f"   {kernel:28s} {ms * 1e3:9.1f} us" + (f"   >= {b / 1e6:7.1f} MB written + read of S^2-sized data -> {b / (ms * 1e-3) / 1e12:5.2f} TB/s" if b else ""))
    print(f"   {len(recs)} launches, {total * 1e3:.1f} us in kernels" + fraction(total))
    # host / device / wall of one direct call
    host, devms, wall = [], [], []
    for _ in range(BATCHES):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        checked = prep._validate(frames, fans, mps)
        slot = prep._next_slot()
        st = prep._stage(slot, checked)
        t1 = time.perf_counter()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        cur = torch.cuda.current_stream()
        e0.record(cur)
        prep._upload(slot, st)
        slot.ev_in.record(cur)
        prep._enqueue(slot, st, rng)
        slot.ev_done.record(cur)
        slot.used = True
        e1.record(cur)
        torch.cuda.synchronize()
        t2 = time.perf_counter()
        host.append((t1 - t0) * 1e3); devms.append(e0.elapsed_time(e1)); wall.append((t2 - t0) * 1e3)
    med = lambda v: float(np.median(v))
    rng_ = lambda v: f"[{np.percentile(v, 10):.2f}, {np.percentile(v, 90):.2f}]"
    print(f"   host   validate + pack      {med(host):8.2f} ms {rng_(host)}" + fraction(med(host)))
    print(f"   device H2D + kernels        {med(devms):8.2f} ms {rng_(devms)}  ({h2d / (med(devms) * 1e-3) / 1e9:.1f} GB/s of packed frames; kernels alone {total:.2f} ms)" + fraction(med(devms)))
    print(f"   wall   call -> synchronize  {med(wall):8.2f} ms {rng_(wall)}" + fraction(med(wall)))
    # steady state of run(): the upload of batch i + 1 overlaps batch i
    samples = [(frames[i], fans[i], mps[i]) for i in range(N)] * (BATCHES + 2)
    torch.cuda.synchronize()
    t0, done = None, 0
    for k, _ in enumerate(prep.run(iter(samples), batch_size=N, rng=rng)):
        if k == 1:                                              # two batches in: the pipeline is full; from here on nothing synchronises until the end
            torch.cuda.synchronize()
            t0 = time.perf_counter()
        elif k > 1:
            done += 1
    torch.cuda.synchronize()
    per = (time.perf_counter() - t0) * 1e3 / done
    print(f"   run()  steady state / batch {per:8.2f} ms over {done} batches  ({N / (per * 1e-3):.0f} samples/s)" + fraction(per))


print(f"device: {torch.cuda.get_device_name(0)}; {BATCHES} timed batches per case after {WARMUP} warm-up batches")
print("train64 step of this session (bench.py --workload train64): " + ("not given" if step_ms is None else f"{step_ms:.2f} ms for 64 frames"))
for name, sizes in (("64 x 1024 x 1024", ((1024, 1024),)), ("mixed sizes", MIXED)):
    for test in (False, True):
        measure(name, sizes, test)
