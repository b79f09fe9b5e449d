"""What smirk_amd.visualize costs per sheet on one device, against the host path it replaces on the same box.

    python tools/visual_times.py [B] [repeats] > profiles/visual_times.txt

One sheet of the reference's full column set at B = 64, S = 224, Ke = 1 with the landmark overlay: img (with the dots), img_mica (112 x 112, resampled),
rendered_img_base, rendered_img, the two overlap blends, rendered_img_mica_zero, rendered_img_zero, masked_1st_path, reconstructed_img, loss_img (one channel) and
the four second-path batches.  Panels are seeded random values in [0, 1], landmarks uniform in [-1, 1].
    kernels    per-launch durations from smirk_profile_start / smirk_profile_stop (events around every launch; runs of their own), median over the repeats,
               with the bytes each launch states (every source value read once, every sheet byte written once) and the bandwidth that makes
    sustained  perf_counter per sheet over `repeats` calls of render_sheet + download_sheet (launches, one device-to-host copy into the cached pinned buffer,
               one stream synchronise), and the same with save_visualizations' copy out of the pinned buffer
    host path  what the reference does with the same tensors: .detach().cpu() of every panel and landmark array (pageable memory), then the law of
               tests/visual_law.py in numpy (make_grid, blends, interleave, resample, keypoints, quantisation).  cv2 and torchvision are not installed, so this is
               the restated host arithmetic, not the reference's own libraries; its sheet is compared with the device's byte for byte.
JPEG / PNG encoding is host work in both paths and is not timed.
"""
import os
import sys
import time

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.join(REPO, "tests"))
import numpy as np
import torch

import visual_law as LAW

S, KE, STREAM_TB_S = 224, 1, (4.9, 5.9)            # the streaming rate measured for the BatchNorm kernels


def make_panels(B, device, seed=0):
    g = torch.Generator().manual_seed(seed)
    r = lambda *s: torch.rand(*s, generator=g).to(device)
    vis = {k: r(B, 3, S, S) for k in ('img', 'rendered_img_base', 'rendered_img', 'rendered_img_mica_zero', 'rendered_img_zero', 'masked_1st_path', 'reconstructed_img')}
    vis['img_mica'], vis['loss_img'] = r(B, 3, 112, 112), r(B, 1, S, S)
    vis['2nd_path'] = tuple(r(KE * B, 3, S, S) for _ in range(4))
    for key, n in (('landmarks_mp', 105), ('landmarks_mp_gt', 105), ('landmarks_fan', 68), ('landmarks_fan_gt', 68)):
        vis[key] = 2 * r(B, n, 2) - 1
    return vis


def host_path(vis):
    """the reference's route: every panel through .detach().cpu(), then the sheet in numpy"""
    t0 = time.perf_counter()
    host = {k: ([t.detach().cpu().numpy() for t in v] if isinstance(v, tuple) else v.detach().cpu().numpy()) for k, v in vis.items()}
    t1 = time.perf_counter()
    sheet = LAW.sheet(host, show_landmarks=True, Ke=KE)
    return sheet, (t1 - t0) * 1e3, (time.perf_counter() - t1) * 1e3


def main():
    from smirk_amd import _lib as L, visualize
    args = sys.argv[1:]
    B = int(args[0]) if args else 64
    repeats = int(args[1]) if len(args) > 1 else 20
    assert torch.cuda.is_available(), "visual_times.py measures on the MI355X; there is no CPU path"
    dev = torch.device("cuda", 0)
    vis = make_panels(B, dev)
    panel_bytes = sum(t.numel() * 4 for v in vis.values() for t in (v if isinstance(v, tuple) else (v,)))
    med = lambda v: float(np.median(v))
    spread = lambda v: f"[{np.percentile(v, 10):.3f}, {np.percentile(v, 90):.3f}]"
    for _ in range(3):
        sheet, H, W = visualize.render_sheet(vis, show_landmarks=True, Ke=KE)
        got = visualize.download_sheet(sheet, H, W)
    print(f"device: {torch.cuda.get_device_name(0)}; B = {B}, S = {S}, Ke = {KE}, landmarks on; sheet {H} x {W} x 3 = {H * W * 3 / 1e6:.1f} MB, "
          f"panels {panel_bytes / 1e6:.1f} MB of float32; {repeats} repeats after 3 warm-up sheets")
    # per launch: the profiler's events, runs of their own
    runs = []
    for _ in range(repeats):
        L.profile_start()
        visualize.render_sheet(vis, show_landmarks=True, Ke=KE)
        torch.cuda.synchronize()
        runs.append(L.profile_stop())
    assert all(len(r) == 3 for r in runs), [len(r) for r in runs]
    print("\n== kernels (median over the repeats) ==")
    total = 0.0
    for i in range(3):
        name, _, nbytes, _ = runs[0][i]
        ms = [r[i][3] for r in runs]
        total += med(ms)
        print(f"   {name:22s} {med(ms) * 1e3:9.1f} us {spread([m * 1e3 for m in ms])}   {nbytes / 1e6:8.2f} MB -> {nbytes / (med(ms) * 1e-3) / 1e12:5.2f} TB/s")
    sheet_ms = med([r[2][3] for r in runs])
    rate = runs[0][2][2] / (sheet_ms * 1e-3) / 1e12
    print(f"   3 launches, {total * 1e3:.1f} us in kernels; the sheet kernel at {rate:.2f} TB/s against the {STREAM_TB_S[0]}-{STREAM_TB_S[1]} TB/s of the BatchNorm "
          f"streaming kernels (DESIGN §12.2): {rate / STREAM_TB_S[0]:.0%} of the lower figure")
    # sustained: launches + pinned download + synchronise
    for name, fn in (("render_sheet + download_sheet (view of the pinned buffer)", lambda: visualize.download_sheet(*visualize.render_sheet(vis, show_landmarks=True, Ke=KE))),
                     ("save_visualizations (an array of its own)", lambda: visualize.save_visualizations(vis, show_landmarks=True, Ke=KE))):
        ts = []
        for _ in range(repeats):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            fn()
            ts.append((time.perf_counter() - t0) * 1e3)
        print(f"\n== sustained, {name} ==\n   {med(ts):8.2f} ms per sheet {spread(ts)}  ({H * W * 3 / (med(ts) * 1e-3) / 1e9:.1f} GB/s of finished sheet to the host)")
    # the host path on the same box
    copies, laws = [], []
    for _ in range(2):
        torch.cuda.synchronize()
        want, c, l = host_path(vis)
        copies.append(c); laws.append(l)
    same = bool(np.array_equal(got, want))
    print(f"\n== host path: .cpu() of every panel, then the law in numpy ==\n   copies {med(copies):9.1f} ms ({panel_bytes / (med(copies) * 1e-3) / 1e9:.1f} GB/s through pageable memory)"
          f"\n   numpy  {med(laws):9.1f} ms\n   total  {med(copies) + med(laws):9.1f} ms per sheet; sheets equal byte for byte: {same}")
    assert same


if __name__ == "__main__":
    main()
