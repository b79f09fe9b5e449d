"""What smirk_amd.jpeg costs on one device, against PIL's encoder over the same arrays on the same box.

    python tools/jpeg_times.py [repeats] > profiles/jpeg_times.txt

Two workloads, both at quality 95:
    sheet   the trainer's visualisation sheet at B = 64, S = 224, Ke = 1 with the landmark overlay (one picture of about 148 MB, rendered by smirk_amd.visualize
            from seeded panels: smooth fields plus sigma = 0.03 noise, so the picture compresses like an image and not like white noise)
    grids   64 video grids of 3840 x 720 (demo_video.py with render_orig and the generator panel): a smooth field plus +-12 levels of noise per frame
For every restart interval R of RESTART_SET, in alternating windows (one call of every R per repeat, so drift hits them alike):
    kernels    per-launch durations from smirk_profile_start / smirk_profile_stop (events around every launch; runs of their own): median and p10 .. p90 over the
               repeats, the input rate of the whole encode (picture bytes over the four launches' time) and the files' bytes
    wall       perf_counter around encode_jpeg + JpegBatch.to_host() (four launches, the 8 B-byte span read-back, one pinned download of the files, one
               synchronise), profiler off
and once: PIL's Image.save(quality=95, subsampling=2) of the same arrays already on the host (the download PIL needs first is timed on its own), and its files'
bytes.  No threshold is attached to any of it.
"""
import io
import os
import sys
import time

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
import numpy as np
import torch

RESTART_SET = (1, 2, 4, 8)
QUALITY = 95
S, KE = 224, 1


def make_panels(B, device, seed=0):
    g = torch.Generator().manual_seed(seed)
    yy, xx = torch.meshgrid(torch.arange(S, dtype=torch.float32), torch.arange(S, dtype=torch.float32), indexing="ij")

    def field(n, c, s=S):
        ph = torch.rand(n, c, 1, 1, generator=g) * 6.283
        fx, fy = torch.rand(n, c, 1, 1, generator=g) * 0.08 + 0.01, torch.rand(n, c, 1, 1, generator=g) * 0.08 + 0.01
        sc = S / s
        x = 0.5 + 0.35 * torch.sin(xx[:s, :s] * sc * fx + yy[:s, :s] * sc * fy + ph) + 0.03 * torch.randn(n, c, s, s, generator=g)
        return x.clamp(0, 1).to(device)
    vis = {k: field(B, 3) for k in ('img', 'rendered_img_base', 'rendered_img', 'rendered_img_mica_zero', 'rendered_img_zero', 'masked_1st_path', 'reconstructed_img')}
    vis['img_mica'], vis['loss_img'] = field(B, 3, 112), field(B, 1)
    vis['2nd_path'] = tuple(field(KE * B, 3) for _ in range(4))
    for key, n in (('landmarks_mp', 105), ('landmarks_mp_gt', 105), ('landmarks_fan', 68), ('landmarks_fan_gt', 68)):
        vis[key] = (2 * torch.rand(B, n, 2, generator=g) - 1).to(device)
    return vis


def make_grids(n, H, W, device, seed=1):
    g = torch.Generator(device=device).manual_seed(seed)
    yy, xx = torch.meshgrid(torch.arange(H, dtype=torch.float32, device=device), torch.arange(W, dtype=torch.float32, device=device), indexing="ij")
    base = torch.stack([128 + 60 * torch.sin(xx / 37) + 50 * torch.cos(yy / 23), 128 + 80 * torch.sin(xx / 53 + yy / 41), 128 + 40 * torch.cos(xx / 19) * torch.sin(yy / 31)], -1)
    out = torch.empty(n, H, W, 3, dtype=torch.uint8, device=device)
    for i in range(n):
        out[i] = (base + torch.randint(-12, 13, (H, W, 3), generator=g, device=device) + 3 * i).clamp(0, 255).to(torch.uint8)
    return out


def measure(name, images, bgr, repeats):
    from smirk_amd import _lib as L, encode_jpeg
    med = lambda v: float(np.median(v))
    spread = lambda v: f"[{np.percentile(v, 10):.3f}, {np.percentile(v, 90):.3f}]"
    B, H, W, _ = images.shape
    nbytes = images.numel()
    print(f"\n==== {name}: {B} x {H} x {W} x 3 = {nbytes / 1e6:.1f} MB, {B * (-(-H // 16)) * (-(-W // 16))} MCUs ====")
    for R in RESTART_SET:                                             # warm-up: code objects, workspace, pinned buffer
        files = encode_jpeg(images, QUALITY, bgr, R).to_host()
    kern = {R: [] for R in RESTART_SET}
    for _ in range(repeats):
        for R in RESTART_SET:
            L.profile_start()
            encode_jpeg(images, QUALITY, bgr, R)
            torch.cuda.synchronize()
            kern[R].append(L.profile_stop())
    wall, size = {R: [] for R in RESTART_SET}, {}
    for _ in range(repeats):
        for R in RESTART_SET:
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            files = encode_jpeg(images, QUALITY, bgr, R).to_host()
            wall[R].append((time.perf_counter() - t0) * 1e3)
            size[R] = sum(len(f) for f in files)
    for R in RESTART_SET:
        runs = kern[R]
        assert all(len(r) == 4 for r in runs), [len(r) for r in runs]
        print(f"-- R = {R}: files {size[R] / 1e6:.2f} MB ({nbytes / size[R]:.1f} : 1)")
        total = [sum(rec[3] for rec in r) for r in runs]
        for i in range(4):
            ms = [r[i][3] for r in runs]
            print(f"   {runs[0][i][0].split('(')[0]:34s} {med(ms):8.3f} ms {spread(ms)}")
        print(f"   four launches                      {med(total):8.3f} ms {spread(total)}  -> {nbytes / (med(total) * 1e-3) / 1e9:.1f} GB/s of pictures in")
        print(f"   wall, encode_jpeg + to_host()      {med(wall[R]):8.3f} ms {spread(wall[R])}")
    # the host's encoder over the same arrays
    from PIL import Image
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    host = images.cpu().numpy()
    copy_ms = (time.perf_counter() - t0) * 1e3
    ts, pil_bytes = [], 0
    for _ in range(3):
        t0 = time.perf_counter()
        pil_bytes = 0
        for im in host:
            b = io.BytesIO()
            Image.fromarray(im[..., ::-1] if bgr else im).save(b, "JPEG", quality=QUALITY, subsampling=2)
            pil_bytes += b.tell()
        ts.append((time.perf_counter() - t0) * 1e3)
    print(f"-- PIL {Image.__version__ if hasattr(Image, '__version__') else ''} save(quality={QUALITY}, subsampling=2), one thread: {med(ts):.1f} ms {spread(ts)} for the {B} pictures "
          f"({nbytes / (med(ts) * 1e-3) / 1e9:.2f} GB/s), after {copy_ms:.1f} ms to bring them to pageable host memory; files {pil_bytes / 1e6:.2f} MB")
    for R in RESTART_SET:
        print(f"   R = {R}: device files are {size[R] / pil_bytes:.3f} of PIL's bytes; wall {med(ts) / med(wall[R]):.0f} x shorter than PIL alone")
    # and PIL reads what the device wrote
    im = Image.open(io.BytesIO(files[0]))
    im.load()
    err = np.abs(np.asarray(im).astype(int) - (host[0][..., ::-1] if bgr else host[0])).mean()
    print(f"   PIL decodes the first device file: size {im.size}, mean absolute error against the source {err:.3f}")


def main():
    from smirk_amd import visualize
    repeats = int(sys.argv[1]) if len(sys.argv) > 1 else 10
    assert torch.cuda.is_available(), "jpeg_times.py measures on the MI355X; there is no CPU path"
    dev = torch.device("cuda", 0)
    print(f"device: {torch.cuda.get_device_name(0)}; quality {QUALITY}; restart intervals {RESTART_SET}; {repeats} repeats in alternating windows after one warm-up each")
    sheet, H, W = visualize.render_sheet(make_panels(64, dev), show_landmarks=True, Ke=KE)
    measure("sheet", sheet[:H * W * 3].view(1, H, W, 3), True, repeats)
    del sheet
    measure("grids", make_grids(64, 720, 3840, dev), True, repeats)


if __name__ == "__main__":
    main()
