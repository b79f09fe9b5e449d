"""Per-launch GPU time of one MobileNetV3 backbone (the library's launch profiler around smirk_backbone_forward) + the bytes each launch must move."""
import os, sys
import torch
os.environ["SMIRK_ENCODER_SERIAL"] = "1"
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from smirk_amd import SmirkEncoder, _lib as L
import synthdata as synth
B = int(sys.argv[1]) if len(sys.argv) > 1 else 128
enc = SmirkEncoder().cuda().eval()
img = synth.synth_images(B, seed=1).cuda()
for name in ("shape_encoder", "pose_encoder"):
    bb = getattr(enc, name).encoder
    for _ in range(2): bb(img)
    torch.cuda.synchronize()
    L.profile_start()
    try:
        bb(img)
    finally:
        rec = L.profile_stop()
    print("=====", name)
    for kernel, flop, byt, ms in rec:
        print(f"{kernel:44s} {ms*1e3:8.1f} us  {byt/1e6:8.1f} MB  {byt/max(ms, 1e-6)/1e9:7.2f} TB/s  {flop/max(ms, 1e-6)/1e9:8.1f} TFLOP/s")
    print(f"total {sum(r[3] for r in rec):.3f} ms")
