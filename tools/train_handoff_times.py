"""A/B of the training paths' hand-off in ONE process on one box: $SMIRK_DISABLE_TRAIN_HANDOFF set and unset, alternating, at 64 frames.

    python tools/train_handoff_times.py [rounds] [iterations per window]

For Ke = 1 and Ke = 2 (64 source frames, 64 / 128 output frames):
  front        cycle.render_second_path - FLAME x2, renderer x2, the masking stage - as tools/train_phase_times.py times its "front" phase
  front+input  the same plus the generator's input step: torch.cat + the pack launch with the switch set, nothing with it unset (the packed tensor comes out of
               the masking launch)
  masking only the masking stage alone (masking.train_masked_image_packed on fixed renderer outputs)
Each window is `iterations` calls between two HIP events after a warm-up; the table gives the median and the range over the rounds.  Then the launches the
library's launch profiler sees for front+input, both ways (torch's own launches - repeats, comparisons, cat - and the memsets are not library launches: DESIGN.md
33 counts them from the code), and a bit comparison of the two ways under one PhiloxStream.
"""
import os, statistics, sys, tempfile
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
os.environ.setdefault("GPU_MAX_HW_QUEUES", "16")
import torch
import bench
from smirk_amd import _lib as L, masking as MK
from smirk_amd import cycle

SWITCH = "SMIRK_DISABLE_TRAIN_HANDOFF"
rounds = int(sys.argv[1]) if len(sys.argv) > 1 else 5
iters = int(sys.argv[2]) if len(sys.argv) > 2 else 20
args = bench.parse_args(["--workload", "train64"])
args.micro_batch = 1024
dev = torch.device("cuda", 0)
wl = bench.TrainWorkload(args, dev, 0, 1, tempfile.mkdtemp())
B = wl.B


def switch(off):
    if off:
        os.environ[SWITCH] = "1"
    else:
        os.environ.pop(SWITCH, None)


def feats_for(Ke):
    """Ke target parameter sets per source frame: the workload's augmented ones, then (Ke = 2) the plain estimates"""
    return wl.feats if Ke == 1 else {k: torch.cat([wl.feats[k], wl.enc_out[k]]) for k in wl.feats}


def front(Ke, with_input):
    r, m, p = cycle._render_second_path(wl.flame, wl.rend, wl.enc_out, feats_for(Ke), wl.img, wl.mask, wl.face_prob, MK, 0.01, 10, Ke)
    if with_input and p is None:                                  # what GeneratorTrainFunction does with cat(rendered, masked)
        x = torch.cat([r, m], 1)
        p = torch.empty(Ke * B, 224, 224, 8, device=dev)
        L.check(L.lib().smirk_pack_generator_input_split16(L.ptr(x), 6, None, 0, L.ptr(p), Ke * B, 224, 224, L.stream_ptr()))
    return r, m, p


def masking_only(Ke, fixed):
    rendered, tv_src, tv_dst = fixed
    return MK.train_masked_image_packed(wl.img, wl.mask, rendered, tv_src, wl.flame.faces_tensor, wl.face_prob, trans_verts_dst=tv_dst, Ke=Ke, rendered_rule="positive",
                                        random_mask=0.005, image_size=224)


def window(fn):
    for _ in range(3):
        fn()
    torch.cuda.synchronize()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(iters):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / iters


print(f"# training paths' hand-off, {B} source frames, 224 x 224: milliseconds per call, median [min .. max] of {rounds} windows of {iters} calls, the two ways alternating")
print(f"{'':34s} {'separate launches (switch set)':>34s} {'fused (switch unset)':>34s}")
for Ke in (1, 2):
    with torch.no_grad():
        fo = wl.flame.forward(wl.enc_out)
        tv_src = wl.rend.forward(fo['vertices'], wl.enc_out['cam'])['transformed_vertices']
        f2 = feats_for(Ke)
        ro = wl.rend.forward(wl.flame.forward(f2)['vertices'], wl.enc_out['cam'].repeat(Ke, 1))
    fixed = (ro['rendered_img'].detach(), tv_src, ro['transformed_vertices'])
    for name, fn in (("front", lambda: front(Ke, False)), ("front+input", lambda: front(Ke, True)), ("masking only", lambda: masking_only(Ke, fixed))):
        t = {True: [], False: []}
        for _ in range(rounds):
            for off in (True, False):
                switch(off)
                t[off].append(window(fn))
        cell = lambda v: f"{statistics.median(v):8.3f} [{min(v):7.3f} .. {max(v):7.3f}]"
        print(f"Ke = {Ke}  {name:26s} {cell(t[True]):>34s} {cell(t[False]):>34s}")

print("\n# launches of front+input as the library's launch profiler sees them (kernels of libsmirk_hip.so; torch's own launches and memsets are not among them)")
for Ke in (1, 2):
    for off in (True, False):
        switch(off)
        front(Ke, True); torch.cuda.synchronize()
        L.profile_start()
        front(Ke, True); torch.cuda.synchronize()
        recs = L.profile_stop()
        names = {}
        for r in recs:
            k = r[0].split("[")[0]
            names[k] = names.get(k, 0) + 1
        way = "separate" if off else "fused"
        print(f"Ke = {Ke} {way:9s} library launches {len(recs):3d}")
        masking_part = {k: v for k, v in names.items() if "masking" in k or not any(s in k for s in ("flame", "raster", "render", "lbs", "skin", "landmark", "project", "shade",
                                                                                                     "bin", "tile"))}
        print("    of them outside FLAME and the renderer: " + ", ".join(f"{k} x{v}" if v > 1 else k for k, v in masking_part.items()))

print("\n# same bits: the two ways under PhiloxStream(0x5EED, 12345)")
for Ke in (1, 2):
    with torch.no_grad():
        fo = wl.flame.forward(wl.enc_out)
        tv_src = wl.rend.forward(fo['vertices'], wl.enc_out['cam'])['transformed_vertices']
        ro = wl.rend.forward(wl.flame.forward(feats_for(Ke))['vertices'], wl.enc_out['cam'].repeat(Ke, 1))
    out = {}
    for off in (True, False):
        switch(off)
        rng = MK.PhiloxStream(0x5EED, 12345)
        out[off] = MK.train_masked_image_packed(wl.img, wl.mask, ro['rendered_img'].detach(), tv_src, wl.flame.faces_tensor, wl.face_prob,
                                                trans_verts_dst=ro['transformed_vertices'], Ke=Ke, rendered_rule="positive", random_mask=0.005, rng=rng,
                                                image_size=224)[0], rng.offset
    torch.cuda.synchronize()
    print(f"Ke = {Ke}: masked equal {torch.equal(out[True][0], out[False][0])}, stream offsets equal {out[True][1] == out[False][1]}")
switch(False)
