"""smirk_amd.losses on the MI355X against the float64 law of tests/loss_law.py evaluated on the same fp32 inputs.

Bounds (from the arithmetic, not from what the kernels give):
  values      relative 5e-7: the summands are non-negative, the only roundings are the fp32 difference d (2^-24 relative per summand) and the final fp32 store
              (2^-24): about 1.2e-7, with a 4x margin.  Weights are positive in these tests, so the same holds for the total.
  loss_img    absolute 2e-7 on inputs in [0, 1]: each |d| < 1 carries at most 2^-25 from the fp32 difference, the stored mean at most 2^-25 more.
  gradients   1e-6 of max|g| of the tensor: at most four fp32 roundings per element (d, the scale g * w * 2 / n, their product, the cast of the upstream
              gradient); exactly 0 outside `cols`, in unflagged rows and everywhere when no row is flagged.
Largest distances seen on one MI355X (printed by the tests): values 6.1e-08 relative, loss_img 9.9e-09, gradients 9.4e-08 of max|g|.
"""
import os

import pytest
import torch

from loss_law import (WEIGHTS_PRETRAIN, WEIGHTS_TRAIN, cycle_law, first_path_law, synth_cycle_feats, synth_first_path_inputs, term_law)

pytestmark = pytest.mark.gpu
VALUE_REL, IMG_ABS, GRAD_REL = 5e-7, 2e-7, 1e-6
seen = dict(value=0.0, loss_img=0.0, grad=0.0)


def _c():
    from smirk_amd.losses import CHUNK
    return CHUNK


def _rand(shape, seed, scale=1.0, kind="uniform"):
    g = torch.Generator().manual_seed(seed)
    return (torch.rand(shape, generator=g) if kind == "uniform" else torch.randn(shape, generator=g)) * scale


def _check_value(got, want, what):
    got, want = [float(x.detach()) if torch.is_tensor(x) else float(x) for x in (got, want)]
    if want == 0.0:
        assert got == 0.0, what
        return
    rel = abs(got - want) / abs(want)
    seen["value"] = max(seen["value"], rel)
    assert rel <= VALUE_REL, (what, got, want, rel)


def _check_grad(got, want, what):
    assert torch.isfinite(got).all(), what                                             # the buffer came pre-filled with NaN or uninitialised: written in full
    want = want.to(got.device)
    gmax = float(want.abs().max())
    zero = want == 0
    assert torch.equal(got[zero], torch.zeros_like(got[zero])), what                   # exactly 0 wherever the law's gradient is exactly 0
    if gmax == 0.0:
        return
    rel = float((got.double() - want.double()).abs().max()) / gmax
    seen["grad"] = max(seen["grad"], rel)
    assert rel <= GRAD_REL, (what, rel)


def _run_case(specs, upstream=1.0):
    """specs: [dict(kind, pred, target, flags, cols, weight, loss_img)] of CPU tensors.  Runs weighted_loss on the device and the float64 law on the host, compares
    every term, the total, every loss_img and every gradient; returns what the device produced."""
    from smirk_amd.losses import Term, weighted_loss
    dev = torch.device("cuda")
    terms, leaves64, values64, imgs64 = [], [], [], []
    for s in specs:
        pred = s["pred"].to(dev).requires_grad_(True)
        cu = lambda k: None if s.get(k) is None else s[k].to(dev)
        terms.append(Term(pred, cu("target"), flags=cu("flags"), cols=s.get("cols"), weight=s.get("weight", 1.0), kind=s.get("kind", "mse"),
                          loss_img=s.get("loss_img", False)))
        leaf = s["pred"].double().requires_grad_(True)
        v, img = term_law(s.get("kind", "mse"), leaf, s.get("target"), s.get("flags"), s.get("cols"))
        leaves64.append(leaf); values64.append(v); imgs64.append(img)
    total, values, imgs = weighted_loss(terms, return_loss_img=True)
    assert total.shape == () and total.dtype == torch.float32 and tuple(values.shape) == (len(specs),) and not values.requires_grad
    total64 = sum(float(s.get("weight", 1.0)) * v for s, v in zip(specs, values64))
    for i, (v, v64) in enumerate(zip(values.tolist(), values64)):
        _check_value(v, v64, f"term {i}")
    _check_value(total, total64, "total")
    for i, (s, img, img64) in enumerate(zip(specs, imgs, imgs64)):
        if s.get("loss_img"):
            d = float((img.double().cpu() - img64.detach()).abs().max())
            seen["loss_img"] = max(seen["loss_img"], d)
            assert img.shape == img64.shape and d <= IMG_ABS, (i, d)
        else:
            assert img is None
    (upstream * total).backward()
    if torch.is_tensor(total64) and total64.requires_grad:
        (upstream * total64).backward()
    for i, (t, leaf) in enumerate(zip(terms, leaves64)):
        want = torch.zeros_like(leaf) if leaf.grad is None else leaf.grad
        assert t.pred.grad is not None and t.pred.grad.shape == t.pred.shape
        _check_grad(t.pred.grad, want, f"gradient of term {i}")
    return total.detach(), values, imgs, [t.pred.grad for t in terms]


def _row(rows, stride, cols, seed, flags=None, target=True, weight=1.0):
    return dict(kind="mse", pred=_rand((rows, stride), seed, 1.0, "normal"), target=_rand((rows, stride), seed + 1, 1.0, "normal") if target else None,
                flags=None if flags is None else torch.tensor(flags, dtype=torch.bool), cols=cols, weight=weight)


def _image(B, C, H, W, seed, weight=1.0, loss_img=True):
    img = _rand((B, C, H, W), seed)
    return dict(kind="l1_image", pred=(img + 0.1 * _rand((B, C, H, W), seed + 1, 1.0, "normal")).clamp(0, 1), target=img, weight=weight, loss_img=loss_img)


ROW_SHAPES = [(1, 136, 34), (3, 136, 34), (5, 210, 210), (2, 50, 50), (7, 300, 300)]


@pytest.mark.parametrize("rows,stride,cols", ROW_SHAPES)
def test_row_terms(rows, stride, cols):
    _run_case([_row(rows, stride, cols, seed=rows)])
    _run_case([_row(rows, stride, cols, seed=rows + 10, target=False, weight=0.25)])             # NULL target: regularisation towards zero
    print("largest distances so far:", seen)


def test_row_terms_around_the_chunk_size():
    c = _c()
    for n in (c - 1, c, c + 1):                                                                  # participating elements: one short of a chunk, a chunk, one over
        _run_case([_row(1, n + 3, n, seed=n)])
    assert (c - 1, c, c + 1) == (9 * 455, 8 * 512, 17 * 241)                                     # the same counts through several rows, the slice narrower than the row
    for rows, cols in ((9, 455), (8, 512), (17, 241)):
        _run_case([_row(rows + 2, cols + 5, cols, seed=cols, flags=[True] * rows + [False, False])])
    print("largest distances so far:", seen)


@pytest.mark.parametrize("flags", [[True] * 5, [False] * 5, [True, False, False, False, False], [False, False, False, False, True],
                                   [True, False, True, True, False]], ids=["all", "none", "first", "last", "mixed"])
def test_flags(flags):
    total, values, _, grads = _run_case([_row(5, 136, 34, seed=3, flags=flags, weight=100.0)])
    if not any(flags):
        assert float(total) == 0.0 and float(values[0]) == 0.0 and not grads[0].any()            # the trainer's int 0, and no gradient anywhere
    keep = torch.tensor(flags, device="cuda")
    assert not grads[0][~keep].any() and not grads[0][:, 34:].any()
    assert all(bool(grads[0][i, :34].any()) for i in range(5) if flags[i])
    # uint8 flags are the same flags
    from smirk_amd.losses import Term, weighted_loss
    s = _row(5, 136, 34, seed=3, flags=flags, weight=100.0)
    t8 = weighted_loss([Term(s["pred"].cuda(), s["target"].cuda(), flags=s["flags"].to(torch.uint8).cuda() * 7, cols=34, weight=100.0)])[0]
    assert torch.equal(t8, total)


IMAGE_SHAPES = [(1, 3, 1, 1), (2, 3, 5, 7), (3, 1, 16, 16), (1, 3, 64, 65), (2, 3, 224, 224)]


@pytest.mark.parametrize("shape", IMAGE_SHAPES)
def test_image_terms(shape):
    _run_case([_image(*shape, seed=sum(shape))])
    _run_case([_image(*shape, seed=sum(shape) + 1, weight=10.0, loss_img=False)])
    print("largest distances so far:", seen)


def test_image_terms_one_pixel_over_a_chunk():
    c = _c()
    assert (c + 1) % 17 == 0 and ((c + 1) // 17) % 4 != 0 and (c + 4) % 4 == 0
    _run_case([_image(1, 3, 17, (c + 1) // 17, seed=5)])                                         # c + 1 pixels, scalar path
    _run_case([_image(1, 2, 4, (c + 4) // 4, seed=6)])                                           # one 16-byte vector over a chunk, vector path
    _run_case([_image(1, 3, 4, c // 4, seed=7)])                                                 # exactly a chunk
    print("largest distances so far:", seen)


def _first_path_specs(B, seed, H=224, W=224, flags=None):
    enc, lf, lm, batch, recon, base = synth_first_path_inputs(B, seed, H, W, flags=flags, with_base=True)
    w = WEIGHTS_TRAIN
    return [dict(kind="mse", pred=lf, target=batch["landmarks_fan"], flags=batch["flag_landmarks_fan"], cols=34, weight=w["landmark_loss"]),
            dict(kind="mse", pred=lm, target=batch["landmarks_mp"], weight=w["landmark_loss"]),
            dict(kind="mse", pred=enc["expression_params"], target=base["expression_params"], weight=w["expression_regularization"]),
            dict(kind="mse", pred=enc["shape_params"], target=None, weight=float(w["shape_regularization"])),
            dict(kind="mse", pred=enc["jaw_params"], target=base["jaw_params"], weight=w["jaw_regularization"]),
            dict(kind="l1_image", pred=recon, target=batch["img"], weight=w["reconstruction_loss"], loss_img=True)]


def test_all_first_path_terms_in_one_call():
    _run_case(_first_path_specs(5, seed=1, H=32, W=36))
    _run_case(_first_path_specs(3, seed=2, H=15, W=15, flags=[False, False, False]))
    print("largest distances so far:", seen)


def test_gradient_buffers_are_written_in_full():
    """The C entry on gradient buffers the test pre-filled with NaN: every element is written, zeros outside `cols` and in unflagged rows."""
    import ctypes as C
    from smirk_amd import _lib as L
    from smirk_amd import losses
    specs = _first_path_specs(5, seed=12, H=10, W=14, flags=[False, True, False, True, True]) + [_row(3, 40, 7, seed=2, flags=[False] * 3, weight=2.0)]
    cu = lambda x: None if x is None else x.cuda()
    terms, ops = losses._prepare([losses.Term(cu(s["pred"]), cu(s["target"]), flags=cu(s.get("flags")), cols=s.get("cols"), weight=s["weight"], kind=s["kind"])
                                  for s in specs])
    grads = [torch.full_like(p, float("nan")) for p, _, _ in ops]
    arr = losses._structs(terms, ops, [None] * len(terms), grads)
    lib = L.lib()
    ws = torch.empty(max(lib.smirk_loss_workspace_bytes(arr, len(terms)), 256), dtype=torch.uint8, device="cuda")
    g = torch.tensor([1.5], device="cuda")
    L.check(lib.smirk_loss_backward(arr, len(terms), L.ptr(g), C.c_void_p(ws.data_ptr()), ws.numel(), L.stream_ptr()))
    for i, (s, got) in enumerate(zip(specs, grads)):
        leaf = s["pred"].double().requires_grad_(True)
        v, _ = term_law(s["kind"], leaf, s.get("target"), s.get("flags"), s.get("cols"))
        if torch.is_tensor(v):
            (1.5 * s["weight"] * v).backward()
        want = torch.zeros_like(leaf) if leaf.grad is None else leaf.grad
        _check_grad(got.view(want.shape), want, f"term {i}")
    assert not grads[0][[0, 2]].any() and not grads[0].view(5, 136)[:, 34:].any() and not grads[-1].any()


def test_l1_ties():
    """A known tenth of the pixels has pred == target bit for bit in one channel: the gradient there is exactly 0 (sign(0) = 0, torch's l1_loss backward), and
    loss_img there is the mean of the other channels (a third of their sum)."""
    s = _image(2, 3, 20, 24, seed=9)
    B, C, H, W = s["pred"].shape
    pix = torch.arange(B * H * W).reshape(B, H, W)
    tie = torch.zeros(B, C, H, W, dtype=torch.bool)
    for ch in range(C):
        tie[:, ch] = (pix % 10 == 0) & ((pix // 10) % C == ch)
    assert int(tie.sum()) == B * H * W // 10
    s["pred"] = torch.where(tie, s["target"], s["pred"] + (s["pred"] == s["target"]).float() * 0.25)      # ties exactly where planted, nowhere else
    assert torch.equal(s["pred"] == s["target"], tie)
    _, _, imgs, grads = _run_case([s], upstream=2.0)
    tie = tie.cuda()
    assert not grads[0][tie].any() and bool((grads[0][~tie] != 0).all())
    d = (s["pred"].double() - s["target"].double()).abs().cuda()
    others = torch.where(tie, torch.zeros_like(d), d).sum(1, keepdim=True) / C
    at = tie.any(1, keepdim=True)
    assert float((imgs[0].double() - others)[at].abs().max()) <= IMG_ABS


def test_upstream_gradient_and_no_grad():
    from smirk_amd import _lib as L
    from smirk_amd.losses import Term, weighted_loss
    specs = _first_path_specs(3, seed=4, H=12, W=12)
    _run_case(specs, upstream=3.0)                                                               # (3 * total).backward() against 3x the float64 law
    g1 = _run_case(specs, upstream=1.0)[3]
    g3 = _run_case(specs, upstream=3.0)[3]
    for a, b in zip(g1, g3):
        assert float((b - 3 * a).abs().max()) <= GRAD_REL * float((3 * a).abs().max())
    pred = specs[1]["pred"].cuda().requires_grad_(True)
    L.profile_start()
    with torch.no_grad():
        total = weighted_loss([Term(pred, specs[1]["target"].cuda())])[0]
        _ = 3.0 * total
    names = [r[0] for r in L.profile_stop()]
    assert total.grad_fn is None and not total.requires_grad
    assert names == ["loss_partial_kernel", "loss_finalise_kernel"], names                       # two launches forward, no backward
    # only predictions that require grad get one: one backward launch, and it covers just those
    a, b = specs[1]["pred"].cuda().requires_grad_(True), specs[0]["pred"].cuda()
    total = weighted_loss([Term(a, specs[1]["target"].cuda()), Term(b, specs[0]["target"].cuda(), cols=34)])[0]
    L.profile_start()
    total.backward()
    recs = L.profile_stop()
    assert [r[0] for r in recs] == ["loss_backward_kernel"] and recs[0][2] > 0 and a.grad is not None and b.grad is None


def test_two_calls_are_bitwise_equal():
    from smirk_amd.losses import Term, weighted_loss
    specs = _first_path_specs(4, seed=6, H=64, W=66) + [_image(2, 3, 224, 224, seed=8, weight=0.5)]

    def run():
        terms = [Term(s["pred"].cuda().requires_grad_(True), None if s["target"] is None else s["target"].cuda(),
                      flags=None if s.get("flags") is None else s["flags"].cuda(), cols=s.get("cols"), weight=s["weight"], kind=s["kind"],
                      loss_img=s.get("loss_img", False)) for s in specs]
        total, values, imgs = weighted_loss(terms, return_loss_img=True)
        total.backward()
        return [total.detach(), values] + [i for i in imgs if i is not None] + [t.pred.grad for t in terms]

    first = run()
    _ = torch.rand(1 << 20, device="cuda").sum()                                                 # other work in between
    second = run()
    assert len(first) == 2 + 2 + 7 and all(torch.equal(a, b) for a, b in zip(first, second))


def test_autograd_contract():
    """The operands are saved for backward: a prediction changed in place between forward and backward raises torch's version error instead of being used
    silently; the backward is differentiable once, so a double backward raises instead of returning zeros."""
    from smirk_amd.losses import Term, weighted_loss
    leaf = torch.randn(4, 136, device="cuda", requires_grad=True)
    pred = leaf * 1.0
    total = weighted_loss([Term(pred, torch.randn(4, 136, device="cuda"), cols=34)])[0]
    pred.add_(1.0)
    with pytest.raises(RuntimeError, match="modified by an inplace operation"):
        total.backward()
    total = weighted_loss([Term(leaf, None)])[0]
    (g,) = torch.autograd.grad(total, leaf, create_graph=True)
    with pytest.raises(RuntimeError):
        g.sum().backward()


def test_offset_views_and_other_dtypes():
    """Inputs are made fp32-contiguous and 16-byte aligned on the Python side: an offset view, a strided view, a float64 prediction."""
    from smirk_amd.losses import Term, weighted_loss
    big = torch.randn(4 * 136 + 1, device="cuda")
    pred = big[1:].view(4, 136).detach().requires_grad_(True)
    assert pred.data_ptr() % 16 == 4
    tgt = torch.randn(4, 272, device="cuda")[:, ::2]
    p64 = torch.randn(4, 50, device="cuda", dtype=torch.float64, requires_grad=True)
    total, values = weighted_loss([Term(pred, tgt, cols=34), Term(p64, None, weight=2.0)])
    want0 = float(((pred.double() - tgt.double())[:, :34] ** 2).mean())
    want1 = float((p64.float().double() ** 2).mean())
    _check_value(values[0], want0, "offset view"); _check_value(values[1], want1, "float64 prediction"); _check_value(total, want0 + 2.0 * want1, "total")
    total.backward()
    assert pred.grad.shape == pred.shape and p64.grad.dtype == torch.float64
    _check_grad(p64.grad.float(), (2.0 * 2.0 * p64.detach().float().double() / p64.numel()), "float64 prediction")
    want = 2.0 * (pred.detach().double() - tgt.double()) / (4 * 34)
    want[:, 34:] = 0
    _check_grad(pred.grad, want, "offset view")


def test_no_host_synchronisation():
    """FirstPathLoss forward plus backward under torch's sync debug mode: nothing in it waits for the host.  Captured in no graph."""
    from smirk_amd import FirstPathLoss
    enc, lf, lm, batch, recon, base = synth_first_path_inputs(4, seed=11, H=64, W=64, with_base=True, device="cuda")
    leaves = [lf.requires_grad_(True), lm.requires_grad_(True), recon.requires_grad_(True)] + [v.requires_grad_(True) for v in enc.values()]
    vgg = torch.tensor(0.125, device="cuda", requires_grad=True)
    first = FirstPathLoss(WEIGHTS_TRAIN, optimize_shape=True)
    first(enc, lf, lm, batch, reconstructed_img=recon, base_output=base, extra={"perceptual_vgg_loss": vgg})[0].backward()      # warm-up: library load, workspaces
    torch.cuda.synchronize()
    prev = torch.cuda.get_sync_debug_mode()
    torch.cuda.set_sync_debug_mode("error")
    try:
        try:
            torch.ones(1, device="cuda").item()
            honoured = False
        except RuntimeError:
            honoured = True
        if honoured:
            total, terms = first(enc, lf, lm, batch, reconstructed_img=recon, base_output=base, extra={"perceptual_vgg_loss": vgg})
            total.backward()
    finally:
        torch.cuda.set_sync_debug_mode(prev)
    if not honoured:
        pytest.skip("this torch build does not honour torch.cuda.set_sync_debug_mode('error'): a probe .item() under it did not raise")
    d = terms.as_dict()                                                                           # outside the guard: ONE copy for all terms
    law, losses, loss_img = first_path_law(enc, lf, lm, batch, WEIGHTS_TRAIN, reconstructed_img=recon, base_output=base, extra={"perceptual_vgg_loss": vgg},
                                           head_dtype=torch.float64)
    assert list(d) == list(losses)                                                                # the trainer's keys in the trainer's order
    for k, v in losses.items():
        _check_value(d[k], v, k)
    assert d["emotion_loss"] == 0 and d["mica_loss"] == 0 and isinstance(d["mica_loss"], int)
    _check_value(total, law, "loss_first_path")
    assert float((terms.loss_img.double() - loss_img).abs().max()) <= IMG_ABS
    assert all(t.grad is not None for t in leaves[:3]) and vgg.grad is not None and float(vgg.grad) == 2 * 10.0        # two backward passes, weight 10


@pytest.mark.parametrize("switches", [(True, True, True), (False, True, True), (True, False, False), (False, False, False)])
def test_first_path_loss_follows_the_law(switches):
    from smirk_amd import FirstPathLoss
    for w, with_base, flags in ((WEIGHTS_TRAIN, False, None), (WEIGHTS_PRETRAIN, True, [False] * 3)):
        enc, lf, lm, batch, recon, base = synth_first_path_inputs(3, seed=21, H=20, W=22, flags=flags, with_base=with_base, device="cuda")
        extra = {"mica_loss": torch.tensor(0.75, device="cuda", requires_grad=True), "emotion_loss": torch.tensor(0.5, device="cuda")}
        leaves = dict(enc, landmarks_fan=lf, landmarks_mp=lm, recon=recon)
        for v in leaves.values():
            v.requires_grad_(True)
        total, terms = FirstPathLoss(w, *switches)(enc, lf, lm, batch, reconstructed_img=recon, base_output=base, extra=extra)
        total.backward()
        got = {k: (torch.zeros_like(v) if v.grad is None else v.grad.clone()) for k, v in leaves.items()}
        for v in leaves.values():
            v.grad = None
        law, losses, loss_img = first_path_law(enc, lf, lm, batch, w, reconstructed_img=recon, base_output=base, extra=extra, optimize_shape=switches[0],
                                               optimize_expression=switches[1], enable_fuse_generator=switches[2], head_dtype=torch.float64)
        law.backward()
        d = terms.as_dict()
        assert list(d) == list(losses)
        for k, v in losses.items():
            _check_value(d[k], v, k)
        _check_value(total, law, "loss_first_path")
        assert (terms.loss_img is None) == (loss_img is None)
        for k, v in leaves.items():
            _check_grad(got[k], torch.zeros_like(v) if v.grad is None else v.grad, k)
    print("largest distances so far:", seen)


@pytest.mark.parametrize("use_eyelids", [True, False])
@pytest.mark.parametrize("generator_frozen", [True, False])
def test_cycle_loss(use_eyelids, generator_frozen):
    from smirk_amd import cycle, losses
    recon, feats = synth_cycle_feats(6, seed=3, device="cuda")
    for v in recon.values():
        v.requires_grad_(True)
    got = losses.cycle_loss(recon, feats, use_eyelids, generator_frozen)
    got.backward()
    grads = {k: (torch.zeros_like(v) if v.grad is None else v.grad.clone()) for k, v in recon.items()}
    for v in recon.values():
        v.grad = None
    want = cycle_law(recon, feats, use_eyelids, generator_frozen, head_dtype=torch.float64)
    want.backward()
    _check_value(got, want, "cycle loss")
    eager = cycle.cycle_loss(recon, feats, use_eyelids, generator_frozen)
    dist = abs(float(got) - float(eager)) / abs(float(want))
    print(f"losses.cycle_loss against cycle.cycle_loss: {dist:.2e} relative")
    assert dist <= VALUE_REL                                                                      # equal within the value bound
    for k, v in recon.items():
        _check_grad(grads[k], torch.zeros_like(v) if v.grad is None else v.grad, k)


# ---- the whole first path -----------------------------------------------------------------------------------------------------------------------------------------
def test_whole_first_path(sandbox):
    """smirk_amd.first_path at B = 2, 224 x 224, seeded synthetic weights, modules in train mode.  The terms equal the float64 law on the module outputs it returns;
    backward reaches all three encoder backbones and the generator.  Parameter gradients: the yardstick is the eager law run twice through the same graph, once in
    fp32 and once with a float64 loss head on the fp32 module outputs; per parameter tensor, relative to max(1, max|g|), their distance says how strongly rounding
    in the loss head moves that gradient, and the fused run has to lie within 4x that distance of the float64-head run (floor 1e-6).
    The fused head's upstream gradients are the correctly rounded ones; its distance is of the same order as the eager fp32 head's all the same (see the note at the
    assertion for what it consists of).
    Seen on one MI355X: eager fp32 head at most 3.85e-04, fused head at most 2.57e-04, ratio to the bound 0.53, identically in two runs."""
    from oracle import assets as A
    from oracle import generator_ref as G
    from oracle import mobilenet_ref as M
    from smirk_amd import FLAME, FirstPathLoss, Renderer, SmirkEncoder, SmirkGenerator, masking
    from smirk_amd.first_path import first_path, forward_first_path
    cwd = os.getcwd(); os.chdir(sandbox)
    try:
        fl, rn = FLAME().cuda(), Renderer().cuda()
        prob = masking.load_probabilities_per_FLAME_triangle()
    finally:
        os.chdir(cwd)
    enc = SmirkEncoder(); enc.load_state_dict(M.synth_encoder_state_dict()); enc = enc.cuda().train()
    gen = SmirkGenerator(6, 3, 32, 5); gen.load_state_dict(G.synth_state_dict()); gen = gen.cuda().train()
    B = 2
    batch = synth_first_path_inputs(B, seed=31, device="cuda")[3]
    batch["img"] = A.synth_images(B, seed=81).cuda()
    yy, xx = torch.meshgrid(torch.arange(224.0), torch.arange(224.0), indexing="ij")
    batch["mask"] = (((yy - 112) ** 2 + (xx - 112) ** 2) > 80 ** 2).float()[None, None].repeat(B, 1, 1, 1).cuda()          # 0 inside the "hull", 1 outside
    batch["flag_landmarks_fan"] = torch.tensor([True, False], device="cuda")
    w = dict(WEIGHTS_TRAIN, mica_loss=10)
    params = [("smirk_encoder." + k, p) for k, p in enc.named_parameters()] + [("smirk_generator." + k, p) for k, p in gen.named_parameters()]

    def grads():
        out = {k: (None if p.grad is None else p.grad.clone()) for k, p in params}
        for _, p in params:
            p.grad = None
        return out

    mica = lambda out: {"mica_loss": (out["encoder_output"]["shape_params"] ** 2).mean()}        # a stand-in for a term computed elsewhere
    loss, terms, out = first_path(enc, fl, rn, gen, FirstPathLoss(w), batch, prob, extra=mica, _rng_stream=masking.PhiloxStream(7))
    loss.backward()
    fused = grads()
    d = terms.as_dict()
    law, losses, loss_img = first_path_law(out["encoder_output"], out["landmarks_fan"], out["landmarks_mp"], batch, w, reconstructed_img=out["reconstructed_img"],
                                           extra=mica(out), head_dtype=torch.float64)
    assert all(torch.isfinite(torch.tensor(v)) for v in d.values()) and list(d) == list(losses)
    for k, v in losses.items():
        _check_value(d[k], v, k)
    _check_value(loss, law, "loss_first_path")
    assert float((out["loss_img"].double() - loss_img).abs().max()) <= IMG_ABS
    for part in ("smirk_encoder.pose_encoder.", "smirk_encoder.shape_encoder.", "smirk_encoder.expression_encoder.", "smirk_generator."):
        mine = [g for k, g in fused.items() if k.startswith(part)]
        assert mine and all(g is not None and torch.isfinite(g).all() for g in mine) and any(bool(g.any()) for g in mine), part

    eager = {}
    for name, dt in (("fp32", None), ("float64 head", torch.float64)):
        o = forward_first_path(enc, fl, rn, gen, batch, prob, _rng_stream=masking.PhiloxStream(7))
        assert torch.equal(o["reconstructed_img"], out["reconstructed_img"]) and torch.equal(o["landmarks_mp"], out["landmarks_mp"])   # the same graph
        first_path_law(o["encoder_output"], o["landmarks_fan"], o["landmarks_mp"], batch, w, reconstructed_img=o["reconstructed_img"], extra=mica(o),
                       head_dtype=dt)[0].backward()
        eager[name] = grads()
    worst_ref, worst_fused, worst_ratio = 0.0, 0.0, ("", 0.0)
    failed = []
    for k, _ in params:
        g64, g32, gf = eager["float64 head"][k], eager["fp32"][k], fused[k]
        assert (g64 is None) == (gf is None), k
        if g64 is None:
            continue
        scale = max(1.0, float(g64.abs().max()))
        ref = float((g32 - g64).abs().max()) / scale
        mine = float((gf - g64).abs().max()) / scale
        worst_ref, worst_fused = max(worst_ref, ref), max(worst_fused, mine)
        if mine / max(4 * ref, 1e-6) > worst_ratio[1]:
            worst_ratio = (k, mine / max(4 * ref, 1e-6))
        if mine > max(4 * ref, 1e-6):
            failed.append((k, mine, ref))
    print(f"whole first path, {len(params)} parameter tensors, distance to the float64-head run relative to max(1, max|g|): eager fp32 head at most {worst_ref:.2e}, "
          f"fused head at most {worst_fused:.2e}; largest fused / max(4 x eager, 1e-6) = {worst_ratio[1]:.2f} [{worst_ratio[0]}]; largest distances of the "
          f"module: {seen}")
    # NOTE: two runs of this code gave identical figures, so the distances are reproducible as far as seen.  The fused head's distance does not come from its upstream
    # gradients (they are the correctly rounded ones); its likely cause is the order in which autograd adds the gradients that reach one tensor from several nodes (one
    # fused node here, a dozen eager ones in the law), amplified by the ill-conditioned chain.  Caveat: FLAME's flame_bwd_gather adds the landmark gradients onto the
    # vertices with float atomicAdd in no fixed order; should that ever vary between runs, both distances would carry it and this assertion, whose bound is 4x a
    # distance of the same kind, could fail with the loss head unchanged.
    assert not failed, failed[:5]
