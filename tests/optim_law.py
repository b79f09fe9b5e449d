"""The float64 law of smirk_amd.optim (include/smirk_optim.h), its inputs and its bounds, shared by tests/test_optim_cpu.py and tests/test_optim_gpu.py.

Law: torch's non-capturable Adam (no weight decay, no amsgrad) per element,
    m += (g - m) (1 - beta1);  v = v beta2 + (1 - beta2) g g;  p -= lr / (1 - beta1^t) * m / (sqrt(v) / sqrt(1 - beta2^t) + eps)
and the clip by its definition: norm = ||g||_2 over all tensors, coef = min(1, max_norm / (norm + 1e-6)), g *= coef — all in float64 from the fp32 inputs.
`ref32` is the reference itself on the CPU in fp32 on the same inputs: torch.optim.Adam(foreach=False) and torch.nn.utils.clip_grad_norm_.

Bounds (none of them is taken from what the HIP code gives):
  p, exp_avg, exp_avg_sq   per step and tensor, max |HIP - law| <= 4 x max |ref32 - law|, floored at one fp32 ulp of the tensor's largest magnitude.  Both sides
                           round the same dozen operations to fp32 but may associate them differently (torch's lerp has two forms, its GPU kernels multiply
                           by a reciprocal where the CPU divides): hence the margin of 4.  The margin does NOT cover an implementation that rounds the
                           products of lerp and addcmul on their own: ref32 fuses them, and an emulation without the fusion sits at 1.8 x (exp_avg_sq)
                           and 1.1 x (exp_avg) of this bound.
  norm                     relative error to the float64 norm <= 2^-22: float64 sums (error ~1e-13), one rounding to fp32 (2^-24), one square root.
  coef                     relative error <= 2^-22: three fp32 roundings (the norm, the sum with 1e-6, the quotient) of 2^-24 each.
  clipped gradients        within 4 fp32 ulp of g * coef64, per element: coef is within 1.5 ulp (above), the product adds half an ulp.
"""
import functools
import math

import numpy as np
import torch

from smirk_amd._lib import OPTIM_CHUNK

C = OPTIM_CHUNK
STEPS = 5
HYPERS = (dict(lr=1e-3, betas=(0.5, 0.999), eps=1e-8), dict(lr=0.25e-3, betas=(0.9, 0.999), eps=1e-8))       # base_trainer.py:62 (generator), :51 (encoder)
MAX_NORM = 0.1                                                                                              # smirk_trainer.py:379
# (name, shape).  "view": a 4-byte-aligned view base[1:1 + C + 2] on the device; "never": no gradient on any step; "skip3": none on step 3 only
CASES = [(f"n{n}", (n,)) for n in (1, 3, 4, 5, 63, 64, 65, C - 1, C, C + 1, 2 * C + 7, 0)] + [("conv", (8, 3, 3, 3)), ("view", (C + 2,)), ("never", (10,)), ("skip3", (70,))]
NAMES = [n for n, _ in CASES]
ZERO_START = ("n64", f"n{C}")                                                                               # parameters that start at exactly 0
ZEROS_IN_GRAD = (f"n{C - 1}", 2, 100)                                                                       # tensor, step (1-based), leading exact zeros
assert sum(math.prod(s) for _, s in CASES) < 10 ** 5


def has_grad(name, step):
    """step is 1-based"""
    return name != "never" and not (name == "skip3" and step == 3)


def expected_chunks():
    """first_chunk per tensor and total_chunks, from the shapes alone"""
    first, c = [], 0
    for _, s in CASES:
        first.append(c)
        c += -(-math.prod(s) // C)
    return first, c


@functools.lru_cache(maxsize=None)
def inputs(seed=20250):
    """-> (params, grads): params[i] an fp32 CPU tensor per case; grads[k][i] the gradient of step k + 1, or None.  Gradients are normal draws times
    10^u, u uniform in [-8, 0] per element; parameters are normal draws times 0.1 (an update of ~lr would drown in the rounding of larger ones)."""
    g = torch.Generator().manual_seed(seed)
    params = [torch.zeros(s) if n in ZERO_START else torch.randn(s, generator=g) * 0.1 for n, s in CASES]
    grads = []
    for k in range(1, STEPS + 1):
        row = []
        for n, s in CASES:
            t = torch.randn(s, generator=g) * 10.0 ** (torch.rand(s, generator=g) * 8.0 - 8.0)
            if (n, k) == ZEROS_IN_GRAD[:2]:
                t.view(-1)[:ZEROS_IN_GRAD[2]] = 0.0
            row.append(t if has_grad(n, k) else None)
        grads.append(row)
    return params, grads


def _schedule(opt, lr):
    return torch.optim.lr_scheduler.CosineAnnealingLR(opt, T_max=STEPS, eta_min=0.01 * lr)


@functools.lru_cache(maxsize=None)
def learning_rates(lr):
    """the learning rate each of the STEPS steps sees, from torch's own scheduler"""
    opt = torch.optim.SGD([torch.nn.Parameter(torch.zeros(1))], lr=lr)
    sched, out = _schedule(opt, lr), []
    for _ in range(STEPS):
        out.append(opt.param_groups[0]["lr"])
        opt.step(); sched.step()
    return tuple(out)


def clip_law(grads, max_norm, clamp=True):
    """grads: fp32 tensors -> (norm, coef) as Python floats (float64)"""
    norm = math.sqrt(sum(float((g.double() ** 2).sum()) for g in grads))
    coef = max_norm / (norm + 1e-6)
    return norm, (min(1.0, coef) if clamp else coef)


def adam_law(p, m, v, g, t, lr, beta1, beta2, eps, variant=None):
    """one step, float64 tensors in and out; t = the tensor's step count after this step.  `variant` names a deliberate mistake."""
    t = t + 1 if variant == "step_off_by_one" else t
    m = m + (g - m) * (1.0 - beta1)
    v = v * beta2 + (1.0 - beta2) * g * g
    bc1 = 1.0 if variant == "no_bias_correction1" else 1.0 - beta1 ** t
    bc2 = 1.0 if variant == "no_bias_correction2" else 1.0 - beta2 ** t
    denom = torch.sqrt(v / bc2 + eps) if variant == "eps_inside_sqrt" else torch.sqrt(v) / math.sqrt(bc2) + eps
    return p - (lr / bc1) * m / denom, m, v


def _record(ps, ms, vs, ts, norm, coef, clipped):
    return dict(p=[x.clone() for x in ps], m=[None if x is None else x.clone() for x in ms], v=[None if x is None else x.clone() for x in vs], t=list(ts),
                norm=norm, coef=coef, clipped=clipped)


@functools.lru_cache(maxsize=None)
def law(hyper_index, max_norm=MAX_NORM, variant=None):
    """-> [per step: dict(p, m, v: float64 tensors per case (m, v None without state), t: step counts, norm, coef, clipped: g * coef64 per case)]"""
    h, (params, grads) = HYPERS[hyper_index], inputs()
    lrs = learning_rates(h["lr"])
    ps, ms, vs, ts = [p.double() for p in params], [None] * len(params), [None] * len(params), [0] * len(params)
    out = []
    for k in range(STEPS):
        gs = grads[k]
        norm = coef = None
        if max_norm is not None:
            norm, coef = clip_law([g for g in gs if g is not None], max_norm, clamp=variant != "clip_not_clamped")
        clipped = [None if g is None else g.double() * (1.0 if coef is None else coef) for g in gs]
        for i, g in enumerate(clipped):
            if g is None:
                continue
            if ms[i] is None:
                ms[i], vs[i] = torch.zeros_like(ps[i]), torch.zeros_like(ps[i])
            ts[i] += 1
            ps[i], ms[i], vs[i] = adam_law(ps[i], ms[i], vs[i], g, ts[i], lrs[k], *h["betas"], h["eps"], variant if variant != "clip_not_clamped" else None)
        out.append(_record(ps, ms, vs, ts, norm, coef, clipped))
    return out


@functools.lru_cache(maxsize=None)
def ref(hyper_index, max_norm=MAX_NORM, dtype=torch.float32):
    """the reference on the CPU in `dtype`: torch.optim.Adam(foreach=False) + CosineAnnealingLR + torch.nn.utils.clip_grad_norm_; same record as law()"""
    h, (params, grads) = HYPERS[hyper_index], inputs()
    ps = [torch.nn.Parameter(p.clone().to(dtype)) for p in params]
    opt = torch.optim.Adam(ps, lr=h["lr"], betas=h["betas"], eps=h["eps"], foreach=False)
    sched, out = _schedule(opt, h["lr"]), []
    for k in range(STEPS):
        for p, g in zip(ps, grads[k]):
            p.grad = None if g is None else g.clone().to(dtype)
        norm = None
        if max_norm is not None:
            norm = float(torch.nn.utils.clip_grad_norm_(ps, max_norm, foreach=False))
        clipped = [None if p.grad is None else p.grad.clone() for p in ps]
        opt.step(); sched.step()
        st = [opt.state.get(p, {}) for p in ps]
        out.append(_record([p.detach() for p in ps], [s.get("exp_avg") for s in st], [s.get("exp_avg_sq") for s in st],
                           [int(s["step"]) if "step" in s else 0 for s in st], norm, None, clipped))
    return out


def ref32(hyper_index, max_norm=MAX_NORM):
    return ref(hyper_index, max_norm, torch.float32)


def ulp32(x):
    """one fp32 unit in the last place at magnitude x (float or float64 tensor)"""
    if torch.is_tensor(x):
        return torch.from_numpy(np.spacing(x.abs().float().numpy()).astype(np.float64)).reshape(x.shape)
    return float(np.spacing(np.float32(abs(x))))


def state_bound(ref_value, law_value):
    """the bound of one tensor at one step: 4 x the reference's own distance to the law, at least one ulp of the tensor's largest magnitude"""
    if law_value.numel() == 0:
        return 0.0
    return max(4.0 * float((ref_value.double() - law_value).abs().max()), ulp32(float(law_value.abs().max())))


def distance(value, law_value):
    return 0.0 if law_value.numel() == 0 else float((value.double().cpu() - law_value).abs().max())


NORM_REL = COEF_REL = 2.0 ** -22
CLIP_ULPS = 4.0


def check_states(got, hyper_index, max_norm=MAX_NORM, what="", ref_record=None, law_record=None):
    """got: [per step dict(p, m, v, t)] from the code under test.  Asserts every tensor of every step against the bound; prints and returns the largest
    error / bound ratio per quantity."""
    lw = law(hyper_index, max_norm) if law_record is None else law_record
    rf = ref32(hyper_index, max_norm) if ref_record is None else ref_record
    worst = {}
    for k, (g, l, r) in enumerate(zip(got, lw, rf)):
        assert list(g["t"]) == list(l["t"]) == list(r["t"]), (what, k, g["t"], l["t"])
        for q in ("p", "m", "v"):
            for i, name in enumerate(NAMES):
                if l[q][i] is None:
                    assert g[q][i] is None and r[q][i] is None, (what, k, q, name)
                    continue
                err, bound = distance(g[q][i], l[q][i]), state_bound(r[q][i], l[q][i])
                ratio = err / bound if bound > 0 else 0.0
                if ratio > worst.get(q, (0.0,))[0]:
                    worst[q] = (ratio, err, bound, name, k + 1)
                assert err <= bound, f"{what} step {k + 1} {q}[{name}]: |HIP - law| {err:.3e} > bound {bound:.3e}"
    for q, (ratio, err, bound, name, k) in sorted(worst.items()):
        print(f"{what} hyper {hyper_index} {q}: largest error / bound {ratio:.3f} (error {err:.3e}, bound {bound:.3e}, tensor {name}, step {k})")
    return worst
