"""The trainer's optimiser stage on the HIP path (include/smirk_optim.h, csrc/optim.hip): drop-ins for the last three lines of the reference's step,

    torch.nn.utils.clip_grad_norm_(self.smirk_generator.parameters(), 0.1)        smirk_trainer.py:379
    self.encoder_optimizer.step(); self.smirk_generator_optimizer.step()          base_trainer.py:51, 62, 123-127   (torch.optim.Adam)

as multi-tensor kernels: the clip is three launches whatever the number of gradients, an Adam step one launch per parameter group.

    from smirk_amd import Adam, clip_grad_norm_

`Adam` is a `torch.optim.Optimizer`: schedulers, `param_groups[i]['lr'] = ...`, `zero_grad()`, `add_param_group` and `state_dict()` work as with
`torch.optim.Adam`, the state has torch's keys (`step`: an fp32 scalar on the CPU, `exp_avg`, `exp_avg_sq`) and loads into `torch.optim.Adam` and back.  What
the reference never uses is refused at construction by name (house rule): weight_decay != 0, amsgrad, maximize, capturable, differentiable, fused,
decoupled_weight_decay.  There is no CPU path and no fallback to torch's kernels: a CPU, non-fp32, sparse or non-contiguous tensor raises SmirkHipError.

The arithmetic is torch's `_single_tensor_adam` in fp32, operation for operation as torch's CPU kernels compute it: ATen's two fused lerp forms, the fused
addcmul, `denom = sqrt(v) / bias_correction2_sqrt + eps` with a true division, everything else rounded on its own (include/smirk_optim.h; DESIGN.md §24 has
the bounds against the float64 law).  Nothing here synchronises, reads a device value back or makes the
library allocate; everything runs on torch's current stream.
"""
import ctypes as C
import math

import numpy as np
import torch

from . import _lib as L
from ._lib import SmirkHipError, check, lib

_STEP_ROW = np.dtype([("grad", "<u8"), ("step_size", "<f4"), ("bias_correction2_sqrt", "<f4")])
assert _STEP_ROW.itemsize == C.sizeof(L.SmirkOptimStep) == 16 and C.sizeof(L.SmirkOptimTensor) == 40
_REFUSED = ("amsgrad", "maximize", "capturable", "differentiable", "fused", "decoupled_weight_decay")


def _upload(nbytes, fill, device):
    """pinned host buffer filled by `fill(address)` -> device copy on the current stream without a synchronisation (torch's host allocator keeps the pinned
    block until the copy has run)"""
    pin = torch.empty(max(int(nbytes), 16), dtype=torch.uint8, pin_memory=True)
    fill(pin.data_ptr())
    return pin.to(device, non_blocking=True)


def _static_tables(rows, kinds, device):
    """rows: [(param ptr, exp_avg ptr, exp_avg_sq ptr, numel)] -> (static table on the device, chunk map on the device, total_chunks, first_chunk list).
    smirk_optim_plan validates the rows and lays out the chunks; nothing here touches the device but the two copies."""
    n = len(rows)
    host = (L.SmirkOptimTensor * n)()
    for r, (p, m, v, numel) in zip(host, rows):
        r.param, r.exp_avg, r.exp_avg_sq, r.numel = p, m, v, numel
    total = C.c_longlong(0)
    check(lib().smirk_optim_plan(host, None, n, kinds, C.byref(total)))
    total = total.value
    table = _upload(C.sizeof(host), lambda a: C.memmove(a, host, C.sizeof(host)), device)
    cmap = _upload(4 * total, lambda a: check(lib().smirk_optim_chunk_map(host, n, C.c_void_p(a), total)), device)
    return table, cmap, total, [r.first_chunk for r in host]


def _check_grad(g, device, what="gradient"):
    if g.layout is not torch.strided:
        raise SmirkHipError(f"smirk_amd.optim: sparse {what}s are not supported (layout {g.layout})")
    if not g.is_cuda:
        raise SmirkHipError(f"smirk_amd.optim runs on the MI355X HIP device only: got a CPU {what} (no CPU fallback exists)")
    if g.dtype is not torch.float32:
        raise SmirkHipError(f"smirk_amd.optim: expected an fp32 {what}, got {g.dtype}")
    if not g.is_contiguous():
        raise SmirkHipError(f"smirk_amd.optim: expected a contiguous {what} (shape {tuple(g.shape)}, strides {g.stride()})")
    if device is not None and g.device != device:
        raise SmirkHipError(f"smirk_amd.optim: tensors on more than one device ({device} and {g.device})")


def _refuse_capture(what):
    if torch.cuda.is_current_stream_capturing():
        raise SmirkHipError(f"{what} cannot be captured into a graph: it bakes host values (gradient pointers, the step's scalars) into what it launches")


class _Plan:
    """what one parameter group keeps between steps: the static table and the chunk map of the parameters that had a gradient when it was made"""
    __slots__ = ("ids", "pptrs", "params", "state", "steps", "n", "total", "table", "cmap", "device")


class Adam(torch.optim.Optimizer):
    """torch.optim.Adam (no weight decay, no amsgrad) with the update in one HIP launch per parameter group.  See the module docstring."""

    def __init__(self, params, lr=1e-3, betas=(0.9, 0.999), eps=1e-8, weight_decay=0, amsgrad=False, *, foreach=None, maximize=False, capturable=False,
                 differentiable=False, fused=None, decoupled_weight_decay=False):
        defaults = dict(lr=lr, betas=betas, eps=eps, weight_decay=weight_decay, amsgrad=amsgrad, maximize=maximize, foreach=foreach, capturable=capturable,
                        differentiable=differentiable, fused=fused, decoupled_weight_decay=decoupled_weight_decay)
        self._check_options(defaults)
        self._plans = {}
        super().__init__(params, defaults)

    @staticmethod
    def _check_options(group):
        lr, betas, eps = group["lr"], group["betas"], group["eps"]
        if isinstance(lr, torch.Tensor):
            raise ValueError("smirk_amd.Adam: a tensor lr is not supported (the step's scalars are computed on the host); pass a float")
        if not 0.0 <= lr or not math.isfinite(lr):
            raise ValueError(f"Invalid learning rate: {lr}")
        if isinstance(eps, torch.Tensor) or not 0.0 <= eps or not math.isfinite(eps):
            raise ValueError(f"Invalid epsilon value: {eps}")
        if len(betas) != 2 or any(isinstance(b, torch.Tensor) for b in betas):
            raise ValueError(f"Invalid betas: {betas} (two floats)")
        for i, b in enumerate(betas):
            if not 0.0 <= b < 1.0:
                raise ValueError(f"Invalid beta parameter at index {i}: {b}")
        if group["weight_decay"] != 0:
            raise ValueError(f"smirk_amd.Adam: weight_decay={group['weight_decay']} is not supported (the reference trains with weight_decay=0); "
                             "use torch.optim.Adam")
        for name in _REFUSED:
            if group.get(name):
                raise ValueError(f"smirk_amd.Adam: {name}={group[name]} is not supported (the reference never sets it); use torch.optim.Adam")

    def add_param_group(self, param_group):
        super().add_param_group(param_group)
        self._check_options(self.param_groups[-1])
        self._plans.clear()

    def load_state_dict(self, state_dict):
        """torch's, then the descriptor tables are dropped: the restored exp_avg / exp_avg_sq are new tensors (and may be 4-byte aligned only)."""
        super().load_state_dict(state_dict)
        self._plans.clear()
        for group in self.param_groups:
            self._check_options(group)

    def __setstate__(self, state):
        super().__setstate__(state)
        self._plans = {}

    def _make_plan(self, params, pptrs):
        device = params[0].device
        rows, steps, kept = [], [], []
        for p in params:
            _check_grad(p, device, "parameter")
            st = self.state[p]
            if len(st) == 0:                                                       # torch's lazy state initialisation, torch's keys
                st["step"] = torch.tensor(0.0, dtype=torch.float32)
                st["exp_avg"] = torch.zeros_like(p, memory_format=torch.preserve_format)
                st["exp_avg_sq"] = torch.zeros_like(p, memory_format=torch.preserve_format)
            m, v, t = st["exp_avg"], st["exp_avg_sq"], st["step"]
            for name, s in (("exp_avg", m), ("exp_avg_sq", v)):
                _check_grad(s, device, f"state tensor {name}")
                if s.shape != p.shape:
                    raise SmirkHipError(f"smirk_amd.Adam: state tensor {name} has shape {tuple(s.shape)}, its parameter {tuple(p.shape)}")
            if not (torch.is_tensor(t) and t.device.type == "cpu" and t.dim() == 0 and t.dtype is torch.float32):
                raise SmirkHipError("smirk_amd.Adam: state['step'] must be an fp32 scalar tensor on the CPU (torch's default for Adam)")
            rows.append((p.data_ptr(), m.data_ptr(), v.data_ptr(), p.numel()))
            steps.append(float(t))
            kept.append((m, v))
        # The step counts of the plan's tensors live in ONE fp32 CPU tensor and each state["step"] is a 0-dim view of it: advancing and reading them is one
        # host operation each instead of one per tensor (measured: 175 us of torch._foreach_add_ per group of ~200 tensors).  State dicts keep torch's form.
        flat = torch.tensor(steps, dtype=torch.float32)
        for i, p in enumerate(params):
            self.state[p]["step"] = flat[i]
        plan = _Plan()
        plan.ids, plan.pptrs, plan.params, plan.state, plan.steps, plan.n, plan.device = list(map(id, params)), pptrs, params, kept, flat, len(params), device
        plan.table, plan.cmap, plan.total, _ = _static_tables(rows, L.OPTIM_KIND_ADAM, device)
        return plan

    @torch.no_grad()
    def step(self, closure=None, grad_scale=None):
        """One Adam step.  Parameters whose `.grad` is None are skipped and their `step` does not advance, as in torch.

        grad_scale: None, or a one-element fp32 device tensor — normally the `coef` of `clip_grad_norm_(..., defer=True)`.  Every gradient is multiplied by it
        in registers on its way into the update (the result is bit-identical to scaling the gradients in place first); the gradients in memory stay unscaled.

        Per group and step one pinned-host -> device copy carries what changes every step (gradient pointers, which autograd re-allocates after zero_grad(),
        and each tensor's step_size = lr / (1 - beta1^t) and sqrt(1 - beta2^t), computed in double precision from its own step count and rounded to fp32 as
        torch rounds them); parameter and state pointers and the chunk map stay on the device and are re-planned when the set of tensors with a gradient
        changes, a parameter's storage moves, or a state dict is loaded.  No synchronisation.  Host values are baked into what is launched, so the step
        cannot be captured into a HIP graph (raises SmirkHipError on a capturing stream)."""
        loss = None
        if closure is not None:
            with torch.enable_grad():
                loss = closure()
        device, gs_ptr = None, None
        for gi, group in enumerate(self.param_groups):
            params, gptrs, pptrs = [], [], []
            for p in group["params"]:
                g = p.grad
                if g is None:
                    continue
                if device is None:
                    device = g.device
                if g.dtype is not torch.float32 or g.device != device or g.layout is not torch.strided or not g.is_contiguous() or g.shape != p.shape:
                    _check_grad(g, device)
                    raise SmirkHipError(f"smirk_amd.Adam: gradient of shape {tuple(g.shape)} for a parameter of shape {tuple(p.shape)}")
                params.append(p); gptrs.append(g.data_ptr()); pptrs.append(p.data_ptr())
            if not params:
                continue
            if device.type != "cuda":
                _check_grad(params[0].grad, None)
            if gs_ptr is None:
                _refuse_capture("smirk_amd.Adam.step")
                if grad_scale is not None:
                    if not torch.is_tensor(grad_scale) or grad_scale.numel() != 1:
                        raise SmirkHipError("smirk_amd.Adam.step: grad_scale must be a one-element fp32 device tensor")
                    _check_grad(grad_scale, device, "grad_scale tensor")
                gs_ptr = C.c_void_p(grad_scale.data_ptr() if grad_scale is not None else 0)
            self._check_options(group)
            plan = self._plans.get(gi)
            if plan is None or plan.pptrs != pptrs or plan.ids != list(map(id, params)):
                plan = self._plans[gi] = self._make_plan(params, pptrs)
            plan.steps += 1.0                                                      # CPU scalars: host arithmetic, seen through every state["step"]
            ts = plan.steps.tolist()
            lr, (beta1, beta2), eps = group["lr"], group["betas"], group["eps"]
            scal = {t: (lr / (1.0 - beta1 ** t), (1.0 - beta2 ** t) ** 0.5) for t in set(ts)}       # torch's expressions, in Python floats (double precision)
            n = plan.n

            def fill(address, gptrs=gptrs, ts=ts, scal=scal, n=n):
                rows = np.ctypeslib.as_array(C.cast(address, C.POINTER(C.c_uint8)), shape=(16 * n,)).view(_STEP_ROW)
                rows["grad"] = gptrs
                if len(scal) == 1:
                    rows["step_size"], rows["bias_correction2_sqrt"] = scal[ts[0]]
                else:
                    rows["step_size"] = [scal[t][0] for t in ts]
                    rows["bias_correction2_sqrt"] = [scal[t][1] for t in ts]
            with torch.cuda.device(device):
                steps_dev = _upload(16 * n, fill, device)
                check(lib().smirk_optim_adam_step(plan.table.data_ptr(), steps_dev.data_ptr(), plan.cmap.data_ptr(), n, plan.total, beta1, beta2, eps, gs_ptr,
                                                  L.stream_ptr()))
        return loss


_CLIP_PLANS = {}                                                                   # (device, element counts) -> (static table, chunk map, total_chunks); a handful of entries


def _clip_plan(device, numels):
    key = (device, numels)
    plan = _CLIP_PLANS.get(key)
    if plan is None:
        if len(_CLIP_PLANS) >= 8:
            _CLIP_PLANS.pop(next(iter(_CLIP_PLANS)))
        plan = _CLIP_PLANS[key] = _static_tables([(0, 0, 0, k) for k in numels], L.OPTIM_KIND_NORM | L.OPTIM_KIND_SCALE, device)[:3]
    return plan


@torch.no_grad()
def clip_grad_norm_(parameters, max_norm, norm_type=2.0, error_if_nonfinite=False, foreach=None, *, defer=False):
    """torch.nn.utils.clip_grad_norm_ for fp32 gradients on the HIP device: the global L2 norm of all gradients (one float64 sum in a fixed order, rounded
    once), then g *= coef with coef = min(1, max_norm / (norm + 1e-6)) in fp32, in place.  Three launches for any number of tensors, no synchronisation.
    Returns the total norm as a 0-dim fp32 device tensor (with no gradients at all: a zero tensor, like torch).

    norm_type other than 2 raises.  `foreach` is accepted and ignored (the kernels are multi-tensor either way).  error_if_nonfinite=True reads the norm
    back — the ONE synchronisation this module can make — and raises RuntimeError like torch when it is nan or inf.

    defer=True skips the scaling launch and returns (norm, coef), coef a one-element fp32 device tensor (None with no gradients): hand it to
    `Adam.step(grad_scale=coef)`, which applies it in registers — one launch and one read + write pass over the gradients less.  The gradients in memory then
    stay UNSCALED.  Cannot be captured into a HIP graph (gradient pointers are baked into the launch)."""
    if isinstance(parameters, torch.Tensor):
        parameters = [parameters]
    grads = [p.grad for p in parameters if p.grad is not None]
    max_norm, norm_type = float(max_norm), float(norm_type)
    if norm_type != 2.0:
        raise SmirkHipError(f"smirk_amd.clip_grad_norm_: norm_type={norm_type} is not supported (the reference clips the L2 norm); use torch.nn.utils.clip_grad_norm_")
    if not grads:
        zero = torch.tensor(0.0)
        return (zero, None) if defer else zero
    device = grads[0].device
    for g in grads:
        _check_grad(g, device)
    _refuse_capture("smirk_amd.clip_grad_norm_")
    table, cmap, total = _clip_plan(device, tuple(g.numel() for g in grads))
    n, gptrs = len(grads), [g.data_ptr() for g in grads]

    def fill(address):
        rows = np.ctypeslib.as_array(C.cast(address, C.POINTER(C.c_uint8)), shape=(16 * n,)).view(_STEP_ROW)
        rows["grad"] = gptrs
        rows["step_size"] = rows["bias_correction2_sqrt"] = 0.0
    with torch.cuda.device(device):
        steps_dev = _upload(16 * n, fill, device)
        ws_bytes = lib().smirk_optim_grad_norm_workspace_bytes(total)
        ws = torch.empty(ws_bytes // 8, dtype=torch.float64, device=device)
        out = torch.empty(2, dtype=torch.float32, device=device)
        st = L.stream_ptr()
        check(lib().smirk_optim_grad_norm(table.data_ptr(), steps_dev.data_ptr(), cmap.data_ptr(), n, total, max_norm, ws.data_ptr(), ws_bytes, out.data_ptr(), st))
        norm, coef = out[0], out[1:2]
        if error_if_nonfinite and not bool(torch.isfinite(norm)):                  # the documented synchronisation
            raise RuntimeError(f"The total norm of order {norm_type} for gradients from `parameters` is non-finite, so it cannot be clipped. To disable this "
                               "error and scale the gradients by the non-finite norm anyway, set `error_if_nonfinite=False`")
        if defer:
            return norm, coef
        check(lib().smirk_optim_scale_grads(table.data_ptr(), steps_dev.data_ptr(), cmap.data_ptr(), n, total, coef.data_ptr(), st))
    return norm
