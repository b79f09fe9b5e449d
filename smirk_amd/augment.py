"""The augmented FLAME parameters that start the reference trainer's second path (smirk_trainer.py:192-248), drawn on the MI355X.

    templates = load_templates()                                    # utils.py:5-25, host
    bank = TemplateBank(templates, num_expression=50).cuda()        # flattened once into a device table
    flame_feats = augment_flame_params(encoder_output, bank, Ke=1)  # two launches of libsmirk_hip.so (smirk_amd/csrc/augment.hip)

The reference runs this block in eager torch: about 150 small launches, and a Python loop over a quarter of the rows that copies one template per iteration
from pageable host memory (a host stall each).  Here the whole law — four random groups, the per-group expression laws, jaw and eyelid jitter, the copies —
is stream-ordered device work with no host synchronisation, so the host can keep enqueueing.  Random numbers come from the counter-based Philox stream of
smirk_amd.masking (`torch.manual_seed` reproduces a run, successive calls differ, an explicit PhiloxStream pins a call); like there they are not torch's
numbers, and tests pin the law (tests/augment_law.py), not the draws.
"""
import ctypes as C
import os

import numpy as np
import torch

from . import _lib as L
from .masking import _rng

TEMPLATE_CLASSES = ("lips_back", "rolling_lips", "mouth_side", "kissing", "high_smile", "mouth_up", "mouth_middle", "mouth_down", "blow_cheeks", "cheeks_in",
                    "jaw", "lips_up")                        # utils.py:7-8: the expression classes the trainer injects
MAX_ROWS = 8192                                              # include/smirk_hip.h SMIRK_AUGMENT_MAX_ROWS
KEYS = ("expression_params", "jaw_params", "eyelid_params", "shape_params", "pose_params", "cam")


def load_templates(path="assets/expression_templates_famos"):
    """utils.py:5-25: {subject + class: ndarray [n, >= 50]} of the FaMoS expression templates under `path` (cwd-relative like the reference).  One directory per
    subject, one per class inside it, one .npy per template holding a pickled dict whose 'expression' entry is the parameter vector."""
    templates = {}
    for subject in os.listdir(path):
        sdir = os.path.join(path, subject)
        if not os.path.isdir(sdir):
            continue
        for cls in os.listdir(sdir):
            if cls.endswith(".mp4") or cls not in TEMPLATE_CLASSES:
                continue
            cdir = os.path.join(sdir, cls)
            templates[subject + cls] = np.array([np.load(os.path.join(cdir, f), allow_pickle=True).item()["expression"].squeeze() for f in os.listdir(cdir)])
    return templates


class TemplateBank:
    """The template dict flattened once: `table` float32 [T, num_expression] (the columns the trainer injects, base_trainer.py:74) and `offsets` int32 [C + 1],
    class c owning rows offsets[c]:offsets[c + 1] in the dict's key order (the order `random.choice(list(templates.keys()))` indexes, base_trainer.py:70).
    `.to(device)` / `.cuda()` move the two tensors; the host copy of the offsets stays (the library validates it before it launches)."""

    def __init__(self, templates, num_expression=50):
        if not templates:
            raise ValueError("TemplateBank needs at least one template class")
        rows, off = [], [0]
        for key, t in templates.items():
            t = np.asarray(t, dtype=np.float32)
            t = t.reshape(1, -1) if t.ndim == 1 else t
            if t.shape[0] < 1 or t.shape[1] < num_expression:
                raise ValueError(f"template class {key!r}: expected [n >= 1, >= {num_expression}], got {t.shape}")
            rows.append(t[:, :num_expression])
            off.append(off[-1] + t.shape[0])
        self.num_expression = int(num_expression)
        self.names = tuple(templates.keys())
        self.table = torch.from_numpy(np.ascontiguousarray(np.concatenate(rows, 0)))
        self.offsets_host = np.asarray(off, dtype=np.int32)
        self.offsets = torch.from_numpy(self.offsets_host.copy())

    @property
    def n_classes(self):
        return len(self.names)

    @property
    def device(self):
        return self.table.device

    def to(self, device):
        self.table, self.offsets = self.table.to(device), self.offsets.to(device)
        return self

    def cuda(self, device=None):
        return self.to(torch.device("cuda", torch.cuda.current_device() if device is None else device))


def n_counters(N, E):
    """Philox counters one call consumes (smirk_amd/csrc/augment_rng.h): four per row on one stream id, one per expression element on another."""
    return int(N) * max(int(E), 4)


_ws = L.Workspace()


def augment_flame_params(encoder_output, bank, Ke=1, num_expression=50, use_eyelids=True, _rng_stream=None, _return_plan=False):
    """smirk_trainer.py:192-248.  encoder_output: the SmirkEncoder dict ([B, .] tensors on the device); returns `flame_feats`: the same keys with Ke * B rows,
    detached (row r starts as row r % B, i.e. torch.cat(Ke * [v])).  `bank`: a TemplateBank on the same device built with the same `num_expression`.
    `_rng_stream`: an explicit masking.PhiloxStream (advanced by n_counters(Ke * B, E)); `_return_plan`: also return the int32 [Ke * B, 4] plan
    (group, position in the group, source row of group 1, template row of group 2)."""
    src = {k: encoder_output[k] for k in KEYS}
    for k, v in src.items():
        if not v.is_cuda:
            raise L.SmirkHipError(f"smirk_amd runs on the MI355X HIP device only: {k} is a CPU tensor (no CPU fallback exists)")
    if not bank.table.is_cuda:
        raise L.SmirkHipError("the TemplateBank is on the host: call .cuda() / .to(device) once after building it")
    if bank.num_expression != int(num_expression):
        raise L.SmirkHipError(f"the TemplateBank was built for num_expression={bank.num_expression}, the call asks for {num_expression}")
    src = {k: L.as_f32c(v.detach()) for k, v in src.items()}
    e = src["expression_params"]
    B, E = e.shape
    S, Ke = src["shape_params"].shape[1], int(Ke)
    widths = dict(jaw_params=3, eyelid_params=2, pose_params=3, cam=3)
    for k, w in widths.items():
        if tuple(src[k].shape) != (B, w):
            raise L.SmirkHipError(f"{k}: expected [{B}, {w}], got {tuple(src[k].shape)}")
    if src["shape_params"].shape[0] != B:
        raise L.SmirkHipError("shape_params: batch size differs from expression_params")
    N, dev = Ke * B, e.device
    lib = L.lib()
    out = {k: torch.empty((max(N, 0),) + tuple(v.shape[1:]), device=dev) for k, v in src.items()}
    plan = torch.empty(max(N, 0), 4, dtype=torch.int32, device=dev)
    need = lib.smirk_cycle_augment_workspace_bytes(N)
    ws = _ws.get(need, dev)
    seed, off = _rng(n_counters(N, E), _rng_stream)
    L.check(lib.smirk_cycle_augment(*[L.ptr(src[k]) for k in KEYS], B, E, S, Ke, int(num_expression), int(bool(use_eyelids)), L.ptr(bank.table),
                                    L.ptr(bank.offsets, torch.int32), bank.offsets_host.ctypes.data_as(C.c_void_p), bank.n_classes, seed, off,
                                    *[L.ptr(out[k]) for k in KEYS], L.ptr(plan, torch.int32), C.c_void_p(ws.data_ptr()), ws.numel(), L.stream_ptr()))
    for k, v in encoder_output.items():                       # the reference clones every entry of the dict (smirk_trainer.py:194-197)
        if k not in out:
            out[k] = torch.cat(Ke * [v.detach()], dim=0)
    return (out, plan) if _return_plan else out
