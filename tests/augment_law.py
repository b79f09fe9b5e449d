"""The law of the cycle path's parameter augmentation (smirk_trainer.py:192-248), twice — helper module, no tests.

(a) `restate`: what smirk_amd/csrc/augment.hip computes, in numpy float64 on the SAME Philox integers (counter layout: smirk_amd/csrc/augment_rng.h).  Every
    discrete choice of the kernel is a function of the integer draw, so the plan is reproduced exactly and the outputs up to fp32 rounding.
(b) `reference_law`: the reference's block in eager torch, statement by statement with its line numbers — the oracle of the law test and the comparator of
    tools/augment_times.py.  Like the reference it draws on the host and moves every draw to `device`.
"""
import random

import numpy as np
import torch

STREAM_ROW, STREAM_ELEM = 4, 5
_M32 = np.uint64(0xFFFFFFFF)
KEYS = ("expression_params", "jaw_params", "eyelid_params", "shape_params", "pose_params", "cam")


def philox(idx, stream, seed):
    """Philox4x32-10, counter = (idx lo, idx hi, stream, 0), key = seed -> four uint64 arrays holding 32-bit words."""
    idx = np.asarray(idx, dtype=np.uint64)
    c0, c1, c2, c3 = idx & _M32, idx >> np.uint64(32), np.full_like(idx, stream), np.zeros_like(idx)
    k0, k1 = np.uint64(seed & 0xFFFFFFFF), np.uint64((seed >> 32) & 0xFFFFFFFF)
    for _ in range(10):
        p0, p1 = np.uint64(0xD2511F53) * c0, np.uint64(0xCD9E8D57) * c2
        c0, c1, c2, c3 = (p1 >> np.uint64(32)) ^ c1 ^ k0, p1 & _M32, (p0 >> np.uint64(32)) ^ c3 ^ k1, p0 & _M32
        k0, k1 = (k0 + np.uint64(0x9E3779B9)) & _M32, (k1 + np.uint64(0xBB67AE85)) & _M32
    return c0, c1, c2, c3


def _u01(x):
    return (x >> np.uint64(8)).astype(np.float64) / 16777216.0


def _normal2(xa, xb):
    rad = np.sqrt(-2.0 * np.log(((xa >> np.uint64(8)) + np.uint64(1)).astype(np.float64) / 16777216.0))
    ang = 2.0 * np.pi * _u01(xb)
    return rad * np.cos(ang), rad * np.sin(ang)


def _rank(key, rows):
    """position of every element when sorted by (key, row)"""
    order = np.lexsort((rows, key))
    rank = np.empty(len(key), dtype=np.int64)
    rank[order] = np.arange(len(key))
    return rank


def n_counters(N, E):
    return N * max(E, 4)


def restate(enc, Ke, table, offsets, num_expression, use_eyelids, seed, offset):
    """enc: dict of numpy arrays [B, .]; table [T, num_expression], offsets [C + 1].  -> (dict of float64 arrays [Ke * B, .], plan int32 [Ke * B, 4])"""
    e0 = np.asarray(enc["expression_params"], dtype=np.float64)
    B, E = e0.shape
    N = Ke * B
    rows = np.arange(N, dtype=np.int64)
    base = np.uint64(offset) + np.uint64(4) * rows.astype(np.uint64)
    k1, k2, xc, xr = philox(base, STREAM_ROW, seed)
    rank = _rank(k1, rows)
    b1, b2, b3 = N // 4, 2 * N // 4, 3 * N // 4
    group = (rank >= b1).astype(np.int64) + (rank >= b2) + (rank >= b3)
    pos = rank - np.array([0, b1, b2, b3])[group]
    plan = np.full((N, 4), -1, dtype=np.int32)
    plan[:, 0], plan[:, 1] = group, pos
    g0, g1, g2, g3 = (group == k for k in range(4))
    # group 1: the row whose position in the group equals this row's rank by the second key
    m1 = rows[g1]
    src = rows % B
    if len(m1):
        at = np.empty(len(m1), dtype=np.int64)
        at[pos[m1]] = m1
        plan[m1, 2] = at[_rank(k2[m1], m1)]
        src[m1] = plan[m1, 2] % B
    # group 2: class, then row of the class
    offsets = np.asarray(offsets, dtype=np.int64)
    cls = ((xc * np.uint64(len(offsets) - 1)) >> np.uint64(32)).astype(np.int64)
    lo, n_in = offsets[cls], offsets[cls + 1] - offsets[cls]
    trow = lo + ((xr * n_in.astype(np.uint64)) >> np.uint64(32)).astype(np.int64)
    plan[g2, 3] = trow[g2]

    xu, xn, xb, _ = philox(base + np.uint64(1), STREAM_ROW, seed)
    u, noise, jbern = _u01(xu)[:, None], 0.2 * _u01(xn)[:, None], (xb & np.uint64(1)).astype(np.float64)
    eidx = np.uint64(offset) + (rows[:, None] * E + np.arange(E)[None, :]).astype(np.uint64)
    ea, eb, em, _ = philox(eidx, STREAM_ELEM, seed)
    za, zb = _normal2(ea, eb)
    cur = e0[rows % B]
    expr = np.zeros((N, E))
    expr[g0] = np.clip(za[g0] * (1 + 2 * u[g0]) * (em[g0] & np.uint64(1)).astype(np.float64) + cur[g0], -4.0, 4.0)
    expr[g1] = (0.25 + 1.25 * u[g1]) * e0[src[g1]]
    t = cur[g2].copy()
    t[:, :num_expression] = (0.25 + 1.25 * u[g2]) * np.asarray(table, dtype=np.float64)[trow[g2]]
    expr[g2] = t
    expr += noise * zb

    j0, j1, j2, j3 = philox(base + np.uint64(2), STREAM_ROW, seed)
    (n0, n1), (n2, _) = _normal2(j0, j1), _normal2(j2, j3)
    jaw = np.asarray(enc["jaw_params"], dtype=np.float64)[rows % B] + 0.2 * np.stack([n0, n1, n2], 1) * np.array([1.0, 0.1, 0.1]) * jbern[:, None]
    jaw[:, 0] = np.clip(jaw[:, 0], 0.0, 0.5)
    jaw[g3] = 0.0
    l0, l1, l2, l3 = philox(base + np.uint64(3), STREAM_ROW, seed)
    eye = np.asarray(enc["eyelid_params"], dtype=np.float64)[rows % B]
    if use_eyelids:
        eye = np.clip(eye + 0.25 * (2 * np.stack([_u01(l0), _u01(l1)], 1) - 1), 0.0, 1.0)
    eye[g3] = np.stack([_u01(l2), _u01(l3)], 1)[g3]
    out = dict(expression_params=expr, jaw_params=jaw, eyelid_params=eye)
    for k in ("shape_params", "pose_params", "cam"):
        out[k] = np.asarray(enc[k])[rows % B]
    return out, plan


def reference_law(enc, Ke, templates, seed=None, device="cpu", num_expression=50, use_eyelids=True, _return_groups=False):
    """smirk_trainer.py:192-248 in eager torch.  enc: dict of torch tensors [B, .] on `device`; templates: the dict of load_templates (utils.py:5-25).
    seed: seeds torch's generator and the host RNG of the template pick (None: leave both as they are, as the trainer does)."""
    rnd = random if seed is None else random.Random(seed)
    if seed is not None:
        torch.manual_seed(seed)
    B = enc["expression_params"].shape[0]
    N = Ke * B
    feats = {k: torch.cat(Ke * [v.clone().detach()], dim=0) for k, v in enc.items()}                                  # :194-197
    perm = torch.randperm(N)                                                                                          # :200
    gids = [perm[:N // 4], perm[N // 4: 2 * N // 4], perm[2 * N // 4: 3 * N // 4], perm[3 * N // 4:]]                 # :202
    D = feats["expression_params"].size(1)                                                                            # :204
    ex = feats["expression_params"]
    n0, n1, n2, n3 = (len(g) for g in gids)
    pmask = torch.bernoulli(torch.ones((n0, D)) * 0.5).to(device)                                                     # :208
    new = torch.randn((n0, D)).to(device) * (1 + 2 * torch.rand((n0, 1)).to(device)) * pmask + ex[gids[0]]            # :210
    ex[gids[0]] = torch.clamp(new, -4.0, 4.0) + (0 + 0.2 * torch.rand((n0, 1)).to(device)) * torch.randn((n0, D)).to(device)   # :211
    ex[gids[1]] = (0.25 + 1.25 * torch.rand((n1, 1)).to(device)) * ex[gids[1]][torch.randperm(n1)] + \
        (0 + 0.2 * torch.rand((n1, 1)).to(device)) * torch.randn((n1, D)).to(device)                                  # :215-216
    keys = list(templates.keys())
    for i in range(n2):                                                                                               # :220
        t = templates[rnd.choice(keys)]                                                                               # base_trainer.py:70-71
        row = t[rnd.randint(0, t.shape[0] - 1)][:num_expression]                                                      # base_trainer.py:72-74
        ex[gids[2][i], :num_expression] = (0.25 + 1.25 * torch.rand((1, 1)).to(device)) * torch.Tensor(row).to(device)   # :222
    ex[gids[2]] += (0 + 0.2 * torch.rand((n2, 1)).to(device)) * torch.randn((n2, D)).to(device)                       # :223
    smask = torch.Tensor([1, .1, .1]).to(device).view(1, 3) * torch.bernoulli(torch.ones(N) * 0.5).to(device).view(-1, 1)   # :226
    feats["jaw_params"] = feats["jaw_params"] + torch.randn(feats["jaw_params"].size()).to(device) * 0.2 * smask      # :227
    feats["jaw_params"][..., 0] = torch.clamp(feats["jaw_params"][..., 0], 0.0, 0.5)                                  # :228
    if use_eyelids:                                                                                                   # :231
        feats["eyelid_params"] += (-1 + 2 * torch.rand(size=feats["eyelid_params"].size()).to(device)) * 0.25         # :232
        feats["eyelid_params"] = torch.clamp(feats["eyelid_params"], 0.0, 1.0)                                        # :233
    ex[gids[3]] *= 0.0                                                                                                # :238
    ex[gids[3]] += (0 + 0.2 * torch.rand((n3, 1)).to(device)) * torch.randn((n3, D)).to(device)                       # :239
    feats["jaw_params"][gids[3]] *= 0.0                                                                               # :241
    feats["eyelid_params"][gids[3]] = torch.rand(size=feats["eyelid_params"][gids[3]].size()).to(device)              # :242
    feats = {k: v.detach() for k, v in feats.items()}                                                                 # :244-248
    return (feats, gids) if _return_groups else feats


def synth_inputs(B, E=50, S=300, seed=0):
    """encoder outputs of the size and spread the law test names: expression ~ 0.7 N(0,1), jaw = U * [.3, .02, .02], eyelid ~ U"""
    r = np.random.default_rng(seed)
    return dict(expression_params=(0.7 * r.standard_normal((B, E))).astype(np.float32),
                jaw_params=(r.uniform(size=(B, 3)) * np.array([.3, .02, .02])).astype(np.float32),
                eyelid_params=r.uniform(size=(B, 2)).astype(np.float32),
                shape_params=r.standard_normal((B, S)).astype(np.float32),
                pose_params=(0.1 * r.standard_normal((B, 3))).astype(np.float32),
                cam=(r.standard_normal((B, 3)) * 0.05 + np.array([8.0, 0.0, 0.0])).astype(np.float32))


def synth_templates(sizes=(1, 3, 7, 12, 5), width=50, seed=1):
    """{class name: float32 [n, width]} with unequal class sizes"""
    r = np.random.default_rng(seed)
    return {f"s{i}class{i}": (1.5 * r.standard_normal((n, width))).astype(np.float32) for i, n in enumerate(sizes)}


def ks_distance(a, b):
    """two-sample Kolmogorov-Smirnov distance sup |F_a - F_b| (ties handled: both CDFs are evaluated at every sample point)"""
    a, b = np.sort(np.asarray(a, dtype=np.float64)), np.sort(np.asarray(b, dtype=np.float64))
    pts = np.concatenate([a, b])
    return float(np.abs(np.searchsorted(a, pts, side="right") / len(a) - np.searchsorted(b, pts, side="right") / len(b)).max())
