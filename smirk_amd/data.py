"""The trainer's batch preparation (reference: datasets/base_dataset.py:124-215 BaseDataset.prepare_data) on the MI355X.

    prep = BatchPreparer(image_size=224, scale=(1.2, 1.8), test=False, augment=AugmentConfig(), device='cuda')    # scale=1.6 with test=True (config: test_scale)
    batch = prep(frames, landmarks_fan, landmarks_mp)                    # one call = one batch: the reference's data_dict, stacked, on the device
    for batch in prep.run(sample_iter, batch_size=64): ...               # pinned staging + copy-in stream, depth 2, like VideoPipeline

Decoded uint8 BGR frames (any mix of resolutions) and their landmark arrays go in; `img`, `landmarks_fan`, `flag_landmarks_fan`, `landmarks_mp`, `mask` and
`img_mica` come out with the reference's shapes and dtypes.  Decoding and the landmark files stay with the caller.  The host validates in numpy, packs the frames
into one pinned byte buffer with a descriptor table and everything else into a second one, and uploads each with one copy; after that nothing synchronises,
allocates scratch or copies: three launches of libsmirk_hip.so on the deterministic path, seven on the training path, whatever N (smirk_amd/csrc/data.hip,
include/smirk_data.h).

The reference does this arithmetic with cv2, skimage and albumentations, none of which is on disk: parity with them is UNPINNED.  The law is this project's own,
written down function by function in tests/data_law.py after the documented behaviour of albumentations 1.3.0, OpenCV 4.9 and skimage 0.22, with these stated
deviations: ColorJitter applies brightness, contrast, saturation, hue in that fixed order (albumentations shuffles it); RandomGamma's exponent is a continuous
uniform (albumentations draws an integer percentage); ShiftScaleRotate resamples in float64 without cv2's 1/32-pixel coordinate quantisation; Lab and HSV are
computed in float64 without cv2's tables; with `landmarks_fan=None` `img_mica` is zeros (the reference fits a transform to all-zero points, which is undefined).
Random numbers follow the contract of smirk_amd.masking / augment: keyed by `torch.manual_seed` by default, pinned by `rng=PhiloxStream(seed, offset)` which
advances by `n_counters(N, S)` on the training path (the deterministic path draws nothing and leaves it alone); the draws are not numpy's or albumentations'
(layout: smirk_amd/csrc/data_rng.h).
"""
import ctypes as C
import math
from dataclasses import dataclass

import numpy as np
import torch

from . import _lib as L
from .masking import _rng

MICA_SIZE = L.DATA_MICA_SIZE
KEYS = ("img", "landmarks_fan", "flag_landmarks_fan", "landmarks_mp", "mask", "img_mica")
FRAME_COUNTERS = 8                                         # smirk_amd/csrc/data_rng.h DATA_FRAME_COUNTERS


def n_counters(N, S):
    """Philox counters one training-path call consumes (smirk_amd/csrc/data_rng.h): eight per frame on one stream id, one per crop pixel on another."""
    return int(N) * max(int(S) * int(S), FRAME_COUNTERS)


def load_mediapipe_indices(path="assets/mediapipe_landmark_embedding/mediapipe_landmark_embedding.npz"):
    """The 105 mediapipe points FLAME2020's mediapipe embedding has barycentric coordinates for (`landmark_indices` of the asset FLAME itself loads,
    cwd-relative like there): the rows prepare_data keeps (base_dataset.py:156)."""
    return np.asarray(np.load(path)["landmark_indices"]).astype(np.int64).ravel()


@dataclass
class AugmentConfig:
    """Probabilities and limits of the reference's A.Compose (base_dataset.py:41-52) at albumentations 1.3.0 defaults.  Set a probability to 0 or 1 to isolate a
    transform."""
    p_brightness_contrast: float = 0.5
    brightness_limit: float = 0.2
    contrast_limit: float = 0.2
    p_gamma: float = 0.5
    gamma_limit: tuple = (80.0, 120.0)
    p_color_jitter: float = 0.25
    jitter_brightness: float = 0.05
    jitter_contrast: float = 0.05
    jitter_saturation: float = 0.05
    jitter_hue: float = 0.05
    p_clahe: float = 0.255
    clahe_clip_limit: tuple = (1.0, 4.0)
    p_rgb_shift: float = 0.25
    rgb_shift_limit: float = 20.0
    p_blur: float = 0.1
    blur_limit: int = 7
    p_gauss_noise: float = 0.5
    noise_var_limit: tuple = (10.0, 50.0)
    p_shift_scale_rotate: float = 0.9
    shift_limit: float = 0.05
    scale_limit: float = 0.1
    rotate_limit: float = 10.0

    def probabilities(self):
        return (self.p_brightness_contrast, self.p_gamma, self.p_color_jitter, self.p_clahe, self.p_rgb_shift, self.p_blur, self.p_gauss_noise,
                self.p_shift_scale_rotate)

    def struct(self):
        """include/smirk_data.h SmirkDataAugment; ValueError for what the library would refuse"""
        a = L.SmirkDataAugment()
        for t, p in enumerate(self.probabilities()):
            if not 0.0 <= float(p) <= 1.0:
                raise ValueError(f"probability of {L.DATA_TRANSFORMS[t]} outside [0, 1]: {p}")
            a.p[t] = float(p)
        a.brightness_limit, a.contrast_limit = float(self.brightness_limit), float(self.contrast_limit)
        a.gamma_lo, a.gamma_hi = map(float, self.gamma_limit)
        a.cj_brightness, a.cj_contrast, a.cj_saturation, a.cj_hue = (float(self.jitter_brightness), float(self.jitter_contrast), float(self.jitter_saturation),
                                                                     float(self.jitter_hue))
        a.clahe_lo, a.clahe_hi = map(float, self.clahe_clip_limit)
        a.rgb_shift = float(self.rgb_shift_limit)
        a.noise_var_lo, a.noise_var_hi = map(float, self.noise_var_limit)
        a.shift_limit, a.scale_limit, a.rotate_limit = float(self.shift_limit), float(self.scale_limit), float(self.rotate_limit)
        a.blur_max = int(self.blur_limit)
        sym = dict(brightness_limit=1e6, contrast_limit=1e6, jitter_brightness=1.0, jitter_contrast=1.0, jitter_saturation=1.0, jitter_hue=0.5, rgb_shift_limit=255.0,
                   shift_limit=1.0, rotate_limit=360.0)
        for name, cap in sym.items():
            if not 0.0 <= float(getattr(self, name)) <= cap:
                raise ValueError(f"{name} outside [0, {cap}]: {getattr(self, name)}")
        if not 0.0 <= a.scale_limit < 1.0:
            raise ValueError(f"scale_limit outside [0, 1): {self.scale_limit}")
        for name, floor, (lo, hi) in (("gamma_limit", 0.0, (a.gamma_lo, a.gamma_hi)), ("clahe_clip_limit", 1.0, (a.clahe_lo, a.clahe_hi)),
                                      ("noise_var_limit", 0.0, (a.noise_var_lo, a.noise_var_hi))):
            if not (floor <= lo <= hi < math.inf) or (name == "gamma_limit" and lo <= 0.0):
                raise ValueError(f"{name}: expected {floor} <= lo <= hi, got {(lo, hi)}")
        if a.blur_max not in (3, 5, 7):
            raise ValueError(f"blur_limit must be 3, 5 or 7, got {self.blur_limit}")
        return a


def _align(n, a=256):
    return (n + a - 1) // a * a


class _Staged:
    """one batch validated and packed on the host: views into a slot's two pinned buffers"""
    __slots__ = ("N", "Lmax", "frames_bytes", "meta_bytes", "off")


class _Slot:
    def __init__(self):
        self.h_frames = self.h_meta = self.d_frames = self.d_meta = None
        self.ev_in = self.ev_done = None
        self.used = False

    def reserve(self, frames_bytes, meta_bytes, device):
        if self.ev_in is None:
            self.ev_in, self.ev_done = torch.cuda.Event(), torch.cuda.Event()
        if self.used:
            self.ev_in.synchronize()                       # the previous upload out of these pinned buffers (the only host wait, and it precedes the copies)
        if self.used and (self.h_frames.numel() < frames_bytes or self.h_meta.numel() < meta_bytes):
            self.ev_done.synchronize()                     # growing: the batch that still reads the old device buffers must have run
        if self.h_frames is None or self.h_frames.numel() < frames_bytes:
            self.h_frames = torch.empty(_align(frames_bytes, 1 << 20), dtype=torch.uint8).pin_memory()
            self.d_frames = torch.empty(self.h_frames.numel(), dtype=torch.uint8, device=device)
        if self.h_meta is None or self.h_meta.numel() < meta_bytes:
            self.h_meta = torch.empty(_align(meta_bytes, 1 << 16), dtype=torch.uint8).pin_memory()
            self.d_meta = torch.empty(self.h_meta.numel(), dtype=torch.uint8, device=device)


class BatchPreparer:
    """prepare_data for a whole batch on the device.

    image_size  S, a multiple of 8 (CLAHE's 8 x 8 tiles), at most 2040
    scale       (lo, hi) on the training path (config: train_scale_min / train_scale_max), one float with test=True (config: test_scale)
    test        True: the deterministic path (no augmentation, fixed scale)
    augment     AugmentConfig (training path only)
    mp_indices  the mediapipe rows that become `landmarks_mp`; default: load_mediapipe_indices() (the FLAME asset, cwd-relative)

    __call__(frames, landmarks_fan, landmarks_mp, rng=None) -> dict of device tensors
        frames          list of N uint8 [H_i, W_i, 3] BGR arrays; resolutions may differ
        landmarks_fan   list of [68, >= 2] arrays or None entries (None = the reference's flag_landmarks_fan False)
        landmarks_mp    list of [L_i, >= 2] arrays, max(mp_indices) < L_i <= 1024
        img [N,3,S,S] f32 | landmarks_fan [N,68,2] f32 | flag_landmarks_fan [N] bool | landmarks_mp [N,K,2] f32 | mask [N,1,S,S] f32 (1 outside the hull) |
        img_mica [N,3,112,112] f32
    ValueError: what numpy can see before anything is uploaded (dtypes, shapes, list lengths, non-finite landmarks, a landmark box with
    old_size * scale_min < 1, five ArcFace points without spread).  SmirkHipError: a device that is not the HIP device, or a refusal of the library."""

    def __init__(self, image_size=224, scale=(1.2, 1.8), test=False, augment=None, device="cuda", mp_indices=None, depth=2):
        self.S, self.test = int(image_size), bool(test)
        if self.S <= 0 or self.S % 8 or self.S > L.DATA_MAX_SIZE:
            raise ValueError(f"image_size must be a positive multiple of 8 up to {L.DATA_MAX_SIZE}, got {image_size}")
        if self.test:
            if isinstance(scale, (tuple, list)):
                raise ValueError("test=True takes one scale (config: test_scale), not a range")
            self.scale = (float(scale), float(scale))
        else:
            if not isinstance(scale, (tuple, list)) or len(scale) != 2:
                raise ValueError("test=False takes scale=(min, max)")
            self.scale = (float(scale[0]), float(scale[1]))
        if not (0.0 < self.scale[0] <= self.scale[1] < math.inf):
            raise ValueError(f"scale: expected 0 < min <= max, got {scale}")
        self.augment = (augment if augment is not None else AugmentConfig()) if not self.test else None
        self._aug = self.augment.struct() if self.augment is not None else None
        self.device = torch.device(device)
        if self.device.type != "cuda":
            raise L.SmirkHipError("smirk_amd runs on the MI355X HIP device only (no CPU fallback exists)")
        idx = load_mediapipe_indices() if mp_indices is None else np.asarray(mp_indices).astype(np.int64).ravel()
        if idx.size < 1 or idx.size > L.DATA_MAX_POINTS or idx.min() < 0 or idx.max() >= L.DATA_MAX_POINTS:
            raise ValueError("mp_indices: expected 1..1024 row numbers in [0, 1024)")
        self.mp_indices = idx
        self.depth = max(2, int(depth))                  # run() uploads batch i + 1 before batch i is enqueued: two slots at least
        self._slots = [_Slot() for _ in range(self.depth)]
        self._k = 0
        self._in_stream = None
        self._ws = L.Workspace()

    # ---- host side: validate, pack ---------------------------------------------------------------------------------------------------------------------------
    def _validate(self, frames, landmarks_fan, landmarks_mp):
        if not (len(frames) == len(landmarks_fan) == len(landmarks_mp)):
            raise ValueError(f"list lengths differ: {len(frames)} frames, {len(landmarks_fan)} landmarks_fan, {len(landmarks_mp)} landmarks_mp")
        if len(frames) == 0:
            raise ValueError("empty batch")
        need = int(self.mp_indices.max())
        fr, fan, mp = [], [], []
        for i, (f, lf, lm) in enumerate(zip(frames, landmarks_fan, landmarks_mp)):
            f = np.asarray(f)
            if f.dtype != np.uint8 or f.ndim != 3 or f.shape[2] != 3 or f.shape[0] < 1 or f.shape[1] < 1:
                raise ValueError(f"frame {i}: expected uint8 [H, W, 3] (decoded BGR), got {f.dtype} {f.shape}")
            lm = np.asarray(lm)
            if lm.ndim != 2 or lm.shape[1] < 2 or not np.issubdtype(lm.dtype, np.number):
                raise ValueError(f"landmarks_mp {i}: expected [L, >= 2], got {lm.shape}")
            if not need < lm.shape[0] <= L.DATA_MAX_POINTS:
                raise ValueError(f"landmarks_mp {i}: {lm.shape[0]} points, expected more than {need} (the largest mediapipe index) and at most {L.DATA_MAX_POINTS}")
            lm = lm[:, :2].astype(np.float64)
            if not np.isfinite(lm).all():
                raise ValueError(f"landmarks_mp {i}: non-finite coordinates")
            old_size = (lm[:, 0].max() - lm[:, 0].min() + lm[:, 1].max() - lm[:, 1].min()) / 2
            if not old_size * self.scale[0] >= 1.0:
                raise ValueError(f"landmarks_mp {i}: degenerate landmark box (old_size * scale_min = {old_size * self.scale[0]:.3g} < 1)")
            if lf is not None:
                lf = np.asarray(lf)
                if lf.ndim != 2 or lf.shape[0] != L.DATA_FAN_POINTS or lf.shape[1] < 2:
                    raise ValueError(f"landmarks_fan {i}: expected [68, >= 2] or None, got {lf.shape}")
                lf = lf[:, :2].astype(np.float64)
                if not np.isfinite(lf).all():
                    raise ValueError(f"landmarks_fan {i}: non-finite coordinates")
                five = np.stack([(lf[36] + lf[39]) / 2, (lf[42] + lf[45]) / 2, lf[32], lf[48], lf[54]])
                if not ((five - five.mean(0)) ** 2).sum() > 0.0:
                    raise ValueError(f"landmarks_fan {i}: the five ArcFace points coincide")
            fr.append(f); fan.append(lf); mp.append(lm)
        return fr, fan, mp

    def _stage(self, slot, checked):
        fr, fan, mp = checked
        N, K = len(fr), self.mp_indices.size
        Lmax = max(m.shape[0] for m in mp)
        offs, o = [], 0
        for f in fr:
            offs.append(o)
            o = _align(o + f.size, 16)
        st = _Staged()
        st.N, st.Lmax, st.frames_bytes = N, Lmax, o
        off, m = {}, 0
        for name, nbytes in (("table", N * C.sizeof(L.SmirkDataFrame)), ("mp", N * Lmax * 16), ("fan", N * L.DATA_FAN_POINTS * 16), ("n_mp", N * 4), ("index", K * 4),
                             ("flag", N)):
            off[name] = m
            m = _align(m + nbytes)
        st.off, st.meta_bytes = off, m
        slot.reserve(o, m, self.device)
        hf, hm = slot.h_frames.numpy(), slot.h_meta.numpy()
        table = hm[off["table"]:off["table"] + N * 16].view(np.dtype([("offset", "<u8"), ("H", "<i4"), ("W", "<i4")]))
        h_mp = hm[off["mp"]:off["mp"] + N * Lmax * 16].view(np.float64).reshape(N, Lmax, 2)
        h_fan = hm[off["fan"]:off["fan"] + N * 68 * 16].view(np.float64).reshape(N, 68, 2)
        h_n = hm[off["n_mp"]:off["n_mp"] + N * 4].view(np.int32)
        hm[off["index"]:off["index"] + K * 4].view(np.int32)[:] = self.mp_indices
        h_flag = hm[off["flag"]:off["flag"] + N]
        for i, f in enumerate(fr):
            hf[offs[i]:offs[i] + f.size] = f.reshape(-1)
            table[i] = (offs[i], f.shape[0], f.shape[1])
            h_mp[i, :mp[i].shape[0]] = mp[i]
            h_mp[i, mp[i].shape[0]:] = 0.0
            h_n[i] = mp[i].shape[0]
            h_fan[i] = 0.0 if fan[i] is None else fan[i]
            h_flag[i] = fan[i] is not None
        return st

    # ---- device side ---------------------------------------------------------------------------------------------------------------------------------------------
    def _upload(self, slot, st):
        slot.d_frames[:st.frames_bytes].copy_(slot.h_frames[:st.frames_bytes], non_blocking=True)
        slot.d_meta[:st.meta_bytes].copy_(slot.h_meta[:st.meta_bytes], non_blocking=True)

    def _enqueue(self, slot, st, rng):
        lib, dev, S, N = L.lib(), self.device, self.S, st.N
        train = 0 if self.test else 1
        K = self.mp_indices.size
        out = dict(img=torch.empty(N, 3, S, S, device=dev), landmarks_fan=torch.empty(N, L.DATA_FAN_POINTS, 2, device=dev),
                   flag_landmarks_fan=torch.empty(N, dtype=torch.bool, device=dev), landmarks_mp=torch.empty(N, K, 2, device=dev),
                   mask=torch.empty(N, 1, S, S, device=dev), img_mica=torch.empty(N, 3, MICA_SIZE, MICA_SIZE, device=dev))
        need = lib.smirk_data_workspace_bytes(N, S, train)
        if need == 0:
            raise L.SmirkHipError(f"smirk_data_workspace_bytes refused N={N}, S={S}")
        ws = self._ws.get(need, dev)
        wsp, meta, st_ptr = ws.data_ptr(), slot.d_meta.data_ptr(), L.stream_ptr()
        at = lambda name: C.c_void_p(meta + st.off[name])
        seed, off = _rng(n_counters(N, S), rng) if train else (0, 0)
        L.check(lib.smirk_data_params(at("mp"), at("n_mp"), st.Lmax, at("fan"), at("flag"), at("index"), K, N, S, self.scale[0], self.scale[1],
                                      C.byref(self._aug) if train else None, seed, off, L.ptr(out["landmarks_fan"]), L.ptr(out["landmarks_mp"]),
                                      L.ptr(out["flag_landmarks_fan"], torch.bool), C.c_void_p(wsp), ws.numel(), st_ptr))
        L.check(lib.smirk_data_crop(C.c_void_p(slot.d_frames.data_ptr()), st.frames_bytes, at("table"), N, S, train, None if train else L.ptr(out["img"]),
                                    L.ptr(out["img_mica"]), C.c_void_p(wsp), ws.numel(), st_ptr))
        pts = C.c_void_p(wsp + lib.smirk_data_hull_points_offset(N, S, train))
        hull = C.c_void_p(wsp + lib.smirk_data_hull_offset(N, S, train)) if train else L.ptr(out["mask"])
        L.check(lib.smirk_hull_mask(pts, N, st.Lmax, 2, S, S, hull, st_ptr))               # the existing entry of csrc/video.hip, on the truncated points
        if train:
            L.check(lib.smirk_data_stats(N, S, C.c_void_p(wsp), ws.numel(), st_ptr))
            L.check(lib.smirk_data_colour(N, S, C.c_void_p(wsp), ws.numel(), st_ptr))
            L.check(lib.smirk_data_finish(N, S, seed, off, L.ptr(out["img"]), L.ptr(out["mask"]), C.c_void_p(wsp), ws.numel(), st_ptr))
        return out

    def _next_slot(self):
        slot = self._slots[self._k % self.depth]
        self._k += 1
        return slot

    @torch.no_grad()
    def __call__(self, frames, landmarks_fan, landmarks_mp, rng=None):
        checked = self._validate(frames, landmarks_fan, landmarks_mp)              # numpy only: raises before the device is touched
        with torch.cuda.device(self.device):
            slot = self._next_slot()
            st = self._stage(slot, checked)
            cur = torch.cuda.current_stream(self.device)
            if slot.used:
                cur.wait_event(slot.ev_done)
            self._upload(slot, st)
            slot.ev_in.record(cur)
            out = self._enqueue(slot, st, rng)
            slot.ev_done.record(cur)
            slot.used = True
            return out

    @torch.no_grad()
    def run(self, sample_iter, batch_size=64, rng=None):
        """sample_iter: iterable of (frame, landmarks_fan or None, landmarks_mp).  Yields one batch dict per `batch_size` samples (the last one may be shorter), in
        order.  The upload of batch i + 1 runs on a copy-in stream while batch i computes on the current stream; nothing here waits for the device except the
        re-use of a slot's pinned buffers, `depth` batches later."""
        batch_size = int(batch_size)
        if batch_size < 1:
            raise ValueError("batch_size must be positive")
        with torch.cuda.device(self.device):
            if self._in_stream is None:
                self._in_stream = torch.cuda.Stream(device=self.device)
            cur = torch.cuda.current_stream(self.device)
            staged = None                                   # (slot, st) uploaded ahead

            def submit(samples):
                checked = self._validate([s[0] for s in samples], [s[1] for s in samples], [s[2] for s in samples])
                slot = self._next_slot()
                st = self._stage(slot, checked)
                with torch.cuda.stream(self._in_stream):
                    if slot.used:
                        self._in_stream.wait_event(slot.ev_done)      # the slot's device buffers: wait for ITS previous batch only
                    self._upload(slot, st)
                    slot.ev_in.record(self._in_stream)
                slot.used = True
                return slot, st

            def compute(slot, st):
                cur.wait_event(slot.ev_in)
                out = self._enqueue(slot, st, rng)
                slot.ev_done.record(cur)
                return out

            buf = []
            for sample in sample_iter:
                buf.append(sample)
                if len(buf) == batch_size:
                    nxt = submit(buf)
                    buf = []
                    if staged is not None:
                        yield compute(*staged)
                    staged = nxt
            if buf:
                nxt = submit(buf)
                if staged is not None:
                    yield compute(*staged)
                staged = nxt
            if staged is not None:
                yield compute(*staged)
