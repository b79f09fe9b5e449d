"""Baseline JPEG encoding of finished uint8 pictures on the device: what the reference leaves to cv2.imwrite (base_trainer.py:162, the visualisation sheet) and to
cv2.VideoWriter (demo_video.py:211-214, every grid).

    batch = encode_jpeg(images, quality=95)            # uint8 [B, H, W, 3] or [H, W, 3] on the device; four launches, nothing synchronises
    files = batch.to_host()                            # list of B bytes objects, each a complete JFIF file

Sequential DCT, 8 bit, YCbCr 4:2:0, the Annex K Huffman tables, restart intervals.  The arithmetic is integer throughout; tests/jpeg_law.py restates it and the
files equal the law's byte for byte.  Only the compressed bytes cross to the host.  Kernels: csrc/jpeg.hip; C ABI: include/smirk_jpeg.h; design and measurements:
DESIGN.md §34.
"""
import ctypes as C

import numpy as np
import torch

from . import _lib as L

DEFAULT_QUALITY = 95                  # cv2.imwrite's default
DEFAULT_RESTART_INTERVAL = 2          # MCUs per restart interval; the entropy stage runs one lane per interval.  Of 1, 2, 4, 8 the only one measured no slower
                                      # than 1 on both the sheet and the video grids (profiles/jpeg_times.txt)

_ws = L.Workspace()
_pinned = {}


def quant_tables(quality=DEFAULT_QUALITY):
    """-> uint8 [2, 64], natural order: the Annex K base tables under the IJG quality rule (host only)"""
    qt = L.JpegQuantTables()
    L.check(L.lib().smirk_jpeg_quant_tables(int(quality), C.byref(qt)))
    return np.ctypeslib.as_array(qt).copy()


class JpegBatch:
    """The files of one encode_jpeg call, still on the device: `stream` uint8 [bound] holds them back to back, `spans` int32 [B, 2] their (offset, length)."""

    def __init__(self, stream, spans, count):
        self.stream, self.spans, self.count = stream, spans, count

    def __len__(self):
        return self.count

    def to_host(self, stream=None):
        """One read-back of the 8 * B-byte span table, then one pinned download of exactly the files' bytes.  -> list of bytes.  `stream`: the stream the two copies
        run on (default: the current one); it must already be ordered after the encode."""
        dev = self.stream.device
        st = torch.cuda.current_stream(dev) if stream is None else stream
        with torch.cuda.stream(st):
            spans = self.spans.cpu().numpy().astype(np.int64)
            total = int(spans[-1, 0] + spans[-1, 1])
            host = _pinned.get(dev)
            if host is None or host.numel() < total:
                host = _pinned[dev] = torch.empty(max(total, 1 << 20), dtype=torch.uint8).pin_memory()
            host[:total].copy_(self.stream[:total], non_blocking=True)
            st.synchronize()
        raw = host.numpy()
        return [raw[o:o + n].tobytes() for o, n in spans]


def encode_jpeg(images, quality=DEFAULT_QUALITY, bgr=False, restart_interval=None):
    """uint8 [B, H, W, 3] or [H, W, 3] device tensor (RGB, or BGR with bgr=True) -> JpegBatch.  `restart_interval`: MCUs (16 x 16 pixels) per restart interval,
    default DEFAULT_RESTART_INTERVAL.  Enqueued on the current stream; nothing synchronises.  CPU tensors raise SmirkHipError, what the shapes show ValueError."""
    if not torch.is_tensor(images) or images.dtype != torch.uint8 or images.dim() not in (3, 4) or images.shape[-1] != 3:
        raise ValueError(f"encode_jpeg: images must be a uint8 tensor [B, H, W, 3] or [H, W, 3], got "
                         f"{(tuple(images.shape), images.dtype) if torch.is_tensor(images) else type(images).__name__}")
    if images.dim() == 3:
        images = images.unsqueeze(0)
    B, H, W, _ = images.shape
    R = DEFAULT_RESTART_INTERVAL if restart_interval is None else int(restart_interval)
    if B < 1 or not (1 <= H <= L.JPEG_MAX_DIM and 1 <= W <= L.JPEG_MAX_DIM):
        raise ValueError(f"encode_jpeg: a batch of {B} pictures of {H} x {W}: B must be at least 1, H and W within 1 .. {L.JPEG_MAX_DIM}")
    if not 1 <= int(quality) <= 100:
        raise ValueError(f"encode_jpeg: quality {quality} outside 1 .. 100")
    if R < 1:
        raise ValueError(f"encode_jpeg: restart interval {R} below 1")
    lib = L.lib()
    bound = lib.smirk_jpeg_max_bytes(B, H, W, R)
    if B * H * W * 3 >= 1 << 31 or bound >= 1 << 31:
        raise ValueError(f"encode_jpeg: {B} pictures of {H} x {W} hold {B * H * W * 3} bytes and could reach {bound} encoded; both must stay below 2^31: "
                         "encode the batch in parts")
    if not images.is_contiguous() and images.is_cuda:
        images = images.contiguous()
    if images.is_cuda and images.data_ptr() % 16:
        images = images.clone()
    src = L.ptr(images, torch.uint8)
    qt = L.JpegQuantTables()
    L.check(lib.smirk_jpeg_quant_tables(int(quality), C.byref(qt)))
    dev = images.device
    ws_bytes = lib.smirk_jpeg_workspace_bytes(B, H, W, R)
    ws = _ws.get(ws_bytes, dev)
    out = torch.empty(bound, dtype=torch.uint8, device=dev)
    spans = torch.empty((B, 2), dtype=torch.int32, device=dev)
    L.check(lib.smirk_jpeg_encode_u8(src, B, H, W, int(bool(bgr)), C.byref(qt), R, C.c_void_p(ws.data_ptr()), ws_bytes, C.c_void_p(out.data_ptr()), bound,
                                     C.c_void_p(spans.data_ptr()), L.stream_ptr()))
    return JpegBatch(out, spans, B)
