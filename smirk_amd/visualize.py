"""The reference trainer's visualisation sheet (train.py:64-67; base_trainer.py:130-224 `create_visualizations` + `save_visualizations`; utils.py:65-90) on the
device: the panels stay where the modules left them, one launch (three with landmarks) writes the finished uint8 sheet, one pinned download brings it to the host.

    vis = create_visualizations(batch, outputs, flame, renderer, base_encoder=..., mica=..., second_path=(rendered, masked, reconstructed, rendered_2))
    sheet = save_visualizations(vis, "sheet.png", show_landmarks=True, Ke=1)          # uint8 [H, W, 3], BGR like the array the reference hands to cv2.imwrite

The law, operation for operation in float32, is tests/visual_law.py (cv2 and torchvision are not available, so parity with them is unpinned: make_grid and the
radius-1 filled circle are restated there).  Deviations from the reference, all on inputs it does not produce:
  * a pixel outside [0, 1] on the landmark panel saturates; numpy's astype('uint8') would wrap;
  * a NaN pixel becomes 0;
  * a non-finite landmark is skipped; the reference's int() raises;
  * a set of columns whose grids differ in height is refused with ValueError before anything is launched (B == 1 together with a second-path panel is one: the
    reference's torch.cat raises on it).
Kernels: csrc/visual.hip; C ABI: include/smirk_visual.h; design and measurements: DESIGN.md §32.
"""
import ctypes as C

import numpy as np
import torch

from . import _lib as L

IMAGE_KEYS = ('img_mica', 'rendered_img_base', 'rendered_img', 'overlap_image', 'overlap_image_pixels', 'rendered_img_mica_zero', 'rendered_img_zero',
              'masked_1st_path', 'reconstructed_img', 'loss_img', '2nd_path')                      # base_trainer.py:147-151
LANDMARK_LAYERS = (('landmarks_mp', None), ('landmarks_mp_gt', None), ('landmarks_fan', 17), ('landmarks_fan_gt', 17))   # base_trainer.py:138-141, in drawing order
OVERLAP_WEIGHTS = (0.7, 0.3)                                                                       # base_trainer.py:134-135
LANDMARK_CENTRE = 112.0                                                                            # utils.py:68

_ws = L.Workspace()
_pinned = {}


def create_visualizations(batch, outputs, flame, renderer, base_encoder=None, mica=None, num_shape=300, second_path=None):
    """base_trainer.py:165-224 over the modules, on the device and under no_grad.  `outputs`: the dict `first_path` returns.  `base_encoder`: the frozen base model
    (without one, `outputs['base_output']` is used if first_path computed it).  `mica`: a smirk_amd.MICA when the config's mica_loss weight is positive (it needs the
    base output for the pose and camera it renders with, like the reference); `num_shape`: config.arch.num_shape.  `second_path`: the four [Ke * B, 3, H, W] batches of
    smirk_trainer.py:327-330 in that order, optionally followed by Ke; they stay four tensors, the sheet interleaves them by index.  `img_mica` stays at its
    112 x 112: the sheet resamples it.  Every tensor of the returned dict is on the device."""
    with torch.no_grad():
        img = batch['img']
        L.ptr(img)
        B = img.shape[0]
        zero_pose_cam = torch.tensor([7.0, 0.0, 0.0], device=img.device).unsqueeze(0).repeat(B, 1)
        vis = {'img': img, 'rendered_img': outputs['rendered_img'].detach()}
        base_output = base_encoder(img) if base_encoder is not None else outputs.get('base_output')
        if base_output is not None:
            flame_output_base = flame.forward(base_output)
            vis['rendered_img_base'] = renderer.forward(flame_output_base['vertices'], base_output['cam'])['rendered_img']
        flame_output_zero = flame.forward(outputs['encoder_output'], zero_expression=True, zero_pose=True)
        vis['rendered_img_zero'] = renderer.forward(flame_output_zero['vertices'], zero_pose_cam)['rendered_img']
        for key in ('reconstructed_img', 'masked_1st_path', 'loss_img'):
            if outputs.get(key) is not None:
                vis[key] = outputs[key].detach()
        if mica is not None:
            if base_output is None:
                raise ValueError("create_visualizations: the MICA render takes its pose and camera entries from the base model's output; pass base_encoder")
            mica_output = dict(base_output)
            mica_output['shape_params'] = mica(batch['img_mica'].reshape(-1, 3, 112, 112))['shape_params'][:, :num_shape]
            flame_output_mica = flame.forward(mica_output, zero_expression=True, zero_pose=True)
            vis['rendered_img_mica_zero'] = renderer.forward(flame_output_mica['vertices'], zero_pose_cam)['rendered_img']
            vis['img_mica'] = batch['img_mica'].reshape(-1, 3, 112, 112)
        if second_path is not None:
            panels = tuple(second_path)
            if len(panels) == 5:
                if panels[0].shape[0] != int(panels[4]) * B:
                    raise ValueError(f"create_visualizations: second_path batches of {panels[0].shape[0]} images are not Ke * B = {int(panels[4])} * {B}")
                panels = panels[:4]
            if len(panels) != 4 or any(not torch.is_tensor(t) or t.shape != panels[0].shape for t in panels):
                raise ValueError("create_visualizations: second_path is four tensors of one shape (rendered, masked, reconstructed, rendered_2), optionally followed by Ke")
            vis['2nd_path'] = tuple(t.detach() for t in panels)
        for key in ('landmarks_mp', 'landmarks_mp_gt', 'landmarks_fan', 'landmarks_fan_gt'):
            vis[key] = outputs[key].detach()
    return vis


def _shape(t, what):
    if not torch.is_tensor(t) or t.dim() != 4 or t.shape[1] not in (1, 3):
        raise ValueError(f"save_visualizations: {what} must be a tensor [N, 1 or 3, H, W], got {tuple(t.shape) if torch.is_tensor(t) else type(t).__name__}")
    return tuple(t.shape)


def sheet_layout(visualizations, show_landmarks=False, Ke=1):
    """The columns of the sheet in the reference's order (`img` first, then IMAGE_KEYS as far as present), from shapes alone: -> ([(sources, blend or None, nrow,
    carries the landmarks)], B, S, H).  Raises ValueError for what the sheet cannot show: panels of the wrong rank, channel or batch count, landmark arrays of the
    wrong shape, grids of unequal height.  Nothing is launched and no device is needed."""
    vis = visualizations
    img, Ke = vis['img'], int(Ke)
    B, _, S, Wimg = _shape(img, "'img'")
    if Wimg != S:
        raise ValueError(f"save_visualizations: 'img' must be square, got {tuple(img.shape)}")
    if Ke < 1:
        raise ValueError("save_visualizations: Ke must be at least 1")
    if not L.VISUAL_MIN_SIZE <= S <= L.VISUAL_MAX_SIZE:
        raise ValueError(f"save_visualizations: image size {S} outside {L.VISUAL_MIN_SIZE} .. {L.VISUAL_MAX_SIZE}")
    cols = [([img], None, 1, bool(show_landmarks))]
    overlap = all(k in vis for k in ('img', 'rendered_img', 'masked_1st_path'))                  # base_trainer.py:133
    for key in IMAGE_KEYS:
        if key in ('overlap_image', 'overlap_image_pixels'):
            if overlap:
                other = vis['rendered_img' if key == 'overlap_image' else 'masked_1st_path']
                if _shape(other, f"the panel blended into '{key}'") != tuple(img.shape):
                    raise ValueError(f"save_visualizations: '{key}' blends 'img' {tuple(img.shape)} with a panel of another shape {tuple(other.shape)}")
                cols.append(([img], other, 1, False))
        elif key == '2nd_path':
            if key in vis:
                panels = vis[key]
                if torch.is_tensor(panels) or len(panels) != 4:
                    raise ValueError("save_visualizations: '2nd_path' is the tuple of the four second-path batches (create_visualizations keeps them apart)")
                shapes = [_shape(t, "'2nd_path'") for t in panels]
                if any(s != shapes[0] for s in shapes) or shapes[0][0] != Ke * B:
                    raise ValueError(f"save_visualizations: '2nd_path' batches must each hold Ke * B = {Ke * B} images of one shape, got {shapes}")
                cols.append((list(panels), None, 4 * Ke, False))
        elif key in vis:
            if _shape(vis[key], f"'{key}'")[0] != B:
                raise ValueError(f"save_visualizations: '{key}' holds {vis[key].shape[0]} images, 'img' holds {B}")
            cols.append(([vis[key]], None, 1, False))
    if len(cols) > L.VISUAL_MAX_COLUMNS:
        raise ValueError(f"save_visualizations: {len(cols)} columns, at most {L.VISUAL_MAX_COLUMNS}")
    heights = set()
    for src, _, nrow, _ in cols:
        n = B * nrow if len(src) == 4 else B
        heights.add(S if n == 1 else -(-n // min(nrow, n)) * (S + L.VISUAL_PADDING) + L.VISUAL_PADDING)
    if len(heights) != 1:
        raise ValueError(f"save_visualizations: the columns' grids differ in height ({sorted(heights)}): torch.cat along the width refuses them "
                         "(B == 1 shows a panel without padding, a second-path panel always has it)")
    if show_landmarks:
        for key, first in LANDMARK_LAYERS:
            lm = vis[key]
            if not torch.is_tensor(lm) or lm.dim() != 3 or lm.shape[0] != B or lm.shape[2] != 2:
                raise ValueError(f"save_visualizations: '{key}' must be a tensor [{B}, points, 2], got {tuple(lm.shape) if torch.is_tensor(lm) else type(lm).__name__}")
            if (lm.shape[1] if first is None else min(first, lm.shape[1])) > L.VISUAL_MAX_POINTS:
                raise ValueError(f"save_visualizations: '{key}' draws {lm.shape[1]} points per frame, at most {L.VISUAL_MAX_POINTS}")
    return cols, B, S, heights.pop()


def plan_sheet(visualizations, show_landmarks=False, Ke=1):
    """sheet_layout, then the descriptors over the device pointers: -> (SmirkVisualColumn array, tensors to keep alive, B, S, H, W, bytes)"""
    layout, B, S, _ = sheet_layout(visualizations, show_landmarks, Ke)
    keep, cols = [], []
    for src, blend, nrow, marked in layout:
        src = [L.as_f32c(t.detach()) for t in src]
        blend = None if blend is None else L.as_f32c(blend.detach())
        c = L.SmirkVisualColumn()
        for k, t in enumerate(src):
            c.src[k] = L.ptr(t).value
        c.blend = None if blend is None else L.ptr(blend).value
        c.w_src, c.w_blend = OVERLAP_WEIGHTS if blend is not None else (0.0, 0.0)
        c.nsrc, c.channels, c.Hs, c.Ws, c.nrow, c.landmarks = len(src), src[0].shape[1], src[0].shape[2], src[0].shape[3], nrow, int(marked)
        keep += src + ([] if blend is None else [blend])
        cols.append(c)
    arr = (L.SmirkVisualColumn * len(cols))(*cols)
    H, W, nbytes = C.c_int32(), C.c_int32(), C.c_size_t()
    L.check(L.lib().smirk_visual_sheet_size(arr, len(cols), B, S, C.byref(H), C.byref(W), C.byref(nbytes)))
    return arr, keep, B, S, H.value, W.value, nbytes.value


def _dots(visualizations):
    d, keep = L.SmirkVisualDots(), []
    for layer, (key, first) in enumerate(LANDMARK_LAYERS):
        lm = L.as_f32c(visualizations[key].detach())
        d.lm[layer], d.rows[layer], d.npts[layer] = L.ptr(lm).value, lm.shape[1], lm.shape[1] if first is None else min(first, lm.shape[1])
        keep.append(lm)
    return d, keep


def render_sheet(visualizations, show_landmarks=False, Ke=1, bgr=True, landmark_centre=None):
    """The launches of the sheet on the current stream: -> (uint8 device tensor of the rounded byte count, H, W).  `landmark_centre`: where landmark 0 lands and the
    scale that takes [-1, 1] to the image, S / 2; the reference hard-codes 112 (utils.py:68), which is the default whatever S."""
    arr, keep, B, S, H, W, nbytes = plan_sheet(visualizations, show_landmarks, Ke)
    dev = keep[0].device
    lib, st = L.lib(), L.stream_ptr()
    ws, ws_bytes = None, 0
    if show_landmarks:
        dots, lms = _dots(visualizations)
        ws_bytes = lib.smirk_visual_workspace_bytes(B, S)
        ws = _ws.get(ws_bytes, dev)
        L.check(lib.smirk_visual_dots(C.byref(dots), B, S, LANDMARK_CENTRE if landmark_centre is None else float(landmark_centre), C.c_void_p(ws.data_ptr()), ws_bytes, st))
    sheet = torch.empty(nbytes, dtype=torch.uint8, device=dev)
    L.check(lib.smirk_visual_sheet(arr, len(arr), B, S, int(bool(bgr)), None if ws is None else C.c_void_p(ws.data_ptr()), ws_bytes, C.c_void_p(sheet.data_ptr()),
                                   nbytes, st))
    return sheet, H, W


def download_sheet(sheet, H, W):
    """One copy of the finished sheet into the pinned buffer cached for its byte count; -> a uint8 [H, W, 3] view of that buffer, valid until the next sheet of the
    same size is downloaded."""
    host = _pinned.get(sheet.numel())
    if host is None:
        host = _pinned[sheet.numel()] = torch.empty(sheet.numel(), dtype=torch.uint8).pin_memory()
    host.copy_(sheet, non_blocking=True)
    torch.cuda.current_stream(sheet.device).synchronize()
    return host.numpy()[:H * W * 3].reshape(H, W, 3)


def save_visualizations(visualizations, save_path=None, show_landmarks=False, Ke=1, bgr=True, encoder=None, return_sheet=True, quality=None):
    """base_trainer.py:130-162.  -> the sheet, uint8 [H, W, 3], BGR (what the reference hands to cv2.imwrite) or RGB with bgr=False; an array of its own, not the
    pinned buffer.  With `save_path` the file is written with PIL (ImportError where it is absent); encoding stays on the host.  CPU tensors raise SmirkHipError.
    encoder="hip" with a .jpg / .jpeg path encodes the sheet on the device instead (smirk_amd.jpeg, `quality` default 95 like cv2.imwrite): only the file's bytes are
    downloaded and written, and return_sheet=False skips the download of the sheet itself (-> None)."""
    if encoder not in (None, "hip"):
        raise ValueError(f"save_visualizations: encoder must be None (PIL on the host) or 'hip', got {encoder!r}")
    if encoder == "hip" and (save_path is None or not str(save_path).lower().endswith((".jpg", ".jpeg"))):
        raise ValueError("save_visualizations: encoder='hip' writes JPEG files: save_path must end in .jpg or .jpeg")
    if encoder is None and (quality is not None or not return_sheet):
        raise ValueError("save_visualizations: quality and return_sheet=False belong to encoder='hip'")
    sheet, H, W = render_sheet(visualizations, show_landmarks, Ke, bgr)
    if encoder == "hip":
        from .jpeg import DEFAULT_QUALITY, encode_jpeg
        data = encode_jpeg(sheet[:H * W * 3].view(1, H, W, 3), DEFAULT_QUALITY if quality is None else quality, bgr=bgr).to_host()[0]
        with open(save_path, "wb") as f:
            f.write(data)
        return download_sheet(sheet, H, W).copy() if return_sheet else None
    out = download_sheet(sheet, H, W).copy()
    if save_path is not None:
        from PIL import Image
        Image.fromarray(out[..., ::-1] if bgr else out).save(save_path)
    return out
