"""Image-space distortion resampling of the rendered image (utils/util_distortion.py:271-311, the ``apply2gt == False``
branch of ``apply_distortion``; call site train.py:255-263).

``resample_image``        the HIP kernels of csrc/resample.hip (``bags_resample_forward`` / ``bags_resample_backward``):
                          control-flow upsample + grid_sample + centre crop + mask in one pass each way. GPU only.
``resample_image_torch``  the same pipeline with the PyTorch calls the reference makes (any device); used on the host.

The cubemap stitch of the large-FoV mode (utils/cubemap_utils.py:181-186,219-288): the faces ``render_views`` returns, warped
into the distorted image and stitched.
``resample_faces``        the HIP kernels of csrc/resample_faces.hip: one pass each way over the output pixels. GPU only.
``resample_faces_torch``  the same function in plain PyTorch (any device and dtype); replays a given face map.
``cube_face_matrices``    the rotations of the five faces and the matrices the stitch takes, from one place.
"""
from __future__ import annotations

import ctypes
from typing import Optional, Sequence, Tuple

import torch
import torch.nn.functional as F

from . import _lib as L


def center_crop(t: torch.Tensor, th: int, tw: int) -> torch.Tensor:
    """(N,C,H,W) -> (N,C,th,tw): the reference crops with a second grid_sample on an integer grid
    (utils/util_distortion.py:58-77)."""
    _, _, H, W = t.shape
    sy, sx = (H - th) // 2, (W - tw) // 2
    gy, gx = torch.meshgrid(torch.linspace(sy, sy + th - 1, th), torch.linspace(sx, sx + tw - 1, tw), indexing="ij")
    grid = torch.stack((gx, gy), 2).unsqueeze(0).to(t.device)
    grid = 2.0 * grid / torch.tensor([W - 1, H - 1], device=t.device, dtype=grid.dtype) - 1.0
    return F.grid_sample(t, grid.expand(t.shape[0], th, tw, 2).to(t.dtype), align_corners=True)


def resample_image_torch(image: torch.Tensor, ctrl_flow: torch.Tensor, flow_hw: Tuple[int, int], crop_hw: Tuple[int, int]):
    flow = ctrl_flow
    if tuple(flow.shape[:2]) != tuple(flow_hw):
        flow = F.interpolate(flow.permute(2, 0, 1).unsqueeze(0), size=tuple(flow_hw), mode="bilinear",
                             align_corners=False).permute(0, 2, 3, 1).squeeze(0)
    img = F.grid_sample(image.unsqueeze(0), flow.unsqueeze(0), mode="bilinear", padding_mode="zeros", align_corners=True)
    img = center_crop(img, crop_hw[0], crop_hw[1]).squeeze(0)
    mask = (~((img[0] == 0.0) & (img[1] == 0.0)).unsqueeze(0)).float()
    return img, mask


class _Resample(torch.autograd.Function):
    @staticmethod
    def forward(ctx, image, ctrl_flow, flow_hw, crop_hw):
        for name, t in (("image", image), ("ctrl_flow", ctrl_flow)):
            L.require("resample_image", name, t, gpu=True, host=" (use resample_image_torch on the host)")
        if image.dim() != 3 or ctrl_flow.dim() != 3 or ctrl_flow.shape[2] != 2:
            raise RuntimeError(f"resample_image: expected image (C,H,W) and flow (h,w,2), got {tuple(image.shape)}, {tuple(ctrl_flow.shape)}")
        img, ctl = L.as_f32c(image), L.as_f32c(ctrl_flow)
        Cn, H, W = img.shape
        h, w = ctl.shape[:2]
        Hf, Wf = int(flow_hw[0]), int(flow_hw[1])
        Hc, Wc = int(crop_hw[0]), int(crop_hw[1])
        out = torch.empty(Cn, Hc, Wc, dtype=torch.float32, device=img.device)
        mask = torch.empty(1, Hc, Wc, dtype=torch.float32, device=img.device)
        L.call("bags_resample_forward", img.device, img.data_ptr(), Cn, H, W, ctl.data_ptr(), h, w, Hf, Wf, Hc, Wc, out.data_ptr(),
               mask.data_ptr(), None)
        ctx.save_for_backward(img, ctl)
        ctx.dims = (Cn, H, W, h, w, Hf, Wf, Hc, Wc)
        ctx.mark_non_differentiable(mask)
        return out, mask

    @staticmethod
    def backward(ctx, g_out, _g_mask):
        img, ctl = ctx.saved_tensors
        Cn, H, W, h, w, Hf, Wf, Hc, Wc = ctx.dims
        g_out = L.as_f32c(g_out)
        g_img = torch.empty_like(img) if ctx.needs_input_grad[0] else None
        g_ctl = torch.empty_like(ctl) if ctx.needs_input_grad[1] else None
        ws = L.workspace(L.load().bags_resample_workspace_size(H, W, Hc, Wc), img.device)
        L.call("bags_resample_backward", img.device, img.data_ptr(), Cn, H, W, ctl.data_ptr(), h, w, Hf, Wf, Hc, Wc, g_out.data_ptr(),
               ws.data_ptr(), ws.numel(), L.ptr(g_img), L.ptr(g_ctl))
        return g_img, g_ctl, None, None


def resample_image(image: torch.Tensor, ctrl_flow: torch.Tensor, flow_hw: Tuple[int, int], crop_hw: Tuple[int, int]):
    """(warped image (C,Hc,Wc), mask (1,Hc,Wc)); gradients reach ``image`` (the rasterizer) and ``ctrl_flow`` (the lens net)."""
    return _Resample.apply(image, ctrl_flow, tuple(flow_hw), tuple(crop_hw))


# ------------------------------------------------------------------------------------------------ cubemap stitch
def cube_face_matrices(tan_front, tan_face: float = 1.0):
    """``(R (5,3,3), M (5,3,3))``, float64, for the faces front, left, right, up, down of a cubemap; x right, y down, z forward.

    ``R[f]`` rotates a ray of the front camera into face ``f``'s camera frame: the world-to-camera rotation of sub-camera ``f`` is
    ``R[f] @ R_front`` (same centre), so a caller builds its four sub-cameras and the stitch from this one place.
    ``M[f] = diag(1/tan_face, 1/tan_face, 1) @ R[f] @ diag(tx_0, ty_0, 1)`` is what ``resample_faces`` takes: ``tan_front`` is the
    front camera's ``(tan(fovx/2), tan(fovy/2))`` (one number: both), for which the control flow is meant; ``tan_face`` the
    tangent of every face's half field of view (1.0: 90 degree faces that tile the cube exactly; more: overlapping faces)."""
    tx0, ty0 = (tan_front, tan_front) if isinstance(tan_front, (int, float)) else (float(tan_front[0]), float(tan_front[1]))
    R = torch.tensor([[[1, 0, 0], [0, 1, 0], [0, 0, 1]],        # front
                      [[0, 0, 1], [0, 1, 0], [-1, 0, 0]],       # left:  -x of the front frame becomes +z
                      [[0, 0, -1], [0, 1, 0], [1, 0, 0]],       # right: +x becomes +z
                      [[1, 0, 0], [0, 0, 1], [0, -1, 0]],       # up:    -y becomes +z
                      [[1, 0, 0], [0, 0, -1], [0, 1, 0]]],      # down:  +y becomes +z
                     dtype=torch.float64)
    D0 = torch.diag(torch.tensor([tx0, ty0, 1.0], dtype=torch.float64))
    Df = torch.diag(torch.tensor([1.0 / tan_face, 1.0 / tan_face, 1.0], dtype=torch.float64))
    return R, Df @ R @ D0


def _host_mats(mats, n_faces: int):
    m = torch.as_tensor(mats, dtype=torch.float64, device="cpu") if not isinstance(mats, torch.Tensor) else mats.detach().to("cpu", torch.float64)
    if tuple(m.shape) != (n_faces, 3, 3):
        raise RuntimeError(f"resample_faces: expected mats ({n_faces},3,3) for {n_faces} faces, got {tuple(m.shape)}")
    return m


def resample_faces_torch(faces: Sequence[torch.Tensor], ctrl_flow: torch.Tensor, mats, flow_hw: Tuple[int, int], crop_hw: Tuple[int, int],
                         face_index: Optional[torch.Tensor] = None):
    """``resample_faces`` in plain PyTorch, in ``ctrl_flow``'s dtype, on its device: interpolate, integer crop, per pixel
    ``(a, b, c) = M_f (gx, gy, 1)``, ``u = a/c``, ``v = b/c``, then ``grid_sample`` of every face times ``(face_index == f)``.
    With ``face_index`` given the choice is taken from that map (a replay: nothing is decided); otherwise a pixel belongs to the
    first face with ``c > 0 and |u| <= 1 and |v| <= 1``.  Returns ``(image (C,Hc,Wc), face_index (Hc,Wc) int8)``."""
    M = _host_mats(mats, len(faces)).to(ctrl_flow.device, ctrl_flow.dtype)
    flow = ctrl_flow
    if tuple(flow.shape[:2]) != tuple(flow_hw):
        flow = F.interpolate(flow.permute(2, 0, 1).unsqueeze(0), size=tuple(flow_hw), mode="bilinear",
                             align_corners=False).squeeze(0).permute(1, 2, 0)
    Hc, Wc = int(crop_hw[0]), int(crop_hw[1])
    sy, sx = (flow.shape[0] - Hc) // 2, (flow.shape[1] - Wc) // 2
    g = flow[sy:sy + Hc, sx:sx + Wc]
    abc = torch.einsum("fij,hwj->fhwi", M, torch.cat([g, torch.ones_like(g[..., :1])], -1))
    c = abc[..., 2]
    cd = torch.where(c == 0, torch.ones_like(c), c)          # c == 0 is never valid (c > 0 is asked for); keeps autograd's 0 / c finite
    u, v = abc[..., 0] / cd, abc[..., 1] / cd
    if face_index is None:
        valid = (c > 0) & (u.abs() <= 1) & (v.abs() <= 1)
        idx = torch.full((Hc, Wc), -1, dtype=torch.int8, device=g.device)
        for f in reversed(range(len(faces))):
            idx = torch.where(valid[f], torch.full_like(idx, f), idx)
    else:
        idx = face_index.to(g.device)
    out = None
    for f, face in enumerate(faces):
        own = idx == f
        # the coordinates of pixels that are not this face's are never used: keep them finite and harmless for grid_sample
        grid = torch.where(own.unsqueeze(-1), torch.stack([u[f], v[f]], -1), torch.zeros_like(g)).unsqueeze(0)
        s = F.grid_sample(face.to(g.dtype).unsqueeze(0), grid, mode="bilinear", padding_mode="zeros", align_corners=True)[0]
        s = s * own.to(s.dtype)
        out = s if out is None else out + s
    return out, idx.to(torch.int8)


class _ResampleFaces(torch.autograd.Function):
    @staticmethod
    def forward(ctx, ctrl_flow, mats, flow_hw, crop_hw, *faces):
        for i, t in enumerate(faces):
            L.require("resample_faces", f"faces[{i}]", t, gpu=True, on=faces[0], host=" (use resample_faces_torch on the host)")
        L.require("resample_faces", "ctrl_flow", ctrl_flow, gpu=True, on=faces[0], host=" (use resample_faces_torch on the host)")
        if ctrl_flow.dim() != 3 or ctrl_flow.shape[2] != 2 or any(t.dim() != 3 or t.shape != faces[0].shape for t in faces):
            raise RuntimeError(f"resample_faces: expected faces of one shape (C,H,W) and flow (h,w,2), got "
                               f"{[tuple(t.shape) for t in faces]}, {tuple(ctrl_flow.shape)}")
        imgs, ctl = [L.as_f32c(t) for t in faces], L.as_f32c(ctrl_flow)
        Cn, H, W = imgs[0].shape
        h, w = ctl.shape[:2]
        Hf, Wf, Hc, Wc = int(flow_hw[0]), int(flow_hw[1]), int(crop_hw[0]), int(crop_hw[1])
        fs = L.BagsFaces(len(imgs), Cn, H, W)
        for i, t in enumerate(imgs):
            fs.image[i] = t.data_ptr()
        ctypes.memmove(fs.mats, (ctypes.c_float * len(mats))(*mats), 4 * len(mats))       # the F x 9 floats in one go, row-major
        out = torch.empty(Cn, Hc, Wc, dtype=torch.float32, device=ctl.device)
        index = torch.empty(Hc, Wc, dtype=torch.int8, device=ctl.device)
        L.call("bags_resample_faces_forward", ctl.device, fs, ctl.data_ptr(), h, w, Hf, Wf, Hc, Wc, out.data_ptr(), index.data_ptr())
        ctx.save_for_backward(ctl, index, *imgs)
        ctx.fs, ctx.dims = fs, (h, w, Hf, Wf, Hc, Wc)
        ctx.mark_non_differentiable(index)
        ctx.set_materialize_grads(False)        # or every backward would fill an (Hc,Wc) int8 of zeros for the map's cotangent
        return out, index

    @staticmethod
    def backward(ctx, g_out, _g_index):
        ctl, index, *imgs = ctx.saved_tensors
        h, w, Hf, Wf, Hc, Wc = ctx.dims
        fs = ctx.fs
        if g_out is None:                       # the image is not on the path to the loss
            return (None,) * (4 + len(imgs))
        g_out = L.as_f32c(g_out)
        g_ctl = torch.empty_like(ctl) if ctx.needs_input_grad[0] else None
        g_imgs = [torch.empty_like(t) if ctx.needs_input_grad[4 + i] else None for i, t in enumerate(imgs)]
        ws = L.workspace(L.load().bags_resample_faces_workspace_size(fs.n_faces, fs.H, fs.W, Hc, Wc), ctl.device)
        L.call("bags_resample_faces_backward", ctl.device, fs, ctl.data_ptr(), h, w, Hf, Wf, Hc, Wc, index.data_ptr(), g_out.data_ptr(),
               ws.data_ptr(), ws.numel(), L.ptr_table(g_imgs + [None] * (L.MAX_FACES - len(g_imgs))), L.ptr(g_ctl))
        return (g_ctl, None, None, None, *g_imgs)


def resample_faces(faces: Sequence[torch.Tensor], ctrl_flow: torch.Tensor, mats, flow_hw: Tuple[int, int], crop_hw: Tuple[int, int]):
    """Warp and stitch the faces of a cubemap in one pass: ``(image (C,Hc,Wc), face_index (Hc,Wc) int8)``.

    ``faces``: up to 8 tensors ``(C,Hs,Ws)``, ``C <= 4``, of one shape -- the images ``render_views`` returns, as they are (no
    ``torch.stack``).  ``ctrl_flow (h,w,2)``, ``flow_hw`` and ``crop_hw`` are ``resample_image``'s: the lens network's output on
    the control grid in ``grid_sample`` coordinates of the FRONT image, upsampled as ``F.interpolate(align_corners=False)`` does and
    cropped by exact integer indexing.  ``mats (F,3,3)`` (``cube_face_matrices``) are host numbers and are not differentiated.
    Per output pixel the flow is projected onto every face, ``(a, b, c) = M_f (gx, gy, 1)``, ``u = a/c``, ``v = b/c``; the pixel
    belongs to the first face in list order with ``c > 0 and |u| <= 1 and |v| <= 1`` and is its bilinear sample at ``(u, v)``
    (``grid_sample``, ``align_corners=True``); with no such face it is 0 in every channel and ``face_index`` is -1.

    The coverage mask is ``face_index >= 0`` -- NOT ``resample_image``'s ``(img[0] == 0) & (img[1] == 0)`` test, which also
    masks covered pixels that happen to be black.  Gradients reach every face (the rasterizer) and ``ctrl_flow`` (the lens
    net, through ``u = a/c``, ``v = b/c``); the choice of face is piecewise constant, the backward replays it from
    ``face_index``, and nothing flows to ``mats``.  Both gradients are bitwise reproducible."""
    faces = tuple(faces)
    if not 1 <= len(faces) <= L.MAX_FACES:
        raise RuntimeError(f"resample_faces: 1..{L.MAX_FACES} faces, got {len(faces)}")
    m = _host_mats(mats, len(faces))
    return _ResampleFaces.apply(ctrl_flow, tuple(m.reshape(-1).tolist()), tuple(flow_hw), tuple(crop_hw), *faces)
