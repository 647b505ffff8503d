"""PoseBank and PoseAdam -- the bundle adjustment's cameras as device tables (csrc/camera.hip, csrc/adam.hip).

The reference keeps one learnable ``Camera`` per training image and, per camera, Adam optimizers over its rotation, translation
and fov leaves (scene/cameras.py:95-110; train.py steps the rotation / translation pair under ``--opt_cam`` and the fovx / fovy
pair under ``--opt_intrinsic``, for the camera it rendered).  With ``PoseCamera`` and ``torch.optim.Adam`` that is, per rendered
camera, one chain launch each way and two to four optimizer steps over tensors of 4, 3, 1 and 1 floats.

``PoseBank`` holds the leaves of all N cameras in one ``(N,9)`` parameter (``delta_quaternion`` 0..3 | ``delta_translation`` 4..6 |
``fovx`` 7 | ``fovy`` 8) beside the ``(N,4)`` / ``(N,3)`` / ``(N,2)`` tables of the initial pose and the clip planes.  The cameras
of one step go through the chain in ONE launch each way (``bags_pose_bank_forward`` / ``bags_pose_bank_backward``), 16 per launch;
the backward writes the dense ``(N,9)`` gradient, rows that were not rendered as zeros.  ``PoseAdam`` is every camera's own Adam
over the three groups, stepped for the listed cameras only, in ONE launch per 16 cameras (``bags_pose_adam_step``); the step
counts, one per (camera, group), live on the host, where the row indices already are.  A bank row gets the bits
``PoseCamera`` gets from the single-camera kernel.  On the CPU the chain is ``PoseCamera``'s getters, row by row.
"""
from __future__ import annotations

import math
from typing import Optional, Sequence

import torch

from . import _lib as L
from .camera import PoseCamera, rotation_to_quaternion

_GROUPS = ("rotation", "translation", "fov")                   # columns 0..3, 4..6, 7..8 of a row


def _rows(op: str, rows, N: int):
    """``rows`` as a list of distinct Python ints in [0, N)."""
    if torch.is_tensor(rows):
        rows = rows.tolist()
    rows = [int(r) for r in rows]
    if not rows:
        raise ValueError(f"{op}: the row list is empty")
    seen = set()
    for r in rows:
        if not 0 <= r < N:
            raise ValueError(f"{op}: row {r} is not in [0, {N})")
        if r in seen:
            raise ValueError(f"{op}: row {r} is listed twice")
        seen.add(r)
    return rows


def _row_table(rows):
    return (L.C.c_int32 * L.MAX_POSE_ROWS)(*rows)


class _PoseBankChain(torch.autograd.Function):
    """The leaves table -> the four camera tensors of at most 16 rows (csrc/camera.hip's bank kernels)."""

    @staticmethod
    def forward(ctx, leaves, grot, gscale, q0, t0, near_far, rows):
        L.require("PoseBank.get_matrices", "leaves", leaves, gpu=True, f32=True, contiguous=True, host=" (a bank on the host uses PoseCamera's getters)")
        dev, N, n = leaves.device, leaves.shape[0], len(rows)

        def f32(t, count, name):
            if t is None:
                return None
            L.require("PoseBank.get_matrices", name, t)
            t = L.as_f32c(t.to(dev)).reshape(-1)
            if t.numel() != count:
                raise RuntimeError(f"PoseBank.get_matrices: {name}: expected {count} values, got {t.numel()}")
            return t
        for name, t in (("init_quaternion", q0), ("init_translation", t0), ("near_far", near_far)):
            L.require("PoseBank.get_matrices", name, t, f32=True, contiguous=True, on=leaves)
        ctx.save_for_backward(leaves)                          # its version is checked at backward: the adjoint re-reads the table
        keep = dict(leaves=L.as_f32c(leaves), grot=f32(grot, 9, "global_rotation"), gscale=f32(gscale, 1, "global_translation_scale"),
                    q0=q0, t0=t0, near_far=near_far)
        bank = L.BagsPoseBank(N, L.ptr(q0), L.ptr(t0), L.ptr(near_far), L.ptr(keep["leaves"]), L.ptr(keep["grot"]), L.ptr(keep["gscale"]),
                              n, _row_table(rows))
        out = torch.empty(n * 51, dtype=torch.float32, device=dev)
        V, M, K = (out[16 * n * i:16 * n * (i + 1)].view(n, 4, 4) for i in range(3))
        Cc = out[48 * n:].view(n, 3)
        L.call("bags_pose_bank_forward", dev, bank, V.data_ptr(), M.data_ptr(), K.data_ptr(), Cc.data_ptr())
        ctx.keep, ctx.bank = keep, bank
        ctx.shapes = (None if grot is None else grot.shape, None if gscale is None else gscale.shape)
        return V, M, K, Cc

    @staticmethod
    def backward(ctx, gV, gM, gK, gC):
        keep, bank = ctx.keep, ctx.bank
        ctx.saved_tensors                                      # raises if the leaves were stepped in place since the forward
        leaves = keep["leaves"]
        dev = leaves.device
        gV, gM, gK, gC = L.as_f32c(gV), L.as_f32c(gM), L.as_f32c(gK), L.as_f32c(gC)
        need = ctx.needs_input_grad
        want_grot = need[1] and keep["grot"] is not None
        want_gscale = need[2] and keep["gscale"] is not None
        g_leaves = torch.empty_like(leaves)                    # every element is written by the kernel: no fill launch
        g_align = torch.empty(10, dtype=torch.float32, device=dev)
        L.call("bags_pose_bank_backward", dev, bank, L.ptr(gV), L.ptr(gM), L.ptr(gK), L.ptr(gC), g_leaves.data_ptr(),
               g_align[0:9].data_ptr() if want_grot else None, g_align[9:10].data_ptr() if want_gscale else None)
        return (g_leaves if need[0] else None, g_align[0:9].reshape(ctx.shapes[0]) if want_grot else None,
                g_align[9:10].reshape(ctx.shapes[1]) if want_gscale else None, None, None, None, None)


class PoseBankCamera:
    """Row ``row`` of a ``PoseBank`` as ``render()`` sees a camera: the static image size and fov, and ``get_matrices``."""

    def __init__(self, bank: "PoseBank", row: int):
        self.bank, self.row = bank, int(row)
        self.image_width, self.image_height = bank.image_width[self.row], bank.image_height[self.row]
        self.FoVx, self.FoVy = bank.FoVx[self.row], bank.FoVy[self.row]

    def get_matrices(self, global_rotation: Optional[torch.Tensor] = None, global_translation_scale: Optional[torch.Tensor] = None):
        V, M, K, Cc = self.bank.get_matrices([self.row], global_rotation, global_translation_scale)
        return V[0], M[0], K[0], Cc[0]


def _per_camera(value, N: int, name: str, cast):
    if isinstance(value, (int, float)):
        return [cast(value)] * N
    value = [cast(v) for v in (value.tolist() if torch.is_tensor(value) else value)]
    if len(value) != N:
        raise ValueError(f"PoseBank: {name} has {len(value)} entries for {N} cameras")
    return value


class PoseBank(torch.nn.Module):
    """N learnable pinhole cameras.  ``R`` ``(N,3,3)`` camera-to-world rotations and ``T`` ``(N,3)`` world-to-camera translations as
    ``PoseCamera`` takes them; ``FoVx``, ``FoVy``, ``width``, ``height``, ``znear``, ``zfar`` each a scalar or one value per camera.
    Buffers ``init_quaternion`` ``(N,4)``, ``init_translation`` ``(N,3)``, ``near_far`` ``(N,2)``; the one parameter is ``leaves``
    ``(N,9)``.  The static fov and image size of every camera stay on the host (Python lists)."""

    def __init__(self, R, T, FoVx, FoVy, width, height, device="cpu", znear=0.01, zfar=100.0):
        R = torch.as_tensor(R, dtype=torch.float32).reshape(-1, 3, 3)
        N = R.shape[0]
        T = torch.as_tensor(T, dtype=torch.float32).reshape(N, 3)
        q0 = torch.stack([rotation_to_quaternion(R[i].t()) for i in range(N)])
        fovx, fovy = _per_camera(FoVx, N, "FoVx", float), _per_camera(FoVy, N, "FoVy", float)
        leaves = torch.zeros(N, L.POSE_LEAVES)
        leaves[:, 7], leaves[:, 8] = torch.tensor(fovx), torch.tensor(fovy)
        super().__init__()
        self._set_tables(q0, T, leaves, fovx, fovy, _per_camera(width, N, "width", int), _per_camera(height, N, "height", int),
                         _per_camera(znear, N, "znear", float), _per_camera(zfar, N, "zfar", float), torch.device(device))

    def _set_tables(self, q0, t0, leaves, fovx, fovy, width, height, znear, zfar, dev):
        if len(fovx) < 1:
            raise ValueError("PoseBank: no cameras")
        for i, (zn, zf) in enumerate(zip(znear, zfar)):
            if not 0.0 < zn < zf:
                raise ValueError(f"PoseBank: camera {i}: need 0 < znear < zfar (got {zn}, {zf})")
        self.FoVx, self.FoVy, self.image_width, self.image_height, self.znear, self.zfar = fovx, fovy, width, height, znear, zfar
        self.register_buffer("init_quaternion", q0.to(dev, torch.float32).contiguous())
        self.register_buffer("init_translation", t0.to(dev, torch.float32).contiguous())
        self.register_buffer("near_far", torch.tensor(list(zip(znear, zfar)), dtype=torch.float32).to(dev))
        self.leaves = torch.nn.Parameter(leaves.to(dev, torch.float32).contiguous())

    @classmethod
    def from_cameras(cls, cameras: Sequence[PoseCamera], device=None) -> "PoseBank":
        """A bank holding the state of ``cameras`` (``PoseCamera``), row i = ``cameras[i]``, on their device (or ``device``)."""
        cameras = list(cameras)
        if not cameras:
            raise ValueError("PoseBank: no cameras")
        dev = torch.device(device) if device is not None else cameras[0].delta_quaternion.device
        with torch.no_grad():
            q0 = torch.stack([c.init_quaternion.reshape(4) for c in cameras])
            t0 = torch.stack([c.init_translation.reshape(3) for c in cameras])
            leaves = torch.stack([torch.cat([c.delta_quaternion.reshape(4), c.delta_translation.reshape(3), c.learnable_fovx.reshape(1),
                                             c.learnable_fovy.reshape(1)]) for c in cameras])
        self = cls.__new__(cls)
        torch.nn.Module.__init__(self)
        self._set_tables(q0, t0, leaves, [float(c.FoVx) for c in cameras], [float(c.FoVy) for c in cameras],
                         [int(c.image_width) for c in cameras], [int(c.image_height) for c in cameras],
                         [float(c.znear) for c in cameras], [float(c.zfar) for c in cameras], dev)
        return self

    def __len__(self) -> int:
        return self.leaves.shape[0]

    def _host_camera(self, i: int) -> PoseCamera:
        """Row i as a ``PoseCamera`` whose leaves are views of ``self.leaves``: the host chain is that class's own getters."""
        c = PoseCamera.__new__(PoseCamera)
        torch.nn.Module.__init__(c)
        c.image_width, c.image_height, c.FoVx, c.FoVy = self.image_width[i], self.image_height[i], self.FoVx[i], self.FoVy[i]
        c.znear, c.zfar = self.znear[i], self.zfar[i]
        c.init_quaternion, c.init_translation = self.init_quaternion[i], self.init_translation[i].view(3, 1)
        c.last_row = torch.tensor([[0.0, 0.0, 0.0, 1.0]], device=self.leaves.device)
        row = self.leaves[i]
        c.delta_quaternion, c.delta_translation, c.learnable_fovx, c.learnable_fovy = row[0:4], row[4:7].view(3, 1), row[7], row[8]
        return c

    def get_matrices(self, rows, global_rotation: Optional[torch.Tensor] = None, global_translation_scale: Optional[torch.Tensor] = None):
        """(viewmatrix, projmatrix, intrinsic, campos) of the cameras ``rows``: ``(len(rows),4,4)`` x 3 and ``(len(rows),3)``,
        differentiable w.r.t. ``leaves`` and the global alignment.  On a GPU one launch each way per 16 rows."""
        rows = _rows("PoseBank.get_matrices", rows, len(self))
        if not self.leaves.is_cuda:
            per = [self._host_camera(i).get_matrices(global_rotation, global_translation_scale) for i in rows]
            return tuple(torch.stack([p[k] for p in per]) for k in range(4))
        parts = [_PoseBankChain.apply(self.leaves, global_rotation, global_translation_scale, self.init_quaternion, self.init_translation,
                                      self.near_far, rows[b:b + L.MAX_POSE_ROWS]) for b in range(0, len(rows), L.MAX_POSE_ROWS)]
        return parts[0] if len(parts) == 1 else tuple(torch.cat([p[k] for p in parts]) for k in range(4))

    def camera(self, i: int) -> PoseBankCamera:
        """Row i as the camera object ``render()`` and ``render_views()`` take."""
        return PoseBankCamera(self, _rows("PoseBank.camera", [i], len(self))[0])

    def export(self, i: int) -> PoseCamera:
        """A ``PoseCamera`` with row i's state (copies), on the bank's device: for checkpoints and the reference's camera lists."""
        i = _rows("PoseBank.export", [i], len(self))[0]
        c = PoseCamera(torch.eye(3), torch.zeros(3), self.FoVx[i], self.FoVy[i], self.image_width[i], self.image_height[i],
                       device=self.leaves.device, znear=self.znear[i], zfar=self.zfar[i])
        with torch.no_grad():
            row = self.leaves[i]
            c.init_quaternion.copy_(self.init_quaternion[i]); c.init_translation.copy_(self.init_translation[i].view(3, 1))
            c.delta_quaternion.copy_(row[0:4]); c.delta_translation.copy_(row[4:7].view(3, 1))
            c.learnable_fovx.copy_(row[7]); c.learnable_fovy.copy_(row[8])
        return c


class PoseAdam:
    """Every camera of ``bank`` has its own ``torch.optim.Adam`` over three groups -- rotation (columns 0..3 of its row),
    translation (4..6), fov (7..8) -- at ``lr_rotation``, ``lr_translation``, ``lr_fov``, stepped only when the camera is listed.
    ``exp_avg`` / ``exp_avg_sq`` are ``(N,9)`` device tables; ``step`` is ``(N,3)`` int64 on the host, one count per (camera,
    group).  The three rates are plain attributes read at every call: a per-iteration schedule is an assignment.  No amsgrad, no
    weight decay, no capturable state; there is no CPU fallback."""

    def __init__(self, bank: PoseBank, lr_rotation: float, lr_translation: float, lr_fov: float, betas=(0.9, 0.999), eps: float = 1e-8):
        if min(lr_rotation, lr_translation, lr_fov) < 0.0 or eps < 0.0 or not 0.0 <= betas[0] < 1.0 or not 0.0 <= betas[1] < 1.0:
            raise ValueError(f"PoseAdam: invalid hyper-parameters lr=({lr_rotation}, {lr_translation}, {lr_fov}), betas={betas}, eps={eps}")
        self.bank = bank
        self.lr_rotation, self.lr_translation, self.lr_fov = lr_rotation, lr_translation, lr_fov
        self.betas, self.eps = (float(betas[0]), float(betas[1])), float(eps)
        self.exp_avg = torch.zeros_like(bank.leaves, memory_format=torch.contiguous_format)
        self.exp_avg_sq = torch.zeros_like(bank.leaves, memory_format=torch.contiguous_format)
        self.step_count = torch.zeros(len(bank), 3, dtype=torch.int64)

    def zero_grad(self, set_to_none: bool = True) -> None:
        if self.bank.leaves.grad is not None:
            if set_to_none:
                self.bank.leaves.grad = None
            else:
                self.bank.leaves.grad.zero_()

    @torch.no_grad()
    def step(self, rows, rotation: bool = True, translation: bool = True, fov: bool = True) -> None:
        """One Adam step of the enabled groups of the cameras ``rows`` from ``bank.leaves.grad``; every other (camera, group) keeps
        parameters, moments and step count.  One launch per 16 rows."""
        p = self.bank.leaves
        rows = _rows("PoseAdam.step", rows, p.shape[0])
        g = p.grad
        if g is None:
            raise RuntimeError("PoseAdam.step: bank.leaves has no .grad (call backward() first)")
        arg = dict(gpu=True, f32=True, contiguous=True, host=" (use torch.optim.Adam on the host)")
        for name, t in (("bank.leaves", p), ("bank.leaves.grad", g), ("exp_avg", self.exp_avg), ("exp_avg_sq", self.exp_avg_sq)):
            L.require("PoseAdam.step", name, t, on=p, **arg)
            if t.shape != p.shape:
                raise RuntimeError(f"PoseAdam.step: {name} has shape {tuple(t.shape)}, the bank's leaves {tuple(p.shape)}")
        enabled = (bool(rotation), bool(translation), bool(fov))
        if not any(enabled):
            return
        lrs = (self.lr_rotation, self.lr_translation, self.lr_fov)
        beta1, beta2 = self.betas
        for b in range(0, len(rows), L.MAX_POSE_ROWS):
            part = rows[b:b + L.MAX_POSE_ROWS]
            args = L.BagsPoseAdamArgs(p.shape[0], len(part), p.data_ptr(), g.data_ptr(), self.exp_avg.data_ptr(), self.exp_avg_sq.data_ptr(),
                                      beta1, beta2, self.eps, _row_table(part))
            for v, r in enumerate(part):
                for k in range(3):
                    if not enabled[k]:
                        continue                               # zero-initialised: enabled = 0
                    self.step_count[r, k] += 1
                    step = int(self.step_count[r, k])
                    args.groups[v][k] = L.BagsPoseAdamGroup(1, float(lrs[k]) / (1.0 - beta1 ** step), math.sqrt(1.0 - beta2 ** step))
            L.call("bags_pose_adam_step", p.device, args)

    def state_dict(self) -> dict:
        return {"step": self.step_count.clone(), "exp_avg": self.exp_avg.clone(), "exp_avg_sq": self.exp_avg_sq.clone(),
                "lr": {n: getattr(self, "lr_" + n) for n in _GROUPS}, "betas": self.betas, "eps": self.eps}

    def load_state_dict(self, state: dict) -> None:
        shape = tuple(self.bank.leaves.shape)
        for name in ("exp_avg", "exp_avg_sq"):
            if tuple(state[name].shape) != shape:
                raise ValueError(f"PoseAdam.load_state_dict: {name} has shape {tuple(state[name].shape)}, the bank's leaves {shape}")
        if tuple(state["step"].shape) != (shape[0], 3):
            raise ValueError(f"PoseAdam.load_state_dict: step has shape {tuple(state['step'].shape)}, expected {(shape[0], 3)}")
        self.exp_avg.copy_(state["exp_avg"]); self.exp_avg_sq.copy_(state["exp_avg_sq"])
        self.step_count = state["step"].to("cpu", torch.int64).clone()
        for n in _GROUPS:
            setattr(self, "lr_" + n, state["lr"][n])
        self.betas, self.eps = (float(state["betas"][0]), float(state["betas"][1])), float(state["eps"])
