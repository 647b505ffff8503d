"""The named cases of the 3D smoothing filter's tests (bags_raster.filter_3D, csrc/filter3d.hip; the filtered activations of
csrc/activations.hip), built seeded on the CPU, and their float32 / float64 PyTorch references, computed once and shared.

A camera table is the first N of ``N_MAX`` cameras on a ring around the origin with mixed image sizes and focal lengths; a case is
``P_FULL`` world points (float32) placed for what its name says, a smaller cloud the first P rows of it.  Every candidate row is
tested in float64 against ALL ``N_MAX`` cameras and dropped if it sits closer to one of the five thresholds than ``MARGIN`` -- in
``tz``, or in ``px`` / ``W`` and ``py`` / ``H`` -- so that the float32 and the float64 statement take the same decisions;
``flips`` counts the rows where they still differ.
"""
import functools
import math

import torch

from bags_raster.filter3d import FAR, _decide_torch, filter_3D_torch

BLOCK = 256                                       # csrc/filter3d.hip: F3_BLOCK
P_FULL = 1000
SIZES = (1, BLOCK - 1, BLOCK, BLOCK + 1, 2 * BLOCK + 1, P_FULL)      # the block edges, two blocks and a tail, and the whole case
P_MAX_ROW = 2 * BLOCK + 1                         # max_last / max_first: 513 rows, the row holding dmax in the tail block / in block 0
NS = (1, 3, 17, 70)
N_MAX = NS[-1]
MARGIN = 1e-3
VARIANCE = 0.2
CASES = ("ring", "behind", "none_valid", "edge", "max_last", "max_first")
IMAGE_SIZES = ((64, 48), (80, 60), (50, 37), (128, 96), (33, 65))
F32, F64 = torch.float32, torch.float64


@functools.lru_cache(maxsize=None)
def cameras():
    """``(viewmatrices (N_MAX,4,4), intrinsics (N_MAX,4,4), sizes (N_MAX,2) int32)``, float32, row-vector convention: camera c sits
    on a ring of radius 3..5 at a height of -1..1, looks at the origin, and has image size ``IMAGE_SIZES[c % 5]`` with a vertical
    field of view of 35..75 degrees."""
    g = torch.Generator().manual_seed(70)
    V = torch.zeros(N_MAX, 4, 4, dtype=F64)
    K = torch.zeros(N_MAX, 4, 4, dtype=F64)
    wh = torch.zeros(N_MAX, 2, dtype=torch.int32)
    for c in range(N_MAX):
        ang = 2.0 * math.pi * (c * 0.381966 + 0.05 * torch.rand(1, generator=g, dtype=F64).item())          # golden-angle steps
        rad = 3.0 + 2.0 * torch.rand(1, generator=g, dtype=F64).item()
        centre = torch.tensor([rad * math.sin(ang), -1.0 + 2.0 * torch.rand(1, generator=g, dtype=F64).item(), -rad * math.cos(ang)], dtype=F64)
        fwd = -centre / centre.norm()
        right = torch.linalg.cross(torch.tensor([0.0, -1.0, 0.0], dtype=F64), fwd)
        right = right / right.norm()
        down = torch.linalg.cross(fwd, right)
        R = torch.stack([right, down, fwd], 1)                           # columns: the camera's axes in the world
        V[c, :3, :3] = R                                                 # row vector: t = p @ R - centre @ R
        V[c, 3, :3] = -(centre @ R)
        V[c, 3, 3] = 1.0
        W, H = IMAGE_SIZES[c % len(IMAGE_SIZES)]
        fovy = math.radians(35.0 + 40.0 * torch.rand(1, generator=g, dtype=F64).item())
        K[c, 1, 1] = 1.0 / math.tan(0.5 * fovy)                          # fy = k5 * H / 2
        K[c, 0, 0] = K[c, 1, 1] * H / W * (0.9 + 0.2 * torch.rand(1, generator=g, dtype=F64).item())      # fx: not quite square pixels
        K[c, 2, 2], K[c, 2, 3], K[c, 3, 2] = 1.0001, 1.0, -0.01
        wh[c, 0], wh[c, 1] = W, H
    return V.float(), K.float(), wh


def table(N):
    V, K, wh = cameras()
    return V[:N], K[:N], wh[:N]


def margins(xyz, N=N_MAX):
    """Per row, in float64 on the float32 inputs: the smallest distance to a threshold over the first N cameras, ``|tz - 0.2|`` and
    the four margin lines in units of W (H)."""
    V, K, wh = table(N)
    x = xyz.double()
    v, k = V.double().reshape(-1, 16), K.double().reshape(-1, 16)
    W, H = wh.double().unbind(1)
    t = [x[:, 0:1] * v[:, 0 + a] + x[:, 1:2] * v[:, 4 + a] + x[:, 2:3] * v[:, 8 + a] + v[:, 12 + a] for a in range(3)]
    px = t[0] / t[2] * (k[:, 0] * 0.5 * W) + 0.5 * W
    py = t[1] / t[2] * (k[:, 5] * 0.5 * H) + 0.5 * H
    m = torch.stack([(t[2] - 0.2).abs(), (px / W + 0.15).abs(), (px / W - 1.15).abs(), (py / H + 0.15).abs(), (py / H - 1.15).abs()], 0)
    return torch.nan_to_num(m, nan=1.0).amin(dim=0).amin(dim=1)


def _keep(cands, P=P_FULL):
    """The first P candidates (float32) that keep the decision margin against every camera of the full table."""
    cands = cands.float()
    ok = margins(cands) >= 1.5 * MARGIN                                  # (1.5: the test asserts MARGIN on what is kept)
    rows = cands[ok]
    assert rows.shape[0] >= P, (rows.shape[0], P)
    return rows[:P].contiguous()


def _blob(g, n):
    return 0.6 * torch.randn(n, 3, generator=g, dtype=F64)


def _above(g, n):
    """Points far above the ring: outside every camera's margin lines by a wide margin."""
    p = 0.3 * torch.randn(n, 3, generator=g, dtype=F64)
    p[:, 1] = -(40.0 + 5.0 * torch.rand(n, generator=g, dtype=F64))
    return p


def _beside_thresholds(g, n):
    """Candidate j sits beside threshold ``j % 5`` (tz = 0.2, px = -0.15 W, px = 1.15 W, py = -0.15 H, py = 1.15 H) of camera
    ``(j // 10) % 3``, on side ``(j // 5) % 2``, 2e-3 .. 2e-2 away (in tz, or in units of W / H)."""
    V, K, wh = (t.double() for t in cameras())
    out = torch.zeros(n, 3, dtype=F64)
    for j in range(n):
        c, which, side = (j // 10) % 3, j % 5, 1.0 if (j // 5) % 2 else -1.0
        u = side * (2e-3 + 1.8e-2 * torch.rand(1, generator=g, dtype=F64).item())
        W, H = wh[c, 0].item(), wh[c, 1].item()
        fx, fy = K[c, 0, 0].item() * 0.5 * W, K[c, 1, 1].item() * 0.5 * H
        a, b = (torch.rand(2, generator=g, dtype=F64) * 0.8 + 0.1).tolist()          # an inside position, in units of the image
        tz = 2.0 + 2.0 * torch.rand(1, generator=g, dtype=F64).item()
        px, py = a * W, b * H
        if which == 0:
            tz = 0.2 + u
        elif which == 1:
            px = (-0.15 + u) * W
        elif which == 2:
            px = (1.15 + u) * W
        elif which == 3:
            py = (-0.15 + u) * H
        else:
            py = (1.15 + u) * H
        t = torch.tensor([(px - 0.5 * W) / fx * tz, (py - 0.5 * H) / fy * tz, tz], dtype=F64)
        out[j] = (t - V[c, 3, :3]) @ V[c, :3, :3].t()
    return out


@functools.lru_cache(maxsize=None)
def points(name, N):
    """The case's ``(P,3)`` float32 world points under the first N cameras (only ``max_last`` / ``max_first`` depend on N)."""
    g = torch.Generator().manual_seed(1000 + CASES.index(name))
    if name == "ring":
        return _keep(_blob(g, 3 * P_FULL))
    if name == "behind":
        blob, above = _keep(_blob(g, 3 * P_FULL)), _keep(_above(g, 3 * P_FULL))
        hidden = torch.rand(P_FULL, generator=g) < 0.2
        hidden[:4] = torch.tensor([False, True, False, True])
        return torch.where(hidden[:, None], above, blob).contiguous()
    if name == "none_valid":
        return _keep(_above(g, 3 * P_FULL))
    if name == "edge":
        return _keep(_beside_thresholds(g, 4 * P_FULL))
    # max_last / max_first: the row that holds dmax goes to the end (the tail block) / to the front
    xyz = _keep(_blob(g, 3 * P_MAX_ROW), P_MAX_ROW)
    ref = _statement(xyz, N, F64)
    top = int(torch.where(ref["any"], ref["dist"], torch.full_like(ref["dist"], -1.0)).argmax())
    to = P_MAX_ROW - 1 if name == "max_last" else 0
    order = list(range(P_MAX_ROW))
    order[top], order[to] = order[to], order[top]
    return xyz[order].contiguous()


def sizes_of(name):
    return (P_MAX_ROW,) if name.startswith("max_") else SIZES


def _statement(xyz, N, dtype):
    V, K, wh = table(N)
    valid, tz, fx = _decide_torch(xyz.to(dtype), V.to(dtype), K.to(dtype), wh)
    far = torch.as_tensor(FAR, dtype=dtype)
    return dict(valid=valid, any=valid.any(dim=1), dist=torch.where(valid, tz, far).amin(dim=1), focal=fx.amax(), argfocal=int(fx.argmax()))


@functools.lru_cache(maxsize=None)
def decisions(name, N, dtype, P=None):
    """What the statement decided in ``dtype``: ``valid (P,N)``, ``any (P,)``, ``dist (P,)``, ``focal``, ``argfocal``."""
    xyz = points(name, N)
    return _statement(xyz[:P if P is not None else xyz.shape[0]], N, dtype)


@functools.lru_cache(maxsize=None)
def flips(name, N, P=None):
    """Rows whose set of valid cameras differs between the float32 and the float64 statement."""
    return (decisions(name, N, F32, P)["valid"] != decisions(name, N, F64, P)["valid"]).any(dim=1)


@functools.lru_cache(maxsize=None)
def reference(name, N, dtype, P=None):
    """``filter_3D_torch`` on the CPU in ``dtype`` on the first P rows: ``(P,1)``."""
    xyz = points(name, N)
    V, K, wh = table(N)
    return filter_3D_torch(xyz[:P if P is not None else xyz.shape[0]].to(dtype), V.to(dtype), K.to(dtype), wh, VARIANCE)


# ---------------------------------------------------------------------------------------------------- the filtered activations
K_SH = 4                                          # SH coefficients per Gaussian of the activation inputs (degree 1)
FILTERS = ("ring", "zero", "huge")
COTANGENTS = ("opacity", "scales", "both")


@functools.lru_cache(maxsize=None)
def raw(P):
    """Raw leaves of P Gaussians (float32, CPU): features_dc, features_rest, opacity, scaling, rotation."""
    g = torch.Generator().manual_seed(4000 + P)
    return dict(features_dc=torch.randn(P, 1, 3, generator=g), features_rest=0.1 * torch.randn(P, K_SH - 1, 3, generator=g),
                opacity=1.5 * torch.randn(P, 1, generator=g), scaling=math.log(0.05) + 0.7 * torch.randn(P, 3, generator=g),
                rotation=torch.randn(P, 4, generator=g))


@functools.lru_cache(maxsize=None)
def filter_values(kind, P):
    """``(P,1)`` float32: the `ring` case's filter under 17 cameras (4e-3 .. 1e-2, beside scales of about 0.05), zeros, or 1e3."""
    if kind == "ring":
        return reference("ring", 17, F32, P).clone()
    return torch.full((P, 1), 0.0 if kind == "zero" else 1e3)


@functools.lru_cache(maxsize=None)
def cotangents(P):
    g = torch.Generator().manual_seed(5000 + P)
    return dict(opacity=torch.randn(P, 1, generator=g, dtype=F64), scales=torch.randn(P, 3, generator=g, dtype=F64))


def by_hand_f64(kind, P, which):
    """The two formulas and their derivative written out in float64, no autograd: ``(opacity', scales', g_opacity_raw, g_scaling_raw)``
    under the cotangents named by ``which`` (a missing one counts as zero).

        s = exp(raw), s' = sqrt(s^2 + f^2), c = prod s_i / s'_i, sig = sigmoid(raw_o)
        g_raw_s_i = g_s'_i s_i^2 / s'_i + g_o' sig c f^2 / s'_i^2 ;  g_raw_o = g_o' c sig (1 - sig)"""
    r, f, ct = raw(P), filter_values(kind, P).double(), cotangents(P)
    g_o = ct["opacity"] if which in ("opacity", "both") else torch.zeros(P, 1, dtype=F64)
    g_s = ct["scales"] if which in ("scales", "both") else torch.zeros(P, 3, dtype=F64)
    s = torch.exp(r["scaling"].double())
    sp = torch.sqrt(s * s + f * f)
    c = (s / sp).prod(dim=1, keepdim=True)
    sig = 1.0 / (1.0 + torch.exp(-r["opacity"].double()))
    return sig * c, sp, g_o * c * sig * (1.0 - sig), g_s * s * s / sp + g_o * sig * c * f * f / (sp * sp)
