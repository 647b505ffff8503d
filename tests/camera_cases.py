"""Edge-of-pose-space cases, the float64 reference and the measured bar of the fused camera chain (csrc/camera.hip) -- CPU only, so
that tests/test_camera_cases_cpu.py can check the generator and the reference without a GPU before tests/test_camera_gpu.py judges
the kernel with them.

``make_case(name)``            the inputs of one named case and four seeded cotangents, float64 CPU tensors whose values are all
                               float32 numbers: the kernel's float32 cast of them loses nothing, so every error is arithmetic.
``chain(inputs, dtype, on)``   ``PoseCamera``'s own four getters in ``dtype`` on the CPU: the four tensors and, for the loss
                               ``sum_i <cot_i, out_i>`` over the cotangents switched ``on``, the gradient to every present leaf.
``reference(name, on)``        the float64 chain, ``err32`` (what the float32 chain loses against it) and the bars.

Bar (the rule of tests/loss_cases.py and tests/test_sh_colors_gpu.py): the kernel's error against the float64 chain -- each of the
four tensors by max-abs, each gradient by relative L2 -- is at most FACTOR x the error of the project's float32 PyTorch chain on the
same input, and never asked to be below FLOOR = 16 float32 epsilons (relative for a gradient, times the tensor's max-abs for a value):
the reordering slack of the 4x4 products.  Nothing in the bar comes from the kernel.  A gradient whose float64 norm is exactly zero
has no bar (None): it is compared for exact zeros.
"""
import functools
import math

import torch

from bags_raster import camera as cam

FACTOR = 4.0
FLOOR = 16 * torch.finfo(torch.float32).eps
VALUES = ("viewmatrix", "projmatrix", "intrinsic", "campos")
LEAVES = ("dq", "dt", "fovx", "fovy", "grot", "gscale")
ALL_ON = (True, True, True, True)
MAX_CANCELLATION = 4.0

CASES = ("benign", "long_quaternion", "short_quaternion", "half_turn_x", "half_turn_y", "half_turn_z", "identity", "far_translation",
         "zero_translation", "narrow_fov", "wide_fov", "unequal_fov", "near_far", "skewed_alignment", "reflecting_alignment",
         "rotation_only", "scale_only", "unit_scale")


def _unit(v):
    return v / v.norm()


def _rotation(axis, angle):
    """Rodrigues, float64."""
    a = _unit(torch.tensor(axis, dtype=torch.float64))
    Kx = torch.tensor([[0.0, -a[2], a[1]], [a[2], 0.0, -a[0]], [-a[1], a[0], 0.0]], dtype=torch.float64)
    return torch.eye(3, dtype=torch.float64) + math.sin(angle) * Kx + (1.0 - math.cos(angle)) * (Kx @ Kx)


def _benign():
    """The pose, alignment and cotangents of test_fused_camera_chain_matches_pytorch_chain[True] (tests/test_camera_gpu.py)."""
    g = torch.Generator().manual_seed(4)
    R = cam.quaternion_to_rotation(torch.randn(4, generator=g))
    T = torch.randn(3, generator=g) + torch.tensor([0.0, 0.0, 4.0])
    c = cam.PoseCamera(R, T, 1.1, 0.7, 64, 48)
    with torch.no_grad():
        c.delta_quaternion.copy_(0.05 * torch.randn(4, generator=g))
        c.delta_translation.copy_(0.1 * torch.randn(3, 1, generator=g))
        c.learnable_fovx.add_(0.03); c.learnable_fovy.sub_(0.02)
    g = torch.Generator().manual_seed(9)
    cots = [torch.randn(4, 4, generator=g), torch.randn(4, 4, generator=g), torch.randn(4, 4, generator=g), torch.randn(3, generator=g)]
    return dict(q0=c.init_quaternion, dq=c.delta_quaternion.detach(), t0=c.init_translation.reshape(3), dt=c.delta_translation.detach().reshape(3),
                fovx=c.learnable_fovx.detach(), fovy=c.learnable_fovy.detach(), znear=0.01, zfar=100.0,
                grot=cam.quaternion_to_rotation(torch.tensor([1.0, 0.02, -0.03, 0.01])), gscale=torch.tensor(1.3)), cots


def make_case(name):
    """(inputs, cotangents): ``inputs`` is a dict q0 (4), dq (4), t0 (3), dt (3), fovx (), fovy () float64 tensors, znear, zfar floats,
    grot (3,3) or None, gscale () or None; the cotangents are (4,4), (4,4), (4,4), (3,) for viewmatrix, projmatrix, intrinsic, campos.
    Fresh tensors on every call."""
    inp, cots = _make_case(name)
    return {k: (v.clone() if torch.is_tensor(v) else v) for k, v in inp.items()}, [c.clone() for c in cots]


@functools.lru_cache(maxsize=None)
def _make_case(name):
    if name not in CASES:
        raise ValueError(name)
    rn = None
    if name == "benign":
        inp, cots = _benign()
    else:
        g = torch.Generator().manual_seed(1000 + CASES.index(name))
        rn = lambda *s: torch.randn(*s, generator=g, dtype=torch.float64)
        inp = dict(q0=_unit(rn(4)), dq=0.05 * rn(4), t0=rn(3) + torch.tensor([0.0, 0.0, 4.0], dtype=torch.float64), dt=0.1 * rn(3),
                   fovx=torch.tensor(1.1, dtype=torch.float64), fovy=torch.tensor(0.7, dtype=torch.float64), znear=0.01, zfar=100.0,
                   grot=None, gscale=None)
        cots = [rn(4, 4), rn(4, 4), rn(4, 4), rn(3)]
        rot = _rotation((0.3, -1.0, 0.5), 0.7)
        if name == "long_quaternion":                       # |q0 + dq| ~ 8: a missing 1/n is a factor 8, a squared one 64
            inp["q0"] = 8.0 * inp["q0"]
        elif name == "short_quaternion":                    # |q0 + dq| ~ 0.1
            inp["q0"], inp["dq"] = 0.1 * inp["q0"], 0.1 * inp["dq"]
        elif name.startswith("half_turn_"):
            # a camera turned by pi - 1e-3 about the axis, its quaternion by rotation_to_quaternion's branch for that axis
            # (trace < 0); the delta keeps w of the sum within 1e-3 of zero: the R(q) adjoint's terms in w all but vanish
            axis = [0.0, 0.0, 0.0]
            axis["xyz".index(name[-1])] = 1.0
            inp["q0"] = cam.rotation_to_quaternion(_rotation(axis, math.pi - 1e-3))
            inp["dq"] = inp["dq"] * torch.tensor([2e-3, 1.0, 1.0, 1.0], dtype=torch.float64)
        elif name == "identity":
            inp["q0"], inp["dq"] = torch.tensor([1.0, 0.0, 0.0, 0.0], dtype=torch.float64), torch.zeros(4, dtype=torch.float64)
        elif name == "far_translation":                     # |t| ~ 1e3
            inp["t0"] = 1e3 * _unit(inp["t0"])
        elif name == "narrow_fov":
            inp["fovx"], inp["fovy"] = torch.tensor(0.05, dtype=torch.float64), torch.tensor(0.05, dtype=torch.float64)
        elif name == "wide_fov":
            inp["fovx"], inp["fovy"] = torch.tensor(2.8, dtype=torch.float64), torch.tensor(2.8, dtype=torch.float64)
        elif name == "unequal_fov":
            inp["fovx"], inp["fovy"] = torch.tensor(0.05, dtype=torch.float64), torch.tensor(2.8, dtype=torch.float64)
        elif name == "near_far":
            inp["znear"], inp["zfar"] = 0.5, 7.0
        elif name == "skewed_alignment":                    # det 1.144, condition number below 2, G G^T far from 1: R^-1 is not R^T
            inp["grot"] = rot @ (torch.diag(torch.tensor([1.3, 0.8, 1.1], dtype=torch.float64)) + 0.1 * torch.ones(3, 3, dtype=torch.float64).triu(1))
            inp["gscale"] = torch.tensor(0.37, dtype=torch.float64)
        elif name == "reflecting_alignment":                # det < 0
            inp["grot"] = rot @ torch.diag(torch.tensor([1.1, -0.9, 1.2], dtype=torch.float64))
            inp["gscale"] = torch.tensor(1.7, dtype=torch.float64)
        elif name == "rotation_only":
            inp["grot"] = _rotation((1.0, 0.2, -0.4), 1.9) @ torch.diag(torch.tensor([0.9, 1.2, 1.05], dtype=torch.float64))
        elif name == "scale_only":
            inp["gscale"] = torch.tensor(2.3, dtype=torch.float64)
        elif name == "unit_scale":
            inp["grot"], inp["gscale"] = rot, torch.tensor(1.0, dtype=torch.float64)
    inp = {k: (v if isinstance(v, float) else _r32(v)) for k, v in inp.items()}
    if name == "zero_translation":                          # after the rounding: t0 + dt = 0 exactly
        inp["dt"] = -inp["t0"]
    cots = [_r32(c) for c in cots]
    # The three scalar gradients are one short sum each, and a sum that cancels loses its condition number in relative accuracy in
    # whichever order it is added: on such cotangents the float32 chain's error, and so the bar, is luck.  The pose is the case;
    # the cotangents are redrawn until none of the float64 sums cancels by more than MAX_CANCELLATION.  (benign keeps the
    # cotangents of the test it restates: its g_fovy cancels 18-fold.)
    while name != "benign" and max(scalar_cancellation(inp, cots).values()) > MAX_CANCELLATION:
        cots = [_r32(rn(4, 4)), _r32(rn(4, 4)), _r32(rn(4, 4)), _r32(rn(3))]
    return inp, cots


def _r32(t):
    return None if t is None else t.detach().to(torch.float32).to(torch.float64).clone()


def scalar_cancellation(inp, cots):
    """sum |terms| / |sum terms| of the last sum of each scalar gradient under all four cotangents, from the float64 chain:
    g_fovx = dK00/dfovx (gK[0,0] + sum_l V[l,0] gM[l,0]), g_fovy likewise, g_gscale = sum_i g_t[i] (t0 + dt)[i]."""
    values, grads = chain(inp, torch.float64, ALL_ON, cots)
    V = values["viewmatrix"]
    terms = {"fov" + "xy"[j]: torch.cat([cots[2][j, j].reshape(1), V[:, j] * cots[1][:, j]]) for j in (0, 1)}
    if inp["gscale"] is not None:
        terms["gscale"] = grads["dt"] / inp["gscale"] * (inp["t0"] + inp["dt"])
    return {n: (t.abs().sum() / t.sum().abs()).item() for n, t in terms.items()}


class _Chain(cam.PoseCamera):
    """``PoseCamera`` holding the case's leaves in any dtype.  ``get_world_view_transform``, ``get_full_proj_transform`` and
    ``get_camera_center`` are the class's own; ``get_intrinsic`` restates ``projection_matrix``, which casts its entries to float32,
    entry for entry (bit-equal to it in float32: tests/test_camera_cases_cpu.py)."""

    def __init__(self, inp, dtype):
        super().__init__(torch.eye(3), torch.zeros(3), 1.0, 1.0, 64, 48, znear=inp["znear"], zfar=inp["zfar"])
        self.to(dtype)                                      # last_row
        leaf = lambda t: torch.nn.Parameter(t.to(dtype).clone())
        self.init_quaternion = inp["q0"].to(dtype).clone()
        self.init_translation = inp["t0"].to(dtype).reshape(3, 1).clone()
        self.delta_quaternion = leaf(inp["dq"])
        self.delta_translation = leaf(inp["dt"].reshape(3, 1))
        self.learnable_fovx, self.learnable_fovy = leaf(inp["fovx"]), leaf(inp["fovy"])
        self.grot = None if inp["grot"] is None else inp["grot"].to(dtype).clone().requires_grad_(True)
        self.gscale = None if inp["gscale"] is None else inp["gscale"].to(dtype).clone().requires_grad_(True)

    def get_intrinsic(self):
        zn, zf = self.znear, self.zfar
        right, top = torch.tan(self.learnable_fovx / 2) * zn, torch.tan(self.learnable_fovy / 2) * zn
        left, bottom = -right, -top
        P = torch.zeros(4, 4, dtype=right.dtype)
        rows = [[2.0 * zn / (right - left), P[0, 1], (right + left) / (right - left), P[0, 3]],
                [P[1, 0], 2.0 * zn / (top - bottom), (top + bottom) / (top - bottom), P[1, 3]],
                [P[2, 0], P[2, 1], P[2, 2] + zf / (zf - zn), P[2, 3] - (zf * zn) / (zf - zn)],
                [P[3, 0], P[3, 1], P[3, 2] + 1.0, P[3, 3]]]
        return torch.stack([torch.stack(r) for r in rows]).transpose(0, 1)


def chain(inp, dtype, on=ALL_ON, cots=None):
    """(values, grads): the four tensors by name and, when ``cots`` is given, the gradient of ``sum_i <cots[i], out_i>`` over the
    cotangents switched ``on`` to every present leaf by name (zeros where the loss does not reach a leaf), all in ``dtype``."""
    c = _Chain(inp, dtype)
    out = (c.get_world_view_transform(c.grot, c.gscale), c.get_full_proj_transform(c.grot, c.gscale), c.get_intrinsic(),
           c.get_camera_center(c.grot, c.gscale))
    values = {n: o.detach() for n, o in zip(VALUES, out)}
    if cots is None:
        return values, None
    leaves = dict(dq=c.delta_quaternion, dt=c.delta_translation, fovx=c.learnable_fovx, fovy=c.learnable_fovy, grot=c.grot, gscale=c.gscale)
    leaves = {n: t for n, t in leaves.items() if t is not None}
    loss = sum((k.to(dtype) * o).sum() for k, o, use in zip(cots, out, on) if use)
    gs = torch.autograd.grad(loss, list(leaves.values()), allow_unused=True)
    grads = {n: (torch.zeros_like(t) if g is None else g).detach().reshape(-1) for (n, t), g in zip(leaves.items(), gs)}
    return values, grads


def value_error(got, ref):
    return (got.double().reshape(ref.shape) - ref).abs().max().item()


def gradient_error(got, ref):
    """Relative L2; None where the float64 gradient is exactly zero (compare for exact zeros instead)."""
    n = ref.norm().item()
    return None if n == 0.0 else ((got.double().reshape(-1) - ref.reshape(-1)).norm() / n).item()


def bars(ref, err32):
    """``ref``: (values, grads) of the float64 chain; ``err32``: (value errors, gradient errors) of the float32 chain, by name.
    Returns (value bars, gradient bars); a gradient bar is None where the float64 gradient is exactly zero."""
    vb = {n: max(FACTOR * err32[0][n], FLOOR * ref[0][n].abs().max().item()) for n in ref[0]}
    gb = {n: (None if err32[1][n] is None else max(FACTOR * err32[1][n], FLOOR)) for n in ref[1]}
    return vb, gb


@functools.lru_cache(maxsize=None)
def reference(name, on=ALL_ON):
    """dict for one case and one set of cotangents: ``inputs``, ``cots``, ``values`` / ``grads`` (float64), ``err32`` and ``bars``
    ((values, gradients) by name).  Computed once and shared; callers leave it unchanged."""
    inp, cots = make_case(name)
    v64, g64 = chain(inp, torch.float64, on, cots)
    v32, g32 = chain(inp, torch.float32, on, cots)
    err32 = ({n: value_error(v32[n], v64[n]) for n in v64}, {n: gradient_error(g32[n], g64[n]) for n in g64})
    return dict(inputs=inp, cots=cots, values=v64, grads=g64, values32=v32, grads32=g32, err32=err32, bars=bars((v64, g64), err32))
