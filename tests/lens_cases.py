"""Cases, float64 reference and measured bar of tests/test_lens_field_gpu.py -- CPU only, so that tests/test_lens_field_cpu.py can
check the generators and what the bars are built from without a GPU.

``make_case(name)``       net shape, flat float32 parameters, points ``x``, cotangent, all seeded by the case's name (cached).
``reference(name)``       ``lens_field_torch`` in float64 with autograd: y, grad_x, grad_params (cached, never modified).
``errors(name, got)``     the errors of a (y, grad_x, grad_params) triple against that reference: y by max-abs, gradients by relative L2.
``bars(name, device)``    ``4 * err32 + floor``: err32 is what the float32 ``lens_field_torch`` loses against the reference on ``device`` on
                          the same input, the floor 16 float32 epsilons times the reference's scale (max |y|; 1 for a relative L2).
                          Nothing in a bar comes from the kernel.  ELU with alpha = 1 is C^1: no element is left out.
"""
import functools
import zlib

import torch

from bags_raster.lens_field import LensField, lens_field_inverse_torch, lens_field_torch

# (B, H, n, M): the wave, workgroup and partial-reduction edges, an odd H, the largest block
SHAPES = ((1, 1, 0, 1), (1, 2, 0, 63), (2, 16, 1, 64), (2, 16, 1, 65), (3, 33, 2, 255), (3, 33, 2, 257), (5, 64, 1, 1025), (1, 64, 4, 1025))
CASES = {"b%d_h%d_n%d_m%d" % s: dict(B=s[0], H=s[1], n=s[2], shape=(s[3], 2), gain=1.0) for s in SHAPES}
CASES["grid_b5_h64_n1"] = dict(B=5, H=64, n=1, shape=(68, 120, 2), gain=1.0)
# weights times 8 and no correction: the ELU arguments reach both tails
CASES["saturated_b2_h16_n1_m257"] = dict(B=2, H=16, n=1, shape=(257, 2), gain=8.0)
# more tiles than the backward has workgroups (256 tiles of 64 points): a workgroup walks several tiles and sums over them
CASES["strided_b2_h16_n1_m16449"] = dict(B=2, H=16, n=1, shape=(64 * 257 + 1, 2), gain=1.0)
SATURATED = "saturated_b2_h16_n1_m257"
INVERTIBLE = tuple(k for k in CASES if k != SATURATED)       # the fixed-point inverse needs contractions: the corrected nets
FACTOR = 4.0
FLOOR_EPS = 16.0
EPS32 = float(torch.finfo(torch.float32).eps)
INVERSE_ITERATIONS = 50


@functools.lru_cache(maxsize=None)
def make_case(name):
    c = CASES[name]
    seed = zlib.crc32(name.encode())
    net = LensField(c["B"], c["H"], c["n"], seed=seed)
    if c["gain"] == 1.0:
        net.lipschitz_correction(iterations=50, generator=torch.Generator().manual_seed(seed + 1))
    else:
        with torch.no_grad():
            net.params.mul_(c["gain"])
    gen = torch.Generator().manual_seed(seed + 2)
    x = torch.rand(c["shape"], generator=gen) * 3.0 - 1.5
    cot = torch.randn(c["shape"], generator=gen)
    return dict(B=c["B"], H=c["H"], n=c["n"], params=net.params.detach().clone(), x=x, cot=cot)


def dims(name):
    c = CASES[name]
    return c["B"], c["H"], c["n"]


def run_torch(name, dtype, device="cpu"):
    """(y, grad_x, grad_params) of lens_field_torch in ``dtype`` on ``device``, as CPU float64 tensors."""
    c = make_case(name)
    p = c["params"].detach().clone().to(device=device, dtype=dtype).requires_grad_(True)      # the cached case stays as it is
    x = c["x"].detach().clone().to(device=device, dtype=dtype).requires_grad_(True)
    y = lens_field_torch(p, x, *dims(name))
    y.backward(c["cot"].to(device=device, dtype=dtype))
    return tuple(t.detach().double().cpu() for t in (y, x.grad, p.grad))


@functools.lru_cache(maxsize=None)
def reference(name):
    return run_torch(name, torch.float64)


def rel_l2(a, ref):
    return float((a.double().cpu() - ref).norm() / ref.norm())


def errors(name, got):
    """(y max-abs, grad_x relative L2, grad_params relative L2) of ``got`` against the float64 reference."""
    y, gx, gp = reference(name)
    return (float((got[0].double().cpu() - y).abs().max()), rel_l2(got[1], gx), rel_l2(got[2], gp))


@functools.lru_cache(maxsize=None)
def err32(name, device="cpu"):
    return errors(name, run_torch(name, torch.float32, device))


def bars(name, device="cpu"):
    e = err32(name, device)
    scale = float(reference(name)[0].abs().max())
    return (FACTOR * e[0] + FLOOR_EPS * EPS32 * scale, FACTOR * e[1] + FLOOR_EPS * EPS32, FACTOR * e[2] + FLOOR_EPS * EPS32)


# ---- the inverse: y is the reference's output rounded to float32, the same y for every path
@functools.lru_cache(maxsize=None)
def inverse_input(name):
    return reference(name)[0].float()


@functools.lru_cache(maxsize=None)
def inverse_reference(name):
    c = make_case(name)
    return lens_field_inverse_torch(c["params"].double(), inverse_input(name).double(), *dims(name), INVERSE_ITERATIONS)


@functools.lru_cache(maxsize=None)
def inverse_err32(name, device="cpu"):
    c = make_case(name)
    x = lens_field_inverse_torch(c["params"].to(device), inverse_input(name).to(device), *dims(name), INVERSE_ITERATIONS)
    return float((x.double().cpu() - inverse_reference(name)).abs().max())


def inverse_bar(name, device="cpu"):
    return FACTOR * inverse_err32(name, device) + FLOOR_EPS * EPS32 * float(inverse_reference(name).abs().max())
