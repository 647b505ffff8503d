"""The named cases of the antialiasing tests (bags_raster.antialias_opacity, csrc/antialias.hip), their float64 and float32
PyTorch references, and the counts that show each case does what its name says.

Every case is ``scenes.make_case(1025, W, H, sm, deg=0, seed, dist=...)`` plus the edit in ``CASES``; a smaller cloud is the first
``P`` rows of it.  The references are ``antialias_opacity_torch`` in float64 (autograd = the gradient reference) and in float32 on
the CPU (the statement the kernel rounds like); they are computed once per (case, variant) and shared.
"""
import functools
import math

import torch

from bags_raster.antialias import FLOOR, _chain_torch, antialias_opacity_torch
from bags_raster.gaussians import covariance_from_scaling_rotation
from scenes import camera_tensors, make_case

BLOCK = 256                                      # csrc/antialias.hip: AA_BLOCK
SIZES = (1, BLOCK - 1, BLOCK + 1, 4 * BLOCK + 1)  # 1, 255, 257, 1025: either side of a workgroup, and more than one
P_FULL = SIZES[-1]

#        name            W   H   sm    seed dist  scale edit (column factors)  shift_factors
CASES = {"generic":      (64, 48, 1.0,  0,  4.0, (1.0, 1.0, 1.0),            None),
         "small":        (50, 37, 0.25, 1,  4.0, (1.0, 1.0, 1.0),            None),
         "subpixel":     (64, 48, 1.0,  2,  4.0, (0.015, 0.015, 0.015),      None),
         "inside":       (64, 48, 1.0,  3,  1.0, (1.0, 1.0, 1.0),            None),
         "inside_shift": (64, 48, 1.0,  3,  1.0, (1.0, 1.0, 1.0),            (0.05, -0.02, 0.01)),
         "flat":         (64, 48, 2.0,  5,  4.0, (1e-3, 1.0, 1.0),           None),
         "needles":      (64, 48, 2.0,  5,  4.0, (1e-3, 1e-3, 1.0),          None)}
WELL = ("generic", "small", "subpixel", "inside", "inside_shift")       # everything above `flat`
ILL = ("flat", "needles")
NAMES = ("means3D", "opacities", "viewmatrix", "intrinsic", "scales", "rotations", "cov3D_precomp", "shift_factors")


@functools.lru_cache(maxsize=None)
def case(name):
    """The case's inputs as float32 CPU tensors (shift_factors: None where the case has none) and its static settings."""
    W, H, sm, seed, dist, edit, sf = CASES[name]
    scene, cam = make_case(P_FULL, W, H, sm, deg=0, seed=seed, dist=dist)
    ct = camera_tensors(cam)
    scales = scene["scales"] * torch.tensor(edit)
    return dict(means3D=scene["means3D"], opacities=scene["opacities"], scales=scales, rotations=scene["rotations"],
                viewmatrix=ct["viewmatrix"], intrinsic=ct["intrinsic"], shift_factors=None if sf is None else torch.tensor(sf),
                image_hw=(H, W), tanfov=(math.tan(cam.FoVx * 0.5), math.tan(cam.FoVy * 0.5)))


def leaves(name, dtype, device="cpu", P=P_FULL, cov=False, scale_modifier=1.0):
    """Fresh leaf tensors of the case (first P rows) by argument name; ``cov``: cov3D_precomp instead of the scale pair."""
    c = case(name)
    t = {n: c[n][:P] if n in ("means3D", "opacities", "scales", "rotations") else c[n] for n in NAMES if n != "cov3D_precomp" and c[n] is not None}
    if cov:
        t["cov3D_precomp"] = covariance_from_scaling_rotation(t.pop("scales").double(), scale_modifier, t.pop("rotations").double())
    return {n: v.detach().to(device=device, dtype=dtype).clone().requires_grad_(True) for n, v in t.items()}


def run(fn, name, lv, scale_modifier=1.0, clamp_grad="stock"):
    c = case(name)
    return fn(lv["means3D"], lv["opacities"], lv["viewmatrix"], lv["intrinsic"], c["image_hw"], c["tanfov"], scales=lv.get("scales"),
              rotations=lv.get("rotations"), cov3D_precomp=lv.get("cov3D_precomp"), shift_factors=lv.get("shift_factors"),
              scale_modifier=scale_modifier, clamp_grad=clamp_grad)


@functools.lru_cache(maxsize=None)
def cotangent(P):
    return torch.randn(P, 1, generator=torch.Generator().manual_seed(1234 + P), dtype=torch.float64)


def forward_backward(fn, name, dtype, device="cpu", P=P_FULL, cov=False, scale_modifier=1.0, clamp_grad="stock", row_mask=None):
    """(out, {argument: gradient}) of ``fn`` under the case's fixed cotangent; ``row_mask`` (P bools) zeroes the cotangent of the
    rows that are False, which takes them out of every gradient."""
    lv = leaves(name, dtype, device, P, cov, scale_modifier)
    out = run(fn, name, lv, scale_modifier, clamp_grad)
    g = cotangent(P)
    if row_mask is not None:
        g = g * row_mask.reshape(P, 1).to(g.dtype)
    out.backward(g.to(device=device, dtype=dtype))
    return out.detach(), {n: t.grad for n, t in lv.items()}


@functools.lru_cache(maxsize=None)
def reference(name, dtype, P=P_FULL, cov=False, scale_modifier=1.0, clamp_grad="stock", masked=False):
    """``antialias_opacity_torch`` on the CPU in ``dtype``: (out, gradients).  masked: without the rows of ``floor_flips``."""
    mask = ~floor_flips(name, P, cov, scale_modifier) if masked else None
    return forward_backward(antialias_opacity_torch, name, dtype, "cpu", P, cov, scale_modifier, clamp_grad, mask)


def _decisions(name, dtype, P, cov, scale_modifier):
    """Per row, as full-length masks: culled by the near plane, on the floor, an axis on the field-of-view clamp; and h."""
    with torch.no_grad():
        lv = {n: t.detach() for n, t in leaves(name, dtype, "cpu", P, cov, scale_modifier).items()}
        c = case(name)
        r = _chain_torch(lv["means3D"], lv["opacities"], lv["viewmatrix"], lv["intrinsic"], c["image_hw"], c["tanfov"], lv.get("scales"),
                         lv.get("rotations"), lv.get("cov3D_precomp"), lv.get("shift_factors"), scale_modifier, "stock")
        full = lambda m, fill: torch.full((P,), fill, dtype=m.dtype).index_copy(0, r.idx, m)          # noqa: E731
        culled = full(~r.ok, True)
        return dict(culled=culled, floor=full(r.ok & ~r.above, False), clamped=full(r.clx | r.cly, False), h=full(r.h, 1.0))


@functools.lru_cache(maxsize=None)
def floor_flips(name, P=P_FULL, cov=False, scale_modifier=1.0):
    """Rows whose floor (or cull) decision differs between the float32 and the float64 statement."""
    a, b = _decisions(name, torch.float32, P, cov, scale_modifier), _decisions(name, torch.float64, P, cov, scale_modifier)
    return (a["floor"] != b["floor"]) | (a["culled"] != b["culled"])


@functools.lru_cache(maxsize=None)
def counts(name):
    """What each case is named for, counted on the float64 statement (h error and flips: float32 against it)."""
    d32, d64 = _decisions(name, torch.float32, P_FULL, False, 1.0), _decisions(name, torch.float64, P_FULL, False, 1.0)
    return dict(floor=int(d64["floor"].sum()), culled=int(d64["culled"].sum()), clamped=int((d64["clamped"] & ~d64["culled"]).sum()),
                flips=int(floor_flips(name).sum()), h_err=float((d32["h"].double() - d64["h"]).abs().max()),
                h_min=float(d64["h"].min()), h_max=float(d64["h"][~d64["culled"]].max()))
