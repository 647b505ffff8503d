"""The inputs of the cubemap-stitch tests (tests/test_resample_faces_cpu.py, tests/test_resample_faces_gpu.py): the named cases,
an equidistant-fisheye control flow, the float64 reference and ``margin`` -- how far a pixel is from a face decision.

The face a pixel belongs to is a discrete decision (c > 0, |u| <= 1, |v| <= 1).  Float32 and float64 can decide differently only
where one of those comparisons is nearly an equality, so the tests (a) never re-decide in a reference: the kernel's own
``face_index`` is replayed, (b) bound the share of such borderline pixels of every case on the CPU, and (c) accept a differing
face only where ``margin`` is tiny."""
import functools
import math

import torch

from bags_raster.distortion import cube_face_matrices, resample_faces_torch

MARGIN = 1e-4                 # a face may differ between float32 and float64 only where margin(...) is below this
MAX_BORDERLINE = 0.01         # ... and at most this share of a case's pixels may be that close (checked on the CPU)

# faces: how many of front, left, right, up, down; S: face size; ctrl / flow / crop: (rows, columns); fov: of the fisheye's diagonal
CASES = {
    "all_faces":    dict(faces=5, C=3, S=24, ctrl=(9, 13), flow=(44, 60), crop=(40, 56), fov=150.0, tan_face=1.0, seed=1),
    "overlap":      dict(faces=5, C=3, S=17, ctrl=(5, 7), flow=(33, 47), crop=(33, 47), fov=120.0, tan_face=1.05, seed=2),
    "larger":       dict(faces=5, C=3, S=40, ctrl=(12, 20), flow=(70, 100), crop=(64, 96), fov=165.0, tan_face=1.0, seed=3),
    "hole":         dict(faces=2, C=3, S=24, ctrl=(9, 13), flow=(44, 60), crop=(40, 56), fov=150.0, tan_face=1.0, seed=4),
    "minification": dict(faces=5, C=3, S=16, ctrl=(6, 8), flow=(176, 224), crop=(160, 208), fov=150.0, tan_face=1.0, seed=5),
    "all_faces_c1": dict(faces=5, C=1, S=24, ctrl=(9, 13), flow=(44, 60), crop=(40, 56), fov=150.0, tan_face=1.0, seed=1),
    "all_faces_c4": dict(faces=5, C=4, S=24, ctrl=(9, 13), flow=(44, 60), crop=(40, 56), fov=150.0, tan_face=1.0, seed=1),
}


def fisheye_ctrl(h, w, fov_deg, aspect, dtype=torch.float64):
    """Control flow of an equidistant fisheye whose diagonal spans ``fov_deg``: control points on [-1,1]^2 of the output image ->
    ray (x/z, y/z), i.e. grid_sample coordinates of a front image with unit tangents."""
    gy, gx = torch.meshgrid(torch.linspace(-1, 1, h, dtype=dtype), torch.linspace(-1, 1, w, dtype=dtype), indexing="ij")
    r = torch.sqrt(gx * gx * aspect * aspect + gy * gy)                      # radius in units of the half height
    per_r = math.radians(fov_deg) / 2 / math.sqrt(aspect * aspect + 1)       # the diagonal reaches fov / 2
    k = torch.where(r > 0, torch.tan(r * per_r) / r.clamp_min(1e-30), torch.full_like(r, per_r))
    return torch.stack([gx * aspect * k, gy * k], -1)


@functools.lru_cache(maxsize=None)
def make_case(name):
    """faces (list of (C,S,S) float32), ctrl (h,w,2) float32, mats (F,3,3) float64 holding float32 values (what the kernel gets),
    cot (C,Hc,Wc) float32, flow_hw, crop_hw.  Nothing here is to be modified."""
    c = CASES[name]
    g = torch.Generator().manual_seed(c["seed"])
    h, w = c["ctrl"]
    ctrl = fisheye_ctrl(h, w, c["fov"], c["flow"][1] / c["flow"][0]) + 0.01 * torch.randn(h, w, 2, generator=g, dtype=torch.float64)
    faces = [torch.rand(c["C"], c["S"], c["S"], generator=g) for _ in range(c["faces"])]
    cot = torch.randn(c["C"], *c["crop"], generator=g)
    mats = cube_face_matrices(1.0, c["tan_face"])[1][:c["faces"]].float().double()
    return dict(faces=faces, ctrl=ctrl.float(), mats=mats, cot=cot, flow_hw=c["flow"], crop_hw=c["crop"])


def coords(ctrl, mats, flow_hw, crop_hw):
    """(u, v, c), each (F,Hc,Wc), float64: every face's coordinates at every cropped pixel."""
    flow = torch.nn.functional.interpolate(ctrl.double().permute(2, 0, 1).unsqueeze(0), size=tuple(flow_hw), mode="bilinear",
                                           align_corners=False).squeeze(0).permute(1, 2, 0)
    sy, sx = (flow_hw[0] - crop_hw[0]) // 2, (flow_hw[1] - crop_hw[1]) // 2
    g = flow[sy:sy + crop_hw[0], sx:sx + crop_hw[1]]
    abc = torch.einsum("fij,hwj->fhwi", mats.double(), torch.cat([g, torch.ones_like(g[..., :1])], -1))
    return abc[..., 0] / abc[..., 2], abc[..., 1] / abc[..., 2], abc[..., 2]


def margin(ctrl, mats, flow_hw, crop_hw):
    """(Hc,Wc) float64: the smallest of |c_f| over all faces and of ||u_f| - 1|, ||v_f| - 1| over the faces with c_f > 0.  A face
    choice can differ between float32 and float64 only where this is tiny."""
    u, v, c = coords(ctrl, mats, flow_hw, crop_hw)
    edge = torch.minimum((u.abs() - 1).abs(), (v.abs() - 1).abs())
    edge = torch.where(c > 0, edge, torch.full_like(edge, float("inf")))
    return torch.minimum(c.abs(), edge).min(0).values


@functools.lru_cache(maxsize=None)
def case_margin(name):
    c = make_case(name)
    return margin(c["ctrl"], c["mats"], c["flow_hw"], c["crop_hw"])


def _run(name, dtype, face_index):
    c = make_case(name)
    faces = [f.to(dtype).clone().requires_grad_(True) for f in c["faces"]]
    ctrl = c["ctrl"].to(dtype).clone().requires_grad_(True)
    out, idx = resample_faces_torch(faces, ctrl, c["mats"], c["flow_hw"], c["crop_hw"], face_index=face_index)
    (out * c["cot"].to(dtype)).sum().backward()
    zero = lambda f: torch.zeros_like(f) if f.grad is None else f.grad
    return out.detach().double(), idx, [zero(f).double() for f in faces], ctrl.grad.double()


_CACHE = {}


def reference(name, face_index=None):
    """(image, face_index, [dL/dface], dL/dctrl) of ``resample_faces_torch`` in float64 for the case's cotangent; with ``face_index``
    given, for THAT map (the kernel's own choice, replayed).  Computed once per (case, map)."""
    key = (name, None if face_index is None else face_index.cpu().numpy().tobytes())
    if key not in _CACHE:
        _CACHE[key] = _run(name, torch.float64, None if face_index is None else face_index.cpu())
    return _CACHE[key]


def float32_route(name, face_index):
    """The same through PyTorch in float32, given the same map: what the bars are to be read against."""
    return _run(name, torch.float32, face_index.cpu())


def errors(got, ref):
    """Largest absolute error of the image, of the face gradients and of the control-flow gradient against ``ref``."""
    return (float((got[0] - ref[0]).abs().max()), max(float((a - b).abs().max()) for a, b in zip(got[2], ref[2])),
            float((got[3] - ref[3]).abs().max()))


def bars(ref):
    """The bars of test_resample_matches_oracle (tests/test_resample_gpu.py) for the same arithmetic: image atol 5e-5, dL/dfaces
    2e-4 * max(1, max |ref|), dL/dctrl_flow 2e-3 * max |ref|."""
    return 5e-5, 2e-4 * max(1.0, max(float(g.abs().max()) for g in ref[2])), 2e-3 * float(ref[3].abs().max())
