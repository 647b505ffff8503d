"""Named cases for bags_raster.gaussian_normals, built on the CPU from a fixed seed (tests/test_gaussian_normals_cpu.py and
tests/test_gaussian_normals_gpu.py run the same ones).

Quaternions are normal draws scaled to lengths in [0.5, 2]; the view matrix is a random rigid transform in the row-vector
convention (t = x @ V[:3,:3] + V[3,:3]).  The means are built FROM the normals: in float64, with m the camera-frame axis of the row,
the view-space point is t = r (a mh + sqrt(1 - a^2) u), u a unit vector perpendicular to mh, and the mean is t carried back through
the view matrix -- so a = mh . th is what the case says it is, up to the float32 rounding of the mean (1e-7).

    generic      scales log-uniform in [1e-2, 1], the smallest at most 0.8 x the middle one; |mh . th| in [0.05, 1]: neither decision
                 can differ between float32 and float64
    scaled_view  the same with the 3x3 block times 1.7 (global alignment)
    disks        the smallest scale 1e-3 of the others
    log_scales   generic fed with log(s): the same output, bit for bit
    ties         a third of the rows with two or three exactly equal scales: the first minimum wins
    dead         generic with rows of q = 0, rows with a NaN in q, rows with |q| = 1e-25 (Q underflows to zero in float32)
    grazing      mh . th uniform in [-1e-3, 1e-3]: sigma may differ between float32 and float64 on a few rows (sigma_flips)

The further views of a multi-view call are the first one turned about its own camera centre (the faces of a cubemap): m and t turn
together, so every view keeps the margin of the first.
"""
import math

import torch

from bags_raster.gaussian_normals import _axis_torch, _view_torch      # (the package attribute of that name is the function)

P_FULL = 4096
SIZES = (1, 63, 64, 65, 255, 256, 257, 1000)
CASES = ("generic", "scaled_view", "disks", "log_scales", "ties", "dead", "grazing")
GRAZING = 1e-3                                    # |mh . th| of `grazing` is uniform in [-GRAZING, GRAZING]
MAX_VIEWS = 17
F64 = torch.float64
_cache = {}


def _gen(seed):
    return torch.Generator().manual_seed(seed)


def _rotation(g):
    q, r = torch.linalg.qr(torch.randn(3, 3, generator=g, dtype=F64))
    q = q * torch.sign(torch.diagonal(r))[None, :]
    if torch.det(q) < 0:
        q[:, 0] = -q[:, 0]
    return q


def _views(block_scale):
    """MAX_VIEWS distinct (4,4) float32 view matrices: a rigid transform (its block times block_scale), then the same turned about
    its camera centre."""
    g = _gen(1234)
    R, T = _rotation(g), torch.randn(3, generator=g, dtype=F64)
    out = []
    for v in range(MAX_VIEWS):
        Gv = torch.eye(3, dtype=F64) if v == 0 else _rotation(g)
        V = torch.eye(4, dtype=F64)
        V[:3, :3] = block_scale * (R @ Gv)
        V[3, :3] = T @ Gv
        out.append(V.float())
    return out


def _scales(name, g):
    P = P_FULL
    lo, hi = math.log(1e-2), math.log(1.0)
    two = torch.exp(lo + (hi - lo) * torch.rand(P, 2, generator=g, dtype=F64))
    base = two.min(1).values
    small = base * (1e-3 if name == "disks" else (0.1 + 0.7 * torch.rand(P, generator=g, dtype=F64)))
    k = torch.randint(0, 3, (P,), generator=g)
    s = torch.empty(P, 3, dtype=F64)
    for j in range(3):                                # the smallest at column k, the two others in the columns left, in order
        s[:, j] = torch.where(k == j, small, torch.where(j < k, two[:, min(j, 1)], two[:, max(j - 1, 0)]))
    s = s.float()
    if name == "ties":
        kind = torch.arange(P) % 9                    # 0: s0 == s1 smallest, 1: s1 == s2 smallest, 2: all equal, 3..8: as drawn
        lo_, hi_ = s.min(1).values, s.max(1).values
        s[kind == 0] = torch.stack([lo_, lo_, hi_], 1)[kind == 0]
        s[kind == 1] = torch.stack([hi_, lo_, lo_], 1)[kind == 1]
        s[kind == 2] = torch.stack([lo_, lo_, lo_], 1)[kind == 2]
        kind6 = torch.arange(P) % 18 == 9             # and: s0 == s2 smallest; the two LARGER ones equal
        s[kind6] = torch.stack([lo_, hi_, lo_], 1)[kind6]
        kind7 = torch.arange(P) % 18 == 10
        s[kind7] = torch.stack([hi_, hi_, lo_], 1)[kind7]
    return s


def first_minimum(scales):
    """The statement's k, row by row in plain Python."""
    out = []
    for s0, s1, s2 in scales.tolist():
        k, sk = 0, s0
        if s1 < sk:
            k, sk = 1, s1
        if s2 < sk:
            k = 2
        out.append(k)
    return torch.tensor(out)


def case(name):
    """{rotations (P,4), scales (P,3), means3D (P,3), views [MAX_VIEWS x (4,4)]} as float32 CPU tensors; the same tensors every call."""
    if name in _cache:
        return _cache[name]
    assert name in CASES, name
    if name == "log_scales":
        c = dict(case("generic"))
        c["scales"] = torch.log(c["scales"])
        _cache[name] = c
        return c
    g = _gen(20240 if name in ("generic", "scaled_view", "dead") else 20240 + CASES.index(name))      # one draw for the three
    P = P_FULL
    q = torch.randn(P, 4, generator=g, dtype=F64)
    q = (q / q.norm(dim=1, keepdim=True) * (0.5 + 1.5 * torch.rand(P, 1, generator=g, dtype=F64))).float()
    scales = _scales(name, g)
    views = _views(1.7 if name == "scaled_view" else 1.0)
    # the camera-frame axis of every row under view 0, in float64 from the float32 inputs
    c, _ = _axis_torch(q.double(), scales.double())
    V0 = views[0].double()
    m = torch.stack(c, 1) @ V0[:3, :3]
    mh = m / m.norm(dim=1, keepdim=True)
    if name == "grazing":
        a = GRAZING * (2 * torch.rand(P, generator=g, dtype=F64) - 1)
    else:
        a = (0.05 + 0.95 * torch.rand(P, generator=g, dtype=F64)) * torch.where(torch.rand(P, generator=g) < 0.5, -1.0, 1.0).double()
    u = torch.linalg.cross(mh, torch.randn(P, 3, generator=g, dtype=F64), dim=1)
    u = u / u.norm(dim=1, keepdim=True)
    r = 2 + 4 * torch.rand(P, 1, generator=g, dtype=F64)
    t = r * (a[:, None] * mh + torch.sqrt(1 - a * a)[:, None] * u)
    means = ((t - V0[3, :3]) @ torch.linalg.inv(V0[:3, :3])).float()
    if name == "dead":
        i = torch.arange(P)
        q[i % 37 == 0] = 0.0
        q[i % 37 == 1, 2] = float("nan")
        q[i % 37 == 2] = q[i % 37 == 2] / q[i % 37 == 2].norm(dim=1, keepdim=True) * 1e-25
    _cache[name] = dict(rotations=q, scales=scales, means3D=means, views=views)
    return _cache[name]


def dead_rows():
    """`dead`: the rows that must come out as zeros under float32."""
    return torch.arange(P_FULL) % 37 <= 2


def cotangents(P, V):
    g = _gen(777)
    return [torch.randn(P_FULL, 3, generator=g, dtype=F64)[:P] for _ in range(MAX_VIEWS)][:V]


def leaves(name, dtype, device, P=P_FULL, V=1, zero_block=False):
    c = case(name)
    views = [m.clone() for m in c["views"][:V]]
    if zero_block:
        for m in views:
            m[:3, :3] = 0.0
    return dict(rotations=c["rotations"][:P].to(device, dtype).requires_grad_(),
                scales=c["scales"][:P].to(device, dtype).requires_grad_(),
                means3D=c["means3D"][:P].to(device, dtype).requires_grad_(),
                views=[m.to(device, dtype).requires_grad_() for m in views])


def forward_backward(fn, name, dtype, device, P=P_FULL, V=1, row_mask=None, zero_block=False):
    """``fn`` is gaussian_normals_views or its PyTorch statement: (outputs [V x (P,3)], {rotations, view0, view1, ...}) with the
    cotangents of ``cotangents`` (zero on the rows ``row_mask`` leaves out)."""
    lv = leaves(name, dtype, device, P, V, zero_block)
    outs = fn(lv["rotations"], lv["scales"], lv["means3D"], lv["views"])
    cots = [c.to(device, dtype) for c in cotangents(P, V)]
    if row_mask is not None:
        cots = [c * row_mask.to(device, dtype)[:, None] for c in cots]
    wanted = [lv["rotations"]] + lv["views"]
    if P > 0:
        gs = torch.autograd.grad(list(outs), wanted + [lv["scales"], lv["means3D"]], cots, allow_unused=True)
        assert gs[-1] is None and gs[-2] is None, "scales / means3D must get no gradient"
    else:
        gs = torch.autograd.grad(list(outs), wanted, cots, allow_unused=True)
    grads = {"rotations": gs[0]}
    grads.update({"view%d" % v: gs[1 + v] for v in range(V)})
    return [o.detach() for o in outs], grads


def sigma_of(name, dtype):
    """sigma of every row under view 0 as the statement decides it in ``dtype``."""
    c = case(name)
    axis, _ = _axis_torch(c["rotations"].to(dtype), c["scales"].to(dtype))
    return _view_torch(axis, c["means3D"].to(dtype), c["views"][0].to(dtype))[1]


def sigma_flips(name):
    """(P,) bool: rows whose sigma differs between the float32 and the float64 statement."""
    return sigma_of(name, torch.float32).double() != sigma_of(name, F64)
