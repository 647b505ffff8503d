"""One multi-view training step, stated once -- CPU only to import, so that tests/test_step_cpu.py can check the step's constants, its
guards and the comparison rule without a GPU; tests/test_step_gpu.py runs the step on the fused code.

The step: ``V = 5`` of seven cameras render ``synth_scene(400, 7, 2.0, 2)`` at ``40 x 72`` (neither a multiple of the operator's 16-pixel
tile nor of the losses' 32 x 8 and 64 x 4 tiles) through ``render_views`` and ``render_normals``, and EIGHT loss terms hang off the maps
of those two passes: ``TERMS``.  A term is a function of ``(side, maps, views, constants)``:

``side``       ``"hip"`` the fused wrapper, ``"t32"`` the ``*_torch`` statement on the maps as they are (float32), ``"t64"`` the statement on
               ``.double()`` inputs.  Everything upstream of the maps is the caller's and the same on every side.
``maps``       per view, in step order: ``depth``, ``weights``, ``render`` of the colour pass, ``normal``, ``depth_n``, ``weights_n`` of the
               normal pass (the same bits as the colour pass's, another autograd node: the normal-consistency term uses them, so that
               both operator calls of a camera take depth and weights cotangents), and ``table``, the appearance table ``(7,16)``.
``views``      the V ``(4,4)`` view matrices the two-view terms see, in step order.
``constants``  ``constants_of(maps, views, pinholes)``: ground-truth images, masks, priors, matches, confidences, built on the CPU from
               one detached float32 set of maps.  Every decision a statement takes on a DERIVED quantity is guarded: the pixel's
               confidence or mask is 0 wherever the float64 statement lies within ``CLEAR`` of it (``guards`` holds the shares).
               ``min_weight = 0.5`` and ``min_norm = 0.125`` are exact in float32 and are compared with the maps themselves, so those
               decisions are the same in float32 and float64 without a gap.

It returns ``(loss, count)``, vectors over views or ordered pairs.  ``run(names, ...)`` evaluates several; the step's scalar is the sum of
every entry of every loss.

The comparison rule (nothing in a bar comes from the fused code; factor and floor are the project's, ``depth_prior_cases.FACTOR`` and
``FLOOR_EPS``):

``element_margin``  ``|got - r64| / (4 |r32 - r64| + 16 eps32 (1 + |r64|))``, the largest over the elements: loss values, gradients at the
                    maps and at the view matrices.
``tensor_margin``   ``err(got) / (4 err(r32) + 16 eps32)`` with ``err(x) = max|x - r64| / max|r64|``: the leaves, whose gradients pass
                    through the operator's float32 backward on all three sides.  A maximum over elements, not a norm, so that one wrong
                    row cannot hide under the rest.
"""
import math

import torch

import depth_prior_cases as DP
import warp_cases as WP
from bags_raster import (appearance_torch, correspondence_loss, correspondence_loss_torch, depth_prior_loss, depth_prior_loss_torch,
                         depth_smooth_loss, depth_smooth_loss_torch, depth_to_normal_torch, normal_map_loss, normal_map_loss_torch,
                         normal_prior_loss, normal_prior_loss_torch, normal_smooth_loss, normal_smooth_loss_torch, reproject_pixels_torch,
                         warp_loss, warp_loss_torch)
from bags_raster.appearance import NEUTRAL, apply_appearance
from bags_raster.correspondence import _geometry_torch, _project
from bags_raster.loss import fused_photometric_loss, photometric_loss
from bags_raster.synth import sphere_views, synth_scene

F32, F64 = torch.float32, torch.float64
FACTOR, FLOOR_EPS, EPS32 = DP.FACTOR, DP.FLOOR_EPS, DP.EPS32
H, W = 40, 72
POINTS, SCENE_SEED, SCENE_SM, SH_DEGREE = 400, 7, 2.0, 2
V, CAMERAS = 5, 7
ROWS = (3, 0, 4, 1, 2)                                       # the bank rows of the step, in step order; rows 5 and 6 are not listed
UNLISTED = tuple(r for r in range(CAMERAS) if r not in ROWS)
PAIRS = tuple((i, j) for i in range(V) for j in range(V) if i != j)          # the 20 ordered pairs: two launches of 16 and 4
MIN_WEIGHT, MIN_NORM = 0.5, 0.125
MIN_DEPTH, OCCLUSION = WP.MIN_DEPTH, WP.OCCLUSION
DELTA, EPS, CLEAR = 1.0, 1e-3, 1e-3
SIDES = ("hip", "t32", "t64")
TERMS = ("photo", "depth_prior", "normal_prior", "normal_consistency", "correspondence", "warp", "depth_smooth", "normal_smooth")
MAP_NAMES = ("depth", "weights", "render", "normal", "depth_n", "weights_n")
EXACT_IN_FLOAT32 = ("normal",)                               # maps whose consumers' statements are float64 from the loads on: |r32 - r64| = 0
# which maps and leaves a term reaches (the view matrices the two-view terms see are "views"; "pose" is bank.leaves)
REACH = {
    "photo": dict(maps=("render",), views=False, sh=True, rotation=True, table=True),
    "depth_prior": dict(maps=("depth", "weights"), views=False, sh=False, rotation=True, table=False),
    "normal_prior": dict(maps=("depth", "weights"), views=False, sh=False, rotation=True, table=False),
    "normal_consistency": dict(maps=("normal", "depth_n", "weights_n"), views=False, sh=False, rotation=True, table=False),
    "correspondence": dict(maps=("depth", "weights"), views=True, sh=False, rotation=True, table=False),
    "warp": dict(maps=("depth", "weights"), views=True, sh=False, rotation=True, table=False),
    "depth_smooth": dict(maps=("depth", "weights"), views=False, sh=False, rotation=True, table=False),
    "normal_smooth": dict(maps=("normal",), views=False, sh=False, rotation=True, table=False),
}
REACH["all"] = dict(maps=MAP_NAMES, views=True, sh=True, rotation=True, table=True)


def scene():
    return synth_scene(POINTS, SCENE_SEED, SCENE_SM, SH_DEGREE)


def cameras():
    """The seven PoseCameras (host): the five of the step and two more that no step lists."""
    return sphere_views(V, W, H, noise=0.05) + sphere_views(CAMERAS - V, W, H, noise=0.05, seed=56)


def table_start():
    """The appearance table the step starts from: the neutral rows, perturbed."""
    g = torch.Generator().manual_seed(41)
    return torch.tensor(NEUTRAL).repeat(CAMERAS, 1) + 0.05 * torch.randn(CAMERAS, 16, generator=g)


# ---------------------------------------------------------------------------------------------------------------- constants
def _rotated(n, g):
    """(3,H,W) float64 unit normals (zeros stay zeros), each turned by its own small rotation: 0.1 to 0.3 rad about a random axis."""
    n = n.permute(1, 2, 0)
    k = torch.randn(H, W, 3, generator=g, dtype=F64)
    k = k / k.norm(dim=-1, keepdim=True)
    th = (0.1 + 0.2 * torch.rand(H, W, 1, generator=g, dtype=F64))
    out = n * torch.cos(th) + torch.linalg.cross(k, n, dim=-1) * torch.sin(th) + k * (k * n).sum(-1, keepdim=True) * (1 - torch.cos(th))
    length = out.norm(dim=-1, keepdim=True)
    out = torch.where(length > 0, out / length.clamp_min(1e-300), torch.zeros_like(out))
    return out.permute(2, 0, 1)


def _pair_geometry(m, views, pins, i, j):
    """The float64 statement of the pair (i -> j) on the float32 maps: (x_j.z (H,W), proj (H,W,2), geometric (H,W))."""
    D, A = m["depth"][i].reshape(H, W), m["weights"][i].reshape(H, W)
    _, xj, geometric, _, _ = _geometry_torch(D, A, views[i], views[j], pins[i], MIN_WEIGHT, 1e-30)
    return xj[..., 2], _project(xj, pins[j]), geometric


def constants_of(maps, views, pinholes, seed=31):
    """The constants of a step from one detached set of maps (``MAP_NAMES`` -> V tensors; only depth, weights, render and normal are
    read), the V view matrices and the V pinholes ``(fx, fy, cx, cy)``: a dict of host float32 tensors (lists over views or pairs),
    ``pinholes`` and the figures ``guards`` (name -> largest share of a view's or pair's pixels a guard zeroed), ``solid`` (smallest
    share of a view), ``warp_valid`` (smallest share of a pair), ``gt_gap`` (smallest ``|image - gt|``)."""
    m = {k: [t.detach().to("cpu", F32).contiguous() for t in maps[k]] for k in ("depth", "weights", "render", "normal")}
    views = [t.detach().to("cpu", F32).contiguous() for t in views]
    pins = [tuple(float(x) for x in p) for p in pinholes]
    g = torch.Generator().manual_seed(seed)
    rnd = lambda *s: torch.rand(*s, generator=g)                                         # noqa: E731
    c = dict(pinholes=pins, guards={}, views0=views)
    solid = [(m["weights"][v][0] >= MIN_WEIGHT) & (m["depth"][v][0] > 0) for v in range(V)]
    c["solid"] = min(float(s.float().mean()) for s in solid)
    # ground truth: the image plus noise of magnitude 0.02 to 0.1 with a random sign, so no |x - gt| is near 0
    c["gt"] = [(m["render"][v] + torch.where(rnd(3, H, W) < 0.5, -1.0, 1.0) * (0.02 + 0.08 * rnd(3, H, W))).contiguous() for v in range(V)]
    c["gt_gap"] = min(float((m["render"][v] - c["gt"][v]).abs().min()) for v in range(V))
    # masks: a tenth zeros, the rest in [0.25, 1]
    c["mask"] = [torch.where(rnd(H, W) < 0.1, 0.0, 1.0) * (0.25 + 0.75 * rnd(H, W)) for _ in range(V)]
    # the depth prior: the rendered inverse depth, 10 % noise, 5 % "no prior here"
    c["depth_prior"] = []
    for v in range(V):
        D, A = m["depth"][v][0], m["weights"][v][0]
        p = torch.where(solid[v], A / torch.where(solid[v], D, torch.ones_like(D)), torch.ones_like(D))
        p = p * (1.0 + 0.1 * torch.randn(H, W, generator=g).clamp(-3, 3))
        p[rnd(H, W) < 0.05] = 0.0
        c["depth_prior"].append(p.contiguous())
    # normals of the depth: the consistency target as it is, the prior turned a little (the unturned one has loss 0 in float64)
    c["normal_target"], c["normal_prior"] = [], []
    for v in range(V):
        n, _ = depth_to_normal_torch(m["depth"][v], m["weights"][v], pins[v], min_weight=MIN_WEIGHT)
        c["normal_target"].append(n.contiguous())
        n64, _ = depth_to_normal_torch(m["depth"][v].double(), m["weights"][v].double(), pins[v], min_weight=MIN_WEIGHT)
        c["normal_prior"].append(_rotated(n64, g).float().contiguous())
    # |N| of the rendered normals against min_norm (normal_map_loss, normal_smooth_loss) and against the prior rule's 0.5
    # (normal_prior_loss with the rendered normal as its prior)
    c["mask_norm"], c["mask_length"] = [], []
    near_norm, near_length = [], []
    for v in range(V):
        length = m["normal"][v].double().norm(dim=0)
        a, b = (length - MIN_NORM).abs() < CLEAR, (length - 0.5).abs() < CLEAR
        near_norm.append(float(a.double().mean())), near_length.append(float(b.double().mean()))
        c["mask_norm"].append(torch.where(a, torch.zeros(H, W), c["mask"][v]).contiguous())
        c["mask_length"].append(torch.where(b, torch.zeros(H, W), c["mask"][v]).contiguous())
    c["guards"]["min_norm"], c["guards"]["prior_length"] = max(near_norm), max(near_length)
    # the two-view terms over the 20 ordered pairs
    c["match"], c["conf_match"], c["conf_warp"] = [], [], []
    near_depth, near_delta = [], []
    for i, j in PAIRS:
        proj, _ = reproject_pixels_torch(m["depth"][i], m["weights"][i], views[i], views[j], pins[i], pins[j], (H, W), min_weight=MIN_WEIGHT,
                                         min_depth=MIN_DEPTH)
        match = (proj + 1.5 * (2.0 * rnd(2, H, W) - 1.0)).contiguous()
        zj, p64, geometric = _pair_geometry(m, views, pins, i, j)
        a = geometric & ((zj - MIN_DEPTH).abs() < CLEAR)
        e = (p64 - match.double().permute(1, 2, 0)).norm(dim=-1)
        b = geometric & ((e - DELTA).abs() < CLEAR)
        near_depth.append(float(a.double().mean())), near_delta.append(float(b.double().mean()))
        c["match"].append(match)
        c["conf_match"].append(torch.where(a | b, torch.zeros(H, W), 0.25 + 0.75 * rnd(H, W)).contiguous())
        c["conf_warp"].append(torch.where(a, torch.zeros(H, W), 0.25 + 0.75 * rnd(H, W)).contiguous())
    c["guards"]["min_depth"], c["guards"]["huber_delta"] = max(near_depth), max(near_delta)
    wc = warp_case(m, c)
    guard, _ = WP.guard_mask(wc)
    c["conf_warp"] = [torch.where(guard[k], torch.zeros(H, W), c["conf_warp"][k]).contiguous() for k in range(len(PAIRS))]
    c["guards"]["warp"] = float(guard.double().mean((1, 2)).max())
    c["warp_valid"] = float(WP._pieces(warp_case(m, c))["valid"].double().mean((1, 2)).min())
    return c


def warp_case(m, c):
    """The warp term's 20 pairs as a case of tests/warp_cases.py (for its ``guard_mask`` and ``_pieces``)."""
    src, dst = [i for i, _ in PAIRS], [j for _, j in PAIRS]
    stack = lambda ts, idx: torch.stack([ts[i] for i in idx])                            # noqa: E731
    pins = torch.tensor(c["pinholes"], dtype=F64)
    return dict(H=H, W=W, K=len(PAIRS), Hd=H, Wd=W, C=3, eps=EPS, min_weight=MIN_WEIGHT, degenerate=(), has_dst=torch.ones(len(PAIRS), dtype=torch.bool),
                D=stack(m["depth"], src), A=stack(m["weights"], src), D_dst=stack(m["depth"], dst), A_dst=stack(m["weights"], dst),
                Vi=stack(c["views0"], src), Vj=stack(c["views0"], dst), color=stack(c["gt"], src), image=stack(c["gt"], dst),
                conf=torch.stack(c["conf_warp"]), pin_i=pins[src], pin_j=pins[dst], cot=torch.ones(len(PAIRS)))


TENSOR_LISTS = ("gt", "mask", "depth_prior", "normal_target", "normal_prior", "mask_norm", "mask_length", "match", "conf_match", "conf_warp")


def constants_on(c, device):
    """The constants with their tensors on ``device``, and their float64 copies under ``name + "64"``."""
    out = dict(c)
    for name in TENSOR_LISTS:
        out[name] = [t.to(device) for t in c[name]]
        out[name + "64"] = [t.double() for t in out[name]]
    return out


# ---------------------------------------------------------------------------------------------------------------- the terms
def _k(c, name, side):
    return c[name + "64"] if side == "t64" else c[name]


def _in(ts, side):
    return [t.double() for t in ts] if side == "t64" else list(ts)


def term_photo(side, maps, views, c):
    rows = list(ROWS)
    if side == "hip":
        outs = apply_appearance(list(maps["render"]), maps["table"], rows)
        loss = torch.stack([fused_photometric_loss(o, gt) for o, gt in zip(outs, c["gt"])])
    else:
        table = maps["table"][rows]
        outs = appearance_torch(_in(maps["render"], side), table.double() if side == "t64" else table)
        loss = torch.stack([photometric_loss(o, gt) for o, gt in zip(outs, _k(c, "gt", side))])
    return loss, torch.full((V,), 3.0 * H * W, dtype=loss.dtype, device=loss.device)


def term_depth_prior(side, maps, views, c):
    fn = depth_prior_loss if side == "hip" else depth_prior_loss_torch
    return fn(_in(maps["depth"], side), _in(maps["weights"], side), _k(c, "depth_prior", side), _k(c, "mask", side), mode="pearson",
              space="inverse", min_weight=MIN_WEIGHT)


def term_normal_prior(side, maps, views, c):
    fn = normal_prior_loss if side == "hip" else normal_prior_loss_torch
    return fn(_in(maps["depth"], side), _in(maps["weights"], side), _k(c, "normal_prior", side), c["pinholes"], _k(c, "mask", side), mode="cos",
              min_weight=MIN_WEIGHT)


def term_normal_consistency(side, maps, views, c):
    """The rendered normals held to the normals of the depth, and the normals of the depth held to the rendered normals."""
    f_map, f_prior = (normal_map_loss, normal_prior_loss) if side == "hip" else (normal_map_loss_torch, normal_prior_loss_torch)
    normal, depth, weights = _in(maps["normal"], side), _in(maps["depth_n"], side), _in(maps["weights_n"], side)
    l1, n1 = f_map(normal, weights, _k(c, "normal_target", side), _k(c, "mask_norm", side), mode="cos", min_weight=MIN_WEIGHT, min_norm=MIN_NORM)
    l2, n2 = f_prior(depth, weights, [t.detach() for t in normal], c["pinholes"], _k(c, "mask_length", side), mode="cos", min_weight=MIN_WEIGHT)
    return l1 + l2, n1 + n2


def _pairs(maps, views, side, swap_pair=None):
    D, A = _in(maps["depth"], side), _in(maps["weights"], side)
    Vs = _in(views, side)
    src, dst = [i for i, _ in PAIRS], [j for _, j in PAIRS]
    vi, vj = [Vs[i] for i in src], [Vs[j] for j in dst]
    if swap_pair is not None:                                  # the wrong side of tests/test_step_cpu.py
        vi[swap_pair], vj[swap_pair] = vj[swap_pair], vi[swap_pair]
    return D, A, src, dst, vi, vj


def term_correspondence(side, maps, views, c):
    fn = correspondence_loss if side == "hip" else correspondence_loss_torch
    D, A, src, dst, vi, vj = _pairs(maps, views, side)
    pins = c["pinholes"]
    return fn([D[i] for i in src], [A[i] for i in src], vi, vj, _k(c, "match", side), [pins[i] for i in src], [pins[j] for j in dst],
              _k(c, "conf_match", side), delta=DELTA, min_weight=MIN_WEIGHT, min_depth=MIN_DEPTH)


def term_warp(side, maps, views, c, swap_pair=None):
    fn = warp_loss if side == "hip" else warp_loss_torch
    D, A, src, dst, vi, vj = _pairs(maps, views, side, swap_pair)
    pins, gt = c["pinholes"], _k(c, "gt", side)
    return fn([D[i] for i in src], [A[i] for i in src], vi, vj, [gt[i] for i in src], [gt[j] for j in dst], [pins[i] for i in src],
              [pins[j] for j in dst], _k(c, "conf_warp", side), [D[j].detach() for j in dst], [A[j].detach() for j in dst], eps=EPS,
              occlusion=OCCLUSION, min_weight=MIN_WEIGHT, min_depth=MIN_DEPTH)


def term_depth_smooth(side, maps, views, c, detach_mean=False):
    fn = depth_smooth_loss if side == "hip" else depth_smooth_loss_torch
    D, A = _in(maps["depth"], side), _in(maps["weights"], side)
    kw = dict(space="inverse", order=1, penalty="l1", eps=EPS, gamma=1.0, min_weight=MIN_WEIGHT)
    if detach_mean:                                            # the wrong side of tests/test_step_cpu.py: mu as a constant
        assert side != "hip"
        with torch.no_grad():
            mu = []
            for d, a, m in zip(D, A, _k(c, "mask", side)):
                usable = (a[0] >= MIN_WEIGHT) & (d[0] > 0) & (m > 0)
                mu.append((a[0] / d[0]).double()[usable].mean().to(d.dtype))
        return fn([d * u for d, u in zip(D, mu)], A, _k(c, "gt", side), _k(c, "mask", side), normalize=False, **kw)
    return fn(D, A, _k(c, "gt", side), _k(c, "mask", side), normalize=True, **kw)


def term_normal_smooth(side, maps, views, c):
    fn = normal_smooth_loss if side == "hip" else normal_smooth_loss_torch
    return fn(_in(maps["normal"], side), _in(maps["weights"], side), None, _k(c, "mask_norm", side), order=2, penalty="l2", min_weight=MIN_WEIGHT,
              min_norm=MIN_NORM)


TERM_FUNCTIONS = dict(photo=term_photo, depth_prior=term_depth_prior, normal_prior=term_normal_prior, normal_consistency=term_normal_consistency,
                      correspondence=term_correspondence, warp=term_warp, depth_smooth=term_depth_smooth, normal_smooth=term_normal_smooth)


def terms_of(name):
    return TERMS if name == "all" else (name,)


def run(name, side, maps, views, c, **wrong):
    """The terms of ``name`` (one of TERMS, or "all"): ({term: loss}, {term: count}); ``wrong``: the switches of the wrong sides, passed
    to the term that knows them."""
    assert side in SIDES
    losses, counts = {}, {}
    for t in terms_of(name):
        kw = {k: v for k, v in wrong.items() if (t, k) in (("warp", "swap_pair"), ("depth_smooth", "detach_mean"))}
        losses[t], counts[t] = TERM_FUNCTIONS[t](side, maps, views, c, **kw)
    return losses, counts


def total(losses):
    """The step's scalar: every entry of every loss, weight 1, summed in float64 on the float64 side and in float32 elsewhere."""
    return sum(l.sum() for l in losses.values())


# ---------------------------------------------------------------------------------------------------------------- the rule
def _f64(t):
    return t.detach().double().cpu()


def element_margin(got, r32, r64):
    got, r32, r64 = _f64(got), _f64(r32), _f64(r64)
    bar = FACTOR * (r32 - r64).abs() + FLOOR_EPS * EPS32 * (1.0 + r64.abs())
    worst = ((got - r64).abs() / bar).max().item()
    return worst if math.isfinite(worst) else math.inf                                    # (a NaN fails)


def tensor_err(x, r64):
    x, r64 = _f64(x), _f64(r64)
    return ((x - r64).abs().max() / r64.abs().max()).item()


def tensor_margin(got, r32, r64):
    worst = tensor_err(got, r64) / (FACTOR * tensor_err(r32, r64) + FLOOR_EPS * EPS32)
    return worst if math.isfinite(worst) else math.inf


def map_margins(got, r32, r64):
    """The margins of a gradient at the maps or the view matrices: the per-element rule and, beside it, the per-tensor rule.  The
    gradients of a step are small (every loss is a mean over a thousand pixels and more), so the per-element floor of 16 eps32 * (1 + |r64|)
    alone is a few per cent of the largest of them: a gradient term that is spread thinly over every pixel -- the one through
    ``depth_smooth_loss``'s mean -- can be dropped under it (tests/test_step_cpu.py measures 5 x over the bar, not 10).  The per-tensor
    rule has a floor relative to the largest element and sees it."""
    return {"element": element_margin(got, r32, r64), "tensor": tensor_margin(got, r32, r64)}


def counts_agree(counts, counts64):
    """Every count within eps32 relative of the float64 side's: all sides took the same decisions."""
    return all(bool(((_f64(counts[t]) - _f64(counts64[t])).abs() <= EPS32 * _f64(counts64[t]).abs()).all()) for t in counts64)
