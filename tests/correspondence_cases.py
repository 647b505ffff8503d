"""Cases, float64 reference and bars of tests/test_correspondence_gpu.py -- CPU only, so that tests/test_correspondence_cpu.py can check
the generators and what the bars are built from without a GPU.

``make_case(H, W, K, delta)``  K ordered pairs of ``H x W``: a smooth source depth ``z`` around 3 with per-pair random frequencies, a
                         twenty-fifth of the pixels at ``z`` in [0.3, 0.5] (they land behind the target camera, which stands a unit
                         in front of the source); ``A`` in [0.56, 0.98] with 12 % holes in [0.1, 0.4]; ``D = A z``; view matrices
                         ``A_k = S R_k`` with one world alignment ``S`` (scale 1.3, shear 0.05) per pair and rotations of up to 0.1 rad;
                         matches from the true geometry plus noise of 0 to 3 px in a random direction, so both Huber branches occur
                         at ``delta = 1``; 5 % NaN matches (one component or both); a confidence with a tenth zeros and three tenths
                         fractional; different pinholes on the two sides; per-pair cotangents of mixed sign; all from a seed
                         (cached, never modified).  Images of fewer than 32 pixels have every pixel valid and ``conf = 0.75``.  The
                         generator asserts what keeps float32 and float64 on the same branch (``check_case``).
``degenerate_case(delta)``  the 16-pair case of 17 x 67 with five pairs replaced: nothing solid, an all-zero confidence, all-NaN
                         matches, a singular ``Ai`` (a zero row), the target behind the camera.
                         A case is a dict; the key ``min_weight`` (the chain test's case) overrides ``MIN_WEIGHT``.
``run_torch(case, dt)``  ``correspondence_loss_torch`` in ``dt`` on the host with autograd: (loss, dL/dD, dL/dA, dL/dVi, dL/dVj) as
                         float64 tensors and the count.  ``reference`` is that in float64 (cached), ``float32_path`` in float32.
``closed_form(case)``    the same five from the closed forms of the issue, in float64, with the inverse from ``torch.linalg.inv``, and
                         the four wrong variants of tests/test_correspondence_cpu.py as switches.
``bars(...)``            the project's rule: 4 x what the float32 statement loses against the float64 statement on the same input,
                         plus 16 float32 epsilons times the sum of the absolute values of the terms of the closed form.  Nothing in
                         a bar comes from the kernel.  Where the scale is 0 (an invalid pixel, the fourth column of a matrix
                         gradient, a degenerate pair) the bar is 0: exact zeros.
"""
import functools
import math

import torch

from bags_raster import _lib as L
from bags_raster.correspondence import correspondence_loss_torch
from bags_raster.synth import so3_exp

MIN_WEIGHT = 0.5
MIN_DEPTH = 0.01
FACTOR, FLOOR_EPS = 4.0, 16.0
EPS32 = float(torch.finfo(torch.float32).eps)
F64 = torch.float64
CHUNK = L.CORRESPONDENCE_CHUNK
DELTAS = (1.0, math.inf)
NAMES = ("loss", "dL/dD", "dL/dA", "dL/dVi", "dL/dVj")


def _seam_shape():
    """From the kernel's chunk: more than two chunks with a partial last one, and rows that straddle the seams (W does not divide
    the chunk)."""
    H, W = 7, (2 * CHUNK + CHUNK // 2) // 7 + 1
    assert H * W > 2 * CHUNK and (H * W) % CHUNK != 0 and CHUNK % W != 0 and H * W < 100000
    return H, W


SEAM = _seam_shape()                                         # (7, 92) with a chunk of 256: 644 pixels, three chunks
SHAPES = ((1, 1), (1, CHUNK - 1), (1, CHUNK + 1), (3, 5), (17, 67), SEAM)
PAIRS = (1, 2, 16, 17)
SEED = 3
SMALL = 32                                                   # fewer pixels than this: every pixel valid


def _det3(a):
    return (a[..., 0, 0] * (a[..., 1, 1] * a[..., 2, 2] - a[..., 1, 2] * a[..., 2, 1])
            + a[..., 0, 1] * (a[..., 1, 2] * a[..., 2, 0] - a[..., 1, 0] * a[..., 2, 2])) \
        + a[..., 0, 2] * (a[..., 1, 0] * a[..., 2, 1] - a[..., 1, 1] * a[..., 2, 0])


def _pieces(c, transpose=False):
    """The float64 pieces of the closed forms for the case's maps as they are (z formed in float64): a dict of (K,H,W[,n]) tensors,
    (K,3,3) matrices and (K,) sums.  ``transpose``: the wrong answer with ``Ai^T`` in place of ``inv(Ai)``."""
    D, A, cf = c["D"][:, 0].double(), c["A"][:, 0].double(), c["conf"].double()
    m = c["match"].double().permute(0, 2, 3, 1)
    K, H, W = D.shape
    Vi, Vj = c["Vi"].double(), c["Vj"].double()
    Ai, bi, Aj, bj = Vi[:, :3, :3], Vi[:, 3, :3], Vj[:, :3, :3], Vj[:, 3, :3]
    det = _det3(Ai)
    ok = (det != 0) & torch.isfinite(det)
    safe = torch.where(ok[:, None, None], Ai, torch.eye(3, dtype=F64).expand(K, 3, 3))
    P = safe.transpose(1, 2) if transpose else torch.linalg.inv(safe)
    M = P @ Aj
    cc = bj - (bi[:, None, :] @ M)[:, 0]
    solid = (A >= c.get("min_weight", MIN_WEIGHT)) & (D > 0)
    z = torch.where(solid, D, torch.ones_like(D)) / torch.where(solid, A, torch.ones_like(A))
    pi, pj = c["pin_i"].double(), c["pin_j"].double()
    e3 = lambda t: t[:, None, None]                                                      # noqa: E731
    u = torch.arange(W, dtype=F64)[None, None, :].expand(K, H, W)
    v = torch.arange(H, dtype=F64)[None, :, None].expand(K, H, W)
    ray = torch.stack([(u - e3(pi[:, 2])) / e3(pi[:, 0]), (v - e3(pi[:, 3])) / e3(pi[:, 1]), torch.ones(K, H, W, dtype=F64)], -1)
    xi = z[..., None] * ray
    xj = (xi.reshape(K, H * W, 3) @ M).reshape(K, H, W, 3) + cc[:, None, None, :]
    zj = xj[..., 2]
    finite = torch.isfinite(m).all(-1)
    front = zj >= MIN_DEPTH
    valid = solid & e3(ok) & (cf > 0) & finite & front
    xs = torch.where(valid[..., None], xj, torch.tensor((0.0, 0.0, 1.0), dtype=F64))
    proj = torch.stack([e3(pj[:, 0]) * xs[..., 0] / xs[..., 2] + e3(pj[:, 2]), e3(pj[:, 1]) * xs[..., 1] / xs[..., 2] + e3(pj[:, 3])], -1)
    r = torch.where(valid[..., None], proj - torch.where(finite[..., None], m, torch.zeros_like(m)), torch.zeros_like(proj))
    e = torch.sqrt((r * r).sum(-1))
    w = torch.where(valid, cf, torch.zeros_like(cf))
    return dict(valid=valid, solid=solid, ok=ok, finite=finite, front=front, z=z, A=A, ray=ray, xi=xi, xj=xs, zj=zj, r=r, e=e, w=w,
                cnt=w.sum((1, 2)), P=P, M=M, c=cc, Ai=Ai, Aj=Aj, bi=bi, det=det, cf=cf, pj=pj)


def check_case(c):
    """What keeps float32 and float64 on the same branch, and the case non-trivial; returns the figures."""
    q = _pieces(c)
    K, H, W = q["z"].shape
    gap = float((q["A"] - c.get("min_weight", MIN_WEIGHT)).abs().min())
    assert gap >= 1e-3, gap                                                               # no A within 1e-3 of min_weight
    live = [k for k in range(K) if k not in c["degenerate"]]
    reach = q["solid"] & q["ok"][:, None, None]
    front = float((q["zj"] - MIN_DEPTH).abs()[reach].min()) if reach.any() else 1.0
    assert front >= 1e-3, front                                                           # no x_j.z within 1e-3 of min_depth
    figures = dict(gap=gap, front=front, valid=1.0, linear=None)
    for k in live:
        share = float(q["valid"][k].double().mean())
        assert share >= 0.5, (k, share)                                                   # at least half of the pixels valid
        figures["valid"] = min(figures["valid"], share)
    if H * W >= 200 and live:                                                             # every reason for invalidity occurs
        s = q["solid"][live]
        assert (~s).any() and (s & ~(q["cf"][live] > 0)).any() and (s & ~q["finite"][live]).any() and (s & ~q["front"][live]).any()
        if math.isfinite(c["delta"]):                                                     # both Huber branches occur
            lin = (q["e"][live] > c["delta"]) & q["valid"][live]
            quad = (q["e"][live] <= c["delta"]) & q["valid"][live]
            assert lin.any() and quad.any()
            figures["linear"] = float(lin.sum()) / float(q["valid"][live].sum())
    ortho = (q["Ai"].transpose(1, 2) @ q["Ai"] - torch.eye(3, dtype=F64)).abs().amax((1, 2))
    assert int((ortho[live] > 0.1).sum()) * 2 >= len(live)                                # Ai is not orthonormal in at least half the pairs
    return figures


def _view(g):
    """``S R`` with an alignment ``S`` (scale 1.3, shear 0.05, turned by up to 0.3 rad per axis) and a rotation of up to 0.1 rad per
    axis, and a translation of up to 0.2 per axis: the (4,4) matrix and ``S``."""
    S = 1.3 * torch.eye(3, dtype=F64)
    S[0, 1] += 0.05
    S = so3_exp(0.3 * (2 * torch.rand(3, generator=g) - 1)).double() @ S
    R = so3_exp(0.1 * (2 * torch.rand(3, generator=g) - 1)).double()
    V = torch.eye(4, dtype=F64)
    V[:3, :3] = S @ R
    V[3, :3] = 0.2 * (2 * torch.rand(3, generator=g, dtype=F64) - 1)
    return V, S


@functools.lru_cache(maxsize=None)
def make_case(H, W, K, delta, seed=SEED):
    g = torch.Generator().manual_seed(1000003 * seed + 7919 * H + 31 * W + K)
    px = H * W
    rnd = lambda *s: torch.rand(*s, generator=g)                                         # noqa: E731
    size = float(max(H, W, 16))

    def pinholes():
        fx = size * (0.9 + 0.3 * rnd(K))
        return torch.stack([fx, fx * (1.0 + 0.05 * (2 * rnd(K) - 1)), (W - 1) / 2 + 1.5 * (2 * rnd(K) - 1), (H - 1) / 2 + 1.5 * (2 * rnd(K) - 1)], 1).double()

    pin_i, pin_j = pinholes(), pinholes()
    u = torch.arange(W, dtype=torch.float32)[None, None, :] / max(W, 32)
    v = torch.arange(H, dtype=torch.float32)[None, :, None] / max(H, 32)
    f, ph0 = 0.5 + 0.75 * rnd(K, 2), 6.2831853 * rnd(K, 2)
    z = 3.0 + 0.5 * torch.sin(6.2831853 * f[:, 0, None, None] * u + ph0[:, 0, None, None]) * torch.cos(6.2831853 * f[:, 1, None, None] * v + ph0[:, 1, None, None])
    z = z.reshape(K, px).contiguous()
    A = 0.56 + 0.42 * rnd(K, px)
    conf = torch.ones(K, px)
    Vi, Vj = torch.zeros(K, 4, 4, dtype=F64), torch.zeros(K, 4, 4, dtype=F64)
    small = px < SMALL
    n_near, n_hole, n_off, n_frac, n_nan = px // 25, (12 * px) // 100, px // 10, (3 * px) // 10, px // 20
    for k in range(K):
        Vi[k], S = _view(g)
        # the target: the source's alignment, another rotation, and a unit nearer to the scene (x_j.z = z - 1 or so)
        R = so3_exp(0.1 * (2 * torch.rand(3, generator=g) - 1)).double()
        Vj[k] = torch.eye(4, dtype=F64)
        Vj[k, :3, :3] = S @ R
        Vj[k, 3, :3] = torch.tensor((0.0, 0.0, -1.0), dtype=F64) + 0.2 * (2 * torch.rand(3, generator=g, dtype=F64) - 1)
        if small:
            continue
        z[k, torch.randperm(px, generator=g)[:n_near]] = 0.3 + 0.2 * rnd(n_near)
        A[k, torch.randperm(px, generator=g)[:n_hole]] = 0.1 + 0.3 * rnd(n_hole)
        at = torch.randperm(px, generator=g)
        conf[k, at[:n_off]] = 0.0
        conf[k, at[n_off:n_off + n_frac]] = 0.1 + 0.9 * rnd(n_frac)
    if small:
        conf[:] = 0.75                                       # cnt != the number of pixels also for a single pixel
    D = A * z
    Vi, Vj = Vi.float(), Vj.float()                          # what the kernel is given
    c = dict(H=H, W=W, K=K, delta=delta, D=D.view(K, 1, H, W), A=A.view(K, 1, H, W), conf=conf.view(K, H, W), Vi=Vi, Vj=Vj, pin_i=pin_i,
             pin_j=pin_j, match=torch.zeros(K, 2, H, W), degenerate=())
    q = _pieces(c)                                           # the true geometry: proj of every pixel (valid where conf > 0)
    fx, fy, cx, cy = (c["pin_j"][:, i, None, None] for i in range(4))
    xj = torch.where((q["zj"] >= MIN_DEPTH)[..., None], (q["xi"].reshape(K, px, 3) @ q["M"]).reshape(K, H, W, 3) + q["c"][:, None, None, :],
                     torch.tensor((0.0, 0.0, 1.0), dtype=F64))
    true = torch.stack([fx * xj[..., 0] / xj[..., 2] + cx, fy * xj[..., 1] / xj[..., 2] + cy], 1)
    ang, mag = 6.2831853 * rnd(K, H, W), 3.0 * rnd(K, H, W)
    match = (true + torch.stack([mag * torch.cos(ang), mag * torch.sin(ang)], 1).double()).float()
    for k in range(K if not small else 0):
        at = torch.randperm(px, generator=g)[:n_nan]
        kind = torch.randint(0, 3, (n_nan,), generator=g)    # x, y or both
        flat = match[k].view(2, px)
        flat[0, at[kind != 1]] = float("nan")
        flat[1, at[kind != 0]] = float("nan")
    c["match"] = match.contiguous()
    c["cot"] = (0.5 + rnd(K)) * torch.where(torch.arange(K) % 2 == 0, 1.0, -1.0)
    c["figures"] = check_case(c)
    return c


DEGENERATE_PAIRS = {"none_solid": 2, "conf_zero": 5, "match_nan": 9, "singular": 11, "behind": 14}


@functools.lru_cache(maxsize=None)
def degenerate_case(delta):
    """The 16-pair case of 17 x 67 with the five pairs of DEGENERATE_PAIRS replaced; the other eleven are that case's."""
    base = make_case(17, 67, 16, delta)
    c = {k: (v.clone() if torch.is_tensor(v) else v) for k, v in base.items()}
    k = DEGENERATE_PAIRS
    c["A"][k["none_solid"]] = 0.125
    c["D"][k["none_solid"]] = 0.125 * 3.0
    c["conf"][k["conf_zero"]] = 0.0
    c["match"][k["match_nan"]] = float("nan")
    c["Vi"][k["singular"], 1, :3] = 0.0                      # a zero row: det(Ai) is an exact zero however it is evaluated
    c["Vj"][k["behind"], 3, 2] = -10.0
    c["degenerate"] = tuple(k.values())
    c["figures"] = check_case(c)
    return c


def run_torch(c, dtype, pairs=None):
    """(loss (K,), dL/dD (K,1,H,W), dL/dA (K,1,H,W), dL/dVi (K,4,4), dL/dVj (K,4,4)) of correspondence_loss_torch in ``dtype`` on the
    host for L = sum cot_k loss_k, as float64, and the count (K,)."""
    idx = list(range(c["K"])) if pairs is None else list(pairs)
    leaf = lambda t: t.detach().clone().to(dtype).requires_grad_(True)                   # noqa: E731  (the cached case stays as it is)
    D, A = [leaf(c["D"][i]) for i in idx], [leaf(c["A"][i]) for i in idx]
    Vi, Vj = [leaf(c["Vi"][i]) for i in idx], [leaf(c["Vj"][i]) for i in idx]
    loss, count = correspondence_loss_torch(D, A, Vi, Vj, [c["match"][i].to(dtype) for i in idx], c["pin_i"][idx], c["pin_j"][idx],
                                            [c["conf"][i].to(dtype) for i in idx], delta=c["delta"], min_weight=c.get("min_weight", MIN_WEIGHT), min_depth=MIN_DEPTH)
    assert loss.dtype == dtype and count.dtype == dtype and not count.requires_grad
    (loss.double() * c["cot"][idx].double()).sum().backward()
    grads = lambda ts: torch.stack([torch.zeros_like(t) if t.grad is None else t.grad for t in ts]).double()      # noqa: E731
    return loss.detach().double(), grads(D), grads(A), grads(Vi), grads(Vj), count.detach().double()


@functools.lru_cache(maxsize=None)
def reference(H, W, K, delta):
    return run_torch(make_case(H, W, K, delta), F64)


@functools.lru_cache(maxsize=None)
def float32_path(H, W, K, delta):
    return run_torch(make_case(H, W, K, delta), torch.float32)


def _pad44(A3, b3):
    K = A3.shape[0]
    out = torch.zeros(K, 4, 4, dtype=F64)
    out[:, :3, :3] = A3
    out[:, 3, :3] = b3
    return out


def _chain(q, GM, gc, absolute=False):
    """The two (K,4,4) matrix gradients from G_M = sum x_i^T g_xj (K,3,3) and g_c = sum g_xj (K,3); ``absolute``: the sum of the
    absolute values of the terms instead."""
    P, M, bi = q["P"], q["M"], q["bi"]
    ok = q["ok"][:, None, None].double()
    if absolute:
        P, M, bi = P.abs(), M.abs(), bi.abs()
        G = GM + bi[:, :, None] * gc[:, None, :]
        gAi, gbi = P.transpose(1, 2) @ G @ M.transpose(1, 2), (M @ gc[:, :, None])[:, :, 0]
    else:
        G = GM - bi[:, :, None] * gc[:, None, :]
        gAi, gbi = -(P.transpose(1, 2) @ G @ M.transpose(1, 2)), -(M @ gc[:, :, None])[:, :, 0]
    gAj = P.transpose(1, 2) @ G
    return _pad44(gAi, gbi) * ok, _pad44(gAj, gc) * ok


def _pixel_terms(c, q, inv_g, drop_delta_over_e=False):
    """s w d rho/dr (K,H,W,2) of the closed form."""
    e3 = lambda t: t[:, None, None]                                                      # noqa: E731
    s = e3(c["cot"].double()) * q["w"] * e3(inv_g)
    if math.isfinite(c["delta"]) and not drop_delta_over_e:
        lin = q["e"] > c["delta"]
        s = torch.where(lin, s * c["delta"] / torch.where(lin, q["e"], torch.ones_like(q["e"])), s)
    return s[..., None] * q["r"]


def closed_form(c, transpose=False, flip_dA=False, n_is_pixels=False, drop_delta_over_e=False):
    """(loss, dL/dD, dL/dA, dL/dVi, dL/dVj) from the closed forms, in float64, the cotangent included.  The switches make the four
    wrong answers the bars must reject: ``Ai^T`` in place of ``inv(Ai)``, the sign of dL/dA flipped, 1/cnt of the gradient replaced
    by 1 / (H W), the linear branch's gradient without its ``delta / e`` factor."""
    q = _pieces(c, transpose)
    cnt, w, e, xj = q["cnt"], q["w"], q["e"], q["xj"]
    K, H, W = w.shape
    inv = torch.where(cnt > 0, 1.0 / cnt.clamp_min(1e-300), torch.zeros_like(cnt))
    inv_g = torch.where(cnt > 0, torch.full_like(cnt, 1.0 / (H * W)), inv) if n_is_pixels else inv
    delta = c["delta"]
    rho = 0.5 * e * e
    if math.isfinite(delta):
        rho = torch.where(e <= delta, rho, delta * (e - 0.5 * delta))
    loss = (w * rho).sum((1, 2)) * inv
    gr = _pixel_terms(c, q, inv_g, drop_delta_over_e)
    gx, gy = gr[..., 0] * q["pj"][:, 0, None, None], gr[..., 1] * q["pj"][:, 1, None, None]
    gj = torch.stack([gx / xj[..., 2], gy / xj[..., 2], -(gx * xj[..., 0] + gy * xj[..., 1]) / xj[..., 2] ** 2], -1)
    gi = (gj.reshape(K, H * W, 3) @ q["M"].transpose(1, 2)).reshape(K, H, W, 3)
    gz = (q["ray"] * gi).sum(-1)
    gD = gz / q["A"]
    gA = -(q["z"] / q["A"]) * gz * (-1.0 if flip_dA else 1.0)
    zero = torch.zeros_like(gz)
    xi = torch.where(q["valid"][..., None], q["xi"], torch.zeros_like(q["xi"]))
    GM = xi.reshape(K, H * W, 3).transpose(1, 2) @ gj.reshape(K, H * W, 3)
    gVi, gVj = _chain(q, GM, gj.sum((1, 2)))
    return loss, torch.where(q["valid"], gD, zero)[:, None], torch.where(q["valid"], gA, zero)[:, None], gVi, gVj


def scales(c):
    """sum |terms| of the closed forms in float64: (loss (K,), dL/dD (K,1,H,W), dL/dA (K,1,H,W), dL/dVi (K,4,4), dL/dVj (K,4,4))."""
    q = _pieces(c)
    cnt, xj = q["cnt"], q["xj"].abs()
    K, H, W = q["w"].shape
    inv = torch.where(cnt > 0, 1.0 / cnt.clamp_min(1e-300), torch.zeros_like(cnt))
    loss = closed_form(c)[0].abs()                                                        # every term of the loss is non-negative
    gr = _pixel_terms(c, q, inv).abs()
    gx, gy = gr[..., 0] * q["pj"][:, 0, None, None].abs(), gr[..., 1] * q["pj"][:, 1, None, None].abs()
    gj = torch.stack([gx / xj[..., 2], gy / xj[..., 2], (gx * xj[..., 0] + gy * xj[..., 1]) / xj[..., 2] ** 2], -1)
    gi = (gj.reshape(K, H * W, 3) @ q["M"].abs().transpose(1, 2)).reshape(K, H, W, 3)
    gz = (q["ray"].abs() * gi).sum(-1)
    zero = torch.zeros_like(gz)
    xi = torch.where(q["valid"][..., None], q["xi"].abs(), torch.zeros_like(q["xi"]))
    GM = xi.reshape(K, H * W, 3).transpose(1, 2) @ gj.reshape(K, H * W, 3)
    sVi, sVj = _chain(q, GM, gj.sum((1, 2)), absolute=True)
    return loss, torch.where(q["valid"], gz / q["A"], zero)[:, None], torch.where(q["valid"], (q["z"] / q["A"]) * gz, zero)[:, None], sVi, sVj


def bars_of(c, r64, r32):
    """The five bars from the two runs of the statement and the case's scales."""
    return tuple(FACTOR * (b - a).abs() + FLOOR_EPS * EPS32 * s for a, b, s in zip(r64[:5], r32[:5], scales(c)))


@functools.lru_cache(maxsize=None)
def bars(H, W, K, delta):
    return bars_of(make_case(H, W, K, delta), reference(H, W, K, delta), float32_path(H, W, K, delta))


def margins_of(bar, ref, got):
    """Largest error over bar of each of the five against ``ref``; where a bar is 0 the value must be the reference's exactly (an
    invalid pixel, a fourth column, a degenerate pair: zeros), which counts as margin 0 -- anything else as infinity."""
    m = []
    for b, r, g in zip(bar, ref[:5], got):
        err = (g.detach().double().cpu() - r).abs()
        ratio = torch.where(b > 0, err / b.clamp_min(1e-300), torch.where(err == 0, torch.zeros_like(err), torch.full_like(err, float("inf"))))
        ratio = torch.where(torch.isnan(err), torch.full_like(err, float("inf")), ratio)
        m.append(float(ratio.max()))
    return tuple(m)


def margins(H, W, K, delta, got):
    return margins_of(bars(H, W, K, delta), reference(H, W, K, delta), got)
