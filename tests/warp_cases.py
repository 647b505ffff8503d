"""Cases, float64 reference and bars of tests/test_warp_gpu.py -- CPU only, so that tests/test_warp_cpu.py can check the generators and
what the bars are built from without a GPU.

``make_case(H, W, K, C, eps)``  K ordered pairs of ``H x W`` sources and one target size ``(Hd, Wd) = (H + 2, W + 3)``.  The source
                         side is the correspondence cases': a smooth depth ``z`` around 3, a fiftieth of the pixels at ``z`` in
                         [0.3, 0.5] (they land behind the target camera, which stands a unit in front of the source), ``A`` in
                         [0.56, 0.98] with 6 % holes in [0.1, 0.4], ``D = A z``, view matrices ``A_k = S R_k`` with one world alignment
                         ``S`` (scale 1.3, shear 0.05) per pair, a confidence with a twentieth zeros and three tenths fractional,
                         mixed-sign cotangents.  The target pinhole of a pair is chosen from the float64 geometry so that the central
                         share s of ``x_j.x / x_j.z`` maps onto ``[0, Wd - 1]``, and likewise for y, with s such that 0.81 of the
                         projections fall inside and 0.19 outside: s = 0.9 where x and y are independent, less in a single row.
                         (0.8 per axis leaves 0.64 inside; with a tenth of the target pixels holes and the occluded ones on top,
                         no pair could keep half of its pixels valid, which ``check_case`` demands.)
                         ``image_dst`` is a sum of sinusoids per channel with amplitude of order 1 and periods of 6 to 14 pixels,
                         with one NaN texel per pair; ``color_src`` is the true warped colour plus noise of 1e-4 to 0.5 in magnitude,
                         so residuals lie on both sides of ``eps`` = 1e-3 and 0.1, with 1 % NaN colours.  The target maps are the
                         mean of ``x_j.z`` of the source pixels that land on a target pixel (the overall mean elsewhere), a twentieth
                         of the target pixels moved by a quarter (occluders), ``A_t`` in [0.56, 0.98] with a tenth holes; pair 1 of a
                         case of two or more has no target maps.  Images of fewer than 32 pixels have every projection inside, no
                         holes, no occluders, ``conf = 0.75``.
                         GUARDS: float32 and float64 must take the same decisions, so the generator sets ``conf = 0`` where the float64
                         reference lies within 1e-3 of a cell line (``|proj - round(proj)|`` in either axis, which is also the border
                         of ``inside``), of the occlusion threshold, or -- where there are target maps -- of a line between two nearest
                         pixels (``proj + 0.5`` near a whole number: the neighbour may be a hole).  ``check_case`` asserts the
                         conditions for every case made.  Geometry, images and maps do not depend on ``C`` (the first channels) or on
                         ``eps``.  All from a seed: the first of up to ``ATTEMPTS`` draws on which the conditions hold (cached, never
                         modified).
                         A case is a dict; the key ``min_weight`` (the chain test's case) overrides ``MIN_WEIGHT``.
``degenerate_case(C, eps)``  the 16-pair case of 17 x 67 with six pairs replaced: nothing solid, an all-zero confidence, a singular ``Ai``
                         (a zero row), the target behind the camera, every projection outside the image, everything occluded.
``run_torch(case, dt)``  ``warp_loss_torch`` in ``dt`` on the host with autograd: (loss, dL/dD, dL/dA, dL/dVi, dL/dVj) as float64 tensors
                         and the count.  ``reference`` is that in float64 (cached), ``float32_path`` in float32.
``closed_form(case)``    the same five from the closed forms of the issue, in float64, with the inverse from ``torch.linalg.inv``, and
                         the four wrong variants of tests/test_warp_cpu.py as switches.
``bars(...)``            the project's rule: 4 x what the float32 statement loses against the float64 statement on the same input,
                         plus 16 float32 epsilons times the sum of the absolute values of the terms of the closed form.  Nothing in
                         a bar comes from the kernel.  Where the scale is 0 (an invalid pixel, the fourth column of a matrix
                         gradient, a degenerate pair) the bar is 0: exact zeros.
"""
import functools

import torch

import correspondence_cases as CC
from bags_raster import _lib as L
from bags_raster.synth import so3_exp
from bags_raster.warp import warp_loss_torch

MIN_WEIGHT = CC.MIN_WEIGHT
MIN_DEPTH = CC.MIN_DEPTH
OCCLUSION = 0.05
FACTOR, FLOOR_EPS, EPS32, F64 = CC.FACTOR, CC.FLOOR_EPS, CC.EPS32, CC.F64
CHUNK = L.CORRESPONDENCE_CHUNK
SEAM = CC.SEAM
SHAPES = CC.SHAPES                                           # from the kernel's chunk: (1,1), (1,255), (1,257), (3,5), (17,67), the seam shape
PAIRS = (1, 2, 16, 17)
CHANNELS = (1, 3)
EPSES = (1e-3, 0.1)
NAMES = CC.NAMES
SEED = 5
SMALL = 32                                                   # fewer pixels than this: every pixel valid
CLEAR = 1e-3                                                 # the guards' distance
CENTRAL = 0.90                                               # the largest share of x_j.x / x_j.z (and of y) that maps onto the target image
INSIDE = 0.81                                                # the share of a pair's projections that falls inside it (0.9 x 0.9)
margins_of = CC.margins_of


def size_dst(H, W):
    return H + 2, W + 3


def _e3(t):
    return t[:, None, None]


def _taps(T, y0, x0, y1, x1):
    """T (K,C,Hd,Wd), indices (K,H,W): the four taps (K,C,H,W) each."""
    K = T.shape[0]
    k = torch.arange(K)[:, None, None]
    g = lambda y, x: T[k, :, y, x].permute(0, 3, 1, 2)                                   # noqa: E731
    return g(y0, x0), g(y0, x1), g(y1, x0), g(y1, x1)


def _pieces(c, half_pixel=False):
    """The float64 pieces of the closed forms for the case's maps as they are (z and z_t formed in float64): a dict of (K,H,W[,n])
    tensors, (K,3,3) matrices and (K,) sums.  ``half_pixel``: the wrong answer that samples at ``proj + 0.5``."""
    D, A, cf = c["D"][:, 0].double(), c["A"][:, 0].double(), c["conf"].double()
    K, H, W = D.shape
    Hd, Wd = c["Hd"], c["Wd"]
    C = c["C"]
    Vi, Vj = c["Vi"].double(), c["Vj"].double()
    Ai, bi, Aj, bj = Vi[:, :3, :3], Vi[:, 3, :3], Vj[:, :3, :3], Vj[:, 3, :3]
    det = CC._det3(Ai)
    ok = (det != 0) & torch.isfinite(det)
    safe = torch.where(ok[:, None, None], Ai, torch.eye(3, dtype=F64).expand(K, 3, 3))
    P = torch.linalg.inv(safe)
    M = P @ Aj
    cc = bj - (bi[:, None, :] @ M)[:, 0]
    min_weight = c.get("min_weight", MIN_WEIGHT)
    solid = (A >= min_weight) & (D > 0)
    z = torch.where(solid, D, torch.ones_like(D)) / torch.where(solid, A, torch.ones_like(A))
    pi, pj = c["pin_i"].double(), c["pin_j"].double()
    u = torch.arange(W, dtype=F64)[None, None, :].expand(K, H, W)
    v = torch.arange(H, dtype=F64)[None, :, None].expand(K, H, W)
    ray = torch.stack([(u - _e3(pi[:, 2])) / _e3(pi[:, 0]), (v - _e3(pi[:, 3])) / _e3(pi[:, 1]), torch.ones(K, H, W, dtype=F64)], -1)
    xi = z[..., None] * ray
    xj = (xi.reshape(K, H * W, 3) @ M).reshape(K, H, W, 3) + cc[:, None, None, :]
    zj = xj[..., 2]
    front = zj >= MIN_DEPTH
    reach = solid & _e3(ok) & front                                                       # geometric
    xs = torch.where(reach[..., None], xj, torch.tensor((0.0, 0.0, 1.0), dtype=F64))
    x = _e3(pj[:, 0]) * xs[..., 0] / xs[..., 2] + _e3(pj[:, 2])
    y = _e3(pj[:, 1]) * xs[..., 1] / xs[..., 2] + _e3(pj[:, 3])
    inside = reach & (x >= 0) & (x <= Wd - 1) & (y >= 0) & (y <= Hd - 1)
    sx, sy = torch.where(inside, x, torch.zeros_like(x)), torch.where(inside, y, torch.zeros_like(y))
    # the occlusion test at the nearest target pixel
    has = c["has_dst"]                                                                    # (K,) bool
    nx, ny = torch.floor(sx + 0.5).long(), torch.floor(sy + 0.5).long()
    k = torch.arange(K)[:, None, None]
    Dt, At = c["D_dst"][:, 0].double()[k, ny, nx], c["A_dst"][:, 0].double()[k, ny, nx]
    solid_t = (At >= min_weight) & (Dt > 0)
    zt = torch.where(solid_t, Dt, torch.ones_like(Dt)) / torch.where(solid_t, At, torch.ones_like(At))
    miss = (zj - zt).abs() - OCCLUSION * zt                                               # <= 0: passes
    visible = ~_e3(has) | (solid_t & (miss <= 0))
    # the bilinear cell
    if half_pixel:
        sx, sy = (sx + 0.5).clamp(max=Wd - 1), (sy + 0.5).clamp(max=Hd - 1)
    fx0, fy0 = torch.floor(sx), torch.floor(sy)
    x0, y0 = fx0.long(), fy0.long()
    x1, y1 = (x0 + 1).clamp(max=Wd - 1), (y0 + 1).clamp(max=Hd - 1)
    ax, ay = (sx - fx0)[:, None], (sy - fy0)[:, None]
    T = c["image"].double()[:, :C]
    t00, t01, t10, t11 = _taps(T, y0, x0, y1, x1)
    S = (1 - ay) * ((1 - ax) * t00 + ax * t01) + ay * ((1 - ax) * t10 + ax * t11)
    col = c["color"].double()[:, :C]
    finite = torch.isfinite(S).all(1) & torch.isfinite(col).all(1)
    valid = inside & visible & (cf > 0) & finite
    live = valid[:, None]
    zero = torch.zeros_like(S)
    t00, t01, t10, t11 = (torch.where(live, t, zero) for t in (t00, t01, t10, t11))
    S = torch.where(live, S, zero)
    r = torch.where(live, S - torch.where(live, col, zero), zero)
    w = torch.where(valid, cf, torch.zeros_like(cf))
    return dict(valid=valid, solid=solid, ok=ok, front=front, reach=reach, inside=inside, visible=visible, finite=finite, solid_t=solid_t,
                miss=miss, has=has, x=x, y=y, z=z, A=A, ray=ray, xi=xi, xj=xs, zj=zj, ax=ax, ay=ay, taps=(t00, t01, t10, t11), S=S, r=r, w=w,
                cnt=w.sum((1, 2)), P=P, M=M, c=cc, Ai=Ai, Aj=Aj, bi=bi, det=det, cf=cf, pj=pj, At=At)


def guard_mask(c, q=None):
    """(K,H,W) bool: where the float64 reference lies within CLEAR of a decision float32 could take the other way -- a cell line of
    the bilinear sample (also the border of ``inside``), the occlusion threshold, a line between two nearest target pixels."""
    q = _pieces(c) if q is None else q
    Hd, Wd = c["Hd"], c["Wd"]
    x, y = q["x"], q["y"]
    near = q["reach"] & (x >= -CLEAR) & (x <= Wd - 1 + CLEAR) & (y >= -CLEAR) & (y <= Hd - 1 + CLEAR)
    line = lambda t: (t - torch.round(t)).abs() < CLEAR                                   # noqa: E731
    cell = near & (line(x) | line(y))
    maps = near & _e3(q["has"])
    half = maps & (line(x + 0.5) | line(y + 0.5))
    threshold = maps & q["inside"] & q["solid_t"] & (q["miss"].abs() < CLEAR)
    return cell | half | threshold, cell


def check_case(c):
    """What keeps float32 and float64 on the same branch, and the case non-trivial; returns the figures."""
    q = _pieces(c)
    K, H, W = q["z"].shape
    gap = float((q["A"] - c.get("min_weight", MIN_WEIGHT)).abs().min())
    assert gap >= CLEAR, gap                                                              # no A within 1e-3 of min_weight
    gap_t = float((c["A_dst"].double() - c.get("min_weight", MIN_WEIGHT)).abs().min())
    assert gap_t >= CLEAR, gap_t                                                          # ... and no A_t
    live = [k for k in range(K) if k not in c["degenerate"]]
    reach = q["solid"] & _e3(q["ok"])
    front = float((q["zj"] - MIN_DEPTH).abs()[reach].min()) if reach.any() else 1.0
    assert front >= CLEAR, front                                                          # no x_j.z within 1e-3 of min_depth
    guard, cell = guard_mask(c, q)
    assert bool((q["cf"][guard] == 0).all())                                              # conf = 0 at every guarded pixel ...
    assert torch.equal(guard[live], c["guarded"][live])                                   # ... and the generator set it there and nowhere else
    figures = dict(gap=min(gap, gap_t), front=front, valid=1.0, guard=0.0, cell=(1.0, 0.0), inside=(1.0, 0.0), outside=1.0, occluded=(1.0, 0.0))
    for k in live:
        share = float(q["valid"][k].double().mean())
        assert share >= 0.5, (k, share)                                                   # at least half of the pixels valid
        figures["valid"] = min(figures["valid"], share)
        g = float(guard[k].double().mean())
        assert g <= 0.03, (k, g)                                                          # the guards take out at most 3 % of a pair's pixels
        figures["guard"] = max(figures["guard"], g)
        cl = float(cell[k].double().mean())
        figures["cell"] = (min(figures["cell"][0], cl), max(figures["cell"][1], cl))
        ins = float(q["inside"][k].double().mean())
        figures["inside"] = (min(figures["inside"][0], ins), max(figures["inside"][1], ins))
        figures["outside"] = min(figures["outside"], float((q["reach"][k] & ~q["inside"][k]).double().sum() / q["reach"][k].double().sum().clamp_min(1)))
        if bool(q["has"][k]) and H * W >= SMALL:
            occ = float((q["inside"][k] & ~q["visible"][k]).double().sum() / q["inside"][k].double().sum())
            assert 0.10 <= occ <= 0.20, (k, occ)                                          # 10 to 20 % fail the occlusion test
            figures["occluded"] = (min(figures["occluded"][0], occ), max(figures["occluded"][1], occ))
    if H * W < SMALL and live:                                                            # every projection inside
        assert bool(q["inside"][live].all())
    if H * W >= 200 and live:                                                             # every reason for invalidity occurs
        s, cf = q["solid"][live], q["cf"][live]
        assert (~s).any() and (s & ~(cf > 0)).any() and (s & ~q["front"][live]).any()
        assert (q["reach"][live] & ~q["inside"][live]).any() and (q["inside"][live] & ~q["finite"][live]).any()
        if q["has"][live].any():
            assert (q["inside"][live] & ~q["visible"][live]).any()
        assert figures["outside"] >= 0.17, figures["outside"]
    if live and q["valid"][live].any():                                                   # residuals on both sides of eps
        r = q["r"][live].abs()[q["valid"][live][:, None].expand_as(q["r"][live])]
        if H * W >= SMALL:
            assert (r < c["eps"]).any() and (r > c["eps"]).any()
    ortho = (q["Ai"].transpose(1, 2) @ q["Ai"] - torch.eye(3, dtype=F64)).abs().amax((1, 2))
    assert int((ortho[live] > 0.1).sum()) * 2 >= len(live)                                # Ai is not orthonormal in at least half the pairs
    return figures


def _texture(g, K, Hd, Wd):
    """(K,3,Hd,Wd) float32: per pair and channel 0.5 + 0.4 sin cos + 0.3 sin, periods of 6 to 14 pixels."""
    x = torch.arange(Wd, dtype=F64)[None, None, None, :]
    y = torch.arange(Hd, dtype=F64)[None, None, :, None]
    rnd = lambda: torch.rand(K, 3, 1, 1, generator=g, dtype=F64)                          # noqa: E731
    per = lambda: 6.0 + 8.0 * rnd()                                                       # noqa: E731
    tau = 6.283185307179586
    T = 0.5 + 0.4 * torch.sin(tau * (x / per() + rnd())) * torch.cos(tau * (y / per() + rnd())) + 0.3 * torch.sin(tau * ((x + y) / per() + rnd()))
    return T.float()


def _target_pinholes(q_x, q_y, reach, Hd, Wd, small, offset):
    """(K,4) float64: per pair the pinhole that maps the central share s of X = x_j.x / x_j.z onto [0, Wd - 1] and of Y = x_j.y / x_j.z
    onto [0, Hd - 1], with s (at most CENTRAL, by bisection) such that INSIDE of the pair's projections fall inside the image: 0.9 per
    axis where X and Y are independent, less where they are not (a single row).  ``small``: every X onto the middle 0.8 of the image,
    ``offset`` px off its centre."""
    K = q_x.shape[0]
    out = torch.zeros(K, 4, dtype=F64)
    cap = 8.0 * max(Hd, Wd)

    def axis_of(vals, n, s, off):
        if small:
            lo, hi = float(vals.min()), float(vals.max())
            f = min(0.8 * (n - 1) / max(hi - lo, 1e-12), cap)
            return f, 0.5 * (n - 1) + off - f * 0.5 * (lo + hi)
        lo, hi = float(torch.quantile(vals, 0.5 - s / 2)), float(torch.quantile(vals, 0.5 + s / 2))
        f = (n - 1) / max(hi - lo, 1e-12)
        return (f, -f * lo) if f <= cap else (cap, 0.5 * (n - 1) + off - cap * float(vals.median()))

    def pinhole(k, s):
        X, Y = q_x[k][reach[k]], q_y[k][reach[k]]
        (fx, cx), (fy, cy) = axis_of(X, Wd, s, offset[0]), axis_of(Y, Hd, s, offset[1])
        x, y = fx * X + cx, fy * Y + cy
        return (fx, fy, cx, cy), float(((x >= 0) & (x <= Wd - 1) & (y >= 0) & (y <= Hd - 1)).double().mean())

    for k in range(K):
        lo, hi = 0.5, CENTRAL
        pin, share = pinhole(k, hi)
        if not small and share > INSIDE:
            for _ in range(30):
                mid = 0.5 * (lo + hi)
                pin, share = pinhole(k, mid)
                lo, hi = (mid, hi) if share < INSIDE else (lo, mid)
            pin, share = pinhole(k, lo)
        out[k] = torch.tensor(pin, dtype=F64)
    return out


ATTEMPTS = 32


@functools.lru_cache(maxsize=None)
def _scene(H, W, K, seed=SEED):
    """Everything of a case that depends on neither C nor eps: the first of ATTEMPTS draws from ``seed`` on which the conditions of
    ``check_case`` hold (in a single row of 255 pixels a draw can have x advance by nearly a simple fraction of a pixel per pixel, and
    then too many projections lie near a cell line).  What decides is the float64 reference alone."""
    for attempt in range(ATTEMPTS):
        c = _draw(H, W, K, seed + 1009 * attempt)
        try:
            for eps in EPSES:
                check_case(dict(c, eps=eps, C=1, image=c["image"][:, :1], color=c["color"][:, :1]))
                check_case(dict(c, eps=eps))
        except AssertionError:
            continue
        return c
    raise AssertionError("no draw of %dx%d K=%d meets the conditions of check_case" % (H, W, K))


def _draw(H, W, K, seed):
    g = torch.Generator().manual_seed(1000003 * seed + 7919 * H + 31 * W + K)
    px = H * W
    Hd, Wd = size_dst(H, W)
    rnd = lambda *s: torch.rand(*s, generator=g)                                         # noqa: E731
    size = float(max(H, W, 16))
    fx = size * (0.9 + 0.3 * rnd(K))
    pin_i = torch.stack([fx, fx * (1.0 + 0.05 * (2 * rnd(K) - 1)), (W - 1) / 2 + 1.5 * (2 * rnd(K) - 1), (H - 1) / 2 + 1.5 * (2 * rnd(K) - 1)], 1).double()
    u = torch.arange(W, dtype=torch.float32)[None, None, :] / max(W, 32)
    v = torch.arange(H, dtype=torch.float32)[None, :, None] / max(H, 32)
    f, ph0 = 0.5 + 0.75 * rnd(K, 2), 6.2831853 * rnd(K, 2)
    z = 3.0 + 0.5 * torch.sin(6.2831853 * f[:, 0, None, None] * u + ph0[:, 0, None, None]) * torch.cos(6.2831853 * f[:, 1, None, None] * v + ph0[:, 1, None, None])
    z = z.reshape(K, px).contiguous()
    A = 0.56 + 0.42 * rnd(K, px)
    conf = torch.ones(K, px)
    Vi, Vj = torch.zeros(K, 4, 4, dtype=F64), torch.zeros(K, 4, 4, dtype=F64)
    small = px < SMALL
    n_near, n_hole, n_off, n_frac, n_nan = px // 50, (6 * px) // 100, px // 20, (3 * px) // 10, px // 100
    for k in range(K):
        Vi[k], S = CC._view(g)
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
        conf[:] = 0.75
    D = A * z
    has = torch.ones(K, dtype=torch.bool)
    if K >= 2:
        has[1] = False                                       # one pair without target maps
    c = dict(H=H, W=W, K=K, Hd=Hd, Wd=Wd, C=3, eps=EPSES[0], D=D.view(K, 1, H, W), A=A.view(K, 1, H, W), conf=conf.view(K, H, W), Vi=Vi.float(),
             Vj=Vj.float(), pin_i=pin_i, pin_j=torch.tensor((1.0, 1.0, 0.0, 0.0), dtype=F64).repeat(K, 1), has_dst=has, degenerate=(),
             image=torch.zeros(K, 3, Hd, Wd), color=torch.zeros(K, 3, H, W), D_dst=torch.ones(K, 1, Hd, Wd), A_dst=torch.ones(K, 1, Hd, Wd))
    q = _pieces(c)                                           # with the unit pinhole: x = x_j.x / x_j.z, y = x_j.y / x_j.z
    for attempt in range(64):
        offset = (0.137, 0.137) if attempt == 0 else tuple((0.05 + 0.1 * torch.rand(2, generator=g, dtype=F64)).tolist())
        c["pin_j"] = _target_pinholes(q["x"], q["y"], q["reach"], Hd, Wd, small, offset)
        if not small or not guard_mask(c)[0].any():          # a small image keeps every pixel: its projections stay clear of every line
            break
    q = _pieces(c)
    # the target maps: the mean x_j.z of the source pixels that land on a target pixel, occluders, holes
    A_dst = 0.56 + 0.42 * rnd(K, Hd * Wd)
    z_dst = torch.zeros(K, Hd * Wd, dtype=F64)
    for k in range(K):
        m = q["inside"][k]
        at = (torch.floor(q["y"][k][m] + 0.5).long() * Wd + torch.floor(q["x"][k][m] + 0.5).long())
        total = torch.zeros(Hd * Wd, dtype=F64).index_add_(0, at, q["zj"][k][m])
        n = torch.zeros(Hd * Wd, dtype=F64).index_add_(0, at, torch.ones_like(q["zj"][k][m]))
        mean = q["zj"][k][m].mean() if m.any() else torch.tensor(2.0, dtype=F64)
        z_dst[k] = torch.where(n > 0, total / n.clamp_min(1), mean)
        if small:
            continue
        at = torch.randperm(Hd * Wd, generator=g)
        n_occ, n_hole_t = (Hd * Wd) // 20, (Hd * Wd) // 10
        z_dst[k, at[:n_occ]] *= torch.where(rnd(n_occ) < 0.5, 0.75, 1.25).double()
        A_dst[k, at[n_occ:n_occ + n_hole_t]] = 0.1 + 0.3 * rnd(n_hole_t)
    c["A_dst"] = A_dst.view(K, 1, Hd, Wd)
    c["D_dst"] = (A_dst.double() * z_dst).float().view(K, 1, Hd, Wd)
    c["image"] = _texture(g, K, Hd, Wd)
    q = _pieces(c)
    true = q["S"]                                            # the float64 sample where valid, 0 elsewhere
    mag = 10.0 ** (-4.0 + 3.7 * torch.rand(K, 3, H, W, generator=g, dtype=F64))
    sign = torch.where(torch.rand(K, 3, H, W, generator=g) < 0.5, -1.0, 1.0).double()
    color = (true + sign * mag).float()
    if not small:
        for k in range(K):
            color.view(K, 3, px)[k, 0, torch.randperm(px, generator=g)[:n_nan]] = float("nan")           # the first channel: also with C = 1
            c["image"][k, 0, Hd // 2, Wd // 2] = float("nan")
    c["color"] = color
    guard = guard_mask(c)[0]
    c["conf"] = torch.where(guard, torch.zeros_like(c["conf"]), c["conf"])
    c["guarded"] = guard
    c["cot"] = (0.5 + rnd(K)) * torch.where(torch.arange(K) % 2 == 0, 1.0, -1.0)
    return c


@functools.lru_cache(maxsize=None)
def make_case(H, W, K, C, eps):
    c = dict(_scene(H, W, K))
    c["C"], c["eps"] = C, eps
    c["image"], c["color"] = c["image"][:, :C].contiguous(), c["color"][:, :C].contiguous()
    c["figures"] = check_case(c)
    return c


DEGENERATE_PAIRS = {"none_solid": 2, "conf_zero": 5, "outside": 7, "occluded": 9, "singular": 11, "behind": 14}


@functools.lru_cache(maxsize=None)
def degenerate_case(C, eps):
    """The 16-pair case of 17 x 67 with the six pairs of DEGENERATE_PAIRS replaced; the other ten are that case's."""
    base = make_case(17, 67, 16, C, eps)
    c = {k: (v.clone() if torch.is_tensor(v) else v) for k, v in base.items()}
    k = DEGENERATE_PAIRS
    assert bool(c["has_dst"][k["occluded"]])
    c["A"][k["none_solid"]] = 0.125
    c["D"][k["none_solid"]] = 0.125 * 3.0
    c["conf"][k["conf_zero"]] = 0.0
    c["pin_j"][k["outside"], 2] += 10.0 * c["Wd"]            # every projection far to the right of the image
    c["D_dst"][k["occluded"]] = c["A_dst"][k["occluded"]] * 50.0             # a wall far behind everything
    c["Vi"][k["singular"], 1, :3] = 0.0                      # a zero row: det(Ai) is an exact zero however it is evaluated
    c["Vj"][k["behind"], 3, 2] = -10.0
    c["degenerate"] = tuple(k.values())
    q = _pieces(c)
    for i in c["degenerate"]:                                # nothing valid in them, and nothing near a decision that matters
        assert not q["valid"][i].any(), i
    c["figures"] = check_case(c)
    return c


def _lists(c, idx, dtype):
    maps = lambda name: [c[name][i].to(dtype) if bool(c["has_dst"][i]) else None for i in idx]           # noqa: E731
    return ([c["color"][i].to(dtype) for i in idx], [c["image"][i].to(dtype) for i in idx], c["pin_i"][idx], c["pin_j"][idx],
            [c["conf"][i].to(dtype) for i in idx], maps("D_dst"), maps("A_dst"))


def run_torch(c, dtype, pairs=None):
    """(loss (K,), dL/dD (K,1,H,W), dL/dA (K,1,H,W), dL/dVi (K,4,4), dL/dVj (K,4,4)) of warp_loss_torch in ``dtype`` on the host for
    L = sum cot_k loss_k, as float64, and the count (K,)."""
    idx = list(range(c["K"])) if pairs is None else list(pairs)
    leaf = lambda t: t.detach().clone().to(dtype).requires_grad_(True)                   # noqa: E731  (the cached case stays as it is)
    D, A = [leaf(c["D"][i]) for i in idx], [leaf(c["A"][i]) for i in idx]
    Vi, Vj = [leaf(c["Vi"][i]) for i in idx], [leaf(c["Vj"][i]) for i in idx]
    loss, count = warp_loss_torch(D, A, Vi, Vj, *_lists(c, idx, dtype), eps=c["eps"], occlusion=OCCLUSION, min_weight=c.get("min_weight", MIN_WEIGHT),
                                  min_depth=MIN_DEPTH)
    assert loss.dtype == dtype and count.dtype == dtype and not count.requires_grad
    (loss.double() * c["cot"][idx].double()).sum().backward()
    grads = lambda ts: torch.stack([torch.zeros_like(t) if t.grad is None else t.grad for t in ts]).double()      # noqa: E731
    return loss.detach().double(), grads(D), grads(A), grads(Vi), grads(Vj), count.detach().double()


@functools.lru_cache(maxsize=None)
def reference(H, W, K, C, eps):
    return run_torch(make_case(H, W, K, C, eps), F64)


@functools.lru_cache(maxsize=None)
def float32_path(H, W, K, C, eps):
    return run_torch(make_case(H, W, K, C, eps), torch.float32)


def _gproj(c, q, inv_g, absolute=False, swap=False, drop_c=False, l1=False):
    """dL/dproj (K,H,W,2) of the closed form; ``absolute``: the sum of the absolute values of its terms instead."""
    t00, t01, t10, t11 = q["taps"]
    ax, ay = (q["ay"], q["ax"]) if swap else (q["ax"], q["ay"])
    eps, C = c["eps"], c["C"]
    d = torch.sign(q["r"]) if l1 else q["r"] / torch.sqrt(q["r"] * q["r"] + eps * eps)
    if absolute:
        d = d.abs()
        sx = (1 - ay) * (t01.abs() + t00.abs()) + ay * (t11.abs() + t10.abs())
        sy = (1 - ax) * (t10.abs() + t00.abs()) + ax * (t11.abs() + t01.abs())
    else:
        sx = (1 - ay) * (t01 - t00) + ay * (t11 - t10)
        sy = (1 - ax) * (t10 - t00) + ax * (t11 - t01)
    s = _e3(c["cot"].double()) * q["w"] * _e3(inv_g)
    if absolute:
        s = s.abs()
    scale = 1.0 if drop_c else 1.0 / C
    return torch.stack([s * scale * (d * sx).sum(1), s * scale * (d * sy).sum(1)], -1)


def _back(c, q, gr, absolute=False):
    """From dL/dproj to (dL/dD, dL/dA, dL/dVi, dL/dVj); ``absolute``: with the absolute values of every term."""
    K, H, W = q["w"].shape
    a = (lambda t: t.abs()) if absolute else (lambda t: t)
    xj = a(q["xj"])
    gx, gy = gr[..., 0] * a(q["pj"][:, 0, None, None]), gr[..., 1] * a(q["pj"][:, 1, None, None])
    last = (gx * xj[..., 0] + gy * xj[..., 1]) / xj[..., 2] ** 2
    gj = torch.stack([gx / xj[..., 2], gy / xj[..., 2], last if absolute else -last], -1)
    gi = (gj.reshape(K, H * W, 3) @ a(q["M"]).transpose(1, 2)).reshape(K, H, W, 3)
    gz = (a(q["ray"]) * gi).sum(-1)
    gD = gz / q["A"]
    gA = (q["z"] / q["A"]) * gz * (1.0 if absolute else -1.0)
    zero = torch.zeros_like(gz)
    xi = torch.where(q["valid"][..., None], a(q["xi"]), torch.zeros_like(q["xi"]))
    GM = xi.reshape(K, H * W, 3).transpose(1, 2) @ gj.reshape(K, H * W, 3)
    gVi, gVj = CC._chain(q, GM, gj.sum((1, 2)), absolute=absolute)
    return torch.where(q["valid"], gD, zero)[:, None], torch.where(q["valid"], gA, zero)[:, None], gVi, gVj


def closed_form(c, half_pixel=False, swap_ax_ay=False, drop_one_over_c=False, l1_gradient=False):
    """(loss, dL/dD, dL/dA, dL/dVi, dL/dVj) from the closed forms, in float64, the cotangent included.  The switches make the four
    wrong answers the bars must reject: the sample taken at ``proj + 0.5``, ``dS/dproj`` with ``ax`` and ``ay`` exchanged, the ``1/C``
    missing from the gradient, the L1 gradient ``sign(r)`` in place of ``r / sqrt(r^2 + eps^2)``."""
    q = _pieces(c, half_pixel)
    cnt, w = q["cnt"], q["w"]
    inv = torch.where(cnt > 0, 1.0 / cnt.clamp_min(1e-300), torch.zeros_like(cnt))
    eps = c["eps"]
    rho = (torch.sqrt(q["r"] * q["r"] + eps * eps) - eps).sum(1) / c["C"]
    loss = (w * rho).sum((1, 2)) * inv
    gr = _gproj(c, q, inv, swap=swap_ax_ay, drop_c=drop_one_over_c, l1=l1_gradient)
    return (loss,) + _back(c, q, gr)


def scales(c):
    """sum |terms| of the closed forms in float64: (loss (K,), dL/dD (K,1,H,W), dL/dA (K,1,H,W), dL/dVi (K,4,4), dL/dVj (K,4,4))."""
    q = _pieces(c)
    cnt = q["cnt"]
    inv = torch.where(cnt > 0, 1.0 / cnt.clamp_min(1e-300), torch.zeros_like(cnt))
    loss = closed_form(c)[0].abs()                                                        # every term of the loss is non-negative
    return (loss,) + _back(c, q, _gproj(c, q, inv, absolute=True), absolute=True)


def bars_of(c, r64, r32):
    """The five bars from the two runs of the statement and the case's scales."""
    return tuple(FACTOR * (b - a).abs() + FLOOR_EPS * EPS32 * s for a, b, s in zip(r64[:5], r32[:5], scales(c)))


@functools.lru_cache(maxsize=None)
def bars(H, W, K, C, eps):
    return bars_of(make_case(H, W, K, C, eps), reference(H, W, K, C, eps), float32_path(H, W, K, C, eps))


def margins(H, W, K, C, eps, got):
    return margins_of(bars(H, W, K, C, eps), reference(H, W, K, C, eps), got)
