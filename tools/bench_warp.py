"""The warping loss at full resolution: views of 1080 x 1920 (a depth and a weights map, a view matrix and a 3-channel image each),
K = 1 (one ordered pair of two views) and K = 20 (the ordered pairs of five views), each pair with a confidence and the target view's
maps for the occlusion test.
  a  warp_loss            (csrc/warp.hip): forward alone (no_grad) and forward + backward through autograd with dL/ddepth,
                          dL/dweights and both view-matrix gradients wanted
  b  warp_loss_torch      the same function in plain PyTorch in float32 on the GPU, the same two measurements
  c  correspondence_loss  (csrc/correspondence.hip) at the same shape and pairs: the neighbour whose pixel work the warping loss shares
                          (matches are reproject_pixels at the true poses plus noise of up to 3 px)
  copy                    a device-to-device copy of 256 MiB, timed the same way: the rate the byte floors below are computed with
The maps are separate tensors, as render_views returns them; a view used in several pairs is passed several times.  The images are
sums of sinusoids with periods of 12 to 40 pixels, the same scene shifted per view, so residuals are small but not zero.  Median of
--repeats after --warmup runs, device events around each run, host work between the launches included; the routes alternate so that
the device's drift hits all alike.  Prints one JSON line.  The bytes a pair must move: the forward reads depth, weights, confidence
(4 B/px each), color_src (12 B/px), the target image (12 B per target pixel, each texel counted once) and the two target maps (8 B):
44 B/px; the backward reads the same and writes 8 B/px.
Usage: python tools/bench_warp.py [--repeats 100] [--warmup 10] [--pairs 1,20] [--only abc] [--eps 1e-3]"""
import argparse, json, os, statistics, sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "bundle-adjusting-gaussian-splatting_amd")]
from bags_raster import correspondence_loss, reproject_pixels, warp_loss, warp_loss_torch
from bags_raster.synth import so3_exp

VIEWS = 5
FWD_BYTES, BWD_BYTES = 44, 52                                # per pixel and pair (module docstring)


def timed(fn):
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    fn()
    e1.record(); torch.cuda.synchronize()
    return e0.elapsed_time(e1)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=100); ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--pairs", default="1,20"); ap.add_argument("--only", default="abc")
    ap.add_argument("--H", type=int, default=1080); ap.add_argument("--W", type=int, default=1920)
    ap.add_argument("--eps", type=float, default=1e-3)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_warp needs the GPU: a time measured anywhere else says nothing")
    dev = torch.device("cuda", 0)
    H, W = args.H, args.W
    gen = torch.Generator(device=dev).manual_seed(0)
    cpu = torch.Generator().manual_seed(0)
    u = torch.arange(W, device=dev)[None, None, :] / W
    v = torch.arange(H, device=dev)[None, :, None] / H
    x = torch.arange(W, device=dev, dtype=torch.float32)[None, None, :]
    y = torch.arange(H, device=dev, dtype=torch.float32)[None, :, None]
    pins = [(1.1 * W + 3.0 * k, 1.08 * W + 2.0 * k, (W - 1) / 2 + 0.7 * k, (H - 1) / 2 - 0.4 * k) for k in range(VIEWS)]
    A = [torch.where(torch.rand(1, H, W, device=dev, generator=gen) < 0.04, 0.2, 0.55 + 0.45 * torch.rand(1, H, W, device=dev, generator=gen))
         .requires_grad_(True) for _ in range(VIEWS)]
    D = [(a.detach() * (3.0 + 0.5 * torch.sin(6.0 * u) * torch.cos(5.0 * v))).requires_grad_(True) for a in A]       # one surface for every view
    ch = torch.arange(3, device=dev, dtype=torch.float32)[:, None, None]
    images = [(0.5 + 0.3 * torch.sin(6.2831853 * (x + 2.0 * k) / (12.0 + 5.0 * ch)) * torch.cos(6.2831853 * (y - 1.5 * k) / (17.0 + 4.0 * ch))
               + 0.15 * torch.sin(6.2831853 * (x + y) / (40.0 - 6.0 * ch))).contiguous() for k in range(VIEWS)]
    views = []
    for k in range(VIEWS):                                   # a similarity with a shear in front of a small rigid motion
        V = torch.eye(4)
        S = 1.3 * torch.eye(3)
        S[0, 1] += 0.05
        V[:3, :3] = S @ so3_exp(0.03 * (2 * torch.rand(3, generator=cpu) - 1))
        V[3, :3] = 0.1 * (2 * torch.rand(3, generator=cpu) - 1)
        views.append(V.to(dev).requires_grad_(True))
    Dc, Ac = [d.detach() for d in D], [a.detach() for a in A]      # the target maps are constant data
    ordered = [(i, j) for i in range(VIEWS) for j in range(VIEWS) if i != j]
    res, spread, extra = {}, {}, {}

    # the copy rate, in this session on this device
    src = torch.empty(256 << 20, dtype=torch.uint8, device=dev)
    dst = torch.empty_like(src)
    ms = [timed(lambda: dst.copy_(src)) for _ in range(args.warmup + args.repeats)][args.warmup:]
    copy_rate = 2 * src.numel() / (statistics.median(ms) * 1e-3)                          # bytes read + written per second
    del src, dst

    for K in [int(t) for t in args.pairs.split(",")]:
        pairs = ordered[:K]
        match, conf = [], []
        for i, j in pairs:
            with torch.no_grad():
                proj, _ = reproject_pixels(D[i], A[i], views[i], views[j], pins[i], pins[j], (H, W))
            ang, mag = 6.2831853 * torch.rand(H, W, device=dev, generator=gen), 3.0 * torch.rand(H, W, device=dev, generator=gen)
            match.append((proj + torch.stack([mag * torch.cos(ang), mag * torch.sin(ang)])).contiguous())
            conf.append(torch.where(torch.rand(H, W, device=dev, generator=gen) < 0.1, 0.0, 0.25 + 0.75 * torch.rand(H, W, device=dev, generator=gen)))
        cot = torch.randn(K, device=dev, generator=gen)
        src_of = lambda ts: [ts[i] for i, _ in pairs]                                    # noqa: E731
        dst_of = lambda ts: [ts[j] for _, j in pairs]                                    # noqa: E731

        def warp(fn):
            return fn(src_of(D), src_of(A), src_of(views), dst_of(views), src_of(images), dst_of(images), src_of(pins), dst_of(pins), conf,
                      dst_of(Dc), dst_of(Ac), eps=args.eps)

        def corr(fn):
            return fn(src_of(D), src_of(A), src_of(views), dst_of(views), match, src_of(pins), dst_of(pins), conf)

        leaves = D + A + views

        def clear():
            for t in leaves:
                t.grad = None

        def fwd(call, fn):
            with torch.no_grad():
                call(fn)

        def fwd_bwd(call, fn):
            clear()
            call(fn)[0].backward(cot)

        routes = [(k, c, f) for k, c, f in (("a_hip", warp, warp_loss), ("b_torch", warp, warp_loss_torch),
                                            ("c_correspondence", corr, correspondence_loss)) if k[0] in args.only]
        for what, run in (("fwd", fwd), ("fwd_bwd", fwd_bwd)):
            ms = {k: [] for k, _, _ in routes}
            for rep in range(args.warmup + args.repeats):
                for k, c, f in routes:
                    t = timed(lambda: run(c, f))
                    if rep >= args.warmup:
                        ms[k].append(t)
            for k, _, _ in routes:
                key = "%s_%s_K%d" % (k, what, K)
                res[key] = statistics.median(ms[k])
                spread[key] = [min(ms[k]), max(ms[k])]
        if "a" in args.only and "b" in args.only:            # the two routes on the same inputs
            fwd_bwd(warp, warp_loss)
            used = [t for t in leaves if t.grad is not None]
            ga = [t.grad.clone() for t in used]
            fwd_bwd(warp, warp_loss_torch)
            extra["grad_rel_diff_hip_vs_torch_fp32_K%d" % K] = max(
                ((g - t.grad).double().norm() / t.grad.double().norm().clamp_min(1e-30)).item() for g, t in zip(ga, used))
        with torch.no_grad():
            loss, count = warp(warp_loss)
            extra["valid_weight_share_K%d" % K] = (count.sum() / (K * H * W)).item()
            extra["mean_loss_K%d" % K] = loss.mean().item()
    px = H * W
    line = {"metric": f"ms per call, {H}x{W}, C = 3, with a confidence and target maps, eps {args.eps}, median of {args.repeats} after "
                      f"{args.warmup} warm-ups; fwd: forward under no_grad, fwd_bwd: forward + backward through autograd",
            "device": torch.cuda.get_device_name(0), "ms": res, "min_max_ms": spread, "copy_rate_TB_per_s": copy_rate / 1e12,
            "floor_us_per_pair": {"forward_%dB_per_px" % FWD_BYTES: FWD_BYTES * px / copy_rate * 1e6,
                                  "backward_%dB_per_px" % BWD_BYTES: BWD_BYTES * px / copy_rate * 1e6},
            **extra}
    print(json.dumps(line))


if __name__ == "__main__":
    main()
