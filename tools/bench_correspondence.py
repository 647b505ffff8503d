"""The correspondence loss at full resolution: views of 1080 x 1920 (a depth and a weights map and a view matrix each), K = 1 (one
ordered pair of two views) and K = 20 (the ordered pairs of five views), each pair with a (2,H,W) match map and a confidence.
  a  correspondence_loss        (csrc/correspondence.hip): forward alone (no_grad) and forward + backward through autograd with
                                dL/ddepth, dL/dweights and both view-matrix gradients wanted
  b  correspondence_loss_torch  the same function in plain PyTorch in float32 on the GPU, the same two measurements
The maps are separate tensors, as render_views returns them; a source view used in several pairs is passed several times.  The
matches are reproject_pixels at the true poses plus noise of up to 3 px, so both Huber branches are taken.  Median of --repeats after
--warmup runs, device events around each run, host work between the launches included; a and b alternate so that the device's drift
hits both alike.  Prints one JSON line, with the byte model's floor beside it (MI355X_MICROARCH: 6.29 TB/s measured float4 copy
rate; the forward reads 20 B/px -- depth, weights, two match components, the confidence -- the backward reads the same and writes
8 B/px).
Usage: python tools/bench_correspondence.py [--repeats 100] [--warmup 10] [--pairs 1,20] [--only a|b|ab] [--delta 1.0]"""
import argparse, json, os, statistics, sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "bundle-adjusting-gaussian-splatting_amd")]
from bags_raster import correspondence_loss, correspondence_loss_torch, reproject_pixels
from bags_raster.synth import so3_exp

COPY_RATE = 6.29e12                                          # bytes per second, measured float4 copy on the MI355X
VIEWS = 5


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
    ap.add_argument("--pairs", default="1,20"); ap.add_argument("--only", default="ab")
    ap.add_argument("--H", type=int, default=1080); ap.add_argument("--W", type=int, default=1920)
    ap.add_argument("--delta", type=float, default=1.0)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_correspondence needs the GPU: a time measured anywhere else says nothing")
    dev = torch.device("cuda", 0)
    H, W = args.H, args.W
    gen = torch.Generator(device=dev).manual_seed(0)
    cpu = torch.Generator().manual_seed(0)
    u = torch.arange(W, device=dev)[None, None, :] / W
    v = torch.arange(H, device=dev)[None, :, None] / H
    pins = [(1.1 * W + 3.0 * k, 1.08 * W + 2.0 * k, (W - 1) / 2 + 0.7 * k, (H - 1) / 2 - 0.4 * k) for k in range(VIEWS)]
    A = [torch.where(torch.rand(1, H, W, device=dev, generator=gen) < 0.04, 0.2, 0.55 + 0.45 * torch.rand(1, H, W, device=dev, generator=gen))
         .requires_grad_(True) for _ in range(VIEWS)]
    D = [(a.detach() * (3.0 + 0.5 * torch.sin(6.0 * u + k) * torch.cos(5.0 * v))).requires_grad_(True) for k, a in enumerate(A)]
    views = []
    for k in range(VIEWS):                                   # a similarity with a shear in front of a small rigid motion
        V = torch.eye(4)
        S = 1.3 * torch.eye(3)
        S[0, 1] += 0.05
        V[:3, :3] = S @ so3_exp(0.03 * (2 * torch.rand(3, generator=cpu) - 1))
        V[3, :3] = 0.1 * (2 * torch.rand(3, generator=cpu) - 1)
        views.append(V.to(dev).requires_grad_(True))
    ordered = [(i, j) for i in range(VIEWS) for j in range(VIEWS) if i != j]
    res, spread, extra = {}, {}, {}
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
        call = lambda fn: fn([D[i] for i, _ in pairs], [A[i] for i, _ in pairs], [views[i] for i, _ in pairs], [views[j] for _, j in pairs], match,  # noqa: E731
                             [pins[i] for i, _ in pairs], [pins[j] for _, j in pairs], conf, delta=args.delta)
        leaves = D + A + views

        def clear():
            for t in leaves:
                t.grad = None

        def fwd(fn):
            with torch.no_grad():
                call(fn)

        def fwd_bwd(fn):
            clear()
            call(fn)[0].backward(cot)

        routes = [(k, f) for k, f in (("a_hip", correspondence_loss), ("b_torch", correspondence_loss_torch)) if k[0] in args.only]
        for what, run in (("fwd", fwd), ("fwd_bwd", fwd_bwd)):
            ms = {k: [] for k, _ in routes}
            for rep in range(args.warmup + args.repeats):
                for k, f in routes:
                    t = timed(lambda: run(f))
                    if rep >= args.warmup:
                        ms[k].append(t)
            for k, _ in routes:
                key = "%s_%s_K%d" % (k, what, K)
                res[key] = statistics.median(ms[k])
                spread[key] = [min(ms[k]), max(ms[k])]
        if len(routes) == 2:                                 # the two routes on the same inputs
            fwd_bwd(correspondence_loss)
            used = [t for t in leaves if t.grad is not None]
            ga = [t.grad.clone() for t in used]
            fwd_bwd(correspondence_loss_torch)
            extra["grad_rel_diff_hip_vs_torch_fp32_K%d" % K] = max(
                ((x - t.grad).double().norm() / t.grad.double().norm().clamp_min(1e-30)).item() for x, t in zip(ga, used))
        with torch.no_grad():
            loss, count = call(correspondence_loss)
            extra["valid_weight_share_K%d" % K] = (count.sum() / (K * H * W)).item()
            extra["mean_loss_K%d" % K] = loss.mean().item()
    px = H * W
    line = {"metric": f"ms per call, {H}x{W}, with a confidence, delta {args.delta}, median of {args.repeats} after {args.warmup} warm-ups; "
                      f"fwd: forward under no_grad, fwd_bwd: forward + backward through autograd",
            "device": torch.cuda.get_device_name(0), "ms": res, "min_max_ms": spread,
            "floor_us_per_pair": {"forward_20B_per_px": 20 * px / COPY_RATE * 1e6, "backward_28B_per_px": 28 * px / COPY_RATE * 1e6},
            **extra}
    print(json.dumps(line))


if __name__ == "__main__":
    main()
