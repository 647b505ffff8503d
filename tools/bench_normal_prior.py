"""The normal prior at full resolution: V views of 1080 x 1920 (depth, weights, a (3,H,W) prior and a mask of each), V = 1 and V = 5,
both modes.
  a  normal_prior_loss        (csrc/normal_prior.hip): forward alone (no_grad) and forward + backward through autograd with dL/ddepth
                              and dL/dweights wanted
  b  normal_prior_loss_torch  the same function in plain PyTorch in float32 on the GPU, the same two measurements
The maps are V separate tensors, as render_views returns them; b stacks them itself.  Median of --repeats after --warmup runs,
device events around each run, host work between the launches included; a and b alternate so that the device's drift hits both
alike.  Prints one JSON line, with the byte model's floor beside it (MI355X_MICROARCH: 6.29 TB/s measured float4 copy rate; the
forward reads 24 B/px with a mask and 20 without, the backward reads the same and writes 8 B/px; halo re-reads not counted).
Usage: python tools/bench_normal_prior.py [--repeats 200] [--warmup 20] [--views 1,5] [--modes cos,l1] [--only a|b|ab] [--no-mask]
                                          [--max-jump 0.25]"""
import argparse, json, os, statistics, sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "bundle-adjusting-gaussian-splatting_amd")]
from bags_raster import normal_prior_loss, normal_prior_loss_torch

COPY_RATE = 6.29e12                                          # bytes per second, measured float4 copy on the MI355X


def timed(fn):
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    fn()
    e1.record(); torch.cuda.synchronize()
    return e0.elapsed_time(e1)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=200); ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--views", default="1,5"); ap.add_argument("--modes", default="cos,l1"); ap.add_argument("--only", default="ab")
    ap.add_argument("--H", type=int, default=1080); ap.add_argument("--W", type=int, default=1920)
    ap.add_argument("--max-jump", type=float, default=0.25); ap.add_argument("--no-mask", action="store_true")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_normal_prior needs the GPU: a time measured anywhere else says nothing")
    dev = torch.device("cuda", 0)
    H, W = args.H, args.W
    gen = torch.Generator(device=dev).manual_seed(0)
    u = torch.arange(W, device=dev)[None, None, :] / W
    v = torch.arange(H, device=dev)[None, :, None] / H
    res, spread, extra = {}, {}, {}
    for mode in args.modes.split(","):
        for V in [int(t) for t in args.views.split(",")]:
            pins = [(1.1 * W + 3.0 * k, 1.08 * W + 2.0 * k, (W - 1) / 2 + 0.7, (H - 1) / 2 - 0.4) for k in range(V)]
            z = [3.0 + 0.5 * torch.sin(6.0 * u + k) * torch.cos(5.0 * v) + 0.3 * 3.0 / pins[k][0] * torch.randn(1, H, W, device=dev, generator=gen)
                 for k in range(V)]
            A = [torch.where(torch.rand(1, H, W, device=dev, generator=gen) < 0.04, 0.2, 0.55 + 0.45 * torch.rand(1, H, W, device=dev, generator=gen))
                 .requires_grad_(True) for _ in range(V)]
            D = [(a.detach() * t).requires_grad_(True) for a, t in zip(A, z)]
            prior = []
            for _ in range(V):
                p = torch.cat([0.3 * torch.randn(2, H, W, device=dev, generator=gen), -torch.ones(1, H, W, device=dev)], 0)
                prior.append((p / p.norm(dim=0, keepdim=True)).contiguous())
            mask = None if args.no_mask else [(torch.rand(H, W, device=dev, generator=gen) > 0.1).float() for _ in range(V)]
            cot = torch.randn(V, device=dev, generator=gen)
            kw = dict(mode=mode, min_weight=0.5, max_jump=args.max_jump)
            leaves = D + A

            def clear():
                for t in leaves:
                    t.grad = None

            def fwd(fn):
                with torch.no_grad():
                    fn(D, A, prior, pins, mask, **kw)

            def fwd_bwd(fn):
                clear()
                fn(D, A, prior, pins, mask, **kw)[0].backward(cot)

            routes = [(k, f) for k, f in (("a_hip", normal_prior_loss), ("b_torch", normal_prior_loss_torch)) if k[0] in args.only]
            for what, run in (("fwd", fwd), ("fwd_bwd", fwd_bwd)):
                ms = {k: [] for k, _ in routes}
                for rep in range(args.warmup + args.repeats):
                    for k, f in routes:
                        t = timed(lambda: run(f))
                        if rep >= args.warmup:
                            ms[k].append(t)
                for k, _ in routes:
                    key = "%s_%s_%s_V%d" % (k, mode, what, V)
                    res[key] = statistics.median(ms[k])
                    spread[key] = [min(ms[k]), max(ms[k])]
            if len(routes) == 2:                             # the two routes on the same inputs
                fwd_bwd(normal_prior_loss)
                ga = [t.grad.clone() for t in leaves]
                fwd_bwd(normal_prior_loss_torch)
                gb = [t.grad for t in leaves]
                extra["grad_rel_diff_hip_vs_torch_fp32_%s_V%d" % (mode, V)] = max(
                    ((x - y).double().norm() / y.double().norm().clamp_min(1e-30)).item() for x, y in zip(ga, gb))
                with torch.no_grad():
                    extra["valid_weight_share_%s_V%d" % (mode, V)] = (normal_prior_loss(D, A, prior, pins, mask, **kw)[1].sum() / (V * H * W)).item()
    px = H * W
    rd = 20 if args.no_mask else 24
    line = {"metric": f"ms per call, {H}x{W}, {'no mask' if args.no_mask else 'with a mask'}, max_jump {args.max_jump}, median of {args.repeats} "
                      f"after {args.warmup} warm-ups; fwd: forward under no_grad, fwd_bwd: forward + backward through autograd",
            "device": torch.cuda.get_device_name(0), "ms": res, "min_max_ms": spread,
            "floor_us_per_view": {"forward_%dB_per_px" % rd: rd * px / COPY_RATE * 1e6, "backward_%dB_per_px" % (rd + 8): (rd + 8) * px / COPY_RATE * 1e6},
            **extra}
    print(json.dumps(line))


if __name__ == "__main__":
    main()
