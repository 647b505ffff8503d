"""The depth prior at full resolution: V views of 1080 x 1920 (depth, weights, prior and mask of each), V = 1 and V = 5, both modes.
  a  depth_prior_loss        (csrc/depth_prior.hip): forward alone (no_grad) and forward + backward through autograd with dL/ddepth and
                             dL/dweights (and, for l1, dL/dtable) wanted
  b  depth_prior_loss_torch  the same function in plain PyTorch in float32 on the GPU, the same two measurements
The maps are V separate tensors, as render_views returns them; b stacks them itself.  Median of --repeats after --warmup runs,
device events around each run, host work between the launches included; a and b alternate so that the device's drift hits both
alike.  Prints one JSON line, with the byte model's floor beside it (MI355X_MICROARCH: 6.29 TB/s measured float4 copy rate; the
forward reads 16 B/px with a mask and 12 without, the backward reads the same and writes 8 B/px).
Usage: python tools/bench_depth_prior.py [--repeats 200] [--warmup 20] [--views 1,5] [--modes pearson,l1] [--only a|b|ab] [--no-mask]"""
import argparse, json, os, statistics, sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "bundle-adjusting-gaussian-splatting_amd")]
from bags_raster import depth_prior_loss, depth_prior_loss_torch

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
    ap.add_argument("--views", default="1,5"); ap.add_argument("--modes", default="pearson,l1"); ap.add_argument("--only", default="ab")
    ap.add_argument("--H", type=int, default=1080); ap.add_argument("--W", type=int, default=1920); ap.add_argument("--N", type=int, default=200)
    ap.add_argument("--no-mask", action="store_true")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_depth_prior needs the GPU: a time measured anywhere else says nothing")
    dev = torch.device("cuda", 0)
    H, W, N = args.H, args.W, args.N
    gen = torch.Generator(device=dev).manual_seed(0)
    res, spread, extra = {}, {}, {}
    for mode in args.modes.split(","):
        for V in [int(v) for v in args.views.split(",")]:
            z = [2.0 + 3.0 * torch.rand(1, H, W, device=dev, generator=gen) for _ in range(V)]
            A = [(0.3 + 0.7 * torch.rand(1, H, W, device=dev, generator=gen)).requires_grad_(True) for _ in range(V)]
            D = [(a.detach() * t).requires_grad_(True) for a, t in zip(A, z)]
            prior = [(1.0 / t[0]) * (1.0 + 0.1 * torch.randn(H, W, device=dev, generator=gen)) for t in z]
            mask = None if args.no_mask else [(torch.rand(H, W, device=dev, generator=gen) > 0.1).float() for _ in range(V)]
            cot = torch.randn(V, device=dev, generator=gen)
            kw = dict(mode=mode, space="inverse", min_weight=0.5)
            leaves = D + A
            if mode == "l1":
                table = torch.stack([1.0 + 0.1 * torch.randn(N, device=dev, generator=gen), 0.01 * torch.randn(N, device=dev, generator=gen)], 1)
                table.requires_grad_(True)
                kw.update(table=table, rows=[(37 * v + 11) % N for v in range(V)])
                leaves = leaves + [table]

            def clear():
                for t in leaves:
                    t.grad = None

            def fwd(fn):
                with torch.no_grad():
                    fn(D, A, prior, mask, **kw)

            def fwd_bwd(fn):
                clear()
                fn(D, A, prior, mask, **kw)[0].backward(cot)

            routes = [(k, f) for k, f in (("a_hip", depth_prior_loss), ("b_torch", depth_prior_loss_torch)) if k[0] in args.only]
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
                fwd_bwd(depth_prior_loss)
                ga = [t.grad.clone() for t in leaves]
                fwd_bwd(depth_prior_loss_torch)
                gb = [t.grad for t in leaves]
                extra["grad_rel_diff_hip_vs_torch_fp32_%s_V%d" % (mode, V)] = max(
                    ((x - y).double().norm() / y.double().norm().clamp_min(1e-30)).item() for x, y in zip(ga, gb))
    px = H * W
    rd = 12 if args.no_mask else 16
    line = {"metric": f"ms per call, {H}x{W}, {'no mask' if args.no_mask else 'with a mask'}, median of {args.repeats} after {args.warmup} warm-ups; "
                      "fwd: forward under no_grad, fwd_bwd: forward + backward through autograd",
            "device": torch.cuda.get_device_name(0), "ms": res, "min_max_ms": spread,
            "floor_us_per_view": {"forward_%dB_per_px" % rd: rd * px / COPY_RATE * 1e6, "backward_%dB_per_px" % (rd + 8): (rd + 8) * px / COPY_RATE * 1e6},
            **extra}
    print(json.dumps(line))


if __name__ == "__main__":
    main()
