"""The smoothness losses (csrc/smooth.hip) at full size, forward + backward through autograd, against their PyTorch statements in
float32 on the same GPU, at 1080 x 1920 for one view and for five:
  depth1    depth_smooth_loss, inverse depth, normalised, order 1, l1, a 3-channel guide and a mask (Monodepth2's term), dL/ddepth and
            dL/dweights wanted
  depth2    the same at order 2 with eps = 1e-3
  normal    normal_smooth_loss, l2, no guide, no mask (DN-Splatter's TVLoss), dL/dnormal wanted
  copy      a device-to-device copy of 256 MiB, timed the same way: the rate the byte floors below are computed with
Median of --repeats after --warmup runs, device events around each run, host work between the launches included; the routes
alternate so that the device's drift hits all alike.  Prints one JSON line.  The bytes a view must move per pixel: depth with guide
and mask reads D, A, m for the mean (12), D, A, m and the guide for the sums (24) and again for the backward (24), which writes 8;
normals read N, A (16) forward, the same backward and write 12.
  rocprofv3 --kernel-trace --stats --output-format csv -d DIR -- python tools/bench_smooth.py --hip-only --repeats 50 --warmup 5
gives the kernels' own times.
Usage: python tools/bench_smooth.py [--repeats 100] [--warmup 10] [--only depth1,depth2,normal] [--hip-only]"""
import argparse, json, os, statistics, sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "bundle-adjusting-gaussian-splatting_amd")]
from bags_raster import depth_smooth_loss, depth_smooth_loss_torch, normal_smooth_loss, normal_smooth_loss_torch

VIEWS = (1, 5)


def timed(fn):
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    fn()
    e1.record(); torch.cuda.synchronize()
    return e0.elapsed_time(e1)


def alternate(routes, repeats, warmup):
    """{name: (median, min, max)} of the callables of ``routes``, run in turn."""
    ms = {k: [] for k in routes}
    for rep in range(warmup + repeats):
        for k, fn in routes.items():
            t = timed(fn)
            if rep >= warmup:
                ms[k].append(t)
    return {k: (statistics.median(v), min(v), max(v)) for k, v in ms.items()}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=100); ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--only", default="depth1,depth2,normal")
    ap.add_argument("--H", type=int, default=1080); ap.add_argument("--W", type=int, default=1920)
    ap.add_argument("--hip-only", action="store_true", help="leave the PyTorch routes out (for a kernel trace)")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_smooth needs the GPU: a time measured anywhere else says nothing")
    dev = torch.device("cuda", 0)
    only = args.only.split(",")
    H, W = args.H, args.W
    gen = torch.Generator(device=dev).manual_seed(0)
    res, extra = {}, {}

    src = torch.empty(256 << 20, dtype=torch.uint8, device=dev)
    dst = torch.empty_like(src)
    ms = [timed(lambda: dst.copy_(src)) for _ in range(args.warmup + args.repeats)][args.warmup:]
    copy_rate = 2 * src.numel() / (statistics.median(ms) * 1e-3)                          # bytes read + written per second
    del src, dst

    nmax = max(VIEWS)
    rand = lambda *s: torch.rand(*s, device=dev, generator=gen)                           # noqa: E731
    A = [torch.where(rand(1, H, W) < 0.04, 0.2, 0.55 + 0.45 * rand(1, H, W)).requires_grad_(True) for _ in range(nmax)]
    m = [torch.where(rand(H, W) < 0.1, 0.0, 0.25 + 0.75 * rand(H, W)) for _ in range(nmax)]
    guide = [rand(3, H, W) for _ in range(nmax)]

    def measure(tag, hip, ref, fields, call):
        for nv in VIEWS:
            cot = torch.randn(nv, device=dev, generator=gen)

            def fwd_bwd(fn, nv=nv, cot=cot):
                for t in fields + A:
                    t.grad = None
                call(fn, nv)[0].backward(cot)

            fns = {"hip": hip} if args.hip_only else {"hip": hip, "torch": ref}
            for k, st in alternate({k: (lambda f=f: fwd_bwd(f)) for k, f in fns.items()}, args.repeats, args.warmup).items():
                res["%s_%s_fwd_bwd_V%d" % (tag, k, nv)] = {"median": st[0], "min": st[1], "max": st[2]}
            with torch.no_grad():
                loss, count = call(hip, nv)
            extra["%s_valid_weight_share_V%d" % (tag, nv)] = (count.sum() / (2 * nv * H * W)).item()
            if not args.hip_only:
                fwd_bwd(hip)
                ga = [t.grad.clone() for t in fields[:nv]]
                fwd_bwd(ref)
                extra["%s_grad_rel_diff_hip_vs_torch_fp32_V%d" % (tag, nv)] = max(
                    ((a - t.grad).double().norm() / t.grad.double().norm().clamp_min(1e-30)).item() for a, t in zip(ga, fields[:nv]))

    if "depth1" in only or "depth2" in only:
        D = [(a.detach() * (1.0 + 4.0 * rand(1, H, W))).requires_grad_(True) for a in A]
        if "depth1" in only:
            measure("depth1", depth_smooth_loss, depth_smooth_loss_torch, D,
                    lambda fn, nv: fn(D[:nv], A[:nv], guide[:nv], m[:nv], space="inverse", normalize=True, order=1, penalty="l1"))
        if "depth2" in only:
            measure("depth2", depth_smooth_loss, depth_smooth_loss_torch, D,
                    lambda fn, nv: fn(D[:nv], A[:nv], guide[:nv], m[:nv], space="inverse", normalize=True, order=2, penalty="l1", eps=1e-3))
        extra["depth_floor_us_per_view"] = {"fwd": 36 * H * W / copy_rate * 1e6, "bwd": 32 * H * W / copy_rate * 1e6}
        del D
    if "normal" in only:
        d = torch.randn(nmax, 3, H, W, device=dev, generator=gen)
        N = [(d[k] / d[k].norm(dim=0, keepdim=True) * (0.05 + 0.95 * rand(1, H, W))).requires_grad_(True) for k in range(nmax)]
        del d
        measure("normal", normal_smooth_loss, normal_smooth_loss_torch, N, lambda fn, nv: fn(N[:nv], A[:nv], None, None, penalty="l2"))
        extra["normal_floor_us_per_view"] = {"fwd": 16 * H * W / copy_rate * 1e6, "bwd": 28 * H * W / copy_rate * 1e6}

    line = {"metric": f"ms per call, median of {args.repeats} after {args.warmup} warm-ups; fwd_bwd: forward + backward through autograd; "
                      f"{H}x{W}; depth1 / depth2: inverse, normalised, l1, order 1 / 2 (eps 1e-3), 3-channel guide and mask; normal: l2, no guide",
            "device": torch.cuda.get_device_name(0), "ms": res, "copy_rate_TB_per_s": copy_rate / 1e12, **extra}
    print(json.dumps(line))


if __name__ == "__main__":
    main()
