"""alpha_loss (csrc/alpha.hip) at full size, forward + backward through autograd, against its PyTorch statement (alpha_loss_torch) in
float32 on the same GPU in the same process: 1080 x 1920 maps with a target (none in the entropy mode) and a mask, 1 and 5 views,
every mode.
  copy      a device-to-device copy of 256 MiB, timed the same way: the rate the byte floors below are computed with
Median of --repeats after --warmup runs, device events around each run, host work between the launches included; the routes
alternate so that the device's drift hits all alike.  Prints one JSON line.  The bytes a pixel must move: the forward reads 4 each
for the weights, the target (not in the entropy mode) and the mask; the backward reads the same and writes 4.
  rocprofv3 --kernel-trace --stats --output-format csv -d DIR -- python tools/bench_alpha.py --hip-only --repeats 50 --warmup 5
gives the kernels' own times.
Usage: python tools/bench_alpha.py [--repeats 100] [--warmup 10] [--views 1,5] [--modes bce,l1,l2,entropy] [--size 1080x1920] [--hip-only]"""
import argparse, json, os, statistics, sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "bundle-adjusting-gaussian-splatting_amd")]
from bags_raster import _lib, alpha_loss, alpha_loss_torch


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
    ap.add_argument("--views", default="1,5"); ap.add_argument("--modes", default="bce,l1,l2,entropy"); ap.add_argument("--size", default="1080x1920")
    ap.add_argument("--hip-only", action="store_true", help="leave the PyTorch route out (for a kernel trace)")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_alpha needs the GPU: a time measured anywhere else says nothing")
    dev = torch.device("cuda", 0)
    gen = torch.Generator(device=dev).manual_seed(0)
    H, W = (int(s) for s in args.size.split("x"))
    res, extra = {}, {}

    src = torch.empty(256 << 20, dtype=torch.uint8, device=dev)
    dst = torch.empty_like(src)
    ms = [timed(lambda: dst.copy_(src)) for _ in range(args.warmup + args.repeats)][args.warmup:]
    copy_rate = 2 * src.numel() / (statistics.median(ms) * 1e-3)                          # bytes read + written per second
    del src, dst

    for V in [int(s) for s in args.views.split(",")]:
        rand = lambda *s: torch.rand(*s, device=dev, generator=gen)                       # noqa: E731
        # a rendered silhouette: two fifths of the pixels empty, two fifths solid, the rest partly covered; the target a soft mask
        As = [torch.clamp(2.5 * rand(1, H, W) - 0.75, 0.0, 1.0).requires_grad_(True) for _ in range(V)]
        ts = [torch.clamp(2.5 * rand(H, W) - 0.75, 0.0, 1.0) for _ in range(V)]
        ms_ = [0.2 + 0.8 * rand(H, W) for _ in range(V)]
        cot = 1.0 + rand(V)
        for mode in args.modes.split(","):
            target = None if mode == "entropy" else ts

            def fwd_bwd(fn, mode=mode, target=target):
                for a in As:
                    a.grad = None
                (fn(As, target, ms_, mode=mode)[0] @ cot).backward()

            fns = {"hip": alpha_loss} if args.hip_only else {"hip": alpha_loss, "torch": alpha_loss_torch}
            key = "%s_V%d" % (mode, V)
            for k, st in alternate({k: (lambda fn=fn: fwd_bwd(fn)) for k, fn in fns.items()}, args.repeats, args.warmup).items():
                res["%s_%s_fwd_bwd" % (key, k)] = {"median": st[0], "min": st[1], "max": st[2]}
            if not args.hip_only:
                fwd_bwd(alpha_loss)
                ga = [a.grad.clone() for a in As]
                fwd_bwd(alpha_loss_torch)
                extra["%s_grad_rel_diff_hip_vs_torch_fp32" % key] = max(
                    ((g - a.grad).double().norm() / a.grad.double().norm().clamp_min(1e-30)).item() for g, a in zip(ga, As))
                with torch.no_grad():
                    a, b = alpha_loss(As, target, ms_, mode=mode)[0], alpha_loss_torch(As, target, ms_, mode=mode)[0]
                extra["%s_loss_max_rel_diff_hip_vs_torch_fp32" % key] = ((a - b).abs() / b.abs().clamp_min(1e-30)).max().item()
            maps = 2 if mode == "entropy" else 3
            extra["floor_us_%s" % key] = {"fwd": 4 * maps * H * W * V / copy_rate * 1e6, "bwd": 4 * (maps + 1) * H * W * V / copy_rate * 1e6}
        del As, ts, ms_

    line = {"metric": f"ms per call, median of {args.repeats} after {args.warmup} warm-ups; fwd_bwd: forward + backward through autograd of "
                      f"loss @ cotangents at {H}x{W} with a mask; V: views of the call",
            "device": torch.cuda.get_device_name(0), "groups": _lib.ALPHA_GROUPS, "ms": res, "copy_rate_TB_per_s": copy_rate / 1e12, **extra}
    print(json.dumps(line))


if __name__ == "__main__":
    main()
