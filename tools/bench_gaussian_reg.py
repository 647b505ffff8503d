"""The regularisers on the Gaussians (csrc/gaussian_reg.hip) at full size, forward + backward through autograd, against their PyTorch
statement (gaussian_reg_loss_torch) in float32 on the same GPU in the same process, at P = 500 k and 2 M rows, with and without a 3D
filter:
  mcmc      the two 3DGS-MCMC terms alone: terms=("opacity", "scale")
  all       all six terms
  copy      a device-to-device copy of 256 MiB, timed the same way: the rate the byte floors below are computed with
Median of --repeats after --warmup runs, device events around each run, host work between the launches included; the routes
alternate so that the device's drift hits all alike.  Prints one JSON line.  The bytes a row must move: the forward reads 16 (x and
three r), plus 4 with a filter; the backward reads the same and writes 16.  (A select mask adds 1 byte per row each way; the bench
runs without one.)
  rocprofv3 --kernel-trace --stats --output-format csv -d DIR -- python tools/bench_gaussian_reg.py --hip-only --repeats 50 --warmup 5
gives the kernels' own times.
Usage: python tools/bench_gaussian_reg.py [--repeats 100] [--warmup 10] [--sizes 500000,2000000] [--only mcmc,all] [--hip-only]"""
import argparse, json, math, os, statistics, sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "bundle-adjusting-gaussian-splatting_amd")]
from bags_raster import REG_TERMS, gaussian_reg_loss, gaussian_reg_loss_torch

SUBSETS = {"mcmc": ("opacity", "scale"), "all": REG_TERMS}


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
    ap.add_argument("--sizes", default="500000,2000000"); ap.add_argument("--only", default="mcmc,all")
    ap.add_argument("--hip-only", action="store_true", help="leave the PyTorch routes out (for a kernel trace)")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_gaussian_reg needs the GPU: a time measured anywhere else says nothing")
    dev = torch.device("cuda", 0)
    gen = torch.Generator(device=dev).manual_seed(0)
    res, extra = {}, {}

    src = torch.empty(256 << 20, dtype=torch.uint8, device=dev)
    dst = torch.empty_like(src)
    ms = [timed(lambda: dst.copy_(src)) for _ in range(args.warmup + args.repeats)][args.warmup:]
    copy_rate = 2 * src.numel() / (statistics.median(ms) * 1e-3)                          # bytes read + written per second
    del src, dst

    lam = torch.tensor([0.01, 0.01, 1.0, 0.1, 1.0, 0.05], device=dev)
    for P in [int(s) for s in args.sizes.split(",")]:
        rand = lambda *s: torch.rand(*s, device=dev, generator=gen)                       # noqa: E731
        # the value ranges of tests/gaussian_reg_cases.py: scales 0.002 .. 0.3, logits in [-8, 8], a filter in [0.001, 0.05]
        r = (math.log(0.009) + 2.0 * rand(P, 1) + torch.randn(P, 3, device=dev, generator=gen).clamp(-1.5, 1.5)).requires_grad_(True)
        x = (16.0 * rand(P, 1) - 8.0).requires_grad_(True)
        filt = torch.exp(math.log(0.001) + 3.9 * rand(P, 1))
        for tag in args.only.split(","):
            for fname, f in (("plain", None), ("filtered", filt)):
                def fwd_bwd(fn, f=f, tag=tag):
                    x.grad = None; r.grad = None
                    (fn(x, r, f, None, SUBSETS[tag])[0] @ lam).backward()

                fns = {"hip": gaussian_reg_loss} if args.hip_only else {"hip": gaussian_reg_loss, "torch": gaussian_reg_loss_torch}
                key = "%s_%s_P%d" % (tag, fname, P)
                for k, st in alternate({k: (lambda fn=fn: fwd_bwd(fn)) for k, fn in fns.items()}, args.repeats, args.warmup).items():
                    res["%s_%s_fwd_bwd" % (key, k)] = {"median": st[0], "min": st[1], "max": st[2]}
                if not args.hip_only:
                    fwd_bwd(gaussian_reg_loss)
                    ga = [x.grad.clone(), r.grad.clone()]
                    fwd_bwd(gaussian_reg_loss_torch)
                    extra["%s_grad_rel_diff_hip_vs_torch_fp32" % key] = max(
                        ((a - t.grad).double().norm() / t.grad.double().norm().clamp_min(1e-30)).item() for a, t in zip(ga, (x, r)))
                    with torch.no_grad():
                        a, b = gaussian_reg_loss(x, r, f, None, SUBSETS[tag])[0], gaussian_reg_loss_torch(x, r, f, None, SUBSETS[tag])[0]
                    extra["%s_terms_max_rel_diff_hip_vs_torch_fp32" % key] = ((a - b).abs() / b.abs().clamp_min(1e-30)).max().item()
        extra["floor_us_P%d" % P] = {"fwd_plain": 16 * P / copy_rate * 1e6, "fwd_filtered": 20 * P / copy_rate * 1e6,
                                     "bwd_plain": 32 * P / copy_rate * 1e6, "bwd_filtered": 36 * P / copy_rate * 1e6}
        del r, x, filt

    line = {"metric": f"ms per call, median of {args.repeats} after {args.warmup} warm-ups; fwd_bwd: forward + backward through autograd of "
                      "terms @ lambdas; mcmc: the opacity and scale terms alone, all: all six; plain / filtered: without / with a 3D filter",
            "device": torch.cuda.get_device_name(0), "ms": res, "copy_rate_TB_per_s": copy_rate / 1e12, **extra}
    print(json.dumps(line))


if __name__ == "__main__":
    main()
