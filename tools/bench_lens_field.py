"""The lens network of one training iteration: forward + backward of the invertible ResNet (B = 5, H = 64, n = 1, the LensField
defaults) on a control grid, with the gradient of the points off as in the reference's use (the control points are constants).
Grids: 68x120 and 135x240, that is 1080p at 1/16 and 1/8 (the reference's own grid size is not known).  Legs, both float32, both in
this process on the same device:
  fused  lens_field (csrc/lens_field.hip: one launch forward, two backward)
  torch  lens_field_torch (the nn.Linear / nn.ELU calls on views of the same flat parameter) + autograd
Each leg: warm-up, then --steps steps between two device events, median of --repeats: wall per step.  Prints one JSON line.

Kernel sum and launch count come from a kernel trace, taken in a run of its own (tracing slows the host):
  rocprofv3 --kernel-trace --stats --output-format csv -d DIR -- python tools/bench_lens_field.py --only fused --grid 68x120 --repeats 1
  python tools/bench_lens_field.py --summarize DIR --traced-steps <warmup + steps, as the traced run printed them>
which prints, per traced step, the number of kernel launches and the sum of their durations.
Usage: python tools/bench_lens_field.py [--steps 200] [--repeats 5] [--only fused] [--grid 68x120]"""
import argparse, csv, glob, json, os, statistics, sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "bundle-adjusting-gaussian-splatting_amd")]
from bags_raster import LensField, lens_field, lens_field_torch

GRIDS = ((68, 120), (135, 240))


def summarize(directory, traced_steps):
    """Per step of a traced run: launches and kernel time, from rocprofv3's *kernel_stats.csv (Name, Calls, TotalDurationNs, ...)."""
    files = sorted(glob.glob(os.path.join(directory, "**", "*kernel_stats.csv"), recursive=True))
    if not files:
        raise SystemExit(f"no *kernel_stats.csv under {directory}")
    rows = [r for r in csv.DictReader(open(files[0])) if int(r["Calls"]) >= traced_steps]       # set-up kernels run once, not per step
    calls = sum(int(r["Calls"]) for r in rows)
    total_ns = sum(float(r["TotalDurationNs"]) for r in rows)
    line = {"metric": "per traced step: kernel launches and sum of kernel durations (rocprofv3 --kernel-trace --stats)", "traced_steps": traced_steps,
            "launches_per_step": calls / traced_steps, "kernel_sum_us_per_step": total_ns / 1e3 / traced_steps,
            "kernels": {r["Name"][:60]: [int(r["Calls"]), float(r["AverageNs"]) / 1e3] for r in rows}}
    print(json.dumps(line))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=200); ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--only", default="", help="fused or torch (for kernel traces)")
    ap.add_argument("--grid", default="", help="one grid, e.g. 68x120 (default: both)")
    ap.add_argument("--summarize", default="", help="directory of a rocprofv3 --kernel-trace --stats run of this tool")
    ap.add_argument("--traced-steps", type=int, default=0)
    args = ap.parse_args()
    if args.summarize:
        return summarize(args.summarize, args.traced_steps)
    if not torch.cuda.is_available():
        raise SystemExit("bench_lens_field needs the GPU: a time measured anywhere else says nothing")
    dev = torch.device("cuda", 0)
    net = LensField(seed=0)                        # set up on the host: a kernel trace of this tool then holds the timed steps' launches only
    net.lipschitz_correction(iterations=10, generator=torch.Generator().manual_seed(1))
    net = net.to(dev)
    dims = net.dims
    grids = [tuple(int(v) for v in args.grid.split("x"))] if args.grid else list(GRIDS)

    def timed(fn):
        for _ in range(args.warmup):
            fn()
        torch.cuda.synchronize()
        ms = []
        for _ in range(args.repeats):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(args.steps):
                fn()
            e1.record(); torch.cuda.synchronize()
            ms.append(e0.elapsed_time(e1) / args.steps)
        return statistics.median(ms), min(ms), max(ms)

    res, spread, check = {}, {}, {}
    for h, w in grids:
        gy, gx = torch.meshgrid(torch.linspace(-1, 1, h), torch.linspace(-1, 1, w), indexing="ij")
        ctrl = torch.stack((gx, gy), 2).to(dev)
        cot = torch.randn(h, w, 2, generator=torch.Generator().manual_seed(2)).to(dev)

        def step(fn):
            def run():
                net.params.grad = None
                fn(net.params, ctrl, *dims).backward(cot)
            return run
        legs = {"fused": step(lens_field), "torch": step(lens_field_torch)}
        grads = {}
        for name, fn in legs.items():
            if args.only and name != args.only:
                continue
            key = f"{name}_{h}x{w}"
            med, lo, hi = timed(fn)
            res[key], spread[key] = med, [lo, hi]
            grads[name] = net.params.grad.detach().clone()
        if len(grads) == 2:            # faster and different is not faster: the two legs' gradients on this grid
            check[f"{h}x{w}"] = float((grads["fused"] - grads["torch"]).norm() / grads["torch"].norm())
    line = {"metric": f"ms per forward + backward of the lens net (blocks, hidden, internal_layers) = {dims}, grad_x off, float32, "
                      f"median of {args.repeats} x {args.steps} steps", "device": torch.cuda.get_device_name(0), "ms": res, "min_max_ms": spread,
            "grad_params_rel_l2_fused_vs_torch": check, "steps_per_leg_and_grid": args.warmup + args.repeats * args.steps}
    print(json.dumps(line))


if __name__ == "__main__":
    main()
