"""The appearance step at full resolution: V images of 1080 x 1920 through V rows of an N = 200 table, V = 1 and V = 5.
  a  apply_appearance   (csrc/appearance.hip): forward + backward through autograd, dL/dimage and dL/dtable wanted
  b  appearance_torch   the same function in plain PyTorch on the GPU: forward + backward through autograd
The images are V separate tensors, as render_views returns them; b stacks them itself.  Median of --repeats after --warmup runs,
device events around each run, host work between the launches included; a and b alternate so that the device's drift hits both
alike.  Prints one JSON line, with the byte model's floor beside it (MI355X_MICROARCH: 6.29 TB/s measured float4 copy rate;
24 B/px forward, 36 B/px backward per view).
Usage: python tools/bench_appearance.py [--repeats 200] [--warmup 20] [--views 1,5] [--only a|b|ab]"""
import argparse, json, os, statistics, sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "bundle-adjusting-gaussian-splatting_amd")]
from bags_raster import apply_appearance, appearance_torch

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
    ap.add_argument("--views", default="1,5"); ap.add_argument("--only", default="ab")
    ap.add_argument("--H", type=int, default=1080); ap.add_argument("--W", type=int, default=1920); ap.add_argument("--N", type=int, default=200)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_appearance needs the GPU: a time measured anywhere else says nothing")
    dev = torch.device("cuda", 0)
    H, W, N = args.H, args.W, args.N
    gen = torch.Generator(device=dev).manual_seed(0)
    res, spread, extra = {}, {}, {}
    for V in [int(v) for v in args.views.split(",")]:
        images = [torch.rand(3, H, W, device=dev, generator=gen).requires_grad_(True) for _ in range(V)]
        cots = [torch.randn(3, H, W, device=dev, generator=gen) for _ in range(V)]
        table = torch.eye(3, 4, device=dev).reshape(12).repeat(N, 1)
        table = torch.cat([table + 0.1 * torch.randn(N, 12, device=dev, generator=gen), 0.2 * torch.randn(N, 3, device=dev, generator=gen),
                           torch.zeros(N, 1, device=dev)], 1).requires_grad_(True)
        rows = [(37 * v + 11) % N for v in range(V)]

        def clear():
            table.grad = None
            for t in images:
                t.grad = None

        def hip():
            clear()
            torch.autograd.backward(apply_appearance(images, table, rows), cots)

        def torch_path():
            clear()
            torch.autograd.backward(appearance_torch(images, table[rows]), cots)

        routes = [(k, f) for k, f in (("a_hip", hip), ("b_torch", torch_path)) if k[0] in args.only]
        ms = {k: [] for k, _ in routes}
        for rep in range(args.warmup + args.repeats):
            for k, f in routes:
                t = timed(f)
                if rep >= args.warmup:
                    ms[k].append(t)
        for k, _ in routes:
            res["%s_V%d" % (k, V)] = statistics.median(ms[k])
            spread["%s_V%d" % (k, V)] = [min(ms[k]), max(ms[k])]
        if len(routes) == 2:                                 # the two routes on the same inputs
            hip()
            ga = [t.grad.clone() for t in images] + [table.grad.clone()]
            torch_path()
            gb = [t.grad for t in images] + [table.grad]
            extra["grad_rel_diff_hip_vs_torch_fp32_V%d" % V] = max(((x - y).double().norm() / y.double().norm().clamp_min(1e-30)).item()
                                                                  for x, y in zip(ga, gb))
    px = H * W
    line = {"metric": f"ms per forward + backward through autograd, {H}x{W}, N = {N}, median of {args.repeats} after {args.warmup} warm-ups",
            "device": torch.cuda.get_device_name(0), "ms": res, "min_max_ms": spread,
            "floor_us_per_view": {"forward_24B_per_px": 24 * px / COPY_RATE * 1e6, "backward_36B_per_px": 36 * px / COPY_RATE * 1e6}, **extra}
    print(json.dumps(line))


if __name__ == "__main__":
    main()
