"""Mip-Splatting's 3D smoothing filter at the bench workload: synth_scene(500 000, seed 0, sm 0.5), SH degree 3, and N = 200 cameras
of sphere_views (1920x1080) around it.
  a  filter_3D                    (csrc/filter3d.hip, two launches) against
  b  filter_3D_torch              the same function in plain PyTorch on the GPU
  c  the filtered fused activations (GaussianBag.activated() with a filter set), forward + backward through autograd, against
  d  filtered_activations_torch   the two PyTorch formulas beside the PyTorch properties for features and rotation, and against
  e  the unfiltered fused activations (GaussianBag.activated() with filter_3D None)
c, d and e use all four outputs (features, opacity, scaling, rotation) under fixed cotangents; c and e alternate in one loop.
Median of --repeats after --warmup runs, device events around each run, host work between the launches included.  Prints one JSON
line.  Usage: python tools/bench_filter3d.py [--repeats 50] [--warmup 10] [--P 500000] [--N 200] [--only abcde]"""
import argparse, json, os, statistics, sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "bundle-adjusting-gaussian-splatting_amd"), os.path.join(ROOT, "tests")]
from bags_raster import GaussianBag, filter_3D, filter_3D_torch, filtered_activations_torch
from bags_raster.synth import sphere_views, synth_scene


def timed(fn, repeats, warmup):
    ms = []
    for rep in range(warmup + repeats):
        torch.cuda.synchronize()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record(); torch.cuda.synchronize()
        if rep >= warmup:
            ms.append(e0.elapsed_time(e1))
    return ms


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=50); ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--P", type=int, default=500_000); ap.add_argument("--N", type=int, default=200); ap.add_argument("--only", default="abcde")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_filter3d needs the GPU: a time measured anywhere else says nothing")
    dev = torch.device("cuda", 0)
    P, N, W, H = args.P, args.N, 1920, 1080
    scene = synth_scene(P, 0, 0.5, 3)
    bag = GaussianBag.from_activated(scene, 3, device=dev)
    with torch.no_grad():
        mats = [c.get_matrices(None, None) for c in sphere_views(N, W, H, device=dev)]
        V = torch.stack([m[0] for m in mats]).contiguous()
        K = torch.stack([m[2] for m in mats]).contiguous()
    wh = torch.tensor([[W, H]] * N, dtype=torch.int32, device=dev)
    xyz = bag._xyz.detach()
    res, spread, extra = {}, {}, {}

    def record(key, ms):
        res[key], spread[key] = statistics.median(ms), [min(ms), max(ms)]
    if "a" in args.only:
        record("a_hip_filter_3D", timed(lambda: filter_3D(xyz, V, K, wh), args.repeats, args.warmup))
    if "b" in args.only:
        record("b_torch_filter_3D", timed(lambda: filter_3D_torch(xyz, V, K, wh), max(3, args.repeats // 10), min(args.warmup, 2)))
    f = filter_3D(xyz, V, K, wh)
    if "a" in args.only and "b" in args.only:
        ref = filter_3D_torch(xyz, V, K, wh)
        extra["filter_rows_bitwise_equal_hip_vs_torch_fp32"] = int((f == ref).sum())
        extra["filter_max_rel_diff_hip_vs_torch_fp32"] = ((f - ref).abs() / ref.abs()).max().item()
        extra["filter_min_max"] = [f.min().item(), f.max().item()]
    g = torch.Generator(device=dev).manual_seed(1)
    cots = [torch.randn(s, device=dev, generator=g) for s in ((P, 16, 3), (P, 1), (P, 3), (P, 4))]

    def clear():
        for t in bag.leaves():
            t.grad = None

    def fused(filt):
        def run():
            clear()
            bag.filter_3D = filt
            torch.autograd.backward(list(bag.activated()[1:]), cots)
        return run

    def statement():
        clear()
        op, sc = filtered_activations_torch(bag._opacity, bag._scaling, f)
        torch.autograd.backward([bag.get_features, op, sc, bag.get_rotation], cots)
    on, off = fused(f), fused(None)
    if "c" in args.only or "e" in args.only:
        ms = {True: [], False: []}
        for rep in range(args.warmup + args.repeats):                        # filtered and unfiltered alternate: drift hits both alike
            for flt, fn in ((True, on), (False, off)):
                t = timed(fn, 1, 0)[0]
                if rep >= args.warmup:
                    ms[flt].append(t)
        record("c_hip_filtered_activations_fwd_bwd", ms[True]); record("e_hip_unfiltered_activations_fwd_bwd", ms[False])
    if "d" in args.only:
        record("d_torch_filtered_activations_fwd_bwd", timed(statement, args.repeats, args.warmup))
        on()
        ga = [t.grad.clone() for t in bag.leaves() if t.grad is not None]
        statement()
        gb = [t.grad for t in bag.leaves() if t.grad is not None]
        extra["grad_rel_diff_hip_vs_torch_fp32"] = max(((x - y).double().norm() / y.double().norm().clamp_min(1e-30)).item() for x, y in zip(ga, gb))
    line = {"metric": f"ms per call, {P} Gaussians, {N} cameras, median of {args.repeats} after {args.warmup} warm-ups (b: a tenth of the repeats)",
            "device": torch.cuda.get_device_name(0), "P": P, "N": N, "ms": res, "min_max_ms": spread, **extra}
    print(json.dumps(line))


if __name__ == "__main__":
    main()
