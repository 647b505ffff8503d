"""Antialiased rendering at the bench workload: synth_scene(500 000, seed 0, sm 0.5), SH degree 3, one pinhole camera at 1920x1080.
  a  antialias_opacity         (csrc/antialias.hip): forward, and forward + backward with every gradient wanted
  b  antialias_opacity_torch   the same function in plain PyTorch on the GPU: forward, and forward + backward through autograd
  c  the rasterizer operator, forward + backward under a fixed cotangent, with GaussianRasterizationSettings(antialiasing=False)
     and (antialiasing=True), alternating in the same process on the same device
Median of --repeats after --warmup runs, device events around each run, host work between the launches included.  Prints one JSON
line.  Usage: python tools/bench_antialias.py [--repeats 50] [--warmup 10] [--P 500000] [--only a|b|c]"""
import argparse, json, math, os, statistics, sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "bundle-adjusting-gaussian-splatting_amd"), os.path.join(ROOT, "tests")]
from bags_raster import GaussianRasterizationSettings, GaussianRasterizer, antialias_opacity, antialias_opacity_torch
from bags_raster.synth import look_at_origin_camera, synth_scene
from bags_raster import rasterizer as R
from scenes import camera_tensors


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
    ap.add_argument("--P", type=int, default=500_000); ap.add_argument("--only", default="abc")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_antialias needs the GPU: a time measured anywhere else says nothing")
    dev = torch.device("cuda", 0)
    P, W, H = args.P, 1920, 1080
    scene = synth_scene(P, 0, 0.5, 3, device=dev)
    cam = look_at_origin_camera(W, H)
    ct = camera_tensors(cam, dev)
    tanfov = (math.tan(cam.FoVx * 0.5), math.tan(cam.FoVy * 0.5))
    leaf = lambda t: t.detach().clone().requires_grad_(True)                 # noqa: E731
    lv = {k: leaf(scene[k]) for k in ("means3D", "opacities", "scales", "rotations", "shs")}
    pose = {k: leaf(ct[k]) for k in ("viewmatrix", "projmatrix", "intrinsic", "campos")}
    shift = torch.zeros(3, device=dev, requires_grad=True)
    g_out = torch.randn(P, 1, device=dev, generator=torch.Generator(device=dev).manual_seed(1))
    g_img = torch.randn(3, H, W, device=dev, generator=torch.Generator(device=dev).manual_seed(2))
    everything = list(lv.values()) + list(pose.values()) + [shift]

    def clear():
        for t in everything:
            t.grad = None

    def factor(fn, backward):
        def run():
            if not backward:
                with torch.no_grad():
                    return fn(lv["means3D"], lv["opacities"], pose["viewmatrix"], pose["intrinsic"], (H, W), tanfov, scales=lv["scales"],
                              rotations=lv["rotations"], shift_factors=shift)
            clear()
            fn(lv["means3D"], lv["opacities"], pose["viewmatrix"], pose["intrinsic"], (H, W), tanfov, scales=lv["scales"],
               rotations=lv["rotations"], shift_factors=shift).backward(g_out)
        return run

    def operator(aa):
        st = GaussianRasterizationSettings(image_height=H, image_width=W, tanfovx=tanfov[0], tanfovy=tanfov[1], bg=torch.zeros(3, device=dev),
                                           scale_modifier=1.0, viewmatrix=pose["viewmatrix"], projmatrix=pose["projmatrix"],
                                           intrinsic=pose["intrinsic"], sh_degree=3, campos=pose["campos"], antialiasing=aa)
        rast = GaussianRasterizer(st)
        m2d = torch.zeros(P, 3, device=dev, requires_grad=True)

        def run():
            clear(); m2d.grad = None
            img = rast(means3D=lv["means3D"], means2D=m2d, opacities=lv["opacities"], shift_factors=shift, shs=lv["shs"], scales=lv["scales"],
                       rotations=lv["rotations"])[0]
            img.backward(g_img)
        return run

    res, spread, extra = {}, {}, {}

    def record(key, ms):
        res[key], spread[key] = statistics.median(ms), [min(ms), max(ms)]
    if "a" in args.only:
        record("a_hip_forward", timed(factor(antialias_opacity, False), args.repeats, args.warmup))
        record("a_hip_forward_backward", timed(factor(antialias_opacity, True), args.repeats, args.warmup))
    if "b" in args.only:
        record("b_torch_forward", timed(factor(antialias_opacity_torch, False), args.repeats, args.warmup))
        record("b_torch_forward_backward", timed(factor(antialias_opacity_torch, True), args.repeats, args.warmup))
    if "a" in args.only and "b" in args.only:                                # the two routes on the bench scene, same cotangent
        factor(antialias_opacity, True)()
        ga = [t.grad.clone() for t in everything if t.grad is not None]
        factor(antialias_opacity_torch, True)()
        gb = [t.grad for t in everything if t.grad is not None]
        extra["grad_rel_diff_hip_vs_torch_fp32"] = max(((x - y).double().norm() / y.double().norm().clamp_min(1e-30)).item() for x, y in zip(ga, gb))
    if "c" in args.only:
        off, on = operator(False), operator(True)
        ms = {False: [], True: []}
        for rep in range(args.warmup + args.repeats):                        # off and on alternate: the device's drift hits both alike
            for aa, fn in ((False, off), (True, on)):
                t = timed(fn, 1, 0)[0]
                if rep >= args.warmup:
                    ms[aa].append(t)
                extra["num_rendered_on" if aa else "num_rendered_off"] = int(R.LAST_NUM_RENDERED)
        record("c_operator_antialiasing_off", ms[False]); record("c_operator_antialiasing_on", ms[True])
    line = {"metric": f"ms per call, {P} Gaussians, 1920x1080, median of {args.repeats} after {args.warmup} warm-ups",
            "device": torch.cuda.get_device_name(0), "P": P, "ms": res, "min_max_ms": spread, **extra}
    print(json.dumps(line))


if __name__ == "__main__":
    main()
