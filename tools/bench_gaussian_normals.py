"""The rendered-normals half of the library at full size.
  normals   gaussian_normals_views (csrc/gaussian_normals.hip) at --P Gaussians for V = 1 and V = 5 view matrices: forward alone
            (no_grad) and forward + backward through autograd with dL/drotations and every view-matrix gradient wanted, against
            gaussian_normals_views_torch in float32 on the same GPU
  loss      normal_map_loss (csrc/normal_map.hip) at 1080 x 1920 for one view and for five, with a mask: forward + backward with
            dL/dnormal wanted, against normal_map_loss_torch in float32 on the same GPU
  render    one render_normals call forward + backward (a sum of the map) beside one render() call forward + backward on bench.py's
            scene: the price of the second pass
  copy      a device-to-device copy of 256 MiB, timed the same way: the rate the byte floors below are computed with
Median of --repeats after --warmup runs, device events around each run, host work between the launches included; the routes
alternate so that the device's drift hits all alike.  Prints one JSON line.  The bytes gaussian_normals must move per Gaussian: the
forward reads 40 (q, s, x) and writes 12 V; the backward reads 40 + 12 V and writes 16.
  rocprofv3 --kernel-trace --stats --output-format csv -d DIR -- python tools/bench_gaussian_normals.py --only normals,loss --hip-only --repeats 50 --warmup 5
gives the kernels' own times.
Usage: python tools/bench_gaussian_normals.py [--repeats 100] [--warmup 10] [--P 500000] [--only normals,loss,render] [--hip-only]"""
import argparse, json, os, statistics, sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "bundle-adjusting-gaussian-splatting_amd")]
from bags_raster import (PipelineParams, gaussian_normals_views, gaussian_normals_views_torch, normal_map_loss, normal_map_loss_torch, render,
                         render_normals)
from bags_raster.gaussians import GaussianBag
from bags_raster.synth import look_at_origin_camera, so3_exp, synth_scene

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
    ap.add_argument("--P", type=int, default=500_000); ap.add_argument("--only", default="normals,loss,render")
    ap.add_argument("--H", type=int, default=1080); ap.add_argument("--W", type=int, default=1920)
    ap.add_argument("--hip-only", action="store_true", help="leave the PyTorch routes out (for a kernel trace)")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_gaussian_normals needs the GPU: a time measured anywhere else says nothing")
    dev = torch.device("cuda", 0)
    only = args.only.split(",")
    P, H, W = args.P, args.H, args.W
    gen = torch.Generator(device=dev).manual_seed(0)
    cpu = torch.Generator().manual_seed(0)
    res, extra = {}, {}

    def put(key, stats):
        res[key] = {"median": stats[0], "min": stats[1], "max": stats[2]}

    src = torch.empty(256 << 20, dtype=torch.uint8, device=dev)
    dst = torch.empty_like(src)
    ms = [timed(lambda: dst.copy_(src)) for _ in range(args.warmup + args.repeats)][args.warmup:]
    copy_rate = 2 * src.numel() / (statistics.median(ms) * 1e-3)                          # bytes read + written per second
    del src, dst

    if "normals" in only:
        q = torch.randn(P, 4, device=dev, generator=gen).requires_grad_(True)
        s = torch.randn(P, 3, device=dev, generator=gen)                                  # log-scales
        x = 2.6 * torch.rand(P, 3, device=dev, generator=gen) - 1.3
        views = []
        for k in range(max(VIEWS)):
            V = torch.eye(4)
            V[:3, :3] = so3_exp(0.5 * (2 * torch.rand(3, generator=cpu) - 1))
            V[3, :3] = torch.tensor([0.0, 0.0, 4.0]) + 0.2 * (2 * torch.rand(3, generator=cpu) - 1)
            views.append(V.to(dev).requires_grad_(True))
        cots = [torch.randn(P, 3, device=dev, generator=gen) for _ in range(max(VIEWS))]
        for nv in VIEWS:
            def fwd(fn, nv=nv):
                with torch.no_grad():
                    fn(q, s, x, views[:nv])

            def fwd_bwd(fn, nv=nv):
                q.grad = None
                for v in views:
                    v.grad = None
                torch.autograd.backward(list(fn(q, s, x, views[:nv])), cots[:nv])

            fns = {"hip": gaussian_normals_views} if args.hip_only else {"hip": gaussian_normals_views, "torch": gaussian_normals_views_torch}
            for what, run in (("fwd", fwd), ("fwd_bwd", fwd_bwd)):
                for k, st in alternate({k: (lambda f=f: run(f)) for k, f in fns.items()}, args.repeats, args.warmup).items():
                    put("normals_%s_%s_V%d" % (k, what, nv), st)
            if not args.hip_only:
                fwd_bwd(gaussian_normals_views)
                ga = [q.grad.clone()] + [v.grad.clone() for v in views[:nv]]
                fwd_bwd(gaussian_normals_views_torch)
                gb = [q.grad] + [v.grad for v in views[:nv]]
                extra["normals_grad_rel_diff_hip_vs_torch_fp32_V%d" % nv] = max(
                    ((a - b).double().norm() / b.double().norm().clamp_min(1e-30)).item() for a, b in zip(ga, gb))
        extra["normals_floor_us"] = {"fwd_V%d" % nv: (40 + 12 * nv) * P / copy_rate * 1e6 for nv in VIEWS}
        extra["normals_floor_us"].update({"bwd_V%d" % nv: (56 + 12 * nv) * P / copy_rate * 1e6 for nv in VIEWS})

    if "loss" in only:
        nmax = max(VIEWS)
        d = torch.randn(nmax, 3, H, W, device=dev, generator=gen)
        N = [(d[k] / d[k].norm(dim=0, keepdim=True) * (0.05 + 0.95 * torch.rand(1, H, W, device=dev, generator=gen))).requires_grad_(True)
             for k in range(nmax)]
        A = [torch.where(torch.rand(1, H, W, device=dev, generator=gen) < 0.04, 0.2, 0.55 + 0.45 * torch.rand(1, H, W, device=dev, generator=gen))
             for _ in range(nmax)]
        p = [torch.randn(3, H, W, device=dev, generator=gen) for _ in range(nmax)]
        m = [torch.where(torch.rand(H, W, device=dev, generator=gen) < 0.1, 0.0, 0.25 + 0.75 * torch.rand(H, W, device=dev, generator=gen))
             for _ in range(nmax)]
        del d
        for mode in ("cos", "l1"):
            for nv in VIEWS:
                cot = torch.randn(nv, device=dev, generator=gen)

                def fwd_bwd(fn, nv=nv, mode=mode, cot=cot):
                    for t in N:
                        t.grad = None
                    fn(N[:nv], A[:nv], p[:nv], m[:nv], mode=mode)[0].backward(cot)

                fns = {"hip": normal_map_loss} if args.hip_only else {"hip": normal_map_loss, "torch": normal_map_loss_torch}
                for k, st in alternate({k: (lambda f=f: fwd_bwd(f)) for k, f in fns.items()}, args.repeats, args.warmup).items():
                    put("loss_%s_%s_fwd_bwd_V%d" % (k, mode, nv), st)
                with torch.no_grad():
                    _, count = normal_map_loss(N[:nv], A[:nv], p[:nv], m[:nv], mode=mode)
                extra["loss_valid_weight_share"] = (count.sum() / (nv * H * W)).item()
        # with a mask: the forward reads 32 B/px (N, A, p, m), the backward reads the same and writes 12
        extra["loss_floor_us_per_view"] = {"fwd": 32 * H * W / copy_rate * 1e6, "bwd": 44 * H * W / copy_rate * 1e6}

    if "render" in only:
        scene = synth_scene(P, 0, 0.5, 3)
        pipe, bg = PipelineParams(), torch.zeros(3, device=dev)
        bag = GaussianBag.from_activated(scene, 3, device=dev)
        cam = look_at_origin_camera(W, H, device=dev)
        g_img = torch.randn(3, H, W, device=dev, generator=gen)

        def clear():
            for t in (bag._xyz, bag._features_dc, bag._features_rest, bag._opacity, bag._scaling, bag._rotation):
                t.grad = None

        def colour():
            clear()
            (render(cam, bag, pipe, bg, 0.0, None)["render"] * g_img).sum().backward()

        def normals():
            clear()
            (render_normals(cam, bag, pipe, None)["normal"] * g_img).sum().backward()

        for k, st in alternate({"render_fwd_bwd": colour, "render_normals_fwd_bwd": normals}, args.repeats, args.warmup).items():
            put(k, st)

    line = {"metric": f"ms per call, median of {args.repeats} after {args.warmup} warm-ups; fwd: forward under no_grad, fwd_bwd: forward + backward "
                      f"through autograd; normals: P = {P}; loss: {H}x{W} with a mask; render: P = {P}, {W}x{H}",
            "device": torch.cuda.get_device_name(0), "ms": res, "copy_rate_TB_per_s": copy_rate / 1e12, **extra}
    print(json.dumps(line))


if __name__ == "__main__":
    main()
