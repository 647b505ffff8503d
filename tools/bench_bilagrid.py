"""The bilateral-grid step at full resolution: V images of 1080 x 1920 through V grids of an N = 200 bank of (16,16,8) grids, V = 1 and
V = 5, and the total variation of the bank.
  a  apply_bilagrid       (csrc/bilagrid.hip): forward + backward through autograd, dL/dimage and dL/dgrids wanted
  b  bilagrid_torch       the same function in plain PyTorch on the GPU (gathers and lerps): forward + backward through autograd
  c  grid_sample          the published formulation on the GPU: 5-D F.grid_sample + per-pixel matmul, forward + backward
  tv bilagrid_tv_loss against bilagrid_tv_loss_torch, forward + backward
The images are V separate tensors, as render_views returns them; b and c stack them themselves.  Median of --repeats after --warmup
runs, device events around each run, host work between the launches included; a alternates with b and, separately, with c, so that
the device's drift hits both alike.  Prints one JSON line, with the byte model's floors beside it (6.29 TB/s measured copy rate;
24 B/px forward, 36 B/px dL/dimage, and 16 B/px x 12 readers for dL/dgrid as built: every pixel is read by four vertices' workgroups
for each of three output channels).
Usage: python tools/bench_bilagrid.py [--repeats 200] [--warmup 20] [--views 1,5] [--only abc] [--no-tv]"""
import argparse, json, os, statistics, sys

import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "bundle-adjusting-gaussian-splatting_amd")]
from bags_raster import apply_bilagrid, bilagrid_torch, bilagrid_tv_loss, bilagrid_tv_loss_torch

COPY_RATE = 6.29e12                                          # bytes per second, measured float4 copy on the MI355X


def timed(fn):
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    fn()
    e1.record(); torch.cuda.synchronize()
    return e0.elapsed_time(e1)


def published(img, G):
    """gsplat's slice-and-apply: images (V,3,H,W), grids (V,12,L,Gy,Gx)."""
    V, _, H, W = img.shape
    xs = ((torch.arange(W, dtype=img.dtype, device=img.device) + 0.5) / W - 0.5) * 2
    ys = ((torch.arange(H, dtype=img.dtype, device=img.device) + 0.5) / H - 0.5) * 2
    rgb = img.permute(0, 2, 3, 1)
    luma = (rgb * torch.tensor([0.299, 0.587, 0.114], dtype=img.dtype, device=img.device)).sum(-1)
    coords = torch.stack([xs[None, None, :].expand(V, H, W), ys[None, :, None].expand(V, H, W), luma * 2 - 1], -1)[:, None]
    A = F.grid_sample(G, coords, mode="bilinear", align_corners=True, padding_mode="border")[:, :, 0]
    A = A.permute(0, 2, 3, 1).reshape(V, H, W, 3, 4)
    return (torch.matmul(A[..., :3], rgb[..., None])[..., 0] + A[..., 3]).permute(0, 3, 1, 2)


def alternate(routes, warmup, repeats):
    ms = {k: [] for k, _ in routes}
    for rep in range(warmup + repeats):
        for k, f in routes:
            t = timed(f)
            if rep >= warmup:
                ms[k].append(t)
    return {k: statistics.median(v) for k, v in ms.items()}, {k: [min(v), max(v)] for k, v in ms.items()}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=200); ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--views", default="1,5"); ap.add_argument("--only", default="abc"); ap.add_argument("--no-tv", action="store_true")
    ap.add_argument("--H", type=int, default=1080); ap.add_argument("--W", type=int, default=1920); ap.add_argument("--N", type=int, default=200)
    ap.add_argument("--grid", default="16,16,8")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_bilagrid needs the GPU: a time measured anywhere else says nothing")
    dev = torch.device("cuda", 0)
    H, W, N = args.H, args.W, args.N
    Gx, Gy, Lz = (int(g) for g in args.grid.split(","))
    gen = torch.Generator(device=dev).manual_seed(0)
    grids = (torch.eye(3, 4, device=dev).reshape(1, 12, 1, 1, 1) + 0.2 * (torch.rand(N, 12, Lz, Gy, Gx, device=dev, generator=gen) * 2 - 1)).requires_grad_(True)
    res, spread, extra = {}, {}, {}
    for V in [int(v) for v in args.views.split(",")]:
        images = [torch.rand(3, H, W, device=dev, generator=gen).requires_grad_(True) for _ in range(V)]
        cots = [torch.randn(3, H, W, device=dev, generator=gen) for _ in range(V)]
        rows = [(37 * v + 11) % N for v in range(V)]

        def clear():
            grids.grad = None
            for t in images:
                t.grad = None

        def hip():
            clear()
            torch.autograd.backward(apply_bilagrid(images, grids, rows), cots)

        def torch_path():
            clear()
            torch.autograd.backward(bilagrid_torch(images, grids[rows]), cots)

        def grid_sample_path():
            clear()
            torch.autograd.backward(published(torch.stack(images), grids[rows]), torch.stack(cots))

        for key, other in (("b_torch", torch_path), ("c_grid_sample", grid_sample_path)):
            if key[0] not in args.only:
                continue
            routes = ([("a_hip", hip)] if "a" in args.only else []) + [(key, other)]
            med, mm = alternate(routes, args.warmup, args.repeats)
            for k in med:
                name = "%s_V%d" % (k if k != "a_hip" else "a_hip_beside_" + key[0], V)
                res[name], spread[name] = med[k], mm[k]
            if len(routes) == 2:                             # the two routes on the same inputs
                hip()
                ga = [t.grad.clone() for t in images] + [grids.grad.clone()]
                other()
                gb = [t.grad for t in images] + [grids.grad]
                extra["grad_rel_diff_hip_vs_%s_fp32_V%d" % (key[2:], V)] = max(
                    ((x - y).double().norm() / y.double().norm().clamp_min(1e-30)).item() for x, y in zip(ga, gb))
        if args.only == "a":
            med, mm = alternate([("a_hip", hip)], args.warmup, args.repeats)
            res["a_hip_V%d" % V], spread["a_hip_V%d" % V] = med["a_hip"], mm["a_hip"]
    if not args.no_tv:
        def tv_hip():
            grids.grad = None
            bilagrid_tv_loss(grids).backward()

        def tv_torch():
            grids.grad = None
            bilagrid_tv_loss_torch(grids).backward()

        med, mm = alternate([("tv_hip", tv_hip), ("tv_torch", tv_torch)], args.warmup, args.repeats)
        res.update(med); spread.update(mm)
    px = H * W
    line = {"metric": f"ms per forward + backward through autograd, {H}x{W}, N = {N}, grid ({Gx},{Gy},{Lz}), median of {args.repeats} after {args.warmup} warm-ups",
            "device": torch.cuda.get_device_name(0), "ms": res, "min_max_ms": spread,
            "floor_us_per_view": {"forward_24B_per_px": 24 * px / COPY_RATE * 1e6, "dimage_36B_per_px": 36 * px / COPY_RATE * 1e6,
                                  "dgrid_192B_per_px": 192 * px / COPY_RATE * 1e6},
            "floor_us_tv": {"forward_4B_per_elem": 4 * grids.numel() / COPY_RATE * 1e6, "backward_8B_per_elem": 8 * grids.numel() / COPY_RATE * 1e6}, **extra}
    print(json.dumps(line))


if __name__ == "__main__":
    main()
