"""The camera side of one training step for V of N = 200 cameras: the pose -> matrix chain each way under fixed cotangents, then the
per-camera Adam step over rotation, translation and fov.  Routes:
  a_cameras_torch_adam        V PoseCamera.get_matrices (one launch each way per camera) + per camera a torch.optim.Adam over three groups
  a_cameras_torch_adam_fused  the same with fused=True, where PyTorch accepts it for these tensors
  b_pose_bank                 PoseBank.get_matrices over the V rows (one launch each way) + one PoseAdam.step
The work is launch- and host-bound, so the figure is WALL time per step between two device synchronisations around --steps steps, best
of --rounds rounds that alternate the routes; beside it the number of device kernels one step launches on each route (torch.profiler).
Prints one JSON line.
Usage: python tools/bench_pose_bank.py [--steps 200] [--rounds 3] [--views 1,5,16] [--no-count]"""
import argparse, json, os, sys, time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "bundle-adjusting-gaussian-splatting_amd")]
from bags_raster import PoseAdam, PoseBank
from bags_raster.synth import sphere_views

LRS = (1e-3, 1e-3, 1e-4)           # rotation, translation, fov


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=200); ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=20); ap.add_argument("--N", type=int, default=200)
    ap.add_argument("--views", default="1,5,16"); ap.add_argument("--no-count", action="store_true")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_pose_bank needs the GPU: a time measured anywhere else says nothing")
    dev = torch.device("cuda", 0)
    N = args.N
    g = torch.Generator().manual_seed(3)

    def routes(V):
        cots = [torch.randn(V, 4, 4, generator=g).to(dev) for _ in range(3)] + [torch.randn(V, 3, generator=g).to(dev)]
        rows_of = lambda i: [(i * V + j) % N for j in range(V)]

        def per_camera(**kw):
            cams = sphere_views(N, 64, 48, noise=0.05, device=dev)
            opts = [torch.optim.Adam([{"params": [c.delta_quaternion], "lr": LRS[0]}, {"params": [c.delta_translation], "lr": LRS[1]},
                                      {"params": [c.learnable_fovx, c.learnable_fovy], "lr": LRS[2]}], **kw) for c in cams]
            it = [0]

            def step():
                rows = rows_of(it[0]); it[0] += 1
                loss = 0.0
                for v, r in enumerate(rows):
                    out = cams[r].get_matrices()
                    loss = loss + sum((c[v] * o).sum() for c, o in zip(cots, out))
                loss.backward()
                for r in rows:
                    opts[r].step(); opts[r].zero_grad(set_to_none=True)
            return step

        def bank():
            b = PoseBank.from_cameras(sphere_views(N, 64, 48, noise=0.05, device=dev))
            opt = PoseAdam(b, *LRS)
            it = [0]

            def step():
                rows = rows_of(it[0]); it[0] += 1
                out = b.get_matrices(rows)
                sum((c * o).sum() for c, o in zip(cots, out)).backward()
                opt.step(rows); opt.zero_grad()
            return step
        built = {"a_cameras_torch_adam": per_camera(), "b_pose_bank": bank()}
        try:
            fused = per_camera(fused=True)
            fused(); torch.cuda.synchronize()
            built["a_cameras_torch_adam_fused"] = fused
        except Exception as e:                                  # PyTorch refuses fused=True for these tensors: reported, not hidden
            built["a_cameras_torch_adam_fused"] = f"rejected: {type(e).__name__}: {str(e)[:120]}"
        return built

    def wall(fn):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(args.steps):
            fn()
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) / args.steps * 1e3

    def launches(fn):
        from torch.profiler import ProfilerActivity, profile
        fn(); torch.cuda.synchronize()
        with profile(activities=[ProfilerActivity.CPU, ProfilerActivity.CUDA]) as prof:
            fn(); torch.cuda.synchronize()
        return sum(1 for e in prof.events() if e.device_type == torch.autograd.DeviceType.CUDA and "memcpy" not in e.name.lower()
                   and "memset" not in e.name.lower())

    ms, rounds, count = {}, {}, {}
    for V in [int(v) for v in args.views.split(",")]:
        built = routes(V)
        legs = {k: f for k, f in built.items() if callable(f)}
        for f in legs.values():
            for _ in range(args.warmup):
                f()
        per = {k: [] for k in legs}
        for _ in range(args.rounds):                            # alternating: a drift of the machine hits every route alike
            for k, f in legs.items():
                per[k].append(wall(f))
        key = f"V={V}"
        ms[key] = {k: (min(per[k]) if k in legs else built[k]) for k in built}
        rounds[key] = per
        if not args.no_count:
            try:
                count[key] = {k: launches(f) for k, f in legs.items()}
            except Exception as e:
                count[key] = f"not measured: {type(e).__name__}: {str(e)[:120]}"
    print(json.dumps({"metric": f"wall ms per step (chain forward + backward + per-camera Adam) for V of N={N} cameras, best of {args.rounds} "
                                f"alternating rounds of {args.steps} steps between two device synchronisations",
                      "device": torch.cuda.get_device_name(0), "N": N, "ms": ms, "rounds_ms": rounds, "kernel_launches_per_step": count}))


if __name__ == "__main__":
    main()
