"""Cost of the opt-in depth / weights gradients (depth_weights_grad, ABI 11) on the bench workload (BASELINE config 3: 500 k
Gaussians, 1920x1080, SH degree 3, pose gradients): forward + backward with cotangents on image, depth and weights against
image only, the two legs alternating in one process.  Per leg: the step (event-timed on the stream) and blend_bwd alone
(the library's profile mode 1: events on the kernel's own dispatch).  Prints one JSON line.

    python tools/bench_depth_grad.py [--rounds 8] [--steps 40] [--warmup 20]
"""
import argparse
import json
import math
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "bundle-adjusting-gaussian-splatting_amd"))

import torch  # noqa: E402

from bags_raster import GaussianRasterizationSettings, GaussianRasterizer, _lib  # noqa: E402
from bags_raster.synth import look_at_origin_camera, synth_scene  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=8)
    ap.add_argument("--steps", type=int, default=40)
    ap.add_argument("--warmup", type=int, default=20)
    a = ap.parse_args()
    dev = torch.device("cuda")
    W, H = 1920, 1080
    scene = {k: v.to(dev).requires_grad_(True) for k, v in synth_scene(500_000, 0, 0.5, 3).items()}
    cam = look_at_origin_camera(W, H, device=dev)
    with torch.no_grad():
        vm, pm, K, cp = (t.detach().clone() for t in (cam.get_world_view_transform(), cam.get_full_proj_transform(),
                                                      cam.get_intrinsic(), cam.get_camera_center()))
    cams = [t.requires_grad_(True) for t in (vm, pm, K, cp)]
    P = scene["means3D"].shape[0]
    m2, m2d, sf = (torch.zeros(P, 3, device=dev, requires_grad=True), torch.zeros(P, 3, device=dev, requires_grad=True),
                   torch.zeros(3, device=dev, requires_grad=True))
    st = GaussianRasterizationSettings(H, W, math.tan(cam.FoVx * 0.5), math.tan(cam.FoVy * 0.5), torch.zeros(3, device=dev), 1.0,
                                       cams[0], cams[1], cams[2], 3, cams[3], depth_weights_grad=True)
    rast = GaussianRasterizer(st)
    g = torch.Generator(device=dev).manual_seed(0)
    gi = torch.randn(3, H, W, device=dev, generator=g)
    gd = torch.randn(1, H, W, device=dev, generator=g) * 0.1
    gw = torch.randn(1, H, W, device=dev, generator=g)
    params = list(scene.values()) + cams + [m2, m2d, sf]

    def step(extra):
        for p in params:
            p.grad = None
        img, _, depth, weights, _ = rast(means3D=scene["means3D"], means2D=m2, means2D_densify=m2d, shift_factors=sf,
                                         shs=scene["shs"], opacities=scene["opacities"], scales=scene["scales"],
                                         rotations=scene["rotations"])
        if extra:
            torch.autograd.backward([img, depth, weights], [gi, gd, gw])
        else:
            img.backward(gi)

    def leg(extra, n):
        _lib.profile_enable(1)
        _lib.profile_read()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(n):
            step(extra)
        e1.record()
        e1.synchronize()
        prof = _lib.profile_read()
        _lib.profile_enable(0)
        ms, calls = prof.get("blend_bwd", (float("nan"), 1))
        return e0.elapsed_time(e1) / n, ms / max(calls, 1)

    for extra in (False, True):
        leg(extra, a.warmup)
    res = {False: ([], []), True: ([], [])}
    for r in range(a.rounds):
        for extra in ((False, True) if r % 2 == 0 else (True, False)):
            s_ms, b_ms = leg(extra, a.steps)
            res[extra][0].append(s_ms)
            res[extra][1].append(b_ms)
    med = {k: (statistics.median(v[0]), statistics.median(v[1])) for k, v in res.items()}
    out = {"workload": "config3 500k 1920x1080 sh3 pose", "rounds": a.rounds, "steps": a.steps,
           "step_ms_image_only": round(med[False][0], 4), "step_ms_image_depth_weights": round(med[True][0], 4),
           "step_delta_pct": round(100.0 * (med[True][0] / med[False][0] - 1.0), 2),
           "blend_bwd_ms_image_only": round(med[False][1], 4), "blend_bwd_ms_image_depth_weights": round(med[True][1], 4),
           "blend_bwd_delta_pct": round(100.0 * (med[True][1] / med[False][1] - 1.0), 2),
           "per_round": {"image_only": [[round(x, 4) for x in v] for v in res[False]],
                         "image_depth_weights": [[round(x, 4) for x in v] for v in res[True]]},
           "build": _lib.load().bags_build_info().decode()}
    print(json.dumps(out))


if __name__ == "__main__":
    main()
