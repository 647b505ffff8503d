"""The cubemap stitch of one training step, forward + backward under a fixed cotangent, at the workload's shape: five 1080 x 1080
faces, C = 3, control grid 68 x 120, flow 1188 x 2112 cropped to 1080 x 1920, a 150 degree equidistant fisheye.  Routes:
  a_five_resample_image  what the library offered before: per face the control flow projected onto the face plane ON THE CONTROL GRID,
                         one resample_image per face, the product with the face's (precomputed) mask, the sum, and autograd
  b_resample_faces_torch resample_faces_torch on the GPU (interpolate, per-pixel projection, five grid_samples) and autograd
  c_resample_faces       resample_faces: one launch forward, pixels + gather + control-node gather backward
Route a is not the same function near the face boundaries (that is one reason for c); it is the same amount of work.  The figure is
WALL time per step between two device synchronisations around --steps steps, best of --rounds rounds that alternate the routes;
beside it the device kernels one step launches (torch.profiler) and a float4 copy that moves the fused pair's algorithmic bytes.
Prints one JSON line.
Usage: python tools/bench_resample_faces.py [--steps 50] [--rounds 3] [--no-count] [--only c_resample_faces]"""
import argparse, json, os, sys, time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "bundle-adjusting-gaussian-splatting_amd"), os.path.join(ROOT, "tests")]
from bags_raster import cube_face_matrices, resample_faces, resample_faces_torch
from bags_raster.distortion import resample_image
from faces_cases import fisheye_ctrl


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=50); ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=5); ap.add_argument("--no-count", action="store_true")
    ap.add_argument("--face", type=int, default=1080); ap.add_argument("--ctrl", default="68,120")
    ap.add_argument("--flow", default="1188,2112"); ap.add_argument("--crop", default="1080,1920")
    ap.add_argument("--only", default="", help="one route, e.g. c_resample_faces (for a kernel trace)")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_resample_faces needs the GPU: a time measured anywhere else says nothing")
    dev = torch.device("cuda", 0)
    pair = lambda s: tuple(int(v) for v in s.split(","))
    (h, w), fhw, chw, S, Cn = pair(args.ctrl), pair(args.flow), pair(args.crop), args.face, 3
    g = torch.Generator().manual_seed(3)
    faces = [torch.rand(Cn, S, S, generator=g).to(dev).requires_grad_(True) for _ in range(5)]
    ctrl = (fisheye_ctrl(h, w, 150.0, fhw[1] / fhw[0]) + 0.002 * torch.randn(h, w, 2, generator=g, dtype=torch.float64)).float().to(dev).requires_grad_(True)
    cot = torch.randn(Cn, *chw, generator=g).to(dev)
    M = cube_face_matrices(1.0, 1.0)[1]
    Md = M.float().to(dev)
    with torch.no_grad():
        index = resample_faces(faces, ctrl, M, fhw, chw)[1]
    masks = [(index == f).float().unsqueeze(0) for f in range(5)]
    used = [int((index == f).sum()) for f in range(-1, 5)]

    def reset():
        ctrl.grad = None
        for f in faces:
            f.grad = None

    def five_resample_image():
        reset()
        p = torch.cat([ctrl, torch.ones_like(ctrl[..., :1])], -1)
        abc = torch.einsum("fij,hwj->fhwi", Md, p)
        ok = abc[..., 2:] > 1e-6
        uv = torch.where(ok, abc[..., :2] / abc[..., 2:].clamp_min(1e-6), torch.full_like(abc[..., :2], 2.0))   # behind the face: outside
        out = None
        for f in range(5):
            o = resample_image(faces[f], uv[f], fhw, chw)[0] * masks[f]
            out = o if out is None else out + o
        out.backward(cot)

    def faces_torch():
        reset()
        resample_faces_torch(faces, ctrl, M, fhw, chw, face_index=index)[0].backward(cot)

    def fused():
        reset()
        resample_faces(faces, ctrl, M, fhw, chw)[0].backward(cot)
    legs = {"a_five_resample_image": five_resample_image, "b_resample_faces_torch": faces_torch, "c_resample_faces": fused}
    if args.only:
        legs = {args.only: legs[args.only]}

    def wall(fn, steps):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(steps):
            fn()
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) / steps * 1e3

    def launches(fn):
        from torch.profiler import ProfilerActivity, profile
        fn(); torch.cuda.synchronize()
        with profile(activities=[ProfilerActivity.CPU, ProfilerActivity.CUDA]) as prof:
            fn(); torch.cuda.synchronize()
        return sum(1 for e in prof.events() if e.device_type == torch.autograd.DeviceType.CUDA and "memcpy" not in e.name.lower()
                   and "memset" not in e.name.lower())

    for f in legs.values():
        for _ in range(args.warmup):
            f()
    # the fused pair's algorithmic bytes: forward reads the faces, writes the image and the map; backward reads the cotangent, the
    # map and the faces (dL/dflow) and writes every face gradient.  (Not counted: the control grid, and the taps / dL/dflow / lists
    # the backward's kernels hand each other.)
    face_b, img_b, idx_b = 5 * Cn * S * S * 4, Cn * chw[0] * chw[1] * 4, chw[0] * chw[1]
    algo = (face_b + img_b + idx_b) + (img_b + idx_b + face_b + face_b)
    n4 = algo // 2 // 16
    src, dst = torch.empty(n4, 4, device=dev), torch.empty(n4, 4, device=dev)
    copy = lambda: dst.copy_(src)
    for _ in range(args.warmup):
        copy()
    per, copy_ms = {k: [] for k in legs}, []
    for _ in range(args.rounds):                                # alternating: a drift of the machine hits every route alike
        for k, f in legs.items():
            per[k].append(wall(f, args.steps))
        copy_ms.append(wall(copy, 10 * args.steps))                # ten times the steps: a copy is a tenth of a step
    count = {}
    if not args.no_count:
        try:
            count = {k: launches(f) for k, f in legs.items()}
        except Exception as e:
            count = f"not measured: {type(e).__name__}: {str(e)[:120]}"
    print(json.dumps({"metric": f"wall ms per step (stitch forward + backward), best of {args.rounds} alternating rounds of {args.steps} steps "
                                f"between two device synchronisations",
                      "device": torch.cuda.get_device_name(0), "shape": {"faces": [5, Cn, S, S], "ctrl": [h, w], "flow": fhw, "crop": chw},
                      "pixels_per_face_none_first": used, "ms": {k: min(v) for k, v in per.items()}, "rounds_ms": per,
                      "fused_faster_than_a_in_every_round": None if args.only else
                      all(c < a for a, c in zip(per["a_five_resample_image"], per["c_resample_faces"])),
                      "kernel_launches_per_step": count, "algorithmic_bytes": algo, "float4_copy_of_them_ms": min(copy_ms),
                      "float4_copy_rounds_ms": copy_ms}))


if __name__ == "__main__":
    main()
