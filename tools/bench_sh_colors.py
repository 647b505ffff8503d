"""The SH colour path of render(hybrid=True) at 500 k Gaussians, degree 3, on the GPU: csrc/sh_colors.hip against the PyTorch
``_python_colors`` it replaces, and the training iteration around it.  Device events around back-to-back repetitions, after a
warm-up of every leg; the legs of a comparison alternate, each is timed ``--rounds`` times and every round is printed.

  kernel pair        bags_sh_colors_forward / _backward called directly (split layout, all four gradients, 20 % of the cotangent
                     rows zero as for culled Gaussians), with the achieved fraction of 8 TB/s on the algorithmic bytes
  autograd pair      bags_raster.sh_colors forward + backward      |  the same leaves, the same cotangent
  python_colors      render._python_colors forward + backward      |
  iteration          camera chain -> render(hybrid=True) -> photometric loss -> backward @1920x1080; with --parent-render FILE
                     (the render.py of the commit before sh_colors) the same iteration through that file, alternating

  --views V [V ...]  instead of the legs above: a step of V views over the same Gaussians, forward + backward with every gradient,
                     three routes alternating in the same process: (a) V single-view forward + backward calls, the gradients of
                     dc / rest / xyz accumulated as autograd does (``grad += g`` from the second view on); (b) one
                     bags_sh_colors_views_forward + _backward; (c) a float4 copy of (b)'s algorithmic bytes.  Checks (b)'s
                     gradients against (a)'s before timing.

Prints one JSON line.  Usage: python tools/bench_sh_colors.py [--reps 200] [--steps 20] [--rounds 3] [--parent-render FILE]
                              python tools/bench_sh_colors.py --views 2 4 5 [--reps 100] [--rounds 3]"""
import argparse, importlib.util, json, os, sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "bundle-adjusting-gaussian-splatting_amd")]
import bags_raster
from bags_raster import _lib as L, loss as LS, sh_colors
from bags_raster.gaussians import GaussianBag
from bags_raster.synth import synth_scene, sphere_views

PEAK_BYTES_PER_S = 8e12


def timed(fn, reps):
    for _ in range(5):
        fn()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(reps):
        fn()
    e1.record(); torch.cuda.synchronize()
    return e0.elapsed_time(e1) / reps


def views_leg(args, dev):
    """Routes (a), (b), (c) of the module docstring at each V of --views."""
    P, K, deg = args.P, 16, 3
    lib = L.load()
    pc = GaussianBag.from_activated(synth_scene(P, 0, 0.5, 3), 3, device=dev)
    dc, rest, xyz = pc._features_dc.detach(), pc._features_rest.detach(), pc._xyz.detach()
    st = torch.cuda.current_stream().cuda_stream
    res = {"device": torch.cuda.get_device_name(0), "P": P, "K": K, "deg": deg, "build": lib.bags_build_info().decode(), "views": {}}
    for V in args.views:
        with torch.no_grad():
            centres = [c.get_matrices(None, None)[3].clone() for c in sphere_views(V, 64, 64, noise=0.05, device=dev)]
        g = torch.Generator().manual_seed(2)
        cots = []
        for v in range(V):
            cot = torch.randn(P, 3, generator=g)
            cot[(2 + v)::5] = 0.0                                         # 20 % of the rows culled, other rows in each view
            cots.append(cot.to(dev))
        nz = [int((c != 0).any(dim=1).sum()) for c in cots]
        nz_any = int(torch.stack([(c != 0).any(dim=1) for c in cots]).any(dim=0).sum())
        # (a) the single-view pair per view, accumulated into the running gradients
        one = [L.BagsShColors(P, K, deg, 0, dc.data_ptr(), rest.data_ptr(), xyz.data_ptr(), c.data_ptr()) for c in centres]
        rgb_a = [torch.empty(P, 3, device=dev) for _ in range(V)]
        acc = [torch.empty_like(dc), torch.empty_like(rest), torch.empty_like(xyz)]
        tmp = [torch.empty_like(t) for t in acc]
        gc_a = [torch.empty(3, device=dev) for _ in range(V)]
        ws1_bytes = lib.bags_sh_colors_workspace_size(P)
        ws1 = torch.empty(ws1_bytes, dtype=torch.uint8, device=dev)

        def route_a():
            for v in range(V):
                L.check(lib.bags_sh_colors_forward(one[v], rgb_a[v].data_ptr(), st), "fwd")
            for v in range(V):
                into = acc if v == 0 else tmp
                L.check(lib.bags_sh_colors_backward(one[v], cots[v].data_ptr(), ws1.data_ptr(), ws1_bytes, *[t.data_ptr() for t in into],
                                                    gc_a[v].data_ptr(), st), "bwd")
                if v:
                    for a_, t_ in zip(acc, tmp):
                        a_ += t_
        # (b) the multi-view pair
        many = L.BagsShColorsViews(P, K, deg, V, dc.data_ptr(), rest.data_ptr(), xyz.data_ptr(), L.ptr_table(centres + [None] * (L.MAX_SH_VIEWS - V)))
        rgb_b = [torch.empty(P, 3, device=dev) for _ in range(V)]
        g_b = [torch.empty_like(t) for t in acc]
        gc_b = [torch.empty(3, device=dev) for _ in range(V)]
        wsv_bytes = lib.bags_sh_colors_views_workspace_size(P, V)
        wsv = torch.empty(wsv_bytes, dtype=torch.uint8, device=dev)
        t_rgb, t_cot, t_gc = L.ptr_table(rgb_b), L.ptr_table(cots), L.ptr_table(gc_b)

        def route_b():
            L.check(lib.bags_sh_colors_views_forward(many, t_rgb, st), "views fwd")
            L.check(lib.bags_sh_colors_views_backward(many, t_cot, wsv.data_ptr(), wsv_bytes, *[t.data_ptr() for t in g_b], t_gc, st), "views bwd")
        bytes_fwd = P * (12 * K + 12) + V * P * 12
        bytes_bwd = V * P * 12 + nz_any * (12 * K + 12) + P * (12 * K + 12)
        bytes_a = sum(P * (12 * K + 24) + P * (12 + 12 * K + 12) + n * (12 * K + 12) for n in nz) + (V - 1) * 3 * P * (12 * K + 12)
        # (c) a float4 copy moving (b)'s bytes: half of them read, half written
        n4 = (bytes_fwd + bytes_bwd) // 32
        src, dst = torch.empty(n4, 4, device=dev), torch.empty(n4, 4, device=dev)
        route_c = lambda: dst.copy_(src)
        route_a(); route_b(); torch.cuda.synchronize()
        r = {"same_bits_as_fold": [bool(torch.equal(x, y)) for x, y in zip(acc + gc_a + rgb_a, g_b + gc_b + rgb_b)],
             "a_single_view_ms": [], "b_multi_view_ms": [], "c_copy_ms": [], "b_fwd_ms": [], "b_bwd_ms": [],
             "bytes_a_model": bytes_a, "bytes_b_fwd": bytes_fwd, "bytes_b_bwd": bytes_bwd, "rows_with_a_contributing_view": nz_any}
        for _ in range(args.rounds):
            r["a_single_view_ms"].append(timed(route_a, args.reps))
            r["b_multi_view_ms"].append(timed(route_b, args.reps))
            r["c_copy_ms"].append(timed(route_c, args.reps))
        r["b_fwd_ms"] = [timed(lambda: L.check(lib.bags_sh_colors_views_forward(many, t_rgb, st), "f"), args.reps) for _ in range(args.rounds)]
        r["b_bwd_ms"] = [timed(lambda: L.check(lib.bags_sh_colors_views_backward(many, t_cot, wsv.data_ptr(), wsv_bytes, *[t.data_ptr() for t in g_b], t_gc, st), "b"),
                               args.reps) for _ in range(args.rounds)]
        r["b_fraction_of_8TBs"] = (bytes_fwd + bytes_bwd) / (min(r["b_multi_view_ms"]) * 1e-3) / PEAK_BYTES_PER_S
        r["a_over_b"] = min(r["a_single_view_ms"]) / min(r["b_multi_view_ms"])
        res["views"][str(V)] = r
    print(json.dumps(res))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=200); ap.add_argument("--steps", type=int, default=20); ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--P", type=int, default=500_000)
    ap.add_argument("--parent-render", default=None, help="render.py of the parent commit: the iteration 'before'")
    ap.add_argument("--views", type=int, nargs="+", default=None, help="time a step of V views: single-view calls, the multi-view pair, a copy")
    args = ap.parse_args()
    assert torch.cuda.is_available(), "bench_sh_colors needs the GPU: there is nothing to time on the host"
    dev = torch.device("cuda", 0)
    if args.views:
        return views_leg(args, dev)
    R = sys.modules["bags_raster.render"]
    P, K, deg, W, H = args.P, 16, 3, 1920, 1080
    scene = synth_scene(P, 0, 0.5, 3)
    cam = sphere_views(1, W, H, noise=0.05, device=dev)[0]
    pc = GaussianBag.from_activated(scene, 3, device=dev)
    with torch.no_grad():
        campos = cam.get_matrices(None, None)[3].clone()
    cot = torch.randn(P, 3, generator=torch.Generator().manual_seed(2)).to(dev)
    cot[2::5] = 0.0
    nz = int((cot != 0).any(dim=1).sum())
    res = {"device": torch.cuda.get_device_name(0), "P": P, "K": K, "deg": deg, "build": L.load().bags_build_info().decode()}

    # ---- the kernels alone
    lib = L.load()
    dc, rest, xyz = pc._features_dc.detach(), pc._features_rest.detach(), pc._xyz.detach()
    a = L.BagsShColors(P, K, deg, 0, dc.data_ptr(), rest.data_ptr(), xyz.data_ptr(), campos.data_ptr())
    rgb = torch.empty(P, 3, device=dev)
    g = [torch.empty_like(dc), torch.empty_like(rest), torch.empty_like(xyz), torch.empty(3, device=dev)]
    ws_bytes = lib.bags_sh_colors_workspace_size(P)
    ws = torch.empty(ws_bytes, dtype=torch.uint8, device=dev)
    st = torch.cuda.current_stream().cuda_stream
    fwd = lambda: L.check(lib.bags_sh_colors_forward(a, rgb.data_ptr(), st), "fwd")
    bwd = lambda: L.check(lib.bags_sh_colors_backward(a, cot.data_ptr(), ws.data_ptr(), ws_bytes, *[t.data_ptr() for t in g], st), "bwd")
    bytes_fwd = P * (12 * K + 12 + 12)
    bytes_bwd = P * (12 + 12 * K + 12) + nz * (12 * K + 12)          # cotangent, SH rows and xyz rows out; row and position in where the cotangent is non-zero
    res["kernel_fwd_ms"] = [timed(fwd, args.reps) for _ in range(args.rounds)]
    res["kernel_bwd_ms"] = [timed(bwd, args.reps) for _ in range(args.rounds)]
    res["kernel_fwd_bytes"], res["kernel_bwd_bytes"], res["cotangent_rows_nonzero"] = bytes_fwd, bytes_bwd, nz
    res["kernel_fwd_fraction_of_8TBs"] = bytes_fwd / (min(res["kernel_fwd_ms"]) * 1e-3) / PEAK_BYTES_PER_S
    res["kernel_bwd_fraction_of_8TBs"] = bytes_bwd / (min(res["kernel_bwd_ms"]) * 1e-3) / PEAK_BYTES_PER_S

    # ---- forward + backward through autograd: the fused function and the PyTorch path it replaces, same leaves, same cotangent
    leaves = [pc._features_dc, pc._features_rest, pc._xyz]
    campos_leaf = campos.clone().requires_grad_(True)

    def clear():
        for t in leaves + [campos_leaf]:
            t.grad = None

    def fused_pair():
        clear()
        sh_colors(deg, pc._features_dc, pc._xyz, campos_leaf, shs_rest=pc._features_rest).backward(cot)

    def python_pair():
        clear()
        R._python_colors(pc, pc._xyz, pc.get_features, campos_leaf, 0.0).backward(cot)
    res["autograd_pair_ms"], res["python_colors_ms"] = [], []
    for _ in range(args.rounds):
        res["autograd_pair_ms"].append(timed(fused_pair, args.reps // 4))
        res["python_colors_ms"].append(timed(python_pair, args.reps // 4))
    fused_pair(); gf = [t.grad.clone() for t in leaves + [campos_leaf]]
    python_pair(); gp = [t.grad.clone() for t in leaves + [campos_leaf]]
    res["grad_rel_diff_vs_python_colors"] = [((x - y).norm() / y.norm()).item() for x, y in zip(gf, gp)]
    clear()

    # ---- the iteration with hybrid=True, after and (with the parent's render.py) before
    gt = torch.rand(3, H, W, generator=torch.Generator().manual_seed(1)).to(dev)
    bg = torch.zeros(3, device=dev)
    pipe = R.PipelineParams()
    all_leaves = pc.leaves() + cam.pose_leaves()

    def iteration(render_fn):
        for t in all_leaves:
            t.grad = None
        out = render_fn(cam, pc, pipe, bg, 0.0, None, hybrid=True)
        LS.fused_photometric_loss(out["render"], gt).backward()
        return out
    legs = {"iteration_hybrid_ms": R.render}
    if args.parent_render:
        spec = importlib.util.spec_from_file_location("bags_raster._render_parent", args.parent_render)
        parent = importlib.util.module_from_spec(spec)
        parent.__package__ = "bags_raster"
        spec.loader.exec_module(parent)
        legs["iteration_hybrid_parent_ms"] = parent.render
        img_a = iteration(R.render)["render"].detach().clone(); ga = [t.grad.clone() for t in all_leaves]
        img_b = iteration(parent.render)["render"].detach(); gb = [t.grad.clone() for t in all_leaves]
        res["iteration_image_max_abs_diff"] = (img_a - img_b).abs().max().item()
        res["iteration_grad_rel_diff"] = [((x - y).norm() / y.norm()).item() for x, y in zip(ga, gb)]
    for k in legs:
        res[k] = []
    for _ in range(args.rounds):
        for k, fn in legs.items():
            res[k].append(timed(lambda: iteration(fn), args.steps))
    print(json.dumps(res))


if __name__ == "__main__":
    main()
