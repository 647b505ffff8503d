"""The three call sites of the MCMC strategy at 500 k Gaussians, SH degree 3 (59 floats each, both Adam moments):
  relocate    5 % of the rows dead (the most transparent ones), sources drawn by opacity inside the timed call
  add_new     cap_max far away: 5 % new rows, sources drawn inside the timed call
  mcmc_noise  the per-iteration SGLD step on xyz (--noise-calls calls per sample: one call is tens of microseconds)
each as  a  the PyTorch route on the GPU (tests/mcmc_reference.py: the published relocate_gs / add_new_gs / noise block; its draw is the
same torch.multinomial, its compute_relocation the PyTorch statement, its noise torch.randn_like)  and  b  the fused call
(csrc/mcmc.hip).  Every repeat starts from a fresh copy of the same state (made outside the timed region); a and b alternate within
a repeat; median of --repeats after one warm-up round, device events around the call, host work between the launches included.
Prints one JSON line.  Usage: python tools/bench_mcmc.py [--repeats 9] [--P 500000]"""
import argparse, json, os, statistics, sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "bundle-adjusting-gaussian-splatting_amd"), os.path.join(ROOT, "tests")]
import densify_reference as D
import mcmc_reference as M
from bags_raster import GaussianAdam
from bags_raster.gaussians import GaussianBag

LEAF = {"xyz": "_xyz", "f_dc": "_features_dc", "f_rest": "_features_rest", "opacity": "_opacity", "scaling": "_scaling", "rotation": "_rotation"}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=9); ap.add_argument("--P", type=int, default=500_000)
    ap.add_argument("--noise-calls", type=int, default=20)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_mcmc needs the GPU: a time measured anywhere else says nothing")
    dev = torch.device("cuda", 0)
    P = args.P
    opt0, stats0 = M.make_case(P, 1, GaussianAdam, dev, sh_degree=3)
    opacity = torch.sigmoid(D.params(opt0)["opacity"].detach()).reshape(-1)
    dead = opacity <= torch.quantile(opacity, 0.05)
    n_dead = int(dead.sum())

    def fresh(cls):
        opt = D.clone_optimizer(opt0, device=dev, opt_cls=cls)
        bag = GaussianBag(3)
        for n, q in D.params(opt).items():
            setattr(bag, LEAF[n], q)
        for k, v in stats0.items():
            setattr(bag, k, v.clone())
        return opt, bag

    def gen():
        return torch.Generator(device=dev).manual_seed(7)

    def ref_relocate(opt, bag):
        alive = (~dead).nonzero().reshape(-1)
        p = torch.sigmoid(bag._opacity.detach()[alive, 0])
        return M.relocate(opt, dead, alive[torch.multinomial(p / p.sum(), n_dead, replacement=True, generator=gen())])

    def ref_add_new(opt, bag):
        p = torch.sigmoid(bag._opacity.detach()[:, 0])
        return M.add_new(opt, 10 * P, torch.multinomial(p / p.sum(), int(1.05 * P) - P, replacement=True, generator=gen()))

    def ref_noise(opt, bag):
        for _ in range(args.noise_calls):
            with torch.no_grad():
                bag._xyz.copy_(M.mcmc_noise(bag._xyz, bag._opacity, bag._scaling, bag._rotation, 0.08, torch.randn_like(bag._xyz)))

    def fused_noise(opt, bag):
        for i in range(args.noise_calls):
            bag.mcmc_noise(0.08, seed=i)
    legs = {"relocate": ((torch.optim.Adam, ref_relocate), (GaussianAdam, lambda o, b: b.relocate(o, dead, generator=gen()))),
            "add_new": ((torch.optim.Adam, ref_add_new), (GaussianAdam, lambda o, b: b.add_new(o, 10 * P, generator=gen()))),
            "mcmc_noise": ((torch.optim.Adam, ref_noise), (GaussianAdam, fused_noise))}
    res, spread, results = {}, {}, {}
    for name, pair in legs.items():
        ms = ([], [])
        for rep in range(args.repeats + 1):                         # the first round warms up (allocator, code objects)
            for side, (cls, fn) in enumerate(pair):
                state = fresh(cls)
                torch.cuda.synchronize()
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                out = fn(*state)
                e1.record(); torch.cuda.synchronize()
                if rep:
                    ms[side].append(e0.elapsed_time(e1) / (args.noise_calls if name == "mcmc_noise" else 1))
                if isinstance(out, dict):
                    results[f"{'ab'[side]}_{name}"] = {k: v for k, v in out.items() if k != "stats"}
                del state
                torch.cuda.empty_cache()
        for side in (0, 1):
            key = f"{'ab'[side]}_{name}"
            res[key], spread[key] = statistics.median(ms[side]), [min(ms[side]), max(ms[side])]
    line = {"metric": f"ms per call, {P} Gaussians x 59 floats x (param, exp_avg, exp_avg_sq), median of {args.repeats}; a = PyTorch route, b = fused",
            "device": torch.cuda.get_device_name(0), "P": P, "dead": n_dead, "noise_calls_per_sample": args.noise_calls, "results": results,
            "ms": res, "min_max_ms": spread, "speedup_b_over_a": {n: res[f"a_{n}"] / res[f"b_{n}"] for n in legs}}
    print(json.dumps(line))


if __name__ == "__main__":
    main()
