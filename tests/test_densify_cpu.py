"""No-GPU checks of the fused densify-and-prune / opacity reset: the C ABI surface and its argument validation (reported before
anything is enqueued), the GaussianBag methods' refusal of CPU tensors, the plain-PyTorch restatement the GPU tests compare against
(on a hand-written scene whose fates are written out here), and the generator of the GPU tests' inputs."""
import ctypes as C
import math
import os
import re

import pytest
import torch

import adam_reference as R
import densify_reference as D
from bags_raster import _lib
from bags_raster.gaussians import GaussianBag

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FUNCS = ("bags_densify_workspace_size", "bags_densify_plan", "bags_densify_apply", "bags_reset_opacity")
SIZES = (1, 63, 1001, 100_003, 500_000)           # every P tests/test_densify_gpu.py uses


@pytest.fixture(scope="module")
def lib():
    if not os.path.exists(_lib.LIB_PATH):
        import __graft_entry__ as g
        g.build()
    return _lib.load()


def _header_struct_fields(name):
    header = open(os.path.join(ROOT, "include", "bags_raster.h")).read()
    body = re.search(r"typedef struct %s \{(.*?)\} %s;" % (name, name), header, re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    fields = []
    for decl in body.split(";"):
        decl = decl.strip()
        if decl:
            fields += [re.sub(r"\[.*\]", "", part).strip().split()[-1].lstrip("*") for part in decl.split(",")]
    return fields


def test_symbols_are_declared_bound_and_exported(lib):
    header = open(os.path.join(ROOT, "include", "bags_raster.h")).read()
    for name in FUNCS:
        assert re.search(r"\b%s\s*\(" % name, header), name
        assert name in _lib.SYMBOLS and hasattr(lib, name), name
    assert lib.bags_abi_version() == 11 and "#define BAGS_ABI_VERSION 11" in header          # additive: no bump
    assert "#define BAGS_DENSIFY_MAX_GROUPS %d" % _lib.DENSIFY_MAX_GROUPS in header
    assert "#define BAGS_DENSIFY_MAX_CHILDREN %d" % _lib.DENSIFY_MAX_CHILDREN in header
    assert "BAGS_ROLE_OTHER = 0, BAGS_ROLE_XYZ = 1, BAGS_ROLE_SCALING = 2, BAGS_ROLE_ROTATION = 3, BAGS_ROLE_OPACITY = 4" in header
    assert (_lib.ROLE_OTHER, _lib.ROLE_XYZ, _lib.ROLE_SCALING, _lib.ROLE_ROTATION, _lib.ROLE_OPACITY) == (0, 1, 2, 3, 4)
    assert "BAGS_SCREEN_PUBLISHED = 0, BAGS_SCREEN_PRE_DENSIFY = 1" in header and (_lib.SCREEN_PUBLISHED, _lib.SCREEN_PRE_DENSIFY) == (0, 1)
    assert callable(GaussianBag.densify_and_prune) and callable(GaussianBag.reset_opacity)
    assert lib.bags_densify_workspace_size(500_000) >= 500_000 * 4
    assert lib.bags_densify_workspace_size(1000) < lib.bags_densify_workspace_size(100_000)


def test_struct_layout_matches_header():
    for cls in (_lib.BagsDensifyRule, _lib.BagsDensifyGroup):
        assert [f[0] for f in cls._fields_] == _header_struct_fields(cls.__name__), cls.__name__
    assert C.sizeof(_lib.BagsDensifyRule) == 10 * 4 + 8 + 6 * 8 and _lib.BagsDensifyRule.seed.offset == 40
    assert C.sizeof(_lib.BagsDensifyGroup) == 6 * 8 + 2 * 4 and _lib.BagsDensifyGroup.width.offset == 48


def _rule(addr, **kw):
    f = dict(P=10, N=2, max_grad=2e-4, min_opacity=0.005, dense_threshold=0.05, world_threshold=0.5, max_screen_size=20.0, use_screen_size=1,
             screen_size_mode=0, reserved=0, seed=1, noise=None, xyz_gradient_accum=addr, denom=addr, max_radii2D=addr, scaling=addr, opacity=addr)
    f.update(kw)
    return _lib.BagsDensifyRule(**f)


def _groups(addr, **kw):
    roles = ((3, _lib.ROLE_XYZ), (3, _lib.ROLE_OTHER), (45, _lib.ROLE_OTHER), (1, _lib.ROLE_OPACITY), (3, _lib.ROLE_SCALING), (4, _lib.ROLE_ROTATION))
    return (_lib.BagsDensifyGroup * 6)(*[_lib.BagsDensifyGroup(addr, addr, addr, addr, addr, addr, w, r) for w, r in roles])


def test_argument_validation(lib):
    """Every case returns before any GPU call: host addresses are fine, validation never dereferences them."""
    buf = (C.c_char * 4096)()
    addr = (C.addressof(buf) + 15) & ~15
    big = 1 << 40
    counts = (C.c_int64 * _lib.DENSIFY_COUNTS)()

    def plan_refused(rule, text, ws=addr, ws_bytes=big, out=counts, code=-1):
        rc = lib.bags_densify_plan(None if rule is None else C.byref(rule), ws, ws_bytes, out, None)
        msg = lib.bags_last_error()
        assert rc == code and text in msg, (rc, msg)
    plan_refused(None, b"null rule")
    plan_refused(_rule(addr, P=-1), b"P < 0")
    plan_refused(_rule(addr, N=0), b"N 0")
    plan_refused(_rule(addr, N=17), b"N 17")
    plan_refused(_rule(addr, screen_size_mode=2), b"screen_size_mode")
    plan_refused(_rule(addr, use_screen_size=2), b"use_screen_size")
    plan_refused(_rule(addr, max_grad=float("nan")), b"max_grad")
    plan_refused(_rule(addr, max_screen_size=float("nan")), b"max_screen_size")
    for hole in ("xyz_gradient_accum", "denom", "max_radii2D", "scaling", "opacity"):
        plan_refused(_rule(addr, **{hole: None}), b"NULL " + hole.encode())
    plan_refused(_rule(addr), b"NULL workspace", ws=None)
    plan_refused(_rule(addr), b"workspace 16 bytes", ws_bytes=16, code=-3)
    plan_refused(_rule(addr), b"NULL host_counts", out=None)

    def apply_refused(text, rule=None, groups=None, n_groups=6, P_new=12, outs=(addr, addr, addr), prov=addr, edit=None):
        g = _groups(addr) if groups is None else groups
        if edit is not None:
            edit(g)
        rc = lib.bags_densify_apply(C.byref(_rule(addr) if rule is None else rule), g, n_groups, addr, big, P_new, *outs, prov, None)
        msg = lib.bags_last_error()
        assert rc == -1 and text in msg, (rc, msg)
    apply_refused(b"N 0", rule=_rule(addr, N=0))
    apply_refused(b"n_groups", n_groups=0)
    apply_refused(b"n_groups", n_groups=9)
    apply_refused(b"P_new", P_new=-1)
    apply_refused(b"P_new", P_new=21)                                     # more than P * max(2, N)
    apply_refused(b"width", edit=lambda g: setattr(g[1], "width", 0))
    apply_refused(b"role", edit=lambda g: setattr(g[1], "role", 7))
    apply_refused(b"width 4, but its role", edit=lambda g: setattr(g[0], "width", 4))
    apply_refused(b"given together or not at all", edit=lambda g: setattr(g[2], "exp_avg_sq_out", None))
    apply_refused(b"NULL param / param_out", edit=lambda g: setattr(g[3], "param_out", None))
    apply_refused(b"not 16-byte aligned", edit=lambda g: setattr(g[3], "exp_avg_out", addr + 4))
    apply_refused(b"each be given once", edit=lambda g: setattr(g[5], "role", _lib.ROLE_OTHER), groups=None)
    apply_refused(b"each be given once", n_groups=5)                       # no rotation group
    apply_refused(b"max_radii2D_out", outs=(addr, addr, None))
    apply_refused(b"not 16-byte aligned", outs=(addr, addr + 8, addr))
    apply_refused(b"NULL provenance", prov=None)
    assert lib.bags_reset_opacity(addr, addr, addr, -1, None) == -1 and b"P < 0" in lib.bags_last_error()
    assert lib.bags_reset_opacity(None, addr, addr, 5, None) == -1 and b"NULL opacity" in lib.bags_last_error()


def test_empty_set_is_a_noop_without_a_device(lib):
    counts = (C.c_int64 * _lib.DENSIFY_COUNTS)(*([7] * _lib.DENSIFY_COUNTS))
    rule = _rule(None, P=0)
    assert lib.bags_densify_plan(C.byref(rule), None, 0, counts, None) == 0
    assert list(counts) == [0] * _lib.DENSIFY_COUNTS
    g = (_lib.BagsDensifyGroup * 6)(*[_lib.BagsDensifyGroup(None, None, None, None, None, None, w, r) for w, r in
                                      ((3, 1), (3, 0), (45, 0), (1, 4), (3, 2), (4, 3))])
    assert lib.bags_densify_apply(C.byref(rule), g, 6, None, 0, 0, None, None, None, None, None) == 0
    assert lib.bags_reset_opacity(None, None, None, 0, None) == 0


def _bag_of(opt, stats):
    bag = GaussianBag(3)
    p = D.params(opt)
    bag._xyz, bag._features_dc, bag._features_rest = p["xyz"], p["f_dc"], p["f_rest"]
    bag._opacity, bag._scaling, bag._rotation = p["opacity"], p["scaling"], p["rotation"]
    bag.xyz_gradient_accum, bag.denom, bag.max_radii2D = stats["xyz_gradient_accum"], stats["denom"], stats["max_radii2D"]
    return bag


def test_cpu_tensors_and_foreign_optimizers_raise():
    opt, stats, _ = D.make_case(7, seed=1)
    bag = _bag_of(opt, stats)
    before = [p.detach().clone() for p in bag.leaves()]
    with pytest.raises(RuntimeError, match="runs only on an AMD GPU.*no CPU\\s+fallback"):        # no silent CPU fallback
        bag.densify_and_prune(opt, **D.RULE)
    with pytest.raises(RuntimeError, match="runs only on an AMD GPU"):
        bag.reset_opacity(opt)
    assert all(torch.equal(a, b) for a, b in zip(before, bag.leaves()))
    with pytest.raises(ValueError, match="screen_size"):
        bag.densify_and_prune(opt, screen_size="sensible", **D.RULE)
    with pytest.raises(ValueError, match="N must be"):
        bag.densify_and_prune(opt, N=0, **D.RULE)
    other, _, _ = D.make_case(7, seed=1)
    with pytest.raises(RuntimeError, match="is not this bag's"):
        bag.densify_and_prune(other, **D.RULE)
    unnamed = torch.optim.Adam([{"params": [p]} for p in bag.leaves()], lr=0.0)
    with pytest.raises(RuntimeError, match="no parameter group named 'xyz'"):
        bag.densify_and_prune(unnamed, **D.RULE)
    with pytest.raises(RuntimeError, match="group named 'opacity'"):
        bag.reset_opacity(unnamed)


# ---------------------------------------------------------------------------------------------------------------- the restatement
#        mean grad  max scale  opacity  radius     fate under RULE (max_grad 2e-4, thr 0.05, 0.1 extent = 0.5, min_opacity 0.005, screen 20)
HAND = ((0.0,      0.02,      0.5,     5),       # 0  never seen (0 / 0): kept
        (1e-3,     0.02,      0.5,     5),       # 1  clone: kept + copy
        (1e-3,     0.10,      0.5,     5),       # 2  split: two children of scale 0.0625
        (5e-5,     0.02,      0.001,   5),       # 3  transparent: pruned
        (1e-3,     0.02,      0.001,   5),       # 4  clone, transparent: the row and its copy pruned
        (1e-3,     0.10,      0.001,   5),       # 5  split, transparent: both children pruned
        (1e-5,     0.70,      0.5,     5),       # 6  larger than 0.1 extent: pruned (kept when max_screen_size is None)
        (1e-3,     1.20,      0.5,     5),       # 7  split, children of scale 0.75 still too large: pruned (kept with None)
        (1e-3,     0.60,      0.5,     5),       # 8  split, children of scale 0.375: kept although the parent was too large
        (0.0,      0.02,      0.5,     50),      # 9  big on screen: kept as published (radii zeroed first), pruned with pre_densify
        (1e-3,     0.02,      0.5,     50))      # 10 clone, big on screen: as published both stay; pre_densify prunes the original only
EXPECT = {
    ("published", True): dict(kept=4, clones=3, split=4, pruned=8, prov=[(0, 0), (1, 0), (9, 0), (10, 0), (1, 1), (10, 1), (2, 2), (8, 2), (2, 3), (8, 3)]),
    ("pre_densify", True): dict(kept=2, clones=3, split=4, pruned=10, prov=[(0, 0), (1, 0), (1, 1), (10, 1), (2, 2), (8, 2), (2, 3), (8, 3)]),
    ("published", False): dict(kept=5, clones=3, split=4, pruned=5, prov=[(0, 0), (1, 0), (6, 0), (9, 0), (10, 0), (1, 1), (10, 1), (2, 2), (7, 2), (8, 2),
                                                                          (2, 3), (7, 3), (8, 3)]),
}


def _hand_case(dtype):
    P = len(HAND)
    g = torch.Generator().manual_seed(5)
    t = torch.tensor(HAND, dtype=torch.float64)
    scales = t[:, 1:2] * torch.tensor([[1.0, 0.5, 0.25]], dtype=torch.float64)
    denom = torch.full((P, 1), 4.0)
    denom[t[:, 0] == 0] = 0.0
    tensors = {"xyz": torch.randn(P, 3, generator=g), "f_dc": torch.randn(P, 1, 3, generator=g), "f_rest": torch.randn(P, 15, 3, generator=g),
               "opacity": torch.log(t[:, 2:3] / (1 - t[:, 2:3])).float(), "scaling": torch.log(scales).float(),
               "rotation": torch.tensor([[1.0, 0.0, 0.0, 0.0]]).repeat(P, 1)}
    tensors["rotation"][8] = torch.tensor([0.0, 0.0, 0.0, 2.0])               # half a turn about z, unnormalised: (x, y, z) -> (-x, -y, z)
    states = [dict(param=tensors[n], grad=None, exp_avg=torch.randn(tensors[n].shape, generator=g), exp_avg_sq=torch.rand(tensors[n].shape, generator=g))
              for n in R.NAMES]
    opt, _ = R.build(torch.optim.Adam, states, "cpu", dtype, step=7)
    stats = {"xyz_gradient_accum": (t[:, 0:1] * 4.0).float(), "denom": denom, "max_radii2D": t[:, 3].float()}
    noise = torch.randn(P, 2, 3, generator=g)
    return opt, stats, noise, states


@pytest.mark.parametrize("dtype", [torch.float32, torch.float64])
@pytest.mark.parametrize("mode,screen", list(EXPECT))
def test_restatement_on_a_hand_written_scene(dtype, mode, screen):
    opt, stats, noise, states = _hand_case(dtype)
    rule = dict(D.RULE, max_screen_size=D.RULE["max_screen_size"] if screen else None)
    out = D.densify_and_prune(opt, stats, noise=noise, screen_size=mode, **rule)
    want = EXPECT[(mode, screen)]
    assert {k: out[k] for k in ("kept", "clones", "split", "pruned")} == {k: want[k] for k in ("kept", "clones", "split", "pruned")}
    assert out["provenance"].tolist() == [list(x) for x in want["prov"]] and out["P_new"] == len(want["prov"])
    assert out["P_new"] == len(HAND) + out["clones"] + out["split"] - out["pruned"]            # N = 2
    assert out["margin"] > 0.2                                                              # the scene is nowhere near a threshold
    p = D.params(opt)
    src, kind = out["provenance"][:, 0], out["provenance"][:, 1]
    for n, s in zip(R.NAMES, states):
        q, st = p[n], opt.state[p[n]]
        assert q.shape[0] == out["P_new"] and q.is_leaf and q.requires_grad and float(st["step"]) == 7.0
        old = kind == D.KEPT
        assert torch.equal(st["exp_avg"][old], s["exp_avg"].to(dtype)[src[old]]) and torch.equal(st["exp_avg_sq"][old], s["exp_avg_sq"].to(dtype)[src[old]])
        assert st["exp_avg"][~old].abs().max() == 0 and st["exp_avg_sq"][~old].abs().max() == 0
        copied = (kind < D.CHILD) if n in ("xyz", "scaling") else torch.ones_like(old)
        assert torch.equal(q.detach()[copied], s["param"].to(dtype)[src[copied]]), n
    for v in out["stats"].values():
        assert v.shape[0] == out["P_new"] and v.abs().max() == 0
    # the children by hand: identity rotation (row 2) and half a turn about z (row 8)
    tol = 1e-6 if dtype == torch.float32 else 1e-12
    xyz0, sc0 = states[0]["param"].to(dtype), torch.exp(states[4]["param"].to(dtype))
    for i in range(out["P_new"]):
        s, k = int(src[i]), int(kind[i]) - D.CHILD
        if k < 0:
            continue
        d = sc0[s] * noise[s, k].to(dtype)
        if s == 8:
            d = d * torch.tensor([-1.0, -1.0, 1.0], dtype=dtype)
        assert torch.allclose(p["xyz"][i].detach(), xyz0[s] + d, rtol=0, atol=tol * 10), (s, k)
        assert torch.allclose(p["scaling"][i].detach(), torch.log(sc0[s] / 1.6), rtol=0, atol=tol * 10), (s, k)


def test_restatement_resets_opacity():
    opt, _, _, states = _hand_case(torch.float64)
    new = D.reset_opacity(opt)
    o = torch.sigmoid(states[3]["param"].double())
    assert torch.allclose(torch.sigmoid(new.detach()), torch.clamp(o, max=0.01), rtol=1e-12)
    st = opt.state[new]
    assert st["exp_avg"].abs().max() == 0 and st["exp_avg_sq"].abs().max() == 0 and float(st["step"]) == 7.0
    assert D.params(opt)["opacity"] is new and new.is_leaf and new.requires_grad


@pytest.mark.parametrize("P", SIZES)
def test_generated_inputs_populate_every_class_and_avoid_the_thresholds(P):
    """The two conditions tests/test_densify_gpu.py asserts again on the state it really uses (the Adam steps there run on the
    GPU): each of kept / clone / split / pruned holds at least 5 % of the rows (P >= 63), and on the fp64 restatement no tested
    value lies within 1e-4 relative of its threshold -- so fp32 and fp64 agree on every decision and the GPU comparison needs no
    exclusion."""
    for mode, N in (("published", 2), ("pre_densify", 2), ("published", 3)):
        if P == 500_000 and (mode, N) != ("published", 2):
            continue
        opt, stats, noise = D.make_case(P, seed=P)
        o32, o64 = D.clone_optimizer(opt), D.clone_optimizer(opt, dtype=torch.float64)
        a = D.densify_and_prune(o32, stats, noise=noise[:, :N], N=N, screen_size=mode, **D.RULE)
        b = D.densify_and_prune(o64, stats, noise=noise[:, :N], N=N, screen_size=mode, **D.RULE)
        assert b["margin"] > 1e-4, (mode, N, b["margin"])
        assert torch.equal(a["provenance"], b["provenance"])
        assert all(a[k] == b[k] for k in ("kept", "clones", "split", "pruned", "P_new"))
        if P >= 63:
            for k in ("kept", "clones", "split", "pruned"):
                assert b[k] >= math.ceil(0.05 * P), (mode, N, k, b[k])
