"""No-GPU checks of the MCMC strategy (csrc/mcmc.hip): ``compute_relocation_torch`` against closed forms, the C ABI surface and its
argument validation (reported before anything is enqueued), the wrappers' refusals, the plain-PyTorch restatement the GPU tests
compare against, and the generator of the GPU tests' inputs."""
import ctypes as C
import math
import os
import re

import pytest
import torch

import adam_reference as R
import densify_reference as D
import mcmc_reference as M
from bags_raster import _lib, compute_relocation, compute_relocation_torch, relocation_binoms
from bags_raster.gaussians import GaussianBag

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FUNCS = ("bags_compute_relocation", "bags_mcmc_workspace_size", "bags_mcmc_relocate", "bags_mcmc_add_new", "bags_mcmc_noise")
LEAF = {"xyz": "_xyz", "f_dc": "_features_dc", "f_rest": "_features_rest", "opacity": "_opacity", "scaling": "_scaling", "rotation": "_rotation"}
SIZES = (1, 63, 64, 65, 1000)                     # every P of tests/test_mcmc_gpu.py's compute_relocation cases


@pytest.fixture(scope="module")
def lib():
    if not os.path.exists(_lib.LIB_PATH):
        import __graft_entry__ as g
        g.build()
    return _lib.load()


# ---------------------------------------------------------------------------------------------------------------- compute_relocation
def test_one_copy_is_the_identity():
    g = torch.Generator().manual_seed(1)
    o = 0.005 + 0.985 * torch.rand(200, generator=g, dtype=torch.float64)
    s = torch.rand(200, 3, generator=g, dtype=torch.float64)
    for N in (torch.ones(200, dtype=torch.int32), torch.zeros(200, dtype=torch.int64), torch.full((200,), -3)):      # 0 and below clamp to 1
        before = N.clone()
        o_new, s_new = compute_relocation_torch(o, s, N, relocation_binoms(), 51)
        assert torch.equal(N, before)                                                # the caller's N is not modified
        # 1 - (1 - o) loses up to 2^-53 absolute, 2^-53 / 0.005 relative: that is the coefficient's error too
        assert (o_new - o).abs().max().item() <= 2.0 ** -52 and ((s_new - s).abs() / s).max().item() <= 4 * 2.0 ** -52 / 0.005


def test_two_copies_match_the_closed_form():
    """N = 2: o' = 1 - sqrt(1 - o), denom = C(0,0) o' + C(1,0) o' - C(1,1) o'^2 / sqrt(2)."""
    g = torch.Generator().manual_seed(2)
    o = 0.005 + 0.985 * torch.rand(200, generator=g, dtype=torch.float64)
    s = torch.rand(200, 3, generator=g, dtype=torch.float64)
    o_new, s_new = compute_relocation_torch(o.reshape(-1, 1), s, torch.full((200,), 2), relocation_binoms(), 51)
    assert o_new.shape == (200, 1)
    want_o = 1 - torch.sqrt(1 - o)
    want_s = (o / (2 * want_o - want_o ** 2 / math.sqrt(2))).unsqueeze(-1) * s
    assert (o_new[:, 0] - want_o).abs().max().item() <= 1e-15 and ((s_new - want_s).abs() / want_s).max().item() <= 1e-12      # (1e-15 / o')
    # two half-opaque copies side by side are each more transparent and narrower than the original
    assert (o_new[:, 0] < o).all() and (s_new < s).all()


def test_double_loop_and_hockey_stick_forms_agree():
    """In float64 with the exact binomials (all below 2^53) the two forms differ by the rounding of at most 1275 terms; the terms
    are bounded by C(n, k+1) o'^(k+1) <= (n o')^(k+1) / (k+1)! <= e^(-ln(1 - o)) = 100 at o = 0.99 against a sum of order o' n,
    so 1e-11 relative holds with two orders to spare."""
    exact = torch.tensor([[float(math.comb(n, k)) if k <= n else 0.0 for k in range(51)] for n in range(51)], dtype=torch.float64)
    assert torch.equal(exact.float(), relocation_binoms()) and relocation_binoms().dtype == torch.float32
    worst = 0.0
    for o0 in (0.005, 0.1, 0.5, 0.9, 0.99):
        N = torch.arange(1, 51)
        o = torch.full((50,), o0, dtype=torch.float64)
        s = torch.ones(50, 3, dtype=torch.float64)
        a = compute_relocation_torch(o, s, N, exact, 51)
        b = M.compute_relocation_hockey(o, s, N)
        assert torch.equal(a[0], b[0])
        worst = max(worst, M.rel_err(a[1], b[1]))
    print(f"MCMC forms: worst relative difference {worst:.3e}")
    assert worst <= 1e-11


@pytest.mark.parametrize("P", SIZES)
def test_generated_inputs_keep_the_fp32_statement_within_reach(P):
    """What tests/test_mcmc_gpu.py relies on: with opacities in (0.005, 0.99) the float32 statement is within 1e-3 relative of
    float64 on at least 90 % of the rows with N > 8 (in fact on all), and every N of 1..50 and 0, 51, 1000 occurs for P >= 53."""
    o, s, N = M.relocation_inputs(P, P)
    assert 0.005 < o.min() and o.max() < 0.99 and N.dtype == torch.int32
    if P >= 53:
        assert set(N.tolist()) == set(range(0, 52)) | {1000}
    a, b = M.compute_relocation(o, s, N), M.compute_relocation(o.double(), s.double(), N)
    rel = torch.maximum(((a[1].double() - b[1]).abs() / b[1].abs()).max(dim=1).values, (a[0].double() - b[0]).abs() / b[0].abs())
    big = N.clamp(1, 50) > 8
    if big.any():
        assert (rel[big] < 1e-3).float().mean().item() >= 0.9


# ---------------------------------------------------------------------------------------------------------------- the C ABI
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
    assert lib.bags_abi_version() == 11 == _lib.ABI_VERSION and "#define BAGS_ABI_VERSION 11" in header          # additive: no bump
    assert "#define BAGS_MCMC_MAX_BINOMS %d" % _lib.MCMC_MAX_BINOMS in header and _lib.MCMC_MAX_BINOMS == 51
    assert [f[0] for f in _lib.BagsMcmcGroup._fields_] == _header_struct_fields("BagsMcmcGroup")
    assert C.sizeof(_lib.BagsMcmcGroup) == 6 * 8 + 2 * 4 and _lib.BagsMcmcGroup.width.offset == 48
    assert all(callable(getattr(GaussianBag, n)) for n in ("relocate", "add_new", "mcmc_noise"))
    assert lib.bags_mcmc_workspace_size(500_000) >= 500_000 * 20
    assert lib.bags_mcmc_workspace_size(1000) < lib.bags_mcmc_workspace_size(100_000)


def _groups(addr, **kw):
    roles = ((3, _lib.ROLE_XYZ), (3, _lib.ROLE_OTHER), (45, _lib.ROLE_OTHER), (1, _lib.ROLE_OPACITY), (3, _lib.ROLE_SCALING), (4, _lib.ROLE_ROTATION))
    return (_lib.BagsMcmcGroup * 6)(*[_lib.BagsMcmcGroup(addr, addr, addr, addr, addr, addr, w, r) for w, r in roles])


def test_argument_validation(lib):
    """Every case returns before any GPU call: host addresses are fine, validation never dereferences them."""
    buf = (C.c_char * 4096)()
    addr = (C.addressof(buf) + 15) & ~15
    big = 1 << 40

    def refused(rc, text, code=-1):
        msg = lib.bags_last_error()
        assert rc == code and text in msg, (rc, msg)
    cr = lib.bags_compute_relocation
    refused(cr(addr, addr, addr, None, 51, 5, addr, addr, None), b"compute_relocation: NULL binoms")
    refused(cr(None, None, None, None, 51, 0, None, None, None), b"compute_relocation: NULL binoms")          # also when P == 0
    refused(cr(addr, addr, addr, addr, 1, 5, addr, addr, None), b"compute_relocation: n_max 1")
    refused(cr(None, None, None, addr, 52, 0, None, None, None), b"compute_relocation: n_max 52")
    refused(cr(addr, addr, addr, addr, 51, -1, addr, addr, None), b"compute_relocation: P < 0")
    refused(cr(None, addr, addr, addr, 51, 5, addr, addr, None), b"compute_relocation: NULL opacity_old")
    refused(cr(addr, addr, None, addr, 51, 5, addr, addr, None), b"compute_relocation: NULL opacity_old / scale_old / N")
    refused(cr(addr, addr, addr, addr, 51, 5, addr, None, None), b"compute_relocation: NULL opacity_new / scale_new")
    assert cr(None, None, None, addr, 51, 0, None, None, None) == 0                                           # then P == 0 is a no-op
    assert cr(None, None, None, addr, 2, 0, None, None, None) == 0

    def relocate(groups=None, n_groups=6, P=10, dead=addr, sampled=addr, D=3, binoms=addr, n_max=51, min_opacity=0.005, ws=addr, ws_bytes=big, edit=None):
        g = _groups(addr) if groups is None else groups
        if edit is not None:
            edit(g)
        return lib.bags_mcmc_relocate(g, n_groups, P, dead, sampled, D, binoms, n_max, min_opacity, ws, ws_bytes, None)

    def add_new(n_groups=6, P=10, sampled=addr, A=3, binoms=addr, n_max=51, min_opacity=0.005, ws=addr, ws_bytes=big, outs=(addr, addr, addr), edit=None):
        g = _groups(addr)
        if edit is not None:
            edit(g)
        return lib.bags_mcmc_add_new(g, n_groups, P, sampled, A, binoms, n_max, min_opacity, ws, ws_bytes, *outs, None)
    for fn, op in ((relocate, b"mcmc_relocate"), (add_new, b"mcmc_add_new")):
        refused(fn(binoms=None), op + b": NULL binoms")
        refused(fn(n_max=52), op + b": n_max 52")
        refused(fn(P=-1), op + b": P < 0")
        refused(fn(min_opacity=0.0), op + b": min_opacity")
        refused(fn(min_opacity=float("nan")), op + b": min_opacity")
        refused(fn(n_groups=0), op + b": n_groups")
        refused(fn(n_groups=9), op + b": n_groups")
        refused(fn(edit=lambda g: setattr(g[1], "width", 0)), b"width 0")
        refused(fn(edit=lambda g: setattr(g[1], "role", 7)), b"unknown role")
        refused(fn(edit=lambda g: setattr(g[3], "width", 2)), b"width 2, but its role")
        refused(fn(edit=lambda g: setattr(g[3], "role", _lib.ROLE_OTHER)), b"each be given once")
        refused(fn(n_groups=4), b"each be given once")                        # no scaling group
        refused(fn(edit=lambda g: setattr(g[2], "param", None)), b"NULL param")
        refused(fn(edit=lambda g: setattr(g[2], "exp_avg_sq", None)), b"together or not at all")
        refused(fn(sampled=None), op + b": NULL sampled")
        refused(fn(ws=None), op + b": NULL workspace")
        refused(fn(ws_bytes=16), b"workspace 16 bytes", code=-3)
    refused(relocate(D=-1), b"n_sampled < 0")
    refused(relocate(dead=None), b"mcmc_relocate: NULL dead")
    refused(add_new(edit=lambda g: setattr(g[0], "param_out", None)), b"NULL param_out")
    refused(add_new(edit=lambda g: setattr(g[0], "exp_avg_out", None)), b"exactly when the moments are")
    refused(add_new(edit=lambda g: setattr(g[0], "exp_avg_sq_out", addr + 4)), b"not 16-byte aligned")
    refused(add_new(outs=(addr, None, addr)), b"denom_out")
    refused(add_new(outs=(addr, addr, addr + 8)), b"not 16-byte aligned")
    refused(add_new(P=2 ** 31 - 2, A=5), b"rows (> 2^31 - 1)", code=-3)
    # nothing to do: no device is touched
    assert relocate(D=0, dead=None, sampled=None, ws=None, ws_bytes=0) == 0 and relocate(P=0, D=0, ws=None, ws_bytes=0) == 0
    assert add_new(A=0, sampled=None, ws=None, ws_bytes=0, outs=(None, None, None)) == 0
    nz = lib.bags_mcmc_noise
    refused(nz(addr, addr, addr, addr, -1, None, 0, 1.0, 100.0, 0.995, 1.0, None), b"mcmc_noise: P < 0")
    refused(nz(addr, addr, addr, addr, 5, None, 0, float("nan"), 100.0, 0.995, 1.0, None), b"mcmc_noise: scale")
    refused(nz(addr, None, addr, addr, 5, None, 0, 1.0, 100.0, 0.995, 1.0, None), b"mcmc_noise: NULL xyz / opacity")
    assert nz(None, None, None, None, 0, None, 0, 1.0, 100.0, 0.995, 1.0, None) == 0


# ---------------------------------------------------------------------------------------------------------------- the wrappers
def _bag_of(opt, stats, sh_degree=3):
    bag = GaussianBag(sh_degree)
    for n, q in D.params(opt).items():
        setattr(bag, LEAF[n], q)
    bag.xyz_gradient_accum, bag.denom, bag.max_radii2D = stats["xyz_gradient_accum"], stats["denom"], stats["max_radii2D"]
    return bag


def test_wrappers_refuse_what_they_cannot_run():
    """Wrong device, dtype, shape, a sampled row that is dead, foreign optimizer groups: all raised on the host, and nothing changed."""
    opt, stats = M.make_case(8, seed=1)
    bag = _bag_of(opt, stats)
    before = [p.detach().clone() for p in bag.leaves()]
    dead = torch.tensor([0, 1, 0, 0, 1, 0, 0, 0], dtype=torch.bool)
    gpu = "runs only on an AMD GPU.*no CPU\\s+fallback"
    with pytest.raises(RuntimeError, match=gpu):
        bag.relocate(opt, dead)
    with pytest.raises(RuntimeError, match=gpu):
        bag.relocate(opt, dead, sampled=torch.tensor([2, 2]))
    with pytest.raises(RuntimeError, match=gpu):
        bag.add_new(opt, 100)
    with pytest.raises(RuntimeError, match=gpu):
        bag.mcmc_noise(1e-3)
    with pytest.raises(TypeError, match="dead_mask must be bool"):
        bag.relocate(opt, dead.int())
    with pytest.raises(TypeError, match="dead_mask must be a tensor"):
        bag.relocate(opt, [False] * 8)
    with pytest.raises(RuntimeError, match=r"dead_mask must be \(8,\)"):
        bag.relocate(opt, dead[:7])
    with pytest.raises(ValueError, match="sampled lists a dead row"):
        bag.relocate(opt, dead, sampled=torch.tensor([2, 4]))
    with pytest.raises(RuntimeError, match="sampled must be a vector of 2 rows"):
        bag.relocate(opt, dead, sampled=torch.tensor([2, 3, 5]))
    with pytest.raises(TypeError, match="sampled must be int32 or int64"):
        bag.relocate(opt, dead, sampled=torch.tensor([2.0, 3.0]))
    with pytest.raises(IndexError, match="outside 0..7"):
        bag.relocate(opt, dead, sampled=torch.tensor([2, 8]))
    with pytest.raises(RuntimeError, match="sampled must be a vector of 0 rows"):
        bag.add_new(opt, 8, sampled=torch.tensor([1]))                               # cap_max = P: nothing to add
    other, _ = M.make_case(8, seed=1)
    for call in (lambda o: bag.relocate(o, dead), lambda o: bag.add_new(o, 100)):
        with pytest.raises(RuntimeError, match="is not this bag's"):
            call(other)
        with pytest.raises(RuntimeError, match="no parameter group named 'xyz'"):
            call(torch.optim.Adam([{"params": [p]} for p in bag.leaves()], lr=0.0))
    with pytest.raises(NotImplementedError, match="compute_relocation_torch"):
        compute_relocation(None, None, None, None, 51)
    o, s, N = M.relocation_inputs(5, 1)
    with pytest.raises(NotImplementedError, match="compute_relocation_torch"):       # CPU tensors: the PyTorch statement is named, not run
        compute_relocation(o, s, N, relocation_binoms(), 51)
    assert all(torch.equal(a, b) for a, b in zip(before, bag.leaves()))


# ---------------------------------------------------------------------------------------------------------------- the restatement
@pytest.mark.parametrize("dtype", [torch.float32, torch.float64])
def test_restatement_keeps_step_and_every_untouched_row(dtype):
    P = 40
    opt0, stats = M.make_case(P, seed=3)
    dead_mask = torch.zeros(P, dtype=torch.bool)
    dead_mask[[3, 7, 8, 20, 39]] = True
    sampled = torch.tensor([5, 5, 11, 5, 30])
    opt = D.clone_optimizer(opt0, dtype=dtype)
    out = M.relocate(opt, dead_mask, sampled)
    assert out == {"dead": 5, "sources": 3}
    p0, p = D.params(opt0), D.params(opt)
    touched = torch.zeros(P, dtype=torch.bool)
    touched[dead_mask.nonzero().reshape(-1)] = True
    touched[sampled] = True
    for n in R.NAMES:
        st0, st = opt0.state[p0[n]], opt.state[p[n]]
        assert float(st["step"]) == 5.0 == float(st0["step"])
        assert torch.equal(p[n].detach()[~touched], p0[n].detach().to(dtype)[~touched]), n
        for key in ("exp_avg", "exp_avg_sq"):
            assert st[key][sampled].abs().max() == 0                                 # the sources' moments: zero
            keep = torch.ones(P, dtype=torch.bool)
            keep[sampled] = False
            assert torch.equal(st[key][keep], st0[key].to(dtype)[keep]), (n, key)    # everyone else's, the dead rows' too: as they were
        if n not in ("opacity", "scaling"):
            assert torch.equal(p[n].detach()[dead_mask], p0[n].detach().to(dtype)[sampled]), n
            assert torch.equal(p[n].detach()[sampled], p0[n].detach().to(dtype)[sampled]), n
        else:
            assert torch.equal(p[n].detach()[dead_mask], p[n].detach()[sampled]), n
    # row 5 was drawn three times: four copies, each more transparent than the original
    assert torch.sigmoid(p["opacity"].detach()[5]) < torch.sigmoid(p0["opacity"].detach()[5])
    assert M.relocate(opt, torch.zeros(P, dtype=torch.bool), torch.zeros(0, dtype=torch.long)) == {"dead": 0, "sources": 0}
    assert M.relocate(opt, torch.ones(P, dtype=torch.bool), torch.zeros(P, dtype=torch.long)) == {"dead": P, "sources": 0}

    opt = D.clone_optimizer(opt0, dtype=dtype)
    assert M.add_new(opt, P, None)["added"] == 0 and M.add_new(opt, 10, None)["added"] == 0
    src = torch.tensor([5, 5])
    out = M.add_new(opt, 1000, src)                                                  # int(1.05 * 40) = 42
    assert (out["added"], out["P_new"]) == (2, 42) and all(v.shape[0] == 42 and v.abs().max() == 0 for v in out["stats"].values())
    p = D.params(opt)
    rest = torch.ones(P, dtype=torch.bool)
    rest[5] = False
    for n in R.NAMES:
        st0, st = opt0.state[p0[n]], opt.state[p[n]]
        assert p[n].shape[0] == 42 and p[n].is_leaf and p[n].requires_grad and float(st["step"]) == 5.0
        assert torch.equal(p[n].detach()[:P][rest], p0[n].detach().to(dtype)[rest]), n
        assert torch.equal(p[n].detach()[P:], p[n].detach()[src]), n
        for key in ("exp_avg", "exp_avg_sq"):
            assert torch.equal(st[key][:P][rest], st0[key].to(dtype)[rest]) and st[key][P:].abs().max() == 0 and st[key][5].abs().max() == 0


def test_restated_noise_step_by_hand():
    """Identity rotation, scales (1, 2, 3), open gate: the step is (1, 4, 9) * z * g * scale; an opaque row stays where it is."""
    xyz = torch.zeros(2, 3, dtype=torch.float64)
    opacity = torch.tensor([[-20.0], [20.0]], dtype=torch.float64)
    scaling = torch.log(torch.tensor([[1.0, 2.0, 3.0]] * 2, dtype=torch.float64))
    rotation = torch.tensor([[2.0, 0.0, 0.0, 0.0]] * 2, dtype=torch.float64)
    z = torch.tensor([[1.0, -1.0, 0.5]] * 2, dtype=torch.float64)
    out = M.mcmc_noise(xyz, opacity, scaling, rotation, 0.1, z)
    g = 1 / (1 + math.exp(-100 * (1 - 1 / (1 + math.exp(20.0)) - 0.995)))
    assert torch.allclose(out[0], torch.tensor([1.0, -4.0, 4.5], dtype=torch.float64) * g * 0.1, rtol=1e-12)
    assert 0.62 < g < 0.63 and out[1].abs().max().item() < 1e-40
