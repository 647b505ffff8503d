"""No-GPU checks of the fused optimizer step: the C ABI surface and its argument validation (reported before anything is enqueued),
the GaussianAdam class as a torch.optim.Optimizer, and the float64 reference the GPU tests compare against."""
import ctypes as C
import os
import re

import pytest
import torch

import adam_reference as R
from bags_raster.optim import GaussianAdam  # noqa: F401  (the feature under test: without it nothing here can pass)
from bags_raster import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


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


def test_symbol_is_declared_bound_and_exported(lib):
    import bags_raster
    header = open(os.path.join(ROOT, "include", "bags_raster.h")).read()
    assert re.search(r"\bint\s+bags_adam_step\s*\(", header)
    assert "bags_adam_step" in _lib.SYMBOLS and hasattr(lib, "bags_adam_step")
    assert lib.bags_abi_version() == 11 and "#define BAGS_ABI_VERSION 11" in header          # additive: no bump
    assert "#define BAGS_ADAM_MAX_GROUPS %d" % _lib.ADAM_MAX_GROUPS in header
    assert "GaussianAdam" in bags_raster.__all__ and bags_raster.GaussianAdam is bags_raster.optim.GaussianAdam


def test_struct_layout_matches_header():
    for cls in (_lib.BagsAdamGroup, _lib.BagsAdamArgs, _lib.BagsDensifyStats):
        assert [f[0] for f in cls._fields_] == _header_struct_fields(cls.__name__), cls.__name__
    assert C.sizeof(_lib.BagsAdamGroup) == 4 * 8 + 2 * 4 + 2 * 4
    assert C.sizeof(_lib.BagsAdamArgs) == 2 * 4 + 3 * 8 + 8 + 8 * C.sizeof(_lib.BagsAdamGroup)
    assert C.sizeof(_lib.BagsDensifyStats) == 2 * 8 + 2 * 4 + 3 * 8
    assert _lib.BagsAdamArgs.groups.offset == 40 and _lib.BagsAdamGroup.step_size.offset == 40


def _args(addr, P=10, n_groups=1, width=3):
    grp = _lib.BagsAdamGroup(addr, addr, addr, addr, width, 0, 1e-3, 1.0)
    return _lib.BagsAdamArgs(P, n_groups, 0.9, 0.999, 1e-15, None, (_lib.BagsAdamGroup * _lib.ADAM_MAX_GROUPS)(*([grp] * 8)))


def test_argument_validation(lib):
    """Every case returns before any GPU call: host addresses are fine, validation never dereferences them."""
    buf = (C.c_char * 4096)()
    addr = C.addressof(buf)

    def refused(args, stats, text):
        rc = lib.bags_adam_step(C.byref(args), None if stats is None else C.byref(stats), None)
        msg = lib.bags_last_error()
        assert rc == -1 and text in msg, (rc, msg)
    refused(_args(addr, P=-1), None, b"P < 0")
    refused(_args(addr, n_groups=0), None, b"n_groups")
    refused(_args(addr, n_groups=9), None, b"n_groups")
    refused(_args(addr, width=0), None, b"width")
    refused(_args(addr, width=-3), None, b"width")
    for hole in ("param", "exp_avg", "exp_avg_sq"):
        a = _args(addr, n_groups=2)
        setattr(a.groups[1], hole, None)
        refused(a, None, b"NULL param / exp_avg / exp_avg_sq")
    full = dict(radii=addr, grad_means2D=addr, grad_stride=3, xyz_gradient_accum=addr, denom=addr, max_radii2D=addr)
    for hole in ("radii", "grad_means2D", "xyz_gradient_accum", "denom", "max_radii2D"):
        refused(_args(addr), _lib.BagsDensifyStats(**{**full, hole: None}), b"stats")
    refused(_args(addr), _lib.BagsDensifyStats(**{**full, "grad_stride": 1}), b"grad_stride")
    assert lib.bags_adam_step(None, None, None) == -1 and b"null struct" in lib.bags_last_error()


def test_empty_step_is_a_noop_without_a_device(lib):
    buf = (C.c_char * 64)()
    addr = C.addressof(buf)
    assert lib.bags_adam_step(C.byref(_args(addr, P=0)), None, None) == 0
    assert lib.bags_adam_step(C.byref(_args(addr, P=0)), C.byref(_lib.BagsDensifyStats()), None) == 0     # all-NULL stats block = off
    # a group without a gradient may leave its other pointers NULL too
    a = _args(addr, P=0)
    a.groups[0] = _lib.BagsAdamGroup(None, None, None, None, 3, 0, 0.0, 1.0)
    assert lib.bags_adam_step(C.byref(a), None, None) == 0


def test_is_an_optimizer_with_torch_adams_state_dict():
    from bags_raster import GaussianAdam
    states = R.random_state(7, seed=3)
    adam, p_adam = R.build(torch.optim.Adam, states, "cpu", torch.float32, step=0)
    for _ in range(3):
        adam.step()
    ours = GaussianAdam(R.param_groups([torch.nn.Parameter(torch.zeros_like(p)) for p in p_adam]), lr=0.0, eps=1e-15)
    assert isinstance(ours, torch.optim.Optimizer)
    assert [g["name"] for g in ours.param_groups] == list(R.NAMES)
    fresh_keys = set(ours.state_dict()["param_groups"][0])
    assert fresh_keys == set(adam.state_dict()["param_groups"][0])            # a fresh one already carries torch.optim.Adam's keys
    ours.load_state_dict(adam.state_dict())
    a, b = adam.state_dict(), ours.state_dict()
    assert a["param_groups"] == b["param_groups"]
    assert a["state"].keys() == b["state"].keys()
    for k in a["state"]:
        assert a["state"][k].keys() == b["state"][k].keys() == {"step", "exp_avg", "exp_avg_sq"}
        for name in a["state"][k]:
            assert torch.equal(a["state"][k][name], b["state"][k][name]), (k, name)
        assert not b["state"][k]["step"].is_cuda and b["state"][k]["step"].item() == 3.0
    # ... and back: torch.optim.Adam takes a GaussianAdam state dict
    back, _ = R.build(torch.optim.Adam, states, "cpu", torch.float32, step=0)
    back.load_state_dict(ours.state_dict())
    assert all(torch.equal(back.state_dict()["state"][k]["exp_avg_sq"], a["state"][k]["exp_avg_sq"]) for k in a["state"])


def test_unsupported_hyperparameters_and_cpu_tensors_raise():
    from bags_raster import GaussianAdam
    p = torch.nn.Parameter(torch.zeros(4, 3))
    for kw in (dict(amsgrad=True), dict(weight_decay=0.01), dict(maximize=True), dict(capturable=True), dict(differentiable=True)):
        with pytest.raises(RuntimeError, match="not supported"):
            GaussianAdam([p], **kw)
    with pytest.raises(RuntimeError, match="not supported"):
        GaussianAdam([{"params": [p], "amsgrad": True}])
    opt = GaussianAdam([{"params": [p], "lr": 1e-3, "name": "xyz"}], lr=0.0, eps=1e-15)
    opt.step()                                                   # no gradient anywhere: nothing to do, as torch.optim.Adam
    assert len(opt.state) == 0
    p.grad = torch.ones_like(p)
    with pytest.raises(RuntimeError, match="runs only on an AMD GPU"):      # no silent CPU fallback
        opt.step()
    opt.param_groups[0]["amsgrad"] = True                         # e.g. arrived with a loaded state dict
    with pytest.raises(RuntimeError, match="amsgrad"):
        opt.step()


@pytest.mark.parametrize("step", [1, 2, 1000])
def test_reference_helper_equals_float64_adam(step):
    states = R.random_state(101, seed=step)
    states[2]["grad"] = None                                      # a group without a gradient: skipped, its step does not advance
    visible = torch.rand(101, generator=torch.Generator().manual_seed(9)) < 0.4
    for vis in (None, visible):
        ref = R.torch_adam_step(states, step, torch.float64, visible=vis)
        formula = R.closed_form_step64(states, step, visible=vis)
        for i, (a, b) in enumerate(zip(ref, formula)):
            assert a[3] == b[3], (i, a[3], b[3])
            for name, x, y in zip(R.KEYS, a, b):
                assert torch.allclose(x, y, rtol=1e-13, atol=1e-300), (i, name, (x - y).abs().max())
        assert torch.equal(ref[2][0], states[2]["param"].double()) and ref[2][3] == step - 1
        if vis is not None:
            dense = R.torch_adam_step(states, step, torch.float64)
            for i in (0, 3, 5):
                assert torch.equal(ref[i][0][~vis], states[i]["param"].double()[~vis])
                assert torch.equal(ref[i][2][~vis], states[i]["exp_avg_sq"].double()[~vis])
                assert torch.equal(ref[i][0][vis], dense[i][0][vis]) and not torch.equal(ref[i][0][vis], states[i]["param"].double()[vis])
    # the error measure: zero for the reference itself; half an ulp of 1.0 over (|ref| + mean |ref|) = 2 is 0.25
    x = torch.full((1000,), 1.0 + 2.0 ** -24, dtype=torch.float64)
    assert R.err(x, x) == 0.0
    assert abs(R.err(x.float(), x) - 0.25) < 1e-6
    assert not R.err(torch.full((3,), float("nan")), torch.ones(3, dtype=torch.float64)) <= 1e30
