"""No-GPU checks of the lens network: the flat parameter layout against an explicit nn.Linear / nn.ELU stack, the boundary
(symbols, constants, size query, argument errors), lipschitz_correction, the fixed-point inverse in float64, and the inputs of the
bars of tests/test_lens_field_gpu.py (tests/lens_cases.py)."""
import ctypes as C
import math
import os
import re

import pytest
import torch

import bags_raster
import lens_cases as LC
from bags_raster import LensField, _lib, lens_field, lens_field_torch
from bags_raster.lens_field import block_floats, layer_views, lens_field_inverse_torch, param_count

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def lib():
    if not os.path.exists(_lib.LIB_PATH):
        import __graft_entry__ as g
        g.build()
    return _lib.load()


def _stack(linears):
    mods = []
    for lin in linears[:-1]:
        mods += [lin, torch.nn.ELU()]
    return torch.nn.Sequential(*mods, linears[-1])


@pytest.mark.parametrize("B,H,n", [(1, 1, 0), (2, 3, 1), (3, 33, 2), (2, 64, 4)])
def test_flat_layout_is_the_linear_elu_stack(B, H, n):
    net = LensField(B, H, n, seed=7).double()
    stacks = net.export_linear_stacks()
    assert len(stacks) == B and all(len(s) == n + 2 for s in stacks)
    assert [tuple(l.weight.shape) for l in stacks[0]] == [(H, 2)] + [(H, H)] * n + [(2, H)]
    # the order of the flat vector: W_0 b_0 (W_i b_i) x n W_out b_out, block after block, (out, in) row-major
    flat = torch.cat([t.reshape(-1) for s in stacks for l in s for t in (l.weight, l.bias)])
    assert torch.equal(flat, net.params.detach())
    x = torch.rand(37, 2, dtype=torch.float64, generator=torch.Generator().manual_seed(1)) * 3 - 1.5
    want = x
    with torch.no_grad():
        for s in stacks:
            want = want + _stack(s)(want)
        assert torch.equal(net(x), want)
        assert torch.equal(lens_field_torch(net.params, x.view(1, 37, 2), B, H, n), want.view(1, 37, 2))
    # ... and back in: another net loaded from the stacks is the same flat vector
    other = LensField(B, H, n, seed=8).double()
    assert not torch.equal(other.params, net.params)
    other.load_linear_stacks(stacks)
    assert torch.equal(other.params, net.params)
    with pytest.raises(ValueError, match="blocks given"):
        other.load_linear_stacks(stacks + stacks)


def test_module_surface():
    net = LensField(seed=0)
    assert (net.blocks, net.hidden, net.internal_layers) == (5, 64, 1)
    assert [n for n, _ in net.named_parameters()] == ["params"] and net.params.dtype == torch.float32
    assert torch.equal(LensField(seed=0).params, net.params) and not torch.equal(LensField(seed=1).params, net.params)
    layers = net.layers()
    assert len(layers) == 5 and all(len(b) == 3 for b in layers)
    layers[2][1][0][3, 4] = 5.0                                   # a view: writing it writes the parameter
    o = 2 * block_floats(64, 1) + 3 * 64
    assert float(net.params.detach()[o + 3 * 64 + 4]) == 5.0
    # nn.Linear's initial range, +-1 / sqrt(fan_in)
    fresh = LensField(2, 16, 1, seed=3)
    for W, b in fresh.layers()[0]:
        bound = 1.0 / math.sqrt(W.shape[1])
        assert float(W.abs().max()) <= bound and float(b.abs().max()) <= bound and float(W.abs().max()) > 0.5 * bound
    ident = LensField(3, 8, 2, seed=3, identity_init=True)
    x = torch.rand(4, 5, 2)
    assert torch.equal(ident(x), x)
    assert all(float(b[-1][0].abs().max()) == 0.0 and float(b[-1][1].abs().max()) == 0.0 and float(b[0][0].abs().max()) > 0 for b in ident.layers())


def test_parameter_count_and_workspace_size(lib):
    for B, H, n in [(1, 1, 0), (5, 64, 1), (3, 33, 2), (32, 64, 4)]:
        per = 3 * H + n * (H * H + H) + 2 * H + 2
        assert block_floats(H, n) == per and param_count(B, H, n) == B * per
        assert LensField(B, H, n, seed=0).params.numel() == B * per
    size = lib.bags_lens_field_workspace_size
    # the per-point part: at most the B block inputs, 8 bytes per point and block; the rest are the per-workgroup partial sums
    for B, H, n in [(1, 16, 1), (5, 64, 1), (32, 64, 4)]:
        per_point = (size(B, H, n, 1 << 20) - size(B, H, n, 1 << 19)) / float(1 << 19)
        assert per_point <= 8 * B + 1e-3, (B, H, n, per_point)
    assert 0 < size(5, 64, 1, 0) <= 1024
    assert size(5, 64, 1, 8160) >= 4 * 8160 * 8 + 4 * param_count(5, 64, 1)
    assert size(5, 64, 1, 100) <= size(5, 64, 1, 8160) <= size(5, 64, 1, 32400)
    assert size(5, 65, 1, 100) == 0 and size(5, 64, 5, 100) == 0 and size(33, 64, 1, 100) == 0 and size(5, 64, 1, -1) == 0


def test_symbols_constants_and_abi(lib):
    names = ["bags_lens_field_workspace_size", "bags_lens_field_forward", "bags_lens_field_backward", "bags_lens_field_inverse"]
    header = open(os.path.join(ROOT, "include", "bags_raster.h")).read()
    for name in names:
        assert name in _lib.SYMBOLS and hasattr(lib, name) and re.search(r"\b%s\s*\(" % name, header), name
    for macro, value in (("BAGS_LENS_MAX_HIDDEN", 64), ("BAGS_LENS_MAX_INTERNAL_LAYERS", 4), ("BAGS_LENS_MAX_BLOCKS", 32)):
        assert re.search(r"#define\s+%s\s+%d\b" % (macro, value), header), macro
    assert (_lib.LENS_MAX_HIDDEN, _lib.LENS_MAX_INTERNAL_LAYERS, _lib.LENS_MAX_BLOCKS) == (64, 4, 32)
    assert C.sizeof(_lib.BagsLensField) == 4 * 4 + 8
    assert _lib.ABI_VERSION == 11 and lib.bags_abi_version() == 11 and re.search(r"#define\s+BAGS_ABI_VERSION\s+11\b", header)
    assert {"LensField", "lens_field", "lens_field_torch"} <= set(bags_raster.__all__)


@pytest.mark.parametrize("B,H,n,what", [(5, 65, 1, "hidden 65"), (5, 64, 5, "internal_layers 5"), (33, 64, 1, "blocks 33")])
def test_a_larger_net_is_sent_to_the_pytorch_path(lib, B, H, n, what):
    p, x = torch.zeros(param_count(B, H, n)), torch.zeros(3, 2)
    with pytest.raises(ValueError, match="lens_field_torch") as e:
        lens_field(p, x, B, H, n)
    assert what in str(e.value)
    assert lens_field_torch(p, x, B, H, n).shape == (3, 2)                      # which takes it
    # the library says the same, before anything is enqueued (no GPU touched)
    buf = (C.c_char * 64)()
    addr = C.addressof(buf)
    net = _lib.BagsLensField(B, H, n, 0, addr)
    for rc in (lib.bags_lens_field_forward(C.byref(net), addr, 3, addr, None), lib.bags_lens_field_inverse(C.byref(net), addr, 3, 5, addr, None),
               lib.bags_lens_field_backward(C.byref(net), addr, 3, addr, addr, 1 << 40, addr, addr, None)):
        assert rc == -1 and b"lens_field_torch" in lib.bags_last_error() and what.encode() in lib.bags_last_error()


def test_argument_errors(lib):
    good = torch.zeros(param_count(2, 16, 1))
    with pytest.raises(ValueError, match="flat vector"):
        lens_field(good[:-1], torch.zeros(3, 2), 2, 16, 1)
    with pytest.raises(ValueError, match="flat vector"):
        lens_field_torch(good.view(2, -1), torch.zeros(3, 2), 2, 16, 1)
    with pytest.raises(ValueError, match=r"\(\.\.\., 2\)"):
        lens_field(good, torch.zeros(3, 3), 2, 16, 1)
    with pytest.raises(ValueError, match=r"\(\.\.\., 2\)"):
        lens_field_torch(good, torch.zeros(3, 3), 2, 16, 1)
    with pytest.raises(RuntimeError, match="AMD GPU.*lens_field_torch"):       # no silent CPU fallback
        lens_field(good, torch.zeros(3, 2), 2, 16, 1)
    # the library: null pointers, a short workspace, a negative count; M == 0 and "no gradient asked for" are no-ops
    buf, buf2 = (C.c_char * 64)(), (C.c_char * 64)()
    addr, addr2 = C.addressof(buf), C.addressof(buf2)
    net = _lib.BagsLensField(2, 16, 1, 0, addr)
    assert lib.bags_lens_field_forward(C.byref(net), None, 3, addr, None) == -1 and b"null x" in lib.bags_last_error()
    assert lib.bags_lens_field_forward(C.byref(net), addr, -1, addr, None) == -1 and b"M -1" in lib.bags_last_error()
    assert lib.bags_lens_field_inverse(C.byref(net), addr, 3, -1, addr, None) == -1 and b"iterations" in lib.bags_last_error()
    assert lib.bags_lens_field_backward(C.byref(net), addr, 3, addr, addr, 16, addr, None, None) == -3 and b"workspace" in lib.bags_last_error()
    assert lib.bags_lens_field_backward(C.byref(net), addr, 3, addr, None, 0, None, addr2, None) == -3
    assert lib.bags_lens_field_backward(C.byref(net), addr, 3, None, addr, 1 << 40, addr, None, None) == -1 and b"grad_y" in lib.bags_last_error()
    assert lib.bags_lens_field_backward(C.byref(net), addr, 3, addr, addr, 1 << 40, None, addr, None) == -1 and b"params vector" in lib.bags_last_error()
    assert lib.bags_lens_field_forward(C.byref(net), None, 0, None, None) == 0
    assert lib.bags_lens_field_inverse(C.byref(net), None, 0, 50, None, None) == 0
    assert lib.bags_lens_field_backward(C.byref(net), None, 0, None, None, 0, None, None, None) == 0
    assert lib.bags_lens_field_backward(C.byref(net), addr, 3, addr, None, 0, None, None, None) == 0
    net.params = None
    assert lib.bags_lens_field_forward(C.byref(net), addr, 3, addr, None) == -1 and b"null params" in lib.bags_last_error()


def _norms(net):
    return [float(torch.linalg.matrix_norm(W.double(), 2)) for block in net.layers() for W, _ in block]


@pytest.mark.parametrize("B,H,n", [(5, 64, 1), (3, 33, 2), (2, 16, 4), (1, 2, 0)])
def test_lipschitz_correction(B, H, n):
    net = LensField(B, H, n, seed=11)
    with torch.no_grad():
        net.params.mul_(8.0)
    assert max(_norms(net)) > 0.8 * 2
    before = net.params.detach().clone()
    net.lipschitz_correction(iterations=50, generator=torch.Generator().manual_seed(5))
    norms = _norms(net)
    assert max(norms) <= 0.8 * (1 + 1e-3), norms
    # only the matrices change, each by one factor; the biases stay
    for (W, b), (W0, b0) in zip([l for blk in net.layers() for l in blk], [l for blk in layer_views(before, B, H, n) for l in blk]):
        assert torch.equal(b, b0)
        ratio = (W / W0).flatten()
        assert float(ratio.max() - ratio.min()) < 1e-6 and float(ratio.max()) <= 1.0
    # a net already below the maximum is left bitwise untouched, whatever the iteration count and start vector
    kept = net.params.detach().clone()
    with torch.no_grad():
        net.params.mul_(0.9)
        kept.mul_(0.9)
    for it, seed in ((50, 6), (10, 7), (1, 8)):
        net.lipschitz_correction(iterations=it, generator=torch.Generator().manual_seed(seed))
        assert torch.equal(net.params.detach(), kept)


@pytest.mark.parametrize("B,H,n", [(5, 64, 1), (3, 33, 2), (2, 16, 0), (1, 16, 4)])
def test_inverse_round_trip_in_float64(B, H, n):
    net = LensField(B, H, n, seed=21)
    net.lipschitz_correction(iterations=50, generator=torch.Generator().manual_seed(22))
    net = net.double()
    x = torch.rand(200, 2, dtype=torch.float64, generator=torch.Generator().manual_seed(23)) * 3 - 1.5
    with torch.no_grad():
        y = net(x)
        # max |g_b| over the points, at each block's input
        gmax, xb = [], x
        for layers in net.layers():
            step = lens_field_torch(torch.cat([t.reshape(-1) for l in layers for t in l]), xb, 1, H, n) - xb
            gmax.append(float(step.abs().max()))
            xb = xb + step
        assert torch.equal(xb, y)
        c = 0.8 ** (n + 2)                                      # the contraction bound the correction guarantees
        assert net.inverse(y, 0) is not None and torch.equal(net.inverse(y, 0), y)
        last = None
        for k in (1, 3, 10, 50):
            err = float((net.inverse(y, k) - x).abs().max())
            bound = sum(c ** k / (1 - c) * g for g in gmax) + 1e-13
            assert err <= bound, (k, err, bound)
            last = err
        assert last < 1e-9
        assert torch.equal(net.inverse(y, 7), lens_field_inverse_torch(net.params, y, B, H, n, 7))


@pytest.mark.parametrize("name", sorted(LC.CASES))
def test_cases_are_self_consistent(name):
    c = LC.make_case(name)
    B, H, n = LC.dims(name)
    assert c["params"].numel() == param_count(B, H, n) and c["x"].shape == c["cot"].shape == LC.CASES[name]["shape"]
    assert float(c["x"].min()) >= -1.5 and float(c["x"].max()) <= 1.5
    again = LC.make_case.__wrapped__(name)
    assert all(torch.equal(c[k], again[k]) for k in ("params", "x", "cot"))
    ref = LC.reference(name)
    assert all(bool(torch.isfinite(t).all()) for t in ref) and all(float(t.abs().max()) > 0 for t in ref)
    e = LC.err32(name)
    assert all(math.isfinite(v) for v in e), e
    bars = LC.bars(name)
    assert all(math.isfinite(b) and b > 0 for b in bars)
    if c["x"].numel() > 2:
        assert all(v > 0 for v in e), e                                 # the float32 path is not the reference: a bar is built from it
    # the reference does not bless itself, and a wrong answer is far outside the bar
    assert LC.errors(name, ref) == (0.0, 0.0, 0.0)
    off = LC.errors(name, tuple(t * (1 + 1e-4) for t in ref))
    assert all(o > b for o, b in zip(off, bars)), (off, bars)
    if name == LC.SATURATED:
        # both tails of the ELU: arguments below -5 (slope < 1 %) and above +5 in the first layer
        W, b = layer_views(c["params"], B, H, n)[0][0]
        a = c["x"] @ W.t() + b
        assert float(a.min()) < -5 and float(a.max()) > 5
    else:
        assert name in LC.INVERTIBLE
        ie = LC.inverse_err32(name)
        assert math.isfinite(ie) and math.isfinite(LC.inverse_bar(name)) and LC.inverse_bar(name) > 0
        # 50 iterations have converged: the inverse of the reference's output is the input
        assert float((LC.inverse_reference(name) - c["x"].double()).abs().max()) < 1e-5
