"""tests/fenced.py held to what it promises, on CPU tensors: the GPU suite's memory-contract test is only as good as its fences."""
import pytest
import torch

import bags_raster
from bags_raster import _lib as L
from bags_raster import rasterizer
from fenced import BAND, Fences, fenced

_TORCH = {n: getattr(torch, n) for n in ("empty", "empty_like", "zeros", "zeros_like")}
_WORKSPACE, _BYTES = L.workspace, rasterizer._bytes


def _restored():
    return (all(getattr(torch, n) is f for n, f in _TORCH.items()) and L.workspace is _WORKSPACE and rasterizer._bytes is _BYTES)


def _past_the_end(t, n=1):
    """The ``n`` elements behind ``t``'s last, as a kernel that overruns it would reach them."""
    return torch.as_strided(t, (n,), (1,), t.storage_offset() + t.numel())


def _in_front(t, n=1):
    return torch.as_strided(t, (n,), (1,), t.storage_offset() - n)


def test_values_shape_dtype_and_alignment():
    with fenced(0xA5) as f:
        a = torch.empty(3, 5, dtype=torch.float64)
        b = torch.empty_like(a, dtype=torch.int16)
        c = torch.empty((7,), dtype=torch.float32, requires_grad=True)
        a.copy_(torch.arange(15.0).reshape(3, 5))
    assert a.shape == (3, 5) and a.dtype == torch.float64 and a.is_contiguous()
    assert b.shape == (3, 5) and b.dtype == torch.int16
    assert c.requires_grad and c.is_leaf
    assert torch.equal(a, torch.arange(15.0, dtype=torch.float64).reshape(3, 5))
    for t in (a, b, c):
        assert f.is_fenced(t) and t.data_ptr() % 16 == 0 and t.storage_offset() * t.element_size() == BAND
    assert f.fenced == 3 and f.skipped == 0 and f.intact()
    assert f.sites[__name__] == 3 and f.from_package == 0      # asked for here, not by the package
    assert not f.is_fenced(torch.empty(4))


def test_overrun_after_is_seen():
    with fenced(0xA5) as f:
        t = torch.empty(5, dtype=torch.float32)
        ok = torch.empty(5, dtype=torch.float32)
    assert f.intact()
    _past_the_end(t).fill_(1.0)                      # one element: the band starts at the view's very last byte
    assert not f.intact()
    rep = f.report()
    assert "(5,)" in rep and "float32" in rep and "after" in rep and "before" not in rep and "4 bytes" in rep
    assert rep.count("\n") == 0, "the untouched allocation %r is not reported" % (ok.shape,)


def test_underrun_before_is_seen():
    with fenced(0xFF) as f:
        t = torch.zeros(2, 3, dtype=torch.int32)
    assert f.intact()
    _in_front(t.view(-1)).fill_(0)
    assert not f.intact()
    rep = f.report()
    assert "(2, 3)" in rep and "int32" in rep and "before" in rep and "after" not in rep


def test_a_stray_store_of_the_dirt_byte_needs_the_other_dirt():
    with fenced(0xA5) as f:
        t = torch.empty(4, dtype=torch.uint8)
    _past_the_end(t).fill_(0xA5)                     # writing the dirt byte itself cannot be seen: that is why two dirts are used
    assert f.intact()
    with fenced(0xFF) as g:
        u = torch.empty(4, dtype=torch.uint8)
    _past_the_end(u).fill_(0xA5)
    assert not g.intact()


def test_dirt_ff_reads_as_nan_and_minus_one():
    with fenced(0xFF) as f:
        f32, f64 = torch.empty(4), torch.empty(4, dtype=torch.float64)
        i32, i8 = torch.empty(4, dtype=torch.int32), torch.empty(4, dtype=torch.int8)
        like = torch.empty_like(f32)
    assert torch.isnan(f32).all() and torch.isnan(f64).all() and torch.isnan(like).all()
    assert (i32 == -1).all() and (i8 == -1).all()
    assert f.intact()


def test_dirt_a5_is_not_zero():
    with fenced(0xA5):
        t, b = torch.empty(4), torch.empty(4, dtype=torch.uint8)
    assert (b == 0xA5).all() and (t != 0).all() and torch.isfinite(t).all()


def test_zeros_variants_return_zeros():
    with fenced(0xFF) as f:
        z = torch.zeros(3, 4)
        zl = torch.zeros_like(z, dtype=torch.int64)
        z0 = torch.zeros((), dtype=torch.float64)
        zr = torch.zeros_like(z, requires_grad=True)
    assert z.shape == (3, 4) and not z.any() and zl.dtype == torch.int64 and not zl.any() and z0.shape == () and z0 == 0
    assert zr.requires_grad and not zr.detach().any()
    assert all(f.is_fenced(t) for t in (z, zl, z0, zr)) and f.intact()


def test_pass_throughs_are_counted():
    base = torch.arange(12.0).reshape(3, 4).t()      # not contiguous: empty_like preserves the strides
    with fenced(0xA5) as f:
        e0 = torch.empty(0, 3)                       # zero elements: passes through, not counted
        assert f.skipped == 0
        nc = torch.empty_like(base)
        assert f.skipped == 1 and not nc.is_contiguous()
        into = _TORCH["empty"](3)
        torch.zeros(3, out=into)
        assert f.skipped == 2
        c = torch.empty_like(base, memory_format=torch.contiguous_format)
    assert f.skipped == 2 and len(f.skipped_what) == 2 and "(4, 3)" in f.skipped_what[0] and f.skipped_what[0].endswith(" on cpu")
    assert f.skipped_on_device == []
    assert e0.numel() == 0 and not f.is_fenced(e0) and not f.is_fenced(nc) and f.is_fenced(c)
    assert f.fenced == 1


def test_copy_is_fenced_and_equal():
    src = torch.arange(10, dtype=torch.float32).reshape(2, 5).requires_grad_()
    view = torch.arange(12.0).reshape(3, 4).t()
    with fenced(0xA5) as f:
        c, v, e = f.copy(src), f.copy(view), f.copy(torch.empty(0, 3))
    assert torch.equal(c, src) and c.requires_grad and c.is_leaf and f.is_fenced(c) and c.data_ptr() != src.data_ptr()
    assert torch.equal(v, view) and v.is_contiguous() and f.is_fenced(v) and e.shape == (0, 3)
    c.detach().add_(1.0)                             # an in-place step on the copy stays inside it
    assert f.intact()
    _past_the_end(c.detach().view(-1)).fill_(3.0)
    assert not f.intact() and "copy" in f.report()


def test_restored_after_the_block_and_after_an_exception():
    assert _restored()
    with fenced(0xA5):
        assert not _restored() and torch.empty is not _TORCH["empty"] and L.workspace is not _WORKSPACE
    assert _restored()
    with pytest.raises(KeyError):
        with fenced(0xFF):
            assert rasterizer._bytes is not _BYTES
            raise KeyError("inside")
    assert _restored()
    assert not isinstance(torch.empty(3), type(None)) and torch.empty(3).storage_offset() == 0


def test_workspace_and_its_import_time_alias_are_reached():
    assert rasterizer._bytes is L.workspace          # the alias the issue names: bound at import
    with fenced(0xA5) as f:
        assert rasterizer._bytes is L.workspace and L.workspace is not _WORKSPACE
        for mod in (bags_raster.knn, bags_raster.loss, bags_raster.distortion):
            assert mod.L.workspace is L.workspace    # (they look the function up on the module at call time)
        a = L.workspace(1000, "cpu")
        b = rasterizer._bytes(300, torch.device("cpu"))
        z = L.workspace(0, "cpu")
    assert f.workspaces == 2 and f.workspace_calls == 3 and f.workspace_bytes == [1000, 300, 0]
    assert a.dtype == torch.uint8 and a.numel() == 1000 and b.numel() == 300 and z.numel() == 0 and z.data_ptr() == 0
    assert (a == 0xA5).all() and f.is_fenced(a) and f.is_fenced(b) and f.fenced == 0
    assert a.data_ptr() % 16 == 0
    assert f.sites[__name__] == 2 and f.from_package == 0
    assert f.intact()
    _past_the_end(b).fill_(0)
    assert not f.intact() and "workspace #1 of 300 bytes" in f.report()


def test_allocations_of_the_package_are_told_from_the_test_s():
    from bags_raster.mcmc import relocation_binoms
    relocation_binoms.cache_clear() if hasattr(relocation_binoms, "cache_clear") else None
    with fenced(0xA5) as f:
        mine = torch.zeros(3)
        table = relocation_binoms(7, "cpu")                   # bags_raster/mcmc.py fills a torch.zeros table
    assert f.sites[__name__] == 1 and f.is_fenced(mine)
    assert f.from_package >= 1 and f.sites["bags_raster.mcmc"] >= 1 and table.shape == (7, 7) and table[3, 1] == 3.0


@pytest.mark.parametrize("which,hit", [(None, (True, True)), (1, (False, True)), ([0], (True, False))])
def test_workspace_shift_and_shrink(which, hit):
    with fenced(0xFF, shift=1, shrink=3, which=which) as f:
        ws = [L.workspace(512, "cpu"), rasterizer._bytes(256, "cpu")]
    plain = Fences(0xFF)
    for w, n, h in zip(ws, (512, 256), hit):
        assert w.numel() == (n - 3 if h else n)
        assert w.storage_offset() == BAND + (1 if h else 0)
        assert (w == 0xFF).all()
    assert f.intact() and plain.intact()
    _past_the_end(ws[0]).fill_(0)                    # the band follows the SHRUNK region at once: its missing bytes are fence
    assert not f.intact()


def test_nothing_is_replaced_twice_by_nested_blocks():
    with fenced(0xA5) as f:
        with fenced(0xFF) as g:
            t = torch.empty(4, dtype=torch.uint8)
        u = torch.empty(4, dtype=torch.uint8)
    assert _restored()
    assert (u == 0xA5).all() and f.is_fenced(u) and g.is_fenced(t) and f.intact() and g.intact()
