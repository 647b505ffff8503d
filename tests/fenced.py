"""Fenced, poisoned buffers: every tensor the library is handed comes out of the middle of a larger uint8 buffer.

``with fenced(dirt) as f:`` replaces, for the length of the block,

  * ``torch.empty`` / ``torch.empty_like`` / ``torch.zeros`` / ``torch.zeros_like`` by versions that call the original and return a
    view of the same shape and dtype which starts BAND bytes into a uint8 buffer filled with ``dirt`` and is followed, at its very
    last byte, by another BAND bytes of ``dirt`` (the ``zeros`` variants zero the view).  The buffer comes from the allocator, whose
    blocks are 512-byte aligned, and BAND is a multiple of 512: the view keeps the alignment an ordinary tensor has, so no kernel
    changes its vector / scalar branch.  Zero-element tensors pass through; a tensor that cannot be re-homed (not contiguous, not
    strided, pinned, ``out=``) passes through and is counted in ``f.skipped``;
  * ``bags_raster._lib.workspace``, and every name in a ``bags_raster`` module that was bound to it at import
    (``rasterizer._bytes``), likewise -- with ``shift`` bytes added to the start of the region and ``shrink`` bytes taken off its
    length, for the workspace calls ``which`` selects (None: all; an int or a collection of ints: the calls with those indices,
    counted from 0 in the order the block makes them).

``f.sites`` counts the fenced allocations by the module that asked for them and ``f.from_package`` those the package's own code
made: its outputs, gradient buffers and scratch.  ``f.copy(t)`` is a fenced copy of a tensor (what the in-place entry points are handed).  ``f.intact()`` reads back every band
that was handed out, ``f.report()`` names the allocations whose band was written.  The helper holds every buffer until it is
dropped, so that a band is never recycled into another tensor while it is still to be read.  Everything is restored when the block
ends, also by an exception.  References and comparisons belong OUTSIDE the block: inside it every temporary of torch is fenced too.

This is a plain module, not a fixture: the tests that use it import it."""
from __future__ import annotations

import collections
import contextlib
import importlib
import pkgutil
import sys

import torch

BAND = 4096
_NAMES = ("empty", "empty_like", "zeros", "zeros_like")


class Fences:
    def __init__(self, dirt: int, shift: int = 0, shrink: int = 0, which=None):
        if not 0 <= int(dirt) <= 255:
            raise ValueError("dirt is one byte")
        self.dirt, self.shift, self.shrink = int(dirt), int(shift), int(shrink)
        self.which = None if which is None else ({int(which)} if isinstance(which, int) else {int(i) for i in which})
        self.skipped = 0               # tensors that passed through unfenced
        self.skipped_what = []         # ... and what they were
        self.workspaces = 0            # workspace calls served (zero-byte ones included in the index, not in this count)
        self.workspace_calls = 0       # index of the next workspace call
        self.workspace_bytes = []      # what each call asked for, by index
        self.fenced = 0                # tensors handed out fenced (workspaces excluded)
        self.sites = collections.Counter()     # module that asked -> fenced tensors and workspaces it was handed
        self._orig = {}
        self._allocs = []              # (buffer, start of the region, its end, description)
        self._storages = set()

    # ---------------------------------------------------------------------------------------------- the buffers
    def _home(self, nbytes: int, device, what: str, lead: int = 0):
        """A region of ``nbytes`` bytes, ``BAND + lead`` bytes into a dirty buffer and followed by BAND more."""
        lo, hi = BAND + lead, BAND + lead + nbytes
        buf = self._orig["empty"](hi + BAND, dtype=torch.uint8, device=device)
        buf.fill_(self.dirt)
        self._allocs.append((buf, lo, hi, what))
        self._storages.add(buf.untyped_storage().data_ptr())
        return buf[lo:hi]

    def _rehome(self, t: torch.Tensor, what: str, zero: bool = False, requires_grad: bool = False, site: str = ""):
        if not isinstance(t, torch.Tensor) or t.numel() == 0:
            return t
        pinned = (not t.is_cuda) and t.layout == torch.strided and t.is_pinned()
        if t.layout != torch.strided or not t.is_contiguous() or pinned or t.is_meta:
            self.skipped += 1
            self.skipped_what.append("%s %s %s on %s" % (what, tuple(t.shape), t.dtype, t.device.type))
            return t
        desc = "%s %s %s" % (what, tuple(t.shape), str(t.dtype).replace("torch.", ""))
        v = self._home(t.numel() * t.element_size(), t.device, desc).view(t.dtype).view(t.shape)
        if zero:
            v.zero_()
        self.fenced += 1
        self.sites[site] += 1
        return v.requires_grad_() if requires_grad else v

    def _factory(self, name: str):
        orig, zero = self._orig[name], name.startswith("zeros")

        def replacement(*args, **kwargs):
            if kwargs.get("out") is not None or kwargs.get("pin_memory"):
                self.skipped += 1
                self.skipped_what.append("%s(out= / pin_memory=)" % name)
                return orig(*args, **kwargs)
            rg = bool(kwargs.pop("requires_grad", False))
            return self._rehome(orig(*args, **kwargs), "torch." + name, zero=zero, requires_grad=rg,
                                site=sys._getframe(1).f_globals.get("__name__", ""))
        replacement.__name__ = name
        return replacement

    def _workspace(self, nbytes, device):
        nbytes = int(nbytes)
        i = self.workspace_calls
        self.workspace_calls += 1
        self.workspace_bytes.append(nbytes)
        if nbytes == 0:
            return self._orig["workspace"](0, device)
        chosen = self.which is None or i in self.which
        shift, shrink = (self.shift, self.shrink) if chosen else (0, 0)
        self.workspaces += 1
        self.sites[sys._getframe(1).f_globals.get("__name__", "")] += 1
        return self._home(max(nbytes - shrink, 0), device, "workspace #%d of %d bytes (shift %d, shrink %d)" % (i, nbytes, shift, shrink),
                          lead=shift)

    # ---------------------------------------------------------------------------------------------- what the tests ask
    def copy(self, t: torch.Tensor) -> torch.Tensor:
        """A fenced copy of ``t`` (same shape, dtype, device, requires_grad; contiguous)."""
        src = t.detach().contiguous()
        if src.numel() == 0:
            return src.clone().requires_grad_(t.requires_grad)
        v = self._rehome(src, "copy", site="copy")
        v.copy_(src)
        return v.requires_grad_(t.requires_grad)

    @property
    def skipped_on_device(self):
        """The pass-throughs that live on a GPU: only those can reach the library."""
        return [w for w in self.skipped_what if w.endswith(" on cuda")]

    @property
    def from_package(self) -> int:
        """Fenced tensors and workspaces that code of the package itself asked for: its outputs, gradients and scratch."""
        return sum(n for m, n in self.sites.items() if m == "bags_raster" or m.startswith("bags_raster."))

    def is_fenced(self, t: torch.Tensor) -> bool:
        return isinstance(t, torch.Tensor) and t.numel() > 0 and t.untyped_storage().data_ptr() in self._storages

    def _written(self):
        if torch.cuda.is_available() and any(b.is_cuda for b, _, _, _ in self._allocs):
            torch.cuda.synchronize()
        bad = []
        for buf, lo, hi, what in self._allocs:
            before, after = int((buf[:lo] != self.dirt).sum()), int((buf[hi:] != self.dirt).sum())
            if before or after:
                bad.append((what, before, after, buf, lo, hi))
        return bad

    def intact(self) -> bool:
        return not self._written()

    def report(self) -> str:
        lines = []
        for what, before, after, buf, lo, hi in self._written():
            for side, n, band, base in (("before", before, buf[:lo], -lo), ("after", after, buf[hi:], 0)):
                if n:
                    idx = torch.nonzero(band != self.dirt).flatten()
                    lines.append("%s: %d bytes written %s it, at offsets %d .. %d from its %s" %
                                 (what, n, side, int(idx[0]) + base, int(idx[-1]) + base, "start" if side == "before" else "end"))
        return "\n".join(lines) if lines else "every band intact (%d allocations, %d workspaces)" % (self.fenced, self.workspaces)

    # ---------------------------------------------------------------------------------------------- install / restore
    def _install(self):
        import bags_raster
        from bags_raster import _lib
        for m in pkgutil.walk_packages(bags_raster.__path__, "bags_raster."):
            try:
                importlib.import_module(m.name)
            except Exception:                     # a submodule that needs something this machine lacks binds nothing either
                pass
        self._orig = {n: getattr(torch, n) for n in _NAMES}
        self._orig["workspace"] = _lib.workspace
        self._patched = []
        serve = self._workspace                   # ONE bound method: every patched name is the same object
        for n in _NAMES:
            setattr(torch, n, self._factory(n))
            self._patched.append((torch, n, self._orig[n]))
        for name, mod in list(sys.modules.items()):
            if mod is None or not (name == "bags_raster" or name.startswith("bags_raster.")):
                continue
            for attr, val in list(vars(mod).items()):
                if val is self._orig["workspace"]:
                    setattr(mod, attr, serve)
                    self._patched.append((mod, attr, val))

    def _restore(self):
        for obj, attr, val in reversed(self._patched):
            setattr(obj, attr, val)
        self._patched = []


@contextlib.contextmanager
def fenced(dirt: int, shift: int = 0, shrink: int = 0, which=None):
    f = Fences(dirt, shift, shrink, which)
    f._install()
    try:
        yield f
    finally:
        f._restore()
