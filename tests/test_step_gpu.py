"""GPU checks of one whole multi-view training step (tests/step_cases.py): render_views and render_normals of five PoseBank cameras,
eight loss terms on the maps of those two passes, one backward.  Three sides run the SAME fused code up to the operator's outputs --
fresh GaussianBag, PoseBank and AppearanceBank with identical parameters, so the maps are the same bits, which is asserted first --
and differ in what sits downstream of them: the fused wrappers (``hip``), the ``*_torch`` statements in float32 (``t32``) and on
``.double()`` inputs (``t64``).  The fused side is held to the float64 side by the rule of step_cases, with the float32 side as the
yardstick: loss values, the gradients at every map and at the view matrices, and the gradients at the leaves, where the cotangents of
every consumer have come back through the operator and been added up.  The operator's own correctness is test_parity_gpu.py's and
test_depth_grad_gpu.py's.  Every test prints its margins (error over bar); profiles/step/NOTES.md has them."""
import functools
from types import SimpleNamespace

import pytest
import torch

import step_cases as S
from bags_raster import AppearanceBank, GaussianAdam, GaussianBag, PipelineParams, PoseAdam, PoseBank, pinhole_of, render_normals, render_views

pytestmark = pytest.mark.gpu
DEV = "cuda"
NAMES = S.TERMS + ("all",)
BAG_LEAVES = ("xyz", "features_dc", "features_rest", "scaling", "rotation", "opacity")
LEAVES = BAG_LEAVES + ("pose", "table")
# the Adam rates of the second step's optimizers: the reference's training rates
GAUSSIAN_LRS = dict(xyz=1.6e-4, features_dc=2.5e-3, features_rest=1.25e-4, opacity=0.05, scaling=5e-3, rotation=1e-3)
POSE_LRS = (1e-3, 1e-3, 1e-4)


def _objects(mip=False, like=None):
    """Fresh objects of one side: the step's start, or -- ``like`` -- copies of another side's parameters as they are now."""
    bag = GaussianBag.from_activated(S.scene(), S.SH_DEGREE, device=DEV)
    bank = PoseBank.from_cameras(S.cameras(), device=DEV)
    app = AppearanceBank(S.CAMERAS, DEV)
    with torch.no_grad():
        app.table.copy_(S.table_start())
        if like is not None:
            for mine, theirs in zip(bag.leaves() + [bank.leaves, app.table], like.bag.leaves() + [like.bank.leaves, like.app.table]):
                mine.copy_(theirs)
        if mip:
            views, _, intrinsics, _ = bank.get_matrices(list(range(S.CAMERAS)))
            bag.compute_3D_filter(views, intrinsics, torch.tensor([[S.W, S.H]] * S.CAMERAS))
    return SimpleNamespace(bag=bag, bank=bank, app=app, pipe=PipelineParams(antialiasing=mip))


def _forward(o):
    """Both operator passes of the step's cameras and the view matrices the two-view terms see: (maps, views (V,4,4), intrinsics)."""
    cams = [o.bank.camera(i) for i in S.ROWS]
    pkgs = render_views(cams, o.bag, o.pipe, torch.zeros(3, device=DEV), 0.0, None, depth_weights_grad=True)
    nrm = render_normals(cams, o.bag, o.pipe, None, depth_weights_grad=True)
    views, _, intrinsics, _ = o.bank.get_matrices(list(S.ROWS))
    maps = dict(depth=[p["depth"] for p in pkgs], weights=[p["weights"] for p in pkgs], render=[p["render"] for p in pkgs],
                normal=[n["normal"] for n in nrm], depth_n=[n["depth"] for n in nrm], weights_n=[n["weights"] for n in nrm])
    return maps, views, intrinsics


def _constants_of(o):
    """The step's constants from a no_grad fused pass of ``o``; the caps tests/test_step_cpu.py holds on the oracle's maps hold here."""
    with torch.no_grad():
        maps, views, intrinsics = _forward(o)
        pins = [pinhole_of(intrinsics[v], S.H, S.W) for v in range(S.V)]
    c = S.constants_of(maps, list(views), pins)
    assert c["solid"] >= 0.5 and c["warp_valid"] >= 0.4 and c["gt_gap"] >= 1e-3 and all(v <= 0.03 for v in c["guards"].values()), \
        (c["solid"], c["warp_valid"], c["gt_gap"], c["guards"])
    return S.constants_on(c, DEV)


@functools.lru_cache(maxsize=None)
def _constants(mip):
    return _constants_of(_objects(mip))


def _leaf_tensors(o):
    return dict(zip(LEAVES, o.bag.leaves() + [o.bank.leaves, o.app.table]))


def _step(side, term, o, c):
    """One step of ``term`` on ``o``: forward, the terms of ``side`` on the maps, one backward.  Everything on the host."""
    maps, views, _ = _forward(o)
    for k in S.MAP_NAMES:
        for t in maps[k]:
            assert t.requires_grad, k
            t.retain_grad()
    views.retain_grad()
    losses, counts = S.run(term, side, dict(maps, table=o.app.table), list(views.unbind(0)), c)
    S.total(losses).backward()
    torch.cuda.synchronize()
    host = lambda t: None if t is None else t.detach().cpu()                             # noqa: E731
    g_maps = {}
    for k in S.MAP_NAMES:
        gs = [t.grad for t in maps[k]]
        g_maps[k] = None if all(g is None for g in gs) else torch.stack([torch.zeros_like(t) if g is None else g for t, g in zip(maps[k], gs)]).cpu()
    return SimpleNamespace(loss={t: host(l) for t, l in losses.items()}, count={t: host(n) for t, n in counts.items()},
                           maps={k: torch.stack([host(t) for t in maps[k]]) for k in S.MAP_NAMES}, views=host(views), g_maps=g_maps,
                           g_views=host(views.grad), g_leaves={k: host(t.grad) for k, t in _leaf_tensors(o).items()})


def _reached(term):
    r = S.REACH[term]
    leaves = {k: True for k in LEAVES}                          # every term comes back through the operator: geometry, opacity, pose
    leaves["features_dc"] = leaves["features_rest"] = r["sh"]
    leaves["table"] = r["table"]
    return r, leaves


def _nothing(g):
    return g is None or g.abs().max().item() == 0.0


def _hold(hip, t32, t64, term, what):
    """The three sides of one step against the rule; returns the margins, asserted to be at most 1."""
    for k in S.MAP_NAMES:                                      # the premise: the same maps, bit for bit, on all three sides
        assert torch.equal(hip.maps[k], t32.maps[k]) and torch.equal(hip.maps[k], t64.maps[k]), k
    assert torch.equal(hip.views, t32.views) and torch.equal(hip.views, t64.views)
    assert S.counts_agree(hip.count, t64.count) and S.counts_agree(t32.count, t64.count), (hip.count, t32.count, t64.count)
    reach, leaves = _reached(term)
    margins = {}
    for t in S.terms_of(term):
        assert torch.isfinite(t64.loss[t]).all() and (t64.loss[t] != 0).all() and (t64.count[t] > 0).all(), t
        margins["loss " + t] = S.element_margin(hip.loss[t], t32.loss[t], t64.loss[t])
    grads = [(k, hip.g_maps[k], t32.g_maps[k], t64.g_maps[k], k in reach["maps"]) for k in S.MAP_NAMES]
    grads.append(("views", hip.g_views, t32.g_views, t64.g_views, reach["views"]))
    for k, got, r32, r64, reached in grads:
        if not reached:                                        # e.g. photo alone leaves the depth's cotangent None (or zero)
            assert _nothing(got) and _nothing(r32) and _nothing(r64), k
            continue
        assert got is not None and torch.isfinite(got).all() and got.abs().max().item() > 0 and r64.abs().max().item() > 0, k
        for rule, m in S.map_margins(got, r32, r64).items():
            margins["d/d%s %s" % (k, rule)] = m
    if reach["views"]:
        assert hip.g_views[..., 3].abs().max().item() == 0.0  # the fourth column of every view-matrix gradient: exact zeros
    for k in LEAVES:
        got, r32, r64 = hip.g_leaves[k], t32.g_leaves[k], t64.g_leaves[k]
        if not leaves[k]:                                      # e.g. normal_smooth alone does not reach the SH leaves
            assert _nothing(got) and _nothing(r32) and _nothing(r64), k
            continue
        assert got is not None and torch.isfinite(got).all() and got.abs().max().item() > 0 and r64.abs().max().item() > 0, k
        margins["leaf " + k] = S.tensor_margin(got, r32, r64)
    rows, other = list(S.ROWS), list(S.UNLISTED)
    assert hip.g_leaves["pose"][other].abs().max().item() == 0.0 and (hip.g_leaves["pose"][rows].abs().amax(1) > 0).all()
    if leaves["table"]:
        assert hip.g_leaves["table"][other].abs().max().item() == 0.0 and (hip.g_leaves["table"][rows].abs().amax(1) > 0).all()
    print("\n%s %s: margins  %s" % (what, term, "  ".join("%s %.3f" % kv for kv in margins.items())))
    print("%s %s: worst %.3f" % (what, term, max(margins.values())))
    assert all(m <= 1.0 for m in margins.values()), {k: m for k, m in margins.items() if not m <= 1.0}
    return margins


def _three_sides(term, mip=False):
    c = _constants(mip)
    return tuple(_step(side, term, _objects(mip), c) for side in S.SIDES)


@pytest.mark.parametrize("term", NAMES)
def test_a_step_matches_the_float64_statement(term):
    """Each term alone and the whole step: loss values, the gradients at the maps and the view matrices per element and per tensor,
    the leaf gradients per tensor, all within the rule; what a term does not reach stays None or zero on every side; unlisted PoseBank
    and AppearanceBank rows and the fourth column of the view-matrix gradients are exact zeros."""
    _hold(*_three_sides(term), term, "step")


@pytest.mark.parametrize("term", ("all",))
def test_a_step_with_the_mip_filters(term):
    """The same with the 3D smoothing filter set and antialiased rendering: both are upstream of the operator and identical on the
    three sides, so the filtered activations' and the opacity scale's backward take the mixed cotangents."""
    _hold(*_three_sides(term, mip=True), term, "mip step")


def test_two_steps_give_the_same_bits():
    c = _constants(False)
    first, again = _step("hip", "all", _objects(), c), _step("hip", "all", _objects(), c)
    for t in S.TERMS:
        assert torch.equal(first.loss[t], again.loss[t]) and torch.equal(first.count[t], again.count[t]), t
    for k in S.MAP_NAMES:
        assert torch.equal(first.g_maps[k], again.g_maps[k]), k
    assert torch.equal(first.g_views, again.g_views)
    for k in LEAVES:
        assert torch.equal(first.g_leaves[k], again.g_leaves[k]), k


def test_the_second_step_after_the_optimizers():
    """A step on the fused side, one GaussianAdam step and one PoseAdam step of the listed rows, zero_grad; then the second step on the
    same objects against the two statement sides on fresh objects with the updated parameters: whatever a first step leaves behind --
    cached workspaces, saved state, gradients that were not cleared -- shows here."""
    o = _objects()
    _step("hip", "all", o, _constants(False))
    before = [t.detach().clone() for t in o.bag.leaves() + [o.bank.leaves]]
    leaf = _leaf_tensors(o)
    g_opt = GaussianAdam([{"params": [leaf[k]], "lr": lr, "name": k} for k, lr in GAUSSIAN_LRS.items()], lr=0.0, eps=1e-15)
    p_opt = PoseAdam(o.bank, *POSE_LRS)
    g_opt.step()
    p_opt.step(list(S.ROWS))
    g_opt.zero_grad()
    p_opt.zero_grad()
    o.app.table.grad = None
    torch.cuda.synchronize()
    for t, b in zip(o.bag.leaves(), before):
        assert not torch.equal(t.detach(), b)
    moved = (o.bank.leaves.detach() != before[-1]).any(1).cpu()
    assert moved[list(S.ROWS)].all() and not moved[list(S.UNLISTED)].any()
    c = _constants_of(o)
    hip = _step("hip", "all", o, c)
    t32, t64 = (_step(side, "all", _objects(like=o), c) for side in ("t32", "t64"))
    _hold(hip, t32, t64, "all", "second step")
