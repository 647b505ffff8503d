"""CPU checks of the training step of tests/step_cases.py: on the maps of the CPU oracle's forward, the conditions the GPU test
(tests/test_step_gpu.py) rests on; every term of the step in float32 against float64, so that the comparison rule is exercised without a
GPU; and two deliberately wrong float32 sides, which the rule must reject by a factor of 10 or more."""
import functools

import pytest
import torch

import step_cases as S
from bags_raster import gaussian_normals_torch, pinhole_of
from depth_oracle import oracle_forward

NAMES = S.TERMS + ("all",)


@functools.lru_cache(maxsize=None)
def _oracle_step():
    """(maps, views, constants) of the step on the oracle's forward: the colour pass and, with the Gaussians' normals as the colour,
    the normal pass, per camera of the step."""
    scene, cams = S.scene(), S.cameras()
    maps = {k: [] for k in S.MAP_NAMES}
    views, pins = [], []
    with torch.no_grad():
        for r in S.ROWS:
            cam = cams[r]
            view = cam.get_world_view_transform().detach().contiguous()
            st = oracle_forward(scene, cam, S.SH_DEGREE)
            sn = oracle_forward(scene, cam, S.SH_DEGREE, colors=gaussian_normals_torch(scene["rotations"], scene["scales"], scene["means3D"], view))
            for k, t in (("depth", st.depth_img), ("weights", st.weights), ("render", st.image), ("normal", sn.image), ("depth_n", sn.depth_img),
                         ("weights_n", sn.weights)):
                maps[k].append(t.detach().contiguous())
            views.append(view)
            pins.append(pinhole_of(cam.get_intrinsic(), S.H, S.W))
    assert all(torch.equal(a, b) for k in ("depth", "weights") for a, b in zip(maps[k], maps[k + "_n"]))
    c = S.constants_of(maps, views, pins)
    return maps, views, S.constants_on(c, "cpu")


def _side(side, **wrong):
    """Every term on ``side`` in one forward on fresh leaves: ({term: loss}, {term: count}, {name: {quantity: gradient}}) with the
    gradients of each term's loss and of the step's scalar at the maps, the view matrices and the appearance table."""
    maps0, views0, c = _oracle_step()
    maps = {k: [t.clone().requires_grad_(True) for t in ts] for k, ts in maps0.items()}
    maps["table"] = S.table_start().requires_grad_(True)
    views = torch.stack(views0).requires_grad_(True)
    losses, counts = S.run("all", side, maps, list(views.unbind(0)), c, **wrong)
    leaves = [t for k in S.MAP_NAMES for t in maps[k]] + [views, maps["table"]]
    grads = {}
    for name in NAMES:
        scalar = S.total(losses) if name == "all" else losses[name].sum()
        g = torch.autograd.grad(scalar, leaves, retain_graph=True, allow_unused=True)
        out = {}
        for i, k in enumerate(S.MAP_NAMES):
            part = g[i * S.V:(i + 1) * S.V]
            if any(t is not None for t in part):
                out[k] = torch.stack([torch.zeros_like(maps[k][v]) if t is None else t for v, t in enumerate(part)])
        if g[-2] is not None:
            out["views"] = g[-2]
        if g[-1] is not None:
            out["table"] = g[-1][list(S.ROWS)]
        grads[name] = out
    return {k: v.detach() for k, v in losses.items()}, counts, grads


@functools.lru_cache(maxsize=None)
def _sides():
    return _side("t32"), _side("t64")


def test_the_conditions_the_gpu_test_rests_on():
    """Caps that keep the test from hiding a failure, not measurements."""
    _, _, c = _oracle_step()
    print("\nstep on the oracle's maps: solid %.3f  warp-valid %.3f  |x - gt| >= %.3g  guards %s"
          % (c["solid"], c["warp_valid"], c["gt_gap"], {k: round(v, 4) for k, v in c["guards"].items()}))
    assert c["solid"] >= 0.5                                  # every view has at least half its pixels solid
    assert c["warp_valid"] >= 0.4                             # every ordered pair keeps 40 % of its pixels in the warp
    assert all(v <= 0.03 for v in c["guards"].values()), c["guards"]
    assert c["gt_gap"] >= 1e-3                                # the L1 sign is no decision
    loss64 = _sides()[1][0]["normal_prior"]
    assert (loss64 > 1e-3).all(), loss64                      # the turned normal prior leaves something to pull on


def test_the_float32_statements_against_float64():
    (l32, n32, g32), (l64, n64, g64) = _sides()
    for t in S.TERMS:
        assert torch.equal(n32[t].double(), n64[t]) or S.counts_agree({t: n32[t]}, {t: n64[t]}), t
        assert (n64[t] > 0).all(), t
        assert torch.isfinite(l64[t]).all() and (l64[t] != 0).all(), t
    for name in NAMES:
        reach = S.REACH[name]
        want = set(reach["maps"]) | ({"views"} if reach["views"] else set()) | ({"table"} if reach["table"] else set())
        assert set(g64[name]) == want == set(g32[name]), (name, sorted(g64[name]))
        for q, r64 in g64[name].items():
            assert torch.isfinite(r64).all() and r64.abs().max().item() > 0, (name, q)
            if q != "table":                                   # the yardstick is usable: the float32 statement errs, and only a little
                err = S.tensor_err(g32[name][q], r64)
                assert err < 1e-4, (name, q, err)
                # normal_map_loss_torch and normal_smooth_loss_torch are float64 from the loads on, so on float32 maps they ARE the
                # float64 statement: that yardstick is 0 by construction and the bar at the rendered normals is the floor alone
                assert err == 0.0 if q in S.EXACT_IN_FLOAT32 else err > 0.0, (name, q, err)


@pytest.mark.parametrize("wrong,term", ((dict(swap_pair=7), "warp"), (dict(detach_mean=True), "depth_smooth")), ids=("warp-pair-swapped", "smooth-mean-detached"))
def test_a_wrong_side_fails_the_rule_tenfold(wrong, term):
    """The float32 side with pair 7's source and destination view exchanged in ``warp``, and with ``depth_smooth``'s gradient through the
    mean dropped: both the term alone and the whole step are over their bars by a factor of 10 at least, in a gradient at the maps or the
    view matrices (step_cases.map_margins: the per-element rule and, beside it, the per-tensor rule; the dropped mean is 5.4 x over the
    per-element bar at the weights and 1.8 x at the depth, because that bar's floor is absolute and these gradients are small, and two
    orders of magnitude over the per-tensor one)."""
    (l32, _, g32), (l64, _, g64) = _sides()
    _, _, bad = _side("t32", **wrong)
    for name in (term, "all"):
        margins = {(q, rule): m for q in g64[name] if q != "table" for rule, m in S.map_margins(bad[name][q], g32[name][q], g64[name][q]).items()}
        print("\n%s, %s: margins %s" % (wrong, name, {"%s/%s" % k: round(v, 1) for k, v in margins.items()}))
        assert max(margins.values()) >= 10.0, margins
        right = [m for q in g64[name] for m in S.map_margins(g32[name][q], g32[name][q], g64[name][q]).values()]
        assert max(right) <= 1.0 / S.FACTOR                   # (and the right side passes its own rule, as it must)
