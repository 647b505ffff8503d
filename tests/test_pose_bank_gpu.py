"""The camera bank on the GPU (bags_raster/pose_bank.py; the bank kernels of csrc/camera.hip and csrc/adam.hip).

1. the chain of a step's rows against the float64 chain at the edges of pose space -- the cases, the reference and the bars are
   tests/camera_cases.py's, nothing in a bar comes from the kernel;
2. a bank row is the single-camera kernel's bits, the rows that are not listed are exact zeros, the alignment gradients are the fp32
   left fold over the row list;
3. PoseAdam against one float64 ``torch.optim.Adam`` per camera, by the rule of tests/adam_reference.py;
4. ``render_views`` over the cameras of a bank; 5. a side stream."""
import itertools

import pytest
import torch

import adam_reference as AR
import camera_cases as CC
from bags_raster import _lib as L
from bags_raster import camera as cam
from bags_raster.pose_bank import PoseAdam, PoseBank

pytestmark = pytest.mark.gpu
DEV = "cuda"
LEAF_SLICES = dict(dq=slice(0, 4), dt=slice(4, 7), fovx=slice(7, 8), fovy=slice(8, 9))


# --------------------------------------------------------------------------------------------- 1. the float64 rule
def _case_camera(inp):
    """The inputs of a camera case (float32 cast) as a PoseCamera on the host."""
    c = cam.PoseCamera(torch.eye(3), torch.zeros(3), 1.1, 0.7, 64, 48, znear=inp["znear"], zfar=inp["zfar"])
    with torch.no_grad():
        c.init_quaternion.copy_(inp["q0"]); c.init_translation.copy_(inp["t0"].reshape(3, 1))
        c.delta_quaternion.copy_(inp["dq"]); c.delta_translation.copy_(inp["dt"].reshape(3, 1))
        c.learnable_fovx.copy_(inp["fovx"]); c.learnable_fovy.copy_(inp["fovy"])
    return c


def _reference(inp, cots):
    """What ``CC.reference`` holds, for inputs that are not a named case (a benign row under another case's alignment)."""
    v64, g64 = CC.chain(inp, torch.float64, CC.ALL_ON, cots)
    v32, g32 = CC.chain(inp, torch.float32, CC.ALL_ON, cots)
    err32 = ({n: CC.value_error(v32[n], v64[n]) for n in v64}, {n: CC.gradient_error(g32[n], g64[n]) for n in g64})
    return dict(values=v64, grads=g64, grads32=g32, err32=err32, bars=CC.bars((v64, g64), err32))


def _judge(tag, got, ref, e32, bar):
    """One gradient against its float64 reference: within ``bar``, or exact zeros where the float64 gradient is exactly zero."""
    e = CC.gradient_error(got.cpu(), ref)
    if e is None:
        assert bar is None and not got.any(), (tag, got)
        print(f"{tag}: exact zeros")
        return
    print(f"{tag}: kernel {e:.3e} pytorch32 {e32:.3e} bar {bar:.3e}")
    assert e <= bar, (tag, e, e32, bar)


def _run_call(tag, rows_inputs, grot, gscale):
    """One bank call over ``rows_inputs`` = [(name, inputs, cotangents, reference)] in row-list order, under one alignment; an extra
    camera that is not listed sits in the bank.  Every row's values and leaf gradients, and the alignment gradients, are judged."""
    n = len(rows_inputs)
    order = list(range(n))[::-1]                                # row v of the call is bank row n - 1 - v: the list is not the identity
    cams = [None] * n
    for v, (_, inp, _, _) in enumerate(rows_inputs):
        cams[order[v]] = _case_camera(inp)
    bank = PoseBank.from_cameras(cams + [_case_camera(CC.make_case("benign")[0])], device=DEV)
    f = lambda t: None if t is None else t.to(torch.float32).to(DEV).requires_grad_(True)
    gr, gs = f(grot), f(gscale)
    out = bank.get_matrices(order, gr, gs)
    cots = [torch.stack([r[2][k] for r in rows_inputs]).to(torch.float32).to(DEV) for k in range(4)]
    sum((c * o).sum() for c, o in zip(cots, out)).backward()
    assert not bank.leaves.grad[n].any()
    for v, (name, _, _, ref) in enumerate(rows_inputs):
        vb, gb = ref["bars"]
        for k, vn in enumerate(CC.VALUES):
            e, e32 = CC.value_error(out[k][v].detach().cpu(), ref["values"][vn]), ref["err32"][0][vn]
            print(f"{tag} row {v} {name} {vn}: kernel {e:.3e} pytorch32 {e32:.3e} bar {vb[vn]:.3e}")
            assert e <= vb[vn], (tag, v, name, vn, e, e32, vb[vn])
        for ln, sl in LEAF_SLICES.items():
            _judge(f"{tag} row {v} {name} d{ln}", bank.leaves.grad[order[v], sl], ref["grads"][ln], ref["err32"][1][ln], gb[ln])
    for ln, leaf in (("grot", gr), ("gscale", gs)):
        if leaf is None:
            continue
        sum64 = sum(r[3]["grads"][ln] for r in rows_inputs)                          # the float64 sum over the call's rows
        fold32 = rows_inputs[0][3]["grads32"][ln]
        for r in rows_inputs[1:]:
            fold32 = fold32 + r[3]["grads32"][ln]                                      # the float32 chain, same rows, same order
        e32 = CC.gradient_error(fold32, sum64)
        bar = CC.bars(({}, {ln: sum64}), ({}, {ln: e32}))[1][ln]                       # the FACTOR / FLOOR rule, as camera_cases states it
        _judge(f"{tag} d{ln} over {n} rows", leaf.grad, sum64, e32, bar)


def test_chain_against_float64_rows_without_alignment():
    names = [n for n in CC.CASES if CC.make_case(n)[0]["grot"] is None and CC.make_case(n)[0]["gscale"] is None]
    assert len(names) == 12
    rows = []
    for n in names:
        ref = CC.reference(n)
        rows.append((n, ref["inputs"], ref["cots"], ref))
    _run_call("plain", rows, None, None)


ALIGNED = [n for n in CC.CASES if CC.make_case(n)[0]["grot"] is not None or CC.make_case(n)[0]["gscale"] is not None]


@pytest.mark.parametrize("name", ALIGNED)
def test_chain_against_float64_aligned_case_with_two_benign_rows(name):
    ref = CC.reference(name)
    inp = ref["inputs"]
    b_inp, b_cots = CC.make_case("benign")
    b_inp["grot"], b_inp["gscale"] = inp["grot"], inp["gscale"]                        # the rows of a call share the alignment
    b_ref = _reference(b_inp, b_cots)
    _run_call(name, [("benign", b_inp, b_cots, b_ref), (name, inp, ref["cots"], ref), ("benign", b_inp, b_cots, b_ref)], inp["grot"], inp["gscale"])


def test_aligned_cases_are_the_six():
    assert ALIGNED == ["benign", "skewed_alignment", "reflecting_alignment", "rotation_only", "scale_only", "unit_scale"]


# --------------------------------------------------------------------------------------------- 2. the single-camera kernel's bits
def _random_cameras(N, seed=21):
    g = torch.Generator().manual_seed(seed)
    out = []
    for i in range(N):
        c = cam.PoseCamera(cam.quaternion_to_rotation(torch.randn(4, generator=g)), torch.randn(3, generator=g) + torch.tensor([0.0, 0.0, 4.0]),
                           0.4 + 0.1 * i, 2.2 - 0.1 * i, 64, 48, znear=0.01 * (1 + i % 5), zfar=100.0 - 3.0 * i)
        with torch.no_grad():
            c.delta_quaternion.copy_(0.05 * torch.randn(4, generator=g)); c.delta_translation.copy_(0.1 * torch.randn(3, 1, generator=g))
            c.learnable_fovx.add_(0.03 * torch.randn((), generator=g)); c.learnable_fovy.sub_(0.02 * torch.randn((), generator=g))
        out.append(c)
    return out


def _alignment(seed=5):
    g = torch.Generator().manual_seed(seed)
    return (cam.quaternion_to_rotation(torch.tensor([1.0, 0.02, -0.03, 0.01])) + 0.05 * torch.randn(3, 3, generator=g)).to(DEV), torch.tensor(1.3, device=DEV)


def _fold(parts):
    acc = parts[0]
    for p in parts[1:]:
        acc = acc + p                                           # fp32, left to right
    return acc


ROW_LISTS = [(1, [0]), (3, [0]), (3, [2, 0]), (17, [2, 0]), (17, list(range(16))[::-1]), (17, [16] + list(range(15, -1, -1)))]


@pytest.mark.parametrize("align", [False, True])
@pytest.mark.parametrize("N,rows", ROW_LISTS, ids=[f"N{n}-{len(r)}rows" for n, r in ROW_LISTS])
def test_bank_rows_are_the_single_camera_kernels_bits(N, rows, align):
    bank = PoseBank.from_cameras(_random_cameras(N), device=DEV)
    singles = [bank.export(r) for r in rows]
    assert all(s.delta_quaternion.is_cuda for s in singles)
    g = torch.Generator().manual_seed(8)
    cots = [torch.randn(len(rows), 4, 4, generator=g).to(DEV) for _ in range(3)] + [torch.randn(len(rows), 3, generator=g).to(DEV)]
    ga = [t.clone().requires_grad_(True) for t in _alignment()] if align else [None, None]
    out = bank.get_matrices(rows, *ga)
    assert [tuple(t.shape) for t in out] == [(len(rows), 4, 4)] * 3 + [(len(rows), 3)]
    sum((c * o).sum() for c, o in zip(cots, out)).backward()
    per_cam = []
    for v, s in enumerate(singles):
        ga_v = [t.clone().requires_grad_(True) for t in _alignment()] if align else [None, None]
        want = s.get_matrices(*ga_v)                            # fused_camera_chain of the same leaves
        for k in range(4):
            assert torch.equal(out[k][v], want[k]), (v, CC.VALUES[k])
        sum((c[v] * w).sum() for c, w in zip(cots, want)).backward()
        assert torch.equal(bank.leaves.grad[rows[v]], torch.cat([t.grad.reshape(-1) for t in s.pose_leaves()])), v
        per_cam.append(ga_v)
    listed = torch.zeros(N, dtype=torch.bool)
    listed[rows] = True
    rest = bank.leaves.grad[~listed.to(DEV)]
    assert rest.shape == (N - len(rows), 9) and not rest.any() and not torch.signbit(rest).any()
    if align:
        for k in range(2):
            assert torch.equal(ga[k].grad, _fold([p[k].grad for p in per_cam])), ("grot", "gscale")[k]


def _c_backward(bank, rows, ga, cots, null):
    """``bags_pose_bank_backward`` itself over buffers filled with NaN beforehand; cotangent i is a real NULL where ``null[i]``."""
    s = L.BagsPoseBank(len(bank), L.ptr(bank.init_quaternion), L.ptr(bank.init_translation), L.ptr(bank.near_far), L.ptr(bank.leaves.detach()),
                       L.ptr(ga[0]), L.ptr(ga[1]), len(rows), (L.C.c_int32 * L.MAX_POSE_ROWS)(*rows))
    g_leaves = torch.full((len(bank), 9), float("nan"), device=DEV)
    g_grot, g_gscale = torch.full((3, 3), float("nan"), device=DEV), torch.full((1,), float("nan"), device=DEV)
    L.call("bags_pose_bank_backward", bank.leaves.device, s, *[None if off else L.ptr(c) for c, off in zip(cots, null)], L.ptr(g_leaves),
           L.ptr(g_grot), L.ptr(g_gscale))
    return g_leaves, g_grot, g_gscale


def test_null_cotangents_are_zero_filled_ones_and_backward_repeats_bitwise():
    bank = PoseBank.from_cameras(_random_cameras(5), device=DEV)
    rows, ga = [3, 0, 4], _alignment()
    g = torch.Generator().manual_seed(12)
    cots = [torch.randn(3, 4, 4, generator=g).to(DEV) for _ in range(3)] + [torch.randn(3, 3, generator=g).to(DEV)]
    for null in itertools.product((False, True), repeat=4):
        zeroed = [torch.zeros_like(c) if off else c for c, off in zip(cots, null)]
        a = _c_backward(bank, rows, ga, cots, null)
        b = _c_backward(bank, rows, ga, zeroed, (False,) * 4)
        for x, y, n in zip(a, b, ("leaves", "grot", "gscale")):
            assert not torch.isnan(x).any() and torch.equal(x, y), (null, n)
        assert not a[0][1].any() and not a[0][2].any()
    # autograd's route twice over one graph
    leaves_ga = [t.clone().requires_grad_(True) for t in ga]
    out = bank.get_matrices(rows, *leaves_ga)
    loss = sum((c * o).sum() for c, o in zip(cots, out))
    first = torch.autograd.grad(loss, [bank.leaves] + leaves_ga, retain_graph=True)
    second = torch.autograd.grad(loss, [bank.leaves] + leaves_ga)
    for x, y in zip(first, second):
        assert torch.equal(x, y)
    for x, y in zip(first, _c_backward(bank, rows, ga, cots, (False,) * 4)):
        assert torch.equal(x.reshape(y.shape), y)


# --------------------------------------------------------------------------------------------- 3. PoseAdam
LRS = (1e-3, 2e-3, 5e-4)                                        # rotation, translation, fov
GROUP_SLICES = (slice(0, 4), slice(4, 7), slice(7, 9))


def _torch_step(state, counts, grad, rows, enabled, dtype):
    """(param, exp_avg, exp_avg_sq) (N,9) in ``dtype`` on the host after every camera of ``rows`` stepped its OWN
    ``torch.optim.Adam`` -- three groups at the three rates, step counts ``counts[camera]`` before the step -- over the enabled
    groups, from the fp32 ``state`` = (param, exp_avg, exp_avg_sq) and ``grad``.  Everything else keeps its value."""
    p, m, v = (t.detach().to("cpu", dtype).clone() for t in state)
    for r in rows:
        params = [torch.nn.Parameter(p[r, sl].clone()) for sl in GROUP_SLICES]
        opt = torch.optim.Adam([{"params": [q], "lr": lr} for q, lr in zip(params, LRS)], betas=AR.BETAS, eps=AR.EPS)
        for k, (q, sl) in enumerate(zip(params, GROUP_SLICES)):
            opt.state[q] = {"step": torch.tensor(float(counts[r, k])), "exp_avg": m[r, sl].clone(), "exp_avg_sq": v[r, sl].clone()}
            q.grad = grad[r, sl].detach().to("cpu", dtype).clone() if enabled[k] else None
        opt.step()
        for k, (q, sl) in enumerate(zip(params, GROUP_SLICES)):
            if enabled[k]:
                assert float(opt.state[q]["step"]) == counts[r, k] + 1
                p[r, sl], m[r, sl], v[r, sl] = q.detach(), opt.state[q]["exp_avg"], opt.state[q]["exp_avg_sq"]
    return p, m, v


def _adam_setup(N, seed):
    st = AR.random_state(N, seed, shapes=((9,),))[0]
    bank = PoseBank.from_cameras(_random_cameras(N), device=DEV)
    with torch.no_grad():
        bank.leaves.copy_(st["param"])
    opt = PoseAdam(bank, *LRS, betas=AR.BETAS, eps=AR.EPS)
    return bank, opt, st


def _checked_step(label, bank, opt, grad, rows, enabled=(True, True, True)):
    """One ``PoseAdam.step`` judged against the float64 reference from the state it started from; what it did not list or enable
    keeps its bits."""
    before = [t.detach().clone() for t in (bank.leaves, opt.exp_avg, opt.exp_avg_sq)]
    counts = opt.step_count.clone()
    bank.leaves.grad = grad.to(DEV)
    opt.step(rows, rotation=enabled[0], translation=enabled[1], fov=enabled[2])
    after = [bank.leaves.detach(), opt.exp_avg, opt.exp_avg_sq]
    ref64 = _torch_step(before, counts, grad, rows, enabled, torch.float64)
    ref32 = _torch_step(before, counts, grad, rows, enabled, torch.float32)
    touched = torch.zeros(len(bank), 9, dtype=torch.bool)
    for r in rows:
        for k, sl in enumerate(GROUP_SLICES):
            touched[r, sl] = enabled[k]
    for key, got, t32, t64, old in zip(AR.KEYS, after, ref32, ref64, before):
        AR.assert_rule(f"{label}/{key}", got[touched.to(DEV)], t32[touched], t64[touched])
        assert torch.equal(got[~touched.to(DEV)], old[~touched.to(DEV)]), (label, key)
    want = counts.clone()
    for r in rows:
        want[r] += torch.tensor([int(e) for e in enabled])
    assert torch.equal(opt.step_count, want), label


@pytest.mark.parametrize("count", [0, 1, 1000])
def test_pose_adam_against_float64_torch_adam_per_camera(count):
    bank, opt, st = _adam_setup(5, 40 + count)
    opt.exp_avg.copy_(st["exp_avg"]); opt.exp_avg_sq.copy_(st["exp_avg_sq"])
    opt.step_count[:] = count
    _checked_step(f"pose_adam[step={count}]", bank, opt, st["grad"], [0, 1, 2, 3, 4])


def test_pose_adam_sequence_keeps_a_count_per_camera_and_group():
    bank, opt, st = _adam_setup(5, 7)
    start = bank.leaves.detach().clone()
    g = torch.Generator().manual_seed(70)
    grads = [0.01 * torch.randn(5, 9, generator=g) for _ in range(3)]
    _checked_step("pose_adam_seq[0]", bank, opt, grads[0], [0, 3])
    _checked_step("pose_adam_seq[1]", bank, opt, grads[1], [3], enabled=(True, True, False))
    _checked_step("pose_adam_seq[2]", bank, opt, grads[2], [1, 3, 4])
    assert opt.step_count.tolist() == [[1, 1, 1], [1, 1, 1], [0, 0, 0], [3, 3, 2], [1, 1, 1]]
    assert torch.equal(bank.leaves[2], start[2]) and not opt.exp_avg[2].any() and not opt.exp_avg_sq[2].any()


def test_pose_adam_seventeen_rows_are_sixteen_and_one():
    N, rows = 20, [19, 3, 0] + list(range(5, 19))
    assert len(rows) == 17
    results = []
    for split in (False, True):
        bank, opt, st = _adam_setup(N, 3)
        opt.exp_avg.copy_(st["exp_avg"]); opt.exp_avg_sq.copy_(st["exp_avg_sq"])
        opt.step_count[:, 1] = 4
        bank.leaves.grad = st["grad"].to(DEV)
        if split:
            opt.step(rows[:16]); opt.step(rows[16:])
        else:
            opt.step(rows)
        results.append((bank.leaves.detach().clone(), opt.exp_avg.clone(), opt.exp_avg_sq.clone(), opt.step_count.clone()))
    for a, b in zip(*results):
        assert torch.equal(a, b)
    assert results[0][3][rows].tolist() == [[1, 5, 1]] * 17 and results[0][3].sum() == 4 * N + 3 * 17
    assert not torch.equal(results[0][0], _adam_setup(N, 3)[0].leaves.detach())


# --------------------------------------------------------------------------------------------- 4. render_views
OUT_KEYS = ("render", "radii", "depth", "weights", "means2D", "visibility_filter", "viewspace_points", "viewspace_points_densify")


def test_render_views_over_bank_cameras(monkeypatch):
    from bags_raster.gaussians import GaussianBag
    from bags_raster.render import PipelineParams, render_views
    from bags_raster.synth import sphere_views, synth_scene
    W = H = 32
    scene = synth_scene(257, seed=17)
    bank = PoseBank.from_cameras(sphere_views(3, W, H, noise=0.05, device=DEV))
    bg = torch.tensor([0.2, 0.1, 0.3], device=DEV)
    g = torch.Generator().manual_seed(6)
    weights = [torch.randn(3, H, W, generator=g).to(DEV) for _ in range(3)]

    def run(cameras):
        pc = GaussianBag.from_activated(scene, 3, device=DEV)
        outs = render_views(cameras, pc, PipelineParams(), bg, 0.0, None)
        sum((o["render"] * w).sum() for o, w in zip(outs, weights)).backward()
        return outs

    for order in ([0, 1, 2], [0, 1, 0]):                        # distinct rows: the bank's launch; a camera twice: the per-camera path
        names = []
        real_call = L.call
        monkeypatch.setattr(L, "call", lambda name, *a: (names.append(name), real_call(name, *a))[1])
        bank.leaves.grad = None
        outs = run([bank.camera(i) for i in order])
        monkeypatch.undo()
        if len(set(order)) == len(order):
            assert names.count("bags_pose_bank_forward") == 1 and names.count("bags_pose_bank_backward") == 1, names
        else:
            assert names.count("bags_pose_bank_forward") == len(order), names
        assert names.count("bags_camera_forward") == 0
        exported = [bank.export(i) for i in range(3)]
        refs = run([exported[i] for i in order])
        for out, ref in zip(outs, refs):
            assert set(out) == set(OUT_KEYS) == set(ref)
            for k in OUT_KEYS:
                assert torch.equal(out[k].detach(), ref[k].detach()), (order, k)
        assert outs[0]["radii"].gt(0).any()
        for i in range(3):
            if i in order:
                assert torch.equal(bank.leaves.grad[i], torch.cat([t.grad.reshape(-1) for t in exported[i].pose_leaves()])), (order, i)
                assert bank.leaves.grad[i].any()
            else:
                assert not bank.leaves.grad[i].any()


# --------------------------------------------------------------------------------------------- 5. a side stream
def test_side_stream_gives_the_default_streams_bits():
    results = []
    for side in (False, True):
        bank, opt, st = _adam_setup(5, 9)
        ga = [t.clone().requires_grad_(True) for t in _alignment()]
        g = torch.Generator().manual_seed(1)
        cots = [torch.randn(2, 4, 4, generator=g).to(DEV) for _ in range(3)] + [torch.randn(2, 3, generator=g).to(DEV)]
        torch.cuda.synchronize()
        stream = torch.cuda.Stream() if side else torch.cuda.current_stream()
        with torch.cuda.stream(stream):
            out = bank.get_matrices([4, 1], *ga)
            sum((c * o).sum() for c, o in zip(cots, out)).backward()
            grad = bank.leaves.grad.clone()
            opt.step([4, 1])
        stream.synchronize()
        results.append([o.detach() for o in out] + [grad, ga[0].grad, ga[1].grad, bank.leaves.detach(), opt.exp_avg, opt.exp_avg_sq])
    for a, b in zip(*results):
        assert torch.equal(a, b)
    assert results[0][4][[4, 1]].any() and not results[0][4][[0, 2, 3]].any()
