"""No-GPU checks of the drop-in boundary: the library loads, exports every symbol include/bags_raster.h declares,
reports sane buffer sizes, and the host shim refuses CPU tensors / bad argument combinations like the reference op."""
import ctypes as C
import os
import re

import pytest
import torch

from bags_raster import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def lib():
    if not os.path.exists(_lib.LIB_PATH):
        import __graft_entry__ as g
        g.build()
    return _lib.load()


def test_every_declared_symbol_is_exported(lib):
    header = open(os.path.join(ROOT, "include", "bags_raster.h")).read()
    declared = set(re.findall(r"\b(bags_[a-z_0-9]+)\s*\(", header))
    assert declared, "no declarations parsed"
    assert declared == set(_lib.SYMBOLS), (declared ^ set(_lib.SYMBOLS))
    for name in declared:
        assert hasattr(lib, name), name
    assert lib.bags_abi_version() == _lib.ABI_VERSION


def test_buffer_sizes_grow_with_problem(lib):
    assert lib.bags_geom_size(0) > 0
    assert lib.bags_geom_size(500_000) > 500_000 * 80
    assert lib.bags_geom_size(1000) < lib.bags_geom_size(100_000)
    assert lib.bags_binning_size(3_700_000, 1920, 1080) >= 3_700_000 * 16
    assert lib.bags_image_size(1920, 1080) >= 1920 * 1080 * 8
    assert lib.bags_backward_workspace_size(500_000, 3_700_000) >= 3_700_000 * 48      # one 48-byte record per instance


def test_buffer_sizes_match_the_recorded_ones(lib):
    """The eight size functions are ABI: callers allocate by them, and the operator counts on equal problems giving equal sizes.
    tests/golden/buffer_sizes.json holds what they reported BEFORE the layouts moved onto one carving helper (written by
    tests/golden/make_buffer_sizes.py from a build of that earlier commit); every entry must still be reported, to the byte."""
    import importlib.util
    import json
    golden = os.path.join(ROOT, "tests", "golden")
    spec = importlib.util.spec_from_file_location("make_buffer_sizes", os.path.join(golden, "make_buffer_sizes.py"))
    gen = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(gen)
    want = json.load(open(os.path.join(golden, "buffer_sizes.json")))["sizes"]
    cases = gen.cases()
    assert len(cases) == 11 + 7 * 6 + 6 + 11 * 7 + 4 + 4 + 11 + 11
    assert set(want) == {gen.key(name, args) for name, args in cases}
    wrong = {}
    for name, args in cases:
        got = int(getattr(lib, name)(*args))
        if got != want[gen.key(name, args)]:
            wrong[gen.key(name, args)] = (got, want[gen.key(name, args)])
    assert not wrong, wrong


def test_struct_layout_matches_header(lib):
    # field counts and pointer-size packing of the POD structs (a mismatch would corrupt every call)
    assert C.sizeof(_lib.BagsSettings) == 14 * 4 + 5 * 8     # + clamp_grad (ABI 5), conic_grad (ABI 8; reserved0 before)
    assert C.sizeof(_lib.BagsInputs) == 8 + 9 * 8 + 8          # + shs_rest (ABI 7)
    assert C.sizeof(_lib.BagsState) == 6 * 8
    assert C.sizeof(_lib.BagsForwardOut) == 5 * 8
    assert C.sizeof(_lib.BagsBackwardArgs) == 4 * 8 + 14 * 8 + 8 + 8 + 8 + 8 + 8  # + binning_capacity (ABI 4), accumulate + dense_per_tile (ABI 6 / 8), grad_shs_rest (ABI 7), phase + reserved2 (ABI 9), grad_dldc (ABI 10)
    assert C.sizeof(_lib.BagsShViews) == 8 + 2 * 16 * 8                         # (ABI 10)
    assert C.sizeof(_lib.BagsDebugViews) == 8 * 8


def test_error_path_reports_message(lib):
    rc = lib.bags_compute_relocation(None, None, None, None, 51, 0, None, None, None)
    assert rc != 0 and b"compute_relocation" in lib.bags_last_error()
    s = _lib.BagsSettings(); i = _lib.BagsInputs(); st = _lib.BagsState(); o = _lib.BagsForwardOut()
    n = C.c_int64(0)
    rc = lib.bags_forward_prepare(C.byref(s), C.byref(i), C.byref(st), C.byref(o), C.byref(n), None)
    assert rc == -1 and b"empty image" in lib.bags_last_error()      # argument validation, no GPU touched


def test_backward_phase_is_validated(lib):
    """ABI 9: BagsBackwardArgs.phase selects the per-tile half, the per-Gaussian half, or both; anything else is an argument error
    (reported before anything is enqueued: no GPU touched)."""
    assert (_lib.BWD_ALL, _lib.BWD_BLEND, _lib.BWD_PREPROCESS) == (0, 1, 2)
    # a syntactically complete call whose only defect is the phase: host pointers are fine, validation never dereferences them
    buf = (C.c_char * 4096)()
    addr = C.addressof(buf)
    s = _lib.BagsSettings(16, 16, 0.5, 0.5, 1.0, 0, 1, 0, 0, 0, 1, 0, 0, 0, addr, addr, addr, addr, addr)
    i = _lib.BagsInputs(0, None, None, None, None, None, None, None, None, None, None)
    st = _lib.BagsState(addr, 1 << 40, addr, 1 << 40, addr, 1 << 40)
    a = _lib.BagsBackwardArgs()
    a.grad_color, a.workspace, a.workspace_bytes, a.phase = addr, addr, 1 << 40, 3
    rc = lib.bags_backward(C.byref(s), C.byref(i), C.byref(st), C.byref(a), None)
    assert rc == -1 and b"phase" in lib.bags_last_error(), (rc, lib.bags_last_error())


def test_loss_workspace_is_taken_as_given_and_refused_off_four_bytes(lib):
    """The loss workspace holds float planes and its base is not rounded (include/bags_raster.h): a base off 4 bytes, and a buffer one
    byte short, are argument errors of all four entry points, reported before anything is enqueued (no GPU touched)."""
    buf = (C.c_char * 4096)()
    addr = (C.addressof(buf) + 15) // 16 * 16
    need = lib.bags_loss_workspace_size(3, 5, 4)
    calls = {"loss_forward": lambda ws, n: lib.bags_loss_forward(addr, addr, 3, 5, 4, ws, n, addr, None),
             "loss_backward": lambda ws, n: lib.bags_loss_backward(addr, addr, 3, 5, 4, ws, n, addr, addr, None),
             "photometric_loss_forward": lambda ws, n: lib.bags_photometric_loss_forward(addr, addr, 3, 5, 4, ws, n, 0.2, addr, None),
             "photometric_loss_backward": lambda ws, n: lib.bags_photometric_loss_backward(addr, addr, 3, 5, 4, ws, n, 0.2, addr, addr, None)}
    for op, call in calls.items():
        for off in (1, 2, 3, 5):
            assert call(addr + off, need) != 0
            assert lib.bags_last_error() == (op + ": the workspace is not 4-byte aligned").encode(), (op, off, lib.bags_last_error())
        assert call(addr, need - 1) != 0 and lib.bags_last_error().startswith((op + ": workspace").encode()), (op, lib.bags_last_error())


def test_factored_sh_gradient_arguments_are_validated(lib):
    """ABI 10: bags_sh_gradient_from_views / BagsBackwardArgs.grad_dldc argument errors (reported before anything is enqueued)."""
    buf = (C.c_char * 4096)()
    addr = C.addressof(buf)
    v = _lib.BagsShViews()
    v.n_views = 17
    assert lib.bags_sh_gradient_from_views(10, 16, 3, addr, C.byref(v), addr, None, 0, None) == -1 and b"n_views" in lib.bags_last_error()
    v.n_views = 1
    assert lib.bags_sh_gradient_from_views(10, 4, 3, addr, C.byref(v), addr, None, 0, None) == -1 and b"coefficients" in lib.bags_last_error()
    assert lib.bags_sh_gradient_from_views(10, 16, 3, addr, C.byref(v), addr, None, 0, None) == -1 and b"NULL campos" in lib.bags_last_error()
    assert lib.bags_sh_gradient_from_views(0, 16, 3, None, C.byref(v), None, None, 0, None) == 0          # nothing to do
    # grad_dldc together with grad_shs: refused
    s = _lib.BagsSettings(16, 16, 0.5, 0.5, 1.0, 0, 1, 0, 0, 0, 1, 0, 0, 0, addr, addr, addr, addr, addr)
    i = _lib.BagsInputs(4, addr, None, None, addr, None, addr, addr, addr, None, None)
    st = _lib.BagsState(addr, 1 << 40, addr, 1 << 40, addr, 1 << 40)
    a = _lib.BagsBackwardArgs()
    a.grad_color, a.workspace, a.workspace_bytes, a.grad_shs, a.grad_dldc = addr, addr, 1 << 40, addr, addr
    assert lib.bags_backward(C.byref(s), C.byref(i), C.byref(st), C.byref(a), None) == -1 and b"grad_dldc" in lib.bags_last_error()


def test_operator_api_surface_and_argument_errors():
    import inspect
    import diff_gaussian_rasterization as dgr
    from bags_raster import GaussianRasterizationSettings, GaussianRasterizer
    assert dgr.GaussianRasterizer is GaussianRasterizer and dgr.GaussianRasterizationSettings is GaussianRasterizationSettings
    # the 14 settings keywords of gaussian_renderer/__init__.py:50-65, in order
    assert GaussianRasterizationSettings._fields[:14] == (
        "image_height", "image_width", "tanfovx", "tanfovy", "bg", "scale_modifier", "viewmatrix", "projmatrix",
        "intrinsic", "sh_degree", "campos", "prefiltered", "debug", "debug_iter")
    # the 10 call keywords of gaussian_renderer/__init__.py:110-121
    params = set(inspect.signature(GaussianRasterizer.forward).parameters)
    assert {"means3D", "means2D", "means2D_densify", "shift_factors", "shs", "colors_precomp", "opacities", "scales",
            "rotations", "cov3D_precomp"} <= params
    eye = torch.eye(4)
    st = GaussianRasterizationSettings(32, 32, 0.5, 0.5, torch.zeros(3), 1.0, eye, eye, eye, 0, torch.zeros(3), False, False, 0)
    r = GaussianRasterizer(st)
    x = torch.zeros(4, 3)
    with pytest.raises(Exception, match="excatly one of either SHs or precomputed colors"):
        r(means3D=x, means2D=x, opacities=torch.ones(4, 1), scales=x, rotations=torch.zeros(4, 4))
    with pytest.raises(Exception, match="exactly one of either scale/rotation pair or precomputed 3D covariance"):
        r(means3D=x, means2D=x, opacities=torch.ones(4, 1), shs=torch.zeros(4, 1, 3))
    with pytest.raises(RuntimeError, match="AMD GPU"):     # no silent CPU fallback
        r(means3D=x, means2D=x, opacities=torch.ones(4, 1), shs=torch.zeros(4, 1, 3), scales=x, rotations=torch.zeros(4, 4))
    with pytest.raises(NotImplementedError):
        dgr.compute_relocation(None, None, None, None, 51)


def test_render_signature_is_the_reference_one():
    """gaussian_renderer/__init__.py:30: render(viewpoint_camera, pc, pipe, bg_color, mlp_color, shift_factors, hybrid=True,
    scaling_modifier=1.0, override_color=None, iteration=None, global_alignment=None)."""
    import inspect
    from bags_raster.render import render
    ps = list(inspect.signature(render).parameters.values())
    assert [p.name for p in ps[:11]] == ["viewpoint_camera", "pc", "pipe", "bg_color", "mlp_color", "shift_factors", "hybrid",
                                         "scaling_modifier", "override_color", "iteration", "global_alignment"]
    assert all(p.default is inspect.Parameter.empty for p in ps[:6])
    assert ps[6].default is True and ps[7].default == 1.0 and all(p.default is None for p in ps[8:11])


@pytest.mark.timeout(600)
def test_host_side_is_clean_under_address_sanitizer():
    """the host half of the library (argument validation, buffer carving, size queries, error strings,
    the ctypes struct layout) under AddressSanitizer.  `make asan` instruments HOST code only; the run is CPU-only by
    construction (this file's tests never launch a kernel) and is never made on a GPU box."""
    import shutil
    import subprocess
    import sys
    if os.environ.get("BAGS_RASTER_LIB"):
        pytest.skip("already inside the sanitizer run")
    if torch.cuda.is_available():
        pytest.skip("sanitizer builds are not run on a GPU box")
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    if not os.path.exists(hipcc):
        pytest.skip("no hipcc")
    csrc = os.path.join(ROOT, "bundle-adjusting-gaussian-splatting_amd", "csrc")
    r = subprocess.run(["make", "-C", csrc, "asan", "-j4"], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    rt = subprocess.run([hipcc, "-print-file-name=libclang_rt.asan-x86_64.so"], capture_output=True, text=True).stdout.strip()
    if not os.path.isabs(rt) or not os.path.exists(rt):
        pytest.skip("no shared ASan runtime in this toolchain")
    env = dict(os.environ, BAGS_RASTER_LIB=os.path.join(csrc, "build_asan", "libbags_raster_asan.so"), LD_PRELOAD=rt,
               ASAN_OPTIONS="detect_leaks=0:abort_on_error=0:exitcode=23")
    r = subprocess.run([sys.executable, "-m", "pytest", os.path.abspath(__file__), "-q", "-x", "-p", "no:cacheprovider",
                        "-k", "not address_sanitizer"], capture_output=True, text=True, env=env, cwd=ROOT)
    assert r.returncode == 0 and "AddressSanitizer" not in r.stderr, r.stdout[-3000:] + r.stderr[-3000:]


@pytest.mark.timeout(300)
@pytest.mark.parametrize("define", ["DIAG_PAIRS", "DIAG_PHASES"])
def test_diagnostic_builds_of_the_blend_kernels_still_compile(define, tmp_path):
    """csrc/blend.hip keeps two diagnostic builds (tools/diag_pairs.sh: evaluated against contributing (pixel, splat) pairs;
    tools/diag_phases.py: a wave's time per phase of the backward) behind -DDIAG_PAIRS / -DDIAG_PHASES.  Nothing else compiles
    them, so they are compiled here (gfx950 cross-compile, no GPU) to keep them from rotting, and the shipped source is held to
    the handful of preprocessor conditionals that remain (every tuning switch whose A/B lost was deleted in round 5)."""
    import shutil
    import subprocess
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    if not os.path.exists(hipcc):
        pytest.skip("no hipcc")
    csrc = os.path.join(ROOT, "bundle-adjusting-gaussian-splatting_amd", "csrc")
    r = subprocess.run([hipcc, "-O3", "-fPIC", "-std=c++17", "--offload-arch=gfx950", f"-D{define}", "-c", os.path.join(csrc, "blend.hip"),
                        "-o", str(tmp_path / "blend_diag.o")], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]
    n_if = sum(1 for ln in open(os.path.join(csrc, "blend.hip")) if ln.lstrip().startswith(("#if", "#elif")))
    assert n_if <= 15, n_if
