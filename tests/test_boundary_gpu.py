"""Every wrapper launches on the CURRENT stream of its tensors' device (bags_raster/_lib.py: ``call`` appends it as the entry
point's last argument).  The wrappers run once inside ``torch.cuda.stream(side)``, behind kernels that keep ``side`` busy while
the inputs are produced on it, and once on the default stream: the results are the same bit for bit.  A crossing that launched
on another stream than the one its inputs are produced on would read them before they exist."""
import pytest
import torch

from bags_raster import sh_colors
from bags_raster.camera import fused_camera_chain
from bags_raster.distortion import resample_image
from bags_raster.gaussians import fused_activations
from bags_raster.knn import distCUDA2
from bags_raster.loss import fused_photometric_loss

pytestmark = pytest.mark.gpu
DEV = "cuda"
P = 64


def _host_inputs():
    g = torch.Generator().manual_seed(11)
    r, n = (lambda *s: torch.rand(*s, generator=g)), (lambda *s: torch.randn(*s, generator=g))
    return dict(img=r(3, 16, 20), gt=r(3, 16, 20), src=r(3, 16, 16), ctl=r(4, 4, 2) * 1.6 - 0.8, g_warp=n(3, 12, 12),
                dq=0.05 * n(4), dt=0.1 * n(3, 1), fovx=torch.tensor(1.1), fovy=torch.tensor(0.7), q0=torch.tensor([1.0, 0.0, 0.0, 0.0]),
                t0=torch.tensor([[0.1], [-0.2], [4.0]]), g_cam=n(51), pts=r(P, 3), shs=0.3 * n(P, 16, 3), xyz=r(P, 3) * 2.6 - 1.3,
                campos=torch.tensor([0.3, -0.2, 4.0]), g_rgb=n(P, 3), dc=n(P, 1, 3), rest=0.3 * n(P, 15, 3), opacity=n(P, 1),
                scaling=n(P, 3), rotation=n(P, 4), g_act=n(P, 16 * 3 + 1 + 3 + 4))


def _run_wrappers(host):
    """Each wrapper's forward and one backward on the current stream; the inputs are outputs of kernels on that stream."""
    up = lambda name: host[name].to(DEV) + 0.0                        # noqa: E731
    leaf = lambda name: up(name).requires_grad_(True)                 # noqa: E731
    out = {}

    def keep(name, values, leaves=()):
        for k, t in enumerate(values):
            out[f"{name}[{k}]"] = t.detach()
        for k, t in enumerate(leaves):
            out[f"{name}.grad[{k}]"] = t.grad

    img = leaf("img")
    loss = fused_photometric_loss(img, up("gt"))
    loss.backward()
    keep("fused_photometric_loss", [loss], [img])

    src, ctl = leaf("src"), leaf("ctl")
    warped, mask = resample_image(src, ctl, (16, 16), (12, 12))
    warped.backward(up("g_warp"))
    keep("resample_image", [warped, mask], [src, ctl])

    pose = [leaf(n) for n in ("dq", "dt", "fovx", "fovy")]
    mats = fused_camera_chain(*pose, up("q0"), up("t0"))
    torch.cat([m.reshape(-1) for m in mats]).backward(up("g_cam"))
    keep("fused_camera_chain", mats, pose)

    keep("distCUDA2", [distCUDA2(up("pts"))])

    sh = [leaf(n) for n in ("shs", "xyz", "campos")]
    rgb = sh_colors(3, *sh)
    rgb.backward(up("g_rgb"))
    keep("sh_colors", [rgb], sh)

    raw = [leaf(n) for n in ("dc", "rest", "opacity", "scaling", "rotation")]
    act = fused_activations(*raw)
    torch.cat([a.reshape(P, -1) for a in act], dim=1).backward(up("g_act"))
    keep("fused_activations", act, raw)
    return out


def test_wrappers_launch_on_the_current_stream():
    host = _host_inputs()
    side = torch.cuda.Stream()
    with torch.cuda.stream(side):
        busy = torch.full((4096, 4096), 1e-4, device=DEV)
        for _ in range(10):                                           # ~10 ms of work in front of the inputs' producers
            busy = busy @ busy
        got = _run_wrappers(host)
    side.synchronize()
    want = _run_wrappers(host)
    torch.cuda.synchronize()
    assert got.keys() == want.keys() and len(got) == 28
    for name in want:
        assert got[name] is not None and torch.equal(got[name], want[name]), name
