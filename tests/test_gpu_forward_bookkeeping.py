"""The list handling of composite_forward_q -- chunk appends into the four quadrant queues, the ring of 192 table slots,
the pops of a step -- on frames small enough to place every list length by hand.

Every case renders with the quadrant-queue forward (VTGS_FWD_IMPL = 3, the default) and with the lane = pixel forward
(VTGS_FWD_IMPL = 2, the cross-check library) and asks for the SAME BITS: colour, depth, radii, the sorted tile lists, and --
through the backward, which consumes sorted_gid, sorted_inst and final_T -- every gradient.  Then the float64 oracle at the
tolerances of tests/test_gpu_parity.py (image 1e-4 of the maximum with the audited threshold pixels, gradients 1e-3).

Splats are isotropic with a world scale of 0.3 px (0.62 px on screen after the 0.3 px^2 dilation), so the alpha >= 1/255 region
of the most opaque one used here reaches 2.0 px from its centre: a centre 3.0 .. 4.5 px inside its 8x8 tile stays >= 1 px clear
of the tile's edge under any radius rule, and the tile's list length is exactly the number of splats put there (asserted on
the lists the forward leaves in its workspace, not assumed).
"""
import pytest
import torch

from oracle import gs_oracle as go
from parity_util import (GRAD_KEYS, HIP_CENTRE_ERR_PX, audit_outliers, grad_error, run_oracle, tainted_gaussians,
                         to_settings)

pytestmark = pytest.mark.gpu

IMG_TOL, GRAD_TOL = 1e-4, 1e-3           # the bounds of tests/test_gpu_parity.py


def _opt(name, value):
    """Implementation switch of the library (vtgs_set_option); conftest restores the defaults after every test."""
    import diff_gaussian_rasterization as dgr
    dgr.set_option(name, int(value))


def _check_images(ref_c, ref_d, got_c, got_d, aux, opacities, cam):
    """HIP vs float64 oracle, as tests/test_gpu_parity.py does it: <= 1e-4 of the image maximum; a pixel above that must sit
    on a discrete decision of the composite in the oracle's own per-pair values (alpha at 1/255, transmittance at the 1e-4
    stop) and is then worth <= 8e-3.  Returns the mask of Gaussians that share a 16x16 tile with such a pixel."""
    tiles = set()
    for name, r, g in (("color", ref_c, got_c), ("depth", ref_d, got_d)):
        a = audit_outliers(r, g, aux, opacities, cam, IMG_TOL, centre_err_px=HIP_CENTRE_ERR_PX)
        assert not a["unexplained"], f"{name}: pixels above {IMG_TOL} that sit on no discrete decision: {a['unexplained'][:5]}"
        assert a["frac"] <= 1e-3 and a["max_rel"] <= 8e-3, f"{name}: {a['outliers']} outliers, max {a['max_rel']:.2e}"
        tiles |= a["tiles"]
    return tainted_gaussians(aux, tiles, opacities.shape[0])


def _check_grads(ref, got, taint):
    """<= 1e-3 on the gradients (99.9th percentile element-wise, 2e-3 of the largest gradient worst case); Gaussians beside
    an audited threshold pixel differ by that one pair's contribution (<= 2e-2)."""
    for k in GRAD_KEYS:
        scale = ref[k].abs().max().item()
        if scale == 0:                   # isotropic scenes: dL/drotations is exactly zero, the kernel's is float32 noise around it
            assert got[k].abs().max().item() <= 1e-4 * max(ref["scales"].abs().max().item(), 1e-30), k
            continue
        d = (ref[k].double() - got[k].double()).abs() / scale
        clean, dirty = d[~taint], d[taint]
        assert clean.numel() == 0 or clean.max().item() <= 2 * GRAD_TOL, f"grad {k}: max {clean.max().item():.2e}"
        assert grad_error(ref[k][~taint], got[k][~taint])[1] <= GRAD_TOL, f"grad {k}"
        assert dirty.numel() == 0 or dirty.max().item() <= 2e-2, f"grad {k}: max {dirty.max().item():.2e} beside an outlier pixel"


def _camera(W, H):
    fx = fy = W / 2.0
    cx, cy = W / 2.0 - 0.5, H / 2.0 - 0.5
    return go.setup_camera(W, H, [[fx, 0, cx], [0, fy, cy], [0, 0, 1]], torch.eye(4)), fx, fy, cx, cy


def _scene_at(W, H, px, py, opacity, seed, sigma_px=0.3):
    """Isotropic splats whose centres project to the pixel coordinates (px, py) (pixel centres are the integers), at distinct
    random depths."""
    g = torch.Generator().manual_seed(seed)
    cam, fx, fy, cx, cy = _camera(W, H)
    n = px.numel()
    zz = 1.0 + 4.0 * torch.rand(n, generator=g)
    scene = {
        "means3D": torch.stack([(px - cx + 0.5) / fx * zz, (py - cy + 0.5) / fy * zz, zz], dim=-1).contiguous(),
        "means2D": torch.zeros(n, 3),
        "opacities": opacity.reshape(n, 1).contiguous(),
        "colors_precomp": torch.rand(n, 3, generator=g),
        "scales": (sigma_px * zz / fx)[:, None].repeat(1, 3).contiguous(),
        "rotations": torch.tensor([[1.0, 0.0, 0.0, 0.0]]).repeat(n, 1),
    }
    return scene, cam


def _in_tiles(lengths, seed, lo=3.0, hi=4.5, op=(0.05, 0.6)):
    """lengths[t] splats inside 8x8 tile t of a 16x16 frame (tiles row-major), centres lo..hi px inside the tile."""
    g = torch.Generator().manual_seed(1000 + seed)
    xs, ys = [], []
    for t, n in enumerate(lengths):
        xs.append(8.0 * (t & 1) + lo + (hi - lo) * torch.rand(n, generator=g))
        ys.append(8.0 * (t >> 1) + lo + (hi - lo) * torch.rand(n, generator=g))
    px, py = torch.cat(xs), torch.cat(ys)
    opacity = op[0] + (op[1] - op[0]) * torch.rand(px.numel(), generator=g)
    return _scene_at(16, 16, px, py, opacity, seed)


def _run(scene, cam, dev, impl, grad_color):
    import diff_gaussian_rasterization as dgr
    _opt("VTGS_FWD_IMPL", impl)
    leaves = {k: v.detach().to(dev).clone().requires_grad_(grad_color is not None) for k, v in scene.items()}
    rast = dgr.GaussianRasterizer(raster_settings=to_settings(cam, dev))
    color, radii, depth = rast(**leaves)
    offs, gid, _geom, qmask = dgr.debug_tile_lists(rast, with_qmask=True)
    grads = None
    if grad_color is not None:
        (color * grad_color.to(dev)).sum().backward()
        grads = {k: leaves[k].grad.cpu() for k in GRAD_KEYS}
    return {"color": color.detach().cpu(), "radii": radii.cpu(), "depth": depth.detach().cpu(), "grads": grads,
            "offs": offs, "gid": gid, "qmask": qmask}


def _compare(scene, cam, dev, lengths=None, backward=False, oracle=True):
    """lane = pixel forward vs quadrant-queue forward bit for bit, then the oracle.  Returns the quadrant-queue run."""
    g = torch.Generator().manual_seed(5)
    grad_color = torch.rand(3, cam.image_height, cam.image_width, generator=g) * 2 - 1
    ref = _run(scene, cam, dev, 2, grad_color)
    got = _run(scene, cam, dev, 3, grad_color)
    for k in ("color", "depth", "radii", "offs", "gid"):
        assert torch.equal(ref[k], got[k]), k
    for k in GRAD_KEYS:                                  # the backward reads sorted_gid, sorted_inst and final_T of ITS forward
        assert torch.equal(ref["grads"][k], got["grads"][k]), k
    if lengths is not None:
        assert (got["offs"][1:] - got["offs"][:-1]).tolist() == list(lengths)
    if oracle and scene["opacities"].numel():
        ref_c, _ref_r, ref_d, ref_g, aux = run_oracle(scene, cam, grad_color)
        taint = _check_images(ref_c, ref_d, got["color"], got["depth"], aux, scene["opacities"], cam)
        if backward:
            _check_grads(ref_g, got["grads"], taint)
    return got


# chunk boundaries (64), the ring's wrap (192), the first append alone and with one and two more chunks behind it
CASE1 = [(0, 1, 15, 16), (17, 63, 64, 65), (191, 192, 193, 255), (256, 257, 0, 64)]


@pytest.mark.parametrize("lengths", CASE1)
def test_list_lengths_around_every_chunk_and_ring_boundary(gpu_device, lengths):
    scene, cam = _in_tiles(lengths, seed=sum(lengths))
    _compare(scene, cam, gpu_device, lengths=lengths, backward=True)


def test_lists_at_the_lds_copy_limit_and_the_counting_sort_limit(gpu_device):
    """416 ids stay in the wavefront's LDS copy, the 417th comes back from memory; 512 entries is the longest list the counting
    sort takes, 513 goes to the bitonic network and is re-read from memory as a whole."""
    lengths = (416, 417, 512, 513)
    scene, cam = _in_tiles(lengths, seed=7, op=(0.02, 0.2))
    _compare(scene, cam, gpu_device, lengths=lengths)


@pytest.mark.parametrize("order", ["one_quadrant", "round_robin"])
def test_quadrant_skew(gpu_device, order):
    """300 faint splats (opacity 1 %: the alpha >= 1/255 region reaches 0.86 px) at the centre of ONE quadrant each: one queue
    fills while three stay empty (pops with fewer than 16 entries, the dummy slot), then the four in turn along the list."""
    n = 300
    g = torch.Generator().manual_seed(11)
    quad = torch.zeros(n, dtype=torch.long) + 3 if order == "one_quadrant" else torch.arange(n) % 4
    px = 4.0 * (quad & 1) + 1.3 + 0.4 * torch.rand(n, generator=g)
    py = 4.0 * (quad >> 1) + 1.3 + 0.4 * torch.rand(n, generator=g)
    scene, cam = _scene_at(16, 16, px, py, torch.full((n,), 0.01), seed=12)
    if order == "round_robin":                            # the quadrant follows the DEPTH order, which is the list order
        scene["means3D"] = scene["means3D"] / scene["means3D"][:, 2:3] * (1.0 + 0.01 * torch.arange(n))[:, None]
        scene["scales"] = (0.3 * scene["means3D"][:, 2:3] / 8.0).repeat(1, 3).contiguous()
    got = _compare(scene, cam, gpu_device, lengths=(n, 0, 0, 0), backward=True)
    assert torch.equal(got["qmask"].long(), 1 << quad[got["gid"]]), "every splat reaches exactly its own quadrant"


def test_frame_that_is_no_multiple_of_the_tile(gpu_device):
    """20 x 12: the right-hand tiles have four live columns, the lower ones four live rows (off-image lanes pop and step too)."""
    g = torch.Generator().manual_seed(21)
    n = 700
    px, py = torch.rand(n, generator=g) * 21 - 1, torch.rand(n, generator=g) * 13 - 1
    scene, cam = _scene_at(20, 12, px, py, 0.05 + 0.5 * torch.rand(n, generator=g), seed=22, sigma_px=0.8)
    _compare(scene, cam, gpu_device)


def test_clamped_splats_and_a_pixel_that_ends_with_chunks_in_flight(gpu_device):
    """Opacity 0.99 mixed into the lists (the chunks' `hot` flags, the clamped sweeps) and 40 opaque splats stacked on one
    pixel in front of everything else in their tile: its pixels end in the first steps (exact sweep, `done`), the tile's
    other pixels go on, and the block's other tiles break out early or not at all."""
    g = torch.Generator().manual_seed(31)
    base, cam = _in_tiles((150, 200, 70, 260), seed=32)
    n = base["opacities"].numel()
    hot = torch.rand(n, generator=g) < 0.1
    base["opacities"][hot] = 0.99
    stack, _ = _scene_at(16, 16, torch.full((40,), 12.0), torch.full((40,), 4.0), torch.full((40,), 0.99), seed=33, sigma_px=2.0)
    stack["means3D"] = stack["means3D"] / stack["means3D"][:, 2:3] * (0.5 + 0.005 * torch.arange(40))[:, None]
    stack["scales"] = (2.0 * stack["means3D"][:, 2:3] / 8.0).repeat(1, 3).contiguous()
    scene = {k: torch.cat([base[k], stack[k]]).contiguous() for k in base}
    _compare(scene, cam, gpu_device, backward=True)


# ---- the same hand-placed frames through the other two kernel modes: composite_forward_q<1> (dual render, six payload columns,
# a second payload table read through the popped slots) and <2> (the [z, 1, z^2] contract forward, z in the depth column) --------
def _frame_params(scene, dev):
    """The scene as the caller chain's parameter dict with an IDENTITY camera transform at every time index, so that
    render_frame composites exactly the hand-placed splats (opacity through logit -> sigmoid and scale through log -> exp move
    by an ulp: 1e-7 px of reach against >= 1 px of clearance)."""
    o = scene["opacities"].double()
    p = {"means3D": scene["means3D"], "rgb_colors": scene["colors_precomp"], "unnorm_rotations": scene["rotations"],
         "logit_opacities": torch.log(o / (1 - o)).float(), "log_scales": torch.log(scene["scales"][:, :1]),
         "cam_unnorm_rots": torch.tensor([1.0, 0, 0, 0]).reshape(1, 4, 1).repeat(1, 1, 3), "cam_trans": torch.zeros(1, 3, 3)}
    return {k: torch.nn.Parameter(v.contiguous().to(dev)) for k, v in p.items()}


@pytest.mark.parametrize("lengths", CASE1)
def test_dual_render_on_the_hand_placed_lists(gpu_device, monkeypatch, lengths):
    """The cross-check of tests/test_gpu_fused_frame.py::test_dual_composite_equals_two_renders on case 1: the one-pass dual
    render (VTGS_DUAL = 1, the default) against two single renders over shared bins and two backwards (VTGS_DUAL = 0): images and
    radii bit-identical, gradients equal up to float32 summation order (2e-4 of each tensor's largest gradient)."""
    from diff_gaussian_rasterization.fused import render_frame
    dev = gpu_device
    scene, cam = _in_tiles(lengths, seed=sum(lengths))
    params = _frame_params(scene, dev)
    st = to_settings(cam, dev, bg=torch.tensor([0.3, 0.1, 0.7]))
    w2c = torch.eye(4, device=dev)
    g = torch.Generator().manual_seed(4)
    g1 = (torch.rand(3, 16, 16, generator=g) * 2 - 1).to(dev)
    g2 = (torch.rand(3, 16, 16, generator=g) * 2 - 1).to(dev)
    res = {}
    for mode in ("0", "1"):
        monkeypatch.setenv("VTGS_DUAL", mode)
        for v in params.values():
            v.grad = None
        im, ds, radii = render_frame(params, 1, st, w2c, True, True)
        ((im * g1).sum() + (ds * g2).sum()).backward()
        res[mode] = (im.detach().clone(), ds.detach().clone(), radii.clone(), {k: v.grad.clone() for k, v in params.items()})
    assert int((res["1"][2] > 0).sum()) == sum(lengths), "every hand-placed splat is on screen"
    assert torch.equal(res["0"][0], res["1"][0]) and torch.equal(res["0"][1], res["1"][1]) and torch.equal(res["0"][2], res["1"][2])
    for k in params:
        a, b = res["0"][3][k], res["1"][3][k]
        if k == "unnorm_rotations":                       # isotropic: float noise around zero in both routes
            continue
        assert (a - b).abs().max().item() <= 2e-4 * a.abs().max().item() + 1e-7, (k, (a - b).abs().max().item())


@pytest.mark.parametrize("lengths", CASE1)
def test_contract_forward_on_the_hand_placed_lists(gpu_device, lengths):
    """The cross-check of tests/test_gpu_fused_frame.py::test_get_loss_contract_forward_against_the_full_dual_forward on case 1:
    the depth-column forward against the full dual forward (VTGS_DEPTH_LITE = 0): colour image and plane 0 bit-identical, plane 1
    (1 - T_final against sum w) within 2e-6, plane 2 exactly plane 0 squared."""
    import diff_gaussian_rasterization as dgr
    from diff_gaussian_rasterization.fused import render_frame
    dev = gpu_device
    scene, cam = _in_tiles(lengths, seed=sum(lengths))
    params = _frame_params(scene, dev)
    st = to_settings(cam, dev, bg=torch.tensor([0.1, 0.2, 0.3]))
    w2c = torch.eye(4, device=dev)
    out = {}
    try:
        for lite in (0, 1):
            assert dgr._lib.vtgs_set_option(b"VTGS_DEPTH_LITE", lite) == 0
            with torch.no_grad():
                out[lite] = render_frame(params, 1, st, w2c, False, False, get_loss_contract=True)
    finally:
        dgr._lib.vtgs_set_option(b"VTGS_DEPTH_LITE", -1)
    (im0, ds0, r0), (im1, ds1, r1) = out[0], out[1]
    assert torch.equal(im0, im1) and torch.equal(r0, r1)
    assert torch.equal(ds0[0], ds1[0])
    assert (ds0[1] - ds1[1]).abs().max().item() <= 2e-6
    assert torch.equal(ds1[2], ds1[0] * ds1[0])
    assert torch.isfinite(ds0[2] - ds0[0] ** 2).all()
