"""Which kernel instantiation the host layer launches (csrc/vtgs_api.hip: one table of kernel pointers, one launch per kernel).

Every reachable cell of the binning table [LDS][MODE] and every branch of the forward-composite, backward-composite and gather
choices runs here once at a small shape and is compared with another route to the same numbers.  A wrong cell shows in the
outputs: a band kernel's tile counts stop at the band, a planned kernel follows the plan's offsets, a cov3D kernel reads six
floats per Gaussian, a dual kernel writes a second image.

Where each branch is reached (here = this file; the others are the tests that check the same branch at full size):

    project_and_bin[_capped]<LDS, MODE>   LDS 0, 1, 2 x whole frame, band, planned, planned band, cov3D, cov3D band: here
                                          (test_binning_cells); LDS 1 above 64 KB: here (test_raised_lds_table);
                                          LDS 2 at its real size: test_gpu_planned_bins::test_windowed_tile_table_equals_global_atomic_bins
    bin_deferred_splats<PLANNED>          false / true: here (every uniform / planned cell); with deferred splats:
                                          test_gpu_tier_edges, test_gpu_no_defer_hint
    composite_forward_q<0>                here (every binning cell; the VTGS_DUAL=0 route of test_frame_branches)
    composite_forward_q<1>                here (dual, dual_two_kernel, b1_off's forward with VTGS_DEPTH_LITE=0)
    composite_forward_q<2>                here (contract); test_gpu_fused_frame::test_get_loss_contract_forward_against_the_full_dual_forward
    composite_backward_mx<4, false, true>          here (binning cells' backward, VTGS_DUAL=0 route)
    composite_backward_mx<4, true, true, false>    here (dual, dual_two_kernel, contract with VTGS_DUAL_B1=0)
    composite_backward_mx<4, true, true, true>     here (contract); test_gpu_fused_frame::test_depth_only_backward_equals_the_full_dual_backward
    gather_splat_grads<false>                      here (binning cells' backward, VTGS_DUAL=0 route)
    gather_splat_grads<false, false, true>         here (cov3D cells' backward); test_gpu_surface::test_cov3d_precomp_against_the_oracle
    gather_splat_grads<true>                       here (dual_two_kernel: VTGS_FRAME_EPILOGUE=0)
    gather_splat_grads<true, true>                 here (dual; contract with VTGS_DUAL_B1=0)
    gather_splat_grads<true, true, false, true>    here (contract)
    g_colors not requested (bwd_flags bit 0)       here (tracking: no appearance gradient, frame flag 4 clear)
    lower_median_pass<0|1|2>                       test_gpu_median, test_gpu_densify, test_gpu_tracking_mask
    the empty dual render                          test_gpu_owned_sets::test_an_empty_list_renders_the_background
"""
import types

import pytest
import torch

from oracle import gs_oracle as go
from parity_util import oracle_instances_8x8, to_settings

pytestmark = pytest.mark.gpu

W, H, N = 160, 120, 3000
BAND = (2, 5)                                    # of the 8 rows of 16x16 tiles
MODES = ("whole", "band", "planned", "planned_band", "cov3d", "cov3d_band")
CELL_KEYS = ("color", "depth", "radii", "offs", "gid", "instances")


@pytest.fixture(scope="module")
def tied_scene():
    return go.view_tied_scene(N, W, H, seed=N % 89)


def _cov6(scales, rotations):
    R = go.quat_to_rotmat(torch.nn.functional.normalize(rotations).double())
    S = R @ torch.diag_embed(scales.double() ** 2) @ R.transpose(1, 2)
    return torch.stack([S[:, 0, 0], S[:, 0, 1], S[:, 0, 2], S[:, 1, 1], S[:, 1, 2], S[:, 2, 2]], 1).float()


def _render(dgr, dev, scene, cam, mode, grad_color=None):
    """One forward (and backward, with grad_color) of the operator in `mode`: its images, radii, instance count, the sorted
    8x8 tile lists and the gradients, on the CPU."""
    band = BAND if mode.endswith("band") else None
    dgr._BINS_MODE = "planned" if mode.startswith("planned") else "uniform"
    rast = dgr.GaussianRasterizer(raster_settings=to_settings(cam, dev), tile_rows=band)
    leaves = {k: v.to(dev).clone().requires_grad_(True) for k, v in scene.items()}
    if mode.startswith("cov3d"):
        del leaves["scales"], leaves["rotations"]
        leaves["cov3D_precomp"] = _cov6(scene["scales"], scene["rotations"]).to(dev).requires_grad_(True)
        color, radii, depth = rast(**leaves)
        fs = color.grad_fn.fs                      # (this path keeps its forward state on the autograd node only)
        instances = fs._instances
    else:
        color, radii, depth = rast(**leaves)
        fs = rast._last_state
        instances = dgr.last_forward_info()["instances"]
        assert bool(fs.tile_cap & dgr.PLANNED) == mode.startswith("planned")
    offs, gid, geom = dgr.debug_tile_lists(types.SimpleNamespace(_last_state=fs))
    out = {"color": color.detach().cpu(), "depth": depth.detach().cpu(), "radii": radii.cpu(), "offs": offs, "gid": gid,
           "instances": instances, "geom": geom, "grads": {}}
    if grad_color is not None:
        color.backward(grad_color.to(dev))
        dgr.settle_pending()
        out["grads"] = {k: v.grad.cpu() for k, v in leaves.items() if v.grad is not None}
    return out


def _same_cell(a, b, what):
    for k in CELL_KEYS:
        assert (a[k] == b[k]) if k == "instances" else torch.equal(a[k], b[k]), (what, k)
    assert a["grads"].keys() == b["grads"].keys()
    for k in a["grads"]:
        assert torch.equal(a["grads"][k], b["grads"][k]), (what, k)


def test_binning_cells(gpu_device, tied_scene, monkeypatch):
    """VTGS_BIN_IMPL 0 / 1 / 2 (global atomics, the tile table in LDS, the windowed table) x the six forms of the projection
    kernel: images, radii, instance count, tile lists and gradients of rows 1 and 2 of the table are bit-equal to row 0 of the
    same form (cov3D has no windowed form: VTGS_BIN_IMPL = 2 falls back to row 0 there, as the library documents).  Row 0 of the
    whole frame is pinned to the oracle's lists, as test_gpu_configs::test_tile_lists_equal_the_oracle_lists does."""
    import diff_gaussian_rasterization as dgr
    scene, cam = tied_scene
    monkeypatch.setattr(dgr, "_BINS_MODE", "uniform")                     # (_render sets it per mode; restored after the test)
    grad_color = torch.rand(3, H, W, generator=torch.Generator().manual_seed(1)) * 2 - 1
    ref = {}
    try:
        for impl in (0, 1, 2):
            dgr.set_option("VTGS_BIN_IMPL", impl)
            for mode in MODES:
                got = _render(dgr, gpu_device, scene, cam, mode, grad_color)
                if impl == 0:
                    ref[mode] = got
                    assert got["instances"] > 0 and int(got["offs"][-1]) == got["instances"]
                else:
                    _same_cell(ref[mode], got, (impl, mode))
    finally:
        dgr.reset_options()
    # a band's lists stop at the band; the whole frame has entries outside it
    gx8 = (W + 7) // 8
    lens = ref["band"]["offs"][1:] - ref["band"]["offs"][:-1]
    assert int(lens[:2 * BAND[0] * gx8].sum()) == 0 and int(lens[2 * BAND[1] * gx8:].sum()) == 0 and int(lens.sum()) > 0
    assert ref["whole"]["instances"] > ref["band"]["instances"]
    # planned and uniform bins hold the same lists
    for a, b in (("whole", "planned"), ("band", "planned_band")):
        _same_cell(ref[a], ref[b], (a, b))
    # the whole frame against the oracle: strict set <= kernel set <= loose set, depth bits and order (see the test named above)
    whole = ref["whole"]
    with torch.no_grad():
        f = {k: v.double() for k, v in scene.items()}
        sp = go.preprocess(f["means3D"], f["means2D"], f["opacities"], f["scales"], f["rotations"], cam, "3sigma")
    same_rect = sp.radii == whole["radii"]
    assert (~same_rect).double().mean().item() <= 1e-3
    offs, gid, geom = whole["offs"], whole["gid"], whole["geom"]
    lens = offs[1:] - offs[:-1]
    tile_of = torch.repeat_interleave(torch.arange(lens.numel()), lens)
    keep = lambda keys: keys[same_rect[keys & 0xFFFFFFFF]]
    hip = keep((tile_of << 32) | gid)
    strict = keep(oracle_instances_8x8(sp, scene["opacities"], cam))
    loose = keep(oracle_instances_8x8(sp, scene["opacities"], cam, 2e-4, 2e-4))
    assert bool(torch.isin(strict, hip).all()) and bool(torch.isin(hip, loose).all())
    binned = torch.unique(gid)
    assert torch.equal(geom[binned, 6].view(torch.int32), sp.zkey[binned].view(torch.int32))
    key = (geom[:, 6].view(torch.int32).long()[gid] << 32) | gid
    assert bool(((key[1:] > key[:-1]) | (tile_of[1:] != tile_of[:-1])).all())


@pytest.mark.parametrize("band", [None, (0, 58)])
def test_raised_lds_table(gpu_device, band):
    """A tile table between 64 KB and the 79 KB limit: the LDS row of the table needs its dynamic shared memory limit raised
    (once per device, for every kernel of the row).  1160x960 is 145 x 120 tiles of 8x8; the band keeps 116 of the 120 rows.
    Bit-equal to global atomics; the second pass of the loop takes the branch that remembers the raised limit."""
    import diff_gaussian_rasterization as dgr
    w, h = 1160, 960
    rows8 = (h + 7) // 8 if band is None else 2 * (band[1] - band[0])
    table_bytes = rows8 * ((w + 7) // 8) * 4
    assert table_bytes == (69600 if band is None else 67280) and (64 << 10) < table_bytes <= (79 << 10)
    scene, cam = go.view_tied_scene(4000, w, h, seed=17)
    dev = gpu_device
    st = to_settings(cam, dev)
    t = {k: v.to(dev) for k, v in scene.items()}
    out = []
    try:
        for impl in (0, 1, 1):
            dgr.set_option("VTGS_BIN_IMPL", impl)
            rast = dgr.GaussianRasterizer(raster_settings=st, tile_rows=band)
            with torch.no_grad():
                color, radii, depth = rast(**t)
            instances = dgr.last_forward_info()["instances"]
            offs, gid, _ = dgr.debug_tile_lists(rast)
            out.append({"color": color.cpu(), "depth": depth.cpu(), "radii": radii.cpu(), "offs": offs, "gid": gid,
                        "instances": instances, "grads": {}})
    finally:
        dgr.reset_options()
    assert out[0]["instances"] > 4000
    _same_cell(out[0], out[1], "first call")
    _same_cell(out[0], out[2], "second call")


def _frame_params(dev, appearance_grad=True):
    scene, cam = go.view_tied_scene(N, W, H, seed=9)
    g = torch.Generator().manual_seed(9)
    p = {"means3D": scene["means3D"], "rgb_colors": scene["colors_precomp"],
         "unnorm_rotations": scene["rotations"] * (1 + 0.3 * torch.rand(N, 1, generator=g)),
         "logit_opacities": torch.randn(N, 1, generator=g), "log_scales": torch.log(scene["scales"][:, :1]),
         "cam_unnorm_rots": torch.tensor([1.0, 0, 0, 0]).reshape(1, 4, 1).repeat(1, 1, 3) + 0.01 * torch.randn(1, 4, 3, generator=g),
         "cam_trans": 0.01 * torch.randn(1, 3, 3, generator=g)}
    appearance = ("rgb_colors", "logit_opacities", "log_scales")
    return {k: (torch.nn.Parameter(v.to(dev)) if appearance_grad or k not in appearance else v.to(dev)) for k, v in p.items()}, cam


def _close(a, b, tol, what):
    """Gradient dicts equal to `tol` of each tensor's largest gradient (the isotropic map's rotation gradient is float noise
    around an exact zero on every route: measured against the scale gradient, as in test_gpu_fused_frame)."""
    assert a.keys() == b.keys(), what
    for k in a:
        scale = (a["log_scales"] if k == "unnorm_rotations" and "log_scales" in a else a[k]).abs().max().item()
        assert (a[k] - b[k]).abs().max().item() <= tol * scale + 1e-12, (what, k, (a[k] - b[k]).abs().max().item(), scale)


def test_frame_branches(gpu_device, monkeypatch):
    """The three composite choices and the gather choice through fused.render_frame (Python node, so that the environment
    switches of the package pick the route), each against a second route to the same numbers.  The bounds are those of the
    full-size tests of test_gpu_fused_frame.py that compare the same pairs of routes (the lists here are shorter, so the rounding
    that those bounds allow for is no larger):
      two renders (VTGS_DUAL=0: single forward, shared second render, two single backwards) vs the dual render: images
        bit-identical, gradients to 2e-4 (float32 summation order);
      gather with the frame epilogue vs vtgs_backward_dual + vtgs_prepare_frame_backward (VTGS_FRAME_EPILOGUE=0): 4e-6, also
        with no appearance gradient asked for (the composite then skips the first colour set's chain, whose only product is the
        gradient nobody reads);
      the get_loss contract: forward MODE 2 against MODE 1 (VTGS_DEPTH_LITE=0): colour and plane 0 bit-identical, plane 1 to
        2e-6, plane 2 = plane 0 squared; the one-channel backward against the full one (VTGS_DUAL_B1=0): 2e-6."""
    import diff_gaussian_rasterization as dgr
    from diff_gaussian_rasterization.fused import render_frame
    dev = gpu_device
    monkeypatch.setenv("VTGS_FUSED_EXT", "0")
    st_cam = _frame_params(dev)[1]
    st = to_settings(st_cam, dev, bg=torch.tensor([0.3, 0.1, 0.7]))
    w2c = torch.eye(4, device=dev)
    w2c[:3, 3] = torch.tensor([0.02, -0.01, 0.03], device=dev)
    g = torch.Generator().manual_seed(4)
    g1 = (torch.rand(3, H, W, generator=g) * 2 - 1).to(dev)
    g2 = (torch.rand(3, H, W, generator=g) * 2 - 1).to(dev)
    g2_depth_only = g2.clone()
    g2_depth_only[1:] = 0.0

    def run(env=(), options=(), contract=False, gaussians_grad=True, appearance_grad=True, grad_b=g2):
        params, _ = _frame_params(dev, appearance_grad)
        for k in ("VTGS_DUAL", "VTGS_FRAME_EPILOGUE"):
            monkeypatch.setenv(k, dict(env).get(k, "1"))
        try:
            for name, value in options:
                assert dgr._lib.vtgs_set_option(name, value) == 0
            im, ds, radii = render_frame(params, 1, st, w2c, gaussians_grad, True, get_loss_contract=contract)
            ((im * g1).sum() + (ds * grad_b).sum()).backward()
        finally:
            dgr.reset_options()
            for name in (b"VTGS_DUAL_B1", b"VTGS_DEPTH_LITE"):          # (not in the package's list of options)
                dgr._lib.vtgs_set_option(name, -1)
        grads = {k: v.grad.clone() for k, v in params.items() if getattr(v, "grad", None) is not None}
        return im.detach().clone(), ds.detach().clone(), radii.clone(), grads

    dual = run()
    two_renders = run(env={"VTGS_DUAL": "0"})
    two_kernel = run(env={"VTGS_FRAME_EPILOGUE": "0"})
    assert len(dual[3]) == 7 and float(dual[1][1].max()) > 0.5
    for other in (two_renders, two_kernel):
        assert torch.equal(dual[0], other[0]) and torch.equal(dual[1], other[1]) and torch.equal(dual[2], other[2])
    _close({k: v for k, v in two_renders[3].items() if k != "unnorm_rotations"},
           {k: v for k, v in dual[3].items() if k != "unnorm_rotations"}, 2e-4, "two renders")
    _close(two_kernel[3], dual[3], 4e-6, "frame epilogue")
    # tracking without an appearance gradient: only the pose gradient leaves
    track = run(gaussians_grad=False, appearance_grad=False)
    track_two_kernel = run(env={"VTGS_FRAME_EPILOGUE": "0"}, gaussians_grad=False, appearance_grad=False)
    assert set(track[3]) == {"cam_unnorm_rots", "cam_trans"} and track[3]["cam_trans"].abs().max().item() > 0
    _close(track_two_kernel[3], track[3], 4e-6, "tracking")
    # the get_loss contract
    lite = run(contract=True, grad_b=g2_depth_only)
    full_forward = run(contract=True, grad_b=g2_depth_only, options=((b"VTGS_DEPTH_LITE", 0),))
    full_backward = run(contract=True, grad_b=g2_depth_only, options=((b"VTGS_DUAL_B1", 0),))
    assert torch.equal(lite[0], full_forward[0]) and torch.equal(lite[2], full_forward[2]) and torch.equal(lite[1][0], full_forward[1][0])
    assert torch.equal(full_forward[0], dual[0]) and torch.equal(full_forward[1], dual[1])
    assert (lite[1][1] - full_forward[1][1]).abs().max().item() <= 2e-6
    assert torch.equal(lite[1][2], lite[1][0] * lite[1][0])
    assert torch.equal(lite[0], full_backward[0]) and torch.equal(lite[1], full_backward[1])
    _close(full_backward[3], lite[3], 2e-6, "one-channel backward")
