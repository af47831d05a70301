"""vtgs_tracking_mask (csrc/vtgs_masks.hip) through `losses.tracking_extra_mask`: the visibility decision against the
reference's own masks (tests/golden/get_loss.npz) and against the float64 restatement on synthetic frames with hand-placed
edge situations, by the band rule of tests/tracking_mask_util.py; the far filter and the outlier mask bit for bit against
torch; `get_loss` with NATIVE_MASKS against the torch route.

Measured on the CPU (tracking_mask_util.measure_tau): the float32 torch route disagrees with the float64 restatement on
no pixel of these cases (worst margin 0), so tau is its floor of 4 float32 ulps = 4.77e-7; in-band pixels: none in any case.
That the call makes no host wait is established from the kernel trace and the host-return time in
profiles/tracking_mask_timing.md (the repository's tests have no pattern for that claim)."""
import pytest
import torch

import tracking_mask_util as tm

SYNTHETIC = ("s67x45", "s256x4")
SUBSETS = ([], [0], [1, 2], [0, 3, 1], [2, 3, 0])        # frames of the pool A B C D: 0, 1, 2 and 3 overlaps


def _native(c, frames, dev, **kw):
    from diff_gaussian_rasterization.losses import tracking_extra_mask
    ov = [(c["frames"][j][0].to(dev), c["frames"][j][1].to(dev)) for j in frames]
    out, u8, bits = tracking_extra_mask(c["gt"].to(dev), c["k"].to(dev), c["curr_w2c"].to(dev) if frames else None, ov, tm.THRES,
                                        return_parts=True, **kw)
    H, W = c["gt"].shape[-2:]
    assert out.shape == (1, H, W) and out.dtype == torch.float32 and u8.shape == (H, W) and u8.dtype == torch.bool
    out, u8, bits = out.cpu(), u8.cpu(), bits.cpu()
    assert bool(((out == 0) | (out == 1)).all()) and torch.equal(out[0] != 0, u8)       # float and byte outputs agree
    return out, u8, bits


def test_cases_are_not_vacuous_and_stay_under_the_band_cap():
    """CPU, float64 restatement alone: every hand-placed situation occurs, every case keeps its in-band share under
    BAND_SHARE (asserted inside band_of), tau obeys its floor."""
    tau, worst, floor = tm.measure_tau()
    print("tau", tau, "worst disagreeing margin", worst, "floor", floor)
    assert tau >= floor and tau == max(4 * worst, floor) and tau < 1e-3
    shares = tm.band_shares()
    print("in-band shares", shares)
    assert all(s <= tm.BAND_SHARE for s in shares.values())
    for name in SYNTHETIC:
        s = tm.situations(name)
        print(name, s)
        assert all(v > 0 for v in s.values()), (name, {k: v for k, v in s.items() if v <= 0})
    g = tm.cases()["golden"]
    for r, ref in zip(tm.f64_of("golden"), g["ref"]):                 # the float64 restatement restates the reference
        diff = r["vis"] != ref
        assert bool((r["margin"][diff].abs() < tau).all())
        assert 0.05 < ref.double().mean().item() < 0.999


@pytest.mark.gpu
def test_reference_fixture_per_overlap_bits_and_or(gpu_device):
    c = tm.cases()["golden"]
    tau = tm.measure_tau()[0]
    out, u8, bits = _native(c, [0, 1, 2], gpu_device)
    want_or = torch.zeros_like(u8)
    for j, (r, ref) in enumerate(zip(tm.f64_of("golden"), c["ref"])):
        got = ((bits >> j) & 1).bool()
        diff = got != ref
        print("overlap", j, "differs from the reference at", int(diff.sum()), "pixels; margins", r["margin"][diff].tolist())
        assert bool((r["margin"][diff].abs() < tau).all()), (j, r["margin"][diff].abs().max().item(), tau)
        want_or |= ref
        one = _native(c, [j], gpu_device)
        assert torch.equal((one[2] & 1).bool(), got) and torch.equal(one[1], got)          # alone: the same decision, bit 0
    assert bool((bits >> 3 == 0).all())
    assert torch.equal(u8, bits != 0)
    assert bool(((u8 != want_or) <= tm.band_of("golden", [0, 1, 2])).all())


@pytest.mark.gpu
@pytest.mark.parametrize("name", SYNTHETIC)
@pytest.mark.parametrize("frames", SUBSETS, ids=lambda f: "n%d_%s" % (len(f), "".join("ABCD"[j] for j in f)))
def test_synthetic_edges_against_float64(gpu_device, name, frames):
    c, rs = tm.cases()[name], tm.f64_of(name)
    tau = tm.measure_tau()[0]
    out, u8, bits = _native(c, frames, gpu_device)
    if not frames:
        assert bool((out == 1).all()) and bool((bits == 0).all())      # nothing requested: ones
        return
    want_or = torch.zeros_like(u8)
    for slot, j in enumerate(frames):
        got = ((bits >> slot) & 1).bool()
        diff = got != rs[j]["vis"]
        print(name, "frame", "ABCD"[j], "differs at", int(diff.sum()), "margins", rs[j]["margin"][diff].tolist())
        assert bool((rs[j]["margin"][diff].abs() < tau).all()), (j, rs[j]["margin"][diff].abs().max().item(), tau)
        want_or |= rs[j]["vis"]
    assert bool((bits >> len(frames) == 0).all()) and torch.equal(u8, bits != 0)
    assert bool(((u8 != want_or) <= tm.band_of(name, frames)).all())
    for r, col in c["invalid"]:                                         # gt < 0 and NaN: 0 in the mask
        assert out[0, r, col] == 0 and bits[r, col] == 0
    if 2 in frames and len(frames) == 2:
        assert int(((bits >> 1) & 1).sum()) == 0                        # C looks the other way: z' < 0, nothing visible


def _exact_case(W, H, variant):
    g = torch.Generator().manual_seed(W * 31 + H)
    gt = 1.0 + 2.0 * torch.rand(1, H, W, generator=g)
    gt[torch.rand(1, H, W, generator=g) < (0.6 if variant == "mostly_zero" else 0.1)] = 0.0
    rd = gt * (1.0 + 0.01 * torch.randn(1, H, W, generator=g)) + 0.003 * torch.randn(1, H, W, generator=g)
    if variant == "patch":
        gt[:, H // 2:H // 2 + 2, W // 3:W // 3 + 20] *= 60.0            # the outlier patch of test_get_loss_mirror.py
    if variant == "nan":
        rd[0, H // 2, W // 2] = float("nan")
    return gt, rd


@pytest.mark.gpu
@pytest.mark.parametrize("W,H", [(67, 45), (256, 4)], ids=["odd_3015", "even_1024"])
@pytest.mark.parametrize("variant", ["plain", "mostly_zero", "nan", "patch"])
def test_far_filter_and_outlier_mask_equal_torch_bit_for_bit(gpu_device, W, H, variant):
    from diff_gaussian_rasterization import losses
    dev = gpu_device
    gt, rd = _exact_case(W, H, variant)
    gt, rd = gt.to(dev), rd.to(dev)
    far = 2.2
    want_far, want_out = losses.far_depth_mask(gt, far), losses.outlier_depth_mask(gt, rd)
    both = losses.tracking_extra_mask(gt, None, None, [], far_depth_filter_thres=far, rendered_depth=rd)
    assert torch.equal(both != 0, want_far & want_out) and bool(((both == 0) | (both == 1)).all())
    only_far = losses.tracking_extra_mask(gt, None, None, [], far_depth_filter_thres=far)
    only_out = losses.tracking_extra_mask(gt, None, None, [], rendered_depth=rd)
    assert torch.equal(only_far != 0, want_far) and torch.equal(only_out != 0, want_out)
    kept = int(want_out.sum())
    print(variant, W, H, "outlier mask keeps", kept, "far keeps", int(want_far.sum()))
    if variant in ("mostly_zero", "nan"):
        assert kept == 0 and int((only_out != 0).sum()) == 0           # median 0 / NaN median: everything masked off
    else:
        assert 0 < kept < W * H and 0 < int(want_far.sum()) < W * H
    if variant == "patch":
        assert not bool(want_out[:, H // 2:H // 2 + 2, W // 3:W // 3 + 20].any())


@pytest.mark.gpu
@pytest.mark.parametrize("name", SYNTHETIC + ("golden",))
def test_all_three_masks_are_the_and_of_the_parts(gpu_device, name):
    from diff_gaussian_rasterization import losses
    c = dict(tm.cases()[name])
    c["gt"] = torch.nan_to_num(c["gt"], nan=0.0)        # a NaN in gt makes the median NaN and the whole mask 0 (tested above)
    frames = [0, 1, 2]
    g = torch.Generator().manual_seed(9)
    rd = (c["gt"] * (1.0 + 0.02 * torch.randn(c["gt"].shape, generator=g))).to(gpu_device)
    far = float(c["gt"][c["gt"] > 0].median())                          # cuts about half of the frame
    out, u8, bits = _native(c, frames, gpu_device, far_depth_filter_thres=far, rendered_depth=rd)
    vis = _native(c, frames, gpu_device)[1]
    gt = c["gt"].to(gpu_device)
    parts = losses.tracking_extra_mask(gt, None, None, [], far_depth_filter_thres=far, rendered_depth=rd).cpu()[0] != 0
    assert torch.equal(u8, vis & parts) and torch.equal(bits != 0, vis)
    assert 0 < int(u8.sum()) < int(vis.sum())
    assert torch.equal(losses.visibility_mask_native(gt, c["k"].to(gpu_device), c["curr_w2c"].to(gpu_device),
                                                     [(w.to(gpu_device), d.to(gpu_device)) for w, d in c["frames"][:3]], tm.THRES).cpu(), vis)
    assert losses.visibility_mask_native(gt, c["k"], c["curr_w2c"], []) is None


def _scene(dev, n, W, H, seed):
    from oracle import gs_oracle as go
    from parity_util import to_settings
    scene, cam = go.view_tied_scene(n, W, H, seed=seed)
    T = 4
    g = torch.Generator().manual_seed(seed)
    params = {
        "means3D": scene["means3D"], "rgb_colors": scene["colors_precomp"], "unnorm_rotations": scene["rotations"] * 1.7,
        "logit_opacities": torch.logit(scene["opacities"].clamp(1e-4, 1 - 1e-4)), "log_scales": torch.log(scene["scales"][:, :1]),
        "cam_unnorm_rots": torch.tensor([1.0, 0.01, -0.02, 0.005]).reshape(1, 4, 1).repeat(1, 1, T),
        "cam_trans": (0.01 * torch.randn(1, 3, T, generator=g)),
    }
    params = {k: torch.nn.Parameter(v.to(dev).float().contiguous()) for k, v in params.items()}
    k = torch.tensor([[W / 2.0, 0, W / 2.0 - 0.5], [0, W / 2.0, H / 2.0 - 0.5], [0, 0, 1]])
    return params, to_settings(cam, dev), k


@pytest.mark.gpu
@pytest.mark.parametrize("dataset,outlier,far,n_over", [("tum", False, 5.0, 1), ("scannet", True, 6.0, 3)])
def test_get_loss_with_native_masks_equals_the_torch_route(gpu_device, dataset, outlier, far, n_over):
    """The tum and scannet cases of test_get_loss_mirror.py's scene.  The two masks are compared first: they may differ
    only at in-band pixels (float64 restatement of this scene); when they are equal, loss and gradients are equal."""
    import diff_gaussian_rasterization as dgr
    import slam_callers as sc
    from diff_gaussian_rasterization import get_loss as gl
    from diff_gaussian_rasterization import losses
    dev = gpu_device
    W, H, N = 160, 120, 24000
    params, st, K = _scene(dev, N, W, H, seed=17)
    g = torch.Generator().manual_seed(2)
    w2c0 = torch.eye(4, device=dev)
    with torch.no_grad():
        gt_p = {k: v.detach().clone() for k, v in params.items()}
        gt_p["cam_trans"] = gt_p["cam_trans"] + 0.004
        tg = sc.transform_to_frame(gt_p, 1, False, False)
        gim, _, _ = dgr.GaussianRasterizer(raster_settings=st)(**sc.transformed_params2rendervar(gt_p, tg))
        gds, _, _ = dgr.GaussianRasterizer(raster_settings=st)(**sc.transformed_params2depthplussilhouette(gt_p, w2c0, tg))
        gt_im = (gim + 0.03 * torch.randn(3, H, W, generator=g).to(dev)).clamp(0, 1)
        gt_depth = torch.where(gds[1:2] > 0.5, gds[0:1] / gds[1:2].clamp(min=1e-6), torch.zeros_like(gds[0:1]))
        gt_depth[:, 30:40, 50:70] = 0.0
        gt_depth[:, 80:84, 20:40] *= 60.0
    curr = {"cam": st, "im": gt_im, "depth": gt_depth, "w2c": w2c0, "intrinsics": K.to(dev), "id": 1}
    weights = {"im": 0.5, "depth": 1.0}
    curr_w2c = torch.eye(4, device=dev)
    overlaps = []
    for i in range(3):
        o = torch.eye(4, device=dev)
        o[:3, 3] = torch.tensor([0.03 * (i + 1), -0.02, 0.01 * i], device=dev)
        overlaps.append((o, (gt_depth * (1.0 + 0.02 * i)).clone()))
    okw = dict(curr_w2c=curr_w2c, overlap_w2c=overlaps[0][0], overlap_gtdepth=overlaps[0][1])
    if n_over == 3:
        okw.update(overlap_mid_w2c=overlaps[1][0], overlap_mid_gtdepth=overlaps[1][1],
                   overlap_last_w2c=overlaps[2][0], overlap_last_gtdepth=overlaps[2][1])

    # the masks first: torch route against the native call, band from the float64 restatement of this scene
    m_torch = losses.visibility_mask(gt_depth, K.to(dev), curr_w2c, overlaps[:n_over], 0.05).cpu()
    m_native = losses.visibility_mask_native(gt_depth, K.to(dev), curr_w2c, overlaps[:n_over], 0.05).cpu()
    tau = tm.measure_tau()[0]
    band = torch.zeros(H, W, dtype=torch.bool)
    for w, d in overlaps[:n_over]:
        band |= tm.vis_f64(gt_depth.cpu(), K, curr_w2c.cpu(), w.cpu(), d.cpu())["margin"].abs() < tau
    differ = m_torch != m_native
    print(dataset, "masks differ at", int(differ.sum()), "pixels; in band", int(band.sum()))
    assert bool((differ <= band).all()) and band.double().mean().item() <= tm.BAND_SHARE
    assert 0 < int(m_native.sum()) < H * W

    def run(native):
        variables = {"max_2D_radius": torch.zeros(N, device=dev), "means2D_gradient_accum": torch.zeros(N, device=dev),
                     "denom": torch.zeros(N, device=dev)}
        for v in params.values():
            v.grad = None
        before = gl.NATIVE_MASKS
        try:
            gl.NATIVE_MASKS = native
            out = gl.get_loss(params, curr, variables, 1, weights, True, 0.9, True, outlier, tracking=True, tracking_iteration=1,
                              dataset_name=dataset, far_depth_filter_thres=far, **okw)
        finally:
            gl.NATIVE_MASKS = before
        out[0].backward()
        return out[0].item(), {k: (None if v.grad is None else v.grad.clone()) for k, v in params.items()}

    assert gl.NATIVE_MASKS is False                                        # off by default
    loss_t, grads_t = run(False)
    loss_n, grads_n = run(True)
    assert gl.NATIVE_MASKS is False
    assert loss_n == loss_n and loss_t == loss_t                          # finite
    if not bool(differ.any()):
        # equal masks: the same loss node over the same inputs.  The bounds are those tests/test_get_loss_mirror.py holds the
        # same function to against its unfused composition (the backward sums with float atomics: not bitwise repeatable)
        assert abs(loss_n - loss_t) <= 2e-5 * abs(loss_t), (loss_n, loss_t)
        for k in grads_t:
            assert (grads_t[k] is None) == (grads_n[k] is None), k
            if grads_t[k] is None or k == "unnorm_rotations":
                continue
            scale = grads_t[k].abs().max().item()
            assert (grads_t[k] - grads_n[k]).abs().max().item() <= 2e-3 * scale + 1e-7, k
