"""CPU self-checks of tests/loss_ref.py: the hand-placed frames really put every pixel class on every float4 lane and in the
one-by-one tails that tests/test_gpu_loss_paths.py relies on, and the float64 references say what slam_callers (itself pinned
by reference fixtures) says where the two overlap."""
import numpy as np
import pytest
import torch

import loss_ref as lr
import slam_callers as sc

ALL = set(range(lr.N_CLASSES))
# the bands of the 8x6 frame whose one-by-one tails (two pixels each) hold all seven classes between them
TAIL_BANDS_8X6 = ((0, 1), (2, 3), (2, 5), (4, 7))


def test_every_class_on_every_lane_and_in_the_tails():
    for H, W in ((12, 20), (8, 6), (40, 36), (8, 129), (513, 513), (1026, 1024)):
        lanes, _ = lr.placement(lr.frame(H, W)["cls"], 0, H * W, vec=True)
        assert all(l == ALL for l in lanes), (H, W, lanes)
    for H, W in ((13, 19), (12, 20)):                       # odd P, and the alignment fallback: all pixels one by one
        lanes, tail = lr.placement(lr.frame(H, W)["cls"], 0, H * W, vec=False)
        assert tail == ALL and not any(lanes)
    cls = lr.frame(8, 6)["cls"]
    tails = set()
    for r0, r1 in TAIL_BANDS_8X6:
        assert (r0 * 6) % 4 == 0 and ((r1 - r0) * 6) % 4 == 2          # float4 groups, then a tail of two
        tails |= lr.placement(cls, r0 * 6, r1 * 6, vec=True)[1]
    assert tails == ALL
    lanes, tail = lr.placement(cls, 12, 30, vec=True)                  # rows (2, 5): 16 by fours plus a tail of 2
    assert all(len(l) == 4 for l in lanes) and len(tail) == 2


def test_the_classes_are_what_they_claim():
    f = lr.frame(12, 20)
    cls, ds, gd = f["cls"], f["ds"], f["gt_depth"][0]
    m0 = lr.mask_of(ds, f["gt_depth"], lr.SIL_THRES, 0, f["extra_mask"])
    m1 = lr.mask_of(ds, f["gt_depth"], lr.SIL_THRES, 1, f["extra_mask"])
    assert m0[(cls == lr.IN) | (cls == lr.EXACT_ZERO)].all() and not m0[(cls != lr.IN) & (cls != lr.EXACT_ZERO)].any()
    assert m1[cls == lr.SIL_AT_THRES].all() and not m0[cls == lr.SIL_AT_THRES].any()       # strict test, tracking only
    assert (ds[1][cls == lr.SIL_AT_THRES] == np.float32(0.95)).all() and (ds[1][cls != lr.SIL_AT_THRES] > lr.SIL_THRES).all()
    assert (gd[cls == lr.GT_ZERO] == 0).all() and torch.isnan(ds[0][cls == lr.NAN_DEPTH]).all()
    assert torch.isnan(ds[2][cls == lr.NAN_UNC]).all() and not torch.isnan(ds[0][cls == lr.NAN_UNC]).any()
    assert (f["extra_mask"][cls == lr.EXTRA_OUT] == 0).all() and (f["extra_mask"][cls != lr.EXTRA_OUT] == 1).all()
    assert lr.mask_of(ds, f["gt_depth"], lr.SIL_THRES, 0, None)[cls == lr.EXTRA_OUT].all()  # out by extra_mask alone
    ez = cls == lr.EXACT_ZERO
    assert (gd[ez] == ds[0][ez]).all() and ((f["gt_im"] == f["im"]).sum(0)[ez] == 1).all()
    t = lr.pixel_terms(f["im"], ds, f["gt_im"], f["gt_depth"], lr.SIL_THRES, 0, f["extra_mask"])
    assert (t["g_depth"][ez] == 0).all() and ((t["g_im"] == 0).sum(0)[ez] == 1).all()       # gradient 0, not +-w
    assert ((t["g_im"] != 0).sum(0)[cls == lr.IN] == 3).all()
    assert sorted(set(lr.color_weight(f).flatten().tolist())) == [float(np.float32(0.8)), float(np.float32(10.8))]


@pytest.mark.parametrize("shape", [(13, 19), (40, 36)])
def test_references_agree_with_the_restatement(shape):
    f = lr.frame(*shape)
    im, ds, gt_im, gd = (f[k].double() for k in ("im", "ds", "gt_im", "gt_depth"))
    out, _, _, _ = lr.loss_reference(f, 0, 0.7, 1.3, use_extra=False)
    w = lambda x: float(np.float32(x))
    assert lr.rel(out[0], sc.tracking_loss(im, ds, gt_im, gd, lr.SIL_THRES, w(0.7), w(1.3)).item()) < 1e-12
    imr = im.clone().requires_grad_(True)
    ref = sc.mapping_loss(imr, ds, gt_im, gd, w(0.7), w(1.3))
    ref.backward()
    out, _, ssim_sum, g = lr.loss_reference(f, 1, 0.7, 1.3, use_extra=False, want_grad=True)
    assert lr.rel(out[0], ref.item()) < 1e-12 and (g - imr.grad).abs().max().item() < 1e-15
    assert lr.rel(out[4], sc.calc_ssim(im, gt_im).item()) < 1e-12
    # bands: the shares of a partition add up to the loss
    H = shape[0]
    cuts = [0, 3, H // 2, H]
    shares = [lr.loss_reference(f, 1, 0.7, 1.3, use_weight=True, rows=(a, b), count_all=lr.loss_reference(f, 1, 0.7, 1.3, use_weight=True)[1]["count"],
                                first_band=(a == 0))[0][0] for a, b in zip(cuts[:-1], cuts[1:])]
    assert lr.rel(sum(shares), lr.loss_reference(f, 1, 0.7, 1.3, use_weight=True)[0][0]) < 1e-12


def test_bookkeeping_alignment_is_refused_before_any_device_work():
    """No device here: the status must come from the host check alone (addresses are never dereferenced)."""
    import diff_gaussian_rasterization as dgr
    from diff_gaussian_rasterization import losses  # noqa: F401  (declares the signatures)
    lib, a = dgr._lib, 0x10000
    for radii, mx, seen in ((a + 4, a, a), (a, a + 8, a), (a, a, a + 1), (a, a, a + 2)):
        assert lib.vtgs_seen_and_max_radius(5, radii, mx, seen, None) == 1
        assert lib.vtgs_slam_loss_forward_seen(0, a, a, a, a, 2, 2, 0.5, 1.0, 1.0, a, None, a, None, None, 5, radii, mx, seen, None) == 1
    assert lib.vtgs_seen_and_max_radius(0, a + 4, a + 4, a + 1, None) == 0      # n = 0 touches nothing


def test_adam_and_bookkeeping_references():
    p, g = np.array([1.0, -2.0, 0.5]), np.array([0.1, 0.0, -3.0])
    p1, m1, v1 = lr.adam_reference(p, g, np.zeros(3), np.zeros(3), 1e-3, 1e-8, 0.9, 0.999, 1)
    # first step from zero moments: m / (1 - b1) = g, sqrt(v / (1 - b2)) = |g|  ->  the step is lr * sign(g)
    np.testing.assert_allclose(p1 - p, -float(np.float32(1e-3)) * np.sign(g), rtol=1e-6)
    t = torch.tensor(p, dtype=torch.float64, requires_grad=True)
    opt = torch.optim.Adam([t], lr=float(np.float32(1e-3)), betas=(float(np.float32(0.9)), float(np.float32(0.999))), eps=float(np.float32(1e-8)))
    m, v, q = np.zeros(3), np.zeros(3), p
    for step in (1, 2, 3):
        t.grad = torch.tensor(g * step, dtype=torch.float64)
        opt.step()
        q, m, v = lr.adam_reference(q, g * step, m, v, 1e-3, 1e-8, 0.9, 0.999, step)
    np.testing.assert_allclose(q, t.detach().numpy(), rtol=1e-13)
    seen, mx = lr.bookkeeping_reference([0, 3, 7], [2.5, 2.5, 9.0])
    assert seen.tolist() == [0, 1, 1] and mx.tolist() == [2.5, 3.0, 9.0]
