"""csrc/vtgs_loss.hip on both of its code paths and on every tail: the masked L1 sums, the whole loss forward and backward,
the band forms, the silhouette sweep and the seen / max-radius bookkeeping against the float64 statements of
tests/loss_ref.py, on frames whose pixel classes are placed by hand (tests/test_loss_ref_placement.py proves the placement on
the CPU).  The float4 path needs a plane stride and band start that are multiples of 4 and 16-byte bases; everything else
takes the one-by-one path.  The C entry points are called directly wherever the test has to own the output buffers: those sit
between 64 sentinel floats inside one allocation, so a vector store past the end shows without any access outside it."""
import ctypes

import numpy as np
import pytest
import torch

import loss_ref as lr

pytestmark = pytest.mark.gpu

GUARD = 64
SENT = float(np.float32(-12345.678))
THR = lr.SIL_THRES
UP = 2.5                                            # upstream gradient (other than 1)
W_IM, W_D = 0.7, 1.3                                # weights other than 1
F32 = np.float32
TINY = [(1, 1), (1, 3), (1, 4), (1, 5), (2, 2), (1, 255), (1, 256), (1, 257), (8, 129), (12, 20), (13, 19)]


def _api():
    import diff_gaussian_rasterization as dgr
    from diff_gaussian_rasterization import losses
    return dgr._lib, dgr._stream_ptr, losses


def guarded(dev, n, offset=0):
    """n floats between GUARD sentinel floats (+ `offset` floats: a base 4-byte but not 16-byte aligned), all set to SENT."""
    buf = torch.full((GUARD + offset + n + GUARD,), SENT, dtype=torch.float32, device=dev)
    view = buf[GUARD + offset:GUARD + offset + n]
    assert view.data_ptr() % 16 == 4 * (offset % 4) and view.is_contiguous()
    return buf, view


def intact(buf, view):
    """Every float of the allocation outside `view` still holds the sentinel."""
    lo = (view.data_ptr() - buf.data_ptr()) // 4
    return bool((buf[:lo] == SENT).all()) and bool((buf[lo + view.numel():] == SENT).all())


def place(dev, t, offset):
    """A contiguous device copy of `t` whose base sits `offset` floats past a 16-byte boundary."""
    buf = torch.empty(t.numel() + 8, dtype=torch.float32, device=dev)
    view = buf[offset:offset + t.numel()]
    view.copy_(t.reshape(-1))
    assert view.data_ptr() % 16 == 4 * offset and view.is_contiguous()
    return view


def upload(dev, f, off=()):
    src = {"im": f["im"], "ds": f["ds"], "gt_im": f["gt_im"], "gt_depth": f["gt_depth"], "extra_mask": f["extra_mask"],
           "color_weight": lr.color_weight(f)}
    return {k: place(dev, v, 1 if (k in off or off == "all") else 0) for k, v in src.items()}


def ptr(t):
    return None if t is None else t.data_ptr()


def c_masked_l1(dev, d, P, mode, out_offset=0):
    lib, stream, _ = _api()
    rows = int(lib.vtgs_masked_l1_partial_rows(P))
    pb, part = guarded(dev, rows * 3)
    ib, gi = guarded(dev, 3 * P, out_offset)
    db, gd = guarded(dev, 3 * P, out_offset)
    assert lib.vtgs_masked_l1(ptr(d["im"]), ptr(d["ds"]), ptr(d["gt_im"]), ptr(d["gt_depth"]), P, THR, mode, ptr(part), ptr(gi),
                              ptr(gd), stream(dev)) == 0
    torch.cuda.synchronize()
    assert intact(pb, part) and intact(ib, gi) and intact(db, gd)
    return part.reshape(rows, 3).double().sum(0).cpu(), gi.reshape(3, P).cpu(), gd.reshape(3, P).cpu()


def c_forward(dev, d, H, W, mode, w_im, w_d, em, cw, maps=True):
    lib, stream, _ = _api()
    scratch = torch.empty(int(lib.vtgs_loss_scratch_floats(H, W)), dtype=torch.float32, device=dev)
    ob, out = guarded(dev, 8)
    gm = torch.empty(9 * H * W, dtype=torch.float32, device=dev) if (mode == 1 and maps) else None
    assert lib.vtgs_slam_loss_forward(mode, ptr(d["im"]), ptr(d["ds"]), ptr(d["gt_im"]), ptr(d["gt_depth"]), H, W, THR, w_im, w_d,
                                      ptr(scratch), ptr(gm), ptr(out), ptr(d["extra_mask"]) if em else None,
                                      ptr(d["color_weight"]) if cw else None, stream(dev)) == 0
    torch.cuda.synchronize()
    assert intact(ob, out)
    return out, gm


def c_backward(dev, d, H, W, mode, w_im, w_d, gm, out, em, cw, out_offset=0):
    lib, stream, _ = _api()
    P = H * W
    ib, gi = guarded(dev, 3 * P, out_offset)
    db, gd = guarded(dev, 3 * P, out_offset)
    up = torch.tensor([UP], dtype=torch.float32, device=dev)
    assert lib.vtgs_slam_loss_backward(mode, ptr(d["im"]), ptr(d["ds"]), ptr(d["gt_im"]), ptr(d["gt_depth"]), H, W, THR, w_im, w_d,
                                       ptr(gm), ptr(out), ptr(up), ptr(gi), ptr(gd), ptr(d["extra_mask"]) if em else None,
                                       ptr(d["color_weight"]) if cw else None, stream(dev)) == 0
    torch.cuda.synchronize()
    assert intact(ib, gi) and intact(db, gd)
    return gi.reshape(3, H, W).cpu(), gd.reshape(3, H, W).cpu()


def coef(*factors):
    """The product of float32 factors, rounded to float32 after every multiplication (as the kernel forms up * w)."""
    c = F32(factors[0])
    for x in factors[1:]:
        c = F32(c * F32(x))
    return c


def check_l1_grads(mode, gi, gd, t, w_im, w_d, count, rows=None, g_im_ref=None, halo=0):
    """The gradient images: tracking / mode 2 images equal float32(sign * up * w) exactly; the mapping depth plane is
    float32(sign) times ONE coefficient within float32 rounding of up * w_depth / count, planes 1 and 2 exactly 0; the
    mapping colour image (L1 + SSIM) within 1e-3 of the largest reference gradient.  `rows`: only those rows were written
    (g_im: widened by `halo`); every other row still holds the sentinel, bit for bit."""
    H = gi.shape[-2]
    r0, r1 = (0, H) if rows is None else rows
    h0, h1 = max(r0 - halo, 0), min(r1 + halo, H)
    sent = torch.full((), SENT, dtype=torch.float32)
    for img, a, b in ((gd, r0, r1), (gi, h0, h1)):
        assert torch.equal(img[:, :a], sent.expand_as(img[:, :a])) and torch.equal(img[:, b:], sent.expand_as(img[:, b:]))
    sign_d = t["g_depth"][r0:r1]
    assert torch.equal(gd[1:, r0:r1], torch.zeros_like(gd[1:, r0:r1]))
    if mode != 1:
        assert torch.equal(gd[0, r0:r1], (sign_d * float(coef(UP, w_d))).float())
        assert torch.equal(gi[:, r0:r1], (t["g_im"][:, r0:r1] * float(coef(UP, w_im))).float())
        return
    got = gd[0, r0:r1]
    mags = got[got != 0].abs().unique()
    if float(F32(w_d)) != 0.0 and sign_d.abs().sum() > 0:
        want = float(F32(UP)) * float(F32(w_d)) / count
        assert torch.equal(torch.sign(got).double(), sign_d)
        assert mags.numel() == 1 and abs(mags.item() - want) <= 2 * float(np.spacing(F32(want))), (mags, want)
    else:
        assert mags.numel() == 0                                         # w_depth = 0 (use_l1 = False): no depth gradient
    ref = g_im_ref[:, h0:h1] * UP
    assert (gi[:, h0:h1].double() - ref).abs().max().item() <= 1e-3 * g_im_ref.abs().max().item() * UP


def check_out8(out, ref, fields=range(7)):
    got = out.cpu().tolist()
    assert got[1] == ref[1] and got[7] == 0.0                        # the mask count is exact
    for k in fields:
        assert lr.rel(got[k], ref[k]) <= 2e-5, (k, got[k], ref[k])


# ---- vtgs_masked_l1, the standalone call with its gradient images --------------------------------------------------------
@pytest.mark.parametrize("shape", TINY, ids=lambda s: f"{s[0]}x{s[1]}")
def test_masked_l1_sums_and_gradient_images(gpu_device, shape):
    H, W = shape
    f = lr.frame(H, W)
    d = upload(gpu_device, f)
    for mode in (0, 1, 2):
        t = lr.pixel_terms(f["im"], f["ds"], f["gt_im"], f["gt_depth"], THR, mode)
        sums, gi, gd = c_masked_l1(gpu_device, d, H * W, mode)
        assert sums[2].item() == t["count"]
        assert lr.rel(sums[0], t["sum_im"]) <= 2e-5 and lr.rel(sums[1], t["sum_depth"]) <= 2e-5
        assert torch.equal(gi.double(), t["g_im"].reshape(3, -1))    # +-1 / 0: exact
        assert torch.equal(gd[0].double(), t["g_depth"].reshape(-1)) and not gd[1:].any()


# ---- the whole loss, forward (all of out8) and backward -----------------------------------------------------------------
# (mode, extra_mask, color_weight, w_depth)
CONFIGS = [(0, True, False, W_D), (2, True, False, W_D), (1, True, False, W_D), (1, False, True, W_D), (0, False, False, 0.0),
           (1, True, True, 0.0)]


@pytest.mark.parametrize("shape", TINY, ids=lambda s: f"{s[0]}x{s[1]}")
def test_whole_loss_forward_and_backward(gpu_device, shape):
    H, W = shape
    f = lr.frame(H, W)
    d = upload(gpu_device, f)
    for mode, em, cw, w_d in CONFIGS:
        ref, t, _, g_ref = lr.loss_reference(f, mode, W_IM, w_d, use_extra=em, use_weight=cw, want_grad=(mode == 1))
        out, gm = c_forward(gpu_device, d, H, W, mode, W_IM, w_d, em, cw)
        check_out8(out, ref)
        gi, gd = c_backward(gpu_device, d, H, W, mode, W_IM, w_d, gm, out, em, cw)
        check_l1_grads(mode, gi, gd, t, W_IM, w_d, t["count"], g_im_ref=g_ref)


# ---- 12x20 with bases one float past a 16-byte boundary: the one-by-one path under an aligned plane stride ----------------
def test_masked_l1_alignment_fallback_gives_the_same_bits(gpu_device):
    H, W = 12, 20
    f = lr.frame(H, W)
    aligned = upload(gpu_device, f)
    for mode in (0, 1, 2):
        t = lr.pixel_terms(f["im"], f["ds"], f["gt_im"], f["gt_depth"], THR, mode)
        s0, gi0, gd0 = c_masked_l1(gpu_device, aligned, H * W, mode)
        for off, out_off in (("all", 1), (("gt_depth",), 0), ((), 1)):     # every base; one input only; the outputs only
            s1, gi1, gd1 = c_masked_l1(gpu_device, upload(gpu_device, f, off), H * W, mode, out_off)
            assert torch.equal(gi0, gi1) and torch.equal(gd0, gd1) and s0[2] == s1[2] == t["count"]
            for k, key in ((0, "sum_im"), (1, "sum_depth")):
                assert lr.rel(s1[k], s0[k]) <= 2e-6 and lr.rel(s1[k], t[key]) <= 2e-5 and lr.rel(s0[k], t[key]) <= 2e-5


def test_whole_loss_alignment_fallback_gives_the_same_bits(gpu_device):
    H, W = 12, 20
    f = lr.frame(H, W)
    aligned = upload(gpu_device, f)
    for mode, em, cw, w_d in CONFIGS[:4]:
        ref, t, _, g_ref = lr.loss_reference(f, mode, W_IM, w_d, use_extra=em, use_weight=cw, want_grad=(mode == 1))
        out0, gm0 = c_forward(gpu_device, aligned, H, W, mode, W_IM, w_d, em, cw)
        gi0, gd0 = c_backward(gpu_device, aligned, H, W, mode, W_IM, w_d, gm0, out0, em, cw)
        offs = ["all", ("gt_depth",)] + ([("extra_mask",)] if em else []) + ([("color_weight",)] if cw else [])
        for off in offs:
            d = upload(gpu_device, f, off)
            out1, gm1 = c_forward(gpu_device, d, H, W, mode, W_IM, w_d, em, cw)
            check_out8(out1, ref)
            assert out1[1].item() == out0[1].item()
            for k in (0, 2, 3, 5, 6):
                assert lr.rel(out1[k].item(), out0[k].item()) <= 2e-6
            gi1, gd1 = c_backward(gpu_device, d, H, W, mode, W_IM, w_d, gm1, out1, em, cw, out_offset=1 if off == "all" else 0)
            check_l1_grads(mode, gi1, gd1, t, W_IM, w_d, t["count"], g_im_ref=g_ref)
            assert torch.equal(gd0, gd1)
            if mode != 1:
                assert torch.equal(gi0, gi1)
        check_out8(out0, ref)


# ---- grid stride: more pixels than 1024 workgroups cover in one sweep ----------------------------------------------------
def _summation_bound(f, mode, t, em=None):
    """max(2e-5, 4 x the distance of a float32 pairwise evaluation on the CPU from float64), per sum."""
    s32 = lr.sums_float32(f["im"], f["ds"], f["gt_im"], f["gt_depth"], THR, mode, em)
    d32 = (lr.rel(s32[0], t["sum_im"]), lr.rel(s32[1], t["sum_depth"]))
    return d32, tuple(max(2e-5, 4 * x) for x in d32)


@pytest.mark.parametrize("shape", [(513, 513), (1026, 1024)], ids=["513x513-scalar-wraps", "1026x1024-float4-wraps"])
def test_grid_stride_masked_l1_and_tracking(gpu_device, shape):
    _, _, losses = _api()
    H, W = shape
    f = lr.frame(H, W)
    dev = gpu_device
    gt_im, gt_depth = f["gt_im"].to(dev), f["gt_depth"].to(dev)
    for mode in (0, 1, 2):
        t = lr.pixel_terms(f["im"], f["ds"], f["gt_im"], f["gt_depth"], THR, mode)
        d32, bound = _summation_bound(f, mode, t)
        im, ds = f["im"].to(dev).requires_grad_(True), f["ds"].to(dev).requires_grad_(True)
        s_im, s_d, cnt = losses._MaskedL1.apply(im, ds, gt_im, gt_depth, THR, mode)
        (2.0 * s_im + 3.0 * s_d).backward()
        got = (lr.rel(s_im.item(), t["sum_im"]), lr.rel(s_d.item(), t["sum_depth"]))
        print(f"masked_l1 {H}x{W} mode {mode}: GPU distance from float64 {got[0]:.2e} / {got[1]:.2e} (colour / depth), "
              f"float32 pairwise CPU {d32[0]:.2e} / {d32[1]:.2e}")
        assert cnt.item() == t["count"]
        assert got[0] <= bound[0] and got[1] <= bound[1]
        assert torch.equal(im.grad.cpu().double(), 2.0 * t["g_im"])
        assert torch.equal(ds.grad[0].cpu().double(), 3.0 * t["g_depth"]) and not ds.grad[1:].any()
    ref, t, _, _ = lr.loss_reference(f, 0, W_IM, W_D)
    d32, bound = _summation_bound(f, 0, t, f["extra_mask"])
    im, ds = f["im"].to(dev).requires_grad_(True), f["ds"].to(dev).requires_grad_(True)
    loss, terms = losses.tracking_loss(im, ds, gt_im, gt_depth, THR, w_im=W_IM, w_depth=W_D, extra_mask=f["extra_mask"].to(dev),
                                       return_terms=True)
    (loss * UP).backward()
    got = terms.cpu().tolist()
    print(f"tracking_loss {H}x{W}: GPU distance from float64 {lr.rel(got[0], ref[0]):.2e}, float32 pairwise CPU "
          f"{d32[0]:.2e} / {d32[1]:.2e}")
    assert got[1] == ref[1] and loss.item() == got[0]
    for k, b in ((0, max(bound)), (2, bound[0]), (3, bound[1]), (5, bound[0]), (6, bound[1])):
        assert lr.rel(got[k], ref[k]) <= b, (k, got[k], ref[k])
    check_l1_grads(0, im.grad.cpu(), ds.grad.cpu(), t, W_IM, W_D, t["count"])


def test_grid_stride_mapping_loss(gpu_device):
    _, _, losses = _api()
    H, W = 513, 513
    f = lr.frame(H, W)
    dev = gpu_device
    ref, t, _, g_ref = lr.loss_reference(f, 1, W_IM, W_D, use_extra=True, use_weight=True, want_grad=True)
    im, ds = f["im"].to(dev).requires_grad_(True), f["ds"].to(dev).requires_grad_(True)
    loss, terms = losses.mapping_loss(im, ds, f["gt_im"].to(dev), f["gt_depth"].to(dev), w_im=W_IM, w_depth=W_D,
                                      extra_mask=f["extra_mask"].to(dev), additional_mask=f["additional_mask"].to(dev),
                                      return_terms=True)
    (loss * UP).backward()
    check_out8(terms, ref)
    check_l1_grads(1, im.grad.cpu(), ds.grad.cpu(), t, W_IM, W_D, t["count"], g_im_ref=g_ref)


# ---- bands ---------------------------------------------------------------------------------------------------------------
def c_band(dev, d, H, W, rows, mode, w_im, w_d, em, cw, total=None, first=True, backward=True):
    """One band through the three C entry points: (sums8, share out8, g_im, g_depth_sil); the gradient images are
    handed in full of sentinels.  total=None: a single band (its own sums are the sums over all bands)."""
    lib, stream, _ = _api()
    P, st = H * W, stream(dev)
    scratch = torch.empty(int(lib.vtgs_loss_scratch_floats(H, W)), dtype=torch.float32, device=dev)
    gm = torch.empty(9 * P, dtype=torch.float32, device=dev) if mode == 1 else None
    sb, sums = guarded(dev, 8)
    e, c = (ptr(d["extra_mask"]) if em else None), (ptr(d["color_weight"]) if cw else None)
    args = (mode, ptr(d["im"]), ptr(d["ds"]), ptr(d["gt_im"]), ptr(d["gt_depth"]), H, W, rows[0], rows[1])
    assert lib.vtgs_slam_loss_band_sums(*args, THR, ptr(scratch), ptr(gm), ptr(sums), e, c, st) == 0
    torch.cuda.synchronize()
    assert intact(sb, sums)
    if not backward and total is None:
        return sums, None, None, None
    ob, out = guarded(dev, 8)
    tot = sums if total is None else total
    assert lib.vtgs_slam_loss_band_share(mode, ptr(sums), ptr(tot), H, W, w_im, w_d, 1 if cw else 0, 1 if first else 0, ptr(out), st) == 0
    if not backward:
        torch.cuda.synchronize()
        return sums, out, None, None
    ib, gi = guarded(dev, 3 * P)
    db, gd = guarded(dev, 3 * P)
    up = torch.tensor([UP], dtype=torch.float32, device=dev)
    assert lib.vtgs_slam_loss_band_backward(*args, THR, w_im, w_d, ptr(gm), ptr(out), ptr(up), ptr(gi), ptr(gd), e, c, st) == 0
    torch.cuda.synchronize()
    assert intact(ob, out) and intact(ib, gi) and intact(db, gd)
    return sums, out, gi.reshape(3, H, W).cpu(), gd.reshape(3, H, W).cpu()


BANDS_8X6 = [(1, 2), (2, 5), (0, 8), (7, 8), (0, 1), (2, 3), (4, 7)]      # p0 = 6: no float4; 16 by fours + 2; whole; last row; tails
PARTITION_8X6 = [(0, 1), (1, 2), (2, 5), (5, 7), (7, 8)]


@pytest.mark.parametrize("mode", [0, 2])
def test_tracking_bands_on_8x6(gpu_device, mode):
    _, _, losses = _api()
    H, W = 8, 6
    f = lr.frame(H, W)
    dev = gpu_device
    d = upload(dev, f)
    full_ref, full_t, _, _ = lr.loss_reference(f, mode, W_IM, W_D)
    out_full, _ = c_forward(dev, d, H, W, mode, W_IM, W_D, True, False)
    gi_full, gd_full = c_backward(dev, d, H, W, mode, W_IM, W_D, None, out_full, True, False)
    for rows in BANDS_8X6:
        ref, t, _, _ = lr.loss_reference(f, mode, W_IM, W_D, rows=rows)
        sums, out, gi, gd = c_band(dev, d, H, W, rows, mode, W_IM, W_D, True, False)
        s = sums.cpu().tolist()
        assert s[2] == t["count"] and lr.rel(s[0], t["sum_im"]) <= 2e-5 and lr.rel(s[1], t["sum_depth"]) <= 2e-5 and s[3:] == [0.0] * 5
        check_out8(out, ref)
        check_l1_grads(mode, gi, gd, t, W_IM, W_D, t["count"], rows=rows)
        if rows == (0, H):                                               # the band that is the frame: the full-frame call's bits
            assert s[:3] == [out_full[2].item(), out_full[3].item(), out_full[1].item()]
            assert torch.equal(gi, gi_full) and torch.equal(gd, gd_full) and lr.rel(out[0].item(), out_full[0].item()) <= 2e-6
    # the Python caller over a partition: the shares add up to the full-frame float64 loss, the gradients to its gradients
    im, ds = d["im"].reshape(3, H, W).clone().requires_grad_(True), d["ds"].reshape(3, H, W).clone().requires_grad_(True)
    gt_im, gt_depth, em = d["gt_im"].reshape(3, H, W), d["gt_depth"].reshape(1, H, W), d["extra_mask"].reshape(H, W)
    share_sum, count = 0.0, 0.0
    for rows in PARTITION_8X6:
        share, rec, tot = losses.band_loss(im, ds, gt_im, gt_depth, rows, mode="tracking", sil_thres=THR, w_im=W_IM, w_depth=W_D,
                                           extra_mask=em, colour_over_all_pixels=(mode == 2), return_terms=True)
        (share * UP).backward()
        share_sum += share.item()
        count += tot[2].item()
    assert count == full_t["count"] and lr.rel(share_sum, full_ref[0]) <= 2e-5
    assert torch.equal(im.grad.cpu(), gi_full) and torch.equal(ds.grad.cpu(), gd_full)


BANDS_40X36 = [(0, 16), (16, 32), (16, 40), (32, 40), (3, 14)]
PARTITION_40X36 = [(0, 16), (16, 32), (32, 40)]


@pytest.mark.parametrize("weights", [False, True], ids=["plain", "extra+weights"])
def test_mapping_bands_on_40x36(gpu_device, weights):
    H, W = 40, 36
    f = lr.frame(H, W)
    dev = gpu_device
    d = upload(dev, f)
    em = cw = weights
    full_ref, full_t, _, _ = lr.loss_reference(f, 1, W_IM, W_D, use_extra=em, use_weight=cw)
    total = sum(c_band(dev, d, H, W, rows, 1, W_IM, W_D, em, cw, backward=False)[0] for rows in PARTITION_40X36)
    assert total[2].item() == full_t["count"]
    share_sum = 0.0
    for rows in BANDS_40X36:
        first = rows[0] == 0
        ref, t, ssim_sum, g_ref = lr.loss_reference(f, 1, W_IM, W_D, use_extra=em, use_weight=cw, rows=rows,
                                                    count_all=full_t["count"], first_band=first, want_grad=True)
        sums, out, gi, gd = c_band(dev, d, H, W, rows, 1, W_IM, W_D, em, cw, total=total, first=first)
        s = sums.cpu().tolist()
        assert s[2] == t["count"] and s[4:] == [0.0] * 4
        for got, want in ((s[0], t["sum_im"]), (s[1], t["sum_depth"]), (s[3], ssim_sum)):
            assert lr.rel(got, want) <= 2e-5, (rows, got, want)
        o = out.cpu().tolist()
        assert o[1] == full_t["count"] and o[7] == 0.0 and lr.rel(o[4], full_ref[4]) <= 2e-5   # count and SSIM of the frame
        for k in (0, 2, 3, 5, 6):
            assert lr.rel(o[k], ref[k]) <= 2e-5, (rows, k, o[k], ref[k])
        check_l1_grads(1, gi, gd, t, W_IM, W_D, full_t["count"], rows=rows, g_im_ref=g_ref, halo=5)
        if rows in PARTITION_40X36:
            share_sum += o[0]
    assert lr.rel(share_sum, full_ref[0]) <= 2e-5


# ---- silhouette sweep ------------------------------------------------------------------------------------------------------
LEVELS = [0.95, 0.90, 0.99, 0.93, 1.0, 0.97, 0.89, 0.96]                  # eight candidates: all 16 columns of the kernel's LDS row


def _sweep_inputs(P):
    g = torch.Generator().manual_seed(P)
    im = torch.rand(3, P, generator=g)
    gt = (im + 0.2 * torch.randn(3, P, generator=g)).clamp(0, 1)
    sil = (0.90 + 0.01 * torch.randint(0, 11, (P,), generator=g).float())  # 0.90, 0.91 .. 1.00 as float32 sums
    gd = (torch.rand(P, generator=g) > 0.2).float() * 1.5
    return im, sil, gt, gd


@pytest.mark.parametrize("P", [1, 255, 257, 263169])
def test_silhouette_sweep_counts_and_sums(gpu_device, P):
    lib, stream, _ = _api()
    dev = gpu_device
    im, sil, gt, gd = _sweep_inputs(P)
    levels = [float(sil[0])] + [float(F32(0.90) + F32(0.01) * F32(k)) for k in (0, 9, 3, 10, 7)] + [0.89, float(sil[-1])]
    assert sum(bool((sil == c).any()) for c in levels) >= (7 if P >= 255 else 1)       # thresholds ON silhouette values
    a, s, b, z = (t.to(dev).contiguous() for t in (im, sil, gt, gd))
    spans = [(0, P)] + ([(7, P - 3)] if P > 16 else [])                   # the full call, and a band with pixel_begin = 7
    for K in (1, 5, 8):
        th = (ctypes.c_float * K)(*levels[:K])
        for p0, p1 in spans:
            rows = int(lib.vtgs_masked_l1_partial_rows(p1 - p0))
            pb, part = guarded(dev, rows * 2 * K)                         # what follows the last row is sentinel
            if (p0, p1) == (0, P):
                st = lib.vtgs_silhouette_sweep(ptr(a), ptr(s), ptr(b), ptr(z), P, th, K, ptr(part), stream(dev))
            else:
                st = lib.vtgs_silhouette_sweep_band(ptr(a), ptr(s), ptr(b), ptr(z), P, p0, p1, th, K, ptr(part), stream(dev))
            assert st == 0
            torch.cuda.synchronize()
            assert intact(pb, part)
            got = part.reshape(rows, K, 2).double().sum(0).cpu()
            ref = lr.sweep_reference(im, sil, gt, gd, levels[:K], p0, p1)
            assert torch.equal(got[:, 1], ref[:, 1]), (K, p0, p1)
            assert ((got[:, 0] - ref[:, 0]).abs() <= 1e-5 * ref[:, 0]).all(), (K, p0, p1)


def test_silhouette_sweep_rows_through_the_python_caller(gpu_device):
    _, _, losses = _api()
    H, W = 8, 6
    im, sil, gt, gd = _sweep_inputs(H * W)
    dev = gpu_device
    args = (im.reshape(3, H, W).to(dev), sil.reshape(H, W).to(dev), gt.reshape(3, H, W).to(dev), gd.reshape(1, H, W).to(dev))
    for rows in ((1, 2), (2, 5), (0, 8), (7, 8)):
        got = losses.silhouette_sweep(*args, LEVELS, rows=rows).cpu()
        ref = lr.sweep_reference(im, sil, gt, gd, LEVELS, rows[0] * W, rows[1] * W)
        assert torch.equal(got[:, 1], ref[:, 1]) and ((got[:, 0] - ref[:, 0]).abs() <= 1e-5 * ref[:, 0]).all()


# ---- seen / running maximum of the radius ------------------------------------------------------------------------------------
def _bookkeeping_inputs(n):
    g = torch.Generator().manual_seed(n)
    radii = torch.randint(1, 40, (n,), generator=g, dtype=torch.int32)
    radii[1::3] = 0                                                      # culled: not seen, the maximum stays
    mx = radii.float() + torch.where(torch.arange(n) % 2 == 0, -0.5, 0.5)   # below the new radius on even, above on odd indices
    return radii, mx.clamp(min=0.0)


def _bookkeeping_buffers(dev, radii, mx):
    n = radii.numel()
    mb, m = guarded(dev, n)
    m.copy_(mx)
    sb = torch.full((64 + n + 16,), 0x5A, dtype=torch.uint8, device=dev)   # 16 guard bytes after seen[n - 1]
    return radii.to(dev), mb, m, sb, sb[64:64 + n]


@pytest.mark.parametrize("n", [1, 2, 3, 4, 5, 1023, 1024, 1025, 1027, 2049])
def test_seen_and_max_radius(gpu_device, n):
    lib, stream, _ = _api()
    dev = gpu_device
    radii, mx = _bookkeeping_inputs(n)
    seen_ref, mx_ref = lr.bookkeeping_reference(radii.numpy(), mx.numpy())
    assert seen_ref[0] == 1 and mx_ref[0] > mx[0] and (n < 4 or (seen_ref[1] == 0 and mx_ref[3] == mx[3] and seen_ref[3] == 1))
    r, mb, m, sb, seen = _bookkeeping_buffers(dev, radii, mx)
    assert lib.vtgs_seen_and_max_radius(n, ptr(r), ptr(m), ptr(seen), stream(dev)) == 0
    torch.cuda.synchronize()
    assert np.array_equal(seen.cpu().numpy(), seen_ref) and np.array_equal(m.cpu().numpy(), mx_ref)
    assert intact(mb, m) and bool((sb[:64] == 0x5A).all()) and bool((sb[64 + n:] == 0x5A).all())


def test_bookkeeping_folded_into_the_loss_gives_the_same_bits(gpu_device):
    lib, stream, losses = _api()
    dev = gpu_device
    H, W, n = 8, 6, 2049                                                 # workgroups 1..3 of the finalize launch do the bookkeeping
    f = lr.frame(H, W)
    radii, mx = _bookkeeping_inputs(n)
    r, mb, m, sb, seen = _bookkeeping_buffers(dev, radii, mx)
    assert lib.vtgs_seen_and_max_radius(n, ptr(r), ptr(m), ptr(seen), stream(dev)) == 0
    r2, mb2, m2, sb2, seen2 = _bookkeeping_buffers(dev, radii, mx)
    args = [f[k].to(dev) for k in ("im", "ds", "gt_im", "gt_depth")]
    plain = losses.tracking_loss(*args, THR, w_im=W_IM, w_depth=W_D)
    folded = losses.tracking_loss(*args, THR, w_im=W_IM, w_depth=W_D, bookkeeping=(r2, m2, seen2.view(torch.bool)))
    torch.cuda.synchronize()
    assert folded.item() == plain.item() and lr.rel(plain.item(), lr.loss_reference(f, 0, W_IM, W_D, use_extra=False)[0][0]) <= 2e-5
    assert torch.equal(seen, seen2) and torch.equal(m, m2) and torch.equal(mb, mb2) and torch.equal(sb, sb2)
    seen_ref, mx_ref = lr.bookkeeping_reference(radii.numpy(), mx.numpy())
    assert np.array_equal(seen2.cpu().numpy(), seen_ref) and np.array_equal(m2.cpu().numpy(), mx_ref)


def test_bookkeeping_refuses_misaligned_pointers_on_the_host(gpu_device):
    """The kernel moves int4 / float4 / one uint32_t per four Gaussians and has no scalar fallback (include/vtgs.h): a base
    that does not allow it is refused before any device work -- status returned, nothing written."""
    lib, stream, _ = _api()
    dev = gpu_device
    n, H, W = 9, 2, 2
    radii = torch.full((n + 8,), 7, dtype=torch.int32, device=dev)
    d = upload(dev, lr.frame(H, W))
    scratch = torch.empty(int(lib.vtgs_loss_scratch_floats(H, W)), dtype=torch.float32, device=dev)
    for r_off, m_off, s_off in ((1, 0, 0), (0, 1, 0), (0, 0, 1), (0, 0, 2), (2, 2, 0)):
        mb, m = guarded(dev, n, m_off)
        sb = torch.full((64 + n + 16,), 0x5A, dtype=torch.uint8, device=dev)
        seen = sb[64 + s_off:64 + s_off + n]
        r = radii[r_off:r_off + n]
        assert (r.data_ptr() % 16, m.data_ptr() % 16, seen.data_ptr() % 4) == (4 * r_off, 4 * m_off, s_off)
        ob, out = guarded(dev, 8)
        assert lib.vtgs_seen_and_max_radius(n, ptr(r), ptr(m), ptr(seen), stream(dev)) == 1      # VTGS_ERR_INVALID_ARGUMENT
        assert lib.vtgs_slam_loss_forward_seen(0, ptr(d["im"]), ptr(d["ds"]), ptr(d["gt_im"]), ptr(d["gt_depth"]), H, W, THR, W_IM,
                                               W_D, ptr(scratch), None, ptr(out), None, None, n, ptr(r), ptr(m), ptr(seen),
                                               stream(dev)) == 1
        torch.cuda.synchronize()
        assert bool((mb == SENT).all()) and bool((sb == 0x5A).all()) and bool((ob == SENT).all())
