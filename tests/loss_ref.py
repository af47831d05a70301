"""Float64 CPU statements of what csrc/vtgs_loss.hip and csrc/vtgs_adam.hip (Adam) compute, written from the text of include/vtgs.h -- TEST
INFRASTRUCTURE, not part of the product -- and the hand-placed frames the path tests run them on.

One function per operation (pixel terms, whole loss, SSIM map, silhouette sweep, one Adam step, the seen / max-radius
bookkeeping).  Inputs are float32 CPU tensors exactly as the kernels receive them; everything is evaluated in float64, so a
difference `gt - x` of two float32 values and a sign are exact.  `frame()` builds images in which every pixel class that the
mask distinguishes sits on every lane of a float4 group and in the one-by-one tails; `placement()` reports where, and
tests/test_loss_ref_placement.py asserts it on the CPU so that the GPU tests cannot be vacuous."""
import functools

import numpy as np
import torch
import torch.nn.functional as F

import slam_callers as sc

# pixel classes of frame(): what the mask of get_loss can make of one pixel
IN, GT_ZERO, NAN_DEPTH, NAN_UNC, SIL_AT_THRES, EXTRA_OUT, EXACT_ZERO = range(7)
N_CLASSES = 7
SIL_THRES = float(np.float32(0.95))                 # the threshold as the kernels see it (a float32 value)


def pixel_class(P):
    """Class of pixel i = 4 j + k: (3 j + k) mod 7.  For a fixed lane k seven consecutive groups j run through all seven
    classes, and the pixels 4 j + {0, 1} that end a band of 8x6 rows (j = 1, 4, 7, 10) carry all seven between them."""
    i = torch.arange(P)
    return (3 * (i // 4) + (i % 4)) % N_CLASSES


@functools.lru_cache(maxsize=None)
def frame(H, W, seed=0):
    """float32 CPU images of one frame with the classes of pixel_class() placed by hand, random colour and depth elsewhere.
    Keys: im, gt_im [3,H,W]; ds [3,H,W] = (depth, silhouette, depth^2 + uncertainty); gt_depth [1,H,W]; extra_mask [H,W]
    (0 / 1); additional_mask [1,H,W] (0 / 1: colour weights 0.8 / 10.8); cls [H,W].  Treat the tensors as read-only."""
    g = torch.Generator().manual_seed(1000 * H + W + seed)
    P = H * W
    cls = pixel_class(P)
    im = torch.rand(3, P, generator=g)
    gt_im = (im + 0.1 * torch.randn(3, P, generator=g)).clamp(0, 1)      # a render close to its ground truth: SSIM well above 0
    z = 1.0 + 2.0 * torch.rand(P, generator=g)
    gt_depth = (z + 0.3 * torch.randn(P, generator=g)).clamp(min=0.05)
    sil = SIL_THRES + 0.001 + 0.049 * torch.rand(P, generator=g)         # strictly above the threshold
    dsq = z * z + 0.01 * torch.rand(P, generator=g)
    extra = torch.ones(P)
    nan = float("nan")
    gt_depth[cls == GT_ZERO] = 0.0
    z[cls == NAN_DEPTH] = nan
    dsq[cls == NAN_UNC] = nan
    sil[cls == SIL_AT_THRES] = SIL_THRES
    extra[cls == EXTRA_OUT] = 0.0
    ez = torch.nonzero(cls == EXACT_ZERO).flatten()
    gt_depth[ez] = z[ez]                                                  # gt - x exactly 0 in depth ...
    ch = (ez // 4) % 3
    gt_im[ch, ez] = im[ch, ez]                                            # ... and in one colour channel
    add = (torch.rand(P, generator=g) > 0.6).float()
    f = {"im": im.reshape(3, H, W), "gt_im": gt_im.reshape(3, H, W), "ds": torch.stack([z, sil, dsq]).reshape(3, H, W),
         "gt_depth": gt_depth.reshape(1, H, W), "extra_mask": extra.reshape(H, W), "additional_mask": add.reshape(1, H, W),
         "cls": cls.reshape(H, W), "H": H, "W": W}
    return f


def color_weight(f):
    """10 * additional_mask + 0.8 in float32, as mapping_loss forms it: the two values float32(0.8) and float32(10.8)."""
    return (10.0 * f["additional_mask"].to(torch.float32) + 0.8).expand(3, f["H"], f["W"]).contiguous()


def placement(cls, p0, p1, vec):
    """Which classes the kernels meet where, for pixels [p0, p1) of the flattened class map: lanes[k] = classes on lane k of
    the float4 groups, tail = classes in the one-by-one loop (everything when `vec` is false)."""
    c = cls.flatten().tolist()
    pv = p0 + ((p1 - p0) & ~3) if vec else p0
    lanes = [set(c[i] for i in range(p0 + k, pv, 4)) for k in range(4)]
    return lanes, set(c[pv:p1])


def mask_of(ds, gt_depth, sil_thres, mode, extra_mask=None):
    """[H,W] bool: gt_depth > 0, depth and ds[2] - ds[0]^2 not NaN, silhouette > threshold (strict; not in mode 1),
    extra_mask != 0."""
    d = ds.double()
    m = (gt_depth[0] > 0) & ~torch.isnan(d[0]) & ~torch.isnan(d[2] - d[0] * d[0])
    if mode != 1:
        m = m & (ds[1] > float(np.float32(sil_thres)))
    if extra_mask is not None:
        m = m & (extra_mask.reshape(m.shape) != 0)
    return m


def pixel_terms(im, ds, gt_im, gt_depth, sil_thres, mode, extra_mask=None, color_weight=None, rows=None):
    """The three sums, the mask count and the two unscaled gradient images of vtgs_masked_l1 over pixel rows `rows`
    (None = all).  mode 0: colour and depth over the mask; 1: depth over the mask (no silhouette test), colour over all
    pixels; 2: as 0 with the colour over all pixels.  g_im [3,H,W] = d sum_im / d im = sign(im - gt_im) * weight on the
    colour mask, g_depth [H,W] = d sum_depth / d depth = sign(depth - gt_depth) on the mask; rows outside `rows` are 0."""
    H, W = im.shape[-2:]
    r0, r1 = (0, H) if rows is None else rows
    band = torch.zeros(H, W, dtype=torch.bool)
    band[r0:r1] = True
    m = mask_of(ds, gt_depth, sil_thres, mode, extra_mask) & band
    mc = (m if mode == 0 else band)[None].expand(3, H, W)
    cw = torch.ones(3, H, W, dtype=torch.float64) if color_weight is None else color_weight.double().expand(3, H, W)
    e = gt_im.double() - im.double()
    d = torch.nan_to_num(gt_depth[0].double() - ds[0].double())           # (NaN depth is outside the mask)
    zero = torch.zeros((), dtype=torch.float64)
    return {"mask": m, "count": int(m.sum()),
            "sum_im": torch.where(mc, e.abs() * cw, zero).sum().item(),
            "sum_depth": torch.where(m, d.abs(), zero).sum().item(),
            "g_im": torch.where(mc, -torch.sign(e) * cw, zero),
            "g_depth": torch.where(m, -torch.sign(d), zero)}


def ssim_map(img1, img2):
    """The SSIM map whose mean is slam_callers.calc_ssim (11x11 Gaussian window, sigma 1.5, zero padding), [C,H,W]."""
    ch = img1.size(-3)
    a, b = img1.reshape(1, ch, *img1.shape[-2:]), img2.reshape(1, ch, *img2.shape[-2:])
    w = sc._gauss_window(11, 1.5, ch, a)
    blur = lambda t: F.conv2d(t, w, padding=5, groups=ch)
    mu1, mu2 = blur(a), blur(b)
    s11, s22, s12 = blur(a * a) - mu1 * mu1, blur(b * b) - mu2 * mu2, blur(a * b) - mu1 * mu2
    c1, c2 = 0.01 ** 2, 0.03 ** 2
    return (((2 * mu1 * mu2 + c1) * (2 * s12 + c2)) / ((mu1 * mu1 + mu2 * mu2 + c1) * (s11 + s22 + c2)))[0]


def whole_loss(mode, sum_im, sum_depth, count, numel_im, w_im, w_depth, ssim=0.0, has_color_weight=False):
    """out8[0..6] of vtgs_slam_loss_forward from the sums: {loss, mask count, sum_im, sum_depth, mean SSIM, weighted colour
    term, weighted depth term}.  Tracking (modes 0, 2): weighted SUMS.  Mapping: w_im (c L1-mean + 0.2 (1 - SSIM)) with c =
    0.8, or 1.0 in the colour-weight form, + w_depth * masked MEAN."""
    w_im, w_depth = float(np.float32(w_im)), float(np.float32(w_depth))   # the weights cross the C ABI as float32
    if mode != 1:
        t_im, t_d = w_im * sum_im, w_depth * sum_depth
    else:
        t_im = w_im * ((1.0 if has_color_weight else 0.8) * sum_im / numel_im + 0.2 * (1.0 - ssim))
        t_d = w_depth * sum_depth / count
    return [t_im + t_d, float(count), sum_im, sum_depth, ssim if mode == 1 else 0.0, t_im, t_d]


def loss_reference(f, mode, w_im, w_depth, use_extra=True, use_weight=False, rows=None, count_all=None, first_band=True,
                   want_grad=False):
    """The loss (rows=None) or one band's share of it, in float64 with autograd through slam_callers' SSIM: (out8[0..6]
    as whole_loss, pixel_terms, band SSIM sum, d value / d im or None).  A band's depth term divides by `count_all` (the
    mask count of the whole frame) and only the first band carries the constant of 0.2 (1 - SSIM)."""
    H, W = f["H"], f["W"]
    em = f["extra_mask"] if use_extra else None
    cw = color_weight(f) if (use_weight and mode == 1) else None
    t = pixel_terms(f["im"], f["ds"], f["gt_im"], f["gt_depth"], SIL_THRES, mode, em, cw, rows)
    numel = 3.0 * H * W
    if mode != 1:
        return whole_loss(mode, t["sum_im"], t["sum_depth"], t["count"], numel, w_im, w_depth), t, 0.0, None
    r0, r1 = (0, H) if rows is None else rows
    im = f["im"].double().requires_grad_(want_grad)
    smap = ssim_map(im, f["gt_im"].double())
    ssim_sum = smap[:, r0:r1].sum()
    cnt = t["count"] if count_all is None else count_all
    l1c = 1.0 if cw is not None else 0.8
    wi, wd = float(np.float32(w_im)), float(np.float32(w_depth))
    cwd = torch.ones(3, H, W, dtype=torch.float64) if cw is None else cw.double()
    s_im = ((f["gt_im"].double() - im).abs() * cwd)[:, r0:r1].sum()
    t_im = wi * (l1c * s_im / numel + 0.2 * ((1.0 if first_band else 0.0) - ssim_sum / numel))
    t_d = wd * t["sum_depth"] / cnt
    g = None
    if want_grad:
        t_im.backward()
        g = im.grad.detach()
    out = [t_im.item() + t_d, float(cnt), s_im.item(), t["sum_depth"], ssim_sum.item() / numel, t_im.item(), t_d]
    return out, t, ssim_sum.item(), g


def sums_float32(im, ds, gt_im, gt_depth, sil_thres, mode, extra_mask=None):
    """(sum_im, sum_depth) of pixel_terms evaluated in plain float32 with numpy's pairwise summation: how far float32
    arithmetic alone sits from the float64 statement at a given frame size."""
    m = mask_of(ds, gt_depth, sil_thres, mode, extra_mask).numpy()
    e = np.abs(gt_im.numpy() - im.numpy())
    d = np.abs(np.nan_to_num(gt_depth[0].numpy() - ds[0].numpy()))
    assert e.dtype == np.float32 and d.dtype == np.float32
    s_im = (e * m[None] if mode == 0 else e).sum(dtype=np.float32)
    return float(s_im), float((d * m).sum(dtype=np.float32))


def sweep_reference(im, sil, gt_im, gt_depth, thresholds, p0=0, p1=None):
    """[K,2] float64: per candidate c (a float32 value, as the launch carries it) the sum over the three channels of
    (gt_im - im)^2 and the pixel count over silhouette > c & gt_depth > 0, pixels [p0, p1)."""
    P = sil.numel()
    p1 = P if p1 is None else p1
    sq = ((gt_im.double() - im.double()) ** 2).reshape(3, P).sum(0)[p0:p1]
    s, valid = sil.reshape(P)[p0:p1], gt_depth.reshape(P)[p0:p1] > 0
    out = []
    for c in thresholds:
        m = valid & (s > float(np.float32(c)))
        out.append([sq[m].sum().item(), float(m.sum())])
    return torch.tensor(out, dtype=torch.float64)


def adam_reference(p, g, m, v, lr, eps, beta1, beta2, step):
    """One Adam step in float64 as include/vtgs.h states it (lerp form of m): returns (p, m, v).  lr, eps and the betas are
    the float32 values the C ABI carries."""
    lr, eps, b1, b2 = (float(np.float32(x)) for x in (lr, eps, beta1, beta2))
    p, g, m, v = (np.asarray(x, dtype=np.float64) for x in (p, g, m, v))
    m = m + (1.0 - b1) * (g - m)
    v = b2 * v + (1.0 - b2) * g * g
    denom = np.sqrt(v) / np.sqrt(1.0 - b2 ** step) + eps
    return p - lr / (1.0 - b1 ** step) * m / denom, m, v


def adam_float32(p, g, m, v, lr, eps, beta1, beta2, step):
    """The same formula evaluated operation by operation in float32 on the CPU (numpy; no fused multiply-adds): what plain
    float32 arithmetic makes of it, to size a bound where float64 agreement to a few ulps cannot be expected."""
    f = np.float32
    lr, eps, b1, b2 = f(lr), f(eps), f(beta1), f(beta2)
    p, g, m, v = (np.asarray(x, dtype=f) for x in (p, g, m, v))
    m = m + (f(1) - b1) * (g - m)
    v = b2 * v + ((f(1) - b2) * g) * g
    scale = f(1.0 / (1.0 - float(b1) ** step))
    bias2 = f(np.sqrt(1.0 - float(b2) ** step))
    denom = np.sqrt(v) / bias2 + eps
    return p - (lr * scale) * (m / denom), m, v


def bookkeeping_reference(radii, max_radius):
    """seen = r > 0 (uint8 0 / 1) and max(max_radius, float(r)) of get_loss's bookkeeping."""
    r = np.asarray(radii, dtype=np.int32)
    return (r > 0).astype(np.uint8), np.maximum(np.asarray(max_radius, dtype=np.float32), r.astype(np.float32))


def rel(got, ref):
    """|got - ref| relative to |ref| (0 / 0 = 0; anything else over 0 = inf)."""
    d = abs(float(got) - float(ref))
    return 0.0 if d == 0 else (d / abs(float(ref)) if ref != 0 else float("inf"))
