"""Shared by the tracking-mask tests: the cases (the reference fixture tests/golden/get_loss.npz and synthetic frames with
hand-placed edge situations), the float64 restatement of the visibility decision of get_vis_mask (src/vtgaussian_slam.py:
376-404, 536-584) with the signed margin of its comparison, the float32 restatement (`losses.visibility_mask` on the CPU)
and the decision band tau measured from the two.  Nothing here runs the kernel under test."""
import math
import os

import numpy as np
import torch

from keyframe_util import BAND_SHARE, EPS32, _bilinear64

HERE = os.path.dirname(os.path.abspath(__file__))
THRES = 0.05
_cache = {}


def fixture():
    if "fx" not in _cache:
        z = np.load(os.path.join(HERE, "golden", "get_loss.npz"))
        _cache["fx"] = {k: torch.from_numpy(z[k]) for k in z.files if z[k].ndim}
    return _cache["fx"]


def _pose(rx, ry, rz, t):
    """A rigid world-to-camera matrix (rotations about x, y, z in radians, then the translation), formed in float64 and
    rounded to float32."""
    cx, sx, cy, sy, cz, sz = math.cos(rx), math.sin(rx), math.cos(ry), math.sin(ry), math.cos(rz), math.sin(rz)
    Rx = torch.tensor([[1, 0, 0], [0, cx, -sx], [0, sx, cx]], dtype=torch.float64)
    Ry = torch.tensor([[cy, 0, sy], [0, 1, 0], [-sy, 0, cy]], dtype=torch.float64)
    Rz = torch.tensor([[cz, -sz, 0], [sz, cz, 0], [0, 0, 1]], dtype=torch.float64)
    m = torch.eye(4, dtype=torch.float64)
    m[:3, :3] = Rz @ Ry @ Rx
    m[:3, 3] = torch.tensor(t, dtype=torch.float64)
    return m.float()


def _project64(gt, k, curr_w2c, w2c):
    """float64: (u, v, z') [H,W] of every pixel of gt [1,H,W] in the overlapping frame `w2c`, the reference's operations."""
    H, W = gt.shape[-2:]
    k, z = k.double(), gt[0].double()
    ys, xs = torch.meshgrid(torch.arange(H, dtype=torch.float64), torch.arange(W, dtype=torch.float64), indexing="ij")
    pc = torch.stack(((xs - k[0, 2]) / k[0, 0] * z, (ys - k[1, 2]) / k[1, 1] * z, z, torch.ones_like(z)), dim=-1).reshape(-1, 4)
    pts = (torch.inverse(curr_w2c.double()) @ pc.T).T
    q = (k @ (w2c.double() @ pts.T)[:3]).T
    zp = q[:, 2] + 1e-5
    return (q[:, 0] / zp).reshape(H, W), (q[:, 1] / zp).reshape(H, W), zp.reshape(H, W)


def vis_f64(gt, k, curr_w2c, w2c, depth, thres=THRES):
    """float64 restatement for ONE overlapping frame: dict(vis [H,W] bool, margin [H,W] = (thres * min(d, z') - |d - z'|) /
    max(|z'|, 1e-12) -- as keyframe_util.masks_f64 forms it --, u, v, zp, d).  A pixel with gt < 0 or NaN: vis False,
    margin -1 (no comparison decides it)."""
    u, v, zp = _project64(gt, k, curr_w2c, w2c)
    finite = torch.isfinite(u) & torch.isfinite(v)
    d = _bilinear64(depth.double().reshape(depth.shape[-2:]), torch.where(finite, u, torch.full_like(u, -9.0)).reshape(-1),
                    torch.where(finite, v, torch.full_like(v, -9.0)).reshape(-1)).reshape(u.shape)
    margin = (thres * torch.minimum(d, zp) - (d - zp).abs()) / zp.abs().clamp(min=1e-12)
    valid = gt[0] >= 0
    margin = torch.where(valid & finite, margin, torch.full_like(margin, -1.0))
    return dict(vis=(margin > 0) & valid, margin=margin, u=u, v=v, zp=zp, d=d, valid=valid)


def vis_f32(gt, k, curr_w2c, w2c, depth, thres=THRES):
    """The float32 torch route (`losses.visibility_mask`, on the CPU) for one overlapping frame.  It needs gt >= 0 on every
    pixel (it drops the others from its point list and cannot reshape): those pixels are given depth 0 here and are
    ignored by the callers."""
    from diff_gaussian_rasterization.losses import visibility_mask
    clean = torch.where(gt >= 0, gt, torch.zeros_like(gt))
    return visibility_mask(clean, k, curr_w2c, [(w2c, depth)], thres)


def _synthetic(W, H, f, seed):
    """A frame of a slanted, gently curved surface with a pool of four overlapping frames:
       A  shifted so that projections leave the image to the left / top (u, v below -1 and in (-1, 0)), depth map with a
          zero patch and a ripple that crosses the threshold;
       B  shifted the other way (u, v in (W-1, W) / (H-1, H) and beyond), depth map hugging the 5 % threshold;
       C  looks the other way (z' < 0 everywhere);
       D  looks along the current frame's x axis: z' changes sign inside the image, and ONE pixel's depth is set so that
          |z'| < 1e-5.
    gt has a patch of zeros, one negative and one NaN pixel."""
    g = torch.Generator().manual_seed(seed)
    k = torch.tensor([[f, 0, W / 2 - 0.3], [0, f, H / 2 - 0.2], [0, 0, 1.0]])
    ys, xs = torch.meshgrid(torch.arange(H, dtype=torch.float32), torch.arange(W, dtype=torch.float32), indexing="ij")
    surf = lambda x, y: 2.0 + 0.3 * x / W + 0.2 * y / H + 0.05 * torch.sin(x / 7.0) * torch.cos(y / 5.0)
    gt = surf(xs, ys)[None].clone()
    curr = _pose(0.01, -0.02, 0.015, [0.02, -0.01, 0.03])
    px_u, px_v = 1.6 * 2.2 / f, 1.3 * 2.2 / f                   # translations worth about 1.6 / 1.3 pixels at depth 2.2
    poses = {"A": _pose(0.0, 0.0, 0.02, [0.02 - px_u, -0.01 - px_v, 0.03]),
             "B": _pose(0.0, 0.0, -0.02, [0.02 + px_u, -0.01 + px_v, 0.03]),
             "C": _pose(0.0, math.pi, 0.0, [0.0, 0.0, 0.5]),
             "D": _pose(0.0, -math.pi / 2, 0.0, [0.0, 0.0, -0.55])}
    ripple = 0.16 * torch.sin(xs / 3.0 + ys / 4.0)
    depths = {"A": (surf(xs, ys) + ripple)[None].clone(),
              "B": (surf(xs, ys) * (1.05 + 0.01 * torch.sin(xs / 2.0 + ys / 1.5)))[None].clone(),
              "C": (surf(xs, ys) + 0.02 * torch.randn(H, W, generator=g))[None].clone(),
              "D": (0.2 + 0.5 * xs / W + 0.1 * ys / H)[None].clone()}
    depths["A"][:, H // 3:H // 3 + max(2, H // 6), W // 4:W // 4 + 9] = 0.0
    # D: one pixel to |z'| < 1e-5, by bisection on its float32 depth against the float64 projection
    r0, c0 = H // 2, (3 * W) // 4
    probe = gt.clone()

    def zp_at(depth):
        probe[0, r0, c0] = depth
        return float(_project64(probe, k, curr, poses["D"])[2][r0, c0])
    lo, hi = torch.tensor(0.05), torch.tensor(50.0)
    sign_lo = zp_at(lo) < 0
    assert (zp_at(hi) < 0) != sign_lo
    for _ in range(80):
        mid = ((lo.double() + hi.double()) / 2).float()
        zp = zp_at(mid)
        if abs(zp) < 2e-6:
            break
        if (zp < 0) == sign_lo:
            lo = mid
        else:
            hi = mid
    gt[0, r0, c0] = mid
    gt[:, 2 * H // 3:2 * H // 3 + max(1, H // 8), W // 2:W // 2 + 11] = 0.0
    invalid = [(H - 1, 3), (1, W - 5)]
    gt[0, invalid[0][0], invalid[0][1]] = -1.5
    gt[0, invalid[1][0], invalid[1][1]] = float("nan")
    return dict(gt=gt, k=k, curr_w2c=curr, poses=poses, depths=depths, zero_zp_pixel=(r0, c0), invalid=invalid)


def cases():
    """name -> dict(gt [1,H,W], k [3,3], curr_w2c [4,4], frames: [(w2c, depth [1,H,W])] -- the pool the tests draw 0..3
    overlaps from --, invalid: [(row, col)] pixels with gt < 0 or NaN, ref: the reference's own masks or None)."""
    if "cases" in _cache:
        return _cache["cases"]
    fx = fixture()
    out = {"golden": dict(gt=fx["gt_depth"], k=fx["intrinsics"], curr_w2c=fx["curr_w2c"],
                          frames=[(fx[f"overlap{i}_w2c"], fx[f"overlap{i}_gtdepth"]) for i in range(3)], invalid=[],
                          ref=[fx[f"vis_mask{i}"] for i in range(3)])}
    for name, (W, H, f, seed) in {"s67x45": (67, 45, 60.0, 5), "s256x4": (256, 4, 200.0, 6)}.items():
        s = _synthetic(W, H, f, seed)
        out[name] = dict(gt=s["gt"], k=s["k"], curr_w2c=s["curr_w2c"], frames=[(s["poses"][n], s["depths"][n]) for n in "ABCD"],
                         invalid=s["invalid"], ref=None, zero_zp_pixel=s["zero_zp_pixel"])
    _cache["cases"] = out
    return out


def f64_of(name):
    """The float64 restatement of every frame of the case's pool, computed once."""
    key = ("f64", name)
    if key not in _cache:
        c = cases()[name]
        _cache[key] = [vis_f64(c["gt"], c["k"], c["curr_w2c"], w, d) for w, d in c["frames"]]
    return _cache[key]


def measure_tau():
    """(tau, worst, floor): worst = the largest |margin| at which the float32 torch route (`losses.visibility_mask` on the
    CPU) disagrees with the float64 restatement over all frames of all cases of this file; tau = 4 x worst, with a floor of
    4 float32 ulps.  The rule of keyframe_util.measure_tau; never taken from the kernel under test."""
    if "tau" not in _cache:
        worst = 0.0
        for name, c in cases().items():
            for (w, d), r in zip(c["frames"], f64_of(name)):
                m32 = vis_f32(c["gt"], c["k"], c["curr_w2c"], w, d)
                diff = (m32 != r["vis"]) & r["valid"]
                if diff.any():
                    worst = max(worst, float(r["margin"][diff].abs().max()))
        floor = 4 * EPS32
        _cache["tau"] = (max(4 * worst, floor), worst, floor)
    return _cache["tau"]


def band_of(name, frames):
    """[H,W] bool: pixels where the decision of one of the pool frames `frames` lies inside the band.  Asserts the condition
    the band rule rests on: in-band pixels are at most BAND_SHARE of the case's pixels (float64 restatement alone)."""
    tau = measure_tau()[0]
    rs = f64_of(name)
    band = torch.zeros_like(rs[0]["vis"])
    for j in frames:
        band |= rs[j]["margin"].abs() < tau
    share = band.double().mean().item()
    assert share <= BAND_SHARE, (name, frames, share, tau)
    return band


def band_shares():
    """name -> the largest in-band share over the single frames and over all frames of the pool together."""
    out = {}
    for name, c in cases().items():
        n = len(c["frames"])
        out[name] = max([band_of(name, [j]).double().mean().item() for j in range(n)] +
                        [band_of(name, list(range(n))).double().mean().item()])
    return out


def situations(name):
    """Counts, in the float64 evaluation, of the situations the synthetic cases place by hand."""
    c, rs = cases()[name], f64_of(name)
    H, W = c["gt"].shape[-2:]
    ok = torch.stack([r["valid"] & (c["gt"][0] > 0) for r in rs])
    u, v, zp, d = (torch.stack([r[key] for r in rs]) for key in ("u", "v", "zp", "d"))
    inside = (u > 0) & (u < W - 1) & (v > 0) & (v < H - 1)
    cnt = lambda m: int((m & ok).sum())
    r0, c0 = c["zero_zp_pixel"]
    return {"u in (-1,0)": cnt((u > -1) & (u < 0)), "u in (W-1,W)": cnt((u > W - 1) & (u < W)), "u < -1": cnt(u < -1), "u > W": cnt(u > W),
            "v in (-1,0)": cnt((v > -1) & (v < 0)), "v in (H-1,H)": cnt((v > H - 1) & (v < H)), "v < -1": cnt(v < -1), "v > H": cnt(v > H),
            "one-tap corner": cnt((u > -1) & (u < 0) & (v > -1) & (v < 0)) + cnt((u > W - 1) & (u < W) & (v > H - 1) & (v < H)),
            "zp < 0": cnt(zp < 0), "|zp| < 1e-5": int(sum(abs(float(r["zp"][r0, c0])) < 1e-5 for r in rs)),
            "gt == 0": int((c["gt"][0] == 0).sum()), "gt < 0": int((c["gt"][0] < 0).sum()), "gt NaN": int(torch.isnan(c["gt"][0]).sum()),
            "zero taps inside": cnt(inside & (d == 0)), "partly zero taps": cnt(inside & (d > 0) & (d < 0.5 * zp) & (zp > 0)),
            "visible": int(torch.stack([r["vis"] for r in rs]).sum()), "hidden inside": cnt(inside & (d > 0) & (zp > 0)) -
            int((torch.stack([r["vis"] for r in rs]) & inside).sum())}
