"""Timing of the densification step at the Replica frame size (1200 x 680, 2400 x 1360 densification frame, ~2.8 k
original-resolution rows per frame like the slam block of bench_slam.py), hipEvent medians of
  (a) the torch sequence of bench_slam.py's densification block behind its render (masks, median, nonzero, the one-in-twelve
      dense stand-in, torch.inverse, five torch.cat onto the map), as it stands;
  (b) vtgs_densify in resident form (the map keeps slack rows; one call, no host wait),
and the per-kernel split of (b) from vtgs_profile_collect.  Run it on the GPU machine under its own timeout:

    timeout -k 10 300 python tools/densify_timing.py [--out profiles/r8_densify.md] [--n 1000000] [--reps 30]
"""
import argparse
import os
import statistics
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "vtgaussian-slam_amd")]
import diff_gaussian_rasterization as dgr  # noqa: E402
import slam_callers as sc  # noqa: E402
from diff_gaussian_rasterization import densify as dz  # noqa: E402

KEYS = {"means3D": 3, "rgb_colors": 3, "unnorm_rotations": 4, "logit_opacities": 1, "log_scales": 1}


def frames(dev, W, H, seed=3):
    g = torch.Generator().manual_seed(seed)
    gd = 1.5 + 2.5 * torch.rand(H, W, generator=g)
    rd = gd + 0.002 * torch.randn(H, W, generator=g)
    sil = torch.ones(H, W)
    sil[100:140, 300:370] = 0.1                                      # 2,800 pixels the map does not explain
    gt_im = torch.rand(3, H, W, generator=g)
    up = lambda x: x.repeat_interleave(2, -2).repeat_interleave(2, -1)
    mask = (torch.rand(H, W, generator=g) < 1.0 / 3.0).to(torch.uint8)   # the slam block takes 4 sub-pixels of one hole pixel in 12
    return {k: v.to(dev).contiguous() for k, v in dict(gd=gd, ds=torch.stack([rd, sil, rd * rd]), gt_im=gt_im, gd_d=up(gd),
                                                       gt_im_d=up(gt_im), mask=mask).items()}


def torch_sequence(f, params, t, W, H, dev):
    """bench_slam.py's block behind render_pair, line for line (the map grows by torch.cat)."""
    ds, gd = f["ds"], f["gd"]
    sil, rd = ds[1], ds[0]
    err = (gd - rd).abs() * (gd > 0)
    hole = (sil < 0.5) | ((rd > gd) & (err > 50 * err.median()))
    idx = (hole & (gd > 0)).reshape(-1).nonzero().reshape(-1)
    if not idx.numel():
        return 0, params
    fxy = W / 2.0
    px, py = (idx % W).float(), (idx // W).float()
    dense = idx[idx % 12 == 0]
    if dense.numel():
        off = torch.tensor([[-0.25, -0.25], [0.25, -0.25], [-0.25, 0.25], [0.25, 0.25]], device=dev)
        dx = ((dense % W).float()[:, None] + off[None, :, 0]).reshape(-1)
        dy = ((dense // W).float()[:, None] + off[None, :, 1]).reshape(-1)
        px, py = torch.cat([px, dx]), torch.cat([py, dy])
        src = torch.cat([idx, dense.repeat_interleave(4)])
        half = torch.cat([torch.ones(idx.numel(), device=dev), torch.full((4 * dense.numel(),), 0.5, device=dev)])
    else:
        src, half = idx, torch.ones(idx.numel(), device=dev)
    z = gd.reshape(-1)[src] * 1.005
    pts_cam = torch.stack([(px - (W / 2.0 - 0.5) + 0.5) / fxy * z, (py - (H / 2.0 - 0.5) + 0.5) / fxy * z, z, torch.ones_like(z)], 1)
    w2c_t = torch.eye(4, device=dev)
    w2c_t[:3, :3] = sc.build_rotation(torch.nn.functional.normalize(params["cam_unnorm_rots"][..., t].detach()))
    w2c_t[:3, 3] = params["cam_trans"][0, :, t].detach()
    new = {"means3D": (torch.inverse(w2c_t) @ pts_cam.T).T[:, :3].contiguous(),
           "rgb_colors": f["gt_im"].reshape(3, -1).T[src].contiguous(),
           "unnorm_rotations": torch.tensor([1.0, 0, 0, 0], device=dev).repeat(src.numel(), 1),
           "logit_opacities": torch.zeros(src.numel(), 1, device=dev),
           "log_scales": torch.log(z / fxy * half)[:, None]}
    grown = dict(params)
    for k, v in new.items():
        grown[k] = torch.nn.Parameter(torch.cat([params[k].detach(), v], 0))
    return src.numel(), grown


def event_median(fn, reps, warmup=3):
    ms = []
    for i in range(warmup + reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        if i >= warmup:
            ms.append(a.elapsed_time(b))
    return statistics.median(ms), min(ms), max(ms)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r8_densify.md"))
    ap.add_argument("--n", type=int, default=1_000_000)
    ap.add_argument("--reps", type=int, default=30)
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    W, H, N, T, t = 1200, 680, args.n, 8, 3
    f = frames(dev, W, H)
    g = torch.Generator().manual_seed(1)
    params = {k: torch.rand(N, c, generator=g).to(dev) for k, c in KEYS.items()}
    params["cam_unnorm_rots"] = (torch.tensor([1.0, 0.02, -0.03, 0.01]).reshape(1, 4, 1).repeat(1, 1, T)).to(dev)
    params["cam_trans"] = (0.05 * torch.randn(1, 3, T, generator=g)).to(dev)
    k = torch.tensor([[W / 2.0, 0, W / 2.0 - 0.5], [0, W / 2.0, H / 2.0 - 0.5], [0, 0, 1.0]], device=dev)
    k_d = torch.tensor([[float(W), 0, W - 0.5], [0, float(W), H - 0.5], [0, 0, 1.0]], device=dev)

    added_a, _ = torch_sequence(f, params, t, W, H, dev)
    med_a = event_median(lambda: torch_sequence(f, params, t, W, H, dev), args.reps)

    slack = 1 << 16
    arrays = {key: torch.empty(N + slack, c, device=dev) for key, c in KEYS.items()}
    arrays["timestep"] = torch.empty(N + slack, device=dev)
    kw = dict(gt_im=f["gt_im"], gt_depth=f["gd"], intrinsics=k, depth_sil=f["ds"], dense=(f["gt_im_d"], f["gd_d"], k_d),
              mask_variation=f["mask"], cam=(params["cam_unnorm_rots"], params["cam_trans"], t), sil_thres=0.5, time_idx_value=float(t))
    info = dz.read_info(dz.densify_into(arrays, N, N + slack, **kw))
    assert info["overflow"] == 0 and info["added_ori"] > 0, info
    med_b = event_median(lambda: dz.densify_into(arrays, N, N + slack, **kw), args.reps)
    dgr.profile_enable(True)
    for _ in range(args.reps):
        dz.densify_into(arrays, N, N + slack, **kw)
    prof = dgr.profile_collect()
    dgr.profile_enable(False)
    lines = ["# Densification step: torch sequence vs vtgs_densify (tools/densify_timing.py)", "",
             f"MI355X, {W} x {H} frame, {2 * W} x {2 * H} densification frame, map of {N:,} Gaussians, hipEvent medians of {args.reps} "
             "calls (min .. max in brackets), one stream.", "",
             "| route | new rows | ms per call |", "|---|---|---|",
             f"| (a) torch sequence of bench_slam.py's block behind its render (median, masks, nonzero, one-in-twelve dense stand-in, "
             f"torch.inverse, five torch.cat onto the map) | {added_a:,} | {med_a[0]:.3f} ({med_a[1]:.3f} .. {med_a[2]:.3f}) |",
             f"| (b) vtgs_densify, resident form through densify_into (exact 2x dense set, no host wait, no copy of the map) | "
             f"{info['added_ori']:,} + {info['added_dense']:,} | {med_b[0]:.3f} ({med_b[1]:.3f} .. {med_b[2]:.3f}) |", "",
             "Per kernel of (b), from vtgs_profile_collect (event brackets around each command; every bracket adds the cost of its "
             "two event records, so the rows sum to more than the unbracketed call above):", "",
             "| command | launches | us per launch |", "|---|---|---|"]
    total = 0.0
    for name, (ms, launches) in prof.items():
        lines.append(f"| {name} | {launches} | {1e3 * ms / max(launches, 1):.1f} |")
        total += 1e3 * ms / max(launches, 1)
    lines += [f"| sum | | {total:.1f} |", ""]
    text = "\n".join(lines)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as fh:
        fh.write(text + "\n")
    print(text)


if __name__ == "__main__":
    main()
