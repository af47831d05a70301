"""Times keyframe overlap counting: vtgs_keyframe_overlap (one pass over points x keyframes, one host read) against the
reference's route -- the per-keyframe torch loop of keyframe_selection_overlap_visbased with a grid_sample and a host-compared
sum per keyframe, restated here device-agnostically -- on the same GPU, in the same process, keyframes already resident
(which favours the torch route: the reference copies every keyframe to the device and back on every call).

    python tools/keyframe_overlap_timing.py [--out profiles/keyframe_overlap_timing.md]

HIP events around warmed repetitions; the host read of the counts is inside both timed regions.
"""
import argparse
import os
import sys

import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "vtgaussian-slam_amd"))


def torch_route(gt_depth, w2c, k, poses, depths, edge, thresh, rc=None, with_counts=False):
    """The reference's steps (utils/keyframe_selection.py:10-37, 136-190) on whatever device the tensors live on."""
    H, W = gt_depth.shape[-2:]
    if rc is None:
        rc = torch.stack(torch.where(gt_depth[0] > 0), dim=1)
    xx = (rc[:, 1] - k[0][2]) / k[0][0]
    yy = (rc[:, 0] - k[1][2]) / k[1][1]
    z = gt_depth[0, rc[:, 0], rc[:, 1]]
    pc = torch.stack((xx * z, yy * z, z), dim=-1)
    pts = (torch.inverse(w2c) @ torch.cat([pc, torch.ones_like(pc[:, :1])], dim=1).T).T[:, :3]
    a = torch.abs(torch.round(pts, decimals=4))
    _, idx, counts = torch.cat([a, torch.zeros((1, 3), device=a.device)], dim=0).unique(dim=0, return_inverse=True, return_counts=True)
    pts = pts[~torch.isin(idx, torch.where(counts.gt(1))[0])[:len(a)]]
    out = []
    for j in range(poses.shape[0]):
        p4 = torch.cat([pts, torch.ones_like(pts[:, :1])], dim=1)
        tp = (poses[j] @ p4.T).T[:, :3]
        p2 = torch.matmul(k, tp.transpose(0, 1)).transpose(0, 1)
        pz = p2[:, 2:] + 1e-5
        pr = (p2 / pz)[:, :2]
        m = (pr[:, 0] < W - edge) * (pr[:, 0] > edge) * (pr[:, 1] < H - edge) * (pr[:, 1] > edge)
        m = m & (pz[:, 0] > 0)
        if thresh is not None:
            grid = pr.reshape(1, 1, -1, 2).clone()
            grid[..., 0] = grid[..., 0] / (W - 1) * 2.0 - 1.0
            grid[..., 1] = grid[..., 1] / (H - 1) * 2.0 - 1.0
            ds = F.grid_sample(depths[j].reshape(1, 1, H, W), grid, padding_mode="zeros", align_corners=True).reshape(-1)
            m = m & (torch.abs(ds - pz[:, 0]) < thresh * torch.min(ds, pz[:, 0]))
        out.append({"id": j, "percent_inside": m.sum() / pr.shape[0], "count": m.sum()})
    out = sorted(out, key=lambda i: i["percent_inside"], reverse=True)               # K host reads, as in the reference
    selected = [d["id"] for d in out if d["percent_inside"] > 0.0]
    if not with_counts:
        return selected
    counts = [0] * len(out)
    for d in out:
        counts[d["id"]] = int(d["count"])
    return selected, counts, pts.shape[0]


def timed(fn, warm=3, reps=10):
    for _ in range(warm):
        fn()
    torch.cuda.synchronize()
    t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    times = []
    for _ in range(reps):
        t0.record()
        fn()
        t1.record()
        t1.synchronize()
        times.append(t0.elapsed_time(t1))
    times.sort()
    return times[len(times) // 2]


def scene(W, H, K, dev, seed=0):
    g = torch.Generator().manual_seed(seed)
    d = 1.8 + 0.9 * torch.rand(1, H, W, generator=g)
    d[torch.rand(1, H, W, generator=g) < 0.05] = 0.0
    k = torch.tensor([[0.9 * W, 0, W / 2 - 0.37], [0, 0.9 * W, H / 2 + 0.21], [0, 0, 1.0]])
    w2c = torch.eye(4)
    w2c[:3, 3] = torch.tensor([0.02, -0.01, 0.03])
    poses = torch.eye(4).repeat(K, 1, 1)
    poses[:, :3, 3] = (torch.rand(K, 3, generator=g) * 2 - 1) * torch.tensor([0.3, 0.2, 0.05])
    depths = (d * (1 + 0.02 * torch.randn(K, H, W, generator=g))).clamp(min=0)
    return d.to(dev), w2c.to(dev), k.to(dev), poses.to(dev), depths.to(dev)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "keyframe_overlap_timing.md"))
    args = ap.parse_args()
    from diff_gaussian_rasterization import keyframes as kf
    dev = torch.device("cuda:0")
    rows = []
    for (W, H) in ((1200, 680), (640, 480)):
        for K in (4, 16, 64):
            gd, w2c, k, poses, depths = scene(W, H, K, dev)
            store = kf.KeyframeStore(H, W, capacity=K, device=dev)
            for j in range(K):
                store.append(poses[j], depths[j])
            for mode in ("dense", "sampled 1600"):
                rc = None
                if mode != "dense":
                    valid = torch.stack(torch.where(gd[0] > 0), dim=1)
                    rc = valid[torch.randint(valid.shape[0], (1600,), generator=torch.Generator().manual_seed(1)).to(dev)]
                thresh = 0.03 if rc is None else None                     # the reference's sampled form has no visibility test
                native = lambda: kf.overlap_counts(gd, w2c, k, store, sampled_indices=rc, edge_value=20,
                                                   kf_depth_thresh=thresh).cpu()
                route = lambda: torch_route(gd, w2c, k, poses, depths, 20, thresh, rc)
                rec = native().numpy()
                want, want_counts, want_n = torch_route(gd, w2c, k, poses, depths, 20, thresh, rc, with_counts=True)
                got = [int(i) for i in kf.select_overlap(rec[:K], rec[K], K)]
                # the counts themselves against the torch route's mask.sum() (it also drops coincident-rounding pairs, and a
                # pair on a float32 decision edge may fall either way), and the ORDERED selection
                worst = max(abs(int(a) - b) for a, b in zip(rec[:K], want_counts))
                agree = f"{worst} / {int(rec[K]) - want_n} / {got == want}"
                tn, tt = timed(native), timed(route)
                kept = int(rec[K])
                gbytes = (W * H * 4 + (16 * kept * K if thresh is not None else 0)) / 1e9
                rows.append((f"{W}x{H}", K, mode, kept, tn, tt, tt / tn, gbytes / (tn * 1e-3), agree))
                print(rows[-1], flush=True)
    lines = ["# Keyframe overlap counting: vtgs_keyframe_overlap against the reference's per-keyframe torch route", "",
             "MI355X, HIP events, median of 10 after 3 warm-up calls; both routes end with their host read; keyframes resident.",
             "`GB/s` = the native call's algorithmic bytes (source depth once + 4 taps x kept points x K) over its whole time.",
             "`agreement` = largest |count difference| over the keyframes / difference of the kept-point counts / same ORDERED",
             "selection, native against the torch route (which also drops coincident-rounding pairs).", "",
             "| frame | K | mode | kept points | native ms | torch route ms | ratio | native GB/s | agreement |",
             "|---|---|---|---|---|---|---|---|---|"]
    for r in rows:
        lines.append(f"| {r[0]} | {r[1]} | {r[2]} | {r[3]} | {r[4]:.3f} | {r[5]:.3f} | {r[6]:.1f} | {r[7]:.1f} | {r[8]} |")
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        f.write("\n".join(lines) + "\n")
    print("wrote", args.out)


if __name__ == "__main__":
    main()
