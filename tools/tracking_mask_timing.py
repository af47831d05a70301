"""Times the detached masks of a tracking iteration (TUM: one overlapping frame, ScanNet(++): three; with and without the
outlier-depth mask; far filter on): the torch chain of get_loss (`losses.visibility_mask`, `outlier_depth_mask`,
`far_depth_mask`, the ANDs and the conversion to the loss node's float mask) against the one native call
`losses.tracking_extra_mask` -- same checkout, same GPU, same process, alternating.

    python tools/tracking_mask_timing.py [--out profiles/tracking_mask_timing.md]
    rocprofv3 --kernel-trace --output-format csv -d DIR -o run -- python tools/tracking_mask_timing.py --segments
    python tools/tracking_mask_timing.py --count-trace DIR [--out ...]      # appends the launch counts to the note

Times: HIP events around warmed repetitions, median.  Host wait: with some ten ms of matrix products queued in front, the
host time until the call returns -- a route that waits for the device returns only after them.  Launch counts: a kernel
trace of its own (--segments runs every route ten times between marker kernels; --count-trace counts the rows).
"""
import argparse
import csv
import glob
import os
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "vtgaussian-slam_amd"))
W, H = 1200, 680
CONFIGS = [(1, False), (1, True), (3, False), (3, True)]          # (overlapping frames, outlier mask)
REPS = 10


def scene(dev, seed=0):
    g = torch.Generator().manual_seed(seed)
    gt = 1.8 + 0.9 * torch.rand(1, H, W, generator=g)
    gt[torch.rand(1, H, W, generator=g) < 0.05] = 0.0
    k = torch.tensor([[0.9 * W, 0, W / 2 - 0.37], [0, 0.9 * W, H / 2 + 0.21], [0, 0, 1.0]])
    curr = torch.eye(4)
    curr[:3, 3] = torch.tensor([0.02, -0.01, 0.03])
    overlaps = []
    for i in range(3):
        o = torch.eye(4)
        o[:3, 3] = torch.tensor([0.05 * (i + 1), -0.03, 0.01 * i])
        overlaps.append((o.to(dev), (gt * (1 + 0.03 * torch.randn(1, H, W, generator=g))).clamp(min=0).to(dev)))
    rendered = (gt * (1 + 0.01 * torch.randn(1, H, W, generator=g))).to(dev)
    return gt.to(dev), k.to(dev), curr.to(dev), overlaps, rendered


def routes(losses, gt, k, curr, overlaps, rendered, n, outlier, far=2.5):
    def torch_route():
        m = losses.visibility_mask(gt, k, curr, overlaps[:n], 0.05)[None]
        if outlier:
            m = losses.outlier_depth_mask(gt, rendered) & m
        m = m & losses.far_depth_mask(gt, far)
        return m.to(torch.float32)                    # what the loss node does with a bool mask

    def native_route():
        return losses.tracking_extra_mask(gt, k, curr, overlaps[:n], 0.05, far, rendered if outlier else None)
    return torch_route, native_route


def timed(fn, warm=3, reps=20):
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
    return times[len(times) // 2], times[0], times[-1]


def host_return_ms(fn, a):
    """Host time until fn() returns with a chain of matrix products queued in front of it, and the device time of that chain."""
    torch.cuda.synchronize()
    t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    t0.record()
    b = a
    for _ in range(12):
        b = (a @ b) * 1e-4
    t1.record()
    h0 = time.perf_counter()
    fn()
    h1 = time.perf_counter()
    torch.cuda.synchronize()
    return (h1 - h0) * 1e3, t0.elapsed_time(t1)


def segments():
    from diff_gaussian_rasterization import losses
    dev = torch.device("cuda:0")
    gt, k, curr, overlaps, rendered = scene(dev)
    marker = torch.linspace(-0.5, 0.5, 8, device=dev)
    for n, outlier in CONFIGS:
        for fn in routes(losses, gt, k, curr, overlaps, rendered, n, outlier):
            fn()
            torch.cuda.synchronize()
            torch.erfinv(marker)                      # marker kernel: no route launches an erfinv
            for _ in range(REPS):
                fn()
            torch.cuda.synchronize()
            torch.erfinv(marker)                      # and one behind: the next route's warm-up call is in no segment
    torch.cuda.synchronize()


def count_trace(directory):
    """Kernel launches per call of every (config, route) segment of a --segments trace: the rows between the marker kernel in
    front of a segment and the one behind it (every other interval; the intervals between them hold the warm-up calls)."""
    files = sorted(glob.glob(os.path.join(directory, "**", "*kernel_trace.csv"), recursive=True))
    if not files:
        raise SystemExit(f"no kernel trace under {directory}")
    rows = sorted(((int(r["Start_Timestamp"]), r["Kernel_Name"]) for r in csv.DictReader(open(files[0]))))
    counts, cur, names, seen = [], 0, set(), False
    for _, name in rows:
        if "erfinv" in name.lower():
            if seen:
                counts.append((cur, sorted(names)))
            seen, cur, names = True, 0, set()
        elif seen:
            cur += 1
            names.add(name.split("(")[0][:60])
    labels = [(n, o, r) for n, o in CONFIGS for r in ("torch", "native")]
    assert len(counts) == 2 * len(labels) - 1, (len(counts), len(labels))
    return [(lab, c / REPS, nm) for lab, (c, nm) in zip(labels, counts[0::2])]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "tracking_mask_timing.md"))
    ap.add_argument("--segments", action="store_true")
    ap.add_argument("--count-trace", default=None)
    args = ap.parse_args()
    if args.segments:
        return segments()
    if args.count_trace:
        lines = ["", "## Kernel launches per call (kernel trace alone, ten calls per segment)", "",
                 "The native route's one fill in front of the select (a memset, no kernel) is not in these counts.", "",
                 "| overlaps | outlier mask | route | kernel launches per call |", "|---|---|---|---|"]
        for (n, o, r), c, _ in count_trace(args.count_trace):
            lines.append(f"| {n} | {'yes' if o else 'no'} | {r} | {c:.1f} |")
        with open(args.out, "a") as f:
            f.write("\n".join(lines) + "\n")
        print("\n".join(lines))
        return
    from diff_gaussian_rasterization import losses
    dev = torch.device("cuda:0")
    gt, k, curr, overlaps, rendered = scene(dev)
    a = torch.randn(4096, 4096, device=dev)
    rows = []
    for n, outlier in CONFIGS:
        t_fn, n_fn = routes(losses, gt, k, curr, overlaps, rendered, n, outlier)
        differ = int((t_fn() != n_fn()).sum())
        tt, tn = timed(t_fn), timed(n_fn)
        tt2, tn2 = timed(t_fn), timed(n_fn)                      # again, alternating: the spread between two windows
        ht, queued_t = host_return_ms(t_fn, a)
        hn, queued_n = host_return_ms(n_fn, a)
        rows.append((n, outlier, tt, tt2, tn, tn2, differ, ht, queued_t, hn, queued_n))
        print(rows[-1], flush=True)
    lines = ["# Tracking masks: the torch chain of get_loss against vtgs_tracking_mask", "",
             f"MI355X, {W}x{H}, far filter on, HIP events, median of 20 after 3 warm-up calls (min .. max), two windows per route,",
             "alternating; both routes end with the float32 mask the loss node reads.  `differ` = pixels where the two masks differ",
             "(visibility decisions within float32 rounding of the threshold).  `host return` = host time until the call returns",
             "with `queued` ms of matrix products in front of it on the stream: a route that waits for the device cannot return",
             "before they finish.", "",
             "| overlaps | outlier mask | torch ms | torch ms (2nd) | native ms | native ms (2nd) | ratio | differ | torch host return / queued ms | native host return / queued ms |",
             "|---|---|---|---|---|---|---|---|---|---|"]
    f3 = lambda t: f"{t[0]:.3f} ({t[1]:.3f} .. {t[2]:.3f})"
    for n, o, tt, tt2, tn, tn2, differ, ht, qt, hn, qn in rows:
        lines.append(f"| {n} | {'yes' if o else 'no'} | {f3(tt)} | {f3(tt2)} | {f3(tn)} | {f3(tn2)} | {tt[0] / tn[0]:.1f} | {differ} | "
                     f"{ht:.2f} / {qt:.1f} | {hn:.2f} / {qn:.1f} |")
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        f.write("\n".join(lines) + "\n")
    print("wrote", args.out)


if __name__ == "__main__":
    main()
