#!/usr/bin/env python3
"""Headline benchmark: rasterize forward+backward throughput (Mgaussians*pixels/s), BASELINE.json metric.

    python bench.py --gpus 1 --steps 50 --warmup 10
    python bench.py --gpus N ...          # starts its own N ranks (torch.distributed.run) when WORLD_SIZE is unset
    python -m torch.distributed.run --nnodes=1 --nproc-per-node N --master-addr 127.0.0.1 --master-port P \
           bench.py --gpus N --steps K --warmup W

One step = one full pass of the hot path through the drop-in operator: GaussianRasterizer forward
(projection, tile bucketing, per-tile sort, composite of colour+depth) and backward (gradients to all six
tensor inputs) on the synthetic view-tied scene of SURVEY.md 8(d): N = 1 M isotropic Gaussians, 1200x680,
inputs resident in HBM.  With N > 1 GPUs the image is partitioned into bands of 16-pixel tile rows (one band
per rank, Gaussians replicated) and the 7-float pose gradient is all-reduced over RCCL each step (strong
scaling: the total work is fixed).

Prints ONE JSON line on rank 0.  A plain run does what the headline needs and no more: scene set-up, clock ramp,
--warmup steps, --steps timed steps (`ms_per_step`, `value`), the --dump-outputs files if asked for, the line.

    python bench.py --gpus 1 --steps 50 --warmup 10 --full
    python bench.py ... --dump-outputs DIR    # DIR/<name>.npy: what the last timed step returned (same inputs every run)

--full adds every other measurement and check to the line: the cold first region, per-step event percentiles,
the tracking / mapping steps, `roofline` for the dominant kernel, timed live with HIP events on the stream it runs
on (vtgs_profile_*), `cpu_baseline` (the float32 oracle on a bounded band of the same scene), the audited float64
`parity` block and the `slam` block.
"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.abspath(__file__))
for p in (ROOT, os.path.join(ROOT, "vtgaussian-slam_amd"), os.path.join(ROOT, "tests")):
    if p not in sys.path:
        sys.path.insert(0, p)

import torch  # noqa: E402

HBM_PEAK_GBS = 8000.0     # MI355X_MICROARCH.md: HBM3E 8.0 TB/s spec
FP32_PEAK_TFLOPS = 157.3  # MI355X_MICROARCH.md: peak FP32 vector (= f32 MFMA) rate
# SURVEY.md 8(d) secondary bound: per (pixel, Gaussian) evaluation the forward costs ~14 flop + 1 exp, the backward ~3x
# that; v_exp_f32 occupies the issue slot of three v_fma_f32 (tests/micro/issue_rate.hip, profiles/r2_issue_rates.md) = 6 flop.
FLOP_PER_EVAL_FWD_BWD = 4 * (14 + 6)


def self_launch(args) -> int:
    """`python bench.py --gpus N` outside torch.distributed.run: start N ranks as CHILD processes (one per GPU, RCCL
    rendezvous on 127.0.0.1) and pass rank 0's JSON line through.  Nothing in this process has touched the GPU yet
    (importing torch does not), and nothing is exec'ed: the children are fresh interpreters."""
    import socket
    import subprocess
    with socket.socket() as sock:
        sock.bind(("127.0.0.1", 0))
        port = sock.getsockname()[1]
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", f"--nproc-per-node={args.gpus}",
           "--master-addr", "127.0.0.1", "--master-port", str(port), os.path.abspath(__file__)] + sys.argv[1:]
    env = dict(os.environ)
    env.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")
    env.setdefault("OMP_NUM_THREADS", "4")
    proc = subprocess.run(cmd, env=env, stdout=subprocess.PIPE, text=True)
    line = None
    for ln in proc.stdout.splitlines():
        if ln.startswith("{") and '"metric"' in ln:
            line = ln
        else:
            print(ln, file=sys.stderr)
    if line is not None:
        print(line)
    return proc.returncode if line is not None or proc.returncode else 1


def kernel_algorithmic_bytes(n, p, r16, grad_bytes=68):
    """B_alg = 180 N + 28 P + 52 R per fwd+bwd call, split over the kernels that own each term
    (DESIGN.md section 3).  R = 16x16 tiles touched, counted by the op."""
    return {
        "project_and_bin": 44 * n + 12 * r16,            # means/scales/rot/opacity read + key/value emit
        "finalize_forward": 8 * r16,                     # tile ranges
        "sort_tiles": 24 * r16,                          # sort read + sort write
        "composite_forward": 12 * n + 4 * r16 + 16 * p,  # colours read + id read + colour/depth out
        "composite_backward": 12 * n + 4 * r16 + 12 * p, # colours re-read + id read + grad_color in
        "gather_splat_grads": 44 * n + grad_bytes * n,   # params re-read + the gradients asked for (68 B: all six)
    }


DUMP_BUDGET_BYTES = 60_000_000   # --dump-outputs: all files together stay under 64 MB


def dump_outputs(dirname, images, per_gaussian, n):
    """--dump-outputs: the arrays a caller of the timed step holds after it, as <dirname>/<name>.npy in float32.  `images` end in
    (H, W), `per_gaussian` arrays (radii, the gradients; saved as radii.npy / grad_<input>.npy) have n rows.  Whole arrays while
    they fit the budget; beyond it the images keep a fixed, seeded sample of pixels (at most half the budget) and the
    per-Gaussian arrays the same fixed, seeded sample of rows each, in ascending order."""
    import numpy as np

    def pick(items, bytes_per_item, budget, seed):
        keep = int(budget // max(bytes_per_item, 1))
        if keep >= items:
            return None
        return torch.randperm(items, generator=torch.Generator().manual_seed(seed))[:keep].sort().values

    os.makedirs(dirname, exist_ok=True)
    images = {k: v.detach().float().cpu() for k, v in images.items() if v is not None}
    rows = {k: v.detach().float().cpu() for k, v in per_gaussian.items() if v is not None}
    out = {}
    img_bytes = sum(4 * v.numel() for v in images.values())
    pixels = next(iter(images.values())).shape[-2:].numel() if images else 0
    pix = pick(pixels, img_bytes // max(pixels, 1), min(img_bytes, DUMP_BUDGET_BYTES // 2), 11) if images else None
    for k, v in images.items():
        out[k] = v if pix is None else v.reshape(-1, pixels)[:, pix]
    left = DUMP_BUDGET_BYTES - sum(4 * v.numel() for v in out.values())
    sel = pick(n, sum(4 * v.numel() // n for v in rows.values()), left, 12)
    for k, v in rows.items():
        out[k] = v if sel is None else v[sel]
    for k, v in out.items():
        np.save(os.path.join(dirname, k + ".npy"), np.ascontiguousarray(v.numpy(), dtype=np.float32))
    print(f"[bench] outputs of the last timed step: {sorted(out)} -> {dirname} "
          f"({sum(4 * v.numel() for v in out.values()) / 1e6:.1f} MB" +
          ("" if sel is None else f", {sel.numel()} of {n} Gaussians") + ("" if pix is None else f", {pix.numel()} of {pixels} pixels") + ")",
          file=sys.stderr, flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--n", type=int, default=1_000_000)
    ap.add_argument("--width", type=int, default=1200)
    ap.add_argument("--height", type=int, default=680)
    ap.add_argument("--ramp-ms", type=float, default=250.0,
                    help="untimed steps for this many milliseconds before the --warmup steps: the GPU's clocks after the idle "
                         "scene set-up (0 = none); reported as `clock_ramp`")
    ap.add_argument("--cpu-rows", type=int, default=1000, help="16-px tile rows rendered by the CPU baseline sample")
    ap.add_argument("--no-cpu-baseline", action="store_true")
    ap.add_argument("--audit-rows", default="4,19,20,21,22,37", help="16-px tile rows of the frame audited against the float64 oracle "
                                                             "('' = skip the parity block)")
    ap.add_argument("--slam-frames", type=int, default=41, help="frames of the tracking+mapping loop in the `slam` block "
                                                               "(BASELINE.json metric 2; 0 = skip)")
    ap.add_argument("--mode", default=None, choices=["rasterize", "tracking", "mapping"],
                    help="which gradients a step asks for.  rasterize (default at EVERY N, SURVEY 8d metric 1): all six inputs.  "
                         "tracking (SURVEY 8e): the Gaussians are detached as in the reference's tracking "
                         "loop (src/vtgaussian_slam.py:428-449) -- means3D + the screen-space term, 24 B per Gaussian written "
                         "instead of 68 -- then the 7-float pose reduction and its all-reduce.  mapping: colours, opacities, "
                         "scales (the trainable set of the mapping loop), one flat all-reduce of 28 B per Gaussian")
    ap.add_argument("--owned-sets", action="store_true",
                    help="bands (N > 1 or --band): run the per-Gaussian kernels over the list of Gaussians that can meet the band "
                         "(partition.OwnedSet) instead of over the whole map.  Off by default: through the plain operator the list "
                         "is an index_select / index_add pair per input, which costs more than the shorter kernels save below "
                         "a few million Gaussians (DESIGN.md 5); the fused frame route (bench_slam.py) gathers inside its kernels")
    ap.add_argument("--band", default=None, metavar="R/W",
                    help="rehearsal on one GPU: run rank R's band of a W-rank tile-row partition in this process, without "
                         "collectives (per-rank kernel times and the replicated share; tools/band_rehearsal.sh)")
    ap.add_argument("--backend", default="nccl", help="torch.distributed backend (nccl = RCCL; gloo only to rehearse "
                                                      "the multi-rank path with all ranks on one GPU)")
    ap.add_argument("--full", action="store_true",
                    help="after the headline region, also measure and check everything else the line can carry: the cold first "
                         "region, per-step hipEvent percentiles, the tracking / mapping steps, per-kernel times + roofline, the CPU "
                         "baseline, the audited float64 parity block, the SLAM block and (N > 1) the per-rank record.  Without it "
                         "the run sets up, ramps the clocks, warms up, times --steps steps and prints the line")
    ap.add_argument("--dump-outputs", default=None, metavar="DIR",
                    help="after the timed steps, write what the LAST timed step returned to its caller -- color, radii, depth and the "
                         "gradient of every input the mode asks for -- as DIR/<name>.npy (float32; at most 64 MB in all: beyond that "
                         "the per-Gaussian arrays keep a fixed, seeded sample of rows)")
    args = ap.parse_args()
    assert args.steps >= 1, "--steps must be at least 1"

    rank = int(os.environ.get("RANK", "0"))
    local_rank = int(os.environ.get("LOCAL_RANK", "0"))
    world = int(os.environ.get("WORLD_SIZE", "1"))
    if "WORLD_SIZE" not in os.environ and args.gpus > 1:
        raise SystemExit(self_launch(args))
    args.gpus = world
    assert torch.cuda.is_available(), "bench.py needs an MI355X (no CPU fallback for the product path)"
    # one process per GPU; the gloo rehearsal mode puts every rank on device 0
    dev = torch.device("cuda", local_rank if args.backend == "nccl" else 0)
    torch.cuda.set_device(dev)
    dist = None
    if world > 1:
        import torch.distributed as dist_mod
        dist = dist_mod
        os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
        if args.backend == "nccl":
            dist.init_process_group("nccl", rank=rank, world_size=world, device_id=dev)
        else:
            dist.init_process_group(args.backend, rank=rank, world_size=world)

    import diff_gaussian_rasterization as dgr
    from oracle import gs_oracle as go           # scene generator + CPU baseline (checker side only)
    from parity_util import HIP_CENTRE_ERR_PX, to_settings

    N, W, H = args.n, args.width, args.height
    P = W * H
    scene, cam = go.view_tied_scene(N, W, H, seed=0)
    settings = to_settings(cam, dev)
    # The SAME step at every N (round 3 switched to the tracking step on N > 1 GPUs, so a scaling curve would have
    # compared different work): `rasterize` = gradients to all six inputs.  The tracking and mapping steps of the SLAM loop
    # are timed after the headline region and reported as extra keys (`loop_steps`).
    mode = args.mode or "rasterize"
    WANTED = {"rasterize": set(scene), "tracking": {"means3D", "means2D"},
              "mapping": {"means2D", "colors_precomp", "opacities", "scales"}}
    wanted = WANTED[mode]
    leaves = {k: v.to(dev).requires_grad_(k in wanted) for k, v in scene.items()}
    grad_bytes = sum(4 * scene[k][0].numel() for k in wanted)          # written per Gaussian by gather_splat_grads
    g = torch.Generator().manual_seed(1)
    grad_color = (torch.rand(3, H, W, generator=g) * 2 - 1).to(dev)

    from diff_gaussian_rasterization.partition import all_reduce_sum, band_for_rank, pose7_reduce
    gy16 = (H + 15) // 16
    tile_rows = band_for_rank(H, world, rank) if world > 1 else None
    emulated = None
    if args.band:
        assert world == 1, "--band is a single-process rehearsal"
        emulated = tuple(int(x) for x in args.band.split("/"))
        tile_rows = band_for_rank(H, emulated[1], emulated[0])
        args.slam_frames, args.audit_rows, args.no_cpu_baseline = 0, "", True
    # a band: the rank runs the per-Gaussian kernels over the LIST of Gaussians that can meet its rows (partition.OwnedSet: built
    # once here -- the bench renders one view -- and checked on the device before every render), not over the whole map
    own = None
    if tile_rows is not None and args.owned_sets:
        from diff_gaussian_rasterization.partition import OwnedSet
        own = OwnedSet.for_operator(leaves["means3D"], leaves["scales"], settings, tile_rows)
    rast = dgr.GaussianRasterizer(raster_settings=settings, tile_rows=tile_rows, owned=own)

    def step(leaves=leaves, mode=mode):
        for t in leaves.values():
            t.grad = None
        color, radii, depth = rast(**leaves)
        color.backward(grad_color)
        if mode == "tracking":
            # tracking: dL/dpose is a 7-float reduction of dL/dmeans3D; all-reduce it
            pose = pose7_reduce(leaves["means3D"], leaves["means3D"].grad)       # 7 floats, two launches
            if dist is not None:
                all_reduce_sum(pose)
        elif mode == "mapping" and dist is not None:
            flat = torch.cat([leaves[k].grad.reshape(-1) for k in ("colors_precomp", "opacities", "scales")])
            all_reduce_sum(flat)                                                 # 28 B per Gaussian, one collective
        elif dist is not None:
            # rasterize on N ranks: every rank holds its band's share of all six gradient arrays (the same kernels over the
            # same work as one GPU, split by tile rows); the collective is the one north_star names -- the pose gradient
            pose = pose7_reduce(leaves["means3D"], leaves["means3D"].grad)
            all_reduce_sum(pose)
        return color, radii, depth

    def fence():
        if dist is not None:
            dist.barrier()
        torch.cuda.synchronize()

    if rank == 0:
        print(f"[bench] scene ready: N={N} {W}x{H}, world={world}", file=sys.stderr, flush=True)
    # Clock ramp (untimed, disclosed in the line as `clock_ramp`).  The GPU idles while the host builds the scene, and its
    # clocks take tens of milliseconds of continuous work to come back: with the driver's `--steps 20 --warmup 5` the timed
    # region ran at 0.411 ms per step -- every kernel ~10 % slow -- the next region of the same process at 0.382 and all later
    # ones at 0.369 (tools/timed_region_study.py, gpurun_out/r5/timed_region_k20.log); with 250 ms of steps first, the FIRST
    # region runs at 0.372.  A handful of warm-up steps (2-4 ms of work) does not cover the ramp, so the steady state the
    # metric is about is reached first.  (This, not a kernel, is most of the 0.3985 -> 0.36x ms between BENCH_r04 and now.)
    # The region the driver's flags describe, taken the way rounds 1-4 took it -- --warmup steps, then --steps steps, right
    # after the scene set-up, before any ramp -- and reported as `first_region_ms_per_step`, so that the series BENCH_r01..r04
    # (which recorded THIS number as ms_per_step) stays comparable with the steady-state value of round 5 on.
    # A second measurement of its own: --full only.
    first_region_ms = None
    if args.full:
        for _ in range(args.warmup):
            step()
        fence()
        t0 = time.perf_counter()
        for _ in range(args.steps):
            step()
        fence()
        first_dt = time.perf_counter() - t0
        if dist is not None:
            tmax = torch.tensor([first_dt], dtype=torch.float64, device=dev)
            dist.all_reduce(tmax, op=dist.ReduceOp.MAX)
            first_dt = float(tmax.item())
        first_region_ms = first_dt / args.steps * 1e3
    else:
        # the first call of a process pays ~0.2 s of first-touch costs (code objects, allocator blocks): taken here, as the first
        # region takes it under --full, so that the ramp below is the same 250 ms of steady steps in both kinds of run
        step()
        fence()
    ramp_steps, ramp_t0 = 0, time.perf_counter()
    if dist is not None:                       # N ranks: a step holds a collective, so every rank takes the SAME number of steps
        for _ in range(int(args.ramp_ms * 2)):
            step()
            ramp_steps += 1
    else:
        while (time.perf_counter() - ramp_t0) * 1e3 < args.ramp_ms:
            step()
            ramp_steps += 1
        # ... and until the step time has settled: the first process on a fresh box keeps paying first-touch costs (code
        # objects, allocator blocks, mappings) well past 250 ms -- one run there took 124 ramp steps where the next took 252,
        # and another box's first run recorded 0.68 ms per step over --steps 20 where three later runs gave 0.357-0.360.
        # Chunks of 20 untimed steps until two consecutive chunks agree within 3 % (at most 2 s more); disclosed in `clock_ramp`.
        prev, settle_t0 = None, time.perf_counter()
        while time.perf_counter() - settle_t0 < 2.0:
            torch.cuda.synchronize(); c0 = time.perf_counter()
            for _ in range(20):
                step()
            torch.cuda.synchronize(); cur = time.perf_counter() - c0
            ramp_steps += 20
            if prev is not None and abs(cur - prev) <= 0.03 * prev:
                break
            prev = cur
    for _ in range(args.warmup):
        step()
    fence()
    t0 = time.perf_counter()
    for _ in range(args.steps - 1):
        step()
    last = step()                              # (what the caller receives from the last timed step: --dump-outputs)
    fence()
    dt = time.perf_counter() - t0
    if dist is not None:
        tmax = torch.tensor([dt], dtype=torch.float64, device=dev)
        dist.all_reduce(tmax, op=dist.ReduceOp.MAX)
        dt = float(tmax.item())
    ms_per_step = dt / args.steps * 1e3
    if rank == 0:
        print(f"[bench] timed region done: {ms_per_step:.3f} ms/step", file=sys.stderr, flush=True)
    value = N * P / (dt / args.steps) / 1e6
    if args.dump_outputs and rank == 0:
        per_gaussian = {"radii": last[1]}
        per_gaussian.update({"grad_" + k: leaves[k].grad for k in scene if k in wanted})
        dump_outputs(args.dump_outputs, {"color": last[0], "depth": last[2]}, per_gaussian, N)
        del per_gaussian
    del last
    info = dgr.last_forward_info()

    def headline(info):
        return {
            "metric": "Mgaussians*pixels/s rasterize fwd+bwd", "value": round(value, 1), "unit": "Mgaussians*pixels/s",
            "n_gpus": world, "steps": args.steps, "warmup": args.warmup, "ms_per_step": round(ms_per_step, 4),
            "higher_is_better": True, "scaling": "strong", "vs_baseline": None, "dtype": "f32", "data": "synthetic",
            "config": {"workload": f"view-tied synthetic scene (SURVEY 8d), N={N} isotropic Gaussians, {W}x{H}, "
                                   f"3-channel render, " + {"rasterize": "grads to all six inputs",
                                                             "tracking": "tracking step: grads to means3D + means2D (Gaussians "
                                                                         "detached), 7-float pose reduction",
                                                             "mapping": "mapping step: grads to colours, opacities, scales, "
                                                                        "means2D"}[mode],
                       "mode": mode,
                       "gaussians": N, "width": W, "height": H, "instances_8x8": info["instances"],
                       "tiles16_touched_R": info["tiles16_touched"], "max_tile_list": info["max_tile_list"],
                       "partition": "none" if tile_rows is None else f"tile-row bands x{emulated[1] if emulated else world} + " +
                                    ("all-reduce(28 B per Gaussian)" if mode == "mapping" else "all-reduce(7 floats)")},
            "clock_ramp": {"untimed_steps_before_warmup": ramp_steps, "ms": args.ramp_ms,
                           "why": "the GPU idles during scene set-up and its clocks need ~25 ms of work to recover: without this, 20 timed steps "
                                  "after 5 warm-ups run ~10 % slower than every later region of the same process (0.411 vs 0.369 ms); "
                                  "on one GPU the untimed steps then continue in chunks of 20 until two chunks agree within 3 % (<= 2 s): "
                                  "the first process on a fresh box keeps paying first-touch costs for longer"},
            "libvtgs_sha256": dgr.library_sha256(),
        }

    if not args.full:
        # the plain run ends here: set-up, clock ramp, warm-up, the timed steps, the dump, the line
        if rank == 0:
            print(json.dumps(dict(headline(info), full=False)))
        if dist is not None:
            dist.destroy_process_group()
        return

    def event_steps(fn, k):
        """HIP events on the op's stream around every one of k steps -> per-step ms (the record of an event is a
        queue marker of its own, so this is a SECOND pass: the contract's `ms_per_step` above is the host-clocked mean of
        exactly --steps steps without a marker in the queue)."""
        ev = [torch.cuda.Event(enable_timing=True) for _ in range(k + 1)]
        ev[0].record()
        for i in range(k):
            fn()
            ev[i + 1].record()
        fence()
        return sorted(ev[i].elapsed_time(ev[i + 1]) for i in range(k))

    def pct(v, q):
        return round(v[min(len(v) - 1, int(q * len(v)))], 4)

    ev_ms = event_steps(step, max(50, args.steps))
    step_events = {"n": len(ev_ms), "p10_ms": pct(ev_ms, 0.10), "p50_ms": pct(ev_ms, 0.50), "p90_ms": pct(ev_ms, 0.90),
                   "note": "hipEvents on the op's stream around every step of a second pass (median + p10 / p90, SURVEY 8d); "
                           "ms_per_step is the host-clocked mean of the first pass"}

    # ---- the SLAM loop's two steps through the same operator (extra keys; the headline above is `mode`) -------------------
    loop_steps = {}
    if not args.band:
        for m in ("tracking", "mapping"):
            if m == mode:
                loop_steps[m + "_step_ms"] = step_events["p50_ms"]
                continue
            lv = {k: v.detach().requires_grad_(k in WANTED[m]) for k, v in leaves.items()}
            for _ in range(5):
                step(lv, m)
            fence()
            # the MEDIAN of 30 event-timed steps (round 4 reported the mean of <= 20 host-clocked steps: ONE stall of a few
            # milliseconds -- a first allocation of the mode's smaller gradient block, a clock ramp -- doubled it in the
            # driver's record, 0.694 vs 0.365 ms; the spread is printed beside it now)
            lm = event_steps(lambda: step(lv, m), 30)
            med = pct(lm, 0.50)
            if dist is not None:
                tm = torch.tensor([med], dtype=torch.float64, device=dev)
                dist.all_reduce(tm, op=dist.ReduceOp.MAX)
                med = round(float(tm.item()), 4)
            loop_steps[m + "_step_ms"] = med
            loop_steps[m + "_step_p10_p90_ms"] = [pct(lm, 0.10), pct(lm, 0.90)]
            del lv
        loop_steps["note"] = ("median of 30 event-timed steps each; tracking: grads to means3D + means2D (Gaussians detached, src/vtgaussian_slam.py:428-449), 7-float "
                              "pose reduction + its all-reduce; mapping: grads to colours, opacities, scales, means2D + one flat "
                              "all-reduce of 28 B per Gaussian on N > 1")
        for t in leaves.values():
            t.grad = None
        step()                                     # (the statistics below describe a step of the headline mode)

    # ---- per-kernel phase (not part of the timed region above): HIP events around every kernel ----------
    info = dgr.last_forward_info()
    r16 = info["tiles16_touched"]
    dgr.profile_enable(True)
    prof_steps = max(5, min(20, args.steps))
    for _ in range(prof_steps):
        step()
    prof = dgr.profile_collect()
    dgr.profile_enable(False)
    kern = {k: {"avg_us": v[0] / v[1] * 1e3, "launches": v[1]} for k, v in prof.items()}
    # The bracket itself: two event records with nothing between them (libvtgs records one such pair per forward while the
    # profile is on).  Every kernel's bracket carries about that much on top of the kernel -- in round 5 the brackets summed to
    # MORE than the step (365 vs 359 us) -- so it is subtracted, and both figures are printed.
    bracket_us = kern.pop("_empty_bracket", {"avg_us": 0.0})["avg_us"]
    for v in kern.values():
        v["raw_us"] = v["avg_us"]
        v["avg_us"] = max(v["avg_us"] - bracket_us, 0.0)
    # rank 0's share: all N Gaussians are projected on every rank, pixels and tile instances only for its band
    if tile_rows is None:
        p_rank, r_rank = P, r16
    else:
        y0, y1 = tile_rows[0] * 16, min(tile_rows[1] * 16, H)
        p_rank, r_rank = W * (y1 - y0), r16             # (the op counts the tiles of what this band looked at)
    alg = kernel_algorithmic_bytes(N, p_rank, r_rank, grad_bytes)
    for fused in ("sort_tiles", "finalize_forward"):    # done inside the forward composite (no launch of their own)
        if kern and fused not in kern:
            alg["composite_forward"] += alg.pop(fused)
    roofline = None
    if kern:
        dom = max(kern, key=lambda k: kern[k]["avg_us"])
        if alg is not None:
            achieved = alg[dom] / (kern[dom]["avg_us"] * 1e-6) / 1e9
            call_bytes = (112 + grad_bytes) * N + 28 * p_rank + 52 * r_rank
            # HBM bytes from the committed PMC passes of the same command (profiles/pmc_traffic.json: separate --pmc FETCH_SIZE /
            # WRITE_SIZE runs, never collected inside this process): `traffic` = the DOMINANT KERNEL's bytes per launch,
            # `traffic_step_total` = all kernels of one step
            # The file is stamped with the sha256 of the libvtgs.so it was collected on (tools/summarize_profiles.py); a different
            # library in this process -- a kernel changed since the passes -- prints `traffic: null` and says why, instead of a
            # stale constant.
            traffic = traffic_total = traffic_src = None
            try:
                pmc = json.load(open(os.path.join(ROOT, "profiles", "pmc_traffic.json")))
                lib_sha = dgr.library_sha256()
                if not (tile_rows is None and mode == "rasterize" and (N, W, H) == (1_000_000, 1200, 680) and dom in pmc):
                    traffic_src = "null: profiles/pmc_traffic.json holds the headline shape in rasterize mode on one GPU only"
                elif pmc.get("_libvtgs_sha256") != lib_sha:
                    traffic_src = (f"null: profiles/pmc_traffic.json was collected on libvtgs.so sha256 {str(pmc.get('_libvtgs_sha256'))[:12]} "
                                   f"(round {pmc.get('_round', '?')}), this process loaded {lib_sha[:12]}: re-run tools/profile_round.sh")
                else:
                    traffic = pmc[dom]["traffic_bytes"]
                    traffic_total = sum(v["traffic_bytes"] for k, v in pmc.items() if isinstance(v, dict) and "traffic_bytes" in v)
                    traffic_src = (f"profiles/pmc_traffic.json (round {pmc.get('_round', '?')}, rocprofv3 --pmc passes of this command on the "
                                   f"SAME libvtgs.so, sha256 {lib_sha[:12]}; not measured in this run)")
            except (OSError, ValueError, KeyError) as e:
                traffic_src = f"null: {e!r}"
            roofline = {"bound": "hbm", "kernel": dom, "achieved": round(achieved, 2), "peak": HBM_PEAK_GBS,
                        "unit": "GB/s", "frac": round(achieved / HBM_PEAK_GBS, 5), "traffic": traffic,
                        "traffic_scope": f"{dom}, per launch", "traffic_step_total": traffic_total, "traffic_source": traffic_src,
                        "kernel_avg_us": round(kern[dom]["avg_us"], 2), "algorithmic_bytes": alg[dom],
                        "call_algorithmic_bytes": call_bytes,
                        "call_frac": round(call_bytes / (ms_per_step * 1e-3) / 1e9 / HBM_PEAK_GBS, 5),
                        "scope": "whole frame" if tile_rows is None else f"one band (tile rows {tile_rows[0]}..{tile_rows[1]})",
                        "note": "the composites are bound by fp32 issue (VALU + f32 MFMA share the lanes), see roofline.valu"}

    # secondary (VALU) bound, SURVEY.md 8(d): E = 256 x (16x16 tile instances) pixel x Gaussian evaluations of the published
    # algorithm, E_effective = 64 x (8x8 tile instances) evaluated here after the exact ellipse-vs-tile culling
    if roofline is not None:
        comp_us = sum(kern[k]["avg_us"] for k in kern if k.startswith("composite_"))
        e_all, e_eff = 256 * r_rank, 64 * info["instances"]          # (the instance count is already this rank's band)
        floor_us = e_eff * FLOP_PER_EVAL_FWD_BWD / (FP32_PEAK_TFLOPS * 1e12) * 1e6
        roofline["valu"] = {"E": e_all, "E_effective": e_eff, "flop_per_eval_fwd_bwd": FLOP_PER_EVAL_FWD_BWD,
                            "peak_tflops": FP32_PEAK_TFLOPS, "valu_floor_us": round(floor_us, 2),
                            "composite_us": round(comp_us, 2), "frac": round(floor_us / comp_us, 4) if comp_us else None}
        if "sort_tiles" not in kern:
            roofline["valu"]["note"] = "composite_forward includes the per-tile depth sort (no separate sort launch)"
        # pairs actually evaluated: the quadrant-queue forward counts its steps on the device (one step = 64 pixels x 16 splats)
        if dgr.get_option("VTGS_FWD_IMPL") == 3:
            dgr.set_option("VTGS_COUNT_STEPS", 1)
            with torch.no_grad():
                rast(**leaves)
            steps = dgr.debug_forward_steps(rast)
            dgr.set_option("VTGS_COUNT_STEPS", 0)
            tiles8 = ((W + 7) // 8) * (((tile_rows[1] - tile_rows[0]) * 2 if tile_rows else (H + 7) // 8))
            roofline["valu"]["forward_steps_per_tile"] = round(steps / max(tiles8, 1), 3)
            roofline["valu"]["pairs_forward"] = steps * 1024
        bwd_q = dgr.get_option("VTGS_BWD_IMPL") == 3
        roofline["valu"]["pairs_backward"] = roofline["valu"].get("pairs_forward") if bwd_q and "pairs_forward" in roofline["valu"] else e_eff

    cpu_baseline = None
    parity = None
    if rank == 0 and world == 1 and not args.no_cpu_baseline:
        rows = (0, min(args.cpu_rows, gy16))
        cpu_scene = {k: v.clone().requires_grad_(True) for k, v in scene.items()}
        # the box's CPU share, not the host's core count (oversubscribed OpenMP spins for minutes)
        torch.set_num_threads(max(1, min(len(os.sched_getaffinity(0)), 16)))
        print(f"[bench] cpu baseline on {torch.get_num_threads()} threads ...", file=sys.stderr, flush=True)
        tc0 = time.perf_counter()
        c_cpu, _, _ = go.rasterize(cam=cam, tile_rows=rows, **cpu_scene)
        c_cpu.backward(grad_color.cpu())
        tcpu = time.perf_counter() - tc0
        p_band = W * min(rows[1] * 16, H)
        cpu_baseline = {"value": round(N * p_band / tcpu / 1e6, 1), "unit": "Mgaussians*pixels/s",
                        "cores": torch.get_num_threads(), "kind": "port",
                        "sample": f"float32 PyTorch oracle fwd+bwd, same scene, tile rows {rows[0]}..{rows[1]} "
                                  f"({p_band} of {P} pixels; projection+binning of all N included), {tcpu:.1f} s"}
        del cpu_scene, c_cpu

    # ---- parity block: the frame of the timed path against the FLOAT64 oracle on a few tile rows, audited ----------------
    # (tests/test_gpu_configs.py does the same at every BASELINE shape).  Every pixel above 1e-4 must sit on a discrete
    # decision of the composite in the oracle's own per-pair values (parity_util.audit_outliers): `unexplained` must be 0.
    # Gradients: Gaussians that share a 16x16 tile with such a pixel carry its flipped pair and are reported apart.
    if rank == 0 and world == 1 and args.audit_rows:
        from parity_util import GRAD_KEYS, audit_outliers, grad_error, oracle_rows, rows_mask, tainted_gaussians
        rows = [int(r) for r in args.audit_rows.split(",") if r.strip() != "" and int(r) < gy16]
        print(f"[bench] parity: float64 oracle on tile rows {rows} ...", file=sys.stderr, flush=True)
        tp0 = time.perf_counter()
        mask = rows_mask(cam, rows)
        gsel = grad_color.cpu().clone()
        gsel[:, ~mask] = 0                                          # the audited loss lives on those rows
        torch.set_num_threads(max(1, min(len(os.sched_getaffinity(0)), 16)))
        ref_c, ref_r, ref_d, ref_g, keep, aux, idx = oracle_rows(scene, cam, rows, gsel)
        for t in leaves.values():
            t.grad = None
        color, radii, depth = rast(**leaves)
        color.backward(gsel.to(dev))
        got_c, got_d = color.detach().cpu().double(), depth.detach().cpu().double()
        hc = torch.where(mask[None, :, None], got_c, ref_c)          # outside the rows the oracle image is just the background
        hd = torch.where(mask[None, :, None], got_d, ref_d)
        sub_op = scene["opacities"][idx]
        a_c = audit_outliers(ref_c, hc, aux, sub_op, cam, 1e-4, centre_err_px=HIP_CENTRE_ERR_PX)
        a_d = audit_outliers(ref_d, hd, aux, sub_op, cam, 1e-4, centre_err_px=HIP_CENTRE_ERR_PX)
        taint = tainted_gaussians(aux, a_c["tiles"] | a_d["tiles"], idx.numel())
        rdiff = ref_r != radii.cpu()                                 # float32 ceil() on the other side moves a tile rectangle
        taint_full = torch.zeros(N, dtype=torch.bool)
        taint_full[idx[taint]] = True
        taint_full |= rdiff
        clean = keep & ~taint_full
        # ... and, of those, the Gaussians whose whole tile rectangle lies inside the audited rows: their gradient is complete
        # (one that only grazes the band is a sum of a few rim pairs, compared against the largest gradient of the frame)
        rect = aux["splats"].rect
        rowset = torch.zeros(gy16 + 1, dtype=torch.bool)
        rowset[rows] = True
        covered = torch.cumsum(rowset.long(), 0)
        inner_sub = (covered[(rect[:, 3] - 1).clamp(0, gy16)] - covered[rect[:, 1].clamp(0, gy16)] + rowset[rect[:, 1].clamp(0, gy16)].long()
                     == (rect[:, 3] - rect[:, 1])) & (rect[:, 3] > rect[:, 1])
        inner = torch.zeros(N, dtype=torch.bool)
        inner[idx[inner_sub]] = True
        clean_inner = clean & inner
        gmax, gp999, gl2 = 0.0, 0.0, 0.0
        gp999_all = 0.0
        for k in GRAD_KEYS:
            if k == "rotations":
                continue                                            # isotropic scene: exactly zero in exact arithmetic
            if ref_g[k].abs().max().item() == 0 or not bool(clean_inner.any()):
                continue
            r, h = ref_g[k][clean_inner].double(), leaves[k].grad.cpu()[clean_inner].double()
            mx, p999 = grad_error(r, h)
            gmax, gp999 = max(gmax, mx), max(gp999, p999)
            gl2 = max(gl2, ((r - h).norm() / (r.norm() + 1e-300)).item())
            gp999_all = max(gp999_all, grad_error(ref_g[k][clean].double(), leaves[k].grad.cpu()[clean].double())[1])
        # The same statistics for the published algorithm itself in float32 (the CPU oracle, which evaluates every exponent
        # directly from the pixel offset) against its float64 form: what single precision of the operator's own inputs --
        # pixel centres carry 2^-24 x 1200 px -- leaves of these figures for ANY float32 implementation.
        f32 = None
        try:
            c32, _, d32, g32, keep32, _, _ = oracle_rows(scene, cam, rows, gsel, dtype=torch.float32)
            sel32 = clean_inner & keep32
            f_p999 = f_max = 0.0
            for k in GRAD_KEYS:
                if k == "rotations" or ref_g[k].abs().max().item() == 0 or not bool(sel32.any()):
                    continue
                mx, p999 = grad_error(ref_g[k][sel32].double(), g32[k][sel32].double())
                f_p999, f_max = max(f_p999, p999), max(f_max, mx)
            img32 = max((((ref_c - c32.double()).abs().amax()) / ref_c.abs().amax()).item(),
                        (((ref_d - d32.double()).abs().amax()) / ref_d.abs().amax()).item())
            f32 = {"grad_p999": f_p999, "grad_max_rel": f_max, "img_max_rel": img32,
                   "note": "float32 CPU oracle vs float64 CPU oracle, same rows, same Gaussians, same statistics"}
        except Exception as e:                                   # (reporting only: never fail the bench line over it)
            f32 = {"error": repr(e)}
        n_px = int(mask.sum()) * W
        parity = {"oracle": "float64, tile rows " + ",".join(map(str, rows)) + f" ({n_px} pixels, {int(keep.sum())} Gaussians)",
                  "float32_oracle_vs_float64": f32,
                  "img_outliers_gt_1e-4": a_c["outliers"] + a_d["outliers"], "img_max_rel": max(a_c["max_rel"], a_d["max_rel"]),
                  "unexplained": len(a_c["unexplained"]) + len(a_d["unexplained"]),
                  "radii_differ": int(rdiff.sum()), "gaussians_beside_an_audited_pixel": int(taint_full.sum()),
                  "gaussians_inside_the_rows": int(clean_inner.sum()),
                  "grad_p999": gp999, "grad_max_rel": gmax, "grad_rel_l2": gl2, "grad_p999_incl_grazing": gp999_all,
                  "seconds": round(time.perf_counter() - tp0, 1),
                  "note": "colour + depth of the timed path vs the float64 oracle; every pixel above 1e-4 is audited against the "
                          "oracle's own per-pair values (alpha within float32 reach of 1/255, T within reach of the 1e-4 stop); "
                          "grad_* over the Gaussians that share no 16x16 tile with an audited pixel and whose tile rectangle lies "
                          "inside the audited rows (grad_p999_incl_grazing: also those that only graze the rows): p999 = 99.9th "
                          "percentile of |d| / (|ref| + 1e-3 max|ref|), max_rel = max|d| / max|ref|"}

    if rank == 0:
        out = headline(info)
        out.update({
            "full": True,
            "roofline": roofline, "cpu_baseline": cpu_baseline, "parity": parity, "slam": None, "loop_steps": loop_steps or None,
            "step_events": step_events,
            "kernels_us": {k: round(v["avg_us"], 2) for k, v in sorted(kern.items(), key=lambda kv: -kv[1]["avg_us"])},
            "kernels_us_note": {"event_bracket_us": round(bracket_us, 2),
                                "raw_us": {k: round(v["raw_us"], 2) for k, v in kern.items()},
                                "what": "kernels_us = HIP-event bracket around each launch minus the measured cost of an empty bracket "
                                        "(two event records back to back, one per forward of the profiled steps); raw_us = the brackets as read"},
            "first_region_ms_per_step": round(first_region_ms, 4),
            "first_region_note": "--warmup steps then --steps steps right after the scene set-up, BEFORE the clock ramp: the region "
                                 "BENCH_r01..r04 recorded as ms_per_step (cold clocks, first-touch costs); ms_per_step / value are the "
                                 "steady state after `clock_ramp`",
        })
        if tile_rows is not None and kern:
            # what every rank of the partition does over ALL Gaussians (projection, per-Gaussian gradient gather) beside what
            # it does for its band only (the two composites): SURVEY 8e "replicated work"
            # With a list: only the check (band_owner_mask) reads the whole map; projection and gather run over the list, whose
            # share beyond the band's own 1/W of the rows is what neighbouring ranks list too.
            W_ranks = emulated[1] if emulated else world
            ideal = (tile_rows[1] - tile_rows[0]) / float(gy16)
            listed = (len(own) / float(N)) if own is not None else 1.0
            whole = sum(v["avg_us"] for k, v in kern.items() if k == "band_owner_mask")
            per_list = sum(v["avg_us"] for k, v in kern.items() if not k.startswith("composite_") and k != "band_owner_mask")
            tot = sum(v["avg_us"] for v in kern.values())
            rep = whole + per_list * (1.0 - ideal / listed)
            out["band"] = {"rank": emulated[0] if emulated else rank, "world": W_ranks,
                           "tile_rows": list(tile_rows), "kernel_us_total": round(tot, 2),
                           "owned_set": None if own is None else {"listed": len(own), "listed_fraction": round(listed, 4),
                                                                   "band_fraction_of_rows": round(ideal, 4), "margin_px": own.margin_px,
                                                                   "scale_growth": own.growth, "escapes": own.escaped()},
                           "whole_map_kernel_us": round(whole, 2), "per_gaussian_kernel_us": round(per_list, 2),
                           "replicated_kernel_us": round(rep, 2), "replicated_frac": round(rep / tot, 4),
                           "replicated_note": "whole-map kernels + per-Gaussian kernels x (1 - band rows / listed fraction): the "
                                              "work other ranks do too (no list: listed fraction = 1; the index_select / "
                                              "index_add launches of the list route are torch's and not in kernels_us -- "
                                              "ms_per_step has them)",
                           "emulated_in_one_process": bool(emulated)}
    # ---- N > 1 ranks: what the first SCALE run has to show -- every rank's kernel times and replicated
    # share, the world size the process group reports, and the collective's own latency (a 7-float all-reduce, event-timed) ----
    if dist is not None:
        mine = {"rank": rank, "tile_rows": list(tile_rows) if tile_rows is not None else None,
                "kernels_us": {k: round(v["avg_us"], 2) for k, v in kern.items()}}
        if tile_rows is not None and kern:
            ideal = (tile_rows[1] - tile_rows[0]) / float(gy16)
            listed = (len(own) / float(N)) if own is not None else 1.0
            whole = sum(v["avg_us"] for k, v in kern.items() if k == "band_owner_mask")
            per_list = sum(v["avg_us"] for k, v in kern.items() if not k.startswith("composite_") and k != "band_owner_mask")
            tot = sum(v["avg_us"] for v in kern.values())
            mine["kernel_us_total"] = round(tot, 2)
            mine["replicated_frac"] = round((whole + per_list * (1.0 - ideal / listed)) / tot, 4) if tot else None
        buf = torch.zeros(7, device=dev)
        for _ in range(5):
            all_reduce_sum(buf)
        fence()
        ev = [torch.cuda.Event(enable_timing=True) for _ in range(21)]
        ev[0].record()
        for i in range(20):
            all_reduce_sum(buf)
            ev[i + 1].record()
        fence()
        coll = sorted(ev[i].elapsed_time(ev[i + 1]) * 1e3 for i in range(20))
        mine["allreduce_7_floats_us"] = {"p10": round(coll[2], 1), "p50": round(coll[10], 1), "p90": round(coll[18], 1)}
        every = [None] * world
        dist.all_gather_object(every, mine)
        if rank == 0:
            out["ranks"] = {"world_size": dist.get_world_size(), "backend": args.backend, "per_rank": every,
                            "collective_us": max(r["allreduce_7_floats_us"]["p50"] for r in every),
                            "step_kernel_us_max_over_ranks": max((r.get("kernel_us_total") or 0.0) for r in every),
                            "note": "per_rank[r].kernels_us: HIP-event averages of rank r's own launches (its band); collective_us: "
                                    "median latency of the step's 7-float all-reduce, the slowest rank's figure; the default route "
                                    "is the plain operator + the 7-float all-reduce (the owner-band exchange stays opt-in)"}
    # ---- slam block (BASELINE.json metric 2): a short run of bench_slam.py's loop through the get_loss mirror ---------------
    # The line above is complete without it.  On N > 1 GPUs the loop has collectives in it (never run on real multi-GPU
    # hardware by the builder: DESIGN.md 5), so a watchdog on every rank prints the line without the block and ends the process
    # if the loop has not finished in time, instead of leaving the driver without a record.
    if world > 1 and args.slam_frames > 3:
        args.slam_frames = 3        # N ranks: a short run (one warm-up + two ordinary frames + one base frame, ~1 min): the N = 8
                                    # case has to finish well inside the driver's 600 s, and its loop was never run on RCCL hardware
    if args.slam_frames > 0 and (N, W, H) == (1_000_000, 1200, 680):     # (every rank takes part in the N-rank loop)
        import bench_slam
        import threading
        finished = threading.Event()
        limit = 300.0

        def bail():
            if finished.is_set():
                return
            if rank == 0:
                out["slam"] = {"error": f"the {world}-rank tracking+mapping loop did not finish within {limit:.0f} s"}
                print(json.dumps(out), flush=True)
            os._exit(0 if rank == 0 else 1)
        timer = None
        if world > 1:
            timer = threading.Timer(limit, bail)
            timer.daemon = True
            timer.start()
        if rank == 0:
            print(f"[bench] slam block: {args.slam_frames} frames of the tracking+mapping loop ...", file=sys.stderr, flush=True)
        del leaves, rast
        torch.cuda.empty_cache()
        # 1 GPU: through the get_loss mirror (the reference's own call); N GPUs: the same fused operators with the band forms
        # of the losses and the collectives of SURVEY 8e (bench_slam.py --fused under torch.distributed)
        # The reference's mapping schedule (src/vtgaussian_slam.py:2525-2610): the LAST of the block's frames is a base frame
        # (current view, both get_loss calls -- the second one over the global set of 2 fixed submaps (+) the current one, 3 N
        # Gaussians -- every iteration), the others are ordinary frames (one keyframe drawn per iteration from the submap's
        # frames so far; the second call when the draw is the submap's base frame).  `value` is the mix for one base frame in
        # forty (configs/replica/room0.py:35).  On N > 1 GPUs the fused N-rank loop has no global set yet: keyframe draw only.
        E = args.slam_frames + 1                                    # one untimed warm-up frame, then `slam_frames`; the last is the base frame
        # 41 frames (the default) = one whole submap cycle of configs/replica/room0.py:35 (40 ordinary frames whose windows grow as
        # in the reference, then the base frame); a shorter run draws the ordinary frames' keyframes as from a 12-frame window
        whole_cycle = args.slam_frames >= 41
        route = (["--get-loss", "--global-submaps", "2"] if world == 1 else ["--fused", "--backend", args.backend]) + \
                ["--base-frame-every", str(E), "--warmup-frames", "1"] + ([] if whole_cycle else ["--emulate-window", "12"])
        try:
            # one GPU: WITH the densification step of every ordinary frame (the reference's per-frame work),
            # then the same cycle without it for comparison
            rec = bench_slam.run(bench_slam.parse_args(["--frames", str(args.slam_frames)] + route + (["--densify"] if world == 1 else [])))
            rec_plain = bench_slam.run(bench_slam.parse_args(["--frames", str(args.slam_frames)] + route)) if world == 1 else None
            reg = rec.get("regimes") or {}
            mix = reg.get("frames_per_s_mix_39_to_1")
            slam = {"metric": "SLAM frames/s, tracking+mapping loop", "value": mix if mix is not None else rec["value"],
                    "unit": "frames/s", "value_is": ("39 ordinary frames : 1 base frame (baseframe_every = 40)" +
                                                    (", measured over one whole submap cycle" if whole_cycle else
                                                     ", extrapolated from a short run with emulated 12-frame windows")) if mix is not None
                                                    else "the frames of this run as they came",
                    "frames": args.slam_frames, "frames_per_s_this_run": rec["value"],
                    "tracking_ms_per_iter": rec["tracking_ms_per_iter"],
                    "mapping_ms_per_iter": rec["mapping_ms_per_iter"], "regimes": reg, "workload": rec["config"]["workload"],
                    "gaussians_in_global_set": rec["config"]["gaussians_in_global_set"],
                    "pose_error_after_tracking_cm_deg": rec["pose_error_after_tracking_cm_deg"], "n_gpus": world,
                    "densification": rec.get("densification"),
                    "without_densification": None if rec_plain is None else {
                        "value": (rec_plain.get("regimes") or {}).get("frames_per_s_mix_39_to_1") or rec_plain["value"],
                        "tracking_ms_per_iter": rec_plain["tracking_ms_per_iter"], "mapping_ms_per_iter": rec_plain["mapping_ms_per_iter"]},
                    "partition": rec["config"]["partition"],
                    "note": "synthetic Replica-room0-like sequence " + ("through the get_loss mirror" if world == 1 else
                            f"on {world} ranks: the fused operators with the band forms of the losses (no second call over a global set)") +
                            "; tracking on the current view, mapping "
                            "on the reference's schedule: ordinary frames draw one keyframe per iteration (ONE get_loss call, plus "
                            "the second one over the 3 N-Gaussian global set when the draw is the base frame), base frames make "
                            "BOTH calls every iteration.  " + ("The windows grow over the 40 ordinary frames as in the reference (the base frame, "
                            "i.e. the second call, is drawn in 0.08 of the iterations); later frames look at the view-tied map from up to 6 degrees / "
                            "16 cm away, which lengthens the tile lists -- the first frames of a cycle run ~20 % faster than its mean.  "
                            if whole_cycle else "The ordinary frames draw as from a 12-frame window (second call in 1 of 12 iterations; the mean "
                            "over a 40-frame submap is 0.084).  ") +
                            ("Every ordinary frame runs the reference's densification step (forward-only render, depth_error.median(), "
                               "new Gaussians appended: N grows over the cycle).  " if world == 1 else "No densification on N > 1 ranks.  ") +
                            "get_loss renders under its own contract (it differentiates the [z,1,z^2] image through z alone: the single render's "
                            "forward kernel with z in the depth column, a four-channel backward -- same loss and gradients, "
                            "tests/test_gpu_fused_frame.py).  "
                            "No dataset I/O and no keyframe-overlap selection (host / small-tensor work outside the rasterizer path)."}
        except Exception as e:                                   # (the headline line must not be lost over the second metric)
            if world == 1:
                raise
            slam = {"error": repr(e)}
        finished.set()
        if timer is not None:
            timer.cancel()
        if rank == 0:
            out["slam"] = slam
    if rank == 0:
        print(json.dumps(out))
    if dist is not None:
        dist.destroy_process_group()


if __name__ == "__main__":
    main()
