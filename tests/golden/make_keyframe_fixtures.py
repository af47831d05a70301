"""Generates tests/golden/keyframes.npz by running the reference's OWN keyframe selection (utils/keyframe_selection.py:
get_pointcloud :10-37, keyframe_selection_overlap :40-116, keyframe_selection_overlap_visbased :121-229,
keyframe_selection_overlap_visbased_earliest_dynamic_new_topkbase :581-724, find_earliest_keyframe :1581-1613) in the build
container.

    python tests/golden/make_keyframe_fixtures.py          # needs /root/reference

The CPU shim of make_get_loss_fixtures.py is reused (the reference's hard-coded 'cuda' mapped to the CPU).  One more shim is
this script's own: while a sampled function of the reference runs, `torch.randint` returns a FIXED draw (seeded, with one
planted pair and one planted triple of equal indices), so that the draw can be stored and every link of
find_earliest_keyframe sees the same sample.  Depth maps are multiples of 1/1024 (a depth sensor's grid; it also keeps the
archive small).  Stored: arrays only -- the inputs and what the reference returned.  No reference source text.

The generator ASSERTS that on every scene the reference's get_pointcloud dropped nothing but repeated sample indices and
points that round to the world origin: its unique() call would also drop two different pixels whose |rounded| world
coordinates coincide, which the native rule (include/vtgs.h) does not reproduce.
"""
import contextlib
import importlib.util
import io
import os
import sys

import numpy as np
import torch

OUT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, OUT)
import make_get_loss_fixtures as base  # noqa: E402  (CPU shim; also puts the repository on sys.path)

_real_randint = torch.randint
_draws = []


def fixed_randint(high, size, **kw):
    """A seeded draw with replacement plus a planted triple (entries 5, 6, 7) and pair (20, 21) when it is long enough."""
    idx = _real_randint(high, size, generator=torch.Generator().manual_seed(4242))
    if idx.numel() >= 32:
        idx[6] = idx[7] = idx[5]
        idx[21] = idx[20]
    _draws.append(idx.clone())
    return idx


def rotation(q):
    r, x, y, z = (torch.tensor(q, dtype=torch.float64) / torch.tensor(q, dtype=torch.float64).norm()).tolist()
    return torch.tensor([[1 - 2 * (y * y + z * z), 2 * (x * y - r * z), 2 * (x * z + r * y)],
                         [2 * (x * y + r * z), 1 - 2 * (x * x + z * z), 2 * (y * z - r * x)],
                         [2 * (x * z - r * y), 2 * (y * z + r * x), 1 - 2 * (x * x + y * y)]], dtype=torch.float64)


def pose(q, t):
    m = torch.eye(4, dtype=torch.float64)
    m[:3, :3] = rotation(q)
    m[:3, 3] = torch.tensor(t, dtype=torch.float64)
    return m.float()


def grid1024(d):
    return torch.round(d * 1024) / 1024


def surface(H, W, g, lo=2.0, invalid=0.05):
    ys, xs = torch.meshgrid(torch.arange(H, dtype=torch.float32), torch.arange(W, dtype=torch.float32), indexing="ij")
    d = lo + 0.5 * torch.sin(xs / W * 3.1) * torch.cos(ys / H * 2.3) + 0.3 * (ys / H) + 0.01 * torch.randn(H, W, generator=g)
    d = grid1024(d)
    d[torch.rand(H, W, generator=g) < invalid] = 0.0
    return d[None].contiguous()


def keyframe_depth(gt_depth, g, noise):
    d = gt_depth * (1 + noise * torch.randn(gt_depth.shape, generator=g))
    return grid1024(d.clamp(min=0)).contiguous()


def kf_list(poses, depths):
    return [{"id": i, "est_w2c": p.clone(), "depth": d.clone()} for i, (p, d) in enumerate(zip(poses, depths))]


def expected_kept(ref, gt_depth, intr, w2c, samples):
    """(kept by the reference, samples in repeated groups, origin points among the others) -- restated only to ASSERT that
    the reference dropped nothing else."""
    kept = ref.get_pointcloud(gt_depth, intr, w2c, samples).shape[0]
    _, inv, cnt = torch.unique(samples, dim=0, return_inverse=True, return_counts=True)
    rep = cnt[inv] > 1
    xx = (samples[:, 1] - intr[0][2]) / intr[0][0]
    yy = (samples[:, 0] - intr[1][2]) / intr[1][1]
    z = gt_depth[0, samples[:, 0], samples[:, 1]]
    pc = torch.stack((xx * z, yy * z, z), dim=-1)
    p4 = torch.cat([pc, torch.ones_like(pc[:, :1])], dim=1)
    pts = (torch.inverse(w2c) @ p4.T).T[:, :3]
    origin = (torch.abs(torch.round(pts, decimals=4)) == 0).all(dim=1) & ~rep
    n_rep, n_org = int(rep.sum()), int(origin.sum())
    assert kept == samples.shape[0] - n_rep - n_org, \
        f"the reference dropped {samples.shape[0] - kept} points, repeats {n_rep} + origin {n_org}: coincident-rounding pairs"
    return kept, n_rep, n_org


def percent_arrays(lst):
    return (np.array([d["id"] for d in lst], dtype=np.int64),
            np.array([d["percent_inside"].item() for d in lst], dtype=np.float32))


def quiet(fn, *a, **kw):
    buf = io.StringIO()
    with contextlib.redirect_stdout(buf):
        out = fn(*a, **kw)
    return out, buf.getvalue()


def main():
    if not os.path.isdir(base.REF):
        raise SystemExit("reference not mounted; fixtures can only be generated in the build container")
    sys.dont_write_bytecode = True
    base.install_cpu_shim()
    sys.path.insert(0, base.REF)
    spec = importlib.util.spec_from_file_location("ref_keyframe_selection", os.path.join(base.REF, "utils", "keyframe_selection.py"))
    ref = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(ref)
    torch.randint = fixed_randint
    g = torch.Generator().manual_seed(20251022)
    store = {}

    def valid_rc(gt_depth):
        return torch.stack(torch.where(gt_depth[0] > 0), dim=1)

    # ---- scene A: 72 x 56, six keyframes under spread poses, 5 % invalid depth, edge 4 -----------------------------------------
    W, H, F, EDGE = 72, 56, 60.0, 4
    k = torch.tensor([[F, 0, W / 2 - 0.5], [0, F, H / 2 - 0.5], [0, 0, 1.0]])
    gt_depth = surface(H, W, g)
    w2c = pose([1.0, 0.004, -0.006, 0.003], [0.01, 0.0, -0.01])
    poses = [pose([1.0, 0.01, -0.02, 0.005], [0.05, -0.02, 0.03]), pose([1.0, -0.03, 0.05, 0.01], [-0.25, 0.03, 0.02]),
             pose([1.0, 0.02, 0.12, -0.02], [0.6, 0.05, -0.04]), pose([1.0, 0.08, -0.01, 0.03], [0.02, 0.45, 0.1]),
             pose([1.0, -0.01, -0.22, 0.0], [-1.1, 0.0, 0.2]), pose([1.0, 0.0, 0.03, 0.2], [0.1, -0.1, -0.3])]
    depths = [keyframe_depth(gt_depth, g, 0.01 + 0.004 * i) for i in range(6)]
    store.update(a_gt_depth=gt_depth.numpy(), a_k=k.numpy(), a_w2c=w2c.numpy(), a_edge=np.int64(EDGE),
                 a_kf_w2c=torch.stack(poses).numpy(), a_kf_depth=torch.cat(depths).numpy())
    dense_rc = valid_rc(gt_depth)
    n_dense, rep, org = expected_kept(ref, gt_depth, k, w2c, dense_rc)
    assert rep == 0 and org == 0
    store["a_dense_n"] = np.int64(n_dense)
    for name, thr in (("t001", 0.01), ("t005", 0.05)):
        lst, _ = quiet(ref.keyframe_selection_overlap_visbased, gt_depth, w2c, k, kf_list(poses, depths), 3, edge_value=EDGE,
                       save_percent=True, kf_depth_thresh=thr)
        ids, pct = percent_arrays(lst)
        et = float(np.sort(pct)[-3]) - 1e-4                       # three keyframes pass: the earliest pick is the LAST of them
        (sel, ear), _ = quiet(ref.keyframe_selection_overlap_visbased, gt_depth, w2c, k, kf_list(poses, depths), 3,
                              edge_value=EDGE, kf_depth_thresh=thr, earliest_thres=et)
        assert pct.max() > 0.2 and len(set(np.round(pct * n_dense).astype(int))) >= 4, pct
        store.update({f"a_{name}_thresh": np.float64(thr), f"a_{name}_ids": ids, f"a_{name}_percent": pct,
                      f"a_{name}_earliest_thres": np.float64(et), f"a_{name}_selected": np.array(sel, dtype=np.int64),
                      f"a_{name}_earliest": np.array(ear, dtype=np.int64)})
        print("A dense", name, "n", n_dense, dict(zip(ids.tolist(), pct.tolist())), "selected", sel, "earliest", ear)
    # sampled, pixels = 100: a planted triple and pair (+ whatever the draw repeats by itself)
    _draws.clear()
    lst, _ = quiet(ref.keyframe_selection_overlap, gt_depth, w2c, k, kf_list(poses, depths), 3, pixels=100, edge_value=EDGE,
                   save_percent=True)
    sel, _ = quiet(ref.keyframe_selection_overlap, gt_depth, w2c, k, kf_list(poses, depths), 3, pixels=100, edge_value=EDGE)
    assert len(_draws) == 2 and torch.equal(_draws[0], _draws[1])
    samples = dense_rc[_draws[0]]
    n_s, rep, org = expected_kept(ref, gt_depth, k, w2c, samples)
    assert rep >= 5 and org == 0 and n_s == 100 - rep
    ids, pct = percent_arrays(lst)
    store.update(a_sampled_rc=samples.numpy().astype(np.int32), a_sampled_n=np.int64(n_s), a_sampled_ids=ids, a_sampled_percent=pct,
                 a_sampled_selected=np.array(sel, dtype=np.int64))
    print("A sampled: kept", n_s, "of 100 (repeats", rep, ")", dict(zip(ids.tolist(), pct.tolist())), "selected", sel)

    # find_earliest_keyframe: a chain of three links 12 -> 4 -> 0 -> 8, i.e. keyframes 1, 0, 2 (baseframe_every 4), the same
    # draw for every link
    corr = [[8, 0, 0], [0, 3, 4], [4, 7, 12], [12, 15, 16]]
    by_id = dict(zip(ids.tolist(), pct.tolist()))
    assert by_id[1] > by_id[2] and by_id[0] > by_id[2], by_id
    thr_chain = (min(by_id[1], by_id[0]) + by_id[2]) / 2          # links 4 and 0 pass, link 8 stops the walk
    _draws.clear()
    res, _ = quiet(ref.find_earliest_keyframe, [list(c) for c in corr], gt_depth, w2c, k, kf_list(poses, depths), 3, EDGE, 4,
                   thr_chain, pixels=100)
    assert len(_draws) == 3 and res == [0, None, 16], (len(_draws), res)
    res_all, _ = quiet(ref.find_earliest_keyframe, [list(c) for c in corr], gt_depth, w2c, k, kf_list(poses, depths), 3, EDGE, 4,
                       0.0, pixels=100)
    assert res_all[0] == 8
    store.update(a_corr_list=np.array(corr, dtype=np.int64), a_chain_threshold=np.float64(thr_chain),
                 a_chain_result=np.array([res[0], res[2]], dtype=np.int64), a_chain_result_thr0=np.array([res_all[0], res_all[2]]))
    print("A chain: threshold", thr_chain, "->", res, "; threshold 0 ->", res_all)

    # ---- scene B: 45 x 37, eight keyframes, the topkbase form with {baseframe_every: 4, overlap_every: 2} -----------------------
    W, H, F, EDGE = 45, 37, 40.0, 4
    kb = torch.tensor([[F, 0, W / 2 - 0.3], [0, F + 1.0, H / 2 + 0.2], [0, 0, 1.0]])
    gt_b = surface(H, W, g)
    w2c_b = pose([1.0, -0.003, 0.005, 0.002], [0.0, 0.01, 0.01])
    poses_b = [pose([1.0, 0.0, 0.02 * i - 0.07, 0.004 * i], [0.13 * i - 0.45, 0.02 * (i % 3), 0.01 * i]) for i in range(8)]
    depths_b = [keyframe_depth(gt_b, g, 0.012 + 0.003 * i) for i in range(8)]
    poses_b[5], depths_b[5] = poses_b[2].clone(), depths_b[2].clone()          # a tie: the stable order decides
    n_b, rep, org = expected_kept(ref, gt_b, kb, w2c_b, valid_rc(gt_b))
    assert rep == 0 and org == 0
    lst, _ = quiet(ref.keyframe_selection_overlap_visbased, gt_b, w2c_b, kb, kf_list(poses_b, depths_b), 3, edge_value=EDGE,
                   save_percent=True, kf_depth_thresh=0.03)
    ids, pct = percent_arrays(lst)
    by_id = dict(zip(ids.tolist(), pct.tolist()))
    assert by_id[2] == by_id[5] and ids.tolist().index(2) < ids.tolist().index(5)
    config = {"baseframe_every": 4, "overlap_every": 2}
    base_best = sorted((max(by_id[2 * b], by_id[2 * b + 1]) for b in range(4)), reverse=True)
    assert base_best[2] > 0.02
    et_b = float(base_best[2]) / 0.64 * 0.995                    # three base frames pass only after two lowering rounds
    store.update(b_gt_depth=gt_b.numpy(), b_k=kb.numpy(), b_w2c=w2c_b.numpy(), b_edge=np.int64(EDGE), b_thresh=np.float64(0.03),
                 b_kf_w2c=torch.stack(poses_b).numpy(), b_kf_depth=torch.cat(depths_b).numpy(), b_n=np.int64(n_b), b_ids=ids,
                 b_percent=pct, b_baseframe_every=np.int64(4), b_overlap_every=np.int64(2), b_earliest_thres=np.float64(et_b),
                 b_lower=np.float64(0.8))
    for name, topk in (("top3", 3), ("top2", 2), ("none", None)):
        out, text = quiet(ref.keyframe_selection_overlap_visbased_earliest_dynamic_new_topkbase, gt_b, w2c_b, kb,
                          kf_list(poses_b, depths_b), 3, config, edge_value=EDGE, kf_depth_thresh=0.03, earliest_thres=et_b,
                          lower_earliest_thres_percent=0.8, topk_base=topk)
        rounds = text.count("quantized_baseframe_id_ls:") - (0 if topk is None else 1)
        assert rounds >= 3, rounds
        store[f"b_{name}"] = np.array(out, dtype=np.int64)
        print("B topkbase", name, "rounds", rounds, "->", out)
    # every keyframe turned away (its camera looks along -z of the current one): all counts 0, the fallback to the last keyframe
    away = [pose([0.0, 0.0, 1.0, 0.0], [0.1 * i, 0.0, 0.0]) for i in range(8)]
    out, _ = quiet(ref.keyframe_selection_overlap_visbased_earliest_dynamic_new_topkbase, gt_b, w2c_b, kb, kf_list(away, depths_b),
                   3, config, edge_value=EDGE, kf_depth_thresh=0.03, earliest_thres=0.5, topk_base=3)
    lst, _ = quiet(ref.keyframe_selection_overlap_visbased, gt_b, w2c_b, kb, kf_list(away, depths_b), 3, edge_value=EDGE,
                   save_percent=True, kf_depth_thresh=0.03)
    (sel0, ear0), _ = quiet(ref.keyframe_selection_overlap_visbased, gt_b, w2c_b, kb, kf_list(away, depths_b), 3, edge_value=EDGE,
                            kf_depth_thresh=0.03)
    ids, pct = percent_arrays(lst)
    assert out == [3] and float(np.abs(pct).max()) == 0.0 and ids.tolist() == list(range(8)) and sel0 == [] and ear0 == []
    store.update(b_away_kf_w2c=torch.stack(away).numpy(), b_away_topkbase=np.array(out, dtype=np.int64))
    print("B turned away -> topkbase", out)
    # n == 0: no valid depth at all; every percent is NaN
    zero = torch.zeros_like(gt_b)
    out0, _ = quiet(ref.keyframe_selection_overlap_visbased_earliest_dynamic_new_topkbase, zero, w2c_b, kb,
                    kf_list(poses_b, depths_b), 3, config, edge_value=EDGE, kf_depth_thresh=0.03, earliest_thres=0.5, topk_base=3)
    (selz, earz), _ = quiet(ref.keyframe_selection_overlap_visbased, zero, w2c_b, kb, kf_list(poses_b, depths_b), 3,
                            edge_value=EDGE, kf_depth_thresh=0.03)
    lst, _ = quiet(ref.keyframe_selection_overlap_visbased, zero, w2c_b, kb, kf_list(poses_b, depths_b), 3, edge_value=EDGE,
                   save_percent=True, kf_depth_thresh=0.03)
    ids, pct = percent_arrays(lst)
    assert np.isnan(pct).all() and ids.tolist() == list(range(8)) and selz == [] and earz == []
    store.update(b_n0_topkbase=np.array(out0, dtype=np.int64))
    print("B n = 0 -> topkbase", out0, "visbased", selz, earz)

    # ---- scene D: the camera looks at the world origin: exactly one point falls to the origin rule -----------------------------
    W, H, F, EDGE = 45, 37, 40.0, 3
    kd = torch.tensor([[F, 0, 22.0], [0, F, 18.0], [0, 0, 1.0]])
    # (a ramp of pairwise DISTINCT depths: with integer cx, cy and an axis-aligned camera, pixels mirrored about the centre reach
    #  |equal| world coordinates whenever their depths agree -- the coincident-rounding pairs the assertion below refuses)
    gt_d = (1.2 + torch.arange(H * W, dtype=torch.float32) / 1024).reshape(1, H, W)
    gt_d[0][torch.rand(H, W, generator=g) < 0.03] = 0.0
    gt_d[0, 18, 22] = 2.0
    w2c_d = torch.eye(4)
    w2c_d[2, 3] = 2.0
    poses_d = [pose([1.0, 0.01, 0.02, 0.0], [0.05, 0.0, 2.02]), pose([1.0, -0.02, -0.06, 0.01], [-0.3, 0.05, 1.9]),
               pose([1.0, 0.05, 0.0, -0.03], [0.0, 0.3, 2.2])]
    depths_d = [keyframe_depth(gt_d, g, 0.02) for _ in range(3)]
    n_d, rep, org = expected_kept(ref, gt_d, kd, w2c_d, valid_rc(gt_d))
    assert rep == 0 and org == 1 and n_d == int((gt_d > 0).sum()) - 1
    lst, _ = quiet(ref.keyframe_selection_overlap_visbased, gt_d, w2c_d, kd, kf_list(poses_d, depths_d), 3, edge_value=EDGE,
                   save_percent=True, kf_depth_thresh=0.05)
    ids, pct = percent_arrays(lst)
    assert pct.max() > 0.2
    store.update(d_gt_depth=gt_d.numpy(), d_k=kd.numpy(), d_w2c=w2c_d.numpy(), d_edge=np.int64(EDGE), d_thresh=np.float64(0.05),
                 d_kf_w2c=torch.stack(poses_d).numpy(), d_kf_depth=torch.cat(depths_d).numpy(), d_n=np.int64(n_d), d_ids=ids,
                 d_percent=pct)
    print("D origin: n", n_d, "of", int((gt_d > 0).sum()), dict(zip(ids.tolist(), pct.tolist())))
    # sampled on the same scene: the draw with the origin pixel planted once (entry 40)
    _draws.clear()
    rc_d = valid_rc(gt_d)
    origin_row = int(torch.where((rc_d[:, 0] == 18) & (rc_d[:, 1] == 22))[0])

    def origin_randint(high, size, **kw):
        idx = fixed_randint(high, size)
        idx[40] = origin_row
        _draws[-1] = idx.clone()
        return idx
    torch.randint = origin_randint
    lst, _ = quiet(ref.keyframe_selection_overlap, gt_d, w2c_d, kd, kf_list(poses_d, depths_d), 3, pixels=100, edge_value=EDGE,
                   save_percent=True)
    torch.randint = fixed_randint
    samples = rc_d[_draws[0]]
    n_ds, rep, org = expected_kept(ref, gt_d, kd, w2c_d, samples)
    assert org == 1 and rep >= 5
    ids, pct = percent_arrays(lst)
    store.update(d_sampled_rc=samples.numpy().astype(np.int32), d_sampled_n=np.int64(n_ds), d_sampled_ids=ids, d_sampled_percent=pct)
    print("D sampled: kept", n_ds, "of 100 (repeats", rep, "origin", org, ")")

    torch.randint = _real_randint
    path = os.path.join(OUT, "keyframes.npz")
    np.savez_compressed(path, **store)
    print("wrote keyframes.npz", os.path.getsize(path), "bytes,", len(store), "arrays")
    assert os.path.getsize(path) < 200 * 1000


if __name__ == "__main__":
    main()
