"""vtgs_keyframe_overlap (csrc/vtgs_keyframes.hip) and its Python mirror (diff_gaussian_rasterization/keyframes.py).

Decision parity: counts cannot be held to a float tolerance, so the kernel's per-pair masks are compared with the float64
restatement of tests/keyframe_util.py.  A pair may differ only where the smallest margin of its comparisons (edge tests
relative to the image extent, z' > 0, visibility relative to z') lies below tau; everywhere else the masks are identical, and
the counts equal the mask sums exactly.  tau is MEASURED: 4 x the largest margin at which the fixture's own float32 masks
(proven equal to the reference's counts in tests/test_keyframe_fixtures.py) disagree with the float64 masks, floor 4 float32
ulps (DESIGN.md 12 records both).  Pairs inside the band may not exceed 0.5 % of a case's pairs.
Hand-placed 45 x 37 and 33 x 17 frames (no multiple of a wavefront or workgroup) cover K in {1, 3, 65}, the sample counts
around a wavefront, slot permutations, the forms without visibility test and the degenerate frames."""
import numpy as np
import pytest
import torch

import keyframe_util as ku

pytestmark = pytest.mark.gpu
POISON = 0x5A
INVALID = 1


@pytest.fixture(scope="module")
def kf():
    from diff_gaussian_rasterization import keyframes
    return keyframes


def run_abi(dev, c, rc=None, kf_w2c=None, kf_depth=None, slots=None, edge=None, thresh="case", want_mask=True):
    """The C entry point on poisoned scratch / record / pair mask.  Returns (record [k + 3] int64, pair mask [k, S] uint8 or
    None) with S = H * W (dense) or the number of samples."""
    from diff_gaussian_rasterization import _stream_ptr
    from diff_gaussian_rasterization import keyframes as kfm
    lib = kfm._lib
    t32 = lambda a: torch.as_tensor(np.ascontiguousarray(a), dtype=torch.float32).contiguous().to(dev)
    gd, kmat, w2c = t32(c["gt_depth"]), t32(c["k"]), t32(c["w2c"])
    H, W = gd.shape[-2:]
    poses = t32(c["kf_w2c"] if kf_w2c is None else kf_w2c).reshape(-1, 16)
    depths = t32(c["kf_depth"] if kf_depth is None else kf_depth)
    edge = c["edge"] if edge is None else edge
    thresh = c["thresh"] if thresh == "case" else thresh
    sl = None if slots is None else torch.tensor(list(slots), dtype=torch.int32).to(dev)
    k = poses.shape[0] if sl is None else sl.numel()
    rct = None if rc is None else torch.as_tensor(np.ascontiguousarray(rc)).to(torch.int32).contiguous().to(dev)
    samples = 0 if rct is None else rct.shape[0]
    S = samples or H * W
    need = lib.vtgs_keyframe_overlap_scratch_bytes(W, H, samples, k)
    assert need > 0
    scratch = torch.full((need + 64,), POISON, dtype=torch.uint8, device=dev)
    record = torch.full((k + 3 + 4,), POISON * 0x01010101, dtype=torch.int32, device=dev)
    pm = torch.full((k * S + 16,), POISON, dtype=torch.uint8, device=dev) if want_mask else None
    p = lambda x: None if x is None else x.data_ptr()
    rcode = lib.vtgs_keyframe_overlap(W, H, gd.data_ptr(), kmat.data_ptr(), w2c.data_ptr(), p(rct), samples, poses.data_ptr(),
                                      depths.data_ptr() if thresh is not None else None, p(sl), k, float(edge),
                                      float(thresh or 0.0), p(pm), scratch.data_ptr(), need, record.data_ptr(), _stream_ptr(dev))
    assert rcode == 0, rcode
    torch.cuda.synchronize(dev)
    assert (scratch[need:] == POISON).all() and (record[k + 3:] == POISON * 0x01010101).all()     # nothing behind the ends
    if pm is not None:
        assert (pm[k * S:] == POISON).all()
        pm = pm[:k * S].reshape(k, S).cpu().numpy()
    return record[:k + 3].cpu().numpy().astype(np.int64), pm


def check(dev, c, rc=None, kf_w2c=None, kf_depth=None, slots=None, edge=None, thresh="case"):
    """Decision parity of one call; returns (record, in-band pairs per keyframe [k])."""
    tau = ku.measure_tau()[0]
    kf_w2c = np.asarray(c["kf_w2c"] if kf_w2c is None else kf_w2c)
    kf_depth = np.asarray(c["kf_depth"] if kf_depth is None else kf_depth)
    record, pm = run_abi(dev, c, rc, kf_w2c, kf_depth, slots, edge, thresh)
    sel = list(range(len(kf_w2c))) if slots is None else list(slots)
    k = len(sel)
    H, W = c["gt_depth"].shape[-2:]
    src = ku.sources(c) if rc is None else torch.as_tensor(np.asarray(rc)).long()
    _, kept = ku.kept_rule(c, src)
    kept = kept.numpy()
    if rc is None:                                           # dense: the mask is indexed by pixel; everything else is 0xFF
        pix = (src[:, 0] * W + src[:, 1]).numpy()
        other = np.ones(H * W, dtype=bool)
        other[pix] = False
        assert (pm[:, other] == 0xFF).all()
        pm = pm[:, pix]
    assert ((pm == 0xFF) == ~kept[None]).all()               # the drop rule: repeats in all copies, the origin point
    assert ((pm == 0) | (pm == 1) | (pm == 0xFF)).all()
    m64, margin = ku.masks_f64(c, src, kf_w2c[sel], kf_depth[sel], edge, thresh)
    m64, margin = m64.numpy(), margin.numpy()
    diff = ((pm == 1) != m64) & kept[None]
    worst = float(margin[diff].max()) if diff.any() else 0.0
    band = (margin < tau) & kept[None]
    print(f"pairs {k * int(kept.sum())} differing {int(diff.sum())} (largest margin {worst:.3e}) in band {int(band.sum())} tau {tau:.3e}")
    assert worst < tau, (worst, tau)
    assert band.sum() <= ku.BAND_SHARE * max(1, k * int(kept.sum()))
    assert record[:k].tolist() == (pm == 1).sum(axis=1).tolist()                    # counts = mask sums, exactly
    assert record[k] == kept.sum() and record[k + 1] == len(kept) and record[k + 2] == len(kept) - kept.sum()
    return record, band.sum(axis=1)


# ---- the fixture ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["a_t001", "a_t005", "a_sampled", "b", "d", "d_sampled"])
def test_fixture_counts_and_decision_parity(gpu_device, name):
    c = ku.cases()[name]
    record, band = check(gpu_device, c, rc=c["rc"])
    k = len(c["counts"])
    assert record[k] == c["n"]                                                       # kept points: exact
    valid = len(c["rc"]) if c["rc"] is not None else int((c["gt_depth"] > 0).sum())
    assert record[k + 1] == valid and record[k + 2] == valid - c["n"]                # dropped: repeats (a triple too), origin
    assert (np.abs(record[:k] - c["counts"]) <= band).all(), (record[:k], c["counts"], band)


# ---- hand-placed sizes -----------------------------------------------------------------------------------------------------------
def hand(W, H, K, seed=0, invalid=0.04, spread=0.12):
    g = torch.Generator().manual_seed(1000 + seed)
    d = 1.8 + 0.9 * torch.rand(1, H, W, generator=g)
    d[torch.rand(1, H, W, generator=g) < invalid] = 0.0
    k = np.array([[0.9 * W, 0, W / 2 - 0.37], [0, 0.95 * W, H / 2 + 0.21], [0, 0, 1]], dtype=np.float32)
    w2c = np.eye(4, dtype=np.float32)
    w2c[:3, 3] = [0.02, -0.01, 0.03]
    poses = np.tile(np.eye(4, dtype=np.float32), (K, 1, 1))
    tr = (torch.rand(K, 3, generator=g) * 2 - 1) * spread
    ang = (torch.rand(K, generator=g) * 2 - 1) * 0.1
    for j in range(K):
        cs, sn = float(torch.cos(ang[j])), float(torch.sin(ang[j]))
        poses[j, :3, :3] = [[cs, 0, sn], [0, 1, 0], [-sn, 0, cs]]
        poses[j, :3, 3] = tr[j].numpy() * [1, 1, 0.3]
    depths = (d * (1 + 0.02 * torch.randn(K, H, W, generator=g))).clamp(min=0)
    return dict(gt_depth=d.numpy(), k=k, w2c=w2c, kf_w2c=poses, kf_depth=depths.numpy(), edge=2, thresh=0.03)


def planted(c, samples, seed=0):
    """`samples` (row, col) pairs on valid pixels; from 4 samples on with a planted pair, from 8 on also a triple."""
    g = torch.Generator().manual_seed(77 + seed)
    src = ku.sources(c)
    rc = src[torch.randint(src.shape[0], (samples,), generator=g)].clone()
    if samples >= 4:
        rc[samples - 1] = rc[0]
    if samples >= 8:
        rc[3] = rc[5] = rc[2]
    return rc.numpy().astype(np.int32)


@pytest.mark.parametrize("size", [(45, 37), (33, 17)])
@pytest.mark.parametrize("K", [1, 3, 65])
def test_dense_sizes(gpu_device, size, K):
    c = hand(size[0], size[1], K, seed=K)
    record, _ = check(gpu_device, c)
    assert record[:K].sum() > 0


@pytest.mark.parametrize("samples", [1, 63, 64, 65, 1600])
def test_sampled_sizes_with_planted_repeats(gpu_device, samples):
    c = hand(45, 37, 3, seed=samples)
    rc = planted(c, samples)
    record, _ = check(gpu_device, c, rc=rc)
    _, cnt = np.unique(rc, axis=0, return_counts=True)
    assert record[3 + 2] == cnt[cnt > 1].sum() and record[3] == samples - cnt[cnt > 1].sum()
    if samples >= 8:
        assert record[3 + 2] >= 5
    c65 = hand(33, 17, 65, seed=samples)
    check(gpu_device, c65, rc=planted(c65, samples, seed=1))


# The host splits keyframes over blockIdx.y only until the grid holds ~1024 workgroups (csrc/vtgs_api.hip): slices =
# min(K, ceil(1024 / gx)), at least ceil(K / 256).  The cases above all run ONE keyframe per workgroup; these run several.
def _slicing(W, H, samples, K):
    gx = ((samples or W * H) + 255) // 256
    slices = max(min(K, max(1, -(-1024 // gx))), -(-K // 256))
    per = -(-K // slices)
    return per, -(-K // per)


@pytest.mark.parametrize("K", [200, 300])
def test_several_keyframes_per_slice_small_frame(gpu_device, K):
    per, slices = _slicing(45, 37, 0, K)
    assert per >= 2 and slices >= 2 and per * slices >= K > per * (slices - 1)      # K = 200: a ragged last slice
    c = hand(45, 37, K, seed=K, spread=0.3)
    record, _ = check(gpu_device, c)
    assert len(set(record[:K].tolist())) > 10 and record[:K].sum() > 0               # the keyframes really differ
    rc = planted(c, 1600, seed=K)
    check(gpu_device, c, rc=rc)


@pytest.mark.parametrize("K", [3, 65, 260])
def test_one_slice_or_forced_split_on_a_large_dense_frame(gpu_device, K):
    """640 x 480: 1200 workgroups by themselves, so every K <= 256 runs in ONE slice (the production dense shape) and K = 260
    takes the forced split into 2 slices of 130.  Sparse valid depth keeps the float64 restatement small; no visibility test
    for the distinct poses (a [K, 480, 640] depth table would be large), and a second run WITH the visibility test whose
    keyframes are slots into four resident rows."""
    W, H = 640, 480
    per, slices = _slicing(W, H, 0, K)
    assert (per, slices) == ((K, 1) if K <= 256 else (130, 2))
    c = hand(W, H, 4, seed=40 + K, invalid=0.0, spread=0.3)                               # keyframe depths stay dense
    keep = torch.rand(H, W, generator=torch.Generator().manual_seed(K)) < 0.008
    keep[H - 1, W - 1] = True                                                             # the last lane of the last workgroup
    c["gt_depth"] = np.where(keep.numpy()[None], c["gt_depth"], 0).astype(np.float32)
    g = torch.Generator().manual_seed(K)
    poses = np.tile(np.eye(4, dtype=np.float32), (K, 1, 1))
    poses[:, :3, 3] = ((torch.rand(K, 3, generator=g) * 2 - 1) * torch.tensor([0.9, 0.7, 0.1])).numpy()
    record, _ = check(gpu_device, c, kf_w2c=poses, kf_depth=np.zeros((K, 1, 1), dtype=np.float32), thresh=None)
    assert len(set(record[:K].tolist())) >= 2
    slots = torch.randint(4, (K,), generator=g).tolist()
    part, _ = check(gpu_device, c, slots=slots)
    full, _ = check(gpu_device, c)
    assert part[:K].tolist() == full[slots].tolist() and len(set(full[:4].tolist())) >= 2 and full[:4].min() > 0


def test_a_negative_slot_counts_nothing(gpu_device):
    c = hand(45, 37, 3, seed=11)
    full, pm_full = run_abi(gpu_device, c)
    part, pm = run_abi(gpu_device, c, slots=[2, -1, 0, -7])
    assert part[:4].tolist() == [full[2], 0, full[0], 0] and part[4:].tolist() == full[3:].tolist()
    assert (pm[0] == pm_full[2]).all() and (pm[2] == pm_full[0]).all()
    dropped = pm_full[0] == 0xFF
    assert (pm[1][~dropped] == 0).all() and (pm[1][dropped] == 0xFF).all() and (pm[3] == pm[1]).all()


def test_slots_permutation_with_a_repeated_slot(gpu_device):
    c = hand(45, 37, 6, seed=5)
    full, _ = check(gpu_device, c)
    slots = [4, 0, 5, 0, 2]
    part, _ = check(gpu_device, c, slots=slots)
    assert part[:5].tolist() == full[slots].tolist() and part[5:].tolist() == full[6:].tolist()
    rc = planted(c, 200)
    full, _ = check(gpu_device, c, rc=rc)
    part, _ = check(gpu_device, c, rc=rc, slots=slots)
    assert part[:5].tolist() == full[slots].tolist()


def test_without_keyframe_depths(gpu_device):
    c = hand(45, 37, 3, seed=9)
    vis, _ = check(gpu_device, c)
    plain, _ = check(gpu_device, c, thresh=None)
    assert (plain[:3] >= vis[:3]).all() and (plain[:3] > vis[:3]).any() and plain[3:].tolist() == vis[3:].tolist()
    check(gpu_device, c, rc=planted(c, 65), thresh=None)


def test_all_invalid_depth_counts_nothing(gpu_device):
    c = hand(33, 17, 3, seed=2)
    c["gt_depth"] = np.zeros_like(c["gt_depth"])
    record, pm = run_abi(gpu_device, c)
    assert record.tolist() == [0] * 6 and (pm == 0xFF).all()


def test_every_point_behind_a_keyframe(gpu_device):
    c = hand(45, 37, 3, seed=3)
    c["kf_w2c"][1] = np.diag([-1, 1, -1, 1]).astype(np.float32)          # turned away: z' < 0 for every point
    record, _ = check(gpu_device, c)
    assert record[1] == 0 and record[0] > 0 and record[2] > 0


def test_edge_zero_reaches_the_zero_padded_tap(gpu_device):
    W, H = 45, 37
    c = hand(W, H, 1, seed=4, invalid=0.0)
    c["gt_depth"][:] = 2.0
    c["w2c"] = np.eye(4, dtype=np.float32)
    c["kf_w2c"] = np.eye(4, dtype=np.float32)[None].copy()
    c["kf_w2c"][0, 0, 3] = 0.5 * 2.0 / c["k"][0, 0]                      # u = column + 0.5: the last column lands in (W-1, W)
    c["kf_w2c"][0, 1, 3] = 0.5 * 2.0 / c["k"][1, 1]                      # v = row + 0.5 likewise (and no pixel sits ON an edge)
    c["kf_depth"] = np.full((1, H, W), 2.0, dtype=np.float32)
    plain, _ = check(gpu_device, c, edge=0, thresh=None)
    vis, _ = check(gpu_device, c, edge=0, thresh=0.03)
    _, pm = run_abi(gpu_device, c, edge=0, thresh=0.03)
    pm = pm.reshape(H, W)
    _, pm_plain = run_abi(gpu_device, c, edge=0, thresh=None)
    assert (pm_plain == 1).all() and plain[0] == W * H                   # all inside the image at edge 0 ...
    assert not pm[:, W - 1].any() and not pm[H - 1, :].any()             # ... but half of the last column's / row's sample is padding
    assert (pm[:H - 1, :W - 1] == 1).all() and vis[0] == (W - 1) * (H - 1)


def test_keyframe_equal_to_the_current_frame(gpu_device):
    c = hand(45, 37, 3, seed=6)
    c["kf_w2c"][1] = c["w2c"]
    c["kf_depth"][1] = c["gt_depth"][0]
    c["gt_depth"][:] = np.where(c["gt_depth"] > 0, 2.25, 0)              # a plane: a neighbour tap of weight ~1e-6 changes nothing
    c["kf_depth"][1] = c["gt_depth"][0]
    vis, _ = check(gpu_device, c, edge=2.5, thresh=0.01)                 # (2.5: no pixel centre sits ON the edge)
    plain, _ = check(gpu_device, c, edge=2.5, thresh=None)
    assert vis[1] == plain[1] > 0                                         # every kept point inside the edge band is visible


# ---- the Python layer ---------------------------------------------------------------------------------------------------------
def _list(c, sel=None):
    idx = range(len(c["kf_w2c"])) if sel is None else sel
    return [{"id": i, "est_w2c": torch.tensor(c["kf_w2c"][i]), "depth": torch.tensor(c["kf_depth"][i])[None]} for i in idx]


def _frame(c, dev):
    return torch.tensor(c["gt_depth"]).to(dev), torch.tensor(c["w2c"]).to(dev), torch.tensor(c["k"]).to(dev)


def _pl(lst):
    return [d["id"] for d in lst], [d["percent_inside"].item() for d in lst]


def _ids(x):
    return [int(i) for i in x]


def test_drop_ins_return_the_reference_lists(gpu_device, kf):
    fx, cs = ku.fixture(), ku.cases()
    for name in ("a_t001", "a_t005"):
        c = cs[name]
        gd, w2c, k = _frame(c, gpu_device)
        lst = _list(c)
        before = [(id(d), id(d["est_w2c"]), id(d["depth"]), d["depth"].device, d["est_w2c"].device) for d in lst]
        store = kf.KeyframeStore.from_list(lst, gpu_device)
        for keyframes in (lst, store):
            got = kf.keyframe_selection_overlap_visbased(gd, w2c, k, keyframes, 3, edge_value=c["edge"], save_percent=True,
                                                         kf_depth_thresh=c["thresh"])
            ids, pct = _pl(got)
            assert ids == _ids(c["ids"]) and np.array_equal(np.array(pct, dtype=np.float32), c["percent"])
            assert all(d["percent_inside"].dim() == 0 and d["percent_inside"].dtype == torch.float32 for d in got)
            sel, ear = kf.keyframe_selection_overlap_visbased(gd, w2c, k, keyframes, 3, edge_value=c["edge"],
                                                              kf_depth_thresh=c["thresh"], earliest_thres=fx[name + "_earliest_thres"])
            assert _ids(sel) == _ids(fx[name + "_selected"]) and _ids(ear) == _ids(fx[name + "_earliest"])
        assert before == [(id(d), id(d["est_w2c"]), id(d["depth"]), d["depth"].device, d["est_w2c"].device) for d in lst]
    c = cs["a_sampled"]
    gd, w2c, k = _frame(c, gpu_device)
    lst, rc = _list(c), torch.tensor(c["rc"])
    store = kf.KeyframeStore.from_list(lst, gpu_device)
    for keyframes in (lst, store):
        ids, pct = _pl(kf.keyframe_selection_overlap(gd, w2c, k, keyframes, 3, pixels=100, edge_value=c["edge"], save_percent=True,
                                                     sampled_indices=rc))
        assert ids == _ids(c["ids"]) and np.array_equal(np.array(pct, dtype=np.float32), c["percent"])
        sel = kf.keyframe_selection_overlap(gd, w2c, k, keyframes, 3, pixels=100, edge_value=c["edge"], sampled_indices=rc)
        assert _ids(sel) == _ids(fx["a_sampled_selected"])
        corr = fx["a_corr_list"].tolist()
        got = kf.find_earliest_keyframe(corr, gd, w2c, k, keyframes, 3, c["edge"], 4, fx["a_chain_threshold"], pixels=100,
                                        sampled_indices=rc)
        assert got == [int(fx["a_chain_result"][0]), None, int(fx["a_chain_result"][1])]
        got = kf.find_earliest_keyframe(corr, gd, w2c, k, keyframes, 3, c["edge"], 4, 0.0, pixels=100, sampled_indices=rc)
        assert got[0] == int(fx["a_chain_result_thr0"][0])
    drawn = kf.keyframe_selection_overlap(gd, w2c, k, store, 3, pixels=100, edge_value=c["edge"])       # its own draw
    assert len(drawn) == 3 and all(0 <= int(i) < 6 for i in drawn)
    b = cs["b"]
    gd, w2c, k = _frame(b, gpu_device)
    cfg = {"baseframe_every": int(fx["b_baseframe_every"]), "overlap_every": int(fx["b_overlap_every"])}
    lst = _list(b)
    for keyframes in (lst, kf.KeyframeStore.from_list(lst, gpu_device)):
        for name, topk in (("top3", 3), ("top2", 2), ("none", None)):
            got = kf.keyframe_selection_overlap_visbased_earliest_dynamic_new_topkbase(
                gd, w2c, k, keyframes, 3, cfg, edge_value=b["edge"], kf_depth_thresh=b["thresh"],
                earliest_thres=fx["b_earliest_thres"], lower_earliest_thres_percent=fx["b_lower"], topk_base=topk)
            assert got == _ids(fx["b_" + name]), name
    away = [{"est_w2c": torch.tensor(fx["b_away_kf_w2c"][i]), "depth": torch.tensor(b["kf_depth"][i])} for i in range(8)]
    assert kf.keyframe_selection_overlap_visbased_earliest_dynamic_new_topkbase(
        gd, w2c, k, away, 3, cfg, edge_value=b["edge"], kf_depth_thresh=b["thresh"]) == _ids(fx["b_away_topkbase"])
    assert kf.keyframe_selection_overlap_visbased_earliest_dynamic_new_topkbase(
        torch.zeros_like(gd), w2c, k, lst, 3, cfg, edge_value=b["edge"], kf_depth_thresh=b["thresh"]) == _ids(fx["b_n0_topkbase"])
    assert all(d["depth"].device.type == "cpu" for d in lst)


def test_store_growth_and_set_pose(gpu_device, kf):
    c = hand(45, 37, 5, seed=8)
    gd, w2c, k = _frame(c, gpu_device)
    store = kf.KeyframeStore(37, 45, capacity=2, device=gpu_device)
    for j in range(2):
        assert store.append(c["kf_w2c"][j], c["kf_depth"][j]) == j
    d0, p0 = store.depth[:2].clone(), store.w2c[:2].clone()
    for j in range(2, 5):
        assert store.append(torch.tensor(c["kf_w2c"][j]), torch.tensor(c["kf_depth"][j])[None]) == j
    assert len(store) == 5 and store.capacity == 8
    assert torch.equal(store.depth[:2], d0) and torch.equal(store.w2c[:2], p0)             # growth keeps earlier slots
    assert torch.equal(store.depth[:5].cpu(), torch.tensor(c["kf_depth"])) and torch.equal(store.w2c[:5].cpu(),
                                                                                            torch.tensor(c["kf_w2c"]).reshape(5, 16))
    first = kf.overlap_counts(gd, w2c, k, store, edge_value=2, kf_depth_thresh=0.03).cpu().numpy()
    assert first.dtype == np.int32 and first.tolist() == check(gpu_device, c)[0].tolist()
    moved = c["kf_w2c"][3].copy()
    moved[0, 3] += 0.4
    store.set_pose(3, moved)
    second = kf.overlap_counts(gd, w2c, k, store, edge_value=2, kf_depth_thresh=0.03).cpu().numpy()
    assert second[3] != first[3] and np.delete(second, 3).tolist() == np.delete(first, 3).tolist()
    with pytest.raises(IndexError):
        store.set_pose(5, moved)
    with pytest.raises(IndexError):
        kf.overlap_counts(gd, w2c, k, store, slots=[0, 5])


def test_malformed_calls_leave_the_record_untouched(gpu_device, kf):
    from diff_gaussian_rasterization import _stream_ptr
    lib = kf._lib
    c = hand(45, 37, 3, seed=1)
    t32 = lambda a: torch.as_tensor(np.ascontiguousarray(a), dtype=torch.float32).contiguous().to(gpu_device)
    gd, kmat, w2c, poses, depths = t32(c["gt_depth"]), t32(c["k"]), t32(c["w2c"]), t32(c["kf_w2c"]), t32(c["kf_depth"])
    rc = torch.zeros(20000, 2, dtype=torch.int32, device=gpu_device)
    need = lib.vtgs_keyframe_overlap_scratch_bytes(45, 37, 100, 3)
    scratch = torch.full((need,), POISON, dtype=torch.uint8, device=gpu_device)
    record = torch.full((64,), POISON, dtype=torch.uint8, device=gpu_device)
    good = dict(rc=None, samples=0, n=3, sbytes=need, record=record.data_ptr())
    def call(**kw):
        a = {**good, **kw}
        return lib.vtgs_keyframe_overlap(45, 37, gd.data_ptr(), kmat.data_ptr(), w2c.data_ptr(), a["rc"], a["samples"], poses.data_ptr(),
                                         depths.data_ptr(), None, a["n"], 2.0, 0.03, None, scratch.data_ptr(), a["sbytes"],
                                         a["record"], _stream_ptr(gpu_device))
    assert call(record=record.data_ptr() + 2) == INVALID                                   # misaligned record
    assert call(rc=rc.data_ptr(), samples=16385) == INVALID
    assert call(n=0) == INVALID and call(n=-4) == INVALID
    assert call(sbytes=lib.vtgs_keyframe_overlap_scratch_bytes(45, 37, 0, 3) - 1) == INVALID
    assert call(rc=rc.data_ptr(), samples=100, sbytes=need - 1) == INVALID
    torch.cuda.synchronize(gpu_device)
    assert (record == POISON).all()
    assert call() == 0
    torch.cuda.synchronize(gpu_device)
    assert not (record[:24] == POISON).all() and (record[24:] == POISON).all()
