"""tests/golden/keyframes.npz (the reference's own keyframe selection, tests/golden/make_keyframe_fixtures.py) against this
repository's restatements, without a GPU: the float32 per-pair masks in the reference's operation order sum to the stored
counts EXACTLY; the pure selection functions of diff_gaussian_rasterization.keyframes return the reference's stored
selections from the stored counts (ties, n == 0, the fallback to the last keyframe); and the decision band the GPU test
grants -- measured here from float32 against float64 -- holds at most 0.5 % of a case's pairs."""
import numpy as np
import pytest

import keyframe_util as ku


@pytest.fixture(scope="module")
def kf():
    from diff_gaussian_rasterization import keyframes
    return keyframes


@pytest.mark.parametrize("name", ["a_t001", "a_t005", "a_sampled", "b", "d", "d_sampled"])
def test_float32_masks_sum_to_the_reference_counts(name):
    c = ku.cases()[name]
    masks, kept = ku.masks_f32(c)
    assert int(kept.sum()) == c["n"]                                    # repeats in all copies + the origin point, nothing else
    assert masks.sum(dim=1).tolist() == c["counts"].tolist()
    assert np.array_equal((c["counts"].astype(np.float32) / np.float32(c["n"]))[c["ids"]], c["percent"])   # counts are exact


def test_fixture_drops_are_the_documented_ones():
    cs = ku.cases()
    assert cs["a_sampled"]["n"] == 95 and cs["a_sampled"]["rc"].shape == (100, 2)         # a planted triple and pair
    rc = cs["a_sampled"]["rc"]
    assert (rc[5] == rc[6]).all() and (rc[5] == rc[7]).all() and (rc[20] == rc[21]).all()
    d = cs["d"]
    assert d["n"] == int((d["gt_depth"] > 0).sum()) - 1 and d["gt_depth"][0, 18, 22] == 2.0
    pts, kept = ku.kept_rule(d)
    src = ku.sources(d)
    assert (~kept).sum() == 1 and src[~kept][0].tolist() == [18, 22]
    assert (cs["d_sampled"]["rc"][40] == [18, 22]).all()


def test_band_share_of_the_reference_masks():
    tau, worst, floor = ku.measure_tau()
    print(f"float32 reference masks vs float64: largest disagreeing margin {worst:.3e}, floor {floor:.3e}, tau {tau:.3e}")
    assert tau < 1e-4                                                    # a band of rounding, not of modelling
    for name, c in ku.cases().items():
        _, kept = ku.masks_f32(c)
        _, margin = ku.masks_f64(c)
        share = float(((margin < tau) & kept[None]).sum()) / max(1, margin.shape[0] * int(kept.sum()))
        print(name, "pairs in band", int(((margin < tau) & kept[None]).sum()), "share", share)
        assert share <= ku.BAND_SHARE, (name, share)


def _ids(x):
    return [int(i) for i in x]


def test_select_overlap_and_visbased_return_the_stored_selections(kf):
    fx, cs = ku.fixture(), ku.cases()
    c = cs["a_sampled"]
    assert _ids(kf.select_overlap(c["counts"], c["n"], 3)) == _ids(fx["a_sampled_selected"])
    order = [i for i, _ in kf._sorted_desc(kf.percents(c["counts"], c["n"]))]
    assert order == _ids(c["ids"]) and np.array_equal(kf.percents(c["counts"], c["n"])[order], c["percent"])
    for name in ("a_t001", "a_t005"):
        c = cs[name]
        sel, ear = kf.select_visbased(c["counts"], c["n"], 3, fx[name + "_earliest_thres"])
        assert _ids(sel) == _ids(fx[name + "_selected"]) and _ids(ear) == _ids(fx[name + "_earliest"])
        sel, ear = kf.select_visbased(c["counts"], c["n"], 3, 2.0)            # nobody passes: earliest falls back to selected
        assert _ids(ear) == _ids(sel) == _ids(fx[name + "_selected"])
    b = cs["b"]                                                               # keyframes 2 and 5 tie: the stable order
    order = [i for i, _ in kf._sorted_desc(kf.percents(b["counts"], b["n"]))]
    assert order == _ids(b["ids"]) and b["counts"][2] == b["counts"][5] and order.index(2) < order.index(5)


def test_select_topkbase_returns_the_stored_base_frames(kf):
    fx, b = ku.fixture(), ku.cases()["b"]
    cfg = {"baseframe_every": int(fx["b_baseframe_every"]), "overlap_every": int(fx["b_overlap_every"])}
    for name, topk in (("top3", 3), ("top2", 2), ("none", None)):
        got = kf.select_topkbase(b["counts"], b["n"], cfg, fx["b_earliest_thres"], fx["b_lower"], topk)
        assert got == _ids(fx["b_" + name]), name
    zeros = np.zeros(8, dtype=np.int64)
    assert kf.select_topkbase(zeros, b["n"], cfg, 0.5, 0.8, 3) == _ids(fx["b_away_topkbase"]) == [3]    # the last keyframe
    assert kf.select_topkbase(zeros, 0, cfg, 0.5, 0.8, 3) == _ids(fx["b_n0_topkbase"]) == [3]          # n == 0: NaN percents
    assert kf.select_overlap(zeros, 0, 3) == [] and kf.select_visbased(zeros, 0, 3, 0.5) == ([], [])
    assert kf.select_overlap(zeros, b["n"], 3) == [] and kf.select_visbased(zeros, b["n"], 3, 0.5) == ([], [])
    assert np.isnan(kf.percents(zeros, 0)).all()


def test_walk_earliest_returns_the_stored_chain_results(kf):
    fx, c = ku.fixture(), ku.cases()["a_sampled"]
    corr = fx["a_corr_list"].tolist()
    counts = {i: int(v) for i, v in enumerate(c["counts"])}
    got = kf.walk_earliest(corr, counts, c["n"], 4, fx["a_chain_threshold"])
    assert got == [int(fx["a_chain_result"][0]), None, int(fx["a_chain_result"][1])] == [0, None, 16]
    got = kf.walk_earliest(corr, counts, c["n"], 4, 0.0)
    assert got == [int(fx["a_chain_result_thr0"][0]), None, int(fx["a_chain_result_thr0"][1])]
    assert kf.resolve_chain(corr) == (12, 16, [4, 0, 8])
    assert kf.walk_earliest(corr, counts, c["n"], 4, 2.0) == [12, None, 16]                 # the first link fails already
    assert kf.walk_earliest([[5, 6, 7]], {}, 0, 4, 0.1) == [5, None, 7]                     # no link at all
    assert kf.walk_earliest(corr, {0: 0, 1: 0, 2: 0}, 0, 4, 0.1) == [12, None, 16]          # n == 0: NaN > threshold is false


def test_an_empty_keyframe_list_gives_the_reference_returns_without_a_launch(kf):
    import torch
    gd, w2c, k = torch.ones(1, 4, 5), torch.eye(4), torch.eye(3)             # CPU tensors: nothing may touch a device
    for empty in ([], kf.KeyframeStore.__new__(kf.KeyframeStore)):
        if not isinstance(empty, list):
            empty._n = 0                                                      # a store that holds no keyframe yet
        assert kf.keyframe_selection_overlap(gd, w2c, k, empty, 3) == []
        assert kf.keyframe_selection_overlap(gd, w2c, k, empty, 3, save_percent=True) == []
        assert kf.keyframe_selection_overlap_visbased(gd, w2c, k, empty, 3) == ([], [])
        assert kf.keyframe_selection_overlap_visbased(gd, w2c, k, empty, 3, save_percent=True) == []
        with pytest.raises(IndexError):
            kf.keyframe_selection_overlap_visbased_earliest_dynamic_new_topkbase(gd, w2c, k, empty, 3, {"baseframe_every": 4,
                                                                                                      "overlap_every": 2})
        with pytest.raises(IndexError):
            kf.find_earliest_keyframe([[0, 3, 4], [4, 7, 8]], gd, w2c, k, empty, 3, 4, 4, 0.1)
        assert kf.find_earliest_keyframe([[5, 6, 7]], gd, w2c, k, empty, 3, 4, 4, 0.1) == [5, None, 7]
