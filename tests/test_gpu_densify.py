"""vtgs_densify (csrc/vtgs_densify.hip) and its Python mirror (diff_gaussian_rasterization/densify.py).

Fixture parity: tests/golden/densify.npz holds what the reference's OWN add_new_gaussians_base_frame and
initialize_params_base_timestep returned (tests/golden/make_densify_fixtures.py).  Count, row order, colours, rotations,
opacities, timestep and the median must be EXACT; means3D and log_scales are float32 results of a different but equivalent
route (rigid inverse and fused multiply-adds instead of torch.inverse and a 4x4 product), so they are held to a tolerance
that is MEASURED, not chosen: the distance of the fixture's own float32 values from the float64 restatement below is the
yardstick, the kernel gets 4 x that, with a floor of 4 float32 ulps of the largest coordinate magnitude (DESIGN.md 11 records
both distances).  Hand-placed 33 x 17 images (66 x 34 dense: no multiple of the wavefront, the workgroup or the 512-pixel
chunk) cover the chunk edges, the empty and the full selection, capacity handling and the parameter forms."""
import ctypes
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
KEYS = ("means3D", "rgb_colors", "unnorm_rotations", "logit_opacities", "log_scales")
COLS = {"means3D": 3, "rgb_colors": 3, "unnorm_rotations": 4, "logit_opacities": 1}
CHUNK = 512                     # kDensifyChunk of csrc/vtgs_kernels.h
POISON = 0x5A


@pytest.fixture(scope="module")
def fx():
    z = np.load(os.path.join(HERE, "golden", "densify.npz"))
    return {k: (z[k] if z[k].ndim else z[k].item()) for k in z.files}


# ---- the float64 restatement ------------------------------------------------------------------------------------------------
def _rot_f64(q):
    q = torch.as_tensor(q, dtype=torch.float64)
    r, x, y, z = (q / q.norm()).tolist()
    return torch.tensor([[1 - 2 * (y * y + z * z), 2 * (x * y - r * z), 2 * (x * z + r * y)],
                         [2 * (x * y + r * z), 1 - 2 * (x * x + z * z), 2 * (y * z - r * x)],
                         [2 * (x * z - r * y), 2 * (y * z + r * x), 1 - 2 * (x * x + y * y)]], dtype=torch.float64)


def _c2w_f64(c):
    if c.get("w2c") is not None:
        return torch.inverse(torch.as_tensor(c["w2c"], dtype=torch.float64))
    rots, trans, t = c["cam"]
    m = torch.eye(4, dtype=torch.float64)
    m[:3, :3] = _rot_f64(np.asarray(rots)[0, :, t])
    m[:3, 3] = torch.as_tensor(np.asarray(trans)[0, :, t], dtype=torch.float64)
    return torch.inverse(m)


def _cloud(im, depth, k, sel, c2w):
    H, W = depth.shape
    k = torch.as_tensor(k, dtype=torch.float64)
    ys, xs = torch.meshgrid(torch.arange(H, dtype=torch.float64), torch.arange(W, dtype=torch.float64), indexing="ij")
    z = torch.as_tensor(depth, dtype=torch.float64) * 1.005
    pts = torch.stack(((xs - k[0, 2] + 0.5) / k[0, 0] * z, (ys - k[1, 2] + 0.5) / k[1, 1] * z, z, torch.ones_like(z)), -1).reshape(-1, 4)
    means = (c2w @ pts.T).T[:, :3]
    ls = torch.log(z / ((k[0, 0] + k[1, 1]) / 2)).reshape(-1)
    cols = torch.as_tensor(im).reshape(3, -1).T
    return means[sel], cols[sel], ls[sel]


def restate(c):
    """The reference's masks in float32 with its own operation order (src/vtgaussian_slam.py:748-788; the SET is exact), the
    rows of the selected pixels in float64."""
    gd = torch.as_tensor(c["gt_depth"], dtype=torch.float32)
    H, W = gd.shape
    med = float("nan")
    if c.get("depth_sil") is not None:
        ds = torch.as_tensor(c["depth_sil"], dtype=torch.float32)
        rd, sil = ds[0], ds[1]
        err = torch.abs(gd - rd) * (gd > 0)
        med_t = err.median()
        un = (sil < c["sil_thres"]) | ((rd > gd) * (err > 50 * med_t))
        med = med_t.item()
    else:
        un = torch.ones(H, W, dtype=torch.bool)
    c2w = _c2w_f64(c)
    parts = [_cloud(c["gt_im"], gd, c["k"], (un & (gd > 0)).reshape(-1), c2w)]
    if c.get("dense") is not None:
        im_d, gd_d, k_d = c["dense"]
        gd_d = torch.as_tensor(gd_d, dtype=torch.float32)
        dH, dW = gd_d.shape
        sel = (gd_d > 0) & un[(torch.arange(dH) * H) // dH][:, (torch.arange(dW) * W) // dW]
        if c.get("mask") is not None:
            m = torch.as_tensor(c["mask"]) != 0
            sel &= m[(torch.arange(dH) * m.shape[0]) // dH][:, (torch.arange(dW) * m.shape[1]) // dW]
        parts.append(_cloud(im_d, gd_d, k_d, sel.reshape(-1), c2w))
    return {"added_ori": parts[0][0].shape[0], "added_dense": parts[1][0].shape[0] if len(parts) > 1 else 0,
            "unexplained": int(un.sum()), "median": med, "means3D": torch.cat([p[0] for p in parts]).numpy(),
            "rgb_colors": torch.cat([p[1] for p in parts]).numpy(), "log_scales": torch.cat([p[2] for p in parts]).numpy()}


# ---- the C ABI, on poisoned memory ------------------------------------------------------------------------------------------
def run_abi(dev, c, n=7, capacity=None, null_maps=False, scale_columns=1, timestep=True, time_value=3.0):
    from diff_gaussian_rasterization import _stream_ptr
    from diff_gaussian_rasterization import densify as dz
    lib = dz._lib
    t32 = lambda a: None if a is None else torch.as_tensor(np.ascontiguousarray(a), dtype=torch.float32).contiguous().to(dev)
    p = lambda x: None if x is None else x.data_ptr()
    gd = t32(c["gt_depth"]); H, W = gd.shape
    im, k, ds = t32(c["gt_im"]), t32(c["k"]), t32(c.get("depth_sil"))
    dW = dH = mW = mH = 0
    im_d = gd_d = k_d = m = None
    if c.get("dense") is not None:
        if c["dense"] == "same":
            im_d, gd_d, k_d = im, gd, k
        else:
            im_d, gd_d, k_d = (t32(a) for a in c["dense"])
        dH, dW = gd_d.shape
        if c.get("mask") is not None:
            m = torch.as_tensor(np.ascontiguousarray(c["mask"]), dtype=torch.uint8).to(dev)
            mH, mW = m.shape
    w = rots = trans = None
    frames = t = 0
    if c.get("w2c") is not None:
        w = t32(c["w2c"]).reshape(16)
    else:
        rots, trans, t = t32(c["cam"][0]), t32(c["cam"][1]), int(c["cam"][2])
        frames = rots.shape[-1]
    cap = 0 if null_maps else capacity
    rows = max(cap, n) + 3 if not null_maps else 0                 # + 3: rows beyond the capacity must stay untouched too
    cols = dict(COLS, log_scales=scale_columns, timestep=1)
    arrays = {}
    if not null_maps:
        for key in KEYS + (("timestep",) if timestep else ()):
            arrays[key] = torch.full((rows * cols[key] * 4,), POISON, dtype=torch.uint8, device=dev)
    before = {key: a.clone() for key, a in arrays.items()}
    sbytes = int(lib.vtgs_densify_scratch_bytes(W, H, dW, dH))
    assert sbytes > 0
    scratch = torch.full((sbytes,), 0xC3, dtype=torch.uint8, device=dev)
    rec = torch.full((8,), 0x6B6B6B6B, dtype=torch.int32, device=dev)
    ptrs = [p(arrays.get(key)) for key in KEYS + ("timestep",)]
    rc = lib.vtgs_densify(W, H, p(ds), p(im), p(gd), p(k), dW, dH, p(im_d), p(gd_d), p(k_d), p(m), mW, mH, p(w), p(rots), p(trans),
                          frames, t, float(c.get("sil_thres", 0.5)), float(time_value), scale_columns, n, cap, *ptrs,
                          scratch.data_ptr(), sbytes, rec.data_ptr(), _stream_ptr(dev))
    assert rc == 0, rc
    info = dz.read_info(rec)
    assert info["complete"] == 1
    out = {key: a.cpu().view(torch.float32).reshape(rows, cols[key]).numpy() for key, a in arrays.items()}
    return info, out, {key: a.cpu().numpy() for key, a in before.items()}, {key: a.cpu().numpy() for key, a in arrays.items()}


def _ulp4(x):
    return 4.0 * float(np.spacing(np.float32(np.abs(x).max())))


@pytest.fixture(scope="module")
def frame_case(fx):
    return {"gt_im": fx["gt_im"], "gt_depth": fx["gt_depth"][0], "k": fx["intrinsics"], "depth_sil": fx["frame_depth_sil"],
            "dense": (fx["gt_im_dense"], fx["gt_depth_dense"][0], fx["intrinsics_dense"]), "mask": fx["mask_variation"],
            "cam": (fx["map_cam_unnorm_rots"], fx["map_cam_trans"], fx["t_idx"]), "sil_thres": fx["sil_thres"]}


@pytest.fixture(scope="module")
def seed_case(fx):
    return {"gt_im": fx["seed_color"], "gt_depth": fx["gt_depth"][0], "k": fx["intrinsics"], "depth_sil": None,
            "dense": (fx["seed_color_dense"], fx["gt_depth_dense"][0], fx["intrinsics_dense"]), "mask": fx["seed_mask"],
            "w2c": fx["seed_w2c"]}


@pytest.fixture(scope="module")
def yardstick(fx, frame_case, seed_case):
    """Distance of the reference's own float32 results from the float64 restatement, relative to the largest magnitude -- and
    a check that the restatement selects exactly the reference's rows (colours are copies: equal colours = equal order)."""
    d = {"means3D": 0.0, "log_scales": 0.0}
    for c, pre in ((frame_case, "frame_tail_"), (seed_case, "seed_")):
        r = restate(c)
        assert np.array_equal(r["rgb_colors"], fx[pre + "rgb_colors"])
        for key in d:
            ref = fx[pre + key].astype(np.float64).reshape(r[key].shape)
            d[key] = max(d[key], float(np.abs(ref - r[key]).max() / np.abs(r[key]).max()))
    print("yardstick (fixture vs float64, relative to the largest magnitude):", d)
    return d


def _allowed(yardstick, key, want):
    mag = float(np.abs(want).max())
    return max(4.0 * yardstick[key] * mag, _ulp4(want))


def _check_rows(yardstick, got, want, n, what):
    """rows [n, n + added) of the kernel's arrays against a restatement / fixture dict"""
    added = want["rgb_colors"].shape[0]
    sl = slice(n, n + added)
    assert np.array_equal(got["rgb_colors"][sl], want["rgb_colors"]), what + ": colours (= selection and order)"
    assert np.array_equal(got["unnorm_rotations"][sl], np.tile(np.float32([1, 0, 0, 0]), (added, 1)))
    assert np.array_equal(got["logit_opacities"][sl], np.zeros((added, 1), np.float32))
    dist = {}
    for key in ("means3D", "log_scales"):
        w = want[key].astype(np.float64)
        w = w.reshape(added, -1)
        g = got[key][sl].astype(np.float64)
        if g.shape[1] != w.shape[1]:                                   # anisotropic: the same value in each column
            w = np.repeat(w, g.shape[1], 1)
        dist[key] = float(np.abs(g - w).max()) if added else 0.0
        tol = _allowed(yardstick, key, w) if added else 0.0
        print(f"{what}: {key} max distance {dist[key]:.3e} (allowed {tol:.3e})")
        assert dist[key] <= tol, (what, key, dist[key], tol)
    return dist


# ---- fixture parity ---------------------------------------------------------------------------------------------------------
def test_frame_fixture_through_the_c_abi(gpu_device, fx, frame_case, yardstick):
    n, add = fx["map_means3D"].shape[0], fx["frame_add_number"]
    info, got, _, _ = run_abi(gpu_device, frame_case, n=n, capacity=n + add, time_value=float(fx["t_idx"]))
    assert (info["added_ori"], info["added_dense"], info["overflow"]) == (fx["frame_added_ori"], add - fx["frame_added_ori"], 0)
    assert info["unexplained"] == fx["frame_unexplained"] and info["nan_count"] == 0
    assert np.float32(info["median"]) == fx["frame_median"]                        # exact: the same element of the same values
    want = {k: fx["frame_tail_" + k] for k in KEYS}
    _check_rows(yardstick, got, want, n, "frame fixture, kernel vs the reference's float32")
    _check_rows(yardstick, got, restate(frame_case), n, "frame fixture, kernel vs float64")
    assert np.array_equal(got["timestep"][n:n + add, 0], fx["frame_timestep"][n:])


def test_seed_fixture_through_the_c_abi(gpu_device, fx, seed_case, yardstick):
    m = fx["seed_means3D"].shape[0]
    info, got, _, _ = run_abi(gpu_device, seed_case, n=0, capacity=m)
    assert (info["added_ori"], info["added_dense"], info["overflow"]) == (fx["seed_added_ori"], m - fx["seed_added_ori"], 0)
    assert info["unexplained"] == fx["W"] * fx["H"] and info["median"] != info["median"]
    _check_rows(yardstick, got, {k: fx["seed_" + k] for k in KEYS}, 0, "seed fixture, kernel vs the reference's float32")
    _check_rows(yardstick, got, restate(seed_case), 0, "seed fixture, kernel vs float64")


def test_frame_fixture_through_the_python_mirror(gpu_device, fx, yardstick):
    """add_new_gaussians_base_frame with the reference's signature: its own render (the HIP rasterizer instead of the oracle
    that stood behind the reference), then the same rows."""
    from oracle import gs_oracle as go
    from parity_util import to_settings
    from diff_gaussian_rasterization.densify import add_new_gaussians_base_frame
    dev = gpu_device
    W, H, t_idx = fx["W"], fx["H"], fx["t_idx"]
    tt = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
    st = to_settings(go.setup_camera(W, H, fx["intrinsics"], fx["first_w2c"]), dev)
    names = KEYS + ("cam_unnorm_rots", "cam_trans")
    params = {k: torch.nn.Parameter(tt(fx["map_" + k])) for k in names}
    n = params["means3D"].shape[0]
    variables = {"max_2D_radius": torch.ones(n, device=dev), "means2D_gradient_accum": torch.ones(n, device=dev),
                 "denom": torch.ones(n, device=dev), "timestep": torch.zeros(n, device=dev)}
    ori = {"cam": st, "im": tt(fx["gt_im"]), "depth": tt(fx["gt_depth"]), "id": t_idx, "intrinsics": tt(fx["intrinsics"]),
           "w2c": tt(fx["first_w2c"])}
    dense = {"cam": None, "im": tt(fx["gt_im_dense"]), "depth": tt(fx["gt_depth_dense"]), "id": t_idx,
             "intrinsics": tt(fx["intrinsics_dense"]), "w2c": tt(fx["first_w2c"])}
    params, variables, add = add_new_gaussians_base_frame(params, variables, ori, dense, fx["sil_thres"], t_idx, "projective",
                                                          "isotropic", {}, mask_variation=fx["mask_variation"].astype(bool))
    assert add == fx["frame_add_number"]
    got = {k: params[k].detach().cpu().numpy() for k in KEYS}
    for k in KEYS:
        assert isinstance(params[k], torch.nn.Parameter) and params[k].requires_grad and params[k].shape[0] == n + add
        assert np.array_equal(got[k][:n], fx["map_" + k])                           # the old rows, copied
    _check_rows(yardstick, got, {k: fx["frame_tail_" + k] for k in KEYS}, n, "frame fixture, Python mirror")
    assert np.array_equal(variables["timestep"].cpu().numpy(), fx["frame_timestep"])
    for k in ("max_2D_radius", "means2D_gradient_accum", "denom"):                   # reset, as at :803-806
        assert variables[k].shape == (n + add,) and float(variables[k].abs().sum()) == 0


def test_seed_fixture_through_the_python_mirror(gpu_device, fx, yardstick):
    from diff_gaussian_rasterization.densify import initialize_new_points
    tt = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(gpu_device)
    cld, msd = initialize_new_points(tt(fx["seed_color"]), tt(fx["gt_depth"]), tt(fx["intrinsics"]), tt(fx["seed_w2c"]),
                                     tt(fx["seed_color_dense"]), tt(fx["gt_depth_dense"]), tt(fx["intrinsics_dense"]),
                                     mask_variation=fx["seed_mask"])
    m = fx["seed_means3D"].shape[0]
    assert cld.shape == (m, 6) and msd.shape == (m,)
    cld, msd = cld.cpu().numpy(), msd.cpu().numpy().astype(np.float64)
    assert np.array_equal(cld[:, 3:], fx["seed_rgb_colors"])
    want = fx["seed_means3D"].astype(np.float64)
    assert np.abs(cld[:, :3] - want).max() <= _allowed(yardstick, "means3D", want)
    # mean3_sq_dist = exp(log scale)^2: what initialize_params makes of it, log sqrt(.), is the log scale again up to the three
    # roundings in between (exp, square, log: 2^-23 relative each, i.e. 3 x 2^-23 absolute in the logarithm; 4 allowed)
    ls = fx["seed_log_scales"].astype(np.float64)[:, 0]
    assert np.abs(0.5 * np.log(msd) - ls).max() <= _allowed(yardstick, "log_scales", ls) + 4 * 2.0 ** -23


# ---- hand-placed 33 x 17 ----------------------------------------------------------------------------------------------------
W0, H0, R0 = 33, 17, 2


def _hand(holes="edges", depth_zero_at_holes=False, ratio=R0):
    rng = np.random.default_rng(7)
    P = W0 * H0
    gd = (2.0 + rng.random((H0, W0))).astype(np.float32)
    sil = np.ones(P, np.float32)
    dW, dH = ratio * W0, ratio * H0
    if holes == "edges":
        idx = {0, P - 1, 63, 64, 255, 256, CHUNK - 1, CHUNK, 100}
        for e in range(CHUNK, dW * dH, CHUNK):                        # both sides of every chunk edge of the dense image
            for pd in (e - 1, e):
                idx.add(((pd // dW) // ratio) * W0 + (pd % dW) // ratio)
        idx |= {0 // 1, ((dH - 1) // ratio) * W0 + (dW - 1) // ratio}
        sil[sorted(idx)] = 0.25
    elif holes == "all":
        sil[:] = 0.0
    elif holes == "zero_depth":
        sil[[5, 300, CHUNK, P - 2]] = 0.1
    sil = sil.reshape(H0, W0)
    if depth_zero_at_holes:
        gd[sil < 0.5] = 0.0
    else:
        gd[3, 7] = 0.0                                                 # an invalid pixel that is not a hole
    rd = (gd + 0.001 * rng.standard_normal((H0, W0))).astype(np.float32)
    rd[8, 20] = gd[8, 20] + 1.5                                        # the depth branch: render well behind the observation
    if holes == "none":
        rd = gd.copy()                                                 # median 0, error 0: nothing exceeds 50 x median
    ds = np.stack([rd, sil, rd * rd]).astype(np.float32)
    gd_d = (np.repeat(np.repeat(gd, ratio, 0), ratio, 1) * (1 + 0.01 * rng.random((dH, dW)))).astype(np.float32)
    gd_d[5, 9] = 0.0
    f = 30.0
    q = np.array([0.9, 0.1, -0.2, 0.05]) * 1.3
    rots = np.tile(np.float32([1, 0, 0, 0]).reshape(1, 4, 1), (1, 1, 3)); rots[0, :, 2] = q
    trans = np.zeros((1, 3, 3), np.float32); trans[0, :, 2] = [0.3, -0.2, 0.1]
    mask = (rng.random((H0, W0)) > 0.3).astype(np.uint8)
    return {"gt_im": rng.random((3, H0, W0)).astype(np.float32), "gt_depth": gd, "depth_sil": ds,
            "k": np.float32([[f, 0, W0 / 2 - 0.3], [0, f * 1.1, H0 / 2 + 0.2], [0, 0, 1]]),
            "dense": (rng.random((3, dH, dW)).astype(np.float32), gd_d,
                      np.float32([[ratio * f, 0, ratio * W0 / 2], [0, ratio * f * 1.1, ratio * H0 / 2], [0, 0, 1]])),
            "mask": mask, "cam": (rots, trans, 2), "sil_thres": 0.5}


def _expect_info(info, r, overflow=0):
    assert (info["added_ori"], info["added_dense"], info["unexplained"], info["overflow"]) == \
        (r["added_ori"], r["added_dense"], r["unexplained"], overflow)
    assert np.float32(info["median"]) == np.float32(r["median"]) or (info["median"] != info["median"] and r["median"] != r["median"])


def _untouched(before, after, keep_rows=None):
    for key in before:
        assert np.array_equal(before[key], after[key]), key + ": bytes changed"


def test_hand_placed_holes_on_every_chunk_edge(gpu_device, yardstick):
    c = _hand("edges")
    r = restate(c)
    assert r["added_ori"] >= 10 and r["added_dense"] >= 20 and r["unexplained"] > r["added_ori"] - 1
    n, add = 7, r["added_ori"] + r["added_dense"]
    info, got, before, after = run_abi(gpu_device, c, n=n, capacity=n + add)
    _expect_info(info, r)
    _check_rows(yardstick, got, r, n, "33x17 edges")
    assert np.all(got["timestep"][n:n + add] == np.float32(3.0))
    rows = n + add + 3
    for key in before:                                                # rows < n and rows >= n + added keep the poison
        w = before[key].size // rows
        b, a = before[key].reshape(rows, w), after[key].reshape(rows, w)
        assert np.array_equal(b[:n], a[:n]) and np.array_equal(b[n + add:], a[n + add:]), key


def test_hand_placed_no_holes_at_all(gpu_device):
    c = _hand("none")
    r = restate(c)
    assert r["unexplained"] == 0 and r["added_ori"] == 0 and r["added_dense"] == 0 and r["median"] == 0.0
    info, _, before, after = run_abi(gpu_device, c, n=7, capacity=40)
    _expect_info(info, r)
    _untouched(before, after)


def test_hand_placed_every_pixel_a_hole(gpu_device, yardstick):
    c = _hand("all")
    r = restate(c)
    assert r["unexplained"] == W0 * H0 and r["added_ori"] == W0 * H0 - 1          # all but the one invalid-depth pixel
    n, add = 2, r["added_ori"] + r["added_dense"]
    info, got, _, _ = run_abi(gpu_device, c, n=n, capacity=n + add)
    _expect_info(info, r)
    _check_rows(yardstick, got, r, n, "33x17 all holes")


def test_hand_placed_holes_only_where_depth_is_invalid(gpu_device):
    c = _hand("zero_depth", depth_zero_at_holes=True)
    c["depth_sil"][0, 8, 20] = c["gt_depth"][8, 20]                                # no depth-branch pixel in this case
    r = restate(c)
    assert r["unexplained"] == 4 and r["added_ori"] == 0 and r["added_dense"] == 0
    info, _, before, after = run_abi(gpu_device, c, n=7, capacity=40)
    _expect_info(info, r)
    _untouched(before, after)


# ---- capacity ---------------------------------------------------------------------------------------------------------------
def test_capacity_exact_fit_one_short_count_only_and_empty_map(gpu_device, yardstick):
    c = _hand("edges")
    r = restate(c)
    n, add = 11, r["added_ori"] + r["added_dense"]
    info, got, _, _ = run_abi(gpu_device, c, n=n, capacity=n + add)               # fits exactly
    _expect_info(info, r)
    _check_rows(yardstick, got, r, n, "exact fit")
    info, _, before, after = run_abi(gpu_device, c, n=n, capacity=n + add - 1)      # one row short: nothing is written
    _expect_info(info, r, overflow=1)
    _untouched(before, after)
    info, _, before, after = run_abi(gpu_device, c, n=n, capacity=n)                # count-only, form 1
    _expect_info(info, r, overflow=1)
    _untouched(before, after)
    info, _, _, _ = run_abi(gpu_device, c, n=n, null_maps=True)                     # count-only, form 2: NULL maps, capacity 0
    _expect_info(info, r, overflow=1)
    info, got, _, _ = run_abi(gpu_device, c, n=0, capacity=add)                     # an empty map
    _expect_info(info, r)
    _check_rows(yardstick, got, r, 0, "n = 0")
    info, _, _, _ = run_abi(gpu_device, c, n=0, null_maps=True)
    _expect_info(info, r, overflow=1)


# ---- parameter coverage -----------------------------------------------------------------------------------------------------
def test_ratio_one_with_the_same_arrays(gpu_device, yardstick):
    c = _hand("edges")
    c1 = dict(c, dense=(c["gt_im"], c["gt_depth"], c["k"]))
    r = restate(c1)
    assert r["added_dense"] > 0
    n, add = 3, r["added_ori"] + r["added_dense"]
    info, got, _, _ = run_abi(gpu_device, dict(c1, dense="same"), n=n, capacity=n + add)
    _expect_info(info, r)
    _check_rows(yardstick, got, r, n, "ratio 1")


def test_anisotropic_scales_no_timestep_no_mask(gpu_device, yardstick):
    c = dict(_hand("edges"), mask=None)
    r = restate(c)
    n, add = 3, r["added_ori"] + r["added_dense"]
    info, got, _, _ = run_abi(gpu_device, c, n=n, capacity=n + add, scale_columns=3, timestep=False)
    _expect_info(info, r)
    _check_rows(yardstick, got, r, n, "scale_columns 3")
    ls = got["log_scales"][n:n + add]
    assert ls.shape[1] == 3 and np.array_equal(ls[:, 0], ls[:, 1]) and np.array_equal(ls[:, 0], ls[:, 2])


def test_pose_forms_agree_and_calls_repeat_bitwise(gpu_device, yardstick):
    c = _hand("edges")
    rots, trans, t = c["cam"]
    w2c = np.eye(4)
    w2c[:3, :3] = _rot_f64(rots[0, :, t]).numpy()
    w2c[:3, 3] = trans[0, :, t]
    cw = {k: v for k, v in c.items() if k != "cam"}
    cw["w2c"] = w2c.astype(np.float32)
    r = restate(c)
    n, add = 5, r["added_ori"] + r["added_dense"]
    _, a, _, raw_a = run_abi(gpu_device, c, n=n, capacity=n + add)
    _, b, _, raw_b = run_abi(gpu_device, c, n=n, capacity=n + add)
    for key in raw_a:
        assert np.array_equal(raw_a[key], raw_b[key]), key + ": two calls differ"
    _, w, _, _ = run_abi(gpu_device, cw, n=n, capacity=n + add)
    _check_rows(yardstick, w, r, n, "matrix pose form vs float64 (quaternion)")
    assert np.array_equal(a["rgb_colors"], w["rgb_colors"]) and np.array_equal(a["log_scales"], w["log_scales"])
    # the two forms against each other: each is within its allowance of the float64 rows, so within twice that of the other
    mags = r["means3D"]
    assert np.abs(a["means3D"][n:n + add].astype(np.float64) - w["means3D"][n:n + add]).max() <= 2 * _allowed(yardstick, "means3D", mags)
