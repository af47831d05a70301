"""Generates tests/golden/densify.npz by running the reference's OWN `add_new_gaussians_base_frame`
(src/vtgaussian_slam.py:732-813, with get_pointcloud :76-128 and initialize_new_params :692-728) and
`initialize_params_base_timestep` (:285-373) in the build container.

    python tests/golden/make_densify_fixtures.py          # needs /root/reference

Like make_get_loss_fixtures.py (whose CPU shim and stand-in modules are reused): the reference file is imported with its
hard-coded 'cuda' device mapped to the CPU, empty stand-ins for the third-party packages it imports and never touches
here, and the float32 CPU ORACLE (oracle/gs_oracle.py) behind `Renderer`.  One stand-in is not empty: `cv2`, whose
`resize(src, (w, h), interpolation=INTER_NEAREST)` is THIS REPOSITORY'S RESTATEMENT of cv2's nearest-neighbour resize for
integer ratios -- source index (x * src_w) // dst_w, likewise y -- which is the rule include/vtgs.h documents for
vtgs_densify; `INTER_NEAREST` is a constant.  cv2 itself is not installed here.

Scene: the 72 x 56 view-tied scene of the get_loss fixtures with a 144 x 112 densification frame, rendered under a MOVED
pose (frame 1), so the image border holds silhouette holes; a block of foreground pixels whose ground-truth depth lies well
in front of the render (the 50 x median branch); invalid-depth pixels and cleared mask_variation pixels inside the holes.
Stored: arrays only -- the inputs, the depth_sil the reference saw, the returned parameter tails and `timestep`, the median,
add_number; for the seed case the parameters initialize_params_base_timestep returned.  No reference source text.
"""
import importlib.util
import os
import sys
import types

import numpy as np
import torch

OUT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, OUT)
import make_get_loss_fixtures as base  # noqa: E402  (CPU shim + stand-in modules; also puts the repository on sys.path)

INTER_NEAREST = 0


def nearest_resize(src, dsize, interpolation=None):
    """The integer nearest rule (see module docstring)."""
    assert interpolation == INTER_NEAREST, "only INTER_NEAREST is restated here"
    dw, dh = int(dsize[0]), int(dsize[1])
    sh, sw = src.shape[:2]
    ys = (np.arange(dh) * sh) // dh
    xs = (np.arange(dw) * sw) // dw
    return np.ascontiguousarray(src[ys][:, xs])


captured = {}


def main():
    if not os.path.isdir(base.REF):
        raise SystemExit("reference not mounted; fixtures can only be generated in the build container")
    sys.dont_write_bytecode = True
    base.install_cpu_shim()
    go = base.install_stand_ins()
    cv2 = types.ModuleType("cv2")
    cv2.resize, cv2.INTER_NEAREST = nearest_resize, INTER_NEAREST
    sys.modules["cv2"] = cv2

    class Renderer:
        """The operator boundary: (color, radii, depth) from the float32 oracle; the image is recorded."""

        def __init__(self, raster_settings):
            self.cam = raster_settings

        def __call__(self, means3D, means2D, opacities, colors_precomp, scales, rotations):
            color, radii, depth = go.rasterize(means3D, means2D, opacities, colors_precomp, scales, rotations, self.cam)
            captured["depth_sil"] = color.detach().clone()
            return color, radii, depth
    sys.modules["diff_gaussian_rasterization"].GaussianRasterizer = Renderer
    sys.path.insert(0, base.REF)
    sys.path.insert(0, os.path.join(base.REF, "src"))
    spec = importlib.util.spec_from_file_location("ref_vtgaussian_slam", os.path.join(base.REF, "src", "vtgaussian_slam.py"))
    ref = importlib.util.module_from_spec(spec)
    saved_argv, sys.argv = sys.argv, ["vtgaussian_slam.py"]
    try:
        spec.loader.exec_module(ref)
    finally:
        sys.argv = saved_argv

    W, H, F, R = 72, 56, 60.0, 2
    dW, dH = R * W, R * H
    g = torch.Generator().manual_seed(20251021)
    k = torch.tensor([[F, 0, W / 2 - 0.5], [0, F, H / 2 - 0.5], [0, 0, 1.0]])
    k_d = torch.tensor([[R * F, 0, R * (W / 2 - 0.5) + 0.5], [0, R * F, R * (H / 2 - 0.5) + 0.5], [0, 0, 1.0]])
    first_w2c = torch.eye(4)
    cam = go.setup_camera(W, H, k.numpy(), first_w2c.numpy())
    scene, _ = go.view_tied_scene(2600, W, H, seed=7, z_range=(1.5, 4.0))
    n = scene["means3D"].shape[0]
    T, t_idx = 3, 1
    rots = torch.tensor([1.0, 0, 0, 0]).reshape(1, 4, 1).repeat(1, 1, T)
    rots[0, :, t_idx] = torch.tensor([0.995, 0.03, -0.05, 0.02]) * 1.7          # un-normalised on purpose
    trans = torch.zeros(1, 3, T)
    trans[0, :, t_idx] = torch.tensor([0.35, -0.22, 0.08])

    def fresh_params():
        gg = torch.Generator().manual_seed(99)
        logit = torch.logit(scene["opacities"] * 0.0 + 0.93) + 0.8 * torch.randn(n, 1, generator=gg)
        m3 = scene["means3D"]
        unmapped = (m3[:, 0] / m3[:, 2] > 0.25) & (m3[:, 1] / m3[:, 2] < 0.05)      # a part of the view the map does not hold yet
        logit[unmapped] = -12.0
        return {
            "means3D": torch.nn.Parameter(scene["means3D"].clone()),
            "rgb_colors": torch.nn.Parameter(scene["colors_precomp"].clone()),
            "unnorm_rotations": torch.nn.Parameter(torch.tensor([[1.0, 0, 0, 0]]).repeat(n, 1)),
            "logit_opacities": torch.nn.Parameter(logit),
            "log_scales": torch.nn.Parameter(torch.log(scene["scales"][:, :1] * 1.6)),
            "cam_unnorm_rots": torch.nn.Parameter(rots.clone()),
            "cam_trans": torch.nn.Parameter(trans.clone()),
        }

    # ground truth of frame 1: the map's own depth under the moved pose + noise where it is covered, a far wall elsewhere
    with torch.no_grad():
        p0 = fresh_params()
        tg = ref.transform_to_frame(p0, t_idx, gaussians_grad=False, camera_grad=False)
        rv = ref.transformed_params2depthplussilhouette(p0, first_w2c, tg)
        ds0, _, _ = go.rasterize(cam=cam, **rv)
    covered = ds0[1] > 0.5
    gt_depth = torch.where(covered, ds0[0] / ds0[1].clamp(min=1e-6), torch.full((H, W), 2.75))
    gt_depth = (gt_depth + 0.004 * torch.randn(H, W, generator=g))[None].contiguous()
    gt_depth[:, 20:25, 30:36] = 0.4                              # foreground object well in front of the render
    gt_depth[:, :5, :11] = 0.0                                   # invalid depth (inside the holes and elsewhere)
    gt_depth[:, 10:14, 58:66] = 0.0
    gt_depth[:, 40:44, 60:] = 0.0
    quant = lambda x: torch.round(x.clamp(0, 1) * 255) / 255     # 8-bit colours, as a dataset holds them
    gt_im = quant(torch.rand(3, H, W, generator=g))
    up = lambda x: x.repeat_interleave(R, -2).repeat_interleave(R, -1)
    gt_im_d = quant(up(gt_im) + 0.1 * torch.rand(3, dH, dW, generator=g))
    gt_depth_d = (up(gt_depth) * (1 + 0.002 * torch.randn(1, dH, dW, generator=g))).contiguous()
    gt_depth_d[:, 70:80, 20:44] = 0.0
    mask_variation = (torch.rand(H, W, generator=g) > 0.35).numpy().astype(np.uint8)       # at the original resolution
    sil_thres = 0.5

    ori = {"cam": cam, "im": gt_im.clone(), "depth": gt_depth.clone(), "id": t_idx, "intrinsics": k.clone(), "w2c": first_w2c.clone()}
    dense = {"cam": None, "im": gt_im_d.clone(), "depth": gt_depth_d.clone(), "id": t_idx, "intrinsics": k_d.clone(),
             "w2c": first_w2c.clone()}
    params = fresh_params()
    variables = {"max_2D_radius": torch.ones(n), "means2D_gradient_accum": torch.ones(n), "denom": torch.ones(n),
                 "timestep": torch.zeros(n)}
    params, variables, add_number = ref.add_new_gaussians_base_frame(params, variables, ori, dense, sil_thres, t_idx, "projective",
                                                                     "isotropic", {}, mask_variation=mask_variation.copy())
    ds = captured["depth_sil"]
    # ---- the fixture must not be vacuous (restated here only to COUNT what the reference selected)
    rd, sil, gd = ds[0], ds[1], gt_depth[0]
    err = (gd - rd).abs() * (gd > 0)
    med = err.median()
    hole = sil < sil_thres
    branch = (rd > gd) & (err > 50 * med)
    unexpl = hole | branch
    n_ori = int((unexpl & (gd > 0)).sum())
    n_hole, n_branch = int((hole & (gd > 0)).sum()), int((branch & ~hole & (gd > 0)).sum())
    n_dense = add_number - n_ori
    un_d = torch.from_numpy(nearest_resize(unexpl.numpy().astype(np.uint8), (dW, dH), INTER_NEAREST)).bool()
    mv_d = torch.from_numpy(nearest_resize(mask_variation, (dW, dH), INTER_NEAREST)).bool()
    assert n_dense == int((un_d & mv_d & (gt_depth_d[0] > 0)).sum()), "the counting restatement disagrees with the reference"
    assert n_hole >= 50 and n_branch >= 20 and n_dense >= 50, (n_hole, n_branch, n_dense)
    assert int((unexpl & (gd == 0)).sum()) >= 1 and int((unexpl & torch.from_numpy(mask_variation == 0)).sum()) >= 1
    assert int((un_d & (gt_depth_d[0] == 0)).sum()) >= 1 and int((un_d & ~mv_d).sum()) >= 1
    assert 0 < float(med) < 0.02 and params["means3D"].shape[0] == n + add_number
    print("frame case: add_number", add_number, "ori", n_ori, "(holes", n_hole, "depth branch", n_branch, ") dense", n_dense,
          "median", float(med))
    fp = fresh_params()
    store = {"W": np.int64(W), "H": np.int64(H), "dW": np.int64(dW), "dH": np.int64(dH), "t_idx": np.int64(t_idx),
             "sil_thres": np.float64(sil_thres), "intrinsics": k.numpy(), "intrinsics_dense": k_d.numpy(),
             "first_w2c": first_w2c.numpy(), "gt_im": gt_im.numpy(), "gt_depth": gt_depth.numpy(), "gt_im_dense": gt_im_d.numpy(),
             "gt_depth_dense": gt_depth_d.numpy(), "mask_variation": mask_variation,
             "frame_depth_sil": ds.numpy(), "frame_median": np.float32(med.item()), "frame_add_number": np.int64(add_number),
             "frame_added_ori": np.int64(n_ori), "frame_unexplained": np.int64(int(unexpl.sum())),
             "frame_timestep": variables["timestep"].numpy(),
             **{"map_" + kk: vv.detach().numpy() for kk, vv in fp.items()},
             **{"frame_tail_" + kk: params[kk].detach().numpy()[n:] for kk in ("means3D", "rgb_colors", "unnorm_rotations",
                                                                              "logit_opacities", "log_scales")}}
    for kk in ("means3D", "rgb_colors", "unnorm_rotations", "logit_opacities", "log_scales"):
        assert np.array_equal(params[kk].detach().numpy()[:n], fp[kk].detach().numpy()), kk
    assert all(float(variables[kk].abs().sum()) == 0 and variables[kk].numel() == n + add_number
               for kk in ("max_2D_radius", "means2D_gradient_accum", "denom"))

    # ---- seed case: initialize_params_base_timestep with a rigid w2c and a SPARSE mask at the dense resolution (ratio 1)
    from utils.slam_external import build_rotation
    w2c = torch.eye(4)
    w2c[:3, :3] = build_rotation(torch.nn.functional.normalize(rots[..., t_idx]))[0]
    w2c[:3, 3] = trans[0, :, t_idx]
    seed_mask = (torch.rand(dH, dW, generator=g) > 0.85).numpy().astype(np.uint8)
    k4, k4_d = torch.eye(4), torch.eye(4)
    k4[:3, :3], k4_d[:3, :3] = k, k_d

    class Frames:
        def __init__(self, im, depth, intr):
            self.item = (im.permute(1, 2, 0) * 255, depth.permute(1, 2, 0).clone(), intr, torch.eye(4))

        def __getitem__(self, i):
            return self.item
    sp, sv = ref.initialize_params_base_timestep(Frames(gt_im, gt_depth, k4), T, t_idx, w2c, 3.0, "projective",
                                                 densify_dataset=Frames(gt_im_d, gt_depth_d, k4_d),
                                                 gaussian_distribution="isotropic", mask_variation=seed_mask.copy())
    m_ori = int((gt_depth[0] > 0).sum())
    m_all = sp["means3D"].shape[0]
    assert m_all - m_ori == int(((gt_depth_d[0] > 0) & torch.from_numpy(seed_mask).bool()).sum()) and m_all - m_ori >= 50
    print("seed case: points", m_all, "ori", m_ori, "dense", m_all - m_ori)
    store.update(seed_w2c=w2c.numpy(), seed_mask=seed_mask, seed_added_ori=np.int64(m_ori),
                 seed_color=(gt_im.permute(1, 2, 0) * 255).permute(2, 0, 1).div(255).numpy(),
                 seed_color_dense=(gt_im_d.permute(1, 2, 0) * 255).permute(2, 0, 1).div(255).numpy(),
                 **{"seed_" + kk: sp[kk].detach().numpy() for kk in ("means3D", "rgb_colors", "unnorm_rotations", "logit_opacities",
                                                                    "log_scales")})
    path = os.path.join(OUT, "densify.npz")
    np.savez_compressed(path, **store)
    print("wrote densify.npz", os.path.getsize(path), "bytes,", len(store), "arrays")
    assert os.path.getsize(path) < 1 << 20


if __name__ == "__main__":
    main()
