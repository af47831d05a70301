"""Densification on the device (csrc/vtgs_densify.hip): the step of the SLAM loop that makes the map grow.

    params, variables, add_number = add_new_gaussians_base_frame(params, variables, ori_curr_data, densify_curr_data, sil_thres,
                                                                 time_idx, mean_sq_dist_method, gaussian_distribution, config,
                                                                 mask_variation=mask_variation)

has the signature and the return tuple of the reference's function (src/vtgaussian_slam.py:732-813) and replaces it together
with `get_pointcloud` (:76-128) and `initialize_new_params` (:692-728): no cv2, no mask on the host, one host read (the
counts).  `initialize_new_points` is the point cloud of `initialize_params_base_timestep` (:302-340), `densify_into` the
resident form for a caller that keeps slack rows in its map arrays, `lower_median` torch.median of a flat float32 tensor
without a host wait.  HIP only: no CPU path.
"""
from __future__ import annotations

import ctypes

import numpy as np
import torch

from . import _I32, _P, _SZ, _check, _lib, _stream_ptr

__all__ = ["lower_median", "densify_into", "read_info", "add_new_gaussians_base_frame", "initialize_new_points"]


class _VtgsDensifyInfo(ctypes.Structure):
    _fields_ = [("added_ori", ctypes.c_uint32), ("added_dense", ctypes.c_uint32), ("unexplained", ctypes.c_uint32),
                ("overflow", ctypes.c_uint32), ("median", ctypes.c_float), ("nan_count", ctypes.c_uint32),
                ("complete", ctypes.c_uint32), ("pad", ctypes.c_uint32)]


_F = ctypes.c_float
_lib.vtgs_median_scratch_bytes.restype, _lib.vtgs_median_scratch_bytes.argtypes = _SZ, [ctypes.c_int64]
_lib.vtgs_lower_median.restype = ctypes.c_int
_lib.vtgs_lower_median.argtypes = [_P, ctypes.c_int64, _P, _SZ, _P, _P, _P]
_lib.vtgs_densify_scratch_bytes.restype, _lib.vtgs_densify_scratch_bytes.argtypes = _SZ, [_I32] * 4
_lib.vtgs_densify.restype = ctypes.c_int
_lib.vtgs_densify.argtypes = ([_I32, _I32, _P, _P, _P, _P, _I32, _I32, _P, _P, _P, _P, _I32, _I32, _P, _P, _P, _I32, _I32, _F, _F,
                               _I32, _I32, _I32] + [_P] * 6 + [_P, _SZ, _P, _P])

_MAP_KEYS = ("means3D", "rgb_colors", "unnorm_rotations", "logit_opacities", "log_scales")


def _need_device(t, what):
    if not isinstance(t, torch.Tensor) or not t.is_cuda:
        raise RuntimeError(f"{what} needs tensors on a HIP device (torch 'cuda'); no CPU path exists")


def _f32(t, dev):
    return t.detach().to(device=dev, dtype=torch.float32).contiguous()


def lower_median(x: torch.Tensor, return_nan_count: bool = False):
    """torch.median(x.flatten()) -- the element of rank (n - 1) // 2, NaN if any element is NaN or x is empty -- as a 0-dim
    device tensor, exact, with no host wait.  `return_nan_count`: also the number of NaNs (0-dim int32 device tensor)."""
    _need_device(x, "lower_median")
    v = _f32(x, x.device).reshape(-1)
    n = v.numel()
    sbytes = int(_lib.vtgs_median_scratch_bytes(n))
    scratch = torch.empty(sbytes, dtype=torch.uint8, device=x.device)
    out = torch.empty(2, dtype=torch.float32, device=x.device)
    _check(_lib.vtgs_lower_median(v.data_ptr() if n else None, n, scratch.data_ptr(), sbytes, out.data_ptr(),
                                  out.data_ptr() + 4, _stream_ptr(x.device)), "vtgs_lower_median")
    return (out[0], out[1].view(torch.int32)) if return_nan_count else out[0]


def read_info(record: torch.Tensor) -> dict:
    """The device record of densify_into as a dict -- a HOST READ (waits for the stream)."""
    raw = record.cpu().numpy().tobytes()
    info = _VtgsDensifyInfo.from_buffer_copy(raw)
    return {k: getattr(info, k) for k, _ in _VtgsDensifyInfo._fields_ if k != "pad"}


def _mask_u8(mask_variation, dev):
    if mask_variation is None:
        return None
    if isinstance(mask_variation, torch.Tensor):
        m = mask_variation.detach().to(device=dev)
        m = (m != 0).to(torch.uint8) if m.dtype != torch.uint8 else m
    else:
        m = torch.from_numpy(np.ascontiguousarray(np.asarray(mask_variation) != 0).astype(np.uint8)).to(dev)
    if m.dim() != 2:
        raise ValueError("mask_variation must be a 2-D [h, w] array")
    return m.contiguous()


def densify_into(map_arrays, n: int, capacity: int, *, gt_im, gt_depth, intrinsics, depth_sil=None, dense=None,
                 mask_variation=None, w2c=None, cam=None, sil_thres: float = 0.5, time_idx_value: float = 0.0,
                 scale_columns: int = None) -> torch.Tensor:
    """vtgs_densify (include/vtgs.h) on the current stream.  `map_arrays`: dict of the five parameter arrays (+ optionally
    'timestep'), contiguous float32 device tensors of at least `capacity` rows whose rows [n, capacity) are free -- or None
    with capacity = 0 for a count-only call.  `dense` = (gt_im_dense, gt_depth_dense, intrinsics_dense) or None;
    pose: `w2c` [4,4] (rigid) or `cam` = (cam_unnorm_rots [1,4,T], cam_trans [1,3,T], t); `depth_sil` None = seed mode.
    Returns the 32-byte device record (int32 [8]); read_info() reads it when the caller wants the counts."""
    _need_device(gt_depth, "densify_into")
    dev = gt_depth.device
    im, gd = _f32(gt_im, dev), _f32(gt_depth, dev)
    H, W = gd.shape[-2], gd.shape[-1]
    if gd.numel() != H * W or im.numel() != 3 * H * W:
        raise ValueError("gt_im must be [3,H,W] and gt_depth [H,W] / [1,H,W]")
    k = _f32(intrinsics, dev)[:3, :3].contiguous()
    ds = None
    if depth_sil is not None:
        ds = _f32(depth_sil, dev)
        if ds.numel() != 3 * H * W:
            raise ValueError("depth_sil must be [3,H,W]")
    dW = dH = mW = mH = 0
    im_d = gd_d = k_d = m = None
    if dense is not None:
        im_d, gd_d, k_d = _f32(dense[0], dev), _f32(dense[1], dev), _f32(dense[2], dev)[:3, :3].contiguous()
        dH, dW = gd_d.shape[-2], gd_d.shape[-1]
        if gd_d.numel() != dH * dW or im_d.numel() != 3 * dH * dW:
            raise ValueError("the dense image must be [3,h,w] and its depth [h,w] / [1,h,w]")
        m = _mask_u8(mask_variation, dev)
        if m is not None:
            mH, mW = m.shape
    if (w2c is None) == (cam is None):
        raise ValueError("exactly one of w2c and cam must be given")
    w, rots, trans, frames, t = None, None, None, 0, 0
    if w2c is not None:
        w = _f32(w2c, dev).reshape(16)
    else:
        rots, trans, t = _f32(cam[0], dev), _f32(cam[1], dev), int(cam[2])
        frames = rots.shape[-1]
        if rots.numel() != 4 * frames or trans.numel() != 3 * frames:
            raise ValueError("cam tensors must be [1,4,T] and [1,3,T]")
    ptrs = [None] * 6
    if map_arrays is not None:
        for i, key in enumerate(_MAP_KEYS + ("timestep",)):
            a = map_arrays.get(key)
            if a is None:
                if key != "timestep":
                    raise ValueError(f"map_arrays lacks {key!r}")
                continue
            if not (a.is_cuda and a.dtype == torch.float32 and a.is_contiguous() and a.shape[0] >= capacity):
                raise ValueError(f"map_arrays[{key!r}] must be a contiguous float32 device tensor of >= capacity rows")
            ptrs[i] = a.data_ptr()
        cols = map_arrays["log_scales"].shape[1] if map_arrays["log_scales"].dim() == 2 else 1
        if scale_columns is not None and scale_columns != cols:
            raise ValueError("scale_columns does not match map_arrays['log_scales']")
        scale_columns = cols
    elif capacity != 0:
        raise ValueError("a call without map arrays is count-only: capacity must be 0")
    if scale_columns is None:
        scale_columns = 1
    sbytes = int(_lib.vtgs_densify_scratch_bytes(W, H, dW, dH))
    if sbytes == 0:
        raise ValueError(f"densify: a {dW}x{dH} dense frame is no integer multiple of the {W}x{H} frame")
    scratch = torch.empty(sbytes, dtype=torch.uint8, device=dev)
    record = torch.empty(8, dtype=torch.int32, device=dev)
    p = lambda x: None if x is None else x.data_ptr()
    _check(_lib.vtgs_densify(W, H, p(ds), im.data_ptr(), gd.data_ptr(), k.data_ptr(), dW, dH, p(im_d), p(gd_d), p(k_d), p(m), mW, mH,
                             p(w), p(rots), p(trans), frames, t, float(sil_thres), float(time_idx_value), int(scale_columns),
                             int(n), int(capacity), *ptrs, scratch.data_ptr(), sbytes, record.data_ptr(), _stream_ptr(dev)),
           "vtgs_densify")
    return record


def _grow(arrays: dict, n: int, added: int, dev) -> dict:
    """n + added rows per array: the old rows copied, the tail left for the emit call."""
    out = {}
    for key, a in arrays.items():
        new = torch.empty((n + added,) + tuple(a.shape[1:]), dtype=torch.float32, device=dev)
        new[:n].copy_(a.detach())
        out[key] = new
    return out


def add_new_gaussians_base_frame(params, variables, ori_curr_data, densify_curr_data, sil_thres, time_idx, mean_sq_dist_method,
                                 gaussian_distribution, config, mask_variation=None):
    """The reference's function (src/vtgaussian_slam.py:732-813): a forward-only [z,1,z^2] render under the pose of frame
    `time_idx`, the non-presence mask, the new Gaussians of both resolutions appended to `params`, `variables` reset /
    extended as at :803-808.  Returns (params, variables, add_number)."""
    from .fused import render_frame
    if mean_sq_dist_method != "projective":
        raise ValueError(f"Unknown mean_sq_dist_method {mean_sq_dist_method}")
    if gaussian_distribution not in ("isotropic", "anisotropic"):
        raise ValueError(f"Unknown gaussian_distribution {gaussian_distribution}")
    cols = 1 if gaussian_distribution == "isotropic" else 3
    for k, v in params.items():
        if isinstance(v, torch.Tensor):
            params[k] = v.cuda()
    for k, v in variables.items():
        if isinstance(v, torch.Tensor):
            variables[k] = v.cuda()
    dev = params["means3D"].device
    if params["log_scales"].shape[1] != cols:
        raise ValueError(f"gaussian_distribution={gaussian_distribution!r} but log_scales has {params['log_scales'].shape[1]} column(s)")
    with torch.no_grad():
        _im, depth_sil, _radii = render_frame(params, time_idx, ori_curr_data["cam"], ori_curr_data["w2c"], False, False)
    n = params["means3D"].shape[0]
    kw = dict(gt_im=ori_curr_data["im"], gt_depth=ori_curr_data["depth"], intrinsics=ori_curr_data["intrinsics"],
              depth_sil=depth_sil.detach(),
              dense=(densify_curr_data["im"], densify_curr_data["depth"], densify_curr_data["intrinsics"]),
              mask_variation=_mask_u8(mask_variation, dev),
              cam=(params["cam_unnorm_rots"], params["cam_trans"], int(time_idx)), sil_thres=float(sil_thres),
              time_idx_value=float(time_idx), scale_columns=cols)
    info = read_info(densify_into(None, n, 0, **kw))                     # count only; the one host read of the step
    if info["unexplained"] == 0:                                         # :810-811
        return params, variables, 0
    added = info["added_ori"] + info["added_dense"]
    arrays = _grow({k: params[k] for k in _MAP_KEYS}, n, added, dev)
    arrays["timestep"] = _grow({"timestep": variables["timestep"].float()}, n, added, dev)["timestep"]
    if added:
        densify_into(arrays, n, n + added, **kw)
    for k in _MAP_KEYS:
        params[k] = torch.nn.Parameter(arrays[k].requires_grad_(True))
    num_pts = n + added
    variables["means2D_gradient_accum"] = torch.zeros(num_pts, device=dev).float()
    variables["denom"] = torch.zeros(num_pts, device=dev).float()
    variables["max_2D_radius"] = torch.zeros(num_pts, device=dev).float()
    variables["timestep"] = arrays["timestep"]
    return params, variables, added


def initialize_new_points(color, depth, intrinsics, w2c, dense_color=None, dense_depth=None, dense_intrinsics=None,
                          mask_variation=None):
    """Seed mode: the point cloud of initialize_params_base_timestep / _first_timestep (src/vtgaussian_slam.py:302-340) --
    every valid-depth pixel of the original image, then every valid-depth pixel of the densification image that
    `mask_variation` keeps.  Returns (init_pt_cld [M,6] = world point | colour, mean3_sq_dist [M]) for `initialize_params`
    (mean3_sq_dist = exp(log scale)^2: within two float32 roundings of the reference's (z / f)^2)."""
    _need_device(depth, "initialize_new_points")
    dev = depth.device
    dense = None if dense_depth is None else (dense_color, dense_depth, dense_intrinsics)
    kw = dict(gt_im=color, gt_depth=depth, intrinsics=intrinsics, dense=dense, mask_variation=mask_variation, w2c=w2c)
    info = read_info(densify_into(None, 0, 0, **kw))
    m = info["added_ori"] + info["added_dense"]
    arrays = {"means3D": torch.empty(m, 3, device=dev), "rgb_colors": torch.empty(m, 3, device=dev),
              "unnorm_rotations": torch.empty(m, 4, device=dev), "logit_opacities": torch.empty(m, 1, device=dev),
              "log_scales": torch.empty(m, 1, device=dev)}
    if m:
        densify_into(arrays, 0, m, **kw)
    return torch.cat((arrays["means3D"], arrays["rgb_colors"]), 1), torch.exp(arrays["log_scales"][:, 0]) ** 2
