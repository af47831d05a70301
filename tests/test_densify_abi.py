"""The densification entry points of include/vtgs.h without a GPU: the symbols are exported, the device record is 32 bytes in
C and in the ctypes mirror, the scratch sizes follow the documented layout, and every malformed call is refused before any
device work (a HIP call on a machine without a GPU would come back as VTGS_ERR_HIP = 4, not as 1 / 2)."""
import ctypes
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIB_DIR = os.path.join(ROOT, "vtgaussian-slam_amd", "lib")
INVALID, TOO_SMALL = 1, 2


@pytest.fixture(scope="module")
def dz():
    from diff_gaussian_rasterization import densify
    return densify


def test_symbols_are_exported():
    lib = ctypes.CDLL(os.path.join(LIB_DIR, "libvtgs.so"))
    for name in ("vtgs_median_scratch_bytes", "vtgs_lower_median", "vtgs_densify_scratch_bytes", "vtgs_densify"):
        assert hasattr(lib, name), name
    lib.vtgs_abi_version.restype = ctypes.c_uint32
    assert lib.vtgs_abi_version() == 16                               # purely additive


def test_record_is_32_bytes_in_c_and_in_the_mirror(tmp_path, dz):
    src = tmp_path / "rec.c"
    src.write_text('#include "vtgs.h"\n#include <stddef.h>\n#include <stdio.h>\n'
                   'int main(void) { printf("%u %u %u %u\\n", (unsigned)sizeof(VtgsDensifyInfo), (unsigned)offsetof(VtgsDensifyInfo, median), '
                   '(unsigned)offsetof(VtgsDensifyInfo, complete), (unsigned)vtgs_median_scratch_bytes(10)); return 0; }\n')
    exe = tmp_path / "rec"
    subprocess.run(["gcc", "-std=c99", "-Wall", "-Wextra", "-pedantic", "-Werror", "-I", os.path.join(ROOT, "include"), str(src),
                    "-L", LIB_DIR, "-lvtgs", "-Wl,-rpath," + LIB_DIR, "-Wl,-rpath,/opt/rocm/lib", "-o", str(exe)], check=True)
    out = [int(x) for x in subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.split()]
    assert out[:3] == [32, 16, 24]
    assert ctypes.sizeof(dz._VtgsDensifyInfo) == 32 and dz._VtgsDensifyInfo.median.offset == 16
    assert dz._VtgsDensifyInfo.complete.offset == 24
    assert out[3] == dz._lib.vtgs_median_scratch_bytes(10)


def test_scratch_sizes(dz):
    lib = dz._lib
    m = lib.vtgs_median_scratch_bytes(1000)
    assert m >= (2048 + 2048 + 1024) * 4 and m % 256 == 0              # three histograms: 11 + 11 + 10 key bits
    assert lib.vtgs_median_scratch_bytes(0) == m and lib.vtgs_median_scratch_bytes(-1) == 0
    assert lib.vtgs_median_scratch_bytes(1 << 32) == 0 and lib.vtgs_median_scratch_bytes((1 << 32) - 1) == m
    a = lib.vtgs_densify_scratch_bytes(72, 56, 0, 0)
    b = lib.vtgs_densify_scratch_bytes(72, 56, 144, 112)
    c = lib.vtgs_densify_scratch_bytes(1200, 680, 2400, 1360)
    assert m < a <= b < c and c < (1 << 20)                              # counts per chunk of pixels: kilobytes, not images
    assert lib.vtgs_densify_scratch_bytes(72, 56, 100, 112) == 0         # not an integer ratio
    assert lib.vtgs_densify_scratch_bytes(72, 56, 144, 100) == 0
    assert lib.vtgs_densify_scratch_bytes(72, 56, 144, 0) == 0 and lib.vtgs_densify_scratch_bytes(0, 56, 0, 0) == 0
    assert lib.vtgs_densify_scratch_bytes(72, -1, 0, 0) == 0 and lib.vtgs_densify_scratch_bytes(72, 56, 36, 28) == 0


def test_lower_median_rejects_malformed_calls_before_any_device_work(dz):
    lib = dz._lib
    buf = (ctypes.c_char * 65536)()
    p = (ctypes.addressof(buf) + 255) & ~255                              # host memory: never dereferenced by a refused call
    need = lib.vtgs_median_scratch_bytes(100)
    good = dict(values=p, n=100, scratch=p + 4096, scratch_bytes=need, out=p + 1024, nan=None)
    call = lambda **kw: lib.vtgs_lower_median(*[{**good, **kw}[k] for k in ("values", "n", "scratch", "scratch_bytes", "out", "nan")], None)
    assert call(values=None) == INVALID
    assert call(n=-1) == INVALID and call(n=1 << 32) == INVALID
    assert call(scratch=None) == INVALID and call(scratch=p + 4096 + 4) == INVALID      # NULL, not 16-byte aligned
    assert call(out=None) == INVALID
    assert call(scratch_bytes=need - 1) == TOO_SMALL and call(scratch_bytes=0) == TOO_SMALL


def test_densify_rejects_malformed_calls_before_any_device_work(dz):
    lib = dz._lib
    buf = (ctypes.c_char * 65536)()
    p = (ctypes.addressof(buf) + 255) & ~255
    need = lib.vtgs_densify_scratch_bytes(72, 56, 144, 112)
    names = ("width", "height", "depth_sil", "gt_im", "gt_depth", "intrinsics", "dense_width", "dense_height", "gt_im_dense",
             "gt_depth_dense", "intrinsics_dense", "mask_variation", "mask_width", "mask_height", "w2c", "cam_unnorm_rots",
             "cam_trans", "frames", "t", "sil_thres", "time_idx_value", "scale_columns", "n", "capacity", "means3D", "rgb_colors",
             "unnorm_rotations", "logit_opacities", "log_scales", "timestep", "scratch", "scratch_bytes", "info", "stream")
    good = dict(width=72, height=56, depth_sil=p, gt_im=p, gt_depth=p, intrinsics=p, dense_width=144, dense_height=112,
                gt_im_dense=p, gt_depth_dense=p, intrinsics_dense=p, mask_variation=p, mask_width=72, mask_height=56, w2c=p,
                cam_unnorm_rots=None, cam_trans=None, frames=0, t=0, sil_thres=0.5, time_idx_value=1.0, scale_columns=1, n=10,
                capacity=20, means3D=p, rgb_colors=p, unnorm_rotations=p, logit_opacities=p, log_scales=p, timestep=None,
                scratch=p + 4096, scratch_bytes=need, info=p + 2048, stream=None)
    call = lambda **kw: lib.vtgs_densify(*[{**good, **kw}[k] for k in names])
    quat = dict(w2c=None, cam_unnorm_rots=p, cam_trans=p, frames=3, t=1)
    # null and invalid arguments
    for kw in (dict(width=0), dict(height=-3), dict(gt_im=None), dict(gt_depth=None), dict(intrinsics=None), dict(scratch=None),
               dict(scratch=p + 4096 + 8), dict(info=None), dict(n=-1), dict(capacity=-1), dict(means3D=None), dict(rgb_colors=None),
               dict(unnorm_rotations=None), dict(logit_opacities=None), dict(log_scales=None),
               dict(gt_im_dense=None), dict(gt_depth_dense=None), dict(intrinsics_dense=None), dict(dense_height=0),
               dict(mask_width=0), dict(mask_height=-1)):
        assert call(**kw) == INVALID, kw
    # pose: both forms, neither, a half quaternion form, a frame index outside the tensors
    assert call(cam_unnorm_rots=p, cam_trans=p, frames=3, t=1) == INVALID
    assert call(w2c=None) == INVALID
    for kw in (dict(cam_trans=None), dict(cam_unnorm_rots=None), dict(frames=0), dict(t=3), dict(t=-1)):
        assert call(**{**quat, **kw}) == INVALID, kw
    # a non-integer dense ratio, a mask the dense frame is no multiple of
    for kw in (dict(dense_width=100), dict(dense_height=100), dict(dense_width=36, dense_height=28), dict(mask_width=50),
               dict(mask_height=50), dict(mask_width=288, mask_height=224)):
        assert call(**kw) == INVALID, kw
    for sc in (0, 2, 4, -1):
        assert call(scale_columns=sc) == INVALID, sc
    assert call(scratch_bytes=need - 1) == TOO_SMALL and call(scratch_bytes=0) == TOO_SMALL
    assert call(**quat, scratch_bytes=need - 1) == TOO_SMALL               # (the quaternion form passes the pose checks)
    # NULL map pointers are the count-only form -- but only together with capacity = 0
    assert call(capacity=0, means3D=None, rgb_colors=None, unnorm_rotations=None, logit_opacities=None, log_scales=None,
                scratch_bytes=0) == TOO_SMALL                              # (accepted up to the scratch check)


def test_python_operators_refuse_cpu_tensors(dz):
    import torch
    with pytest.raises(RuntimeError, match="no CPU path"):
        dz.lower_median(torch.rand(8))
    with pytest.raises(RuntimeError, match="no CPU path"):
        dz.densify_into(None, 0, 0, gt_im=torch.rand(3, 4, 4), gt_depth=torch.rand(4, 4), intrinsics=torch.eye(3), w2c=torch.eye(4))
    with pytest.raises(RuntimeError, match="no CPU path"):
        dz.initialize_new_points(torch.rand(3, 4, 4), torch.rand(1, 4, 4), torch.eye(3), torch.eye(4))
