"""The keyframe-overlap entry points of include/vtgs.h without a GPU: both symbols are exported, the ABI version is still 16,
the scratch size is a pure host function (monotone in `samples`, 0 for invalid sizes), and every malformed call is refused
before any device work (a HIP call on a machine without a GPU would come back as VTGS_ERR_HIP = 4, not as 1)."""
import ctypes
import os

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIB_DIR = os.path.join(ROOT, "vtgaussian-slam_amd", "lib")
INVALID = 1


@pytest.fixture(scope="module")
def kf():
    from diff_gaussian_rasterization import keyframes
    return keyframes


def test_symbols_are_exported():
    lib = ctypes.CDLL(os.path.join(LIB_DIR, "libvtgs.so"))
    for name in ("vtgs_keyframe_overlap_scratch_bytes", "vtgs_keyframe_overlap"):
        assert hasattr(lib, name), name
    lib.vtgs_abi_version.restype = ctypes.c_uint32
    assert lib.vtgs_abi_version() == 16                               # purely additive


def test_scratch_bytes_is_a_pure_host_function(kf):
    f = kf._lib.vtgs_keyframe_overlap_scratch_bytes
    dense = f(1200, 680, 0, 64)
    assert dense >= 64 * 48 and dense % 256 == 0                      # the folded 3x4 rows of the keyframes
    sizes = [f(1200, 680, s, 64) for s in (0, 1, 63, 64, 65, 1600, 16384)]
    assert all(a <= b for a, b in zip(sizes, sizes[1:])) and sizes[1] > sizes[0]       # monotone in samples
    assert sizes[1] - sizes[0] >= 2 * ((1200 * 680 + 31) // 32) * 4                    # two bits per pixel for the repeat rule
    assert f(1200, 680, 0, 4) <= f(1200, 680, 0, 16) <= f(1200, 680, 0, 65) and f(45, 37, 100, 3) < f(1200, 680, 100, 3)
    for bad in ((0, 680, 0, 4), (1200, -1, 0, 4), (1200, 680, -1, 4), (1200, 680, 16385, 4), (1200, 680, 0, 0),
                (1200, 680, 0, -3), (65536, 65536, 0, 4)):
        assert f(*bad) == 0, bad
    assert f(1200, 680, 1600, 64) == f(1200, 680, 1600, 64)


def test_overlap_rejects_malformed_calls_before_any_device_work(kf):
    lib = kf._lib
    buf = (ctypes.c_char * (1 << 20))()
    p = (ctypes.addressof(buf) + 255) & ~255                              # host memory: never dereferenced by a refused call
    for i in range(64):
        buf[(p - ctypes.addressof(buf)) + 2048 + i] = 0x5A
    need_d, need_s = lib.vtgs_keyframe_overlap_scratch_bytes(45, 37, 0, 3), lib.vtgs_keyframe_overlap_scratch_bytes(45, 37, 100, 3)
    good = dict(w=45, h=37, depth=p, k=p + 8192, w2c=p + 8448, rc=None, samples=0, kf_w2c=p + 8704, kf_depth=p + 16384,
                slots=None, n=3, edge=4.0, thresh=0.01, mask=None, scratch=p + 65536, sbytes=need_d, record=p + 2048)
    order = ("w", "h", "depth", "k", "w2c", "rc", "samples", "kf_w2c", "kf_depth", "slots", "n", "edge", "thresh", "mask", "scratch",
             "sbytes", "record")
    call = lambda **kw: lib.vtgs_keyframe_overlap(*[{**good, **kw}[k] for k in order], None)
    sampled = dict(rc=p + 4096, samples=100, sbytes=need_s)
    assert call(w=0) == INVALID and call(h=-2) == INVALID
    assert call(depth=None) == INVALID and call(k=None) == INVALID and call(w2c=None) == INVALID and call(kf_w2c=None) == INVALID
    assert call(n=0) == INVALID and call(n=-1) == INVALID and call(n=(1 << 20) + 1) == INVALID
    assert call(record=None) == INVALID and call(record=p + 2048 + 2) == INVALID             # NULL, not 4-byte aligned
    assert call(scratch=None) == INVALID and call(scratch=p + 65536 + 4) == INVALID          # NULL, not 16-byte aligned
    assert call(sbytes=need_d - 1) == INVALID and call(sbytes=0) == INVALID
    assert call(**{**sampled, "sbytes": need_d}) == INVALID                                  # sampled mode needs the bitmaps
    assert call(**{**sampled, "samples": 16385}) == INVALID and call(**{**sampled, "samples": 0}) == INVALID
    assert call(samples=5) == INVALID and call(**{**sampled, "samples": -1}) == INVALID      # a count without a list
    assert call(edge=-1.0) == INVALID and call(edge=float("nan")) == INVALID and call(edge=float("inf")) == INVALID
    assert bytes(buf[(p - ctypes.addressof(buf)) + 2048:(p - ctypes.addressof(buf)) + 2048 + 64]) == b"\x5a" * 64
