"""The tracking-mask entry points of include/vtgs.h without a GPU: both symbols are exported, the ABI version is still 16,
the scratch size is a pure host function (0 for invalid sizes, growing with the overlaps and with the outlier mask), and
every malformed call is refused before any device work (a HIP call on a machine without a GPU would come back as
VTGS_ERR_HIP = 4, not as 1)."""
import ctypes
import os

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIB_DIR = os.path.join(ROOT, "vtgaussian-slam_amd", "lib")
INVALID = 1


@pytest.fixture(scope="module")
def lib():
    from diff_gaussian_rasterization import losses
    return losses._lib


def test_symbols_are_exported():
    lib = ctypes.CDLL(os.path.join(LIB_DIR, "libvtgs.so"))
    for name in ("vtgs_tracking_mask_scratch_bytes", "vtgs_tracking_mask"):
        assert hasattr(lib, name), name
    lib.vtgs_abi_version.restype = ctypes.c_uint32
    assert lib.vtgs_abi_version() == 16                               # purely additive


def test_scratch_bytes_is_a_pure_host_function(lib):
    f = lib.vtgs_tracking_mask_scratch_bytes
    plain = [f(1200, 680, n, 0) for n in range(4)]
    assert plain[0] < plain[1] <= plain[2] <= plain[3] and plain[1] >= 64          # the folded 64-byte rows
    assert all(b % 256 == 0 for b in plain)
    for n in range(4):
        with_outlier = f(1200, 680, n, 1)
        assert with_outlier - plain[n] >= 1200 * 680 * 4 + (2048 + 2048 + 1024) * 4    # err + the select's histograms
        assert with_outlier % 256 == 0
    assert f(45, 37, 3, 1) < f(1200, 680, 3, 1) and f(45, 37, 3, 0) == f(1200, 680, 3, 0)
    for bad in ((0, 680, 1, 0), (1200, -1, 1, 0), (1200, 680, -1, 0), (1200, 680, 4, 0), (1200, 680, 1, 2), (1200, 680, 1, -1),
                (65536, 65536, 1, 0)):
        assert f(*bad) == 0, bad
    assert f(1200, 680, 3, 1) == f(1200, 680, 3, 1)


def test_mask_rejects_malformed_calls_before_any_device_work(lib):
    buf = (ctypes.c_char * (1 << 20))()
    p = (ctypes.addressof(buf) + 255) & ~255                              # host memory: never dereferenced by a refused call
    off = p - ctypes.addressof(buf)
    for i in range(64):
        buf[off + 2048 + i] = 0x5A
    W, H = 45, 37
    need = lib.vtgs_tracking_mask_scratch_bytes(W, H, 3, 1)
    assert 0 < need <= (1 << 20) - 65536 - 256
    ptrs = lambda *a: (ctypes.c_void_p * len(a))(*a)
    good = dict(w=W, h=H, gt=p, k=p + 8192, curr=p + 8448, n=3, ow=ptrs(p + 8704, p + 8768, p + 8832),
                od=ptrs(p + 16384, p + 24576, p + 32768), thres=0.05, use_far=1, far=5.0, rd=p + 40960, scratch=p + 65536,
                sbytes=need, out=p + 2048, u8=None, bits=None)
    order = ("w", "h", "gt", "k", "curr", "n", "ow", "od", "thres", "use_far", "far", "rd", "scratch", "sbytes", "out", "u8", "bits")
    call = lambda **kw: lib.vtgs_tracking_mask(*[{**good, **kw}[k] for k in order], None)
    assert call(w=0) == INVALID and call(h=-2) == INVALID and call(w=65536, h=65536) == INVALID
    assert call(n=-1) == INVALID and call(n=4) == INVALID
    assert call(gt=None) == INVALID and call(out=None) == INVALID
    assert call(k=None) == INVALID and call(curr=None) == INVALID and call(ow=None) == INVALID and call(od=None) == INVALID
    assert call(ow=ptrs(p + 8704, None, p + 8832)) == INVALID and call(od=ptrs(p + 16384, p + 24576, None)) == INVALID
    assert call(scratch=None) == INVALID and call(scratch=p + 65536 + 4) == INVALID          # NULL, not 16-byte aligned
    assert call(sbytes=need - 1) == INVALID and call(sbytes=0) == INVALID
    # the scratch of a smaller request does not serve a larger one
    assert call(sbytes=lib.vtgs_tracking_mask_scratch_bytes(W, H, 3, 0)) == INVALID
    assert call(n=1, rd=None, sbytes=0) == INVALID and call(n=0, sbytes=lib.vtgs_tracking_mask_scratch_bytes(W, H, 0, 1) - 1) == INVALID
    assert bytes(buf[off + 2048:off + 2048 + 64]) == b"\x5a" * 64
