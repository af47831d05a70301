"""vtgs_lower_median (csrc/vtgs_densify.hip): bit-equal to torch.median of the CPU copy -- the element of rank (n - 1) // 2,
NaN as soon as one value is NaN -- at every size where the kernels change path (wavefront 64, workgroup 256, the 4096
values a workgroup takes per trip, the 1024-workgroup grid beyond which it strides), on every key pattern that exercises
one digit pass alone, and on the float32 specials.  The scratch and the outputs are poisoned before each call."""
import ctypes

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu


def _bits(a):
    return np.asarray(a, dtype=np.uint32).view(np.float32)


def _cases():
    rng = np.random.default_rng(20251021)
    c = {}
    for n in (1, 2, 3, 63, 64, 65, 255, 256, 257, 4095, 4096, 4097, 72 * 56):
        c[f"n{n}"] = rng.standard_normal(n).astype(np.float32) * 3
    c["stride_4096x1024_plus_4097"] = rng.random(4096 * 1024 + 4097, dtype=np.float32)       # workgroups 0 and 1 make a second trip
    c["all_equal"] = np.full(1000, 2.5, np.float32)
    one = np.zeros(1001, np.float32); one[517] = -4.0
    c["one_nonzero_among_zeros"] = one
    c["one_nonzero_among_zeros_even"] = np.concatenate([np.zeros(999, np.float32), [7.0]]).astype(np.float32)
    for name, parts in (("dup_rank_inside", [(1.0, 10), (2.0, 10), (3.0, 10)]), ("dup_rank_last_of_low", [(1.0, 5), (2.0, 5)]),
                        ("dup_rank_first_of_high", [(1.0, 5), (2.0, 7)]), ("dup_many", [(-1.0, 3000), (0.5, 3001), (9.0, 3000)])):
        v = np.concatenate([np.full(k, x, np.float32) for x, k in parts])
        rng.shuffle(v)
        c[name] = v
    c["low_10_key_bits_only"] = _bits(0x3F800000 + rng.integers(0, 1024, 5000))
    c["low_10_key_bits_only_negative"] = _bits(0xBF800000 + rng.integers(0, 1024, 4999))
    hi = rng.integers(0, 2048, 6000).astype(np.uint32)
    hi = hi[((hi >> 2) & 0xFF) != 0xFF]                                  # no exponent of all ones: that would be inf / NaN
    c["high_11_key_bits_only"] = _bits((hi << 21) | 0x12345)
    mid = rng.integers(0, 2048, 5000).astype(np.uint32)
    c["middle_11_key_bits_only"] = _bits(0x40000000 | (mid << 10) | 0x2A5)
    special = np.concatenate([rng.standard_normal(300).astype(np.float32), -np.abs(rng.standard_normal(300)).astype(np.float32) * 1e20,
                              np.full(40, -0.0, np.float32), np.full(40, 0.0, np.float32), _bits(rng.integers(1, 1 << 22, 200)),
                              -_bits(rng.integers(1, 1 << 22, 200)), np.full(30, np.inf, np.float32), np.full(7, -np.inf, np.float32)])
    rng.shuffle(special)
    c["negatives_zeros_denormals_inf"] = special.astype(np.float32)
    c["zeros_of_both_signs"] = np.array([0.0, -0.0, -0.0, 0.0, -0.0], np.float32)
    c["median_is_a_denormal"] = np.concatenate([-np.ones(10, np.float32), _bits([5, 3, 9]), np.ones(10, np.float32)])
    c["mostly_inf"] = np.array([np.inf] * 6 + [1.0, 2.0, -np.inf], np.float32)
    nan_last = rng.standard_normal(5000).astype(np.float32); nan_last[-1] = np.nan
    c["nan_at_the_last_position"] = nan_last
    c["empty"] = np.zeros(0, np.float32)
    return c


CASES = _cases()


def _abi_median(dev, values):
    from diff_gaussian_rasterization import densify as dz
    from diff_gaussian_rasterization import _stream_ptr
    lib = dz._lib
    n = int(values.size)
    v = torch.from_numpy(values).to(dev)
    sbytes = int(lib.vtgs_median_scratch_bytes(n))
    assert sbytes > 0
    scratch = torch.full((sbytes,), 0xA5, dtype=torch.uint8, device=dev)             # poison
    out = torch.full((2,), 0x7A7A7A7A, dtype=torch.int32, device=dev)
    rc = lib.vtgs_lower_median(v.data_ptr() if n else None, n, scratch.data_ptr(), sbytes, out.data_ptr(), out.data_ptr() + 4,
                               _stream_ptr(dev))
    assert rc == 0, rc
    host = out.cpu()
    return host[:1].view(torch.float32)[0].item(), int(host[1].item())


def _same(got: float, want: float) -> bool:
    return (got != got and want != want) or got == want


@pytest.mark.parametrize("name", list(CASES))
def test_lower_median_equals_torch_median(gpu_device, name):
    values = CASES[name]
    want = torch.from_numpy(values).median().item() if values.size else float("nan")   # torch.median of an empty tensor raises
    nans = int(np.isnan(values).sum())
    got, got_nans = _abi_median(gpu_device, values)
    print(name, "n", values.size, "median", got, "want", want, "nan_count", got_nans)
    assert _same(got, want), (name, got, want)
    assert got_nans == nans
    if name == "nan_at_the_last_position":
        assert got != got and got_nans == 1


def test_python_mirror_and_repeatability(gpu_device):
    from diff_gaussian_rasterization.densify import lower_median
    x = torch.from_numpy(CASES["n4032"]).to(gpu_device).reshape(56, 72)
    a, b = lower_median(x), lower_median(x)
    assert a.dim() == 0 and a.is_cuda and a.item() == b.item() == x.cpu().median().item()
    m, k = lower_median(torch.from_numpy(CASES["nan_at_the_last_position"]).to(gpu_device), return_nan_count=True)
    assert m.item() != m.item() and k.item() == 1
    e = lower_median(torch.zeros(0, device=gpu_device))
    assert e.item() != e.item()
    h = lower_median(torch.from_numpy(CASES["n257"]).to(gpu_device).double())     # any dtype: taken as float32, like the loss masks
    assert h.item() == torch.from_numpy(CASES["n257"]).median().item()
