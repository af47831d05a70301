"""vtgs_adam_step / vtgs_adam_step_rows (csrc/vtgs_adam.hip) on every path: the float4 form, its one-by-one tail, the form
taken when a base is not 16-byte aligned and the row-list kernel must give the same bits (the kernel's stated guarantee), a
short group must survive sharing a launch with a long one, FusedAdam must chunk past VTGS_ADAM_MAX_GROUPS, and all of it must
sit within a few float32 ulps of the float64 statement of the update in tests/loss_ref.py.  Every array lives between 64
sentinel floats inside its own allocation, so a float4 store past `count` shows without an access outside any allocation."""
import numpy as np
import pytest
import torch

import loss_ref as lr

pytestmark = pytest.mark.gpu

GUARD = 64
SENT = float(np.float32(-12345.678))
B1, B2 = 0.9, 0.999
LR = 2.5e-3
COUNTS = [1, 2, 3, 4, 5, 1023, 1024, 1025, 4099]
NAMES = ("param", "grad", "exp_avg", "exp_avg_sq")


def _api():
    import diff_gaussian_rasterization as dgr
    from diff_gaussian_rasterization import optim
    return dgr._lib, dgr._stream_ptr, optim


def host_arrays(n, seed, moments=False):
    """float32 CPU arrays of one group: parameters of magnitude 0.5 .. 8, gradients spanning 1e-12 .. 1e6 in magnitude with
    exact zeros, and (moments=True) moment estimates as a long run would have left them."""
    g = torch.Generator().manual_seed(1000 + 7 * n + seed)
    sign = lambda: torch.where(torch.rand(n, generator=g) < 0.5, -1.0, 1.0)
    p = sign() * (0.5 + 7.5 * torch.rand(n, generator=g))
    gr = sign() * 10.0 ** (torch.rand(n, generator=g) * 18.0 - 12.0)
    gr[2::5] = 0.0
    if n > 1:
        gr[0], gr[-1] = 1e-12, -1e6
    m, v = torch.zeros(n), torch.zeros(n)
    if moments:
        m = gr * (0.5 + torch.rand(n, generator=g))
        v = gr * gr * (0.5 + torch.rand(n, generator=g)) + 1e-30
    return {"param": p, "grad": gr, "exp_avg": m, "exp_avg_sq": v}


class Group:
    """One group on the device; `off` = the names whose base sits one float past a 16-byte boundary."""

    def __init__(self, dev, host, off=()):
        self.n = host["param"].numel()
        self.buf, self.t = {}, {}
        for k in NAMES:
            o = 1 if k in off else 0
            self.buf[k] = torch.full((GUARD + o + self.n + GUARD,), SENT, dtype=torch.float32, device=dev)
            self.t[k] = self.buf[k][GUARD + o:GUARD + o + self.n]
            self.t[k].copy_(host[k])
            assert self.t[k].data_ptr() % 16 == 4 * o

    def set_grad(self, gr):
        self.t["grad"].copy_(gr)

    def intact(self):
        for k in NAMES:
            lo = (self.t[k].data_ptr() - self.buf[k].data_ptr()) // 4
            if not (bool((self.buf[k][:lo] == SENT).all()) and bool((self.buf[k][lo + self.n:] == SENT).all())):
                return False
        return True

    def state(self):
        return {k: self.t[k].cpu() for k in ("param", "exp_avg", "exp_avg_sq")}


def c_step(dev, groups, step, eps, lr_=LR, rows=None, n_rows=None, n_total=None):
    lib, stream, optim = _api()
    recs = [optim._Group(g.t["param"].data_ptr(), g.t["grad"].data_ptr(), g.t["exp_avg"].data_ptr(), g.t["exp_avg_sq"].data_ptr(),
                         g.n, lr_, eps) for g in groups]
    arr = (optim._Group * len(recs))(*recs)
    if n_total is None:
        st = lib.vtgs_adam_step(arr, len(recs), step, B1, B2, stream(dev))
    else:
        st = lib.vtgs_adam_step_rows(arr, len(recs), step, B1, B2, None if rows is None else rows.data_ptr(),
                                     int(rows.numel()) if n_rows is None else n_rows, n_total, stream(dev))
    assert st == 0
    torch.cuda.synchronize()
    assert all(g.intact() for g in groups)


def same_bits(a, b):
    return all(torch.equal(a[k].view(torch.int32), b[k].view(torch.int32)) for k in a)


def steps_of(n, seed, n_steps=3):
    """The gradients of `n_steps` iterations: the spanning set of host_arrays, rescaled per step."""
    return [host_arrays(n, seed + s)["grad"] * (10.0 ** (s - 1)) for s in range(n_steps)]


def reference_run(host, grads, eps, first_step=1):
    p, m, v = (host[k].double().numpy() for k in ("param", "exp_avg", "exp_avg_sq"))
    for s, gr in enumerate(grads):
        p, m, v = lr.adam_reference(p, gr.double().numpy(), m, v, LR, eps, B1, B2, first_step + s)
    return p


def assert_within_4_ulps(got, host, ref):
    """The parameter CHANGE within 4 float32 ulps (taken at the parameter's magnitude) of the float64 change."""
    p0 = host["param"].double().numpy()
    ulp = np.spacing(np.maximum(np.abs(host["param"].numpy()), np.abs(ref).astype(np.float32)))
    err = np.abs((got["param"].double().numpy() - p0) - (ref - p0))
    assert (err <= 4.0 * ulp).all(), (float((err / ulp).max()), int(np.argmax(err / ulp)))


@pytest.mark.parametrize("eps", [1e-8, 1e-15])
@pytest.mark.parametrize("n", COUNTS)
def test_every_count_and_alignment_gives_the_same_bits_and_float64_agrees(gpu_device, n, eps):
    dev = gpu_device
    for moments, first_step, n_steps in ((False, 1, 3), (True, 100000, 1)):      # steps 1, 2, 3 from zero moments; one late step
        host = host_arrays(n, 0, moments)
        grads = steps_of(n, 0, n_steps)
        results = []
        for off in ((), NAMES, ("grad",)):                                       # aligned; every base offset; the gradient only
            grp = Group(dev, host, off)
            for s, gr in enumerate(grads):
                grp.set_grad(gr)
                c_step(dev, [grp], first_step + s, eps)
            results.append(grp.state())
        assert same_bits(results[0], results[1]) and same_bits(results[0], results[2])
        assert_within_4_ulps(results[0], host, reference_run(host, grads, eps, first_step))
        zero = (torch.stack(grads) == 0).all(0) & (host["exp_avg"] == 0)
        assert torch.equal(results[0]["param"][zero], host["param"][zero])       # no gradient, no momentum: not a bit moves


def test_short_and_long_groups_share_a_launch(gpu_device):
    dev = gpu_device
    lengths = [1, 2, 3, 4, 5, 1023, 1025, 4099]                                  # VTGS_ADAM_MAX_GROUPS groups, one launch
    offs = [(), NAMES, ("grad",), (), NAMES, ("param",), (), NAMES]
    hosts = [host_arrays(n, 3, moments=True) for n in lengths]
    together = [Group(dev, h, o) for h, o in zip(hosts, offs)]
    c_step(dev, together, 7, 1e-15)
    for h, grp in zip(hosts, together):
        alone = Group(dev, h)
        c_step(dev, [alone], 7, 1e-15)
        assert same_bits(alone.state(), grp.state()), grp.n
        assert_within_4_ulps(grp.state(), h, reference_run(h, [h["grad"]], 1e-15, 7))


def test_fused_adam_chunks_past_the_group_limit(gpu_device):
    _, _, optim = _api()
    dev = gpu_device
    lengths = COUNTS + [7, 300]                                                  # eleven tensors: 8 + 3
    assert len(lengths) > optim._MAX
    hosts = [host_arrays(n, 5) for n in lengths]
    params = [torch.nn.Parameter(h["param"].clone().to(dev)) for h in hosts]
    opt = optim.FusedAdam([{"params": [p], "lr": LR} for p in params], lr=0.0, eps=1e-8)
    singles = [Group(dev, h) for h in hosts]
    all_grads = [steps_of(n, 5) for n in lengths]
    for s in range(3):
        for p, grp, grads in zip(params, singles, all_grads):
            p.grad = grads[s].clone().to(dev)
            grp.set_grad(grads[s])
            c_step(dev, [grp], s + 1, 1e-8)
        opt.step()
    for p, grp, h, grads in zip(params, singles, hosts, all_grads):
        st = opt.state[p]
        got = {"param": p.detach().cpu(), "exp_avg": st["exp_avg"].cpu(), "exp_avg_sq": st["exp_avg_sq"].cpu()}
        assert same_bits(got, grp.state()), grp.n
        assert_within_4_ulps(got, h, reference_run(h, grads, 1e-8))


@pytest.mark.parametrize("width", [1, 3, 4])
def test_row_list_kernel_gives_the_bits_of_the_full_step(gpu_device, width):
    dev = gpu_device
    n_rows = 259
    host = host_arrays(n_rows * width, width, moments=True)
    full = Group(dev, host)
    c_step(dev, [full], 5, 1e-15)
    want = full.state()
    g = torch.Generator().manual_seed(width)
    # all rows, shuffled: the full step's bits (aligned and with every base one float off)
    order = torch.randperm(n_rows, generator=g).to(torch.int32).to(dev)
    for off in ((), NAMES):
        grp = Group(dev, host, off)
        c_step(dev, [grp], 5, 1e-15, rows=order, n_total=n_rows)
        assert same_bits(grp.state(), want)
    # no rows: nothing moves
    grp = Group(dev, host)
    c_step(dev, [grp], 5, 1e-15, rows=None, n_rows=0, n_total=n_rows)
    assert same_bits(grp.state(), {k: host[k] for k in ("param", "exp_avg", "exp_avg_sq")})
    # the first and the last row: those get the full step's bits, every other row keeps parameter and both moments
    grp = Group(dev, host)
    c_step(dev, [grp], 5, 1e-15, rows=torch.tensor([n_rows - 1, 0], dtype=torch.int32, device=dev), n_total=n_rows)
    got = grp.state()
    listed = torch.zeros(n_rows, dtype=torch.bool)
    listed[[0, n_rows - 1]] = True
    for k in got:
        a, w, h = (t.reshape(n_rows, width).view(torch.int32) for t in (got[k], want[k], host[k]))
        assert torch.equal(a[listed], w[listed]) and torch.equal(a[~listed], h[~listed]), k
