"""bench.py: a plain run prints the headline line only and, with --dump-outputs, writes what its last timed step returned;
the files hold float32, stay inside the byte budget (a fixed, seeded sample beyond it) and are the operator's own outputs."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _bench_module():
    sys.path.insert(0, ROOT)
    try:
        import bench
        return bench
    finally:
        sys.path.remove(ROOT)


def test_dump_outputs_whole_then_a_fixed_sample_inside_the_budget(tmp_path, monkeypatch):
    bench = _bench_module()
    n, h, w = 1000, 8, 12
    g = torch.Generator().manual_seed(5)
    images = {"color": torch.rand(3, h, w, generator=g), "depth": torch.rand(1, h, w, generator=g)}
    rows = {"radii": torch.arange(n, dtype=torch.int32), "grad_means3D": torch.rand(n, 3, generator=g), "grad_unused": None}
    bench.dump_outputs(str(tmp_path / "whole"), images, rows, n)
    got = {f[:-4]: np.load(tmp_path / "whole" / f) for f in sorted(os.listdir(tmp_path / "whole"))}
    assert sorted(got) == ["color", "depth", "grad_means3D", "radii"]
    assert all(v.dtype == np.float32 for v in got.values())
    assert np.array_equal(got["color"], images["color"].numpy()) and np.array_equal(got["grad_means3D"], rows["grad_means3D"].numpy())
    assert np.array_equal(got["radii"], np.arange(n, dtype=np.float32))
    # a budget the per-Gaussian arrays do not fit: the images stay whole, every per-Gaussian array keeps the same rows
    img_bytes = 4 * 4 * h * w
    monkeypatch.setattr(bench, "DUMP_BUDGET_BYTES", img_bytes + 16 * 100)
    for d in ("a", "b"):
        bench.dump_outputs(str(tmp_path / d), images, rows, n)
    a = {f[:-4]: np.load(tmp_path / "a" / f) for f in os.listdir(tmp_path / "a")}
    b = {f[:-4]: np.load(tmp_path / "b" / f) for f in os.listdir(tmp_path / "b")}
    assert all(np.array_equal(a[k], b[k]) for k in a) and sorted(a) == sorted(got)
    assert a["color"].shape == (3, h, w) and a["radii"].shape == (100,) and a["grad_means3D"].shape == (100, 3)
    sel = a["radii"].astype(np.int64)                                  # (radii = the row number here)
    assert np.all(np.diff(sel) > 0) and np.array_equal(a["grad_means3D"], rows["grad_means3D"].numpy()[sel])
    assert sum(v.nbytes for v in a.values()) <= img_bytes + 16 * 100
    # a budget the images do not fit either: a pixel sample of at most half of it
    monkeypatch.setattr(bench, "DUMP_BUDGET_BYTES", 16 * 40)
    bench.dump_outputs(str(tmp_path / "c"), images, rows, n)
    c = {f[:-4]: np.load(tmp_path / "c" / f) for f in os.listdir(tmp_path / "c")}
    assert c["color"].shape == (3, 20) and c["depth"].shape == (1, 20) and c["radii"].shape == (20,)
    assert sum(v.nbytes for v in c.values()) <= 16 * 40


@pytest.mark.gpu
def test_plain_run_prints_the_headline_and_dumps_the_operator_outputs(gpu_device, tmp_path):
    import diff_gaussian_rasterization as dgr
    from oracle import gs_oracle as go
    from parity_util import to_settings
    n, w, h = 4000, 128, 96
    out = tmp_path / "dump"
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "3", "--warmup", "1", "--ramp-ms", "0",
                        "--n", str(n), "--width", str(w), "--height", str(h), "--dump-outputs", str(out)],
                       capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr[-800:]
    lines = [ln for ln in r.stdout.splitlines() if ln.strip()]
    assert len(lines) == 1
    line = json.loads(lines[0])
    assert line["steps"] == 3 and line["warmup"] == 1 and line["ms_per_step"] > 0 and line["higher_is_better"] is True
    assert line["dtype"] == "f32" and line["unit"] == "Mgaussians*pixels/s" and line["full"] is False
    assert abs(line["value"] - n * w * h / (line["ms_per_step"] * 1e-3) / 1e6) <= 1e-3 * line["value"]
    # nothing of the --full measurements in a plain line
    assert not {"roofline", "cpu_baseline", "parity", "slam", "loop_steps", "step_events", "kernels_us",
                "first_region_ms_per_step"} & set(line)
    got = {f[:-4]: np.load(out / f) for f in os.listdir(out)}
    assert sorted(got) == sorted(["color", "depth", "radii"] + ["grad_" + k for k in
                                 ("means3D", "means2D", "colors_precomp", "opacities", "scales", "rotations")])
    assert all(v.dtype == np.float32 and np.isfinite(v).all() for v in got.values())
    # the same inputs through the operator in this process
    scene, cam = go.view_tied_scene(n, w, h, seed=0)
    leaves = {k: v.to(gpu_device).requires_grad_(True) for k, v in scene.items()}
    grad_color = (torch.rand(3, h, w, generator=torch.Generator().manual_seed(1)) * 2 - 1).to(gpu_device)
    color, radii, depth = dgr.GaussianRasterizer(raster_settings=to_settings(cam, gpu_device))(**leaves)
    color.backward(grad_color)
    assert np.array_equal(got["radii"], radii.float().cpu().numpy()) and (got["radii"] > 0).any()
    # forward: the same kernels compose each pixel front to back in the same sorted order -- bit for bit.  backward: float32
    # sums over a Gaussian's pixels whose order is not fixed: 1e-4 of the largest gradient, a tenth of what the suite allows
    # the operator against the float64 oracle (rotations: rounding noise around an exact zero on the isotropic scene)
    assert np.array_equal(got["color"], color.detach().cpu().numpy()) and np.array_equal(got["depth"], depth.detach().cpu().numpy())
    for k, v in leaves.items():
        ref = v.grad.cpu().numpy().reshape(got["grad_" + k].shape)
        if k == "rotations":
            assert np.abs(got["grad_" + k]).max() <= 1e-5
            continue
        assert np.abs(ref).max() > 0 and np.abs(got["grad_" + k] - ref).max() <= 1e-4 * np.abs(ref).max(), k
