"""Splats placed ON the size thresholds of the second binning kernel and of the gradient gather.

bin_deferred_splats (csrc/vtgs_binning.hip) takes a splat by its candidate-tile area: up to 9 its own lane inside project_and_bin,
up to 64 a 16-lane group, up to 512 a wavefront, beyond that the workgroup (256 tiles per step, a second pass beyond 131,072).
gather_splat_grads (csrc/vtgs_gather.hip) takes a splat by its instance count: the lane's own first 4 records, records 5..64
through the wavefront's excess list (windows of 64 positions, owners found by a binary search over the lanes' scan), more than 64
summed by the whole wavefront.  The random maps of the other tests land somewhere inside these tiers; here every count is chosen.

The construction: a frame ONE 8x8 tile high (H = 8) under a near-orthographic camera (fx = 65536).  An isotropic splat of opacity o
at v = 3.5, u = 8 t0 + 4 k - 0.5 with screen sigma (4 k - 2) / sqrt(2 ln(255 o)) has its alpha >= 1/255 region end 2.5 px short of the
first pixel of tile t0 - 1 and of tile t0 + k: it reaches exactly the k tiles t0 .. t0 + k - 1.  For o <= 0.353 that region is
narrower than the 3-sigma rectangle, so the kernel's candidate box (the bounding box of the region) is those k tiles too: candidate
area = instance count = k.  Every scene first proves that about itself on the CPU (strict oracle set == loose oracle set, per-splat
counts == the intended k) before anything runs on the device.

Every case then asks: the kernel's (tile, Gaussian) set equals the oracle's exactly, every list strictly (depth bits, id) ordered;
images and gradients against the float64 oracle at the bounds of tests/test_gpu_parity.py (1e-4 / 1e-3); and the same scene
through the round 2-5 route inside project_and_bin (the no-deferred hint, tests/test_gpu_no_defer_hint.py) gives the same bits.
"""
import functools

import pytest
import torch

from oracle import gs_oracle as go
from parity_util import (GRAD_KEYS, HIP_CENTRE_ERR_PX, audit_outliers, grad_error, oracle_instances_8x8, run_oracle,
                         tainted_gaussians, to_settings)

IMG_TOL, GRAD_TOL = 1e-4, 1e-3           # the bounds of tests/test_gpu_parity.py
ROUTE_TOL = 2e-4                         # two routes to the same sums: float32 summation order (the dual-render bound)
STRIP_W, FX = 4160, 65536.0              # 520 tiles in one row
INVISIBLE = 0.003                        # an opacity below 1/255: the splat projects, reaches nothing


# ---------------------------------------------------------------------------------------------------------------------------------
# generators (CPU)
# ---------------------------------------------------------------------------------------------------------------------------------
def _reach_sigma(reach_px, opacity):
    """Screen sigma whose alpha >= 1/255 region has the half-width `reach_px` at this opacity."""
    return reach_px / torch.sqrt(2.0 * torch.log(255.0 * opacity))


def _scene(W, H, u, v, sigma_px, opacity, z, fx=FX, seed=0):
    """Isotropic splats whose centres project to the pixel coordinates (u, v) (pixel centres are the integers) with the screen
    sigma `sigma_px` (which includes the 0.3 px^2 dilation), identity pose, principal point at the frame's centre."""
    f64 = lambda x: torch.as_tensor(x, dtype=torch.float64).reshape(-1)
    u, sigma_px, opacity, z = f64(u), f64(sigma_px), f64(opacity), f64(z)
    n = u.numel()
    v = f64(v).expand(n)
    cx, cy = W / 2.0 - 0.5, H / 2.0 - 0.5
    cam = go.setup_camera(W, H, [[fx, 0, cx], [0, fx, cy], [0, 0, 1]], torch.eye(4))
    g = torch.Generator().manual_seed(seed)
    scene = {
        "means3D": torch.stack([(u - cx + 0.5) / fx * z, (v - cy + 0.5) / fx * z, z], dim=-1).float().contiguous(),
        "means2D": torch.zeros(n, 3),
        "opacities": opacity.float().reshape(n, 1).contiguous(),
        "colors_precomp": torch.rand(n, 3, generator=g),
        "scales": (torch.sqrt(sigma_px * sigma_px - go.DILATION) * z / fx).float()[:, None].repeat(1, 3).contiguous(),
        "rotations": torch.tensor([[1.0, 0.0, 0.0, 0.0]]).repeat(n, 1),
    }
    return scene, cam


def _depths(n, seed):
    """n distinct depths in [1, 4), in an order that has nothing to do with the index."""
    perm = torch.randperm(n, generator=torch.Generator().manual_seed(100 + seed)).double()
    return 1.0 + 3.0 * perm / n


def _strip(ks, t0s, opacity=0.3, seed=0, W=STRIP_W):
    """The one-row frame: splat i reaches exactly the ks[i] tiles from t0s[i] on; ks[i] == 0: an invisible splat (one tile wide,
    opacity below 1/255).  Returns (scene, cam, intended counts)."""
    k = torch.tensor(ks, dtype=torch.float64)
    t0 = torch.tensor(t0s, dtype=torch.float64)
    assert bool((t0 >= 0).all()) and bool((t0 + torch.clamp(k, min=1) <= W // 8).all())
    kg = torch.clamp(k, min=1.0)
    op = torch.where(k > 0, torch.full_like(k, opacity), torch.full_like(k, INVISIBLE))
    sigma = _reach_sigma(4.0 * kg - 2.0, torch.full_like(k, opacity))
    scene, cam = _scene(W, 8, 8.0 * t0 + 4.0 * kg - 0.5, 3.5, sigma, op, _depths(len(ks), seed), seed=seed)
    return scene, cam, [int(x) for x in ks]


def _pack(ks, tiles=STRIP_W // 8):
    """Starts that lay the splats side by side along the strip, wrapping at its end (overlap only between the wraps)."""
    out, cur = [], 0
    for k in ks:
        k = max(int(k), 1)
        if cur + k > tiles:
            cur = 0
        out.append(cur)
        cur += k
    return out


def _self_check(scene, cam, want=None, rows8=None):
    """What every scene proves about itself before the device is touched: no instance sits in the band between the strict reach
    predicate and the one with twice the kernel's slack, and the per-splat counts are the intended ones.  Returns the float64
    splats, the sorted instance keys and the per-splat counts."""
    n = scene["means3D"].shape[0]
    with torch.no_grad():
        f = {k: v.double() for k, v in scene.items()}
        sp = go.preprocess(f["means3D"], f["means2D"], f["opacities"], f["scales"], f["rotations"], cam)
    strict = oracle_instances_8x8(sp, scene["opacities"], cam, rows8=rows8)
    loose = oracle_instances_8x8(sp, scene["opacities"], cam, 2e-4, 2e-4, rows8=rows8)
    assert torch.equal(strict, loose), f"{loose.numel() - strict.numel()} ambiguous instances: move or resize that splat"
    counts = torch.bincount(strict & 0xFFFFFFFF, minlength=n)
    if want is not None:
        assert counts.tolist() == list(want), [(i, c, w) for i, (c, w) in enumerate(zip(counts.tolist(), want)) if c != w][:10]
    return sp, strict, counts


# ---- case 1: one splat on each side of every binning tier edge --------------------------------------------------------------------
EDGE_KS = [9, 10, 11, 63, 64, 65, 66, 511, 512, 513, 514]
EDGE_T0 = [20, 60, 100, 140, 210, 280, 350, 0, 2, 4, 6]


@functools.lru_cache(maxsize=None)
def _edge_strip():
    ks = EDGE_KS + [1] * 40
    t0 = EDGE_T0 + [3 + 13 * i for i in range(40)]
    order = torch.randperm(len(ks), generator=torch.Generator().manual_seed(7)).tolist()     # the edges anywhere in the wavefront
    return _strip([ks[i] for i in order], [t0[i] for i in order], seed=1)


def _disc(W, H, t0, k, seed, others=24):
    """A frame H / 8 tiles high: one disc centred on the frame's middle row, k tiles wide, whose alpha >= 1/255 region comes within
    a tile of the frame's first and last pixel row (or passes them) -- its bounding box meets every tile row: a candidate box of
    k x H / 8 -- over a sprinkle of one-tile splats.  The oracle decides which of the box's tiles the disc reaches (the corners
    are missed)."""
    g = torch.Generator().manual_seed(seed)
    gx8, gy8 = W // 8, H // 8
    tx = torch.randint(0, gx8, (others,), generator=g).double()
    ty = torch.randint(0, gy8, (others,), generator=g).double()
    u = torch.cat([torch.tensor([8.0 * t0 + 4.0 * k - 0.5]), 8.0 * tx + 3.5])
    v = torch.cat([torch.tensor([H / 2.0 - 0.5]), 8.0 * ty + 3.5])
    reach = torch.cat([torch.tensor([4.0 * k - 2.0]), torch.full((others,), 2.0, dtype=torch.float64)])
    op = torch.full((others + 1,), 0.3, dtype=torch.float64)
    scene, cam = _scene(W, H, u, v, _reach_sigma(reach, op), op, _depths(others + 1, seed), seed=seed)
    return scene, cam


DISCS = {                                 # name -> (W, H, first tile, tiles wide): boxes of 8x8 / 9x8 and 32x16 / 33x16 candidates
    "8x8": (320, 64, 5, 8), "9x8": (320, 64, 11, 9), "32x16": (576, 128, 7, 32), "33x16": (576, 128, 20, 33)}
BAND = (2, 6)                             # the 16-pixel tile rows of the band test (8x8 tile rows 4 .. 11 of the 16-row frames)


def _disc_scene(name):
    W, H, t0, k = DISCS[name]
    return _disc(W, H, t0, k, seed=sorted(DISCS).index(name))


# ---- case 2: more than one round of both deferred lists per workgroup -----------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _rounds_strip():
    n = 4270
    ks = [65 if i % 61 == 0 else 10 for i in range(n)]             # 70 large-list entries among 4,200 small-list entries
    t0, a, b = [], 0, 0
    for k in ks:
        if k == 65:
            t0.append((a * 7) % (STRIP_W // 8 - 65 + 1)); a += 1
        else:
            t0.append((b * 37) % (STRIP_W // 8 - 10 + 1)); b += 1
    return _strip(ks, t0, opacity=0.02, seed=2)


# ---- case 3: the huge pass edge ---------------------------------------------------------------------------------------------------
def _huge(H):
    """One splat that reaches every tile of a 4096 x H frame (reach 2600 px at opacity 0.3: more than the half-diagonal) and two
    one-tile splats behind it."""
    W = 4096
    u = torch.tensor([W / 2.0 - 0.5, 8.0 * 100 + 3.5, 8.0 * 400 + 3.5], dtype=torch.float64)
    v = torch.tensor([H / 2.0 - 0.5, 8.0 * 30 + 3.5, 8.0 * (H // 8 - 1) + 3.5], dtype=torch.float64)
    op = torch.tensor([0.3, 0.3, 0.3], dtype=torch.float64)
    sigma = _reach_sigma(torch.tensor([2600.0, 2.0, 2.0], dtype=torch.float64), op)
    return _scene(W, H, u, v, sigma, op, torch.tensor([1.0, 2.0, 3.0]), fx=262144.0, seed=3)


# ---- case 4: instance counts by lane of the gather ------------------------------------------------------------------------------
def _wave(fill, **at):
    """64 counts: `fill` everywhere, except lane L = c for every keyword lL = c."""
    w = [fill] * 64
    for name, c in at.items():
        w[int(name[1:])] = c
    return w


GATHER_WAVES = {
    # (a) each count on the first, a middle and the last lane of a wavefront, single-record splats around it
    "c0": _wave(1, l0=0, l31=0, l63=0), "c1": _wave(2, l0=1, l31=1, l63=1), "c4": _wave(1, l0=4, l31=4, l63=4),
    "c5": _wave(1, l0=5, l31=5, l63=5), "c64": _wave(1, l0=64, l31=64, l63=64), "c65": _wave(1, l0=65, l31=65, l63=65),
    # (b) excess totals of exactly one window, one window and a record, two windows; owners apart, the last one on lane 63
    "T64": _wave(0, l0=24, l17=14, l40=34, l63=8), "T65": _wave(0, l0=5, l30=64, l63=8),
    "T128": _wave(0, l0=64, l1=8, l33=64, l63=8),
    # ... and the same three totals from owners of ONE size (8 or 9 instances: every record weighs about the same in the sums)
    "E64": _wave(0, **{f"l{l}": 8 for l in range(3, 64, 4)}), "E65": _wave(0, **{f"l{l}": (9 if l == 3 else 8) for l in range(3, 64, 4)}),
    "E128": _wave(0, **{f"l{l}": 8 for l in range(1, 64, 2)}),
    # (c) the whole-wavefront sum and the excess list in one wavefront
    "mixed": _wave(1, l0=5, l10=64, l20=65, l21=17, l40=33, l63=6),
    # (d) one splat of 514 instances among splats without any
    "lone514": _wave(0, l37=514), "none": _wave(0),
}
GATHER_MAPS = {                            # name -> (wavefronts in map order, n)
    "a_small": (["c0", "c1", "c4", "c5"], 256), "a_large": (["c64", "c65", "c5", "c4"], 256),
    "b": (["T64", "T65", "T128", "mixed"], 256), "b_250": (["T64", "T65", "T128", "mixed"], 250),
    "b_even": (["E64", "E65", "E128", "c5"], 256),
    "d": (["none", "lone514", "none", "none"], 256),
    "two_blocks_506": (["T64", "T65", "T128", "mixed", "c64", "c65", "c5", "c4"], 506),     # the map is walked from its end
}


@functools.lru_cache(maxsize=None)
def _gather_strip(name):
    waves, n = GATHER_MAPS[name]
    ks = [c for w in waves for c in GATHER_WAVES[w]][:n]
    return _strip(ks, _pack(ks), seed=10 + sorted(GATHER_MAPS).index(name))


def _make(name):
    """Every scene of this file by name: "edges", "rounds", "disc:<DISCS key>", "gather:<GATHER_MAPS key>"."""
    kind, _, arg = name.partition(":")
    return {"edges": _edge_strip, "rounds": _rounds_strip}[kind]() if not arg else {"disc": _disc_scene, "gather": _gather_strip}[kind](arg)


# ---------------------------------------------------------------------------------------------------------------------------------
# CPU: the generators keep their promise (runs everywhere)
# ---------------------------------------------------------------------------------------------------------------------------------
def test_strip_generator_places_exact_tile_counts():
    ks = [1, 2, 3, 4, 5, 8, 9, 10, 16, 17, 63, 64, 65, 66, 128, 511, 512, 513, 514, 0]
    scene, cam, want = _strip(ks, [min(7 * i, STRIP_W // 8 - max(k, 1)) for i, k in enumerate(ks)], seed=0)
    sp, strict, _ = _self_check(scene, cam, want)
    tiles = strict >> 32
    for i, k in enumerate(ks):                                     # ... and they are the k tiles from t0 on
        mine = tiles[(strict & 0xFFFFFFFF) == i].tolist()
        t0 = min(7 * i, STRIP_W // 8 - max(k, 1))
        assert mine == list(range(t0, t0 + k)), (i, k)
    assert bool((sp.radii > 0).all())


@pytest.mark.parametrize("name", ["edges", "rounds"] + ["gather:" + m for m in GATHER_MAPS])
def test_every_strip_scene_passes_its_self_check(name):
    scene, cam, want = _make(name)
    _self_check(scene, cam, want)
    z = scene["means3D"][:, 2]
    assert torch.unique(z).numel() == z.numel(), "distinct depths"


def test_gather_maps_hold_what_their_names_say():
    excess = lambda w: sum(max(c - 4, 0) for c in GATHER_WAVES[w] if c <= 64)
    assert (excess("T64"), excess("T65"), excess("T128")) == (64, 65, 128)
    assert (excess("E64"), excess("E65"), excess("E128")) == (64, 65, 128)
    for w in ("T64", "T65", "T128", "E64", "E65", "E128", "mixed"):
        assert GATHER_WAVES[w][63] > 4, "the last owner sits on lane 63"


@pytest.mark.parametrize("name", list(DISCS))
def test_disc_scenes_are_unambiguous(name):
    W, H, t0, k = DISCS[name]
    scene, cam = _disc_scene(name)
    sp, strict, counts = _self_check(scene, cam)
    tiles = strict[(strict & 0xFFFFFFFF) == 0] >> 32
    tx, ty = tiles % (W // 8), tiles // (W // 8)
    # the disc's instances span the whole k x H / 8 box (that is the kernel's candidate area) and miss its corners
    assert (int(tx.min()), int(tx.max()), int(ty.min()), int(ty.max())) == (t0, t0 + k - 1, 0, H // 8 - 1)
    assert int(counts[0]) < k * (H // 8)
    if H == 128:                                                   # ... and in the band of tile rows the band test renders
        _self_check(scene, cam, rows8=(2 * BAND[0], 2 * BAND[1]))


@pytest.mark.parametrize("H,tiles", [(2048, 131072), (2056, 131584)])
def test_huge_scene_fills_the_frame(H, tiles):
    scene, cam = _huge(H)
    _self_check(scene, cam, [tiles, 1, 1])


# ---------------------------------------------------------------------------------------------------------------------------------
# GPU
# ---------------------------------------------------------------------------------------------------------------------------------
def _clear(dgr):
    for d in (dgr._capacity_hint, dgr._caps_in_use, dgr._tile_cap_hint, dgr._async_ok, dgr._need_hist, dgr._slots_hint,
              dgr._no_deferred, dgr._no_defer_cooldown):
        d.clear()


def _grad_color(cam, seed=5):
    g = torch.Generator().manual_seed(seed)
    return torch.rand(3, cam.image_height, cam.image_width, generator=g) * 2 - 1


def _run(scene, cam, dev, grad_color, tile_rows=None):
    import diff_gaussian_rasterization as dgr
    leaves = {k: v.detach().to(dev).clone().requires_grad_(grad_color is not None) for k, v in scene.items()}
    rast = dgr.GaussianRasterizer(raster_settings=to_settings(cam, dev), tile_rows=tile_rows)
    dgr.profile_enable(True)
    try:
        color, radii, depth = rast(**leaves)
        grads = None
        if grad_color is not None:
            (color * grad_color.to(dev)).sum().backward()
            grads = {k: leaves[k].grad.cpu() for k in GRAD_KEYS}
        dgr.settle_pending()
        prof = dgr.profile_collect()
    finally:
        dgr.profile_enable(False)
    offs, gid, geom = dgr.debug_tile_lists(rast)
    return {"color": color.detach().cpu(), "depth": depth.detach().cpu(), "radii": radii.cpu(), "grads": grads, "offs": offs,
            "gid": gid, "geom": geom, "info": dgr.last_forward_info(), "kernels": set(prof), "key": rast._last_state.key,
            "planned": bool(rast._last_state.tile_cap & dgr.PLANNED)}


def _both_routes(scene, cam, dev, grad_color, tile_rows=None, second=True):
    """The scene through bin_deferred_splats, then through the route inside project_and_bin: colour, depth, radii and the sorted
    lists bit for bit, gradients to the summation-order bound.  Returns the deferring run.  second = False: the first route only
    (the library honours the no-deferred hint for the whole frame in uniform bins, csrc/vtgs_api.hip; a band of tile rows and
    planned bins have other second routes, see their tests)."""
    import diff_gaussian_rasterization as dgr
    _clear(dgr)
    try:
        a = _run(scene, cam, dev, grad_color, tile_rows)
        assert "bin_deferred_splats" in a["kernels"]
        if not second:
            return a
        dgr._no_deferred[a["key"]] = True
        b = _run(scene, cam, dev, grad_color, tile_rows)
        assert "bin_deferred_splats" not in b["kernels"] and "project_and_bin" in b["kernels"]
    finally:
        _clear(dgr)
    for k in ("color", "depth", "radii", "offs", "gid"):
        assert torch.equal(a[k], b[k]), f"{k} differs between the two binning routes"
    assert a["info"]["instances"] == b["info"]["instances"]
    if grad_color is not None:
        for k in GRAD_KEYS:
            ga, gb = a["grads"][k], b["grads"][k]
            assert (ga - gb).abs().max().item() <= ROUTE_TOL * ga.abs().max().item(), (k, (ga - gb).abs().max().item())
    return a


def _check_lists(run, sp, strict, whole_frame=True):
    """The kernel's (tile, Gaussian) set IS the oracle's, every list strictly (depth bits, id) ordered, all of it accounted for."""
    offs, gid, geom = run["offs"], run["gid"], run["geom"]
    if whole_frame:
        assert torch.equal(run["radii"], sp.radii), "radii differ from the oracle's: the rectangles are not the same"
    else:                                   # a band reports the true radius or none (Gaussians that cannot meet its rows)
        assert bool(((run["radii"] == 0) | (run["radii"] == sp.radii)).all())
        assert bool((run["radii"][torch.unique(strict & 0xFFFFFFFF)] > 0).all())
    lens = offs[1:] - offs[:-1]
    tile_of = torch.repeat_interleave(torch.arange(lens.numel()), lens)
    keys = torch.sort((tile_of << 32) | gid).values
    missing, extra = strict[~torch.isin(strict, keys)], keys[~torch.isin(keys, strict)]
    show = lambda x: [(int(t >> 32), int(t & 0xFFFFFFFF)) for t in x[:8]]
    assert missing.numel() == 0 and extra.numel() == 0 and keys.numel() == strict.numel(), \
        f"(tile, Gaussian) missing from the kernel's lists: {show(missing)} ({missing.numel()}); not in the oracle's: {show(extra)} ({extra.numel()})"
    assert run["info"]["instances"] == strict.numel()
    binned = torch.unique(gid)
    assert torch.equal(geom[binned, 6].view(torch.int32), sp.zkey[binned].view(torch.int32))
    zbits = geom[:, 6].view(torch.int32).long()
    key = (zbits[gid] << 32) | gid
    assert bool(((key[1:] > key[:-1]) | (tile_of[1:] != tile_of[:-1])).all()), "a tile list is not strictly (depth, id)-ordered"


def _check_images(ref_c, ref_d, got_c, got_d, aux, opacities, cam):
    """As tests/test_gpu_parity.py: <= 1e-4 of the image maximum; a pixel above that must sit on a discrete decision of the
    composite in the oracle's own per-pair values and is then worth <= 8e-3.  Returns the Gaussians beside such a pixel."""
    tiles = set()
    for name, r, g in (("color", ref_c, got_c), ("depth", ref_d, got_d)):
        a = audit_outliers(r, g, aux, opacities, cam, IMG_TOL, centre_err_px=HIP_CENTRE_ERR_PX)
        assert not a["unexplained"], f"{name}: pixels above {IMG_TOL} that sit on no discrete decision: {a['unexplained'][:5]}"
        assert a["frac"] <= 1e-3 and a["max_rel"] <= 8e-3, f"{name}: {a['outliers']} outliers, max {a['max_rel']:.2e}"
        tiles |= a["tiles"]
    return tainted_gaussians(aux, tiles, opacities.shape[0])


def _check_grads(ref, got, taint):
    """<= 1e-3 (99.9th percentile element-wise) and, for EVERY Gaussian, <= 2e-3 of the largest gradient; Gaussians beside an
    audited threshold pixel differ by that one pair's contribution (<= 2e-2)."""
    for k in GRAD_KEYS:
        scale = ref[k].abs().max().item()
        if k == "rotations":             # isotropic: dL/drotations is zero in exact arithmetic, float noise on both sides
            assert got[k].abs().max().item() <= 1e-4 * max(ref["scales"].abs().max().item(), 1e-30), k
            continue
        d = (ref[k].double() - got[k].double()).abs() / scale
        clean, dirty = d[~taint], d[taint]
        worst = int(clean.reshape(clean.shape[0], -1).amax(1).argmax()) if clean.numel() else -1
        assert clean.numel() == 0 or clean.max().item() <= 2 * GRAD_TOL, f"grad {k}: max {clean.max().item():.2e} (clean row {worst})"
        assert grad_error(ref[k][~taint], got[k][~taint])[1] <= GRAD_TOL, f"grad {k}"
        assert dirty.numel() == 0 or dirty.max().item() <= 2e-2, f"grad {k}: max {dirty.max().item():.2e} beside an outlier pixel"


def _oracle_of(name, tile_rows=None):
    """(splats, instance keys, oracle render) of the scene `name`, after its self-check."""
    made = _make(name)
    scene, cam = made[0], made[1]
    rows8 = None if tile_rows is None else (2 * tile_rows[0], min(2 * tile_rows[1], (cam.image_height + 7) // 8))
    sp, strict, _ = _self_check(scene, cam, made[2] if len(made) > 2 else None, rows8)
    return sp, strict, run_oracle(scene, cam, _grad_color(cam), tile_rows=tile_rows)


_oracle_shared = functools.lru_cache(maxsize=None)(_oracle_of)        # computed once per session and never modified
SHARED = ("edges", "disc:33x16")                                      # the scenes more than one test renders


def _oracle(name, tile_rows=None):
    return (_oracle_shared if name in SHARED else _oracle_of)(name, tile_rows)


def _same_bits(a, b, rows=slice(None)):
    """Two runs that must not differ in a bit: the lists, the images (their rows `rows`), the radii, every gradient."""
    assert torch.equal(a["offs"], b["offs"]) and torch.equal(a["gid"], b["gid"]) and torch.equal(a["radii"], b["radii"])
    assert torch.equal(a["color"][:, rows], b["color"][:, rows]) and torch.equal(a["depth"][:, rows], b["depth"][:, rows])
    for k in GRAD_KEYS:
        assert torch.equal(a["grads"][k], b["grads"][k]), k


def _full_check(name, dev, tile_rows=None, second=True):
    """Conditions 1-4 of the module docstring on the scene `name` (_make)."""
    made = _make(name)
    scene, cam = made[0], made[1]
    sp, strict, (ref_c, _ref_r, ref_d, ref_g, aux) = _oracle(name, tile_rows)
    run = _both_routes(scene, cam, dev, _grad_color(cam), tile_rows, second)
    _check_lists(run, sp, strict, whole_frame=tile_rows is None)
    if tile_rows is not None:              # a band answers for its own rows only
        keep = torch.zeros(cam.image_height, dtype=torch.bool)
        keep[16 * tile_rows[0]: 16 * tile_rows[1]] = True
        run["color"], run["depth"] = run["color"] * keep[None, :, None], run["depth"] * keep[None, :, None]
    taint = _check_images(ref_c, ref_d, run["color"], run["depth"], aux, scene["opacities"], cam)
    _check_grads(ref_g, run["grads"], taint)
    return run


@pytest.mark.gpu
@pytest.mark.parametrize("impl", [0, 1, 2])
def test_binning_tier_edges(gpu_device, impl):
    """9 | 10, 11 .. 63, 64 | 65, 66 .. 511, 512 | 513, 514 candidate tiles, through global-atomic, LDS and windowed bins."""
    import diff_gaussian_rasterization as dgr
    dgr.set_option("VTGS_BIN_IMPL", impl)
    _full_check("edges", gpu_device)


@pytest.mark.gpu
def test_binning_tier_edges_through_planned_bins(gpu_device, monkeypatch):
    """Planned bins are never given the no-deferred hint: their second route is uniform bins, bit for bit, as in
    tests/test_gpu_planned_bins.py."""
    import diff_gaussian_rasterization as dgr
    monkeypatch.setattr(dgr, "_BINS_MODE", "uniform")
    uni = _full_check("edges", gpu_device)
    assert not uni["planned"]
    monkeypatch.setattr(dgr, "_BINS_MODE", "planned")
    for _ in range(2):                     # the first planned forward of a view starts from a uniform plan, the next from its own
        pl = _full_check("edges", gpu_device, second=False)
        assert pl["planned"]
        _same_bits(uni, pl)


@pytest.mark.gpu
@pytest.mark.parametrize("name", list(DISCS))
def test_binning_tier_edges_with_more_than_one_tile_row(gpu_device, name):
    """Candidate boxes of 8x8 = 64 | 9x8 = 72 and 32x16 = 512 | 33x16 = 528 tiles: the row / column split of the walk index."""
    _full_check("disc:" + name, gpu_device)


@pytest.mark.gpu
def test_binning_tier_edges_in_a_band_of_tile_rows(gpu_device):
    """Tile rows 2 .. 5 of the 16-row frame: the walk of the 33 x 16 box clipped to 33 x 8.  A band is never given the no-deferred
    hint: its second route is the whole frame, whose rows it must reproduce bit for bit (the band's gradient is another sum)."""
    band = _full_check("disc:33x16", gpu_device, tile_rows=BAND, second=False)
    full = _full_check("disc:33x16", gpu_device)
    rows = slice(16 * BAND[0], 16 * BAND[1])
    assert torch.equal(band["color"][:, rows], full["color"][:, rows]) and torch.equal(band["depth"][:, rows], full["depth"][:, rows])
    gx8 = DISCS["33x16"][0] // 8
    in_band = lambda r: [r["gid"][int(r["offs"][t]): int(r["offs"][t + 1])].tolist() for t in range(2 * BAND[0] * gx8, 2 * BAND[1] * gx8)]
    assert in_band(band) == in_band(full)


@pytest.mark.gpu
def test_more_than_one_round_of_both_deferred_lists(gpu_device):
    """4,200 small-list entries (64 workgroups x 64 a round) and 70 large-list entries (16 workgroups x 4 wavefronts a round)."""
    _full_check("rounds", gpu_device)


@pytest.mark.gpu
@pytest.mark.parametrize("H,tiles", [(2048, 131072), (2056, 131584)])
def test_the_huge_pass_edge(gpu_device, H, tiles):
    """131,072 candidates: one pass of 512 steps; 131,584: a second pass of two steps over the same per-step counts.  The frame is
    too large for the tile-by-tile oracle; the reference is the same composite rule written out for the three splats over the
    whole frame in float64 (front to back, alpha >= 1/255 counted, alpha clamped at 0.99; T never nears the 1e-4 stop), its
    gradients autograd's."""
    dev = gpu_device
    scene, cam = _huge(H)
    sp, strict, _ = _self_check(scene, cam, [tiles, 1, 1])
    W = cam.image_width
    grad_color = _grad_color(cam)
    run = _both_routes(scene, cam, dev, grad_color)
    _check_lists(run, sp, strict)
    # ---- the closed form, in bands of rows ----
    leaves = {k: v.detach().double().clone().requires_grad_(True) for k, v in scene.items()}
    ref_c, ref_d = torch.zeros(3, H, W, dtype=torch.float64), torch.zeros(1, H, W, dtype=torch.float64)
    step = 128
    for y0 in range(0, H, step):
        s = go.preprocess(leaves["means3D"], leaves["means2D"], leaves["opacities"], leaves["scales"], leaves["rotations"], cam)
        y1 = min(y0 + step, H)
        py, px = torch.meshgrid(torch.arange(y0, y1, dtype=torch.float64), torch.arange(W, dtype=torch.float64), indexing="ij")
        T = torch.ones_like(px)
        col, dep = torch.zeros(3, y1 - y0, W, dtype=torch.float64), torch.zeros(y1 - y0, W, dtype=torch.float64)
        for i in torch.argsort(s.zkey).tolist():                   # front to back
            dx, dy = s.xy[i, 0] - px, s.xy[i, 1] - py
            power = -0.5 * (s.conic[i, 0] * dx * dx + s.conic[i, 2] * dy * dy) - s.conic[i, 1] * dx * dy
            a_raw = leaves["opacities"][i, 0] * torch.exp(torch.clamp(power, max=0.0))
            alpha = a_raw + (torch.clamp(a_raw, max=go.ALPHA_MAX) - a_raw).detach()
            a = torch.where((power > 0) | (alpha < go.ALPHA_MIN), torch.zeros_like(alpha), alpha)
            col = col + (a * T)[None] * leaves["colors_precomp"][i][:, None, None]
            dep = dep + a * T * s.depth[i].detach()
            T = T * (1.0 - a)
        assert float(T.detach().min()) > 10 * go.T_STOP
        (col * grad_color[:, y0:y1].double()).sum().backward()
        ref_c[:, y0:y1], ref_d[0, y0:y1] = col.detach(), dep.detach()
    ref_g = {k: leaves[k].grad for k in GRAD_KEYS}
    gx, gy = (W + 15) // 16, (H + 15) // 16
    sorted_gid, offs16 = go.build_tile_lists(sp, gx, gy)
    aux = {"splats": sp, "tile_offsets": offs16, "sorted_gid": sorted_gid}
    taint = _check_images(ref_c, ref_d, run["color"], run["depth"], aux, scene["opacities"], cam)
    _check_grads(ref_g, run["grads"], taint)


@pytest.mark.gpu
@pytest.mark.parametrize("name", list(GATHER_MAPS))
def test_gather_tiers_by_lane(gpu_device, name):
    """Instance counts 0, 1, 4 | 5, 64 | 65 on the first, a middle and the last lane; excess lists that end on a window boundary,
    one record past it and two windows long, their owners apart and the last on lane 63; the whole-wavefront sum beside the
    list; a map that ends inside a wavefront; two workgroups.  Every Gaussian's gradient is checked (2e-3 of the largest; in
    "b_even" and "a_small" every owner is about the same size, so one lost record is far above that)."""
    run = _full_check("gather:" + name, gpu_device)
    _scene_, _cam, want = _gather_strip(name)
    got = torch.bincount(run["gid"], minlength=len(want)).tolist()
    assert got == want


def _frame_params(scene, dev):
    """The scene as the caller chain's parameter dict with an identity camera transform at every time index (as
    tests/test_gpu_forward_bookkeeping.py: logit -> sigmoid and log -> exp move opacity and scale by an ulp, 1e-7 px of reach)."""
    o = scene["opacities"].double()
    p = {"means3D": scene["means3D"], "rgb_colors": scene["colors_precomp"], "unnorm_rotations": scene["rotations"],
         "logit_opacities": torch.log(o / (1 - o)).float(), "log_scales": torch.log(scene["scales"][:, :1]),
         "cam_unnorm_rots": torch.tensor([1.0, 0, 0, 0]).reshape(1, 4, 1).repeat(1, 1, 3), "cam_trans": torch.zeros(1, 3, 3)}
    return {k: torch.nn.Parameter(v.contiguous().to(dev)) for k, v in p.items()}


@pytest.mark.gpu
@pytest.mark.parametrize("contract", [False, True])
@pytest.mark.parametrize("name", list(GATHER_MAPS))
def test_gather_tiers_by_lane_through_render_frame(gpu_device, name, contract):
    """Every one of those maps through the fused frame: records of 14 floats (dual render) and of 12 (get_loss contract, the second image
    differentiated through its first channel) against the unfused chain -- two single renders, whose gather the test above
    holds against the oracle -- at that comparison's bounds (tests/test_gpu_fused_frame.py)."""
    import diff_gaussian_rasterization as dgr
    import slam_callers as sc
    from diff_gaussian_rasterization.fused import render_frame
    dev = gpu_device
    scene, cam, want = _gather_strip(name)
    sp, _, _ = _self_check(scene, cam, want)
    params = _frame_params(scene, dev)
    st = to_settings(cam, dev)
    w2c = torch.eye(4, device=dev)
    g1, g2 = _grad_color(cam, 6).to(dev), _grad_color(cam, 7).to(dev)
    second = lambda ds: ((ds * g2)[:1] if contract else ds * g2).sum()
    tg = sc.transform_to_frame(params, 1, True, True)
    im0, r0, _ = dgr.GaussianRasterizer(raster_settings=st)(**sc.transformed_params2rendervar(params, tg))
    ds0, _, _ = dgr.GaussianRasterizer(raster_settings=st)(**sc.transformed_params2depthplussilhouette(params, w2c, tg))
    ((im0 * g1).sum() + second(ds0)).backward()
    ref = {k: v.grad.clone() for k, v in params.items()}
    for v in params.values():
        v.grad = None
    im1, ds1, r1 = render_frame(params, 1, st, w2c, True, True, get_loss_contract=contract)
    ((im1 * g1).sum() + second(ds1)).backward()
    dgr.settle_pending()
    assert torch.equal(r0, r1) and torch.equal(r1.cpu(), sp.radii)     # (a splat below 1/255 projects too: it has its radius)
    # the images, channel by channel: colour; depth, silhouette, depth squared (the contract form promises only the depth plane to
    # the unfused chain's accuracy: tests/test_gpu_fused_frame.py::test_get_loss_contract_forward_against_the_full_dual_forward)
    for a, b in zip(list(im0) + list(ds0[:1] if contract else ds0), list(im1) + list(ds1[:1] if contract else ds1)):
        assert (a - b).abs().max().item() <= 2e-5 * a.abs().max().item()
    for k, v in params.items():
        err = (ref[k] - v.grad).abs()
        if k == "unnorm_rotations":                     # isotropic: exactly zero in exact arithmetic
            assert err.max().item() <= 1e-4 * ref["log_scales"].abs().max().item()
            continue
        scale = ref[k].abs().max().item()
        row = int(err.reshape(err.shape[0], -1).amax(1).argmax())
        assert err.max().item() <= 2e-3 * scale + 1e-7, (k, err.max().item(), scale, "row", row)
