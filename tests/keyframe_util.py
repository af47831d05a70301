"""Shared by the keyframe-selection tests: the cases of tests/golden/keyframes.npz, the float32 restatement of the reference's
per-pair masks in its own operation order (utils/keyframe_selection.py:10-37, 64-88, 154-188), the float64 restatement
with the signed margin of every comparison, and the decision band tau measured from the two."""
import os

import numpy as np
import torch
import torch.nn.functional as F

HERE = os.path.dirname(os.path.abspath(__file__))
EPS32 = 2.0 ** -23
BAND_SHARE = 0.005              # pairs inside the band: at most 0.5 % of a case's pairs
_cache = {}


def fixture():
    if "fx" not in _cache:
        z = np.load(os.path.join(HERE, "golden", "keyframes.npz"))
        _cache["fx"] = {k: (z[k] if z[k].ndim else z[k].item()) for k in z.files}
    return _cache["fx"]


def counts_of(ids, percent, n):
    """Counts by keyframe id from a stored save_percent list: exactly round(percent * n)."""
    c = np.zeros(len(ids), dtype=np.int64)
    if n:
        c[np.asarray(ids)] = np.rint(np.asarray(percent, dtype=np.float64) * n).astype(np.int64)
    return c


def cases():
    """name -> dict(gt_depth [1,H,W], k, w2c, kf_w2c [K,4,4], kf_depth [K,H,W], edge, thresh (None: no visibility test),
    rc (None: dense), n, counts [K] by keyframe id)."""
    if "cases" in _cache:
        return _cache["cases"]
    fx = fixture()
    out = {}

    def add(name, s, thresh, rc, n, ids, pct):
        out[name] = dict(gt_depth=fx[s + "_gt_depth"], k=fx[s + "_k"], w2c=fx[s + "_w2c"], kf_w2c=fx[s + "_kf_w2c"],
                         kf_depth=fx[s + "_kf_depth"], edge=int(fx[s + "_edge"]), thresh=thresh, rc=rc, n=int(n),
                         counts=counts_of(ids, pct, int(n)), ids=ids, percent=pct)
    add("a_t001", "a", fx["a_t001_thresh"], None, fx["a_dense_n"], fx["a_t001_ids"], fx["a_t001_percent"])
    add("a_t005", "a", fx["a_t005_thresh"], None, fx["a_dense_n"], fx["a_t005_ids"], fx["a_t005_percent"])
    add("a_sampled", "a", None, fx["a_sampled_rc"], fx["a_sampled_n"], fx["a_sampled_ids"], fx["a_sampled_percent"])
    add("b", "b", fx["b_thresh"], None, fx["b_n"], fx["b_ids"], fx["b_percent"])
    add("d", "d", fx["d_thresh"], None, fx["d_n"], fx["d_ids"], fx["d_percent"])
    add("d_sampled", "d", None, fx["d_sampled_rc"], fx["d_sampled_n"], fx["d_sampled_ids"], fx["d_sampled_percent"])
    _cache["cases"] = out
    return out


def sources(c):
    """[S, 2] int64 (row, col): the stored draw, or every valid-depth pixel in row-major order."""
    if c.get("rc") is not None:
        return torch.as_tensor(c["rc"]).long()
    return torch.stack(torch.where(torch.as_tensor(c["gt_depth"])[0] > 0), dim=1)


def kept_rule(c, rc=None):
    """The native drop rule on float32 points formed as the reference forms them: (points [S,3] float32, kept [S] bool) --
    a sample is dropped with ALL copies of a repeated index, or when its point rounds to the origin."""
    rc = sources(c) if rc is None else rc
    depth, k, w2c = (torch.as_tensor(c[n], dtype=torch.float32) for n in ("gt_depth", "k", "w2c"))
    xx = (rc[:, 1] - k[0][2]) / k[0][0]
    yy = (rc[:, 0] - k[1][2]) / k[1][1]
    z = depth[0, rc[:, 0], rc[:, 1]]
    pc = torch.stack((xx * z, yy * z, z), dim=-1)
    p4 = torch.cat([pc, torch.ones_like(pc[:, :1])], dim=1)
    pts = (torch.inverse(w2c) @ p4.T).T[:, :3]
    _, inv, cnt = torch.unique(rc, dim=0, return_inverse=True, return_counts=True)
    origin = (torch.abs(torch.round(pts, decimals=4)) == 0).all(dim=1)
    return pts, ~(cnt[inv] > 1) & ~origin


def masks_f32(c):
    """[K, S] bool: in & vis of every (keyframe, source) pair in float32 with the reference's operations in its order, False
    for a dropped source; and kept [S]."""
    pts_all, kept = kept_rule(c)
    pts = pts_all[kept]
    k = torch.as_tensor(c["k"], dtype=torch.float32)
    H, W = c["gt_depth"].shape[-2:]
    edge = c["edge"]
    out = torch.zeros(len(c["kf_w2c"]), pts_all.shape[0], dtype=torch.bool)
    for j in range(len(c["kf_w2c"])):
        est = torch.as_tensor(c["kf_w2c"][j], dtype=torch.float32)
        p4 = torch.cat([pts, torch.ones_like(pts[:, :1])], dim=1)
        tp = (est @ p4.T).T[:, :3]
        p2 = torch.matmul(k, tp.transpose(0, 1)).transpose(0, 1)
        pz = p2[:, 2:] + 1e-5
        p2 = p2 / pz
        pr = p2[:, :2]
        m = (pr[:, 0] < W - edge) * (pr[:, 0] > edge) * (pr[:, 1] < H - edge) * (pr[:, 1] > edge)
        m = m & (pz[:, 0] > 0)
        if c["thresh"] is not None:
            d = torch.as_tensor(c["kf_depth"][j], dtype=torch.float32).reshape(1, 1, H, W)
            grid = pr.reshape(1, 1, -1, 2).clone()
            grid[..., 0] = grid[..., 0] / (W - 1) * 2.0 - 1.0
            grid[..., 1] = grid[..., 1] / (H - 1) * 2.0 - 1.0
            ds = F.grid_sample(d, grid, padding_mode="zeros", align_corners=True).reshape(-1)
            m = m & (torch.abs(ds - pz[:, 0]) < c["thresh"] * torch.min(ds, pz[:, 0]))
        out[j, kept] = m
    return out, kept


def _bilinear64(img, u, v):
    H, W = img.shape
    x0, y0 = torch.floor(u), torch.floor(v)
    out = torch.zeros_like(u)
    for dx in (0, 1):
        for dy in (0, 1):
            x, y = (x0 + dx).long(), (y0 + dy).long()
            w = (1 - (u - (x0 + dx)).abs()) * (1 - (v - (y0 + dy)).abs())
            ok = (x >= 0) & (x < W) & (y >= 0) & (y < H)
            out += torch.where(ok, img[y.clamp(0, H - 1), x.clamp(0, W - 1)] * w, torch.zeros_like(u))
    return out


def masks_f64(c, rc=None, kf_w2c=None, kf_depth=None, edge=None, thresh="case"):
    """float64: mask [K, S] (True = in & vis, meaningful for kept sources) and band margin [K, S]: the smallest |margin| over
    the comparisons that can flip the pair -- the four edge tests relative to the image extent, z' > 0 and the visibility
    test relative to |z'| (the visibility test only where the pair is inside the image or within the same distance of its
    edge: elsewhere it decides nothing)."""
    rc = sources(c) if rc is None else rc
    kf_w2c = c["kf_w2c"] if kf_w2c is None else kf_w2c
    kf_depth = c["kf_depth"] if kf_depth is None else kf_depth
    edge = c["edge"] if edge is None else edge
    thresh = c["thresh"] if thresh == "case" else thresh
    depth, k, w2c = (torch.as_tensor(c[n], dtype=torch.float64) for n in ("gt_depth", "k", "w2c"))
    H, W = depth.shape[-2:]
    z = depth[0, rc[:, 0], rc[:, 1]]
    pc = torch.stack(((rc[:, 1] - k[0, 2]) / k[0, 0] * z, (rc[:, 0] - k[1, 2]) / k[1, 1] * z, z, torch.ones_like(z)), dim=-1)
    pts = (torch.inverse(w2c) @ pc.T).T
    masks, margins = [], []
    for j in range(len(kf_w2c)):
        q = (k @ (torch.as_tensor(kf_w2c[j], dtype=torch.float64) @ pts.T)[:3]).T
        zp = q[:, 2] + 1e-5
        u, v = q[:, 0] / zp, q[:, 1] / zp
        geo = torch.stack(((W - edge - u) / W, (u - edge) / W, (H - edge - v) / H, (v - edge) / H, zp / zp.abs().clamp(min=1.0)))
        inside = (geo > 0).all(dim=0)
        margin = geo.abs().min(dim=0).values
        m = inside
        if thresh is not None:
            d = _bilinear64(torch.as_tensor(kf_depth[j], dtype=torch.float64), u, v)
            mv = (thresh * torch.minimum(d, zp) - (d - zp).abs()) / zp.abs().clamp(min=1e-12)
            m = m & (mv > 0)
            margin = torch.where(inside, torch.minimum(margin, mv.abs()), margin)
        masks.append(m)
        margins.append(margin)
    return torch.stack(masks), torch.stack(margins)


def measure_tau():
    """(tau, largest margin at which the fixture's own float32 masks disagree with the float64 masks, floor): tau = 4 x
    that margin, with a floor of 4 float32 ulps of the largest projected coordinate (margins are relative to the image
    extent, of which an in-image coordinate is at most 1)."""
    if "tau" not in _cache:
        worst = 0.0
        for c in cases().values():
            m32, kept = masks_f32(c)
            m64, margin = masks_f64(c)
            diff = (m32 != m64) & kept[None]
            if diff.any():
                worst = max(worst, float(margin[diff].max()))
        floor = 4 * EPS32
        _cache["tau"] = (max(4 * worst, floor), worst, floor)
    return _cache["tau"]
