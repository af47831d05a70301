"""Keyframe / base-frame overlap selection on the device (csrc/vtgs_keyframes.hip): all keyframes in one pass.

    from diff_gaussian_rasterization.keyframes import (keyframe_selection_overlap, keyframe_selection_overlap_visbased,
        keyframe_selection_overlap_visbased_earliest_dynamic_new_topkbase, find_earliest_keyframe)

replaces the same four names of the reference's utils/keyframe_selection.py (:40-116, :121-229, :581-724, :1581-1613) with
their signatures and return values.  Each accepts, in the `keyframe_list` position, the reference's list of dicts
('est_w2c', 'depth') -- uploaded for the call, never mutated or moved -- or a `KeyframeStore`, which keeps the depth maps and
poses resident on the device.  One launch sequence and ONE host read (k + 3 integers) per call; the selection logic itself
lives in the pure functions `select_overlap`, `select_visbased`, `select_topkbase` and `walk_earliest`.  No prints.

Two documented deviations from the reference:
  * its get_pointcloud also drops two DIFFERENT pixels whose |rounded| world coordinates coincide (an accident of the
    unique() call that removes points at the camera origin); this module drops only repeated sample indices -- in all their
    copies, as the reference does -- and points that round to the origin;
  * find_earliest_keyframe draws its sample ONCE and counts every link of the chain in one launch; the reference draws
    afresh for every link.
An EMPTY keyframe list gives what the reference gives: [] from keyframe_selection_overlap (with or without save_percent),
([], []) / [] from the visbased form, and an IndexError from the topkbase form and from a find_earliest_keyframe whose
chain has a link (the reference indexes the empty list there); nothing is launched.
With `sampled_indices=None` the sampled forms draw torch.randint over the valid-depth pixels as the reference does (that
torch.where is a host wait of its own; pass `sampled_indices` to avoid it).  HIP only: no CPU path for the counting.
"""
from __future__ import annotations

import ctypes

import numpy as np
import torch

from . import _I32, _P, _SZ, _check, _lib, _stream_ptr

__all__ = ["KeyframeStore", "overlap_counts", "keyframe_selection_overlap", "keyframe_selection_overlap_visbased",
           "keyframe_selection_overlap_visbased_earliest_dynamic_new_topkbase", "find_earliest_keyframe",
           "select_overlap", "select_visbased", "select_topkbase", "walk_earliest", "percents", "resolve_chain"]

_F = ctypes.c_float
_lib.vtgs_keyframe_overlap_scratch_bytes.restype, _lib.vtgs_keyframe_overlap_scratch_bytes.argtypes = _SZ, [_I32] * 4
_lib.vtgs_keyframe_overlap.restype = ctypes.c_int
_lib.vtgs_keyframe_overlap.argtypes = [_I32, _I32, _P, _P, _P, _P, _I32, _P, _P, _P, _I32, _F, _F, _P, _P, _SZ, _P, _P]

MAX_SAMPLES = 16384


# ---- the selection logic: pure functions of the counts (no GPU, no library) ---------------------------------------------------
def percents(counts, n):
    """count / n in float32, the reference's `mask.sum() / projected_pts.shape[0]`; n == 0 gives NaN for every keyframe."""
    c = np.asarray(counts, dtype=np.int64).astype(np.float32)
    with np.errstate(invalid="ignore", divide="ignore"):
        return c / np.float32(n)


def _sorted_desc(p):
    """[(id, percent)] in the order of the reference's stable `sorted(..., reverse=True)` (NaN compares false: order kept)."""
    return sorted(enumerate(p), key=lambda e: e[1], reverse=True)


def select_overlap(counts, n, k):
    """keyframe_selection_overlap's return: the ids with percent > 0 by descending percent, the first k."""
    sel = [i for i, p in _sorted_desc(percents(counts, n)) if p > 0.0]
    return list(np.array(sel)[:k])


def select_visbased(counts, n, k, earliest_thres):
    """keyframe_selection_overlap_visbased's return tuple (selected, earliest_selected)."""
    order = _sorted_desc(percents(counts, n))
    sel = list(np.array([i for i, p in order if p > 0.0])[:k])
    earliest = list(np.array([i for i, p in order if p > np.float32(earliest_thres)])[-1:])
    return sel, (earliest if len(earliest) else sel)


def _quantize(ids, per_base):
    return list(set(int(i / per_base) for i in ids))


def select_topkbase(counts, n, config, earliest_thres, lower_earliest_thres_percent, topk_base):
    """keyframe_selection_overlap_visbased_earliest_dynamic_new_topkbase's return: the earliest base frames whose keyframes
    overlap by more than a threshold that is lowered until three base frames pass (or it falls under 0.01); the last
    keyframe alone when none does."""
    p = percents(counts, n)
    order = _sorted_desc(p)
    per_base = int(config["baseframe_every"] / config["overlap_every"])
    thres, first = earliest_thres, True
    while True:
        thres = thres if first else lower_earliest_thres_percent * thres
        first = False
        kept = [i for i, q in order if q > np.float32(thres)]
        bases = sorted(_quantize(kept, per_base))
        if len(bases) >= 3 or (len(order) <= 3 * per_base and len(bases) > 0) or thres < 0.01:
            break
    if not kept:
        kept = [len(p) - 1]
    kept = sorted(kept)
    if topk_base is None:
        return sorted(_quantize(kept[:1], per_base))
    bases = sorted(_quantize(kept, per_base))
    return bases[:min(topk_base, len(bases))]


def resolve_chain(corr_list):
    """find_earliest_keyframe's walk without its threshold: (start keyframe, current frame, the candidate keyframe ids in
    the order they are tested).  Pure index arithmetic on corr_list = [[keyframe, latest, current], ...].  A chain that
    returns to an id it already holds ends there (the reference would not terminate on one)."""
    rev = corr_list[::-1]
    start, frame = rev[0][0], rev[0][2]
    chain, cur = [], start
    while cur >= 0:
        cur = next((i for i, _, x in rev if x == cur), -100)
        if cur < 0 or cur in chain:
            break
        chain.append(cur)
    return start, frame, chain


def walk_earliest(corr_list, counts_by_keyframe, n, baseframe_every, threshold):
    """find_earliest_keyframe's return [earliest_keyframe, None, current_frame_idx]; counts_by_keyframe[int(id /
    baseframe_every)] is the overlap count of that entry of the keyframe list, n the common denominator."""
    start, frame, chain = resolve_chain(corr_list)
    earliest = start
    for cur in chain:
        p = percents([counts_by_keyframe[int(cur / baseframe_every)]], n)[0]
        if float(p) > threshold:
            earliest = cur
        else:
            break
    return [earliest, None, frame]


# ---- the resident keyframes ----------------------------------------------------------------------------------------------------
class KeyframeStore:
    """Depth maps [cap, H, W] and world-to-camera poses [cap, 16] of the keyframes, float32, resident on the device; grows by
    doubling.  `append` returns the slot, which is the keyframe's index in the reference's list."""

    def __init__(self, height: int, width: int, capacity: int = 64, device=None):
        if height <= 0 or width <= 0 or capacity <= 0:
            raise ValueError("KeyframeStore needs positive sizes")
        self.device = torch.device("cuda", torch.cuda.current_device()) if device is None else torch.device(device)
        if self.device.type != "cuda":
            raise RuntimeError("KeyframeStore lives on a HIP device (torch 'cuda'); no CPU path exists")
        self.height, self.width = int(height), int(width)
        self.depth = torch.zeros(capacity, self.height, self.width, dtype=torch.float32, device=self.device)
        self.w2c = torch.zeros(capacity, 16, dtype=torch.float32, device=self.device)
        self._n = 0

    def __len__(self):
        return self._n

    @property
    def capacity(self):
        return self.depth.shape[0]

    def _grow(self):
        cap = self.capacity
        depth = torch.zeros(2 * cap, self.height, self.width, dtype=torch.float32, device=self.device)
        w2c = torch.zeros(2 * cap, 16, dtype=torch.float32, device=self.device)
        depth[:cap].copy_(self.depth)
        w2c[:cap].copy_(self.w2c)
        self.depth, self.w2c = depth, w2c

    def append(self, est_w2c, depth) -> int:
        depth = torch.as_tensor(depth)
        if depth.numel() != self.height * self.width:
            raise ValueError(f"keyframe depth must hold {self.height} x {self.width} values")
        if self._n == self.capacity:
            self._grow()
        slot = self._n
        self.depth[slot].copy_(depth.detach().reshape(self.height, self.width))
        self._n += 1
        self.set_pose(slot, est_w2c)
        return slot

    def set_pose(self, slot: int, w2c) -> None:
        if not 0 <= slot < self._n:
            raise IndexError(f"slot {slot} of a store of {self._n} keyframes")
        w2c = torch.as_tensor(w2c)
        if w2c.numel() != 16:
            raise ValueError("a pose is a 4 x 4 world-to-camera matrix")
        self.w2c[slot].copy_(w2c.detach().reshape(16))

    @classmethod
    def from_list(cls, keyframe_list, device=None, capacity=None):
        """The reference's keyframe list ('est_w2c' [4,4], 'depth' [1,H,W] or [H,W] per entry) as a store; the list and its
        tensors are left as they are."""
        if not len(keyframe_list):
            raise ValueError("from_list needs at least one keyframe (the image size comes from its depth)")
        h, w = keyframe_list[0]["depth"].shape[-2:]
        store = cls(h, w, capacity or max(1, len(keyframe_list)), device)
        for kf in keyframe_list:
            store.append(kf["est_w2c"], kf["depth"])
        return store


def _as_store(keyframes, dev):
    return keyframes if isinstance(keyframes, KeyframeStore) else KeyframeStore.from_list(keyframes, dev)


def _f32(t, dev):
    return torch.as_tensor(t).detach().to(device=dev, dtype=torch.float32).contiguous()


def overlap_counts(gt_depth, w2c, intrinsics, store: KeyframeStore, slots=None, sampled_indices=None, edge_value=20,
                   kf_depth_thresh=None, _pair_mask=None) -> torch.Tensor:
    """vtgs_keyframe_overlap (include/vtgs.h) on the current stream, no host wait.  Returns the device int32 record
    [k + 3]: counts per selected keyframe, kept points n, valid-depth sources, dropped (repeats + origin points).
    `slots`: keyframe indices to count (may repeat; None = all of the store, in order).  `sampled_indices` [S, 2] (row,
    col), 1 <= S <= 16384, or None = every valid-depth pixel.  `kf_depth_thresh` None: no visibility test."""
    if not isinstance(gt_depth, torch.Tensor) or not gt_depth.is_cuda:
        raise RuntimeError("overlap_counts needs tensors on a HIP device (torch 'cuda'); no CPU path exists")
    dev = gt_depth.device
    if store.device != dev:
        raise ValueError(f"the store lives on {store.device}, the frame on {dev}")
    gd = _f32(gt_depth, dev)
    H, W = gd.shape[-2], gd.shape[-1]
    if gd.numel() != H * W or (H, W) != (store.height, store.width):
        raise ValueError(f"gt_depth must be [1,H,W] / [H,W] of the store's {store.height} x {store.width}")
    kmat = _f32(intrinsics, dev)[:3, :3].contiguous()
    pose = _f32(w2c, dev).reshape(16)
    sl = None
    if slots is None:
        k = len(store)
    else:
        if isinstance(slots, torch.Tensor) and slots.is_cuda:
            sl = slots.to(torch.int32).contiguous()          # resident slots are the caller's promise: rows < len(store)
        else:
            host = [int(s) for s in (slots.tolist() if isinstance(slots, torch.Tensor) else slots)]
            if any(s < 0 or s >= len(store) for s in host):
                raise IndexError(f"slots {host} outside a store of {len(store)} keyframes")
            sl = torch.tensor(host, dtype=torch.int32).to(dev)
        k = sl.numel()
    if k <= 0:
        raise ValueError("overlap_counts needs at least one keyframe")
    rc, samples = None, 0
    if sampled_indices is not None:
        rc = torch.as_tensor(sampled_indices).detach().to(device=dev, dtype=torch.int32).contiguous()
        if rc.dim() != 2 or rc.shape[1] != 2 or not 1 <= rc.shape[0] <= MAX_SAMPLES:
            raise ValueError(f"sampled_indices must be [S, 2] (row, col) with 1 <= S <= {MAX_SAMPLES}")
        samples = rc.shape[0]
    sbytes = int(_lib.vtgs_keyframe_overlap_scratch_bytes(W, H, samples, k))
    scratch = torch.empty(sbytes, dtype=torch.uint8, device=dev)
    record = torch.empty(k + 3, dtype=torch.int32, device=dev)
    p = lambda x: None if x is None else x.data_ptr()
    vis = kf_depth_thresh is not None
    _check(_lib.vtgs_keyframe_overlap(W, H, gd.data_ptr(), kmat.data_ptr(), pose.data_ptr(), p(rc), samples, store.w2c.data_ptr(),
                                      store.depth.data_ptr() if vis else None, p(sl), k, float(edge_value),
                                      float(kf_depth_thresh) if vis else 0.0, p(_pair_mask), scratch.data_ptr(), sbytes,
                                      record.data_ptr(), _stream_ptr(dev)), "vtgs_keyframe_overlap")
    return record


def _draw(gt_depth, pixels):
    """The reference's draw: torch.randint (host generator, with replacement) over the valid-depth pixels."""
    valid = torch.stack(torch.where(gt_depth[0] > 0), dim=1)
    if valid.shape[0] == 0:
        raise ValueError("the frame has no valid-depth pixel to sample")       # (the reference's randint raises here too)
    return valid[torch.randint(valid.shape[0], (pixels,)).to(valid.device)]


def _percent_dicts(record, host):
    """The reference's save_percent list: 0-dim float32 device tensors count / n, stable descending order."""
    k = record.numel() - 3
    dev_p = record[:k].to(torch.float32) / record[k].to(torch.float32)
    order = _sorted_desc(percents(host[:k], host[k]))
    return [{"id": i, "percent_inside": dev_p[i]} for i, _ in order]


def keyframe_selection_overlap(gt_depth, w2c, intrinsics, keyframe_list, k, pixels=1600, edge_value=20, save_percent=False,
                               sampled_indices=None):
    if len(keyframe_list) == 0:
        return []
    dev = gt_depth.device
    store = _as_store(keyframe_list, dev)
    if sampled_indices is None:
        sampled_indices = _draw(gt_depth, pixels)
    record = overlap_counts(gt_depth, w2c, intrinsics, store, sampled_indices=sampled_indices, edge_value=edge_value)
    host = record.cpu().numpy()                                               # the one host read
    if save_percent:
        return _percent_dicts(record, host)
    return select_overlap(host[:-3], host[-3], k)


def keyframe_selection_overlap_visbased(gt_depth, w2c, intrinsics, keyframe_list, k, pixels=1600, edge_value=20,
                                        save_percent=False, kf_depth_thresh=0.01, earliest_thres=0.5, sampled_indices=None):
    """Dense: every valid-depth pixel (`pixels` and `sampled_indices` are ignored, as the reference ignores `pixels`)."""
    if len(keyframe_list) == 0:
        return [] if save_percent else ([], [])
    store = _as_store(keyframe_list, gt_depth.device)
    record = overlap_counts(gt_depth, w2c, intrinsics, store, edge_value=edge_value, kf_depth_thresh=kf_depth_thresh)
    host = record.cpu().numpy()
    if save_percent:
        return _percent_dicts(record, host)
    return select_visbased(host[:-3], host[-3], k, earliest_thres)


def keyframe_selection_overlap_visbased_earliest_dynamic_new_topkbase(gt_depth, w2c, intrinsics, keyframe_list, k, config,
                                                                      pixels=1600, edge_value=20, kf_depth_thresh=0.01,
                                                                      earliest_thres=0.5, lower_earliest_thres_percent=0.8,
                                                                      topk_base=3, sampled_indices=None):
    """Dense, like the visbased form; returns the earliest base-frame ids."""
    if len(keyframe_list) == 0:
        raise IndexError("keyframe list is empty (the reference takes its last entry)")
    store = _as_store(keyframe_list, gt_depth.device)
    record = overlap_counts(gt_depth, w2c, intrinsics, store, edge_value=edge_value, kf_depth_thresh=kf_depth_thresh)
    host = record.cpu().numpy()
    return select_topkbase(host[:-3], host[-3], config, earliest_thres, lower_earliest_thres_percent, topk_base)


def find_earliest_keyframe(corr_list, gt_depth, w2c, intrinsics, keyframe_list, k, edge_value, baseframe_every, threshold,
                           pixels=1600, sampled_indices=None):
    """The chain is resolved on the host first; ONE launch counts all its links with ONE shared draw (the reference draws
    afresh per link), then the chain is walked over the counts."""
    start, frame, chain = resolve_chain(corr_list)
    if not chain:
        return [start, None, frame]
    if len(keyframe_list) == 0:
        raise IndexError("keyframe list is empty but the chain has a link")
    store = _as_store(keyframe_list, gt_depth.device)
    if sampled_indices is None:
        sampled_indices = _draw(gt_depth, pixels)
    slots = [int(c / baseframe_every) for c in chain]
    record = overlap_counts(gt_depth, w2c, intrinsics, store, slots=slots, sampled_indices=sampled_indices,
                            edge_value=edge_value)
    host = record.cpu().numpy()
    return walk_earliest(corr_list, dict(zip(slots, host[:-3])), host[-3], baseframe_every, threshold)
