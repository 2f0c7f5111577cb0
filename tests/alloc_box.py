"""Host restatement of the alloc walk's ray end points (oracle/tsdf.cpp allocPixelWalk up to `idEnd`), in
float32 and in the oracle's operation order, and of the block boxes the walk's pre-test derives from them:
per ray the box spanned by the block of rayMin and the block of rayMax, per 16x16-pixel tile the union of
its active rays' boxes."""
from __future__ import annotations

import numpy as np

TILE = 16
BOX_MAX = 256  # ALLOC_BOX_MAX (bundlefusion_amd/csrc/tsdf.hip)
F = np.float32


def ray_ends(T, depth, cam, params, want_points=False):
    """(active [H, W] bool, id [H, W, 3], idEnd [H, W, 3]) of every pixel's ray; with want_points also the
    world end points rayMin, rayMax (float32 [H, W, 3]) the blocks were taken from."""
    H, W = cam.imageHeight, cam.imageWidth
    d = np.asarray(depth, F).reshape(H, W)
    maxd, tr, ts, vs = F(params.maxIntegrationDistance), F(params.truncation), F(params.truncScale), F(params.virtualVoxelSize)
    with np.errstate(invalid="ignore", over="ignore"):
        active = ~((d == -np.inf) | (d == 0)) & ~(d >= maxd)
        dd = np.where(active, d, F(1.0)).astype(F)
        t = (tr + ts * dd).astype(F)
        lo = np.minimum(maxd, (dd - t).astype(F)).astype(F)
        hi = np.minimum(maxd, (dd + t).astype(F)).astype(F)
        active &= ~(lo >= hi)
        cx = ((np.arange(W, dtype=F) - F(cam.mx)) / F(cam.fx)).astype(F)[None, :]
        cy = ((np.arange(H, dtype=F) - F(cam.my)) / F(cam.fy)).astype(F)[:, None]
        e = np.asarray(T, F).reshape(4, 4)

        def block(depth_):
            v = [(depth_ * cx).astype(F), (depth_ * cy).astype(F), depth_]
            out, pts = [], []
            for r in range(3):
                w = (((e[r, 0] * v[0]).astype(F) + (e[r, 1] * v[1]).astype(F)).astype(F) + (e[r, 2] * v[2]).astype(F)).astype(F)
                w = (w + (e[r, 3] * F(1.0))).astype(F)
                pts.append(np.broadcast_to(w, d.shape))
                p = (w / vs).astype(F)
                q = (p + np.sign(p).astype(F) * F(0.5)).astype(F)
                out.append(np.floor_divide(np.trunc(q).astype(np.int64), 8))  # v < 0: (v - 7) / 8 truncated
            return np.stack(out, axis=-1), np.stack(pts, axis=-1)

        (b0, p0), (b1, p1) = block(lo), block(hi)
        return (active, b0, b1, p0, p1) if want_points else (active, b0, b1)


def ray_boxes(active, b0, b1):
    """per pixel (lo [H, W, 3], hi [H, W, 3]); inactive rays get an empty box"""
    big = np.iinfo(np.int64).max
    lo = np.where(active[..., None], np.minimum(b0, b1), big)
    hi = np.where(active[..., None], np.maximum(b0, b1), -big)
    return lo, hi


def tile_boxes(active, b0, b1):
    """{(tx, ty): (lo [3], hi [3])} over the tiles with an active ray"""
    lo, hi = ray_boxes(active, b0, b1)
    H, W = active.shape
    out = {}
    for ty in range(-(-H // TILE)):
        for tx in range(-(-W // TILE)):
            sl = (slice(ty * TILE, (ty + 1) * TILE), slice(tx * TILE, (tx + 1) * TILE))
            if active[sl].any():
                out[(tx, ty)] = (lo[sl].reshape(-1, 3).min(axis=0), hi[sl].reshape(-1, 3).max(axis=0))
    return out


def predict_pretest(T, depth, cam, params, present, shard=None) -> dict:
    """What the pre-test does with one integrate op on a scene holding the blocks `present` (a set of
    (x, y, z)): tiles it ends (box within the limit, every block present), tiles that walk, and those of
    the latter whose box is over the limit. shard = (count, index, chunk): only this rank's blocks count."""
    from bundlefusion_amd.dist import chunk_owner

    def mine(b):
        return shard is None or chunk_owner(*b, params.virtualVoxelSize, shard[0], chunk=shard[2]) == shard[1]
    res = {"skipped": 0, "walked": 0, "overLimit": 0}
    for lo, hi in tile_boxes(*ray_ends(T, depth, cam, params)).values():
        n = hi - lo + 1
        if np.all(n <= BOX_MAX) and int(n[0]) * int(n[1]) * int(n[2]) <= BOX_MAX:
            full = all((x, y, z) in present or not mine((x, y, z)) for x in range(lo[0], hi[0] + 1) for y in range(lo[1], hi[1] + 1)
                       for z in range(lo[2], hi[2] + 1))
            res["skipped" if full else "walked"] += 1
        else:
            res["walked"] += 1
            res["overLimit"] += 1
    return res
