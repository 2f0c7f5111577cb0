"""Inputs of the raycaster and mesh-extraction edge tests (test_render_edges.py, test_render_edges_gpu.py): the
synthetic room of test_raycast_gpu.py, un-shifted and translated along x until its blocks straddle either end of
the raycaster's LDS block-table key range; render sizes off the 64x8 splat tile and the 16x16 render tile; renders
at and above the height where the tile-row lists are dropped; a camera inside the allocated band; fronto-parallel
walls on and off the cube-corner lattice. NumPy and the library's host-side synthetic stream only: the same
arrays on every machine.

test_render_edges.py checks, with the oracle alone, that each of these inputs reaches the edge it is named for."""
from __future__ import annotations

import numpy as np

import bundlefusion_amd as bfa

FX = 577.87          # the 640x480 sensor's focal length; scaled with the image
VS = 0.01            # voxel size of every volume here
ROOM_FRAMES = (0, 3, 6, 9)
ROOM_W, ROOM_H = 160, 120
RENDER_POSE = 5

# rc_key (raycast.hip) accepts block coordinates in [KEY_LO, KEY_HI]; any other block takes the plain hash probe
KEY_LO, KEY_HI = -4096, 4094
# World offsets along x (metres). The un-shifted room has block x in -19..25, so +327.38 m puts it at 4074..4117
# (across KEY_HI) and -327.98 m at -4118..-4075 (across KEY_LO).
OFFSETS = (0.0, 327.38, -327.98)

# (W, H): smaller than one tile; one render tile + 1; one pixel short of the splat tile; the splat tile; the splat
# tile + 1 (and 64 k + 1 wide); 2 * 64 + 1 wide with a partial splat tile row (25 = 3 * 8 + 1); the room's own size
RENDER_SIZES = [(2, 2), (17, 17), (63, 7), (64, 8), (65, 9), (129, 25), (160, 120)]
# 256 tile rows of 8 pixels: the last height with tile-row lists (row index 255), and the first without them
TALL_SIZES = [(64, 2048), (64, 2056)]
SPLAT_TILE_H = 8

WALL_DEPTHS = (1.0, 1.005)   # off and on the cube-corner lattice ((k + 1/2) voxels)
THRESH_FACTORS = (10.0, 2.0, 1.0, 0.5)


def shifted(T: np.ndarray, offset: float) -> np.ndarray:
    """(G @ T) rounded once to float32, G the translation by offset along x: the pose both sides are given."""
    G = np.eye(4)
    G[0, 3] = offset
    return (G @ np.asarray(T, np.float32)).astype(np.float32)


def room_params():
    return bfa.hash_params(voxel_size=VS, num_buckets=1 << 16, num_blocks=1 << 15)


def room_camera():
    f = FX * ROOM_W / 640.0
    return bfa.depth_camera(ROOM_W, ROOM_H, fx=f, fy=f)


def room_frames(offset: float = 0.0):
    """[(pose, depth, colour)] of the room's four frames: the images are rendered at the un-shifted pose (the
    synthetic scene stays at the origin), the pose handed to the integration is the shifted one."""
    sc, cam = bfa.synth_scene(0), room_camera()
    out = []
    for f in ROOM_FRAMES:
        T = bfa.synth_pose(f)
        d, c = bfa.synth_render_host(sc, T, cam, 1, f)
        out.append((shifted(T, offset), d, c))
    return out


def view(W: int, H: int, by_height: bool = False, **rp_opts):
    """(cam, rp) for a W x H render, the focal length scaled with the width (tall renders: with the height)."""
    f = FX * H / 480.0 if by_height else FX * W / 640.0
    return bfa.depth_camera(W, H, fx=f, fy=f), bfa.raycast_params(W, H, fx=f, fy=f, **rp_opts)


def render_pose(offset: float = 0.0) -> np.ndarray:
    return shifted(bfa.synth_pose(RENDER_POSE), offset)


def inside_pose() -> np.ndarray:
    """The render pose moved 1.5 m along its own viewing axis: the camera stands inside the allocated band, so
    blocks reach in front of the near plane."""
    T = bfa.synth_pose(RENDER_POSE).copy()
    T[:3, 3] += np.float32(1.5) * T[:3, 2]
    return T


def intervals(rmin: np.ndarray, rmax: np.ndarray, rp):
    """(no-ray mask, lo, hi) of the raw splat outputs, as render_pixel reads them: no ray where either is 0 or
    -inf, else the interval clamped to [minDepth, maxDepth]; lo / hi are 0 where there is no ray."""
    no_ray = (rmin == 0) | np.isneginf(rmin) | (rmax == 0) | np.isneginf(rmax)
    lo = np.where(no_ray, np.float32(0), np.maximum(rmin, np.float32(rp.minDepth))).astype(np.float32)
    hi = np.where(no_ray, np.float32(0), np.minimum(rmax, np.float32(rp.maxDepth))).astype(np.float32)
    return no_ray, lo, hi


def clamped(rmin: np.ndarray, rmax: np.ndarray, rp):
    """Pixels whose raw interval ends beyond a clip plane (where the oracle's clamped depth test can tie)."""
    near = np.isfinite(rmin) & (rmin != 0) & (rmin < np.float32(rp.minDepth))
    far = np.isfinite(rmax) & (rmax > np.float32(rp.maxDepth))
    return near, far


def keyed(blocks: np.ndarray) -> np.ndarray:
    """Which of the int [n, 3] block coordinates rc_key accepts."""
    b = np.asarray(blocks)[:, :3]
    return np.all((b >= KEY_LO) & (b <= KEY_HI), axis=1)


def block_box(block, pad: float = 0.0):
    """(minCorner, maxCorner): the float32 centres of the block's first and last voxel (virtualVoxelPosToWorld:
    float(v) * voxelSize), optionally padded by a fraction of a voxel."""
    b = np.asarray(block[:3], np.int64)
    vs = np.float32(VS)
    lo = (b * 8).astype(np.float32) * vs
    hi = (b * 8 + 7).astype(np.float32) * vs
    p = np.float32(pad) * vs
    return lo - p, hi + p


def on_corner_lattice(z: np.ndarray) -> np.ndarray:
    """Whether each float32 coordinate is exactly a cube corner's: float(k) * voxelSize -+ voxelSize / 2 for the
    voxel k on either side (the corner positions extractIsoSurfaceAtPosition builds)."""
    z = np.asarray(z, np.float32)
    vs, half = np.float32(VS), np.float32(VS) / np.float32(2)
    k = np.floor(z.astype(np.float64) / VS).astype(np.int64)
    ok = np.zeros(z.shape, bool)
    for dk in (-1, 0, 1, 2):
        c = (k + dk).astype(np.float32) * vs
        ok |= (c + half == z) | (c - half == z)
    return ok
