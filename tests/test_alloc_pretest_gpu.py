"""The alloc walk's pre-test (a tile all of whose box blocks exist ends before the DDA) against the CPU
oracle: the same ops run on a scene with the pre-test, on one with it switched off
(BF_SCENE_TEST_ALLOC_NO_PRETEST) and on the oracle; block sets and voxels must be bit-identical, the
candidate counts of the two GPU scenes equal, and the pre-test's tile counters what tests/alloc_box.py
predicts from the oracle's block set before each batch (every integrate op of a batch walks the hash as
it stood before the batch).

72x56 images (4.5 x 3.5 tiles: the right and bottom tiles are partial) at the full-resolution focal
length, so a pixel covers a few millimetres as in the 640x480 stream, and 4 mm voxels."""
import numpy as np
import pytest

import bundlefusion_amd as bfa
from alloc_box import predict_pretest, ray_ends, tile_boxes
from bundlefusion_amd.abi import BF_SCENE_TEST_ALLOC_DIRECT, BF_SCENE_TEST_ALLOC_NO_PRETEST
from oracle_lib import OracleScene, blocks_of
from tsdf_compare import compare_states

pytestmark = pytest.mark.gpu

W, H = 72, 56
KEYS = ("skipped", "walked", "overLimit")


def make_cam():
    return bfa.depth_camera(W, H, fx=577.87, fy=577.87)


def make_params():
    return bfa.hash_params(voxel_size=0.004, num_buckets=1 << 14, num_blocks=1 << 13)


@pytest.fixture(scope="module")
def scene():
    return bfa.synth_scene(0)


def shifted(T, dx=0.0, dy=0.0, dz=0.0):
    T2 = np.array(T, np.float32)
    T2[:3, 3] += T2[:3, :3] @ np.array([dx, dy, dz], np.float32)  # along the camera's own axes
    return T2


def frame(scene, cam, f, T=None):
    T = bfa.synth_pose(f) if T is None else T
    d, c = bfa.synth_render_host(scene, T, cam, 1, f)
    return T, d, c


class Rig:
    """GPU scenes (one per test-flag word) and the oracle, driven with identical batches."""

    def __init__(self, p, cam, flags=(0, BF_SCENE_TEST_ALLOC_NO_PRETEST), shard=None):
        kw = {} if shard is None else dict(shard_count=shard[0], shard_index=shard[1], shard_chunk=shard[2])
        self.p, self.cam, self.flags, self.shard = p, cam, flags, shard
        self.gpus = [bfa.SceneRepHashSDF(p, test_flags=f, **kw) for f in flags]
        self.ora = OracleScene(p, shard=shard)
        self.images, self.dev = {}, {}

    def add(self, key, d, c):
        self.images[key] = (d, c)
        self.dev[key] = (bfa.DeviceArray.from_host(np.ascontiguousarray(d, np.float32)),
                         bfa.DeviceArray.from_host(np.ascontiguousarray(c, np.uint8)))

    def batch(self, ops):
        """ops: (T, image key, deintegrate) in order, as one bf_scene_apply_ops batch. Returns the pre-test's
        predicted tile counts and checks every GPU scene's two counters against them (the tiles over the box
        limit, a part of the walked ones, are known from the prediction only)."""
        present = set(blocks_of(self.ora.export()[0]))
        pred = dict.fromkeys(KEYS, 0)
        active_tiles = 0
        for T, key, deint in ops:
            if deint:
                continue
            one = predict_pretest(T, self.images[key][0], self.cam, self.p, present, self.shard)
            active_tiles += len(tile_boxes(*ray_ends(T, self.images[key][0], self.cam, self.p)))
            for k in KEYS:
                pred[k] += one[k]
        assert pred["skipped"] + pred["walked"] == active_tiles
        cands = []
        for g, fl in zip(self.gpus, self.flags):
            g.resetStats()
            g.apply_ops([(T, self.dev[key][0], self.dev[key][1], deint) for T, key, deint in ops], self.cam)
            got = g.allocPretestStats()
            print(f"flags {fl}: pre-test counters {got}, predicted {pred}")
            if fl & BF_SCENE_TEST_ALLOC_NO_PRETEST:
                assert got == {"skipped": 0, "walked": active_tiles}
            else:
                assert got == {"skipped": pred["skipped"], "walked": pred["walked"]}
            assert got["skipped"] + got["walked"] == active_tiles  # the tiles with a ray to walk
            cands.append(g.stats()["candidates"])
            assert g.errorFlags() == 0
        assert len(set(cands)) == 1, f"candidate counts differ between the scenes: {cands}"
        for T, key, deint in ops:
            self.ora.integrate(T, *self.images[key], self.cam, deintegrate=deint)
        pred["candidates"] = cands[0]
        return pred

    def gc(self):
        for g in self.gpus:
            g.garbageCollect()
        self.ora.garbageCollect()

    def compare(self):
        n = [compare_states(self.p, g, self.ora) for g in self.gpus]
        for g in self.gpus:
            assert g.getHeapFreeCount() == self.ora.getHeapFreeCount()
        return n[0]


# a surface seen once leaves the corners of its tiles' boxes unallocated; seen from a few poses around
# (the state of a scanned room) the boxes fill up
JITTER = [(0.025 * sx, 0.025 * sy, 0.04 * sz) for sx in (-1, 1) for sy in (-1, 1) for sz in (-1, 1)] + \
         [(0.03, 0.0, 0.0), (-0.03, 0.0, 0.0), (0.0, 0.03, 0.0), (0.0, -0.03, 0.0), (0.0, 0.0, 0.05), (0.0, 0.0, -0.05)]


def sequence_a(rig, scene, cam):
    """(a): frame A, and A from fourteen poses around; A again as a two-op re-integration 3 mm off; frame B half
    beside A. Returns the three batches' predictions."""
    TA, dA, cA = frame(scene, cam, 0)
    rig.add("A", dA, cA)
    out = [rig.batch([(TA, "A", False)])]
    assert rig.compare() > 100
    rig.batch([(shifted(TA, *j), "A", False) for j in JITTER])
    TA2 = shifted(TA, dx=0.003, dy=-0.002)
    out.append(rig.batch([(TA, "A", True), (TA2, "A", False)]))
    rig.compare()
    # half of B's footprint (72 px of ~4 mm at ~2-3 m) lies beside A's
    TB, dB, cB = frame(scene, cam, 0, T=shifted(TA, dx=0.12))
    rig.add("B", dB, cB)
    out.append(rig.batch([(TB, "B", False)]))
    rig.gc()
    rig.compare()
    return out


def test_reintegration_skips_and_new_geometry_walks(scene):
    """(a) + (h): nothing is skipped on an empty scene, most tiles of the re-integration are, frame B's
    tiles over new geometry walk; with and without the pre-test the scene is the oracle's."""
    cam, p = make_cam(), make_params()
    first, again, half_new = sequence_a(Rig(p, cam), scene, cam)
    assert first["skipped"] == 0 and first["walked"] > 10 and first["candidates"] > 100
    assert again["skipped"] > again["walked"]
    assert half_new["skipped"] > 0 and half_new["walked"] > half_new["overLimit"] and half_new["candidates"] > 0


def test_congested_path_with_the_pretest(scene):
    """(g): the walk's congested path forced on for every tile that walks, with and without the pre-test."""
    cam, p = make_cam(), make_params()
    d = BF_SCENE_TEST_ALLOC_DIRECT
    first, again, half_new = sequence_a(Rig(p, cam, flags=(d, d | BF_SCENE_TEST_ALLOC_NO_PRETEST)), scene, cam)
    assert again["skipped"] > 0 and half_new["walked"] > 0


@pytest.mark.parametrize("index", [0, 1])
def test_sharded_scene(scene, index):
    """(f): shardCount = 2 against the oracle with the same ownership (or_scene_set_shard). The pre-test asks
    for this rank's blocks of a box only (another rank's cannot be emitted here); the ownership skip of the
    walk's setup still follows it."""
    cam, p = make_cam(), make_params()
    rig = Rig(p, cam, shard=(2, index, 0.5))
    first, again, half_new = sequence_a(rig, scene, cam)
    # a tile all of whose box belongs to the other rank ends at the pre-test even on an empty scene
    assert first["candidates"] > 0 and first["walked"] > 0
    assert again["skipped"] > again["walked"] and half_new["walked"] > 0


def test_step_edge_and_nearly_empty_tiles():
    """(b): a depth step through a tile column (a box far over the limit: the tile walks whatever exists), an
    all-invalid tile and, beside it, a tile with one valid pixel; integrated from an oblique pose, from the
    poses around it, and again, when the small boxes are full."""
    cam, p = make_cam(), make_params()
    rng = np.random.default_rng(3)
    d = np.full((H, W), 1.5, np.float32) + rng.normal(size=(H, W)).astype(np.float32) * np.float32(0.001)
    d[:, 40:] += np.float32(1.2)       # the step runs through tile column 2 (pixels 32..47)
    d[0:16, 0:16] = -np.inf            # tile (0, 0): no ray
    d[0:16, 16:32] = -np.inf           # tile (1, 0): one ray
    d[5, 21] = np.float32(1.5)
    c = rng.integers(0, 255, size=(H, W, 4), dtype=np.uint8)
    a = np.deg2rad(25.0)
    T = np.eye(4, dtype=np.float32)
    T[:3, :3] = np.array([[np.cos(a), 0, np.sin(a)], [0, 1, 0], [-np.sin(a), 0, np.cos(a)]], np.float32)
    T[:3, 3] = (-0.4, 0.3, -1.0)
    rig = Rig(p, cam)
    rig.add("S", d, c)
    first = rig.batch([(T, "S", False)])
    rig.compare()
    rig.batch([(shifted(T, *j), "S", False) for j in JITTER])
    again = rig.batch([(T, "S", False)])
    rig.compare()
    tiles = 5 * 4 - 1
    assert first["skipped"] == 0 and first["walked"] == tiles and first["overLimit"] >= 4
    assert again["skipped"] > 0 and again["overLimit"] == first["overLimit"] and again["candidates"] == 0


def test_removed_blocks_are_allocated_again(scene):
    """(c): the frame's blocks are removed (de-integrated to weight 0, then garbage-collected); the same
    frame finds none of them and allocates them again."""
    cam, p = make_cam(), make_params()
    rig = Rig(p, cam)
    TA, dA, cA = frame(scene, cam, 0)
    rig.add("A", dA, cA)
    first = rig.batch([(TA, "A", False)])
    full = rig.compare()
    rig.batch([(TA, "A", True)])
    rig.gc()
    assert rig.compare() == 0 and rig.gpus[0].getHeapFreeCount() == p.numSDFBlocks
    back = rig.batch([(TA, "A", False)])
    assert rig.compare() == full
    assert back["skipped"] == 0 and back["walked"] == first["walked"] and back["candidates"] == first["candidates"]


def test_absent_box_corner_walks_and_emits_nothing(scene):
    """(d): the same frame at the same pose again: every block its rays visit exists, so no candidate comes
    out, but a tile's box also holds blocks no ray visits; where one of those is absent the tile walks."""
    cam, p = make_cam(), make_params()
    rig = Rig(p, cam)
    TA, dA, cA = frame(scene, cam, 0)
    rig.add("A", dA, cA)
    rig.batch([(TA, "A", False)])
    again = rig.batch([(TA, "A", False)])
    rig.compare()
    assert again["candidates"] == 0
    assert again["walked"] - again["overLimit"] > 0, "no tile with a small box and an absent corner: choose another frame"
    assert again["skipped"] > 0


def test_eleven_integrate_batch(scene):
    """(e): ten re-integrations and one new frame as one batch (11 walks in one launch, birth ops decided
    through the voxel result as in test_op_batch_parity)."""
    cam, p = make_cam(), make_params()
    rig = Rig(p, cam)
    T0 = bfa.synth_pose(0)
    poses = [shifted(T0, dx=0.02 * k, dy=0.01 * (k % 3)) for k in range(11)]
    for k, T in enumerate(poses):
        _, d, c = frame(scene, cam, k, T=T)
        rig.add(k, d, c)
    for k in range(10):
        rig.batch([(poses[k], k, False)])
    rig.gc()
    rig.compare()
    ops = []
    for k in range(10):
        ops += [(poses[k], k, True), (shifted(poses[k], dx=0.004, dz=-0.003), k, False)]
    ops.append((poses[10], 10, False))
    got = rig.batch(ops)
    assert rig.compare() > 300
    rig.gc()
    rig.compare()
    assert got["skipped"] > 0 and got["walked"] > 0 and got["candidates"] > 0
