"""NumPy float32 restatement of key fusing: SIFTImageManager::fuseToGlobal / computeTracks / findTrack
(SiftGPU/SIFTImageManager.cpp:367-476), the stage bf_match_fuse_to_global runs on the device.

Every float operation is one float32 operation in the reference's order (float4x4 * float3: products summed left to
right, translation last; length = sqrtf of x x + y y + z z; the mean divides each component), so with the library's
-ffp-contract=off build and correctly rounded / and sqrtf the device result is bit-identical, not merely close.

`compute_tracks` is the literal form: neighbour lists in record order and the recursive findTrack (an explicit stack with
the recursion's semantics) over roots in ascending key index. `search_tracks` is the form the kernel uses: per component, an
ordinary depth-first search that starts at the first neighbour of the component's lowest key. tests/test_match_fuse.py
checks one against the other on random multigraphs.

Truncation is the project's rule, not the reference's defect: with more fused keys than the limit, the order is (depth
ascending, track order ascending), the first `limit` are kept, and descriptors move with their keys."""
import numpy as np

from bundlefusion_amd.abi import ENTRYJ_DTYPE

F32 = np.float32
NONE = 0xFFFFFFFF
MAX_TRACK_CORR_ERROR = F32(0.03)
MARGIN = 1e-4  # every fixture keeps its records' errors this far from the threshold


def xform(M, v):
    """float4x4 * float3 with w = 1 (cuda_SimpleMatrixUtil.h), float32 throughout."""
    M = np.asarray(M, F32).reshape(4, 4)
    x, y, z = F32(v[0]), F32(v[1]), F32(v[2])
    return np.array([M[r, 0] * x + M[r, 1] * y + M[r, 2] * z + M[r, 3] for r in range(3)], F32)


def length(v):
    return np.sqrt(v[0] * v[0] + v[1] * v[1] + v[2] * v[2])


def record_errors(corr, transforms):
    """length(T[i] pos_i - T[j] pos_j) of every valid record (NaN for invalid ones), float32."""
    err = np.full(len(corr), np.nan, F32)
    for r, e in enumerate(corr):
        if e["i"] != NONE:
            err[r] = length(xform(transforms[e["i"]], e["pos_i"]) - xform(transforms[e["j"]], e["pos_j"]))
    return err


def assert_margin(corr, transforms):
    err = record_errors(corr, transforms)
    err = err[~np.isnan(err)].astype(np.float64)
    assert np.all(np.abs(err - float(MAX_TRACK_CORR_ERROR)) >= MARGIN), np.abs(err - 0.03).min()


def neighbour_lists(n_keys, corr, key_idx, transforms):
    """corrPerKey: per key, in record order, (image of the other key, the other key, its pos or None for a bad edge)."""
    adj = [[] for _ in range(n_keys)]
    for r, e in enumerate(corr):
        if e["i"] == NONE:
            continue
        x, y = int(key_idx[r][0]), int(key_idx[r][1])
        err = length(xform(transforms[e["i"]], e["pos_i"]) - xform(transforms[e["j"]], e["pos_j"]))
        good = bool(err < MAX_TRACK_CORR_ERROR)
        adj[x].append((int(e["j"]), y, np.array(e["pos_j"], F32) if good else None))
        adj[y].append((int(e["i"]), x, np.array(e["pos_i"], F32) if good else None))
    return adj


def find_track(adj, marker, track, key):
    """findTrack: the recursion, run on an explicit stack of (key, next neighbour)."""
    stack = [(key, 0)]
    while stack:
        cur, i = stack.pop()
        while i < len(adj[cur]):
            c = adj[cur][i]
            i += 1
            if not marker[c[1]]:
                track.append(c)
                marker[c[1]] = True
                stack.append((cur, i))  # the call returns here
                cur, i = c[1], 0
    return track


def compute_tracks(adj):
    """computeTracks' loop over every key in ascending index; the empty tracks dropped."""
    marker = [False] * len(adj)
    tracks = []
    for k in range(len(adj)):
        if not tracks or tracks[-1]:
            tracks.append([])
        find_track(adj, marker, tracks[-1], k)
    return [t for t in tracks if t]


def search_tracks(adj):
    """The equivalent the device uses: per component in ascending order of its lowest key, the preorder of a depth-first
    search from the lowest key's first neighbour; the start carries the flag of the lowest key's first record."""
    seen = [False] * len(adj)
    out = []
    for k in range(len(adj)):
        if seen[k] or not adj[k]:
            continue
        first = adj[k][0]
        track = [first]
        seen[first[1]] = True
        stack = [[first[1], 0]]
        while stack:
            top = stack[-1]
            if top[1] == len(adj[top[0]]):
                stack.pop()
                continue
            c = adj[top[0]][top[1]]
            top[1] += 1
            if not seen[c[1]]:
                seen[c[1]] = True
                track.append(c)
                stack.append([c[1], 0])
        assert seen[k]
        out.append(track)
    return out


def track_tables(n_keys, tracks):
    """(root, rank, good) per key, as bf_match_fuse_tracks reports them."""
    root = np.full(n_keys, NONE, np.uint32)
    rank = np.full(n_keys, NONE, np.uint32)
    good = np.zeros(n_keys, np.uint8)
    for t in tracks:
        low = min(c[1] for c in t)
        for pos, c in enumerate(t):
            root[c[1]], rank[c[1]], good[c[1]] = low, pos, c[2] is not None
    return root, rank, good


def fuse(keys, descs, corr, key_idx, transforms, intrinsics, limit):
    """keys [n, 4] float32 (x, y, scale, depth) and descs [n, 128] of the whole local store, linear. Returns a dict:
    tracks, root / rank / good, num_tracks (fused keys before the cut), rep (representative key per stored key), keys
    [m, 4] float32 and descs [m, 128] as stored."""
    keys = np.asarray(keys, F32).reshape(-1, 4)
    adj = neighbour_lists(len(keys), corr, key_idx, transforms)
    tracks = compute_tracks(adj)
    out_keys, rep = [], []
    for t in tracks:
        pos, num = np.zeros(3, F32), 0
        for c in t:
            if c[2] is not None:
                pos = pos + xform(transforms[c[0]], c[2])
                num += 1
        if num > 0:
            pos = pos / F32(num)
            p = xform(intrinsics, pos)
            out_keys.append((p[0] / p[2], p[1] / p[2], keys[t[0][1], 2], p[2]))
            rep.append(t[0][1])
    out_keys = np.array(out_keys, F32).reshape(-1, 4)
    rep = np.array(rep, np.int64)
    num_tracks = len(rep)
    if num_tracks > limit:
        order = np.argsort(out_keys[:, 3], kind="stable")[:limit]
        out_keys, rep = out_keys[order], rep[order]
    root, rank, good = track_tables(len(keys), tracks)
    return {"tracks": tracks, "root": root, "rank": rank, "good": good, "num_tracks": num_tracks, "rep": rep,
            "keys": out_keys, "descs": np.asarray(descs, np.uint8).reshape(-1, 128)[rep]}


# ---- fixtures ----------------------------------------------------------------------------------------------------
def intrinsics():
    K = np.eye(4, dtype=F32)
    K[0, 0], K[1, 1], K[0, 2], K[1, 2] = 580.0, 580.0, 319.5, 239.5
    return K


def small_transforms(rng, n, rot=0.02, trans=0.05):
    """Frame -> first frame, near the identity; frame 0 is the identity."""
    T = np.zeros((n, 4, 4), np.float64)
    for i in range(n):
        w = rng.uniform(-rot, rot, 3) if i else np.zeros(3)
        a = np.linalg.norm(w)
        Kx = np.array([[0, -w[2], w[1]], [w[2], 0, -w[0]], [-w[1], w[0], 0]])
        R = np.eye(3) + (np.sin(a) / a * Kx + (1 - np.cos(a)) / (a * a) * Kx @ Kx if a > 0 else 0)
        T[i] = np.eye(4)
        T[i, :3, :3] = R
        T[i, :3, 3] = rng.uniform(-trans, trans, 3) if i else 0
    return T.astype(F32)


def store(rng, counts):
    """(keys [n, 4], descs [n, 128], offsets): a store of random keys; only the scale and the descriptor are ever read."""
    n = int(sum(counts))
    keys = np.stack([rng.uniform(0, 639, n), rng.uniform(0, 479, n), rng.uniform(1.0, 8.0, n), rng.uniform(0.5, 4.0, n)], 1).astype(F32)
    descs = rng.integers(0, 256, (n, 128), dtype=np.uint8)
    return keys, descs, np.concatenate([[0], np.cumsum(counts)[:-1]]).astype(np.int64)


def image_of(offsets, counts, key):
    return int(np.searchsorted(np.asarray(offsets) + np.asarray(counts), key, side="right"))


def records(rng, transforms, edges, offsets, counts):
    """edges: (key x, key y, kind) with linear keys and kind = error in metres between the two observations, or None for
    an invalidated record. Both ends see one random world point; the second end is moved by `kind` along a random
    direction. Returns (corr, key_idx)."""
    corr = np.zeros(len(edges), ENTRYJ_DTYPE)
    key_idx = np.zeros((len(edges), 2), np.uint32)
    Tinv = [np.linalg.inv(t.astype(np.float64)) for t in transforms]
    for r, (x, y, kind) in enumerate(edges):
        i, j = image_of(offsets, counts, x), image_of(offsets, counts, y)
        P = np.array([rng.uniform(-1, 1), rng.uniform(-0.8, 0.8), rng.uniform(1.0, 3.5), 1.0])
        d = rng.normal(size=3)
        Q = P.copy()
        Q[:3] += (kind or 0.0) * d / np.linalg.norm(d)
        corr[r]["i"], corr[r]["j"] = (NONE if kind is None else i), j
        corr[r]["pos_i"], corr[r]["pos_j"] = (Tinv[i] @ P)[:3], (Tinv[j] @ Q)[:3]
        key_idx[r] = x, y
    return corr, key_idx


GOOD, NEAR, FAR, BAD, GONE = 0.0, 0.02, 0.04, 0.1, None
SHAPES_COUNTS = [12, 10, 12, 9]


def shapes_fixture():
    """Four images holding every graph shape at once (the comments name the keys as image:local index)."""
    rng = np.random.default_rng(21)
    counts = SHAPES_COUNTS
    keys, descs, off = store(rng, counts)
    k = lambda img, local: int(off[img] + local)  # noqa: E731
    E = [
        (k(0, 1), k(1, 1), GOOD),                                      # a 2-key track
        (k(0, 2), k(1, 2), NEAR), (k(1, 2), k(2, 2), GOOD),            # a chain over three images
        (k(0, 3), k(1, 3), GONE),                                      # an invalidated record: both keys stay isolated
        (k(0, 4), k(1, 4), BAD), (k(1, 4), k(2, 4), GOOD),             # a bad first edge: two bad entries, one good
        (k(0, 5), k(1, 5), FAR),                                       # every discovery edge bad: no key
        (k(0, 6), k(1, 6), GOOD), (k(0, 6), k(2, 6), BAD), (k(1, 6), k(2, 6), GOOD),  # cycle: 2:6 found from 0:6, bad
        (k(1, 7), k(2, 7), GOOD), (k(0, 7), k(1, 7), GOOD), (k(0, 7), k(2, 7), BAD),  # cycle: 0:7 found from 2:7, bad
        (k(0, 8), k(1, 8), GOOD), (k(1, 8), k(0, 9), GOOD),            # two keys of image 0 in one component
        (k(2, 9), k(2, 9), GOOD),                                      # a record of a key with itself
        (k(3, 1), k(2, 1), GONE), (k(3, 1), k(1, 0), GOOD),            # an invalidated first record
    ]
    # one key in 20 records (lists above 16 entries take the other sort), towards five keys, good and bad mixed
    star = [k(0, 10), k(0, 11), k(1, 9), k(2, 10), k(2, 11)]
    E += [(k(3, 0), star[n % 5], (GOOD, BAD, NEAR, FAR)[n % 4]) if n % 3 else (star[n % 5], k(3, 0), (BAD, GOOD)[n % 2])
          for n in range(20)]
    T = small_transforms(rng, len(counts))
    corr, key_idx = records(rng, T, E, off, counts)
    return {"counts": counts, "keys": keys, "descs": descs, "off": off, "T": T, "corr": corr, "key_idx": key_idx}


def random_fixture(seed=5, images=11, per_image=64, per_pair=18):
    """Random partial one-to-one matchings per image pair, errors on both sides of the threshold."""
    rng = np.random.default_rng(seed)
    counts = [per_image] * images
    keys, descs, off = store(rng, counts)
    E = []
    for i in range(images):
        for j in range(i + 1, images):
            a, b = rng.permutation(per_image)[:per_pair], rng.permutation(per_image)[:per_pair]
            kinds = rng.choice([GOOD, NEAR, FAR, BAD], per_pair, p=[0.5, 0.2, 0.15, 0.15])
            E += [(int(off[i] + x), int(off[j] + y), float(kd)) for x, y, kd in zip(a, b, kinds)]
    T = small_transforms(rng, images)
    corr, key_idx = records(rng, T, E, off, counts)
    gone = rng.permutation(len(E))[: len(E) // 20]  # what the solver invalidates in place
    corr["i"][gone] = NONE
    return {"counts": counts, "keys": keys, "descs": descs, "off": off, "T": T, "corr": corr, "key_idx": key_idx}


def chain_fixture(per_image=1024):
    """One component through every key of a two-image store: records (k, k + 1) in order. The search starts at key 1,
    finds key 0 and then descends 2, 3, ... to the last key, one recursion level per key."""
    rng = np.random.default_rng(9)
    counts = [per_image, per_image]
    keys, descs, off = store(rng, counts)
    n = 2 * per_image
    E = [(x, x + 1, GOOD if x % 7 else BAD) for x in range(n - 1)]
    T = small_transforms(rng, 2)
    corr, key_idx = records(rng, T, E, off, counts)
    return {"counts": counts, "keys": keys, "descs": descs, "off": off, "T": T, "corr": corr, "key_idx": key_idx}


def depth_fixture(n_tracks, equal=(), nearer=7):
    """n_tracks two-key tracks of a two-image store under identity transforms, so a track's depth is its point's z. The
    depths are distinct and shuffled, except that the tracks listed in `equal` share one depth exactly, with `nearer`
    tracks in front of them: a limit of nearer + 1 keeps the first of them and cuts the others."""
    rng = np.random.default_rng(33)
    counts = [n_tracks, n_tracks]
    keys, descs, off = store(rng, counts)
    T = np.stack([np.eye(4, dtype=F32)] * 2)
    others = [t for t in range(n_tracks) if t not in equal]
    z = np.zeros(n_tracks, F32)
    for t, p in zip(others, rng.permutation(len(others))):
        z[t] = F32(1.0) + F32(0.125) * F32(p if p < nearer else p + 1)  # exact in float32
    for t in equal:
        z[t] = F32(1.0) + F32(0.125) * F32(nearer)
    corr = np.zeros(n_tracks, ENTRYJ_DTYPE)
    key_idx = np.zeros((n_tracks, 2), np.uint32)
    for t in range(n_tracks):
        p = np.array([rng.uniform(-0.5, 0.5), rng.uniform(-0.4, 0.4), z[t]], F32)
        corr[t]["i"], corr[t]["j"], corr[t]["pos_i"], corr[t]["pos_j"] = 0, 1, p, p
        key_idx[t] = t, n_tracks + t
    return {"counts": counts, "keys": keys, "descs": descs, "off": off, "T": T, "corr": corr, "key_idx": key_idx, "z": z}
