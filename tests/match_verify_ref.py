"""NumPy restatement of the matcher's surface-area and dense-verify filters (Bundler.cpp:175-199), written from the
reference: FilterMatchesBySurfaceAreaCU_Kernel (SIFTImageManager.cu:318-389) with cuda_surfaceArea.h,
MYEIGEN::eigenSystem / jacobi (cuda_SVD.h:17-213) and the 2x2 computeEigenValues / computeEigenVector
(cuda_EigenValue.h:56-85); FilterMatchesByDenseVerifyCU_Kernel and computeProjError, float-normal branch
(SIFTImageManager.cu:417-585).

Every routine takes the number format `dt`: np.float32 is the decision arithmetic, in the reference's operation order;
np.float64 is the twin that marks BORDERLINE items, whose verdict a differently rounded but equally valid evaluation
may flip (the pattern of match_ref.borderline_fraction):
  * a pixel whose float64 value lies within a relative 1e-5 of a threshold it is compared to (distThresh,
    normalThresh, the depth range, projDepth against tgtDepth), or whose projected coordinate lies within 1e-3 pixel
    of a rounding half-point (the image border, x = -0.5 or W - 0.5, is one of them);
  * a pair whose area lies within 1 % of the area threshold, or whose two largest 3x3 eigenvalues or two 2x2
    eigenvalues differ by less than 10 % (the box orientation is ill-conditioned there).

What eigenSystem returns: jacobi accumulates the eigenvectors in the COLUMNS of v (ROTATE(v, j, ip, j, iq)), and
eigenSystem copies eigenvectors[i][j] = v[i+1][j+1], the ROWS. The rows of a rotation are an orthonormal frame too,
but not the eigenvectors unless v is symmetric; the result then depends on the sweep order, so the sweep is restated
exactly: pairs (0,1), (0,2), (1,2), threshold 0.2 sm / 9 in sweeps 1-3, t from theta, at most 50 sweeps."""
import numpy as np

import match_ref as mr

F32, F64 = np.float32, np.float64
OPTS = dict(area=0.032, dist=0.15, normal=0.97, err=0.075, corr=0.02, dmin=0.1, dmax=4.0)  # zParameters*Default.txt
REL, PIX = 1e-5, 1e-3
NINF = -np.inf


def opts(**kw):
    o = dict(OPTS)
    o.update(kw)
    return o


# ---- surface area -----------------------------------------------------------------------------------------------
def tree32(vals, dt, op=np.add, fill=0.0):
    """Lane 0 of the reference's 32-lane __shfl_down tree over vals (lanes past len(vals) hold `fill`)."""
    v = np.full(32, fill, dt)
    v[:len(vals)] = vals
    for off in (16, 8, 4, 2, 1):
        v[:off] = op(v[:off], v[off:2 * off])
    return dt(v[0])


def jacobi3(A, dt):
    """MYEIGEN::jacobi<3>: (ok, d eigenvalues, v with the eigenvectors in its columns)."""
    a = np.array(A, dt)
    v = np.eye(3, dtype=dt)
    d = np.array([a[0, 0], a[1, 1], a[2, 2]], dt)
    b, z = d.copy(), np.zeros(3, dt)
    c0, c1, half, hundred = dt(0.0), dt(1.0), dt(0.5), dt(100.0)
    for i in range(1, 51):
        sm = (abs(a[0, 1]) + abs(a[0, 2])) + abs(a[1, 2])
        if sm == c0:
            return True, d, v
        tresh = dt(0.2) * sm / dt(9.0) if i < 4 else c0
        for ip, iq in ((0, 1), (0, 2), (1, 2)):
            g = hundred * abs(a[ip, iq])
            if i > 4 and abs(d[ip]) + g == abs(d[ip]) and abs(d[iq]) + g == abs(d[iq]):
                a[ip, iq] = c0
            elif abs(a[ip, iq]) > tresh:
                h = d[iq] - d[ip]
                if abs(h) + g == abs(h):
                    t = a[ip, iq] / h
                else:
                    theta = half * h / a[ip, iq]
                    t = c1 / (abs(theta) + np.sqrt(c1 + theta * theta))
                    if theta < c0:
                        t = -t
                c = c1 / np.sqrt(c1 + t * t)
                s = t * c
                tau = s / (c1 + c)
                h = t * a[ip, iq]
                z[ip] -= h
                z[iq] += h
                d[ip] -= h
                d[iq] += h
                a[ip, iq] = c0
                j = 3 - ip - iq
                x = (j, ip) if j < ip else (ip, j)
                y = (j, iq) if j < iq else (iq, j)
                gg, hh = a[x], a[y]
                a[x] = gg - s * (hh + gg * tau)
                a[y] = hh + s * (gg - hh * tau)
                for k in range(3):
                    gg, hh = v[k, ip], v[k, iq]
                    v[k, ip] = gg - s * (hh + gg * tau)
                    v[k, iq] = hh + s * (gg - hh * tau)
        b += z
        d = b.copy()
        z[:] = c0
    return False, d, v


def eigen_system3(V, dt, rows=True):
    """MYEIGEN::eigenSystem: (ok, eigenvalues sorted by |.| descending, ev[3, 3] with ev[i] the vector that goes with
    eigenvalue i). rows=True is the reference (ev[i] = row i of jacobi's v); rows=False would be the eigenvectors."""
    ok, d, v = jacobi3(np.asarray(V, dt).T, dt)
    if not ok:
        return False, d, v
    ev = (v if rows else v.T).copy()
    d = d.copy()
    for i in range(3):
        cur_max, at = dt(0.0), -1
        for j in range(i, 3):
            if abs(d[j]) > cur_max:
                cur_max, at = abs(d[j]), j
        if at != i and at != -1:
            d[[i, at]] = d[[at, i]]
            ev[[i, at]] = ev[[at, i]]
    return True, d, ev


def key_points(keys, kinv, dt):
    """intrinsicsInv * (depth * (x, y, 1)) of float32 keys, evaluated in dt."""
    if dt is F32:
        return mr.key_points32(keys, kinv)
    k = np.asarray(kinv, F32).reshape(4, 4).astype(dt)
    keys = np.asarray(keys, F32).reshape(-1, 4).astype(dt)
    v = np.stack([keys[:, 3] * keys[:, 0], keys[:, 3] * keys[:, 1], keys[:, 3]], 1)
    return v @ k[:3, :3].T + k[:3, 3]


def side_area(pts, dt, rows=True):
    """Area of one side: dict(area, ok, ev3 eigenvalues, ev2 eigenvalues)."""
    with np.errstate(all="ignore"):
        pts = np.asarray(pts, dt)
        n = len(pts)
        fn = dt(n)
        mean = np.array([tree32(pts[:, r], dt) / fn for r in range(3)], dt)
        dl = (pts - mean).astype(dt)
        V = np.zeros((3, 3), dt)
        for r in range(3):
            for c in range(r, 3):
                V[r, c] = V[c, r] = tree32(dl[:, r] * dl[:, c], dt) / fn
        ok, ev3, ev = eigen_system3(V, dt, rows)
        if not ok:
            return dict(area=dt(0.0), ok=False, ev3=ev3, ev2=np.zeros(2, dt))
        k = (ev[2, 0] * dl[:, 0] + ev[2, 1] * dl[:, 1]) + ev[2, 2] * dl[:, 2]
        s = np.stack([(pts[:, r] - k * ev[2, r]) - mean[r] for r in range(3)], 1).astype(dt)
        px = (s[:, 0] * ev[0, 0] + s[:, 1] * ev[0, 1]) + s[:, 2] * ev[0, 2]
        py = (s[:, 0] * ev[1, 0] + s[:, 1] * ev[1, 1]) + s[:, 2] * ev[1, 2]
        mx, my = tree32(px, dt) / fn, tree32(py, dt) / fn
        ex, ey = px - mx, py - my
        cxx, cxy, cyy = tree32(ex * ex, dt) / fn, tree32(ex * ey, dt) / fn, tree32(ey * ey, dt) / fn
        disc = dt(0.5) * np.sqrt((cxx - cyy) * (cxx - cyy) + dt(4.0) * cxy * cxy)
        lam = np.array([(cxx + cyy) / dt(2.0) + disc, (cxx + cyy) / dt(2.0) - disc], dt)
        q = []
        for l in lam:
            vx, vy = -cxy, cxx - l
            mag = np.sqrt(vx * vx + vy * vy)
            vx, vy = vx / mag, vy / mag
            inv = dt(1.0) / np.sqrt(vx * vx + vy * vy)
            vx, vy = vx * inv, vy * inv
            q.append(vx * px + vy * py)
        big = np.finfo(np.float32).max
        ext = [tree32(c, dt, np.maximum, -big) - tree32(c, dt, np.minimum, big) for c in q]
        area = dt(0.0) if ext[0] < dt(0.00001) or ext[1] < dt(0.00001) else dt(ext[0] * ext[1])
        return dict(area=area, ok=True, ev3=ev3, ev2=lam)


def _close(a, b, frac):
    a, b = abs(float(a)), abs(float(b))
    return abs(a - b) < frac * max(a, b)


def surface_area_pair(keys, idx, kinv, thresh=OPTS["area"], rows=True):
    """keys: the store's linear key array [., 4]; idx [n <= 25, 2] filtered index pairs. dict(area [2] float32,
    area64 [2], reject, border)."""
    idx = np.asarray(idx, np.int64).reshape(-1, 2)
    out = dict(area=np.zeros(2, F32), area64=np.zeros(2), border=False)
    for which in (0, 1):
        k = np.asarray(keys, F32).reshape(-1, 4)[idx[:, which]]
        a32 = side_area(key_points(k, kinv, F32), F32, rows)
        a64 = side_area(key_points(k, kinv, F64), F64, rows)
        out["area"][which], out["area64"][which] = a32["area"], a64["area"]
        if abs(float(a64["area"]) - thresh) <= 0.01 * thresh or np.isnan(a64["area"]) != np.isnan(a32["area"]):
            out["border"] = True
        if a64["area"] > 0.0 and (_close(a64["ev3"][0], a64["ev3"][1], 0.1) or _close(a64["ev2"][0], a64["ev2"][1], 0.1)):
            out["border"] = True
    t = F32(thresh)
    out["reject"] = bool(out["area"][0] < t and out["area"][1] < t)
    return out


# ---- dense verify -------------------------------------------------------------------------------------------------
def _roundf(x):
    """roundf: half away from zero (np.round is half to even)."""
    a = np.abs(x)
    f = np.floor(a)
    return np.copysign(f + (a - f >= 0.5), x)


def _f2i(x):
    """float -> int as the GPU converts: NaN -> 0, saturating."""
    x = np.where(np.isnan(x), 0.0, x)
    return np.clip(x, -2147483648.0, 2147483647.0).astype(np.int64)


def _near(a, b):
    with np.errstate(all="ignore"):
        return np.abs(a - b) <= REL * np.maximum(np.abs(a), np.abs(b))


def proj_error(inp, model, tr, K, o, dt):
    """computeProjError over every pixel of `inp` carried by `tr` into `model`: dict(res, weight, ok [W H] in dt, and
    border [W H] bool, meaningful for dt = float64)."""
    with np.errstate(all="ignore"):
        H, W = np.asarray(inp["depth"]).shape
        p = np.asarray(inp["campos"], F32).reshape(-1, 4).astype(dt)
        n = np.asarray(inp["normals"], F32).reshape(-1, 4).astype(dt).copy()
        n[:, 3] = 0.0
        d_in = np.asarray(inp["depth"], F32).reshape(-1).astype(dt)
        tr, K = np.asarray(tr, F32).reshape(4, 4).astype(dt), np.asarray(K, F32).reshape(4, 4).astype(dt)
        dmin, dmax, distT, normT = dt(o["dmin"]), dt(o["dmax"]), dt(o["dist"]), dt(o["normal"])
        has = (p[:, 0] != NINF) & (n[:, 0] != NINF)
        v0 = has & (d_in >= dmin) & (d_in <= dmax)
        border = has & (_near(d_in, dmin) | _near(d_in, dmax))
        mul = lambda M, r, v: ((M[r, 0] * v[:, 0] + M[r, 1] * v[:, 1]) + M[r, 2] * v[:, 2]) + M[r, 3] * v[:, 3]  # noqa: E731
        pT = np.stack([mul(tr, r, p) for r in range(4)], 1)
        nT = np.stack([mul(tr, r, n) for r in range(3)], 1)
        one = np.concatenate([pT[:, :3], np.ones((len(pT), 1), dt)], 1)
        q = np.stack([mul(K, r, one) for r in range(3)], 1)
        fx, fy = q[:, 0] / q[:, 2], q[:, 1] / q[:, 2]
        sx, sy = _f2i(_roundf(fx)), _f2i(_roundf(fy))
        inb = (sx >= 0) & (sy >= 0) & (sx < W) & (sy < H)
        half = (np.abs((fx - np.floor(fx)) - 0.5) < PIX) | (np.abs((fy - np.floor(fy)) - 0.5) < PIX)
        border |= v0 & half & (fx > -1.0) & (fy > -1.0) & (fx < W) & (fy < H)
        v1 = v0 & inb
        t = np.where(v1, sy * W + sx, 0)
        pg = np.asarray(model["campos"], F32).reshape(-1, 4).astype(dt)[t]
        ng = np.asarray(model["normals"], F32).reshape(-1, 4).astype(dt)[t]
        tgt = np.asarray(model["depth"], F32).reshape(-1).astype(dt)[t]
        v2 = v1 & (pg[:, 0] != NINF) & (ng[:, 0] != NINF)
        df = pT - pg
        dist = np.sqrt(((df[:, 0] * df[:, 0] + df[:, 1] * df[:, 1]) + df[:, 2] * df[:, 2]) + df[:, 3] * df[:, 3])
        dN = (nT[:, 0] * ng[:, 0] + nT[:, 1] * ng[:, 1]) + nT[:, 2] * ng[:, 2]
        v3 = v2 & (tgt >= dmin) & (tgt <= dmax)
        border |= v2 & (_near(tgt, dmin) | _near(tgt, dmax))
        bad = (tgt != NINF) & (pT[:, 2] < tgt) & (dist > distT)
        ok = v3 & (((dN >= normT) & (dist <= distT)) | bad)
        # distThresh decides every reached pixel; normalThresh those within it; projDepth < tgtDepth those beyond it
        border |= v3 & (_near(dist, distT) | ((dist <= distT) & _near(dN, normT)) | ((dist > distT) & _near(pT[:, 2], tgt)))
        camz = (pT[:, 2] - dmin) / (dmax - dmin)
        w = np.maximum(dt(0.0), dt(0.5) * ((dt(1.0) - dist / distT) + (dt(1.0) - camz)))
        zero = dt(0.0)
        return dict(res=np.where(ok, dist, zero).astype(dt), weight=np.where(ok, w, zero).astype(dt), ok=ok, border=border,
                    dist=dist, reached=v3)


def dense_pair(prev, cur, T, Tinv, K, o=None):
    """Pair (prev, cur) with T prev -> cur and Tinv back. dict(sums [2, 3] float32 (sumResidual, sumWeight, numCorr per
    direction; float32 terms added in float64), sums64, err, corr, reject, nborder [2], flips [2], worst_d)."""
    o = o or OPTS
    H, W = np.asarray(prev["depth"]).shape
    out = dict(sums=np.zeros((2, 3), F32), sums64=np.zeros((2, 3)), nborder=[0, 0], flips=[0, 0], worst_d=0.0, npix=W * H)
    for k, (a, b, tr) in enumerate(((prev, cur, T), (cur, prev, Tinv))):
        r32, r64 = proj_error(a, b, tr, K, o, F32), proj_error(a, b, tr, K, o, F64)
        out["sums"][k] = [r32["res"].astype(F64).sum(), r32["weight"].astype(F64).sum(), r32["ok"].sum()]
        out["sums64"][k] = [r64["res"].sum(), r64["weight"].sum(), r64["ok"].sum()]
        out["nborder"][k] = int(r64["border"].sum())
        out["flips"][k] = int(((r32["ok"] != r64["ok"]) & ~r64["border"]).sum())  # expected 0
        d = r64["dist"][r64["border"] & r64["reached"]]
        if len(d):
            out["worst_d"] = max(out["worst_d"], float(d.max()))
    s = out["sums"]
    with np.errstate(all="ignore"):
        err = F32(s[0, 0] + s[1, 0]) / F32(s[0, 1] + s[1, 1])
        corr = F32(0.5) * F32(s[0, 2] + s[1, 2]) / F32(W * H)
    out.update(err=err, corr=corr, reject=bool(corr < F32(o["corr"]) or err > F32(o["err"]) or np.isnan(err)))
    return out


def verdict_is_safe(r, o=None):
    """True when the borderline pixels of a dense_pair result cannot move corr or err across their thresholds: each
    can add or remove one correspondence of residual <= max(worst_d, distThresh) and weight <= 1."""
    o = o or OPTS
    nb = sum(r["nborder"])
    if nb == 0:
        return True
    R, Wt = float(r["sums"][:, 0].sum()), float(r["sums"][:, 1].sum())
    if abs(float(r["corr"]) - o["corr"]) <= 0.5 * nb / r["npix"]:
        return False
    dmax = max(r["worst_d"], o["dist"])
    lo = max(R - nb * dmax, 0.0) / (Wt + nb)
    hi = (R + nb * dmax) / (Wt - nb) if Wt > nb else np.inf
    if r["reject"] and float(r["corr"]) < o["corr"]:
        return True  # rejected on corr, whose margin holds
    return not (lo <= o["err"] <= hi)


# ---- analytic cache frames: a room corner, ray-plane rendering ----------------------------------------------------
# World: y down, camera looks along +z. Right wall x = 1.6, floor y = 1.1, back wall z = 3.4 with a recess to z = 4.6
# for x in [-1.0, -0.55): behind the sensor range from every pose used here, so a band of out-of-range depth.
def cache_intrinsics(W, H, fov=72.5 / 80.0):
    K = np.eye(4, dtype=F32)
    K[0, 0] = K[1, 1] = fov * W
    K[0, 2], K[1, 2] = (W - 1) / 2.0, (H - 1) / 2.0
    return K


def render_room(T_c2w, W, H, K=None, holes=()):
    """Cache frame (depth [H, W], campos [H, W, 4] w = 1, normals [H, W, 4] w = 0; -inf where invalid) of the room from
    camera -> world pose T_c2w. holes: (row0, row1, col0, col1) blocks set invalid."""
    K = cache_intrinsics(W, H) if K is None else K
    T = np.asarray(T_c2w, F64)
    R, c = T[:3, :3], T[:3, 3]
    u, v = np.meshgrid(np.arange(W, dtype=F64), np.arange(H, dtype=F64))
    dirs = np.stack([(u - K[0, 2]) / K[0, 0], (v - K[1, 2]) / K[1, 1], np.ones_like(u)], -1)  # camera space, z = 1
    dw = dirs @ R.T
    best = np.full((H, W), np.inf)
    normal = np.zeros((H, W, 3))
    planes = [((1.0, 0.0, 0.0), 1.6, None), ((0.0, 1.0, 0.0), 1.1, None), ((0.0, 0.0, 1.0), 3.4, "front"),
              ((0.0, 0.0, 1.0), 4.6, "recess")]
    for nrm, off, kind in planes:
        nrm = np.array(nrm)
        with np.errstate(divide="ignore", invalid="ignore"):
            t = (off - c @ nrm) / (dw @ nrm)
            hit = c + t[..., None] * dw
        ok = (t > 0) & np.isfinite(t)
        in_recess = (hit[..., 0] >= -1.0) & (hit[..., 0] < -0.55)
        if kind == "front":
            ok &= ~in_recess
        if kind == "recess":
            ok &= in_recess
        closer = ok & (t < best)
        best = np.where(closer, t, best)
        normal[closer] = -nrm  # towards the room's inside, where the cameras are
    valid = np.isfinite(best)
    for r0, r1, c0, c1 in holes:
        valid[r0:r1, c0:c1] = False
    pos = dirs * np.where(valid, best, 0.0)[..., None]
    ncam = normal @ R  # world -> camera: R^T n
    depth = np.where(valid, pos[..., 2], NINF).astype(F32)
    campos = np.concatenate([pos, np.ones((H, W, 1))], -1).astype(F32)
    normals = np.concatenate([ncam, np.zeros((H, W, 1))], -1).astype(F32)
    campos[~valid] = NINF
    normals[~valid] = NINF
    return dict(depth=depth, campos=campos, normals=normals)


def room_depth(T_c2w, W, H, fx, fy, cx, cy, holes=()):
    """Sensor-style depth image [H, W] float32 (-inf invalid) of the room, for CUDACache.storeFrame."""
    K = np.eye(4, dtype=F32)
    K[0, 0], K[1, 1], K[0, 2], K[1, 2] = fx, fy, cx, cy
    return render_room(T_c2w, W, H, K, holes)["depth"]


def room_landmarks(rng, n):
    """n points on the room's three surfaces (world)."""
    pts = []
    while len(pts) < n:
        k = rng.integers(0, 3)
        a, b = rng.uniform(-1.4, 1.5), rng.uniform(-1.0, 1.0)
        p = [(1.6, b, rng.uniform(1.8, 3.3)), (a, 1.1, rng.uniform(1.8, 3.3)), (a if not -1.05 <= a < -0.5 else a + 0.8, b, 3.4)][k]
        pts.append(p)
    return np.array(pts, F64)


def pose(tx=0.0, ty=0.0, tz=0.0, yaw=0.0, pitch=0.0):
    cy_, sy_, cp, sp = np.cos(yaw), np.sin(yaw), np.cos(pitch), np.sin(pitch)
    Ry = np.array([[cy_, 0, sy_], [0, 1, 0], [-sy_, 0, cy_]])
    Rx = np.array([[1, 0, 0], [0, cp, -sp], [0, sp, cp]])
    T = np.eye(4)
    T[:3, :3] = Ry @ Rx
    T[:3, 3] = [tx, ty, tz]
    return T


# ---- fixtures of tests/test_match_verify_gpu.py (tests/test_match_verify.py asserts their conditions) ---------------
def patch_keys(w, h, nx, ny, centre, tilt=(0.0, 0.0), spin=0.35, pts=None):
    """Key points [n, 4] float32 (u, v, 1, z in the colour camera of match_ref) of an nx x ny grid spanning w x h metres,
    spun in its plane, tilted about x and y, centred at `centre` in camera space."""
    if pts is None:
        gx, gy = np.meshgrid(np.linspace(-w / 2, w / 2, nx), np.linspace(-h / 2, h / 2, ny))
        pts = np.stack([gx.ravel(), gy.ravel(), np.zeros(nx * ny)], 1)
    c, s = np.cos(spin), np.sin(spin)
    pts = pts @ np.array([[c, -s, 0], [s, c, 0], [0, 0, 1]]).T
    pts = pts @ pose(pitch=tilt[0], yaw=tilt[1])[:3, :3].T + np.asarray(centre, F64)
    u, v = mr.FX * pts[:, 0] / pts[:, 2] + mr.CX, mr.FY * pts[:, 1] / pts[:, 2] + mr.CY
    return np.stack([u, v, np.ones(len(u)), pts[:, 2]], 1).astype(F32)


QUINCUNX = np.array([[-0.2, -0.12, 0], [0.2, -0.12, 0], [0, 0, 0], [-0.2, 0.12, 0], [0.2, 0.12, 0]], F64)
LINE = np.stack([np.linspace(-0.4, 0.4, 9), 0.2 * np.linspace(-0.4, 0.4, 9), 0.1 * np.linspace(-0.4, 0.4, 9)], 1)


def area_fixture():
    """(images, lists): 6 images; image 5 is cur; lists[prev] = index pairs into the linear key array for pair
    (prev, 5): 0: 5 matches (the minimum), 1: 25 (the cap), 2: a small patch on both sides (rejected), 3: small on
    prev's side, large on cur's (kept), 4: a collinear set (area 0, rejected)."""
    sides = [
        (patch_keys(0, 0, 0, 0, (0.1, 0.0, 2.0), (0.2, 0.1), pts=QUINCUNX), patch_keys(0, 0, 0, 0, (-0.1, 0.05, 2.2), (0.1, 0.3), pts=QUINCUNX)),
        (patch_keys(0.9, 0.5, 5, 5, (0.0, 0.0, 2.4), (0.3, 0.2)), patch_keys(0.9, 0.5, 5, 5, (0.1, 0.0, 2.5), (0.25, 0.1))),
        (patch_keys(0.1, 0.07, 3, 3, (0.2, 0.1, 1.8), (0.1, 0.2)), patch_keys(0.1, 0.07, 3, 3, (0.1, 0.1, 1.9), (0.15, 0.1))),
        (patch_keys(0.1, 0.07, 4, 3, (0.0, 0.1, 1.7), (0.2, 0.1)), patch_keys(0.5, 0.3, 4, 3, (0.1, 0.0, 2.1), (0.1, 0.2))),
        (patch_keys(0, 0, 0, 0, (0.0, 0.0, 2.5), pts=LINE, spin=0.0), patch_keys(0, 0, 0, 0, (0.1, 0.0, 2.6), pts=LINE, spin=0.0)),
    ]
    rng = np.random.default_rng(4)
    images, lists, off = [], [], 0
    cur_keys = np.concatenate([c for _, c in sides])
    offs = np.concatenate([[0], np.cumsum([len(p) for p, _ in sides])])
    cur_at = np.concatenate([[0], np.cumsum([len(c) for _, c in sides])])
    for i, (p, c) in enumerate(sides):
        images.append((p, mr.sift_like(rng, len(p))[1]))
        lists.append(np.stack([offs[i] + np.arange(len(p)), offs[-1] + cur_at[i] + np.arange(len(c))], 1))
    images.append((cur_keys, mr.sift_like(rng, len(cur_keys))[1]))
    return images, lists


DENSE_SHAPES = [(80, 60), (20, 13)]
DENSE_KEYS = 120


def dense_poses():
    """Camera -> world of images 0..3: three honest views and image 3's nominal pose; image 3's cache frame is rendered
    from `dense_wrong_pose()` instead, 0.3 m off: the false loop closure."""
    return [pose(0.0, 0.0, 0.0, 0.0), pose(0.12, -0.03, 0.05, -0.06, 0.02), pose(-0.1, 0.02, 0.1, 0.08, -0.03),
            pose(0.2, 0.0, -0.05, -0.1, 0.0)]


def dense_wrong_pose():
    return pose(0.2 - 0.3, 0.05, -0.05, 0.12, 0.0)


def dense_holes(W, H):
    return [(H // 5, H // 5 + max(1, H // 6), W // 8, W // 8 + max(2, W // 5))]


def dense_images():
    """Key points of room landmarks seen from dense_poses() (exact, so the Kabsch transform is the true relative pose)."""
    rng = np.random.default_rng(21)
    return mr.make_images(21, [DENSE_KEYS] * 4, poses=dense_poses(), pts=room_landmarks(rng, 100), share=0.7)[0]


def dense_frames(W, H):
    """The 4 cache frames at W x H: images 0..2 at their poses, image 3 from the wrong pose."""
    P = dense_poses()
    return [render_room(T, W, H, holes=dense_holes(W, H)) for T in P[:3]] + [render_room(dense_wrong_pose(), W, H)]


# Largest relative float32-versus-float64 difference of a side's area over area_fixture(), measured with this
# restatement on the CPU (test_match_verify.py::test_area_fixture_conditions prints and bounds it); the GPU bar is 10 x:
# the margin for a different but equally valid rounding of the same arithmetic.
AREA_F32_VS_F64 = 7.2e-7
AREA_TOL = 10.0 * AREA_F32_VS_F64

SMALL_OPTS = opts(err=0.3)  # at 20 x 13 a pixel spans ~0.15 m at 2.7 m: honest pairs sit near err 0.22


def dense_opts(W, H):
    return OPTS if (W, H) == (80, 60) else SMALL_OPTS


# the store of the skip / indexing test: 6 images, cur = 3 in the middle, start = 1; image 1 is empty, image 2 is set
# invalid after the Kabsch filter, pair 4's count is set to 0, pair 5 is live; image 0 lies before startFrame
SKIP_COUNTS = [110, 0, 90, 120, 100, 115]
SKIP_CUR, SKIP_START, SKIP_EMPTY, SKIP_INVALID, SKIP_ZERO, SKIP_LIVE = 3, 1, 1, 2, 4, 5
SKIP_SHAPE = (20, 13)


def skip_poses():
    return [pose(0.05 * k, 0.01 * k, 0.02 * k, -0.02 * k, 0.0) for k in range(6)]


def skip_images():
    rng = np.random.default_rng(33)
    return mr.make_images(33, SKIP_COUNTS, poses=skip_poses(), pts=room_landmarks(rng, 90), share=0.7)[0]


def skip_frames(live_wrong=False):
    W, H = SKIP_SHAPE
    P = skip_poses()
    if live_wrong:
        P[SKIP_LIVE] = pose(0.05 * SKIP_LIVE - 0.35, 0.0, 0.1, 0.15, 0.0)
    return [render_room(T, W, H) for T in P]


# real cache frames: CUDACache.storeFrame of 160 x 120 depth images of the room; image 2 is cur, image 0 honest, image
# 1's depth rendered 0.3 m off its key points' pose
REAL_IN = (160, 120, 145.0, 145.0, 79.5, 59.5)


def real_poses():
    return [pose(0.0, 0.0, 0.0, 0.0), pose(0.15, 0.0, 0.0, -0.05, 0.0), pose(0.08, -0.02, 0.04, -0.04, 0.01)]


def real_images():
    rng = np.random.default_rng(45)
    return mr.make_images(45, [DENSE_KEYS] * 3, poses=real_poses(), pts=room_landmarks(rng, 100), share=0.7)[0]


def real_depths():
    W, H, fx, fy, cx, cy = REAL_IN
    P = real_poses()
    P[1] = pose(0.15 - 0.3, 0.04, 0.0, 0.1, 0.0)
    color = np.full((H, W, 4), 128, np.uint8)
    color[..., 3] = 255
    return [(room_depth(T, W, H, fx, fy, cx, cy, holes=[(20, 40, 30, 60)]), color) for T in P]
