"""A numpy reference of the reprojection (include/frt_device.h "Reprojection"), written from its definition and not
from the C pass, and an analytic two-surface world the reprojection tests share.

Vectorised over pixels; every ufunc call is one IEEE binary64 operation per element, nothing is fused or reordered. It
takes O_cur, O_prev and prev_fwd from frt_reproject_setup (runtime.reproject_setup), as both passes do.
"""
from types import SimpleNamespace

import numpy as np

import accum_ref

DEFAULTS = {"max_history": 32, "match_material": 1, "normal_cos": 0.9, "sigma_depth": 0.02, "min_weight": 2.0 ** -6}

# per-pixel reasons: the outcome code is 0 for OK, 1 for MISS and 2 for the rest
OK, MISS, BEHIND, RANGE_X, RANGE_Y, WEIGHT = 0, 1, 2, 3, 4, 5
# per-tap reasons, the first test a tap fails in the definition's order; NA: the pixel never came to its taps
NA, ACCEPT, OUTSIDE, NO_COUNT, NODE, MATERIAL, DEPTH, NORMAL = -1, 0, 1, 2, 3, 4, 5, 6


def _xf_point(m, p):
    return tuple(((m[4 * r] * p[0] + m[4 * r + 1] * p[1]) + m[4 * r + 2] * p[2]) + m[4 * r + 3] for r in range(3))


def _dot3(a, b):
    return (a[0] * b[0] + a[1] * b[1]) + a[2] * b[2]


def reproject(src_n, src_mean, src_m2, prev, cur, o_cur, o_prev, prev_fwd, prev_geom, prev_ids, cur_geom, cur_ids, w,
              h, params=None):
    """The definition. prev, cur: objects with half_width, half_height, pixel_size, canvas_distance and inv (16).
    Returns a dict: n (npx,) int32, mean (npx, 4), m2 (npx, 3), outcome (npx,), reason (npx,), tap (npx, 4),
    accepted (npx,) the number of accepted taps, clamped (npx,) whether max_history cut the count."""
    P = dict(DEFAULTS, **(params or {}))
    npx = w * h
    src_n = np.asarray(src_n, dtype=np.int32).reshape(npx)
    src_mean = np.asarray(src_mean, dtype=np.float64).reshape(npx, 4)
    src_m2 = np.asarray(src_m2, dtype=np.float64).reshape(npx, 3)
    pg = np.asarray(prev_geom, dtype=np.float64).reshape(npx, 8)
    cg = np.asarray(cur_geom, dtype=np.float64).reshape(npx, 8)
    pi = np.asarray(prev_ids, dtype=np.int32).reshape(npx, 2)
    ci = np.asarray(cur_ids, dtype=np.int32).reshape(npx, 2)
    cinv = [np.float64(x) for x in cur.inv]
    fwd = [np.float64(x) for x in prev_fwd]
    oc = [np.float64(x) for x in o_cur]
    op = [np.float64(x) for x in o_prev]
    idx = np.arange(npx)
    px, py = (idx % w).astype(np.float64), (idx // w).astype(np.float64)
    with np.errstate(all="ignore"):
        # 1
        d = cg[:, 0]
        node, mat = ci[:, 0], ci[:, 1]
        valid = (node >= 0) & np.isfinite(d) & (d > 0.0)
        # 2
        xoff = (px + 0.5) * np.float64(cur.pixel_size)
        yoff = (py + 0.5) * np.float64(cur.pixel_size)
        cp = (np.float64(cur.half_width) - xoff, np.float64(cur.half_height) - yoff,
              np.full(npx, -np.float64(cur.canvas_distance)))
        Pw = _xf_point(cinv, cp)
        v = tuple(Pw[k] - oc[k] for k in range(3))
        inv = 1.0 / np.sqrt(_dot3(v, v))
        W = tuple(oc[k] + d * (v[k] * inv) for k in range(3))
        # 3
        c = _xf_point(fwd, W)
        front = np.isfinite(c[2]) & (c[2] < 0.0)
        s = -np.float64(prev.canvas_distance) / c[2]
        fx = (np.float64(prev.half_width) - c[0] * s) / np.float64(prev.pixel_size) - 0.5
        fy = (np.float64(prev.half_height) - c[1] * s) / np.float64(prev.pixel_size) - 0.5
        rx, ry = np.floor(fx + 0.5), np.floor(fy + 0.5)
        fx = np.where(np.abs(fx - rx) <= 2.0 ** -20, rx, fx)
        fy = np.where(np.abs(fy - ry) <= 2.0 ** -20, ry, fy)
        in_x = (fx >= -1.0) & (fx < np.float64(w))
        in_y = (fy >= -1.0) & (fy < np.float64(h))
        live = valid & front & in_x & in_y
        flx, fly = np.floor(np.where(live, fx, 0.0)), np.floor(np.where(live, fy, 0.0))
        x0, y0 = flx.astype(np.int64), fly.astype(np.int64)
        tx, ty = np.where(live, fx, 0.0) - flx, np.where(live, fy, 0.0) - fly
        # 4
        u = tuple(W[k] - op[k] for k in range(3))
        e = np.sqrt(_dot3(u, u))
        tol = np.float64(P["sigma_depth"]) * e
        n_p = (cg[:, 1], cg[:, 2], cg[:, 3])
        nnp = _dot3(n_p, n_p)
        cos2 = np.float64(P["normal_cos"]) * np.float64(P["normal_cos"])
        # 5, 6
        ux, uy = 1.0 - tx, 1.0 - ty
        wt = (ux * uy, tx * uy, ux * ty, tx * ty)
        ws, an = np.zeros(npx), np.zeros(npx)
        am, av = np.zeros((npx, 4)), np.zeros((npx, 3))
        tap = np.full((npx, 4), NA, dtype=np.int32)
        for t in range(4):
            qx, qy = x0 + (t & 1), y0 + (t >> 1)
            inside = (qx >= 0) & (qx < w) & (qy >= 0) & (qy < h)
            q = np.where(inside, qy * w + qx, 0)
            nq = src_n[q]
            zq = pg[q, 0]
            n_q = (pg[q, 1], pg[q, 2], pg[q, 3])
            dn = _dot3(n_p, n_q)
            nnq = _dot3(n_q, n_q)
            tests = [(OUTSIDE, inside), (NO_COUNT, nq > 0), (NODE, pi[q, 0] == node),
                     (MATERIAL, (pi[q, 1] == mat) | (P["match_material"] == 0)),
                     (DEPTH, np.isfinite(zq) & (zq > 0.0) & (np.abs(zq - e) <= tol)),
                     (NORMAL, (dn > 0.0) & (dn * dn >= cos2 * (nnp * nnq)))]
            why = np.full(npx, ACCEPT, dtype=np.int32)
            for code, passed in reversed(tests):
                why = np.where(passed, why, code)
            tap[:, t] = np.where(live, why, NA)
            take = live & (why == ACCEPT)
            wq, dq = wt[t], nq.astype(np.float64)
            ws = np.where(take, ws + wq, ws)
            am = np.where(take[:, None], am + wq[:, None] * src_mean[q], am)
            av = np.where(take[:, None], av + wq[:, None] * (src_m2[q] / dq[:, None]), av)
            an = np.where(take, an + wq * dq, an)
        heavy = ws >= np.float64(P["min_weight"])
        ok = live & heavy
        # 7
        r = an / ws + 0.5
        over = r >= np.float64(P["max_history"])
        trunc = np.where(ok & ~over, r, 0.0).astype(np.int32)
        n = np.maximum(np.where(over, np.int32(P["max_history"]), trunc), 1).astype(np.int32)
        mean = am / ws[:, None]
        m2 = (av / ws[:, None]) * n.astype(np.float64)[:, None]
        clamped = ok & (np.where(ok, np.floor(r), 0.0) > np.float64(P["max_history"]))
    reason = np.full(npx, OK, dtype=np.int32)
    for code, passed in reversed([(MISS, valid), (BEHIND, front), (RANGE_X, in_x), (RANGE_Y, in_y), (WEIGHT, heavy)]):
        reason = np.where(passed, reason, code)
    outcome = np.where(reason == OK, 0, np.where(reason == MISS, 1, 2)).astype(np.int32)
    return {"n": np.where(ok, n, 0).astype(np.int32), "mean": np.where(ok[:, None], mean, 0.0),
            "m2": np.where(ok[:, None], m2, 0.0), "outcome": outcome, "reason": reason, "tap": tap,
            "accepted": (tap == ACCEPT).sum(axis=1), "clamped": clamped}


# ---- cameras and an analytic world ----

def camera(w, h, from_, to, up=(0.0, 1.0, 0.0), fov=np.pi / 3, distance=1.0):
    """A pinhole camera as the host library's camera() and view_transform() lay it out (frt_camera's fields)."""
    fr, to, up = (np.asarray(x, dtype=np.float64) for x in (from_, to, up))
    fwd = (to - fr) / np.linalg.norm(to - fr)
    left = np.cross(fwd, up / np.linalg.norm(up))
    true_up = np.cross(left, fwd)
    orient = np.eye(4)
    orient[0, :3], orient[1, :3], orient[2, :3] = left, true_up, -fwd
    trans = np.eye(4)
    trans[:3, 3] = -fr
    inv = np.linalg.inv(orient @ trans)
    half_view = distance * np.tan(fov * 0.5)
    aspect = w / h
    hw, hh = (half_view, half_view / aspect) if aspect >= 1.0 else (half_view * aspect, half_view)
    return SimpleNamespace(hsize=w, vsize=h, half_width=hw, half_height=hh, pixel_size=hw * 2.0 / w,
                           canvas_distance=distance, inv=[float(x) for x in inv.reshape(16)])


def centre_rays(cam):
    """(origin (3,), unit directions (npx, 3)) of the pixels' centre rays."""
    w, h = cam.hsize, cam.vsize
    inv = np.asarray(cam.inv).reshape(4, 4)
    idx = np.arange(w * h)
    x = cam.half_width - ((idx % w) + 0.5) * cam.pixel_size
    y = cam.half_height - ((idx // w) + 0.5) * cam.pixel_size
    p = np.stack([x, y, np.full(w * h, -cam.canvas_distance), np.ones(w * h)], axis=1) @ inv.T
    o = inv[:3, 3]
    v = p[:, :3] - o
    return o, v / np.linalg.norm(v, axis=1, keepdims=True)


SPHERE_C, SPHERE_R = np.array([0.0, 0.0, 1.5]), 0.7
PLANE_EXTENT = 2.6  # the back plane z = 0 ends at |x|, |y| = 2.6: beyond it a ray misses


def world_features(cam):
    """First-hit features of the analytic world under `cam`: a back plane z = 0 facing +z (node 0, material 0 where
    x < 1 and material 2 beyond: one node under two materials) and a sphere in front of it (node 1, material 1).
    Returns (geom (npx, 8), ids (npx, 2), world points (npx, 3)); rays that hit nothing hold zeros and -1."""
    o, d = centre_rays(cam)
    npx = d.shape[0]
    with np.errstate(all="ignore"):
        oc = o - SPHERE_C
        b = d @ oc
        disc = b * b - (oc @ oc - SPHERE_R ** 2)
        ts = -b - np.sqrt(disc)
        hit_s = (disc > 0) & (ts > 0)
        tp = -o[2] / d[:, 2]
        pp = o + tp[:, None] * d
        hit_p = (d[:, 2] < 0) & (tp > 0) & (np.abs(pp[:, 0]) <= PLANE_EXTENT) & (np.abs(pp[:, 1]) <= PLANE_EXTENT)
    t = np.where(hit_s, ts, np.where(hit_p, tp, 0.0))
    pts = o + t[:, None] * d
    geom = np.zeros((npx, 8))
    ids = np.full((npx, 2), -1, dtype=np.int32)
    geom[:, 0] = t
    geom[hit_s, 1:4] = (pts[hit_s] - SPHERE_C) / SPHERE_R
    only_p = hit_p & ~hit_s
    geom[only_p, 1:4] = (0.0, 0.0, 1.0)
    geom[hit_s | hit_p, 4:7] = 0.5
    geom[hit_s | hit_p, 7] = 1.0
    ids[hit_s] = (1, 1)
    ids[only_p, 0] = 0
    ids[only_p, 1] = np.where(pts[only_p, 0] < 1.0, 0, 2)
    return geom, ids, pts


def world_colour(pts, ids):
    """A view-independent colour, smooth in the world point on each surface; rgba, zeros where nothing is hit."""
    k = np.array([0.7, 1.1, 0.5])
    rgb = 0.5 + 0.4 * np.sin(pts @ np.diag(k) + np.array([0.3, 1.0, 2.0]) + 1.5 * (ids[:, :1] == 1))
    out = np.concatenate([rgb, np.ones((pts.shape[0], 1))], axis=1)
    return np.where((ids[:, :1] >= 0), out, 0.0)


def identity_bound(w, h, image, origin, dmin, pixels_per_unit):
    """How far a reprojection under the same camera may move a pixel's mean.

    fx is px up to the rounding of its chain. W = O + d * dir carries an error of a few ulps of |O| + d; the previous
    camera's matrix takes it to c with the same absolute error; the projection divides by |c.z|, which is at least
    about dmin, and turns a unit of the canvas into pixels_per_unit = canvas_distance / pixel_size pixels; fx's own
    last operations round at its magnitude, at most w (fy: h). So |fx - px| + |fy - py| <= delta =
    K * 2^-53 * ((1 + |O| / dmin) * pixels_per_unit + w + h), with K = 32 covering the dozen operations of the chain
    with a margin of about two. The taps other than the pixel's own weigh at most delta together, and each differs
    from the pixel by at most the largest difference between neighbours (diagonal ones included), whether or not the
    tap tests accept them. The weighted mean's own rounding adds a few ulps of the largest value:
    16 * 2^-53 * max|value|."""
    image = np.asarray(image).reshape(h, w, -1)
    diff = 0.0
    for dy, dx in ((0, 1), (1, 0), (1, 1), (1, -1)):
        a = image[dy:, max(0, -dx):w - max(0, dx)]
        b = image[:h - dy, max(0, dx):w - max(0, -dx)]
        if a.size:
            diff = max(diff, float(np.abs(a - b).max()))
    delta = 32 * 2.0 ** -53 * ((1.0 + origin / dmin) * pixels_per_unit + w + h)
    return delta * diff + 16 * 2.0 ** -53 * float(np.abs(image).max())


# ---- the cases the host and the device tests share (rt: fast_ray_tracer_amd.runtime) ----

SIZES = [(1, 1), (63, 2), (64, 4), (65, 3), (130, 67)]
PAIRS = ["identical", "subpixel_pan", "pan", "rotation", "tilt", "behind"]


def flat(rt, cam):
    c = rt.FlatCamera()
    c.hsize, c.vsize, c.usteps, c.vsteps = cam.hsize, cam.vsize, 1, 1
    c.half_width, c.half_height, c.pixel_size = cam.half_width, cam.half_height, cam.pixel_size
    c.canvas_distance = cam.canvas_distance
    c.inv[:] = cam.inv
    c.aperture_type = 6  # (a point)
    return c


def camera_pair(name, w, h):
    """(prev, cur) over the analytic world; the back plane is 5 away, so a pixel of it is about 5.77 / w wide."""
    pixel = 5.77 / w
    cur = camera(w, h, (0.0, 0.0, 5.0), (0.0, 0.0, 0.0))
    if name == "identical":
        return cur, cur
    if name == "subpixel_pan":
        return camera(w, h, (0.3 * pixel, 0.0, 5.0), (0.3 * pixel, 0.0, 0.0)), cur
    if name == "pan":
        return camera(w, h, (4.3 * pixel, -1.6 * pixel, 5.0), (4.3 * pixel, -1.6 * pixel, 0.0)), cur
    if name == "rotation":
        return camera(w, h, (0.0, 0.0, 5.0), (2.0, 0.0, 0.0)), cur
    if name == "tilt":
        return camera(w, h, (0.0, 0.0, 5.0), (0.0, 5.0 * np.tan(np.pi / 6) * h / w, 0.0)), cur
    if name == "behind":  # the previous camera stands between the sphere and the plane: the sphere is behind it
        return camera(w, h, (0.0, 0.0, 0.5), (0.0, 0.0, -1.0)), cur
    raise KeyError(name)


def case_params(w, h, name):
    """Most cases run the defaults; some a history the source's counts exceed, some a weight floor of a half."""
    p = {}
    if name in ("pan", "identical"):
        p["max_history"] = 2
    if name == "subpixel_pan":
        p["min_weight"] = 0.5
    if name == "rotation":
        p["match_material"] = 0
    return p


def disturb(geom, ids, seed):
    """A few previous pixels with another material, another depth, a NaN depth and a turned normal (in place)."""
    npx = geom.shape[0]
    if npx < 64:
        return
    rng = np.random.default_rng(seed)
    pick = rng.choice(npx, size=(4, max(2, npx // 40)), replace=False)
    ids[pick[0], 1] = 7
    geom[pick[1], 0] *= 1.5
    geom[pick[2, ::2], 0] = np.nan
    geom[pick[3], 1:4] = geom[pick[3], 1:4] @ np.array([[0.0, 1.0, 0.0], [-1.0, 0.0, 0.0], [0.0, 0.0, 0.2]])


def build_case(rt, w, h, name):
    prev, cur = camera_pair(name, w, h)
    pgeom, pids, _ = world_features(prev)
    cgeom, cids, _ = world_features(cur)
    disturb(pgeom, pids, seed=w * 131 + h)
    xs = accum_ref.samples(w * h, 4, seed=w * h)
    if w * h >= 64:  # (two pixels in the image's middle that never count a sample, as samples' pixel 0 in its corner)
        xs[:, [(h // 2) * w + w // 3, (h // 2) * w + w // 2], 1] = np.nan
    wf = accum_ref.Welford(w * h)
    for x in xs:
        wf.add(x)
    params = case_params(w, h, name)
    fprev, fcur = flat(rt, prev), flat(rt, cur)
    g = rt.reproject_setup(fprev, fcur)
    want = reproject(wf.n, wf.mean, wf.m2, prev, cur, list(g.o_cur), list(g.o_prev), list(g.prev_fwd), pgeom, pids,
                     cgeom, cids, w, h, params)
    return {"w": w, "h": h, "name": name, "prev": fprev, "cur": fcur, "pfeat": (pgeom, pids), "cfeat": (cgeom, cids),
            "xs": xs, "params": params, "want": want, "src": wf}


_cases = {}


def get_case(rt, w, h, name):
    key = (w, h, name)
    if key not in _cases:
        _cases[key] = build_case(rt, w, h, name)
    return _cases[key]
