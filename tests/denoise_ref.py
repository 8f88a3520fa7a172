"""A numpy reference of the denoise (include/frt_device.h "Denoise"), written from its definition and not from the C
pass, and the seeded inputs the denoise tests share.

The reference is vectorised over pixels; the 25 taps stay a sequential loop (dy outside, dx inside), so each pixel's
additions keep the definition's order. Dot products and three-term sums are written out: every ufunc call is one
IEEE binary64 operation per element, nothing is fused or reordered (no @, np.dot or sum()).
"""
import numpy as np

K = (3.0 / 8.0, 1.0 / 4.0, 1.0 / 16.0)
DEFAULTS = {"iterations": 5, "sigma_color": 1.0, "sigma_depth": 0.1, "normal_squarings": 5, "demodulate": 1,
            "match_material": 1, "albedo_eps": 2.0 ** -10}


def valid_mask(rgba, geom, ids):
    depth = geom[..., 0]
    return ((ids[..., 0] >= 0) & np.isfinite(depth) & (depth > 0) & np.isfinite(rgba[..., 0]) &
            np.isfinite(rgba[..., 1]) & np.isfinite(rgba[..., 2]))


def _image(rgba, geom, ids, p):
    h, w = rgba.shape[:2]
    valid = valid_mask(rgba, geom, ids)
    out = rgba.copy()
    with np.errstate(all="ignore"):
        if p["demodulate"]:
            a = geom[..., 4:7] + p["albedo_eps"]
        else:
            a = np.ones((h, w, 3))
        x = rgba[..., :3] / a
        n0, n1, n2 = geom[..., 1], geom[..., 2], geom[..., 3]
        nn = (n0 * n0 + n1 * n1) + n2 * n2
        inv_nn = np.where(nn > 0, 1.0 / nn, 0.0)
        z = geom[..., 0]
        iz = 1.0 / z
        mat = ids[..., 1]
        kz = 1.0 / (p["sigma_depth"] * p["sigma_depth"])
        for i in range(p["iterations"]):
            s = 1 << i
            kc = float(np.ldexp(1.0 / (p["sigma_color"] * p["sigma_color"]), 2 * i))
            acc = np.zeros((h, w, 3))
            ws = np.zeros((h, w))
            for dy in range(-2, 3):
                for dx in range(-2, 3):
                    oy, ox = s * dy, s * dx
                    py = slice(max(0, -oy), min(h, h - oy))
                    px = slice(max(0, -ox), min(w, w - ox))
                    if py.start >= py.stop or px.start >= px.stop:
                        continue  # every q outside the image
                    qy = slice(py.start + oy, py.stop + oy)
                    qx = slice(px.start + ox, px.stop + ox)
                    P, Q = (py, px), (qy, qx)
                    hk = K[abs(dx)] * K[abs(dy)]
                    use = valid[P] & valid[Q]
                    if dx == 0 and dy == 0:
                        wgt = np.full(use.shape, hk)
                    else:
                        if p["match_material"]:
                            use = use & (mat[Q] == mat[P])
                        d = (n0[P] * n0[Q] + n1[P] * n1[Q]) + n2[P] * n2[Q]
                        use = use & ~(d <= 0)
                        m = (d * d) * (inv_nn[P] * inv_nn[Q])
                        t = np.where(m < 1.0, m, 1.0)
                        for _ in range(p["normal_squarings"]):
                            t = t * t
                        r = z[P] - z[Q]
                        xz = ((r * r) * kz) * (iz[P] * iz[Q])
                        dc0 = x[P + (0,)] - x[Q + (0,)]
                        dc1 = x[P + (1,)] - x[Q + (1,)]
                        dc2 = x[P + (2,)] - x[Q + (2,)]
                        xc = ((dc0 * dc0 + dc1 * dc1) + dc2 * dc2) * kc
                        u = (1.0 + xz) * (1.0 + xc)
                        wgt = (hk * t) / (u * u)
                    for ch in range(3):
                        acc[P + (ch,)] = np.where(use, acc[P + (ch,)] + wgt * x[Q + (ch,)], acc[P + (ch,)])
                    ws[P] = np.where(use, ws[P] + wgt, ws[P])
            x = acc / ws[..., None]
        rgb = x * a
    out[valid, :3] = rgb[valid]
    return out


def denoise(rgba, geom, ids, **params):
    """The filtered copy of rgba (h, w, 4) or (K, h, w, 4); params over DEFAULTS."""
    p = dict(DEFAULTS)
    p.update(params)
    if rgba.ndim == 3:
        return _image(rgba, geom, ids, p)
    return np.stack([_image(rgba[k], geom[k], ids[k], p) for k in range(rgba.shape[0])])


BASE_NORMALS = np.array([(0.0, 0.0, -1.0), (1.0, 0.0, 0.0), (0.6, 0.0, -0.8), (0.0, 1.0, 0.0)])


def random_inputs(shape, seed):
    """Seeded inputs of shape (h, w) or (K, h, w): normals not normalised (a base direction plus noise, scaled by
    0.5 .. 2) and some exactly zero, depth in [1, 10], albedo in [0, 1] with exact zeros, materials in {0, 1, 2},
    about 10 % of the pixels invalid by id and, where there is room, one pixel with a NaN and one with an infinite
    colour channel. Returns (rgba, geom, ids)."""
    rng = np.random.default_rng(seed)
    shape = tuple(shape)
    npx = int(np.prod(shape))
    normal = BASE_NORMALS[rng.integers(0, 4, npx)] + 0.1 * rng.standard_normal((npx, 3))
    normal *= rng.uniform(0.5, 2.0, (npx, 1))
    normal[rng.random(npx) < 0.05] = 0.0
    depth = rng.uniform(1.0, 10.0, npx)
    albedo = rng.uniform(0.0, 1.0, (npx, 3))
    albedo[rng.random((npx, 3)) < 0.1] = 0.0
    geom = np.concatenate([depth[:, None], normal, albedo, rng.uniform(0.0, 1.0, (npx, 1))], axis=1)
    ids = np.stack([rng.integers(0, 50, npx), rng.integers(0, 3, npx)], axis=1).astype(np.int32)
    ids[rng.random(npx) < 0.1] = -1
    rgba = rng.uniform(0.0, 2.0, (npx, 4))
    if npx >= 8:
        a, b = rng.choice(npx, 2, replace=False)
        rgba[a, rng.integers(0, 3)] = np.nan
        rgba[b, rng.integers(0, 3)] = np.inf
        ids[a], ids[b] = (3, 1), (4, 2)  # (invalid by their colour alone)
    return (rgba.reshape(shape + (4,)), geom.reshape(shape + (8,)), ids.reshape(shape + (2,)))
