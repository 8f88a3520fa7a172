"""A numpy reference of the variance-guided denoise (include/frt_device.h "Variance-guided denoise"), written from
its definition and not from the C pass, the seeded variance its tests add to denoise_ref.random_inputs, and the
synthetic image of the behaviour tests.

As in denoise_ref: vectorised over pixels, the taps a sequential loop (dy outside, dx inside), every ufunc call one
IEEE binary64 operation per element.
"""
import numpy as np

import accum_ref
import denoise_ref

K = denoise_ref.K
G = (1.0 / 2.0, 1.0 / 4.0)
DEFAULTS = {"iterations": 5, "sigma_color": 2.0, "sigma_depth": 0.1, "normal_squarings": 5, "demodulate": 1,
            "match_material": 1, "albedo_eps": 2.0 ** -10, "var_eps": 2.0 ** -40}


def valid_mask(rgba, var, geom, ids):
    with np.errstate(all="ignore"):
        ok = np.isfinite(var[..., 0]) & (var[..., 0] >= 0) & np.isfinite(var[..., 1]) & (var[..., 1] >= 0) & \
            np.isfinite(var[..., 2]) & (var[..., 2] >= 0)
    return denoise_ref.valid_mask(rgba, geom, ids) & ok


def _windows(h, w, oy, ox):
    py = slice(max(0, -oy), min(h, h - oy))
    px = slice(max(0, -ox), min(w, w - ox))
    if py.start >= py.stop or px.start >= px.stop:
        return None
    return (py, px), (slice(py.start + oy, py.stop + oy), slice(px.start + ox, px.stop + ox))


def _image(rgba, var, geom, ids, p):
    h, w = rgba.shape[:2]
    valid = valid_mask(rgba, var, geom, ids)
    out, out_var = rgba.copy(), var.copy()
    with np.errstate(all="ignore"):
        if p["demodulate"]:
            a = geom[..., 4:7] + p["albedo_eps"]
        else:
            a = np.ones((h, w, 3))
        x = rgba[..., :3] / a
        v = var[..., :3] / (a * a)
        n0, n1, n2 = geom[..., 1], geom[..., 2], geom[..., 3]
        nn = (n0 * n0 + n1 * n1) + n2 * n2
        inv_nn = np.where(nn > 0, 1.0 / nn, 0.0)
        z = geom[..., 0]
        iz = 1.0 / z
        mat = ids[..., 1]
        kz = 1.0 / (p["sigma_depth"] * p["sigma_depth"])
        kc = 1.0 / (p["sigma_color"] * p["sigma_color"])
        for i in range(p["iterations"]):
            s = 1 << i
            # the guide: 3 x 3 at distance 1
            vs = (v[..., 0] + v[..., 1]) + v[..., 2]
            gsum = np.zeros((h, w))
            gw = np.zeros((h, w))
            for dy in range(-1, 2):
                for dx in range(-1, 2):
                    win = _windows(h, w, dy, dx)
                    if win is None:
                        continue
                    P, Q = win
                    g = G[abs(dx)] * G[abs(dy)]
                    use = valid[P] & valid[Q]
                    gsum[P] = np.where(use, gsum[P] + g * vs[Q], gsum[P])
                    gw[P] = np.where(use, gw[P] + g, gw[P])
            kc_p = kc / (gsum / gw + p["var_eps"])
            acc = np.zeros((h, w, 3))
            vacc = np.zeros((h, w, 3))
            ws = np.zeros((h, w))
            for dy in range(-2, 3):
                for dx in range(-2, 3):
                    win = _windows(h, w, s * dy, s * dx)
                    if win is None:
                        continue  # every q outside the image
                    P, Q = win
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
                        xc = ((dc0 * dc0 + dc1 * dc1) + dc2 * dc2) * kc_p[P]
                        u = (1.0 + xz) * (1.0 + xc)
                        wgt = (hk * t) / (u * u)
                    w2 = wgt * wgt
                    for ch in range(3):
                        acc[P + (ch,)] = np.where(use, acc[P + (ch,)] + wgt * x[Q + (ch,)], acc[P + (ch,)])
                        vacc[P + (ch,)] = np.where(use, vacc[P + (ch,)] + w2 * v[Q + (ch,)], vacc[P + (ch,)])
                    ws[P] = np.where(use, ws[P] + wgt, ws[P])
            x = acc / ws[..., None]
            v = vacc / (ws * ws)[..., None]
        rgb = x * a
        vout = v * (a * a)
    out[valid, :3] = rgb[valid]
    out_var[valid, :3] = vout[valid]
    return out, out_var


def denoise_var(rgba, var, geom, ids, **params):
    """(out, out_var) for rgba, var (h, w, 4) or (K, h, w, 4); params over DEFAULTS."""
    p = dict(DEFAULTS)
    p.update(params)
    if rgba.ndim == 3:
        return _image(rgba, var, geom, ids, p)
    pairs = [_image(rgba[k], var[k], geom[k], ids[k], p) for k in range(rgba.shape[0])]
    return np.stack([a for a, _ in pairs]), np.stack([b for _, b in pairs])


def random_var(shape, seed, among=None):
    """A seeded variance for denoise_ref.random_inputs(shape, ..): uniform in [0, 0.1], about 10 % exact zeros, the
    sample count 4 in channel 3 and, where there is room, one negative value and one NaN (those pixels pass through),
    both at pixels of the mask `among` (the pixels valid by everything else) when it is given and holds two."""
    rng = np.random.default_rng(1000 + seed)
    shape = tuple(shape)
    npx = int(np.prod(shape))
    var = rng.uniform(0.0, 0.1, (npx, 4))
    var[rng.random((npx, 4)) < 0.1] = 0.0
    var[:, 3] = 4.0
    where = np.arange(npx) if among is None else np.flatnonzero(np.asarray(among).reshape(-1))
    if npx >= 8 and where.size >= 2:
        a, b = rng.choice(where, 2, replace=False)
        var[a, rng.integers(0, 3)] = -0.01
        var[b, rng.integers(0, 3)] = np.nan
    return var.reshape(shape + (4,))


# ---------------------------------------------------------------------------------------------------------------------
# the synthetic image of the behaviour tests

def synthetic(h, w):
    """(truth (h, w, 4), geom, ids): a checkered albedo (16-pixel squares, 0.8 / 0.3 times (1, 0.7, 0.5)) under the
    smooth irradiance 0.2 + 0.8 x / w + 0.3 sin^2(y / 7); flat normal, depth and material."""
    yy, xx = np.mgrid[0:h, 0:w]
    check = ((yy // 16) + (xx // 16)) % 2 == 0
    albedo = np.where(check, 0.8, 0.3)[..., None] * np.array([1.0, 0.7, 0.5])
    irr = 0.2 + 0.8 * xx / w + 0.3 * np.sin(yy / 7.0) ** 2
    truth = np.ones((h, w, 4))
    truth[..., :3] = albedo * irr[..., None]
    geom = np.zeros((h, w, 8))
    geom[..., 0] = 5.0
    geom[..., 1:4] = (0.0, 0.0, -1.0)
    geom[..., 4:7] = albedo
    geom[..., 7] = 1.0
    ids = np.ones((h, w, 2), dtype=np.int32)
    return truth, geom, ids


def accumulate_noisy(truth, geom, n, sigma, seed, noisy_from=0):
    """The Welford mean and variance of n samples of truth plus Gaussian noise of std sigma x albedo per sample in the
    columns from noisy_from on (the columns before it are noise-free): (mean, var), (h, w, 4) each."""
    h, w = truth.shape[:2]
    rng = np.random.default_rng(seed)
    acc = accum_ref.Welford(h * w)
    for _ in range(n):
        x = truth.copy()
        noise = sigma * geom[..., 4:7] * rng.standard_normal((h, w, 3))
        x[:, noisy_from:, :3] += noise[:, noisy_from:]
        acc.add(x)
    mean, var = acc.resolve()
    return mean.reshape(h, w, 4), var.reshape(h, w, 4)
