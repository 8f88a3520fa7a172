"""An independent first-hit reference: the closest hit of every camera sample of a Scene / View, its t, its normal
and its leaf, in np.longdouble arithmetic (numpy only, no GPU, no oracle).

Inputs: the flattened scene (runtime._flat_scene; nodes, roots, xforms, prim_data and materials at the offsets of
include/frt_device.h) and the binary64 camera rays of feature_ref.camera_rays. From the rays on everything is
extended precision: the ray goes down the tree through each node's inverse transform, every leaf is intersected
with the reference's rules (the device lines they mirror are cited at each), the smallest t > 0 over all leaves wins
(hit_index, oracle/frt_oracle.c), the local normal is carried back through the transposed inverses and turned towards
the eye. Group boxes and triangle batches are culled in binary64 with a slack of 1e-6, which can only drop misses.
A scene with a CSG node is refused.

Per sample the reference also returns a margin: the smallest distance of any decision it took from flipping,
relative to the sum of the absolute values of the compared expression's terms (and the threshold). A sample is
undecided when that is under 1e-9; the discriminant uses |disc| < 1e-7 (b^2 + 4 |a c|), scaled to the same threshold.
The toroid's roots are the real roots of its quartic: np.roots in binary64 as the start, Newton steps in longdouble."""
import ctypes

import numpy as np

import feature_ref

LD = np.longdouble
assert np.finfo(LD).nmant >= 63
EPS = LD(1e-5)      # the reference's EPSILON (the binary64 value), kEps in csrc/frt_math.hpp
REL = LD(1e-9)      # a decision closer than this (relative) to its threshold is undecided
DISC_REL = LD(1e-7)
CULL = 1e-6         # slack of the binary64 culls
(CONE, CUBE, CYLINDER, PLANE, SMOOTH_TRIANGLE, SPHERE, TOROID, TRIANGLE, CSG, GROUP) = range(10)
TYPE_NAMES = {CONE: "cone", CUBE: "cube", CYLINDER: "cylinder", PLANE: "plane", SMOOTH_TRIANGLE: "smooth_triangle",
              SPHERE: "sphere", TOROID: "toroid", TRIANGLE: "triangle"}
BRANCHES = ("slab_parallel", "plane_parallel", "caps_skipped", "cone_a_zero", "cone_single_root", "inside")


class FlatSceneHead(ctypes.Structure):  # frt_scene up to its camera (include/frt_device.h)
    _fields_ = [("abi_version", ctypes.c_uint32), ("num_nodes", ctypes.c_int32), ("nodes", ctypes.c_void_p),
                ("num_roots", ctypes.c_int32), ("pad0", ctypes.c_int32), ("roots", ctypes.c_void_p),
                ("num_xforms", ctypes.c_int32), ("pad1", ctypes.c_int32), ("xforms", ctypes.c_void_p),
                ("prim_len", ctypes.c_int64), ("prim_data", ctypes.c_void_p),
                ("num_materials", ctypes.c_int32), ("num_patterns", ctypes.c_int32), ("materials", ctypes.c_void_p),
                ("patterns", ctypes.c_void_p), ("num_textures", ctypes.c_int32), ("pad2", ctypes.c_int32),
                ("textures", ctypes.c_void_p), ("texel_len", ctypes.c_int64), ("texels", ctypes.c_void_p),
                ("num_lights", ctypes.c_int32), ("pad3", ctypes.c_int32), ("lights", ctypes.c_void_p),
                ("light_point_len", ctypes.c_int64), ("light_points", ctypes.c_void_p),
                ("camera", feature_ref.FlatCamera)]


MATERIAL_BYTES, MATERIAL_MAP_BUMP = 184, 172  # frt_material: 18 doubles, then 9 int32 (map_bump the 8th) and a pad


def flat_tree(view):
    """{"nodes" (structured, runtime._NODE_DTYPE), "roots", "xforms" (n, 4, 4), "prim" (doubles), "bump" (per
    material: it has a map_bump)} of a Scene / View."""
    from fast_ray_tracer_amd.runtime import _NODE_DTYPE, _flat_scene
    lib, fs = _flat_scene(view)
    try:
        lib.frt_scene_camera_offset.restype = ctypes.c_size_t
        assert lib.frt_scene_camera_offset() == FlatSceneHead.camera.offset and _NODE_DTYPE.itemsize == 80
        head = FlatSceneHead.from_buffer_copy(fs)
        assert head.abi_version == 3

        def arr(ptr, count, dtype):
            dtype = np.dtype(dtype)
            if count <= 0:
                return np.zeros(0, dtype=dtype)
            return np.frombuffer(ctypes.string_at(ptr, count * dtype.itemsize), dtype=dtype).copy()

        mats = arr(head.materials, head.num_materials * MATERIAL_BYTES, np.uint8).reshape(-1, MATERIAL_BYTES)
        bump = mats[:, MATERIAL_MAP_BUMP:MATERIAL_MAP_BUMP + 4].copy().view("<i4")[:, 0] >= 0
        return {"nodes": arr(head.nodes, head.num_nodes, _NODE_DTYPE), "roots": arr(head.roots, head.num_roots, "<i4"),
                "xforms": arr(head.xforms, 16 * head.num_xforms, "<f8").reshape(-1, 4, 4),
                "prim": arr(head.prim_data, head.prim_len, "<f8"), "bump": bump}
    finally:
        lib.frt_flat_scene_free(fs)


def _dot(a, b):
    return a[..., 0] * b[..., 0] + a[..., 1] * b[..., 1] + a[..., 2] * b[..., 2]


def _cross(a, b):
    return np.stack([a[..., 1] * b[..., 2] - a[..., 2] * b[..., 1], a[..., 2] * b[..., 0] - a[..., 0] * b[..., 2],
                     a[..., 0] * b[..., 1] - a[..., 1] * b[..., 0]], axis=-1)


def _unit(v):
    return v / np.sqrt(_dot(v, v))[..., None]


# ---------------------------------------------------------------------------------------------------------------
# the toroid's quartic

def quartic_coeffs(o, d, r1, r2):
    """c[..., k] of sum c_k t^k = (|o + t d|^2 - r1^2 - r2^2)^2 - 4 r1^2 (r2^2 - (o_y + t d_y)^2), any float type."""
    dd, e, f = _dot(d, d), _dot(o, o) - r1 * r1 - r2 * r2, _dot(o, d)
    fa = 4 * r1 * r1
    return np.stack([e * e - fa * (r2 * r2 - o[..., 1] * o[..., 1]), 4 * f * e + 2 * fa * o[..., 1] * d[..., 1],
                     2 * dd * e + 4 * f * f + fa * d[..., 1] * d[..., 1], 4 * dd * f, dd * dd], axis=-1)


def _poly(c, x):
    p, dp, s, ds = c[4], LD(0), abs(c[4]), LD(0)
    for k in (3, 2, 1, 0):  # Horner, with the sums of absolute values next to it
        dp, ds = dp * x + p, ds * abs(x) + s
        p, s = p * x + c[k], s * abs(x) + abs(c[k])
    return p, dp, s, ds


QUARTIC_ZERO = 2e-9


def solver_epsilons(c, z):
    """The smallest magnitude among the quantities the reference's quartic solver (Roots3And4.c, restated in
    oracle/frt_oracle.c:123-233 and csrc/frt_math.hpp) compares against its absolute EQN_EPS = 1e-9, from the
    binary64 coefficients c and roots z: with y = t + A / 4 the roots of the depressed quartic y^4 + p y^2 + q y + r,
    these are r; the resolvent cubic's discriminant (and its q where that vanishes); and for a split into two
    quadratics over the root pairs {a, b}, {c, d}: (y_a + y_b)^2 (the solver's v before its root),
    ((y_c y_d - y_a y_b) / 2)^2 (its u) and the quadratics' ((y_a - y_b) / 2)^2. Which of the three splits the solver
    takes depends on the cubic root it picks, so all three count. Under EQN_EPS the solver takes a degenerate
    branch, which for a quartic whose roots merely lie close together (their differences enter these quantities in
    powers up to the twelfth) is not the branch of its real roots: it returns other roots or none. This reference
    finds the real roots and does not restate that branch, so a sample on which any of them is under QUARTIC_ZERO
    (EQN_EPS and as much again for the solver's own rounding: terms of 1e5 cancel in r) is undecided."""
    A, B, C, D = c[3] / c[4], c[2] / c[4], c[1] / c[4], c[0] / c[4]
    p = -3 / 8 * A * A + B
    q = A * A * A / 8 - A * B / 2 + C
    r = -3 / 256 * A ** 4 + A * A * B / 16 - A * C / 4 + D
    found = [abs(r)]
    a2, a1, a0 = -p / 2, -r, r * p / 2 - q * q / 8  # the resolvent cubic x^3 + a2 x^2 + a1 x + a0
    cp = (a1 - a2 * a2 / 3) / 3
    cq = (2 / 27 * a2 ** 3 - a2 * a1 / 3 + a0) / 2
    found.append(abs(cq * cq + cp ** 3))
    y = z + A / 4
    for (i, j), (k, m) in (((0, 1), (2, 3)), ((0, 2), (1, 3)), ((0, 3), (1, 2))):
        found += [abs((y[i] + y[j]) ** 2), abs((y[k] * y[m] - y[i] * y[j]) / 2) ** 2,
                  abs((y[i] - y[j]) / 2) ** 2, abs((y[k] - y[m]) / 2) ** 2]
    return min(found)


_SPLIT = LD(2) ** 32 + 1


def _two_prod(a, b):
    """a * b = p + e exactly (Dekker's split at 32 of the 64 mantissa bits)."""
    p = a * b
    t = _SPLIT * a
    ah = t - (t - a)
    al = a - ah
    t = _SPLIT * b
    bh = t - (t - b)
    bl = b - bh
    return p, ((ah * bh - p) + ah * bl + al * bh) + al * bl


def _poly_compensated(c, x):
    """p(x) by the compensated Horner scheme (Graillat, Langlois, Louvet 2009): as accurate as Horner's in twice the
    working precision, so a Newton step ends at the root's longdouble rounding, not at its condition number."""
    s, comp = c[4], LD(0)
    for k in (3, 2, 1, 0):
        p, pe = _two_prod(s, x)
        s = p + c[k]
        bb = s - p
        comp = comp * x + (pe + ((p - (s - bb)) + (c[k] - bb)))
    return s + comp


def quartic_real_roots(c):
    """The real roots of one quartic c (5 longdouble, ascending powers), refined in longdouble, ascending, with the
    polynomial's clearance from a double root: (roots, clear, clear_im, solver_epsilons()). clear is the smallest of
    |x p'(x)| / sum k |c_k x^k| over the roots, the reciprocal of a root's condition number up to the cancellation in
    p itself: under 1e-7 (the discriminant's clearance) t's conditioning is no longer bounded as the quadratics' is.
    clear_im is the smallest |Im z| / |z| over the complex roots: under 3e-4 (the square root of that clearance: the
    imaginary part grows as the root of the distance from tangency) the number of real roots is in doubt."""
    z = np.roots(np.asarray(c[::-1], dtype=np.float64))
    roots, clear, clear_im = [], LD(np.inf), LD(np.inf)
    for zi in z:
        x = LD(zi.real)
        for _ in range(60):
            p, dp, s, ds = _poly(c, x)
            if dp == 0:
                break
            step = _poly_compensated(c, x) / dp
            x = x - step
            if abs(step) <= LD(1e-18) * abs(x):
                break
        p, dp, s, ds = _poly(c, x)
        if abs(p) <= LD(1e-17) * s and not any(abs(x - y) <= LD(1e-12) * (abs(x) + abs(y)) for y in roots):
            roots.append(x)
            clear = min(clear, abs(x * dp) / (abs(x) * ds) if x != 0 and ds > 0 else LD(np.inf))
        if zi.imag != 0:
            clear_im = min(clear_im, LD(abs(zi.imag) / max(abs(zi), 1e-300)))
    return sorted(roots), clear, clear_im, solver_epsilons(np.asarray(c, dtype=np.float64), z)


# ---------------------------------------------------------------------------------------------------------------

class _State:
    def __init__(self, n):
        self.t = np.full(n, np.inf, dtype=LD)
        self.t_other = np.full(n, np.inf, dtype=LD)  # smallest positive t of a leaf other than the best one's
        self.leaf = np.full(n, -1, dtype=np.int64)
        self.uv = np.zeros((n, 2), dtype=LD)
        self.lo = np.zeros((n, 3), dtype=LD)
        self.ld = np.zeros((n, 3), dtype=LD)
        self.margin = np.full(n, np.inf, dtype=LD)
        self.branch = {k: np.zeros(n, dtype=bool) for k in BRANCHES}

    def decide(self, idx, diff, sumabs, where=None, rel=None):
        """A comparison `expr against thr` was taken for rays idx: diff = expr - thr, sumabs the sum of the absolute
        values of expr's terms and thr. `where` limits it to the rays on which the comparison mattered."""
        with np.errstate(all="ignore"):
            sumabs = np.broadcast_to(np.asarray(sumabs, dtype=LD), diff.shape)
            m = np.where(np.isfinite(diff) & np.isfinite(sumabs) & (sumabs > 0), np.abs(diff) / sumabs, LD(np.inf))
        if rel is not None:
            m = m * (REL / rel)
        if where is not None:
            m = np.where(where, m, LD(np.inf))
        self.margin[idx] = np.minimum(self.margin[idx], m)

    def offer(self, idx, t, tsum, leaf, o, d, valid, uv=None):
        """Leaf `leaf` lists t on the rays idx[valid]; tsum: the sum of the absolute values of t's terms."""
        self.decide(idx, t, tsum, where=valid)  # t against 0
        with np.errstate(invalid="ignore"):
            pos = valid & (t > 0)
        cur, other, cur_leaf = self.t[idx], self.t_other[idx], self.leaf[idx]
        better = pos & (t < cur)
        same = cur_leaf == leaf
        other = np.where(better & ~same, np.minimum(other, cur), other)
        other = np.where(pos & ~better & ~same, np.minimum(other, t), other)
        self.t_other[idx] = other
        b = idx[better]
        self.t[b], self.leaf[b], self.lo[b], self.ld[b] = t[better], leaf if np.isscalar(leaf) else leaf[better], \
            o[better], d[better]
        if uv is not None:
            self.uv[b] = uv[better]


def _quadratic(st, idx, a, b, c, where=None):
    """The discriminant's hit mask and the sorted roots of a t^2 + b t + c with the sum of the absolute values of
    their terms; the discriminant's clearance is recorded (on the rays `where`)."""
    disc = b * b - 4 * a * c
    st.decide(idx, disc, b * b + 4 * np.abs(a * c), where=where, rel=DISC_REL)
    hit = disc >= 0
    sq = np.sqrt(np.where(hit, disc, 0))
    with np.errstate(all="ignore"):
        t0, t1 = (-b - sq) / (2 * a), (-b + sq) / (2 * a)
        tsum = (np.abs(b) + sq) / np.abs(2 * a)
        swap = t0 > t1
    return hit, np.where(swap, t1, t0), np.where(swap, t0, t1), tsum


def _slab(st, idx, o, d):
    """check_axis (slab(), csrc/frt_math.hpp:244-283) for the planes -1 / +1 of one axis."""
    st.decide(idx, np.abs(d) - EPS, np.abs(d) + EPS)
    par = np.abs(d) < EPS
    nl, nh = -1 - o, 1 - o
    st.decide(idx, nl, 1 + np.abs(o), where=par)  # the sign of n picks the infinity
    st.decide(idx, nh, 1 + np.abs(o), where=par)
    with np.errstate(all="ignore"):
        t0 = np.where(par, np.where(nl < 0, -LD(np.inf), LD(np.inf)), nl / d)
        t1 = np.where(par, np.where(nh < 0, -LD(np.inf), LD(np.inf)), nh / d)
        tsum = np.where(par, LD(np.inf), (1 + np.abs(o)) / np.abs(d))
    return np.minimum(t0, t1), np.maximum(t0, t1), tsum, par


def _leaf(st, typ, p, leaf, idx, o, d):
    """leaf_hits (csrc/frt_math.hpp:653-793) on the rays idx, o / d in the leaf's space."""
    n = len(idx)
    every = np.ones(n, dtype=bool)
    ox, oy, oz, dx, dy, dz = o[:, 0], o[:, 1], o[:, 2], d[:, 0], d[:, 1], d[:, 2]
    if typ == SPHERE:  # frt_math.hpp:657-669
        hit, t0, t1, tsum = _quadratic(st, idx, _dot(d, d), 2 * _dot(d, o), _dot(o, o) - 1)
        st.offer(idx, t0, tsum, leaf, o, d, hit)
        st.offer(idx, t1, tsum, leaf, o, d, hit)
    elif typ == PLANE:  # frt_math.hpp:682-686
        st.decide(idx, np.abs(dy) - EPS, np.abs(dy) + EPS)
        par = np.abs(dy) < EPS
        st.branch["plane_parallel"][idx[par]] = True
        with np.errstate(all="ignore"):
            st.offer(idx, -oy / dy, LD(np.inf), leaf, o, d, ~par)
    elif typ == CUBE:  # frt_math.hpp:670-681
        lo, hi, ts, pars = zip(*(_slab(st, idx, o[:, k], d[:, k]) for k in range(3)))
        tmin, tmax = np.maximum(np.maximum(lo[0], lo[1]), lo[2]), np.minimum(np.minimum(hi[0], hi[1]), hi[2])
        with np.errstate(invalid="ignore"):
            st.decide(idx, tmin - tmax, np.abs(tmin) + np.abs(tmax))
        hit = ~(tmin > tmax)
        st.branch["slab_parallel"][idx[(pars[0] | pars[1] | pars[2]) & hit]] = True
        tsum = np.minimum(np.minimum(ts[0], ts[1]), ts[2])
        st.offer(idx, tmin, tsum, leaf, o, d, hit & np.isfinite(tmin))
        st.offer(idx, tmax, tsum, leaf, o, d, hit & np.isfinite(tmax))
    elif typ in (CYLINDER, CONE):  # frt_math.hpp:708-736 / 737-767
        mn, mx, closed = LD(p[0]), LD(p[1]), p[2] != 0.0
        cone = typ == CONE
        if cone:
            a, asum = dx * dx + dz * dz - dy * dy, _dot(d, d)
            b, bsum = 2 * (ox * dx + oz * dz - oy * dy), 2 * (np.abs(ox * dx) + np.abs(oz * dz) + np.abs(oy * dy))
            c = ox * ox + oz * oz - oy * oy
        else:
            a = dx * dx + dz * dz
            asum = a
            b, c = 2 * (ox * dx + oz * dz), ox * ox + oz * oz - 1
        st.decide(idx, np.abs(a) - EPS, asum + EPS)  # feq(a, 0)
        a0 = np.abs(a) < EPS
        go_on = every.copy()  # (a negative discriminant returns before the caps)
        if cone:
            st.branch["cone_a_zero"][idx[a0]] = True
            st.decide(idx, np.abs(b) - EPS, bsum + EPS, where=a0)  # feq(b, 0)
            single = a0 & ~(np.abs(b) < EPS)
            st.branch["cone_single_root"][idx[single]] = True
            with np.errstate(all="ignore"):
                st.offer(idx, -c / (2 * b), LD(np.inf), leaf, o, d, single)
        hit, t0, t1, tsum = _quadratic(st, idx, a, b, c, where=~a0)
        go_on &= a0 | hit
        for t in (t0, t1):
            y = oy + t * dy
            ysum = np.abs(oy) + np.abs(t * dy)
            w = ~a0 & hit
            st.decide(idx, y - mn, ysum + abs(mn), where=w)
            st.decide(idx, y - mx, ysum + abs(mx), where=w)
            inside = (mn < y) & (y < mx) if cone else (mn <= y) & (y <= mx)  # the cone's < against the cylinder's <=
            st.offer(idx, t, tsum, leaf, o, d, w & inside)
        if closed:
            st.decide(idx, np.abs(dy) - EPS, np.abs(dy) + EPS, where=go_on)  # feq(d_y, 0) skips the caps
            skip = np.abs(dy) < EPS
            st.branch["caps_skipped"][idx[go_on & skip]] = True
            w = go_on & ~skip
            for lim in (mn, mx):
                with np.errstate(all="ignore"):
                    t = (lim - oy) / dy
                    tsum = (abs(lim) + np.abs(oy)) / np.abs(dy)
                with np.errstate(invalid="ignore"):
                    x, z = ox + t * dx, oz + t * dz
                    r = x * x + z * z
                radius = abs(lim) if cone else LD(1)  # x^2 + z^2 <= |y| against <= 1
                st.decide(idx, r - radius, r + radius, where=w)
                with np.errstate(invalid="ignore"):
                    st.offer(idx, t, tsum, leaf, o, d, w & (r <= radius))
    elif typ == TOROID:  # frt_math.hpp:768-789: the real roots of the same quartic, found independently
        coeffs = quartic_coeffs(o, d, LD(p[0]), LD(p[1]))
        scale = np.abs(o).sum(axis=1) / np.sqrt(_dot(d, d))
        # binary64 cull: the ray passes the sphere of radius r1 + r2 about the centre by more than CULL
        o64, d64 = o.astype(np.float64), d.astype(np.float64)
        foot = o64 - d64 * (_dot(o64, d64) / _dot(d64, d64))[:, None]
        near = np.sqrt(_dot(foot, foot)) <= (p[0] + p[1]) * (1 + CULL)
        for j in np.flatnonzero(near):
            roots, clear, clear_im, smallest = quartic_real_roots(coeffs[j])
            one = idx[j:j + 1]
            if smallest < QUARTIC_ZERO:
                st.margin[one] = 0
            st.decide(one, np.array([clear], dtype=LD), LD(1), rel=DISC_REL)
            st.decide(one, np.array([clear_im], dtype=LD), LD(1), rel=LD(3e-4))
            for x in roots:
                st.offer(one, np.array([x], dtype=LD), scale[j:j + 1], leaf, o[j:j + 1], d[j:j + 1], every[:1])
    else:
        raise ValueError("not a leaf type: %d" % typ)


def _triangles(st, prims, leaves, idx, o, d):
    """Triangle leaves sharing one space (frt_math.hpp:687-707): prims (T, >= 9) p1 e1 e2, leaves (T,). A binary64
    pass keeps the (triangle, ray) pairs that are not misses by more than CULL; those are decided in longdouble."""
    o64, d64 = o.astype(np.float64), d.astype(np.float64)
    chunk = max(1, (1 << 21) // max(1, len(idx)))
    for s in range(0, len(leaves), chunk):
        P = prims[s:s + chunk]
        p1, e1, e2 = P[:, None, 0:3], P[:, None, 3:6], P[:, None, 6:9]
        dce2 = _cross(d64[None], e2)
        det = _dot(e1, dce2)
        with np.errstate(all="ignore"):
            f = 1.0 / det
            p1o = o64[None] - p1
            u = f * _dot(p1o, dce2)
            v = f * _dot(d64[None], _cross(p1o, e1))
            keep = (np.abs(det) < 1e-4) | ((u > -CULL) & (u < 1 + CULL) & (v > -CULL) & (u + v < 1 + CULL))
        ti, ri = np.nonzero(keep)
        if len(ti) == 0:
            continue
        _triangle_pairs(st, P[ti].astype(LD), leaves[s:s + chunk][ti], idx[ri], o[ri], d[ri])


def _triangle_pairs(st, P, leaf, idx, o, d):
    # (a ray may occur more than once in idx: one pair at a time per ray)
    order = np.argsort(idx, kind="stable")
    P, leaf, idx, o, d = P[order], leaf[order], idx[order], o[order], d[order]
    rank = np.arange(len(idx)) - np.searchsorted(idx, idx, side="left")
    for k in range(int(rank.max()) + 1):
        m = rank == k
        _triangle_unique(st, P[m], leaf[m], idx[m], o[m], d[m])


def _triangle_unique(st, P, leaf, idx, o, d):
    p1, e1, e2 = P[:, 0:3], P[:, 3:6], P[:, 6:9]
    dce2 = _cross(d, e2)
    det = _dot(e1, dce2)
    detsum = np.abs(e1 * dce2).sum(axis=1)
    st.decide(idx, np.abs(det) - EPS, detsum + EPS)
    ok = ~(np.abs(det) < EPS)
    with np.errstate(all="ignore"):
        f = 1 / det
        p1o = o - p1
        u = f * _dot(p1o, dce2)
        usum = np.abs(f) * np.abs(p1o * dce2).sum(axis=1)
        st.decide(idx, u, usum, where=ok)
        st.decide(idx, u - 1, usum + 1, where=ok)
        ok = ok & ~((u < 0) | (u > 1))
        oce1 = _cross(p1o, e1)
        v = f * _dot(d, oce1)
        vsum = np.abs(f) * np.abs(d * oce1).sum(axis=1)
        st.decide(idx, v, vsum, where=ok)
        st.decide(idx, 1 - u - v, 1 + usum + vsum, where=ok)
        ok = ok & ~((v < 0) | (u + v > 1))
        t = f * _dot(e2, oce1)
        tsum = np.abs(f) * np.abs(e2 * oce1).sum(axis=1)
    st.offer(idx, t, tsum, leaf, o, d, ok, uv=np.stack([u, v], axis=1))


def _box_keeps(box, o, d):
    """binary64, conservative: the rays that come within CULL (relative) of a group's box."""
    lo = box[:3] - CULL * (1 + np.abs(box[:3]))
    hi = box[3:] + CULL * (1 + np.abs(box[3:]))
    o, d = o.astype(np.float64), d.astype(np.float64)
    with np.errstate(all="ignore"):
        tiny = np.abs(d) < 1e-12
        t0, t1 = (lo - o) / d, (hi - o) / d
        a = np.where(tiny, np.where((o >= lo) & (o <= hi), -np.inf, np.inf), np.minimum(t0, t1))
        b = np.where(tiny, np.where((o >= lo) & (o <= hi), np.inf, -np.inf), np.maximum(t0, t1))
        a, b = np.where(np.isnan(a), -np.inf, a), np.where(np.isnan(b), np.inf, b)
        tmin, tmax = a.max(axis=1), b.min(axis=1)
        return tmin <= tmax + CULL * (1 + np.abs(tmin) + np.abs(tmax))


def _visit(st, tree, node, idx, o, d):
    nodes = tree["nodes"]
    nd = nodes[node]
    if nd["type"] == CSG:
        raise ValueError("first_hit_ref: CSG is out of scope (node %d)" % node)
    if nd["xform"] >= 0:  # shape_intersect: the ray through the node's inverse (frt_traverse.hpp, xf_ray)
        m = tree["xforms_ld"][nd["xform"]]
        o, d = o @ m[:3, :3].T + m[:3, 3], d @ m[:3, :3].T
    if nd["type"] in (TRIANGLE, SMOOTH_TRIANGLE):
        _triangles(st, tree["prim"][None, nd["prim"]:nd["prim"] + 9], np.array([node]), idx, o, d)
        return
    if nd["type"] != GROUP:
        _leaf(st, int(nd["type"]), tree["prim"][nd["prim"]:nd["prim"] + 3], node, idx, o, d)
        return
    keep = _box_keeps(nd["bbox"], o, d)
    if not keep.any():
        return
    idx, o, d = idx[keep], o[keep], d[keep]
    child, tris = node + 1, []
    while child < nd["skip"]:
        c = nodes[child]
        if c["type"] in (TRIANGLE, SMOOTH_TRIANGLE) and c["xform"] < 0:
            tris.append(child)
        else:
            _visit(st, tree, child, idx, o, d)
        child = int(c["skip"])
    if tris:
        tris = np.array(tris)
        prims = tree["prim"][nodes["prim"][tris][:, None] + np.arange(9)[None]]
        _triangles(st, prims, tris, idx, o, d)


def _local_normal(st, tree, leaf, idx, lp, uv):
    """local_normal (csrc/frt_shade.hpp:102-171) at the points lp of one leaf."""
    nd = tree["nodes"][leaf]
    typ, p = int(nd["type"]), tree["prim"][nd["prim"]:nd["prim"] + 18].astype(LD)
    n = np.zeros_like(lp)
    x, y, z = lp[:, 0], lp[:, 1], lp[:, 2]
    if typ == SPHERE:
        n = lp.copy()
    elif typ == PLANE:
        n[:, 1] = 1
    elif typ == CUBE:  # frt_shade.hpp:114-121: feq(max, |x|), then feq(max, |y|), else z
        ax, ay, az = np.abs(x), np.abs(y), np.abs(z)
        mx = np.maximum(np.maximum(ax, ay), az)
        st.decide(idx, (mx - ax) - EPS, mx + ax + EPS)
        isx = (mx - ax) < EPS
        st.decide(idx, (mx - ay) - EPS, mx + ay + EPS, where=~isx)
        isy = ~isx & ((mx - ay) < EPS)
        n[:, 0], n[:, 1], n[:, 2] = np.where(isx, x, 0), np.where(isy, y, 0), np.where(~isx & ~isy, z, 0)
    elif typ in (CYLINDER, CONE):  # frt_shade.hpp:122-141: dist < 1 and the +- EPSILON cap rule
        mn, mx = p[0], p[1]
        dist = x * x + z * z
        top, bottom = (mx - EPS) <= y, (mn + EPS) >= y
        st.decide(idx, dist - 1, dist + 1, where=top | bottom)
        within = dist < 1
        st.decide(idx, y - (mx - EPS), np.abs(y) + abs(mx) + EPS, where=within)
        st.decide(idx, y - (mn + EPS), np.abs(y) + abs(mn) + EPS, where=within & ~top)
        up, down = within & top, within & ~top & bottom
        wall = ~up & ~down
        n[:, 0], n[:, 2] = np.where(wall, x, 0), np.where(wall, z, 0)
        if typ == CONE:
            st.decide(idx, y, np.abs(y), where=wall)
            ny = np.where(y > 0, -np.sqrt(dist), np.sqrt(dist))
        else:
            ny = np.zeros_like(y)
        n[:, 1] = np.where(up, 1, np.where(down, -1, ny))
    elif typ == TOROID:  # frt_shade.hpp:142-151
        r1, r2 = p[0], p[1]
        psq, mag = r1 * r1 + r2 * r2, _dot(lp, lp)
        n = np.stack([4 * x * (mag - psq), 4 * y * (mag - psq + 2 * r1 * r1), 4 * z * (mag - psq)], axis=1)
    elif typ == TRIANGLE:
        n[:] = p[9:12]
    elif typ == SMOOTH_TRIANGLE:  # frt_shade.hpp:159-166: n1 w + n2 u + n3 v
        u, v = uv[:, 0:1], uv[:, 1:2]
        n = p[9:12] * (1 - u - v) + p[12:15] * u + p[15:18] * v
    return n


def first_hits(view):
    """Per camera sample of the view, in (row, col, sub) order: {"t" (rows, w, spp) longdouble (-1: a miss),
    "normal" (.., 3) longdouble, "local" (.., 3) the hit point in the leaf's space, "leaf" int32 (-1), "type" int32
    (-1), "hit", "inside", "margin", "undecided",
    "bump" (the hit leaf's material has a bump map), "branch": {name: the sample took that branch at some leaf}}."""
    tree = flat_tree(view)
    tree["xforms_ld"] = tree["xforms"].astype(LD)
    nodes = tree["nodes"]
    if (nodes["type"] == CSG).any():
        raise ValueError("first_hit_ref: CSG is out of scope")
    o64, d64 = feature_ref.camera_rays(view)
    shape = d64.shape[:3]
    o, d = o64.reshape(-1, 3).astype(LD), d64.reshape(-1, 3).astype(LD)
    n = len(o)
    st = _State(n)
    for root in tree["roots"]:
        _visit(st, tree, int(root), np.arange(n), o, d)
    hit = st.leaf >= 0
    # the two smallest positive t of different leaves against each other
    with np.errstate(invalid="ignore"):
        st.decide(np.arange(n), st.t - st.t_other, np.abs(st.t) + np.abs(st.t_other), where=hit)
    normal, local = np.zeros((n, 3), dtype=LD), np.zeros((n, 3), dtype=LD)
    for leaf in np.unique(st.leaf[hit]):
        idx = np.flatnonzero(st.leaf == leaf)
        lp = st.lo[idx] + st.t[idx, None] * st.ld[idx]
        local[idx] = lp
        nl = _local_normal(st, tree, int(leaf), idx, lp, st.uv[idx])
        x = int(leaf)
        while x >= 0:  # normal_to_world: the transposed inverses, leaf first (frt_shade.hpp:95-99)
            if nodes["xform"][x] >= 0:
                nl = _unit(nl @ tree["xforms_ld"][nodes["xform"][x]][:3, :3])
            x = int(nodes["tparent"][x])
        normal[idx] = _unit(nl)
    eye = -d
    facing = _dot(normal, eye)
    st.decide(np.arange(n), facing, np.abs(normal * eye).sum(axis=1), where=hit)
    inside = hit & (facing < 0)
    normal = np.where(inside[:, None], -normal, normal)
    st.branch["inside"] = inside
    leaf = np.where(hit, st.leaf, -1).astype(np.int32)
    typ = np.where(hit, nodes["type"][np.maximum(leaf, 0)], -1).astype(np.int32)
    bump = hit & tree["bump"][np.maximum(nodes["material"][np.maximum(leaf, 0)], 0)]
    out = {"t": np.where(hit, st.t, LD(-1)), "normal": normal, "leaf": leaf, "type": typ, "hit": hit,
           "inside": inside, "margin": st.margin, "undecided": st.margin < REL, "bump": bump, "local": local}
    out = {k: v.reshape(shape + v.shape[1:]) for k, v in out.items()}
    out["branch"] = {k: v.reshape(shape) for k, v in st.branch.items()}
    return out
