"""CPU restatement of the rasterisation contract at the head of spec_amd/csrc/render.hip (NumPy; no GPU, no product code).

The integer parts - snapping, edge functions, the top-left rule, culling, the 64-bit depth key - are exact.  The fp32 parts are
written with ``np.float32`` operands in the kernel's order of operations (the kernel is compiled without contraction and HIP's
fp32 division and square root are correctly rounded), and ``vertex_stage`` and ``resolve`` also run in float64, which is what the
GPU tests measure their bounds against.  Test meshes (octahedron, icosphere) and the shading scene live here as well."""
import numpy as np

ZNEAR, ZFAR, LIMIT, DROPPED = 0.05, 100.0, 2.0 ** 20, -2 ** 31
NORMAL_SCALE, NORMAL_CLAMP = 2.0 ** 28, 2.0 ** 30
TILE, GREY_EVEN, GREY_ODD = 0.5, 140, 191
EMPTY = np.uint64(0xFFFFFFFFFFFFFFFF)


# ---- vertex stage ---------------------------------------------------------------------------------------------------------
def vertex_stage(vertices, cam_t, R, fx, fy, cx, cy, side=False, dtype=np.float32):
    """(M,V,3), (M,3), (3,3) -> x_s, y_s, Z (M,V) in ``dtype`` and the keep mask, in the kernel's order of operations."""
    f = dtype
    v, t, R = np.asarray(vertices, f), np.asarray(cam_t, f)[:, None, :], np.asarray(R, f)
    fx, fy, cx, cy = f(fx), f(fy), f(cx), f(cy)
    px, py, pz = v[..., 0], -v[..., 1], -v[..., 2]
    if side:
        px, pz = -pz, px
    q = [(R[0, k] * px + R[1, k] * py) + R[2, k] * pz for k in range(3)]
    X, Y, Z = q[0] + t[..., 0], t[..., 1] - q[1], t[..., 2] - q[2]
    with np.errstate(all='ignore'):
        xs, ys = (fx * X) / Z + cx, (fy * Y) / Z + cy
        keep = (Z > f(ZNEAR)) & (np.abs(xs) < f(LIMIT)) & (np.abs(ys) < f(LIMIT))
    return xs, ys, Z, keep


def snap(xs, ys, keep):
    """1/256 pixel, round half to even; a dropped vertex is DROPPED in both."""
    with np.errstate(all='ignore'):
        sx = np.where(keep, np.rint(np.where(keep, xs, 0) * xs.dtype.type(256)), DROPPED).astype(np.int64)
        sy = np.where(keep, np.rint(np.where(keep, ys, 0) * ys.dtype.type(256)), DROPPED).astype(np.int64)
    return sx, sy


def lowest_y(vertices, cam_t, R, side=True):
    """The ground plane's height in camera-centred world coordinates (fp32, the kernel's order)."""
    f = np.float32
    v, t, R = np.asarray(vertices, f), np.asarray(cam_t, f), np.asarray(R, f)
    oy = (R[1, 0] * -t[:, 0] + R[1, 1] * t[:, 1]) + R[1, 2] * t[:, 2]
    return (-v[..., 1] - oy[:, None]).min()


# ---- coverage and visibility ----------------------------------------------------------------------------------------------
def _orient(ax, ay, bx, by, cx, cy):
    return (bx - ax) * (cy - ay) - (by - ay) * (cx - ax)


def triangle_cover(x, y, H, W, cull=True):
    """One triangle with snapped int vertices x[3], y[3] -> (rows, cols, E (3, n) int64, A) of the covered pixels of an H x W
    frame, or None when it is not drawn."""
    x, y = [int(v) for v in x], [int(v) for v in y]
    if DROPPED in x:
        return None
    A = _orient(x[0], y[0], x[1], y[1], x[2], y[2])
    if A == 0 or (A > 0 and cull):
        return None
    sgn = -1 if A < 0 else 1
    j0, j1 = max(-((128 - min(x)) // 256), 0), min((max(x) - 128) // 256, W - 1)
    i0, i1 = max(-((128 - min(y)) // 256), 0), min((max(y) - 128) // 256, H - 1)
    if j0 > j1 or i0 > i1:
        return None
    ii, jj = np.meshgrid(np.arange(i0, i1 + 1, dtype=np.int64), np.arange(j0, j1 + 1, dtype=np.int64), indexing='ij')
    X, Y = 256 * jj + 128, 256 * ii + 128
    inside = np.ones(X.shape, bool)
    E = []
    for k in range(3):
        b, c = (k + 1) % 3, (k + 2) % 3
        e = sgn * _orient(x[b], y[b], x[c], y[c], X, Y)
        gx, gy = -sgn * (y[c] - y[b]), sgn * (x[c] - x[b])
        inside &= (e > 0) | ((e == 0) & bool(gx > 0 or (gx == 0 and gy > 0)))
        E.append(e)
    return ii[inside], jj[inside], np.stack([e[inside] for e in E]), A * sgn


def depth_weights(E, A, z):
    """fp32: w_i = E_i / A, 1/z = (w0/z0 + w1/z1) + w2/z2 -> (w (3, n), z (n))."""
    f = np.float32
    w = E.astype(f) / f(A)
    z = np.asarray(z, f)
    s = (w[0] / z[0] + w[1] / z[1]) + w[2] / z[2]
    return w, f(1) / s


def rasterize(sx, sy, z, faces, H, W, cull=True):
    """Snapped (M,V) int coordinates and fp32 depths -> (id_map (H,W) int32 with -1, depth (H,W) fp32 with 0, keys uint64)."""
    sx, sy, z, faces = np.asarray(sx, np.int64), np.asarray(sy, np.int64), np.asarray(z, np.float32), np.asarray(faces, np.int64)
    M, V = sx.shape
    F = faces.shape[0]
    keys = np.full((H, W), EMPTY, np.uint64)
    ok = ((faces >= 0) & (faces < V)).all(axis=1)
    for m in range(M):
        fx_, fy_ = sx[m][np.clip(faces, 0, V - 1)], sy[m][np.clip(faces, 0, V - 1)]              # (F, 3)
        A = _orient(fx_[:, 0], fy_[:, 0], fx_[:, 1], fy_[:, 1], fx_[:, 2], fy_[:, 2])
        draw = ok & (fx_ != DROPPED).all(axis=1) & (A != 0) & ((A < 0) | (not cull))
        draw &= (fx_.max(1) >= 128) & (fx_.min(1) <= 256 * W) & (fy_.max(1) >= 128) & (fy_.min(1) <= 256 * H)
        for f in np.nonzero(draw)[0]:
            c = triangle_cover(fx_[f], fy_[f], H, W, cull)
            if c is None or c[0].size == 0:
                continue
            ii, jj, E, Apos = c
            _, zz = depth_weights(E, Apos, z[m][faces[f]])
            k = (zz.view(np.uint32).astype(np.uint64) << np.uint64(32)) | np.uint64(m * F + f)
            keys[ii, jj] = np.minimum(keys[ii, jj], k)
    hit = keys != EMPTY
    id_map = np.where(hit, (keys & np.uint64(0xFFFFFFFF)).astype(np.int64), -1).astype(np.int32)
    depth = np.where(hit, (keys >> np.uint64(32)).astype(np.uint32).view(np.float32), np.float32(0)).astype(np.float32)
    return id_map, depth, keys


# ---- normals and shading --------------------------------------------------------------------------------------------------
def normal_sums(vertices, faces):
    """(M,V,3) fp32, (F,3) -> (M,V,3) int64 holding the kernel's int32 sums of the quantised face normals.  Every face whose
    three indices lie in [0, V) contributes, drawn or not; any other face contributes nothing.  The quantisation is the kernel's
    ``(int)fminf(fmaxf(rintf(n * 2^28), -2^30), 2^30)``: fmaxf returns its other operand for a NaN, so a NaN component becomes
    -2^30 (+-Inf clamp to +-2^30).  The sums wrap as int32."""
    f = np.float32
    v, faces = np.asarray(vertices, f), np.asarray(faces, np.int64)
    faces = faces[((faces >= 0) & (faces < v.shape[1])).all(axis=1)]
    out = np.zeros(v.shape, np.int64)
    for m in range(v.shape[0]):
        with np.errstate(all='ignore'):
            a, b = v[m][faces[:, 1]] - v[m][faces[:, 0]], v[m][faces[:, 2]] - v[m][faces[:, 0]]
            n = np.stack([a[:, 1] * b[:, 2] - a[:, 2] * b[:, 1], a[:, 2] * b[:, 0] - a[:, 0] * b[:, 2], a[:, 0] * b[:, 1] - a[:, 1] * b[:, 0]], 1)
            s = np.rint(n * f(NORMAL_SCALE))
        q = np.where(np.isnan(s), -NORMAL_CLAMP, np.clip(np.where(np.isnan(s), 0, s), -NORMAL_CLAMP, NORMAL_CLAMP)).astype(np.int64)
        for k in range(3):
            np.add.at(out[m], faces[:, k], q)
    return (out + 2 ** 31) % 2 ** 32 - 2 ** 31


RESOLVE_VARIANTS = (None, 'weights_rotated', 'no_perspective', 'axes_exchanged')


def resolve(sx, sy, z, vertices, faces, id_map, rgb, side=False, dtype=np.float32, variant=None):
    """The resolve stage at the covered pixels of ``id_map`` (H, W; id = m F + f, negative: not a mesh pixel), from the snapped
    (M,V) coordinates and fp32 depths the raster stage saw -> (value (H,W,3) in ``dtype`` = 255 rgb shade before rounding, NaN
    where uncovered; byte (H,W,3) uint8, 0 where uncovered).  The kernel's order of operations:
      w_k = (float)E_k / (float)A,  zz = 1 / ((w0 / z0 + w1 / z1) + w2 / z2),
      len_k = sqrt((x x + y y) + u u) of vertex k's int32 normal sum q_k = (x, y, u) converted to float,
      b_k = ((w_k / z_k) zz) / len_k  (0 where len_k == 0),  n = ((0 + b_0 q_0) + b_1 q_1) + b_2 q_2,
      n.l = (side ? n.x : -n.z) / sqrt((n.x n.x + n.y n.y) + n.z n.z)  (0 for a zero n),
      value = (255 rgb) min(1, 0.3 + 0.7 max(0, n.l)),  byte = rint(value).
    ``dtype`` np.float32 restates the kernel bit for bit; np.float64 is the same chain from the same inputs (the fp32 depths and
    rgb, the integer edge functions and normal sums) with every constant, conversion and operation in float64.
    ``variant`` reruns the chain with one deliberate mistake (the host tests show that the scenes tell them apart):
    'weights_rotated' pairs w_{k+1} with vertex k, 'no_perspective' takes b_k = w_k / len_k, 'axes_exchanged' reads n.x in the
    overlay and -n.z in side view."""
    assert variant in RESOLVE_VARIANTS
    f = dtype
    sx, sy, faces = np.asarray(sx, np.int64), np.asarray(sy, np.int64), np.asarray(faces, np.int64)
    z, id_map = np.asarray(z, np.float32), np.asarray(id_map, np.int64)
    F = faces.shape[0]
    sums = normal_sums(vertices, faces)
    ii, jj = np.nonzero(id_map >= 0)
    m, idx = id_map[ii, jj] // F, faces[id_map[ii, jj] % F]                     # (n), (n, 3)
    x, y, zv = sx[m[:, None], idx], sy[m[:, None], idx], z[m[:, None], idx].astype(f)
    q = sums[m[:, None], idx].astype(f)                                          # (n, 3 vertices, 3 components)
    X, Y = 256 * jj + 128, 256 * ii + 128
    A = _orient(x[:, 0], y[:, 0], x[:, 1], y[:, 1], x[:, 2], y[:, 2])
    sgn = np.where(A < 0, -1, 1)
    E = [sgn * _orient(x[:, (k + 1) % 3], y[:, (k + 1) % 3], x[:, (k + 2) % 3], y[:, (k + 2) % 3], X, Y) for k in range(3)]
    w = [E[k].astype(f) / (A * sgn).astype(f) for k in range(3)]
    zz = f(1) / ((w[0] / zv[:, 0] + w[1] / zv[:, 1]) + w[2] / zv[:, 2])
    n = [np.zeros(ii.shape, f) for _ in range(3)]
    with np.errstate(all='ignore'):
        for k in range(3):
            wk = w[(k + 1) % 3] if variant == 'weights_rotated' else w[k]
            length = np.sqrt((q[:, k, 0] * q[:, k, 0] + q[:, k, 1] * q[:, k, 1]) + q[:, k, 2] * q[:, k, 2])
            b = wk / length if variant == 'no_perspective' else ((wk / zv[:, k]) * zz) / length
            b = np.where(length > 0, b, f(0))
            for c in range(3):
                n[c] = n[c] + b * q[:, k, c]
        length = np.sqrt((n[0] * n[0] + n[1] * n[1]) + n[2] * n[2])
        along = n[0] if bool(side) != (variant == 'axes_exchanged') else -n[2]
        ndl = np.where(length > 0, along / length, f(0))
    shade_ = np.minimum(f(1), f(0.3) + f(0.7) * np.maximum(f(0), ndl))
    value = np.full(id_map.shape + (3,), np.nan, f)
    value[ii, jj] = (f(255) * np.asarray(rgb, np.float32).astype(f))[None, :] * shade_[:, None]
    byte = np.zeros(id_map.shape + (3,), np.uint8)
    byte[ii, jj] = np.rint(value[ii, jj]).astype(np.uint8)
    return value, byte


def half_integer_margin(v32, v64):
    """The fp32 and float64 ``resolve`` values of one picture -> (gap = max |fp32 - float64| in bytes, delta = 4 gap - the
    factor for the GPU's own rounding of the same operations, as Z_BOUND in tests/test_gpu_render.py -, the (H,W,3) mask of
    covered pixel-channels whose float64 value lies within delta of a half-integer, the covered mask): where the first mask is
    False the rounded byte cannot depend on fp32 rounding."""
    covered = ~np.isnan(v64)
    gap = float(np.abs(v32.astype(np.float64) - v64)[covered].max())
    with np.errstate(invalid='ignore'):
        near = covered & (np.abs(v64 - np.floor(v64) - 0.5) <= 4.0 * gap)
    return gap, 4.0 * gap, near, covered


def shade(ndl):
    """min(1, 0.3 + 0.7 max(0, n.l)), fp32"""
    f = np.float32
    return np.minimum(f(1), f(0.3) + f(0.7) * np.maximum(f(0), np.asarray(ndl, f)))


def shaded_byte(rgb, ndl):
    f = np.float32
    return np.rint((f(255) * np.asarray(rgb, f)) * shade(ndl)).astype(np.uint8)


def checker(i, j, R, cam_t0, fx, fy, cx, cy, y_plane):
    """The ground plane at pixel rows i, columns j (arrays): (depth s fp32, grey byte); a pixel shows the plane where
    ZNEAR < s < ZFAR and s is nearer than the mesh."""
    f = np.float32
    R, t = np.asarray(R, f), np.asarray(cam_t0, f)
    fx, fy, cx, cy = f(fx), f(fy), f(cx), f(cy)
    gx, gy, gz = (np.asarray(j, f) + f(0.5) - cx) / fx, -((np.asarray(i, f) + f(0.5) - cy) / fy), f(-1)
    d = [(R[k, 0] * gx + R[k, 1] * gy) + R[k, 2] * gz for k in range(3)]
    o = [(R[k, 0] * -t[0] + R[k, 1] * t[1]) + R[k, 2] * t[2] for k in range(3)]
    with np.errstate(all='ignore'):
        s = f(y_plane) / d[1]
        hx, hz = o[0] + s * d[0], o[2] + s * d[2]
        ok = (s > f(ZNEAR)) & (s < f(ZFAR))
        par = (np.floor(np.where(ok, hx, 0) / f(TILE)).astype(np.int64) + np.floor(np.where(ok, hz, 0) / f(TILE)).astype(np.int64)) & 1
    return s, np.where(par == 1, GREY_ODD, GREY_EVEN).astype(np.uint8), ok


# ---- test meshes ----------------------------------------------------------------------------------------------------------
def rot(pitch, roll):
    """Rx(pitch) Rz(roll), fp32"""
    cp, sp, cr, sr = np.cos(pitch), np.sin(pitch), np.cos(roll), np.sin(roll)
    return (np.array([[1, 0, 0], [0, cp, -sp], [0, sp, cp]]) @ np.array([[cr, -sr, 0], [sr, cr, 0], [0, 0, 1]])).astype(np.float32)


def shading_scene(meshes=1):
    """The scene the smooth shading is pinned on: a spun icosahedron (12 vertices, 20 faces) that fills about 260 pixels of a
    33 x 47 frame with 7 faces, so the interpolated normal varies strongly inside every face.  ``meshes`` = 2 adds a second,
    differently spun and smaller one beside and partly in front of it (the per-mesh offset of the normal sums)."""
    v, f = icosphere(0, 1.0)
    spin = [rot(0.4, 0.7).astype(np.float64), 0.6 * rot(-0.9, 0.3).astype(np.float64)][:meshes]
    t = [[0.1, -0.05, 3.0], [-0.55, 0.3, 2.2]][:meshes]
    return dict(v=np.ascontiguousarray(np.stack([v.astype(np.float64) @ s.T for s in spin]), np.float32), f=f, t=np.asarray(t, np.float32),
                R=rot(0.1, -0.05), cam=(30., 30., 23.5, 16.5), size=(33, 47), rgb=(0.8, 0.5, 0.6))


def octahedron(radius=1.0):
    """6 vertices, 8 outward-wound faces"""
    v = np.array([[1, 0, 0], [-1, 0, 0], [0, 1, 0], [0, -1, 0], [0, 0, 1], [0, 0, -1]], np.float64) * radius
    f = np.array([[0, 2, 4], [2, 1, 4], [1, 3, 4], [3, 0, 4], [2, 0, 5], [1, 2, 5], [3, 1, 5], [0, 3, 5]], np.int32)
    return v.astype(np.float32), f


def icosphere(subdivisions=2, radius=1.0):
    """An icosahedron subdivided ``subdivisions`` times (2: 162 vertices, 320 faces), outward-wound."""
    p = (1 + 5 ** 0.5) / 2
    v = [(-1, p, 0), (1, p, 0), (-1, -p, 0), (1, -p, 0), (0, -1, p), (0, 1, p), (0, -1, -p), (0, 1, -p), (p, 0, -1), (p, 0, 1), (-p, 0, -1), (-p, 0, 1)]
    v = [np.array(a, np.float64) / np.linalg.norm(a) for a in v]
    f = [(0, 11, 5), (0, 5, 1), (0, 1, 7), (0, 7, 10), (0, 10, 11), (1, 5, 9), (5, 11, 4), (11, 10, 2), (10, 7, 6), (7, 1, 8),
         (3, 9, 4), (3, 4, 2), (3, 2, 6), (3, 6, 8), (3, 8, 9), (4, 9, 5), (2, 4, 11), (6, 2, 10), (8, 6, 7), (9, 8, 1)]
    for _ in range(subdivisions):
        mid, nf = {}, []

        def midpoint(a, b):
            key = (min(a, b), max(a, b))
            if key not in mid:
                m = v[a] + v[b]
                v.append(m / np.linalg.norm(m))
                mid[key] = len(v) - 1
            return mid[key]
        for a, b, c in f:
            ab, bc, ca = midpoint(a, b), midpoint(b, c), midpoint(c, a)
            nf += [(a, ab, ca), (b, bc, ab), (c, ca, bc), (ab, bc, ca)]
        f = nf
    v, f = np.array(v) * radius, np.array(f, np.int32)
    n = np.cross(v[f[:, 1]] - v[f[:, 0]], v[f[:, 2]] - v[f[:, 0]])
    assert (np.einsum('ij,ij->i', n, v[f].mean(1)) > 0).all()          # outward-wound
    return v.astype(np.float32), f
