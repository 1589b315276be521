"""The rasteriser of spec_amd/csrc/render.hip on MI355X at the places its contract names and plain scenes never reach: pixel
centres ON edges and vertices (the top-left rule), equal depth keys (the tie goes to the lower id), the drop limits (Z == 0.05f,
|x_s| == 2^20, NaN / Inf, foreign face indices, A == 0, edge functions near 2^60), the smooth shading against a restatement of the
resolve stage (tests/render_ref.py ``resolve``) in fp32 and float64, and ``specmi_render_views`` on views so small that one
wavefront serves many of them.  tests/test_render_host.py states, without a GPU, the conditions the shading bounds rely on.

The exact camera: R = I, cam_t = (0, 0, 4), fx = fy = 4, cx = cy = 0.  A model vertex (x Z / 4, y Z / 4, Z - 4) with Z a power of
two then lands at x_s = x, y_s = y and depth Z with no rounding anywhere in the vertex stage, so a coordinate that is a multiple
of 1/256 snaps to the integer intended.  Every test first asserts the device's ``screen_xy`` / ``screen_z`` against those
integers: a broken premise fails the test instead of silently no longer testing the tie.

Every scene is drawn in both launch shapes (a wavefront per triangle, RENDER_THREAD_PER_TRIANGLE) and the two are compared byte
for byte; ids and depth bits are compared with ``render_ref.rasterize`` fed the device's own snapped coordinates, the bytes of
the covered pixels with ``render_ref.resolve`` in fp32 (the kernel's order of operations, bit for bit)."""
import numpy as np
import pytest
import torch

from tests import render_ref as RR
from tests.util import t

pytestmark = pytest.mark.gpu
torch.set_grad_enabled(False)
DEV = 'cuda:0'
RGB = (0.8, 0.5, 0.6)
KEYS = ('image', 'id_map', 'depth', 'screen_xy', 'screen_z')
INT32_MIN = -2 ** 31


def _flags():
    from spec_amd import _lib
    return _lib.RENDER_CULL, _lib.RENDER_SIDE_VIEW, _lib.RENDER_GROUND_PLANE, _lib.RENDER_THREAD_PER_TRIANGLE


def _exact(points, faces, size):
    """``points`` (V, 3) or (M, V, 3) rows (x_s, y_s, Z) - screen position in pixels and depth - under the exact camera."""
    p = np.asarray(points, np.float64)
    p = p[None] if p.ndim == 2 else p
    v = np.stack([p[..., 0] * p[..., 2] / 4, p[..., 1] * p[..., 2] / 4, p[..., 2] - 4], -1)
    assert (v.astype(np.float32) == v).all() and (np.rint(p[..., :2] * 256) == p[..., :2] * 256).all()
    return dict(v=np.ascontiguousarray(v, np.float32), f=np.ascontiguousarray(faces, np.int32).reshape(-1, 3), t=np.tile(np.float32([[0, 0, 4]]), (p.shape[0], 1)),
                R=np.eye(3, dtype=np.float32), cam=(4., 4., 0., 0.), size=size, rgb=RGB, points=p)


def _render(d, flags):
    from spec_amd import cam_utils
    eng = cam_utils._engine(torch.device(DEV))
    H, W = d['size']
    frame = np.random.default_rng(H * W).integers(0, 256, (H, W, 3), dtype=np.uint8)
    out = eng.render_meshes(t(d['v']).to(DEV), t(d['f']).to(DEV), t(d['t']).to(DEV), t(d['R']).to(DEV), d['cam'][:2], d['cam'][2:],
                            frame=t(frame).to(DEV), rgb=d['rgb'], flags=flags, maps=True)
    return {k: v.cpu().numpy() for k, v in out.items()}, frame


def _both(d, flags):
    """The scene in both launch shapes, equal byte for byte -> (maps of the wavefront-per-triangle launch, the frame)."""
    g, frame = _render(d, flags)
    thread, _ = _render(d, flags | _flags()[3])
    for k in KEYS:
        assert thread[k].tobytes() == g[k].tobytes(), k
    return g, frame


def _assert_screen(g, d, dropped=None):
    """The premise: the device snapped every vertex to the integer intended (``dropped``: the (M, V) mask of those it must drop)."""
    want = np.rint(d['points'][..., :2] * 256).astype(np.int64)
    if dropped is not None:
        want[dropped] = RR.DROPPED
    assert np.array_equal(g['screen_xy'].astype(np.int64), want)
    assert g['screen_z'].tobytes() == d['points'][..., 2].astype(np.float32).tobytes()


def _assert_maps(g, frame, d, flags):
    """ids and depth bits equal ``rasterize``'s, covered bytes ``resolve``'s in fp32, uncovered bytes the frame's -> ids."""
    cull, side = bool(flags & _flags()[0]), bool(flags & _flags()[1])
    sx, sy = g['screen_xy'][..., 0], g['screen_xy'][..., 1]
    ids, depth, _ = RR.rasterize(sx, sy, g['screen_z'], d['f'], *d['size'], cull=cull)
    assert np.array_equal(g['id_map'], ids)
    assert g['depth'].tobytes() == depth.tobytes()
    _, byte = RR.resolve(sx, sy, g['screen_z'], d['v'], d['f'], ids, d['rgb'], side, np.float32)
    assert np.array_equal(g['image'][ids >= 0], byte[ids >= 0])
    assert np.array_equal(g['image'][ids < 0], np.zeros_like(frame)[ids < 0] if side else frame[ids < 0])
    return ids


def _orient(a, b, c):
    return (b[0] - a[0]) * (c[1] - a[1]) - (b[1] - a[1]) * (c[0] - a[0])


def _owner(tris, H, W, cull):
    """Independent of render_ref.  The top-left rule says: a pixel belongs to the triangle that strictly contains its centre
    moved right by eps and down by eps^2, for eps small enough.  With vertices on the 1/256 grid, eps = 2^-20 of a unit is small
    enough (an edge function that is not 0 at the centre is at least 1 there and moves by less than 2^13 eps; one that is 0 takes
    the sign of its x gradient, or of its y gradient when that is 0), and everything is exact in Python integers scaled by 2^40.
    ``tris``: triangles as three (x, y) in 1/256 pixel -> (H, W) index of the owner, -1 where none; no pixel has two."""
    K = 1 << 40
    own = np.full((H, W), -1, np.int32)
    for n, tri in enumerate(tris):
        a, b, c = [(int(x) * K, int(y) * K) for x, y in tri]
        A = _orient(a, b, c)
        if A == 0 or (A > 0 and cull):
            continue
        s = 1 if A > 0 else -1
        for i in range(H):
            for j in range(W):
                p = ((256 * j + 128) * K + (1 << 20), (256 * i + 128) * K + 1)
                if all(s * _orient(u, v, p) > 0 for u, v in ((a, b), (b, c), (c, a))):
                    assert own[i, j] == -1, 'the scene overlaps itself'
                    own[i, j] = n
    return own


def _units(points):
    return [(int(round(256 * x)), int(round(256 * y))) for x, y in points]


# ---- edge ties ---------------------------------------------------------------------------------------------------------------
QUADS = {'square': ([(1, 1), (7, 1), (7, 7), (1, 7)], (9, 13)),                                    # its diagonal runs through pixel centres
         'diamond': ([(4.5, 0.5), (8.5, 4.5), (4.5, 8.5), (0.5, 4.5)], (12, 14)),                  # corners and all four edges through centres
         'rectangle': ([(1.5, 1.5), (8.5, 1.5), (8.5, 6.5), (1.5, 6.5)], (9, 13))}                 # corners ON pixel centres


def _shared_edge_owner(p, q, s0, s1):
    """Pixel centres ON the edge p-q shared by the triangles with third vertices s0 and s1 belong to the one for which p-q is a
    left edge (its inside lies at larger x) or, for a horizontal p-q, a top edge (its inside lies at larger y) -> 0 or 1."""
    if p[1] == q[1]:
        return 0 if s0[1] > p[1] else 1
    right_of = lambda s: ((s[0] - p[0]) * (q[1] - p[1]) - (s[1] - p[1]) * (q[0] - p[0])) * (1 if q[1] > p[1] else -1) > 0
    assert right_of(s0) != right_of(s1)
    return 0 if right_of(s0) else 1


@pytest.mark.parametrize('quad', list(QUADS))
def test_quads_on_pixel_centres_follow_the_top_left_rule(quad):
    CULL = _flags()[0]
    pts, (H, W) = QUADS[quad]
    u = _units(pts)
    ii, jj = np.meshgrid(np.arange(H), np.arange(W), indexing='ij')
    centre = (256 * jj + 128, 256 * ii + 128)
    e = np.stack([_orient(u[k], u[(k + 1) % 4], centre) for k in range(4)])
    inside, outside = (e > 0).all(0) | (e < 0).all(0), (e > 0).any(0) & (e < 0).any(0)
    covers = {}
    for order in ((0, 1, 2, 3), (3, 2, 1, 0)):
        drawn_with_cull = _orient(u[order[0]], u[order[1]], u[order[2]]) < 0
        for split, faces in enumerate(([order[:3], (order[0], order[2], order[3])], [(order[0], order[1], order[3]), order[1:]])):
            d = _exact([p + (4,) for p in pts], faces, (H, W))
            for flags in (0, CULL):
                g, frame = _both(d, flags)
                _assert_screen(g, d)
                ids = _assert_maps(g, frame, d, flags)
                if flags and not drawn_with_cull:
                    assert (ids == -1).all()
                    continue
                assert np.array_equal(ids, _owner([[u[k] for k in f] for f in faces], H, W, bool(flags)))
                assert (ids[inside] >= 0).all() and (ids[outside] == -1).all()
                covers[order, split, flags] = ids >= 0
                # the shared diagonal: faces[0] and faces[1] have exactly two vertices in common
                p, q = [k for k in faces[0] if k in faces[1]]
                s0, s1 = [k for k in faces[0] if k not in (p, q)][0], [k for k in faces[1] if k not in (p, q)][0]
                on = (ids >= 0) & (_orient(u[p], u[q], centre) == 0)
                assert (ids[on] == _shared_edge_owner(u[p], u[q], u[s0], u[s1])).all()
                assert quad == 'rectangle' or on.sum() >= 6                   # pixel centres do lie on the shared edge, in every drawn case
    assert len(covers) == 6
    first = next(iter(covers.values()))
    assert all(np.array_equal(c, first) for c in covers.values())             # either split, either winding, cull or not: the same set
    if quad == 'rectangle':
        assert first.sum() == 7 * 5 and first[1:6, 1:8].all()
        assert first[1, 1] and not first[1, 8] and not first[6, 1] and not first[6, 8]      # the top-left corner is in, right and bottom edges out
    if quad == 'square':
        assert first.sum() == 36 and first[1:7, 1:7].all()


def test_fan_around_a_vertex_on_a_pixel_centre():
    """Eight triangles around (4.5, 4.5), the centre of pixel (4, 4); four spokes run through further pixel centres.  The pixel is
    covered once, by the triangle between the spokes towards east and south-east: the one that holds the point just right of
    and (less) below the vertex."""
    CULL = _flags()[0]
    H, W = 9, 13
    rim = [(8, 4.5), (7, 7), (4.5, 8), (2, 7), (1, 4.5), (2, 2), (4.5, 1), (7, 2)]                # east, then clockwise on the screen (y down)
    pts = [(4.5, 4.5)] + rim
    u = _units(pts)
    for shift in (0, 5):          # the wedge named by the rule is face 0, then face 5
        wedges = [(0, 1 + (k - shift) % 8, 1 + (k - shift + 1) % 8) for k in range(8)]
        named = shift
        assert set(wedges[named][1:]) == {1, 2}
        for flags, faces in ((0, wedges), (0, [w[::-1] for w in wedges]), (CULL, [w[::-1] for w in wedges]), (CULL, wedges)):
            d = _exact([p + (4,) for p in pts], faces, (H, W))
            g, frame = _both(d, flags)
            _assert_screen(g, d)
            ids = _assert_maps(g, frame, d, flags)
            if flags and _orient(u[faces[0][0]], u[faces[0][1]], u[faces[0][2]]) > 0:
                assert (ids == -1).all()
                continue
            assert ids[4, 4] == named
            assert np.array_equal(ids, _owner([[u[k] for k in f] for f in faces], H, W, bool(flags)))
            assert (ids >= 0).sum() > 30 and len(np.unique(ids[ids >= 0])) == 8


# ---- depth ties and crossings ------------------------------------------------------------------------------------------------
T_SLANTED = [(1, 1, 2), (12, 2, 8), (3, 11, 4)]
U_BEHIND = [(6, 5, 16), (13, 5, 16), (13, 11, 16)]
# P and Q: one footprint, depths exchanged between two corners, so each is the nearer one on its side of a line; S cuts through both
CROSSING = [(1, 1, 2), (12, 2, 8), (3, 11, 4), (1, 1, 8), (12, 2, 2), (3, 11, 4), (2, 0.5, 4), (12.5, 6, 4), (1, 10, 2)]


@pytest.mark.parametrize('rows', ['UTT', 'TUT', 'TTU'])
def test_a_face_listed_twice_goes_to_the_lower_id(rows):
    H, W = 12, 14
    faces = [{'T': (0, 1, 2), 'U': (3, 4, 5)}[r] for r in rows]
    d = _exact(T_SLANTED + U_BEHIND, faces, (H, W))
    g, frame = _both(d, 0)
    _assert_screen(g, d)
    ids = _assert_maps(g, frame, d, 0)
    own = _owner([_units([p[:2] for p in T_SLANTED])], H, W, False) == 0
    assert own.sum() > 40 and (ids[own] == rows.index('T')).all()             # T is in front of U wherever both are; its first row wins
    assert (ids == rows.index('U')).sum() > 5 and not (ids == rows.rindex('T')).any()


def test_two_identical_meshes_go_to_mesh_0():
    H, W = 12, 14
    faces = [(0, 1, 2), (3, 4, 5), (6, 7, 8)]
    one, two = _exact(CROSSING, faces, (H, W)), _exact([CROSSING, CROSSING], faces, (H, W))
    g1, _ = _both(one, 0)
    g2, frame = _both(two, 0)
    _assert_screen(g2, two)
    ids = _assert_maps(g2, frame, two, 0)
    assert (ids >= 0).sum() > 60 and (ids < len(faces)).all()
    for k in ('image', 'id_map', 'depth'):
        assert g2[k].tobytes() == g1[k].tobytes(), k


def test_interpenetrating_triangles_bit_for_bit():
    H, W = 12, 14
    faces = [(0, 1, 2), (3, 4, 5), (6, 7, 8)]
    d = _exact(CROSSING, faces, (H, W))
    g, frame = _both(d, 0)
    _assert_screen(g, d)
    ids = _assert_maps(g, frame, d, 0)                                       # ids and depth bits: rasterize's
    assert all((ids == f).sum() >= 8 for f in range(3))                      # all three show: they do cross
    # independently, in float64 from the integer edge functions: where two layers differ by more than 1e-5 relative the nearer shows
    u, z = _units([p[:2] for p in CROSSING]), [p[2] for p in CROSSING]
    layers = np.full((3, H, W), np.inf)
    for f, idx in enumerate(faces):
        ii, jj, E, A = RR.triangle_cover([u[k][0] for k in idx], [u[k][1] for k in idx], H, W, cull=False)
        layers[f, ii, jj] = 1.0 / sum(E[k] / A / z[idx[k]] for k in range(3))
    order = np.sort(layers, axis=0)
    with np.errstate(invalid='ignore'):
        clear = np.isfinite(order[0]) & ((order[1] - order[0]) > 1e-5 * order[0])
    assert clear.sum() > 60 and np.array_equal(ids[clear], layers.argmin(0)[clear])
    assert np.abs(g['depth'][clear] - order[0][clear]).max() < 1e-5


# ---- limits ------------------------------------------------------------------------------------------------------------------
def test_near_plane_is_exclusive_and_a_triangle_behind_it_disappears_whole():
    """cam_t.z = float32(0.05) and R = I: a vertex with z = 0 has Z == 0.05f exactly and is dropped, one with z = 2^-28 (one ulp
    of 0.05f) has the next float and is kept; x_s = 4 x / Z is rounded here, so the integers intended are the fp32 restatement's."""
    near = np.float32(RR.ZNEAR)
    up = np.nextafter(near, np.float32(1))
    assert float(up) - float(near) == 2.0 ** -28
    H, W = 9, 13
    screen = {'A': [(1, 1), (11, 1.5), (1.5, 8)], 'B': [(2, 2), (12, 3), (3, 8.5)], 'C': [(4, 0.5), (12.5, 5), (0.5, 7)]}
    vz = {'A': [2.0 ** -28] * 3, 'B': [2.0 ** -28, 0.0, 2.0 ** -28], 'C': [2.0 ** -28, 2.0 ** -28, -1.0]}
    v = [[x * (float(near) + dz) / 4, y * (float(near) + dz) / 4, dz] for k in 'BCA' for (x, y), dz in zip(screen[k], vz[k])]
    d = dict(v=np.ascontiguousarray([v], np.float32), f=np.arange(9, dtype=np.int32).reshape(3, 3), t=np.array([[0, 0, near]], np.float32),
             R=np.eye(3, dtype=np.float32), cam=(4., 4., 0., 0.), size=(H, W), rgb=RGB)
    g, frame = _both(d, 0)
    xs, ys, z, keep = RR.vertex_stage(d['v'], d['t'], d['R'], *d['cam'])
    sx, sy = RR.snap(xs, ys, keep)
    assert keep[0].tolist() == [True, False, True, True, True, False, True, True, True]
    assert z[0, 1] == near and g['screen_z'][0, 1] == near and g['screen_z'][0, 5] == np.float32(near - 1)
    assert (g['screen_z'][0, [0, 2, 3, 4, 6, 7, 8]] == up).all()
    assert np.array_equal(g['screen_xy'][..., 0], sx) and np.array_equal(g['screen_xy'][..., 1], sy)
    assert (np.abs(sx[0, 6:] - 256 * np.array([1, 11, 1.5])) <= 1).all() and (np.abs(sy[0, 6:] - 256 * np.array([1, 1.5, 8])) <= 1).all()
    ids = _assert_maps(g, frame, d, 0)
    assert (ids == 2).sum() > 25 and set(np.unique(ids)) == {-1, 2}          # B (a vertex AT the plane) and C (one behind it) are gone whole


def test_screen_limit_is_exclusive_and_the_largest_triangle_covers_the_frame():
    """|x_s| or |y_s| == 2^20 drops the vertex, 2^20 - 1/16 keeps it.  The kept triangle spans the whole range: |A| = 4 (2^28 - 16)^2
    = 2.88e17 in snapped units, edge functions of up to that, under the 2^60 the contract allows; it covers all of 9 x 13."""
    CULL = _flags()[0]
    H, W = 9, 13
    L, B = 2.0 ** 20 - 1 / 16, 2.0 ** 20
    kept = [(0, L, 4), (L, -L, 4), (-L, -L, 4)]                                # drawn with cull on (A < 0)
    at = [[(0, L, 2), (L, -L, 2), (-B, -L, 2)], [(0, L, 2), (B, -L, 2), (-L, -L, 2)], [(0, L, 2), (L, -B, 2), (-L, -L, 2)], [(0, B, 2), (L, -L, 2), (-L, -L, 2)]]
    d = _exact([p for tri in at for p in tri] + kept, np.arange(15).reshape(5, 3), (H, W))
    dropped = np.zeros((1, 15), bool)
    dropped[0, [2, 4, 7, 9]] = True
    for flags in (CULL, 0):
        g, frame = _both(d, flags)
        _assert_screen(g, d, dropped)
        x, y = g['screen_xy'][0, 12:, 0].astype(np.int64), g['screen_xy'][0, 12:, 1].astype(np.int64)
        A = _orient((x[0], y[0]), (x[1], y[1]), (x[2], y[2]))
        assert A == -4 * (2 ** 28 - 16) ** 2 and 2 ** 57 < -A < 2 ** 60
        ids = _assert_maps(g, frame, d, flags)                               # ids and depth bits: rasterize's
        assert (ids == 4).all() and ids.size == 117                          # the four nearer triangles with a vertex AT the limit are gone


@pytest.mark.parametrize('bad', ['nan', 'inf', 'nan_x_only'])
def test_a_non_finite_vertex_drops_its_triangles_and_nothing_else(bad):
    """The two-mesh shading scene with one visible vertex of mesh 0 made NaN / Inf.  The faces of mesh 0 that name it are not
    drawn; those that name one of its neighbours are (their own vertices are finite), shaded from the int32 sums the contract
    states - every NaN component of a face normal counts -2^30 at all three vertices, and two such faces wrap the sum; the rest
    of the picture (mesh 1, the frame) is the picture without that vertex's triangles: the one in which the vertex is finite
    and dropped for lying behind the camera."""
    CULL = _flags()[0]
    d = RR.shading_scene(2)
    F = d['f'].shape[0]
    clean, _ = _both(d, CULL)
    cid = clean['id_map']
    shown = np.bincount(d['f'][np.unique(cid[(cid >= 0) & (cid < F)])].ravel(), minlength=12)
    k = int(np.nonzero(shown == 3)[0][0])                                     # a vertex with three of its faces in the picture
    names = (d['f'] == k).any(1)
    near = np.isin(d['f'], np.unique(d['f'][names])).any(1) & ~names         # faces that name a neighbour of k, not k itself
    assert names.sum() == 5 and near.sum() == 10
    v = d['v'].copy()
    v[0, k] = {'nan': [np.nan] * 3, 'inf': [np.inf, v[0, k, 1], v[0, k, 2]], 'nan_x_only': [np.nan, v[0, k, 1], v[0, k, 2]]}[bad]
    broken = dict(d, v=v)
    g, frame = _both(broken, CULL)
    gone = np.zeros((2, 12), bool)
    gone[0, k] = True
    assert np.array_equal((g['screen_xy'] == RR.DROPPED).all(-1), gone) and np.array_equal(g['screen_xy'][~gone], clean['screen_xy'][~gone])
    ids = _assert_maps(g, frame, broken, CULL)                               # the bytes follow the restated sums (resolve calls normal_sums)
    touched = (ids >= 0) & (ids < F) & near[ids % F]
    assert not ((ids >= 0) & (ids < F) & names[ids % F]).any() and touched.sum() > 50 and (ids >= F).sum() > 50
    sums = RR.normal_sums(v, d['f'])
    assert (sums != RR.normal_sums(d['v'], d['f']))[0, np.unique(d['f'][names])].any(1).all() and np.array_equal(sums[1], RR.normal_sums(d['v'], d['f'])[1])
    # the same vertex finite and behind the camera (R^T p has z = 10 for p = 10 x the third column of R, so Z = 3 - 10)
    p = 10 * d['R'].astype(np.float64)[:, 2]
    behind = d['v'].copy()
    behind[0, k] = [p[0], -p[1], -p[2]]
    without, _ = _both(dict(d, v=behind), CULL)
    assert np.array_equal((without['screen_xy'] == RR.DROPPED).all(-1), gone)
    assert np.array_equal(without['id_map'], ids) and without['depth'].tobytes() == g['depth'].tobytes()
    assert (ids >= 0).sum() < (cid >= 0).sum()                                # the vertex's faces did show before
    assert np.array_equal(g['image'][~touched], without['image'][~touched])
    assert (g['image'][touched] != without['image'][touched]).any()           # the NaN did reach the neighbours' normals


def test_faces_that_name_no_vertex_are_ignored_altogether():
    CULL = _flags()[0]
    d = RR.shading_scene()
    V = d['v'].shape[1]
    extra = np.array([[-1, 0, 1], [0, V, 1], [0, 1, INT32_MIN], [-1, -1, -1], [V, V, V], [INT32_MIN, 5, V], [3, -1, 4]], np.int32)
    for flags in (0, CULL):
        base, _ = _both(d, flags)
        assert (base['id_map'] >= 0).sum() > 200
        for faces in (np.concatenate([d['f'], extra]), np.concatenate([d['f'], extra[::-1]])):
            g, _ = _both(dict(d, f=np.ascontiguousarray(faces)), flags)
            for k in KEYS:
                assert g[k].tobytes() == base[k].tobytes(), k
    # and in front of the real faces: the ids shift by the rows, nothing else changes
    g, _ = _both(dict(d, f=np.ascontiguousarray(np.concatenate([extra, d['f']]))), CULL)
    assert np.array_equal(g['id_map'], np.where(base['id_map'] >= 0, base['id_map'] + len(extra), -1))
    assert g['image'].tobytes() == base['image'].tobytes() and g['depth'].tobytes() == base['depth'].tobytes()


def test_triangles_that_draw_nothing():
    """A == 0 (collinear through pixel centres; a repeated vertex), wholly off the frame on each side, and slivers of non-zero
    area that contain no pixel centre: nothing is drawn, culling or not."""
    CULL = _flags()[0]
    H, W = 9, 13
    pts = [(1.5, 1.5), (4.5, 4.5), (7.5, 7.5),                  # collinear, through pixel centres
           (2.5, 6.5), (2.5, 6.5), (9.5, 3.5),                  # a repeated vertex
           (-9, 1), (-1, 2), (-3, 8),                           # left of the frame
           (14, 1), (20, 2), (15, 8),                           # right of it
           (1, -7), (11, -1), (4, -0.25),                       # above it (the last row of centres it could reach is -0.5)
           (1, 9.75), (11, 10), (4, 15),                        # below it
           (1.625, 1.625), (8.625, 1.625), (8.625, 1.75),       # a sliver between two rows of centres
           (3.5625, 0.25), (3.9375, 8.75), (3.625, 0.25)]       # a sliver between two columns of centres
    tris = np.arange(len(pts)).reshape(-1, 3)
    u = _units(pts)
    area = [_orient(*(u[k] for k in f)) for f in tris]
    assert area[0] == 0 and area[1] == 0 and all(a != 0 for a in area[2:])
    for faces in (tris, tris[:, ::-1]):
        d = _exact([p + (4,) for p in pts], faces, (H, W))
        for flags in (0, CULL):
            g, frame = _both(d, flags)
            _assert_screen(g, d)
            ids = _assert_maps(g, frame, d, flags)
            assert (ids == -1).all() and (g['depth'] == 0).all() and np.array_equal(g['image'], frame)


def test_a_frame_of_one_pixel():
    CULL, SIDE = _flags()[:2]
    for pts, want in (([(-3, -3, 4), (-3, 5, 4), (5, -3, 4)], 0), ([(0.5, 0.5, 2), (0.5, 3, 4), (3, 0.5, 8)], 0), ([(0.5, 0.5, 2), (0.5, -3, 4), (-3, 0.5, 8)], -1)):
        d = _exact(pts, [(0, 1, 2)], (1, 1))
        g, frame = _both(d, CULL)
        _assert_screen(g, d)
        ids = _assert_maps(g, frame, d, CULL)
        assert ids.shape == (1, 1) and ids[0, 0] == want                      # a vertex ON the centre: in when it is the top-left corner
    d = dict(RR.shading_scene(), size=(1, 1), cam=(30., 30., 0.5, 0.5))
    for flags in (CULL, CULL | SIDE):
        g, frame = _both(d, flags)
        assert _assert_maps(g, frame, d, flags)[0, 0] >= 0


def test_bounding_box_of_17_pixels_ends_in_a_partial_block():
    """Columns 50 .. 66 and rows 0 .. 10 of a 12 x 70 frame: three 8 x 8 blocks across (8, 8 and 1 columns), two down (8 and 3 rows)."""
    H, W = 12, 70
    pts = [(50.25, 0.25, 4), (67.25, 0.25, 2), (58, 11.25, 8), (50.25, 11.25, 4), (67.25, 11.25, 8), (60, 0.25, 2)]
    d = _exact(pts, [(0, 1, 2), (3, 4, 5)], (H, W))
    g, frame = _both(d, 0)
    _assert_screen(g, d)
    ids = _assert_maps(g, frame, d, 0)
    for f in range(2):          # each triangle's own box is the 17 x 11 one: the pixel centres (index + 0.5) between its extremes
        x, y = [p[0] for p in pts[3 * f:3 * f + 3]], [p[1] for p in pts[3 * f:3 * f + 3]]
        assert (np.ceil(min(x) - 0.5), np.floor(max(x) - 0.5), np.ceil(min(y) - 0.5), np.floor(max(y) - 0.5)) == (50, 66, 0, 10)
        assert (ids == f).sum() > 40
    cols, rows = np.nonzero((ids >= 0).any(0))[0], np.nonzero((ids >= 0).any(1))[0]
    assert (cols[0], cols[-1], rows[0], rows[-1]) == (50, 66, 0, 10)
    assert (ids[:8, 66] >= 0).any() and (ids[8:11, 50:66] >= 0).any() and (ids[8:11, 66] >= 0).any()      # no partial last block is empty


# ---- shading -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('meshes', [1, 2])
@pytest.mark.parametrize('side', [False, True])
def test_smooth_shading_vs_resolve_in_float64_and_fp32(meshes, side):
    """The icosahedron scene of tests/test_render_host.py: the covered bytes against ``resolve`` fed the device's own snapped
    coordinates and depths.  Within 1 of the float64 byte everywhere; equal wherever the float64 value is farther than delta =
    4 x max |fp32 - float64| from a half-integer (at least 99 % of the pixel-channels: the cap is asserted here again, on the
    device's inputs); and equal to the fp32 restatement at every byte.
    Measured on MI355X (profiles/render_edges.json): 0 bytes differ from the fp32 restatement in all four cases - hipcc's
    sqrtf, its fp32 division and its int64 / int32 -> float conversions round as NumPy's do."""
    CULL, SIDE = _flags()[:2]
    d = RR.shading_scene(meshes)
    flags = CULL | (SIDE if side else 0)
    g, frame = _both(d, flags)
    sx, sy = g['screen_xy'][..., 0], g['screen_xy'][..., 1]
    ids = RR.rasterize(sx, sy, g['screen_z'], d['f'], *d['size'])[0]
    assert np.array_equal(g['id_map'], ids)
    cov = ids >= 0
    assert cov.sum() > 200 and len(np.unique(ids[cov])) >= 7 and (meshes == 1 or all(((ids[cov] // 20) == m).sum() > 50 for m in range(2)))
    v32, b32 = RR.resolve(sx, sy, g['screen_z'], d['v'], d['f'], ids, d['rgb'], side, np.float32)
    v64, b64 = RR.resolve(sx, sy, g['screen_z'], d['v'], d['f'], ids, d['rgb'], side, np.float64)
    gap, delta, near, covered = RR.half_integer_margin(v32, v64)
    share = near.sum() / covered.sum()
    img = g['image'].astype(np.int64)
    off64, off32 = int((img != b64)[covered].sum()), int((img != b32)[covered].sum())
    print(f'M={meshes} side={side}: {cov.sum()} px, |fp32 - float64| {gap:.3e} byte, delta {delta:.3e}, near a half-integer {near.sum()} of {covered.sum()}, '
          f'bytes != float64 restatement {off64}, != fp32 restatement {off32}, worst |byte - float64 value| {np.abs(img - v64)[covered].max():.6f}')
    assert share <= 0.01
    assert (np.abs(img - b64)[covered] <= 1).all()
    assert np.array_equal(img[covered & ~near], b64.astype(np.int64)[covered & ~near])
    assert off32 == 0
    assert np.array_equal(g['image'][~cov], np.zeros_like(frame)[~cov] if side else frame[~cov])


# ---- small views in specmi_render_views --------------------------------------------------------------------------------------
@pytest.mark.parametrize('thread', [False, True])
def test_views_of_a_few_pixels_equal_their_render_meshes_calls(thread):
    """Views of 1 x 1, 2 x 3, 5 x 7 and 1 x 70 pixels and one without meshes between them, 6-vertex octahedra: the 72 vertices of
    the 12 (view, mesh) pairs are two wavefronts, the first serving eleven pairs of eight views (the per-lane atomicMin of the
    lowest vertex); the first resolve wavefront crosses six view boundaries (the walk along px_prefix).  Every view equals its own
    render_meshes call byte for byte, the checker - whose height is the view's own lowest vertex - included."""
    from spec_amd import cam_utils, render
    from spec_amd.preprocess import pack_frames
    from tests.test_gpu_render_views import MAPS, _split
    CULL, SIDE, GROUND, THREAD = _flags()
    eng = cam_utils._engine(torch.device(DEV))
    ov, faces = RR.octahedron(1.0)
    ov = (ov.astype(np.float64) @ RR.rot(0.4, 0.7).astype(np.float64).T).astype(np.float32)
    sizes = [(1, 1), (2, 3), (5, 7), (1, 70)]
    counts, first = [1, 2, 1, 2], [0, 1, 3, 4]
    scale = [1.0, 0.8, 1.2, 0.9, 0.7, 1.1]
    cam_t = np.float32([[0.0, 0.0, 4.0], [0.3, -0.1, 4.0], [-0.4, 0.6, 5.0], [0.1, 0.2, 3.5], [-1.5, 0.3, 4.0], [1.2, -0.7, 5.5]])
    verts = np.ascontiguousarray(np.stack([ov * s for s in scale]), np.float32)
    Rs = [RR.rot(0.1, -0.05), RR.rot(-0.2, 0.15), RR.rot(0.3, 0.0), RR.rot(0.25, 0.1)]
    focal, center = [(2., 2.), (3., 3.), (6., 6.), (20., 20.)], [(0.5, 0.5), (1.5, 1.0), (3.5, 2.5), (35.0, 0.5)]
    views = [(0, 1, CULL), (0, 1, CULL | SIDE | GROUND), (1, 2, CULL), (1, 2, CULL | SIDE | GROUND), (1, 0, 0),
             (2, 1, CULL), (2, 1, CULL | SIDE | GROUND), (3, 2, 0), (3, 2, CULL | SIDE | GROUND)]
    assert sum(c for _, c, _ in views) * 6 == 72 and sum(sizes[f][0] * sizes[f][1] for f, _, _ in views[:6]) <= 64
    rng = np.random.default_rng(17)
    frames = [rng.integers(0, 256, (H, W, 3), dtype=np.uint8) for H, W in sizes]
    slab, in_off, _ = pack_frames(frames, DEV)
    v, f, tt = t(verts).to(DEV), t(faces).to(DEV), t(cam_t).to(DEV)
    geom, offsets, off, ref = [], [], 0, []
    for fr, c, fl in views:
        H, W = sizes[fr]
        geom.append((H, W, first[fr] if c else 0, c, fl | (THREAD if thread else 0)))
        offsets.append((int(in_off[fr]), 3 * W, off, 3 * W))
        off += 3 * H * W
        if c == 0:
            ref.append({'image': t(frames[fr]).to(DEV)})
        else:
            ref.append(eng.render_meshes(v[first[fr]:first[fr] + c], f, tt[first[fr]:first[fr] + c], t(Rs[fr]).to(DEV), focal[fr], center[fr],
                                         frame=t(frames[fr]).to(DEV), rgb=RGB, flags=fl, maps=True))
    geom, offsets = np.asarray(geom, np.int32), np.asarray(offsets, np.int64)
    out = torch.full((off,), 0xA5, dtype=torch.uint8, device=DEV)
    got = eng.render_views(v, f, tt, geom, offsets, render.view_cams([fr for fr, _, _ in views], Rs, focal, center), slab, out, rgb=RGB, maps=True)
    plane, mesh = [], 0
    for k, (view, r) in enumerate(zip(_split(got, geom, offsets), ref)):
        assert torch.equal(view['image'], r['image']), (k, 'image')
        if views[k][1] == 0:
            assert (view['id_map'] == -1).all() and (view['depth'] == 0).all() and view['screen_xy'].shape[0] == 0
            continue
        for key in MAPS:
            assert torch.equal(view[key], r[key]), (k, key)
        assert views[k][2] & SIDE or (r['id_map'] >= 0).any(), k              # every overlay shows its meshes (a side view may show the plane alone)
        plane.append(int((r['id_map'] == -2).sum()))
        mesh += int((r['id_map'] >= 0).sum())
    # the views are not empty: the ground plane - drawn only where the view's lowest vertex arrived - is in three side views at least
    assert sum(p > 0 for p in plane) >= 3 and sum(plane) >= 20 and mesh >= 15
    lows = [RR.lowest_y(verts[first[fr]:first[fr] + c], cam_t[first[fr]:first[fr] + c], Rs[fr]) for fr, c, fl in views if fl & GROUND]
    assert len(set(float(x) for x in lows)) == 4                             # and each of them has a lowest vertex of its own
