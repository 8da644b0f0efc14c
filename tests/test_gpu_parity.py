"""Parity of the HIP path (libyart.so on the MI355X) against the CPU restatement (oracle).

Both sides evaluate the reference's hot path in IEEE f64 with the same counter-based RNG, so the
bar is BITWISE equality, not a tolerance: every pixel sum, every hit record, every random draw.
The one libm call the device cannot share, finalize's glibc pow, is replaced by the 255 steps of the
reference's byte map (test_finalize_bytes.py), so the RGBA8 output is bitwise too.
"""
import ctypes as C
import math

import numpy as np
import pytest

import mt_numpy as MT
import oracle_lib as O
import yart
from yart import abi

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def dev():
    L = yart.load_device()
    n = C.c_int()
    assert L.yart_device_count(C.byref(n)) == 0 and n.value >= 1, L.yart_last_error()
    return L


def test_rng_stream_bitwise(dev):
    for seed, pixel, sample in [(0x59415254, 0, 0), (1, 123456, 255), (2**63 + 5, 2**32 - 1, 7)]:
        out = np.empty(1000, dtype=np.float64)
        assert dev.yart_probe_rng(0, seed, pixel, sample, 1000, out.ctypes.data_as(C.c_void_p)) == 0
        np.testing.assert_array_equal(out, O.rng_f64(seed, pixel, sample, 1000))


def _probe(dev, op, a, b=None):
    a = np.ascontiguousarray(a, dtype=np.float64)
    out = np.empty_like(a)
    bp = None if b is None else np.ascontiguousarray(b, dtype=np.float64).ctypes.data_as(C.c_void_p)
    assert dev.yart_probe_math(0, op, a.ctypes.data_as(C.c_void_p), bp, a.size, out.ctypes.data_as(C.c_void_p)) == 0
    return out


def test_device_sqrt_and_div_are_ieee(dev):
    rng = np.random.default_rng(3)
    a = np.concatenate([rng.uniform(0, 1e6, 100000), rng.uniform(0, 1e-3, 10000), 10.0 ** rng.uniform(-300, 300, 10000)])
    b = np.concatenate([rng.uniform(-1e3, 1e3, 110000), 10.0 ** rng.uniform(-300, 300, 10000)])
    np.testing.assert_array_equal(_probe(dev, 0, a), np.sqrt(a))
    with np.errstate(over="ignore", under="ignore"):
        want = a / b
    np.testing.assert_array_equal(_probe(dev, 1, a, b), want)


def _edge_values(rng, n):
    """Magnitudes across the whole f64 range (denormals, the fast paths' guard edges at 2^-767,
    2^-600, 2^-300, 2^300, 2^400, 2^600), signed zeros, inf and nan, plus ordinary values."""
    e = np.array([0.0, -0.0, np.inf, -np.inf, np.nan, 5e-324, -5e-324, 2.0 ** -1022, 2.0 ** -767, 2.0 ** -768,
                  2.0 ** -600, 2.0 ** -601, 2.0 ** -300, 2.0 ** -301, 2.0 ** 300, 2.0 ** 301, 2.0 ** 400,
                  2.0 ** 401, 2.0 ** 600, 2.0 ** 601, 1.0, -1.0, 1e-250, 1e250, 1.7976931348623157e308])
    mag = 2.0 ** rng.uniform(-1074, 1023, n) * rng.choice([-1.0, 1.0], n)
    ordinary = rng.uniform(-2, 2, n)
    picks = rng.choice(e, n)
    return np.where(rng.random(n) < 0.2, picks, np.where(rng.random(n) < 0.5, mag, ordinary))


def _bits(x):
    return np.ascontiguousarray(x, dtype=np.float64).view(np.uint64)


def test_device_fast_sqrt_unit_div_are_bitwise_ieee(dev):
    """kernels.hip's guarded fast paths (sqrt_x, unit, div3_pos) against numpy's correctly
    rounded operations, compared as bit patterns (sign of zero and NaN included)."""
    rng = np.random.default_rng(11)
    with np.errstate(all="ignore"):
        a = np.abs(_edge_values(rng, 200000))
        a[:8] = [0.0, -0.0, np.inf, np.nan, 5e-324, 2.0 ** -767, np.nextafter(2.0 ** -767, 0), -1.0]
        got, want = _probe(dev, 8, a), np.sqrt(a)
        nan = np.isnan(want)
        assert np.array_equal(np.isnan(got), nan)
        np.testing.assert_array_equal(_bits(got[~nan]), _bits(want[~nan]))

        v = _edge_values(rng, 3 * 100000).reshape(-1, 3)
        v[:6] = [[0.0, 1.0, 0.0], [-0.0, 1.0, -0.0], [1.0, 1e-250, 0.0], [3.0, -4.0, -0.0], [2.0 ** -700, 1.0, 0.0],
                 [0.0, 0.0, 0.0]]
        l = np.sqrt(v[:, 0] * v[:, 0] + v[:, 1] * v[:, 1] + v[:, 2] * v[:, 2])
        want = (v / l[:, None]).ravel()
        got = _probe(dev, 9, v.ravel())
        nan = np.isnan(want)
        assert np.array_equal(np.isnan(got), nan)
        np.testing.assert_array_equal(_bits(got[~nan]), _bits(want[~nan]))

        t = _edge_values(rng, 3 * 100000)
        s = np.abs(_edge_values(rng, 100000))
        s[s == 0] = 1.0
        s = np.repeat(s, 3)  # one denominator per triple, laid out like the numerators
        want = t / s
        got = _probe(dev, 10, t, s[::3].copy())
        nan = np.isnan(want)
        assert np.array_equal(np.isnan(got), nan)
        np.testing.assert_array_equal(_bits(got[~nan]), _bits(want[~nan]))


def test_device_sin_cos_match_oracle(dev):
    rng = np.random.default_rng(4)
    a = np.concatenate([rng.uniform(0, 2 * math.pi, 50000), rng.uniform(-500, 500, 50000)])
    L = O.lib()
    np.testing.assert_array_equal(_probe(dev, 2, a), np.array([L.oracle_sin(x) for x in a]))
    np.testing.assert_array_equal(_probe(dev, 3, a), np.array([L.oracle_cos(x) for x in a]))


def test_device_log_matches_oracle(dev):
    rng = np.random.default_rng(6)
    a = np.concatenate([rng.uniform(0, 1, 50000), 10.0 ** rng.uniform(-300, 300, 20000), [0.0, 1.0, 5e-324]])
    L = O.lib()
    np.testing.assert_array_equal(_probe(dev, 5, a), np.array([L.oracle_log(x) for x in a]))


def test_device_acos_atan2_match_oracle(dev):
    rng = np.random.default_rng(7)
    a = np.concatenate([rng.uniform(-1, 1, 50000), [1.0, -1.0, 0.0, -0.0, 0.5, -0.5]])
    L = O.lib()
    np.testing.assert_array_equal(_probe(dev, 6, a), np.array([L.oracle_acos(x) for x in a]))
    y, x = rng.normal(size=(2, 50000)) * 10.0 ** rng.uniform(-5, 5, (2, 50000))
    y = np.concatenate([y, [0.0, -0.0, 1.0, -1.0]])
    x = np.concatenate([x, [-1.0, -1.0, 0.0, 0.0]])
    np.testing.assert_array_equal(_probe(dev, 7, y, x), np.array([L.oracle_atan2(p, q) for p, q in zip(y, x)]))


def _hits_equal(h1, o1, h2, o2):
    np.testing.assert_array_equal(o1, o2)
    m = o1 >= 0
    np.testing.assert_array_equal(h1[m], h2[m])


def test_intersect_qbvh_fixture(dev):
    from test_oracle_known_answers import FIXTURE_RAY, fixture_scene
    for rev in (False, True):
        b = fixture_scene(rev)
        d = b.desc()
        s = yart.DeviceScene(d)
        h, o = s.intersect(np.array(FIXTURE_RAY + [0.0, np.inf]))
        assert o[0] == (2 if rev else 1)
        assert abs(h[0, 0] - 0.954084586) < 1e-9
        h2, o2 = O.OracleScene(d).intersect(np.array(FIXTURE_RAY + [0.0, np.inf]))
        _hits_equal(h, o, h2, o2)


def _random_rays(n, lo, hi, seed):
    rng = np.random.default_rng(seed)
    o = rng.uniform(lo, hi, (n, 3))
    d = rng.normal(size=(n, 3))
    r = np.concatenate([o, d, np.full((n, 1), 0.001), np.full((n, 1), np.inf)], axis=1)
    return r


@pytest.mark.parametrize("scene", ["cornell-box", "david", "sycee", "three-spheres", "random-scene", "cornell-box-smoke",
                                   "two-perlin-spheres"])
def test_intersect_matches_oracle(dev, scene):
    p = yart.Preset(scene)
    bounds = {"cornell-box": (0, 555), "david": (-150, 250), "sycee": (-4, 4), "three-spheres": (-3, 3),
              "random-scene": (-12, 12), "cornell-box-smoke": (0, 555), "two-perlin-spheres": (-6, 6)}[scene]
    rays = _random_rays(200000, *bounds, seed=11)
    # camera-like rays too: from the preset's eye towards the scene
    eye = np.array(p.defaults.lookfrom)
    tgt = _random_rays(50000, *bounds, seed=12)[:, :3]
    cam_rays = np.concatenate([np.tile(eye, (50000, 1)), tgt - eye, np.full((50000, 1), 0.001),
                               np.full((50000, 1), np.inf)], axis=1)
    rays = np.concatenate([rays, cam_rays])
    s = yart.DeviceScene(p.desc)
    h, o = s.intersect(rays)
    h2, o2 = O.OracleScene(p.desc).intersect(rays)
    assert (o >= 0).mean() > 0.05
    _hits_equal(h, o, h2, o2)


@pytest.mark.parametrize("scene,render", [("david", ("david", 48, 27, 2)), ("sycee", ("bunny", 40, 40, 4))])
def test_qbvh_tie_order_does_not_change_hits(dev, scene, render, opt):
    """The reference sorts split ranges with sort_unstable_by (qbvh.rs:679-685), so the order of
    equal centroid keys — and with it leaf membership and lane order at 3,943 of david's cuts — is
    not pinned. Build the BLAS a second time with the opposite tie order and require the same
    closest hits on 250k random and camera rays and the same renders: the answer does not depend
    on the freedom the reference leaves open, on these meshes."""
    p = yart.Preset(scene)
    bounds = {"david": (-150, 250), "sycee": (-4, 4)}[scene]
    rays = _random_rays(200000, *bounds, seed=31)
    eye = np.array(p.defaults.lookfrom)
    tgt = _random_rays(50000, *bounds, seed=32)[:, :3]
    rays = np.concatenate([rays, np.concatenate([np.tile(eye, (50000, 1)), tgt - eye, np.full((50000, 1), 0.001),
                                                 np.full((50000, 1), np.inf)], axis=1)])
    a = yart.DeviceScene(p.desc)
    ha, oa = a.intersect(rays)
    rp = yart.Preset(render[0])
    cam, prm = rp.camera(render[1], render[2]), yart.render_params(render[1], render[2], render[3], 50)
    ra = yart.DeviceScene(rp.desc).render(cam, prm)
    opt("qbvh_ties_desc", 1)
    b = yart.DeviceScene(p.desc)
    assert b.info().bvh_tied_cuts > 0 and a.info().bvh_tied_cuts > 0
    hb, ob = b.intersect(rays)
    rb = yart.DeviceScene(rp.desc).render(cam, prm)
    differ = int(((oa != ob) | np.any((ha != hb) & ~(np.isnan(ha) & np.isnan(hb)), axis=1)).sum())
    assert differ == 0, f"{differ} of {len(rays)} closest hits depend on the tie order"
    assert (oa >= 0).mean() > 0.05
    np.testing.assert_array_equal(ra, rb)


@pytest.mark.parametrize("scene,render", [("david", ("david", 48, 27, 2)), ("sycee", ("bunny", 40, 40, 4))])
def test_forced_rewalk_is_the_reference_answer(dev, scene, render):
    """After the cooperative front-to-back walk, each lane checks its own ray's winner against the
    reference's f64 box test; a ray that fails walks again in the reference's order, per lane
    (qbvh_t). That path is almost never taken on real frames, so yart_debug_force_rewalk sends
    every walk that found a hit down it: closest hits and renders stay bitwise the oracle's."""
    p = yart.Preset(scene)
    bounds = {"david": (-150, 250), "sycee": (-4, 4)}[scene]
    rays = _random_rays(100000, *bounds, seed=41)
    rp = yart.Preset(render[0])
    cam, prm = rp.camera(render[1], render[2]), yart.render_params(render[1], render[2], render[3], 50)
    h2, o2 = O.OracleScene(p.desc).intersect(rays)
    ref = O.OracleScene(rp.desc).render(cam, prm)
    assert dev.yart_debug_force_rewalk(0, 1) == 0
    try:
        h, o = yart.DeviceScene(p.desc).intersect(rays)
        rs = yart.DeviceScene(rp.desc)
        img = rs.render(cam, prm)
        _, st = rs.render_with_stats(cam, prm)
    finally:
        assert dev.yart_debug_force_rewalk(0, 0) == 0
    assert (o2 >= 0).mean() > 0.05
    _hits_equal(h, o, h2, o2)
    np.testing.assert_array_equal(img, ref)
    assert st.mesh_rewalks > 0


def test_box_cull_is_exact_on_grazing_rays(dev):
    """The device's f32 box pre-test may only skip boxes no face of which is hit: rays aimed at
    box edges and corners, nudged by a few ulps to tiny offsets, must hit exactly as the oracle."""
    b = O.DescBuilder()
    m = b.material(abi.MAT_LAMBERTIAN, b.texture((0.5, 0.5, 0.5)))
    b.obj(abi.PRIM_BOX, m, (130.0, 0.0, 65.0, 295.0, 165.0, 230.0))
    b.obj(abi.PRIM_BOX, m, (0.0, 0.0, 0.0, 165.0, 330.0, 165.0),
          xforms=[(abi.XF_TRANSLATE, (265.0, 0.0, 295.0)), (abi.XF_ROTATE_Y, (15.0, 0.0, 0.0))])
    b.obj(abi.PRIM_BOX, m, (-1e-3, -2e-3, -1e-3, 1e-3, 2e-3, 1e-3), xforms=[(abi.XF_TRANSLATE, (400.0, 5.0, 50.0))])
    d = b.desc()
    rng = np.random.default_rng(21)
    n = 120000
    corners = np.array([[x, y, z] for x in (130.0, 295.0) for y in (0.0, 165.0) for z in (65.0, 230.0)])
    tgt = corners[rng.integers(0, 8, n)]
    # slide along a random edge direction, then nudge off the surface by 0..1e-9 relative
    edge = np.eye(3)[rng.integers(0, 3, n)] * rng.uniform(0, 165, (n, 1))
    tgt = tgt + edge * np.where(rng.random((n, 1)) < 0.5, 0.0, 1.0)
    tgt = tgt * (1.0 + rng.choice([-1.0, 0.0, 1.0], (n, 3)) * 10.0 ** rng.uniform(-16, -9, (n, 3)))
    tiny = np.array([400.0, 5.0, 50.0]) + rng.uniform(-2e-3, 2e-3, (20000, 3))
    tgt = np.concatenate([tgt, tiny])
    org = rng.uniform(-600, 1200, (tgt.shape[0], 3))
    dirs = (tgt - org) * rng.choice([1.0, 1e-3, 1e3], (tgt.shape[0], 1))
    rays = np.concatenate([org, dirs, np.full((len(org), 1), 0.001), np.full((len(org), 1), np.inf)], axis=1)
    rays[::7, 7] = rng.uniform(0.5, 2.0, len(rays[::7])) * np.linalg.norm(tgt - org, axis=1)[::7] / \
        np.linalg.norm(dirs, axis=1)[::7]  # finite t_max around the hit distance
    h, o = yart.DeviceScene(d).intersect(rays)
    h2, o2 = O.OracleScene(d).intersect(rays)
    assert (o >= 0).mean() > 0.2
    _hits_equal(h, o, h2, o2)


def test_box_cull_is_exact_on_axis_parallel_and_tiny_direction_rays(dev):
    """r05: the box entity's f32 pre-test leaves an axis unconstrained through a NaN reciprocal
    (fmaxf / fminf ignore it) instead of a branch when the direction's f32 component is below 1e-20
    (zero, denormal, tiny). Rays with one or two such components aimed at the faces, edges and
    corners of plain, rotated and tiny boxes: closest hits bitwise the oracle's."""
    b = O.DescBuilder()
    m = b.material(abi.MAT_LAMBERTIAN, b.texture((0.5, 0.5, 0.5)))
    b.obj(abi.PRIM_BOX, m, (130.0, 0.0, 65.0, 295.0, 165.0, 230.0))
    b.obj(abi.PRIM_BOX, m, (0.0, 0.0, 0.0, 165.0, 330.0, 165.0),
          xforms=[(abi.XF_TRANSLATE, (265.0, 0.0, 295.0)), (abi.XF_ROTATE_Y, (15.0, 0.0, 0.0))])
    b.obj(abi.PRIM_BOX, m, (-1e-3, -2e-3, -1e-3, 1e-3, 2e-3, 1e-3), xforms=[(abi.XF_TRANSLATE, (400.0, 5.0, 50.0))])
    d = b.desc()
    rng = np.random.default_rng(37)
    n = 60000
    lo, hi = np.array([130.0, 0.0, 65.0]), np.array([295.0, 165.0, 230.0])
    tgt = rng.uniform(lo, hi, (n, 3))
    snap = rng.integers(0, 3, (n, 3))  # per axis: inside, on the low face, on the high face
    tgt = np.where(snap == 1, lo, np.where(snap == 2, hi, tgt))
    tgt[: n // 6] = np.array([400.0, 5.0, 50.0]) + rng.uniform(-2e-3, 2e-3, (n // 6, 3))
    dirs = rng.normal(size=(n, 3))
    small = np.array([0.0, -0.0, 1e-30, -5e-324, 1e-21, -2e-20, 1e-19])
    for j in range(3):
        pick = rng.random(n) < 0.4
        dirs[pick, j] = rng.choice(small, pick.sum())
    keep = np.abs(dirs).max(axis=1) > 1e-3
    tgt, dirs = tgt[keep], dirs[keep]
    org = tgt - dirs * rng.uniform(50.0, 900.0, (len(tgt), 1)) / np.linalg.norm(dirs, axis=1)[:, None]
    rays = np.concatenate([org, dirs, np.full((len(org), 1), 0.001), np.full((len(org), 1), np.inf)], axis=1)
    h, o = yart.DeviceScene(d).intersect(rays)
    h2, o2 = O.OracleScene(d).intersect(rays)
    assert (o2 >= 0).mean() > 0.2
    _hits_equal(h, o, h2, o2)


@pytest.mark.parametrize("scene", ["sycee", "david"])
def test_mesh_cull_box_is_exact_on_grazing_rays(dev, scene):
    """A ray whose conservative f32 test misses a mesh's cull box (the union of both roots' child
    boxes, DevMesh::box_lo/hi) is left out of the cooperative walk. Rays aimed at the box's faces,
    edges and corners — nudged by 1e-16..1e-7 relative either way, from outside and inside, with
    infinite and finite t_max — must hit exactly as the oracle's walk of the reference tree."""
    p = yart.Preset(scene)
    m = p.desc.contents.meshes[0]
    pos = np.ctypeslib.as_array(m.positions, shape=(m.n_triangles * 9,)).reshape(-1, 3).astype(np.float64)
    lo, hi = pos.min(0), pos.max(0)  # the first list entry holds the mesh without a wrapper
    rng = np.random.default_rng(51)
    n = 150000
    tgt = rng.uniform(lo, hi, (n, 3))
    ax = rng.integers(0, 3, n)
    tgt[np.arange(n), ax] = np.where(rng.random(n) < 0.5, lo[ax], hi[ax])  # on a face
    pin = rng.random(n) < 0.4  # on an edge or (with a third pin) a corner
    ax2 = (ax + 1 + rng.integers(0, 2, n)) % 3
    tgt[pin, ax2[pin]] = np.where(rng.random(pin.sum()) < 0.5, lo[ax2[pin]], hi[ax2[pin]])
    tgt = tgt * (1.0 + rng.choice([-1.0, 0.0, 1.0], (n, 3)) * 10.0 ** rng.uniform(-16, -7, (n, 3)))
    span = hi - lo
    org = lo - span + rng.random((n, 3)) * 3.0 * span
    dirs = tgt - org
    rays = np.concatenate([org, dirs, np.full((n, 1), 0.001), np.full((n, 1), np.inf)], axis=1)
    rays[::5, 7] = rng.uniform(0.9, 1.1, len(rays[::5]))  # t_max around the box face (|dirs| reaches it at t = 1)
    h, o = yart.DeviceScene(p.desc).intersect(rays)
    h2, o2 = O.OracleScene(p.desc).intersect(rays)
    assert (o2 >= 0).mean() > 0.02 and (o2 < 0).mean() > 0.05
    _hits_equal(h, o, h2, o2)


@pytest.mark.parametrize("scene", ["cornell-box", "three-spheres", "two-spheres", "random-scene"])
def test_world_bvh_forced_on_matches_linear_scan(dev, scene, opt):
    """The world_bvh option = 1 puts every boxable list behind the world BVH (wrappers, boxes, flipped
    light included): closest hits and renders stay bitwise the oracle's linear HittableList."""
    opt("world_bvh", 1)
    p = yart.Preset(scene)
    s = yart.DeviceScene(p)
    assert s.info().world_nodes > 0
    bounds = {"cornell-box": (0, 555), "three-spheres": (-3, 3), "two-spheres": (-12, 12),
              "random-scene": (-12, 12)}[scene]
    rays = _random_rays(100000, *bounds, seed=13)
    h, o = s.intersect(rays)
    h2, o2 = O.OracleScene(p.desc).intersect(rays)
    _hits_equal(h, o, h2, o2)
    W, H, spp = 40, 32, 4
    cam = p.camera(W, H)
    np.testing.assert_array_equal(s.render(cam, yart.render_params(W, H, spp, 50)),
                                  O.OracleScene(p.desc).render(cam, yart.render_params(W, H, spp, 50)))


@pytest.mark.parametrize("world_bvh", [0, 1])
def test_rays_in_face_planes_match_oracle(dev, opt, world_bvh):
    """A ray lying exactly in a rect's plane (d[a] == 0 and o[a] == its k) gets t = 0 / 0 = NaN in
    the reference's rect test, and a NaN t passes the range and bounds tests: the reference reports
    a hit (t = NaN) wherever the ray runs, outside the rect too. Neither the box entity's f32 cull
    nor the world BVH's node culling may drop such an object (r05: both did, since r02 / r03; such
    rays now skip the cull / take the list walk). The cornell box's walls, light and the boxes'
    faces (the rotated boxes' bottom face lies in y = 0 in their frame too), list walk and forced
    world BVH: closest hits bitwise the oracle's."""
    opt("world_bvh", world_bvh)
    p = yart.Preset("cornell-box")
    s = yart.DeviceScene(p)
    assert (s.info().world_nodes > 0) == (world_bvh == 1)
    rng = np.random.default_rng(43)
    n = 40000
    org = rng.uniform(0.0, 555.0, (n, 3))
    dirs = rng.normal(size=(n, 3))
    ax = rng.integers(0, 3, n)
    planes = {0: [0.0, 555.0, 213.0, 343.0], 1: [0.0, 555.0, 554.0, 165.0, 330.0], 2: [555.0, 227.0, 332.0]}
    inplane = rng.random(n) < 0.7
    for a in range(3):
        rows = np.nonzero((ax == a) & inplane)[0]
        org[rows, a] = rng.choice(planes[a], len(rows))
    dirs[np.arange(n), ax] = rng.choice([0.0, -0.0], n)
    rays = np.concatenate([org, dirs, np.full((n, 1), 0.001), np.full((n, 1), np.inf)], axis=1)
    h, o = s.intersect(rays)
    h2, o2 = O.OracleScene(p.desc).intersect(rays)
    assert (o2 >= 0).mean() > 0.2 and np.isnan(h2[:, 0][o2 >= 0]).any()  # NaN-t "hits" are among them
    _hits_equal(h, o, h2, o2)


@pytest.mark.parametrize("world_bvh", [0, 1])
def test_rays_in_rotated_planes_match_oracle(dev, opt, world_bvh):
    """The rotated variant of the test above: rays whose direction has NO zero
    world component but an exactly zero one in a RotateY'd rect's or box's own frame (cos 90° · d_x
    == d_z, and the like at 30°, -18° under Translate, 200° + 271.5°, under FlipFace), half of them
    starting exactly in that local plane, where the reference's rect test "hits" with t = NaN
    wherever the ray runs (tests/inplane_rays.py builds them). A 26-object list, list walk and
    forced world BVH: the BVH's node boxes must not cull those hits (r05 residual: they did; the
    walk now sends such rays to the list walk, DevScene::plane_frames). Closest hits bitwise the
    oracle's."""
    import inplane_rays as IR
    opt("world_bvh", world_bvh)
    b, planes = IR.rotated_planes_scene()
    d = b.desc()
    s = yart.DeviceScene(d)
    assert (s.info().world_nodes > 0) == (world_bvh == 1)
    rays = IR.rotated_plane_rays(planes, 2000)
    assert (rays[:, 3:6] != 0).all()
    h2, o2 = O.OracleScene(d).intersect(rays)
    nan = (o2 >= 0) & np.isnan(h2[:, 0])
    assert nan.sum() > 5000 and len(np.unique(o2[nan])) == 6  # every rotated object gets NaN-t hits
    h, o = s.intersect(rays)
    _hits_equal(h, o, h2, o2)


@pytest.mark.parametrize("n", [17, 64, 257, 600])
def test_world_bvh_4wide_mixed_lists_match_linear_scan(dev, n):
    """The 4-wide world BVH (forced on) over random mixed lists — plain, hollow and translated
    spheres, rects, translated + rotated boxes, triangles, flipped rects (oracle_lib.mixed_list_desc,
    the lists test_qbvh_build checks structurally): 100k random rays from inside and outside the
    cloud, closest hits bitwise the oracle's linear HittableList scan."""
    b = O.mixed_list_desc(n, seed=31 + n, spread=12.0)
    d = b.desc()
    rays = np.concatenate([_random_rays(50000, -15, 15, seed=n), _random_rays(50000, -60, 60, seed=n + 1)])
    h2, o2 = O.OracleScene(d).intersect(rays)
    with yart.option("world_bvh", 1):
        s = yart.DeviceScene(d)
        assert s.info().world_nodes > 0
        h, o = s.intersect(rays)
    assert (o2 >= 0).mean() > 0.025  # 3 % (n = 17) to 32 % (n = 600) of the rays hit
    _hits_equal(h, o, h2, o2)


def test_world_bvh_axis_parallel_and_tiny_direction_rays_match_oracle(dev):
    """The world-BVH walk's slab test leaves an axis unconstrained when the ray's direction has no
    usable f32 reciprocal there (|d| < 1e-20: zero, denormal-small or tiny components). Rays of the
    random scene (its 4-wide world BVH) with one or two such components, aimed through the sphere
    field: closest hits bitwise the oracle's linear HittableList scan."""
    p = yart.Preset("random-scene")
    s = yart.DeviceScene(p.desc)
    assert s.info().world_nodes > 0
    rng = np.random.default_rng(17)
    n = 60000
    o = np.column_stack([rng.uniform(-12, 12, n), rng.uniform(0.05, 1.5, n), rng.uniform(-12, 12, n)])
    d = rng.normal(size=(n, 3))
    small = np.array([0.0, -0.0, 1e-30, -1e-25, 5e-324, 1e-21, 2e-20])
    for j in range(3):  # zero / tiny components on one axis (then two) for blocks of the rays
        pick = rng.random(n) < 0.35
        d[pick, j] = rng.choice(small, pick.sum())
    keep = np.abs(d).max(axis=1) > 1e-3  # at least one usable component
    o, d = o[keep], d[keep]
    rays = np.concatenate([o, d, np.full((len(o), 1), 0.001), np.full((len(o), 1), np.inf)], axis=1)
    h, ob = s.intersect(rays)
    h2, o2 = O.OracleScene(p.desc).intersect(rays)
    assert (o2 >= 0).mean() > 0.2
    _hits_equal(h, ob, h2, o2)


def test_world_bvh_far_origins_and_near_overflow_slab_constants_match_oracle(dev):
    """The walk's per-ray slab constants, -(o + m)/d and (m - o)/d, reach |o| |1/d|: a ray whose
    constants could overflow f32 (|o| |1/d| > 1e37) takes the list walk, one below that walks the
    tree on huge constants. Rays from origins 10^3 .. 10^30 away, aimed at points of the sphere
    field, a third of them with one direction component cut to 1e-19 .. 1e-12 (the target kept on
    the ray): both sides of the cut-off, bitwise the oracle's linear HittableList scan."""
    p = yart.Preset("random-scene")
    s = yart.DeviceScene(p.desc)
    assert s.info().world_nodes > 0
    rng = np.random.default_rng(23)
    n = 40000
    tgt = np.column_stack([rng.uniform(-11, 11, n), rng.uniform(0.0, 1.2, n), rng.uniform(-11, 11, n)])
    u = rng.normal(size=(n, 3))
    u /= np.linalg.norm(u, axis=1)[:, None]
    far = 10.0 ** rng.uniform(3, 30, n)
    d = u * far[:, None]
    o = tgt - d
    pick = rng.random(n) < 0.35
    ax = rng.integers(0, 3, n)
    tiny = rng.choice([1e-19, -3e-18, 5e-16, -1e-12], n)
    rows = np.nonzero(pick)[0]
    d[rows, ax[rows]] = tiny[rows]
    o[rows, ax[rows]] = tgt[rows, ax[rows]] - tiny[rows]
    big = np.abs(o).max(axis=1) / np.maximum(np.abs(d), 1e-20).min(axis=1)
    assert (big > 1e37).sum() > 1000 and ((big < 1e37) & pick).sum() > 1000  # both walks exercised
    rays = np.concatenate([o, d, np.full((n, 1), 0.001), np.full((n, 1), np.inf)], axis=1)
    h, ob = s.intersect(rays)
    h2, o2 = O.OracleScene(p.desc).intersect(rays)
    assert (o2 >= 0).mean() > 0.2
    _hits_equal(h, ob, h2, o2)


def test_world_bvh_of_a_large_clustered_list_matches_linear_scan(dev):
    """65,536 clustered spheres (oracle_lib.big_sphere_desc), a list whose SAH tree
    the area collapse made too deep for the walk's stack — the scene used to lose its BVH. Now it
    keeps one (the median-split fallback of world_bvh.cpp), and closest hits of rays aimed at the
    spheres are bitwise the oracle's linear HittableList scan."""
    d, keep = O.big_sphere_desc(1 << 16, seed=7, clustered=True)
    rng = np.random.default_rng(5)
    objs = np.frombuffer(keep[0], dtype=np.uint8).reshape(1 << 16, C.sizeof(abi.Object))
    cent = objs[:, abi.Object.p.offset:abi.Object.p.offset + 24].copy().view(np.float64)
    n = 4000
    o = rng.uniform(-1100, 1100, (n, 3))
    tgt = cent[rng.integers(0, len(cent), n)] + rng.normal(0, 1e-3, (n, 3))
    rays = np.concatenate([o, tgt - o, np.full((n, 1), 0.001), np.full((n, 1), np.inf)], axis=1)
    s = yart.DeviceScene(d)
    assert s.info().world_nodes > 0
    h, ob = s.intersect(rays)
    h2, o2 = O.OracleScene(d).intersect(rays)
    assert (o2 >= 0).mean() > 0.2
    _hits_equal(h, ob, h2, o2)
    del keep


@pytest.mark.parametrize("world_bvh", [0, 1])
def test_mixed_shaded_lists_render_like_the_oracle(dev, world_bvh):
    """Renders of random mixed lists with every list material (Lambertian, checker, fuzzy metal,
    glass, emitters), RotateY at random angles on spheres, rects, triangles and boxes, Translate,
    FlipFace, and a rect + sphere light list: the linear list kernel (world_bvh = 0) and the
    4-wide world BVH (1), bitwise the oracle's frame (the same Philox stream)."""
    b = O.mixed_list_desc(48, seed=77, spread=8.0, shaded=True)
    b.background = (0.3, 0.4, 0.5)
    d = b.desc()
    W, H, spp = 40, 30, 8
    cam = yart.make_camera((0.0, 2.0, 30.0), (0.0, 0.0, 0.0), 45.0, W / H, 0.05, 10.0)
    with yart.option("world_bvh", world_bvh):
        s = yart.DeviceScene(d)
        assert (s.info().world_nodes > 0) == (world_bvh == 1)
        img = s.render(cam, yart.render_params(W, H, spp, 20))
    ref = O.OracleScene(d).render(cam, yart.render_params(W, H, spp, 20))
    assert np.isfinite(ref).all() and ref.mean() > 0.0
    np.testing.assert_array_equal(img, ref)


def test_mixed_shaded_lists_with_extended_features_render_like_the_oracle(dev):
    """The EXT kernel on a random mixed list: the shaded list above plus noise-textured spheres (all
    five noise types, some under RotateY), an image-textured box and triangle under RotateY, a
    rotated ConstantMedium box with an isotropic phase function, and moving spheres (which put the
    shutter-time draw in every camera ray): the frame bitwise the oracle's."""
    b = O.mixed_list_desc(36, seed=78, spread=8.0, shaded=True)
    b.background = (0.2, 0.3, 0.4)
    rng = np.random.default_rng(79)
    img = rng.integers(0, 256, (16, 24, 3), dtype=np.uint8)
    imat = b.material(abi.MAT_LAMBERTIAN, b.image_texture(img))
    for k in range(5):
        nm = b.material(abi.MAT_LAMBERTIAN, b.noise_texture(k, float(rng.uniform(0.5, 4.0)), seed=80 + k))
        c = tuple(float(x) for x in rng.uniform(-6, 6, 3))
        xf = [(abi.XF_ROTATE_Y, (float(rng.uniform(-180, 180)), 0.0, 0.0))] if k % 2 else []
        b.obj(abi.PRIM_SPHERE, nm, c + (float(rng.uniform(0.8, 2.0)),), xforms=xf)
    rot = (abi.XF_ROTATE_Y, (float(rng.uniform(-180, 180)), 0.0, 0.0))
    b.obj(abi.PRIM_BOX, imat, (-1.0, -1.0, -1.0, 1.0, 2.0, 1.5), xforms=[(abi.XF_TRANSLATE, (3.0, 0.0, -2.0)), rot])
    v = rng.uniform(-3, 3, 9)
    b.obj(abi.PRIM_TRIANGLE, imat, tuple(float(x) for x in v) + (0.0, 1.0, 0.0) * 3 + (0.0, 0.0, 1.0, 0.0, 0.0, 1.0),
          xforms=[rot])
    fog = b.material(abi.MAT_ISOTROPIC, b.texture((0.8, 0.8, 0.9)))
    b.obj(abi.PRIM_BOX, fog, (-2.0, -2.0, -2.0, 2.0, 2.0, 2.0),
          xforms=[(abi.XF_MEDIUM, (0.2, 0.0, 0.0)), (abi.XF_TRANSLATE, (-3.0, 1.0, 1.0)), rot])
    red = b.material(abi.MAT_LAMBERTIAN, b.texture((0.7, 0.3, 0.1)))
    for k in range(3):
        c0 = (-4.0 + 4.0 * k, 3.0, 2.0)
        b.obj(abi.PRIM_MOVING_SPHERE, red, c0 + (c0[0], 3.5 + 0.5 * k, 2.0, 0.0, 1.0, 0.6))
    d = b.desc()
    W, H, spp = 40, 30, 8
    cam = yart.make_camera((0.0, 2.0, 30.0), (0.0, 0.0, 0.0), 45.0, W / H, 0.05, 10.0)
    s = yart.DeviceScene(d)
    out = s.render(cam, yart.render_params(W, H, spp, 20))
    ref = O.OracleScene(d).render(cam, yart.render_params(W, H, spp, 20))
    assert np.isfinite(ref).all() and ref.mean() > 0.0
    np.testing.assert_array_equal(out, ref)


def test_world_bvh_ties_go_to_the_later_object(dev):
    """Coincident primitives hit at the same t: the linear scan keeps the LAST one (t == t_max is
    accepted); the BVH must pick the same object whatever order it visits them in."""
    b = O.DescBuilder()
    mats = [b.material(abi.MAT_LAMBERTIAN, b.texture((0.1 * k, 0.5, 0.5))) for k in range(4)]
    rng = np.random.default_rng(5)
    for k in range(12):  # 12 positions x 3 coincident copies each, interleaved in list order
        c = tuple(rng.uniform(-5, 5, 3))
        for m in range(3):
            b.obj(abi.PRIM_SPHERE, mats[m], c + (0.7,))
    for m in range(3):  # three coincident floors, and a box over a rect face
        b.obj(abi.PRIM_XZ_RECT, mats[m], (-8.0, 8.0, -8.0, 8.0, -6.0))
    b.obj(abi.PRIM_BOX, mats[3], (-1.0, -6.0, -1.0, 1.0, -5.0, 1.0))
    b.obj(abi.PRIM_XZ_RECT, mats[2], (-1.0, 1.0, -1.0, 1.0, -5.0))
    d = b.desc()
    rays = _random_rays(60000, -9, 9, seed=17)
    h2, o2 = O.OracleScene(d).intersect(rays)
    for force in (1, 0):
        with yart.option("world_bvh", force):
            s = yart.DeviceScene(d)
            assert (s.info().world_nodes > 0) == (force == 1)
            h, o = s.intersect(rays)
        assert (o2 >= 0).mean() > 0.15
        _hits_equal(h, o, h2, o2)


def test_world_bvh_sphere_leaves_beside_wrapped_and_hollow_spheres(dev):
    """Leaves of plain spheres take the compact-record walk (kWorldLeafSpheres); spheres under a
    Translate, hollow (negative-radius) spheres and a rect share the list, so some leaves mix the
    two paths. Closest hits and a render stay bitwise the linear scan's."""
    b = O.DescBuilder()
    mats = [b.material(abi.MAT_LAMBERTIAN, b.texture((0.2 * k, 0.4, 0.6))) for k in range(3)]
    glass = b.material(abi.MAT_DIELECTRIC, b=(1.04, 0.23, 1.01), c=(0.006, 0.02, 103.56))
    rng = np.random.default_rng(23)
    for k in range(60):
        c = tuple(rng.uniform(-6, 6, 3))
        r = float(rng.uniform(0.2, 0.9))
        if k % 5 == 1:
            b.obj(abi.PRIM_SPHERE, mats[k % 3], (0.0, 0.0, 0.0, r), xforms=[(abi.XF_TRANSLATE, c)])
        elif k % 7 == 2:
            b.obj(abi.PRIM_SPHERE, glass, c + (-r,))  # hollow: the radius is negative
        else:
            b.obj(abi.PRIM_SPHERE, mats[k % 3], c + (r,))
    b.obj(abi.PRIM_XZ_RECT, mats[1], (-7.0, 7.0, -7.0, 7.0, -6.5))
    b.obj(abi.PRIM_SPHERE, mats[0], (0.0, 2.0, 0.0, 1.5), light=True)
    b.obj(abi.PRIM_SPHERE, b.material(abi.MAT_DIFFUSE_LIGHT, b.texture((8.0, 8.0, 8.0))), (0.0, 9.0, 0.0, 1.5))
    d = b.desc()
    rays = _random_rays(60000, -8, 8, seed=29)
    h2, o2 = O.OracleScene(d).intersect(rays)
    with yart.option("world_bvh", 1):
        s = yart.DeviceScene(d)
        assert s.info().world_nodes > 0
        h, o = s.intersect(rays)
        assert (o2 >= 0).mean() > 0.15
        _hits_equal(h, o, h2, o2)
        W, H, spp = 40, 32, 4
        cam = yart.make_camera((0.0, 3.0, 16.0), (0.0, 0.0, 0.0), 40.0, W / H, 0.0, 10.0)
        np.testing.assert_array_equal(s.render(cam, yart.render_params(W, H, spp, 50)),
                                      O.OracleScene(d).render(cam, yart.render_params(W, H, spp, 50)))


def test_moving_spheres_match_oracle(dev):
    """MovingSphere + the shutter-time draw it switches on (camera.rs:91), with a glass one."""
    from test_scene_features import moving_scene
    b = moving_scene()
    d = b.desc()
    W, H = 48, 32
    cam = yart.make_camera((0.0, 2.0, 12.0), (0.0, 1.0, 0.0), 40.0, W / H, 0.1, 10.0)
    s = yart.DeviceScene(d)
    np.testing.assert_array_equal(s.render(cam, yart.render_params(W, H, 8, 50)),
                                  O.OracleScene(d).render(cam, yart.render_params(W, H, 8, 50)))
    rays = _random_rays(50000, -6, 6, seed=19)
    h, o = s.intersect(rays)
    h2, o2 = O.OracleScene(d).intersect(rays)
    _hits_equal(h, o, h2, o2)


@pytest.mark.parametrize("lookfrom,lookat", [((0.0, 278.0, -800.0), (0.0, 278.0, 0.0)),     # origin.x == 0
                                             ((278.0, 278.0, -800.0), (278.0, 278.0, 0.0)),  # the preset's
                                             ((278.0, 0.0, -800.0), (278.0, 0.0, 555.0))])   # origin.y == 0
def test_pinhole_camera_shortcut_is_exact(dev, lookfrom, lookat):
    """Aperture 0 without shutter time: k_render skips random_in_unit_disk (its draws and its ±0
    offset cannot reach the ray) unless an origin or direction component is zero, where the full
    camera.rs:82-94 path runs (a zero origin component sends every ray there). Both branches must
    equal the oracle, which always runs the loop."""
    p = yart.Preset("cornell-box")
    W, H = 41, 33
    cam = yart.make_camera(lookfrom, lookat, 40.0, W / H, 0.0, 10.0)
    prm = yart.render_params(W, H, 3, 50)
    s = yart.DeviceScene(p.desc)
    np.testing.assert_array_equal(s.render(cam, prm), O.OracleScene(p.desc).render(cam, prm))


def test_scene_info_matches_reference_qbvh(dev):
    p = yart.Preset("david")
    s = yart.DeviceScene(p)
    i = s.info()
    assert (i.bvh_nodes, i.bvh_leaves, i.bvh_max_depth) == (5461, 16384, 7)  # one shared BLAS for both instances
    assert i.n_meshes == 1 and i.n_objects == 7 and i.n_lights == 5


RENDER_CASES = [
    # scene, W, H, spp, depth
    ("cornell-box", 64, 64, 16, 50),
    ("cornell-box", 37, 29, 5, 50),     # ragged: W, H not multiples of 8 -> uncovered crop rows/cols
    ("two-spheres", 100, 56, 8, 8),     # C1 at reduced size (checker texture, no lights)
    ("random-scene", 60, 40, 4, 50),    # C3 at reduced size (metal / negative albedo / glass)
    ("three-spheres", 40, 40, 4, 50),   # negative-radius spheres
    ("bunny", 40, 40, 4, 50),           # C4 (stand-in mesh) at reduced size
    ("david", 48, 27, 2, 50),           # C5 at reduced size (2 mesh instances)
    ("cornell-box", 16, 16, 3, 1),      # depth 1: every path ends at `depth == 0 -> 1.0`
    ("two-perlin-spheres", 40, 24, 4, 50),  # NoiseTexture (Perlin marble), no lights
    ("simple-light", 40, 24, 32, 50),       # + an XY-rect emitter (dark: more samples)
    ("cornell-box-smoke", 32, 32, 4, 50),   # ConstantMedium + Isotropic (free-path draws, stream 2)
    ("earth", 48, 24, 4, 50),               # ImageTexture: sphere uv (acos, atan2) + texel spectra
]


@pytest.mark.parametrize("scene,W,H,spp,depth", RENDER_CASES)
def test_render_bitwise_equal_to_oracle(dev, scene, W, H, spp, depth):
    p = yart.Preset(scene)
    cam = p.camera(W, H)
    prm = yart.render_params(W, H, spp, depth)
    gpu = yart.DeviceScene(p.desc).render(cam, prm)
    cpu = O.OracleScene(p.desc).render(cam, prm, threads=0)
    assert np.isfinite(gpu).all()
    np.testing.assert_array_equal(gpu, cpu)
    cov = O.coverage(W, H)
    assert (gpu[~cov] == 0).all()
    assert (gpu[cov].sum(axis=-1) != 0).mean() > 0.05


@pytest.mark.parametrize("scene,spu", [("cornell-box", 1), ("cornell-box", 3), ("cornell-box", 7), ("david", 2),
                                       ("random-scene", 5), ("cornell-box-smoke", 3)])
def test_chunked_samples_bitwise_equal_to_sequential_sum(dev, scene, spu):
    """samples_per_unit < spp: per-sample values go through HBM and k_accumulate adds them in
    sample order; the sums must not change (main.rs:707's sequential +=)."""
    p = yart.Preset(scene)
    W, H, spp = 40, 24, 8
    cam = p.camera(W, H)
    s = yart.DeviceScene(p)
    fused = s.render(cam, yart.render_params(W, H, spp, 50, samples_per_unit=spp))  # one unit per block
    chunked = s.render(cam, yart.render_params(W, H, spp, 50, samples_per_unit=spu))
    np.testing.assert_array_equal(chunked, fused)
    np.testing.assert_array_equal(chunked, O.OracleScene(p.desc).render(cam, yart.render_params(W, H, spp, 50)))


def test_chunked_multi_pass_and_shards(dev, opt):
    """A scratch budget of a few samples forces several accumulate passes; with shards too."""
    p = yart.Preset("cornell-box")
    W, H, spp = 48, 40, 10
    cam = p.camera(W, H)
    s = yart.DeviceScene(p)
    ref = O.OracleScene(p.desc).render(cam, yart.render_params(W, H, spp, 50))
    opt("scratch_bytes", 3 * 48 * 64 * 24)  # 3 samples x (48/8*40/8 blocks)
    parts = [s.render(cam, yart.render_params(W, H, spp, 50, shard_index=i, shard_count=2, samples_per_unit=1))
             for i in range(2)]
    np.testing.assert_array_equal(parts[0] + parts[1], ref)


def test_overlapped_scratch_passes_back_to_back(dev, opt):
    """A frame larger than the scratch budget renders in overlapped passes (capi.cpp launch_frame):
    the odd passes render on a helper stream into the scratch's second half and the accumulates run
    in pass order on another. Frames enqueued back to back on one stream, with halves of 1, 2 and 3
    samples (several passes each, the mesh frame's overflow regions doubled too) and one frame in a
    single pass between them, must equal their one-pass renders bit for bit."""
    import torch
    st = torch.cuda.current_stream()
    for scene, W, H, spps in [("cornell-box", 48, 40, [7, 5, 9, 6, 4]), ("bunny", 40, 32, [5, 4, 7])]:
        p = yart.Preset(scene)
        cam = p.camera(W, H)
        s = yart.DeviceScene(p)
        per = ((W + 7) // 8) * ((H + 7) // 8) * 64 * 24
        refs = [s.render(cam, yart.render_params(W, H, n, 50)) for n in spps]
        outs = [torch.zeros((H, W, 3), dtype=torch.float64, device="cuda:0") for _ in spps]
        for k, (n, out) in enumerate(zip(spps, outs)):
            opt("scratch_bytes", per * 64 if k == 3 else per * 2 * (k % 3 + 1))
            s.render_async(cam, yart.render_params(W, H, n, 50, samples_per_unit=1), out.data_ptr(), st.cuda_stream)
        torch.cuda.synchronize()
        for k, (out, ref) in enumerate(zip(outs, refs)):
            np.testing.assert_array_equal(out.cpu().numpy(), ref, err_msg=f"{scene} frame {k}")
    assert (refs[0][O.coverage(W, H)].sum(axis=-1) != 0).mean() > 0.05


def test_scratch_pass_shrinks_when_the_device_is_nearly_full(dev):
    """The auto scratch budget (min(16 GiB, device memory / 8), capi.cpp scratch_budget) is sized
    from the device's total memory, not what is free. With all but ~1.5 GB of the device held by
    another allocation, a 1920x1080x64 frame (3.2 GB of sample scratch in one pass) cannot get
    its pass: pass_scratch halves it until the allocation fits (64 -> 32 -> 16 samples), and the
    frame is bitwise the one rendered 8 samples per pass with the device free. The hold goes
    through the HIP runtime libyart uses: opened by soname, dlopen returns the copy already
    loaded (torch's, when torch was imported first; /opt/rocm's otherwise)."""
    hip = C.CDLL("libamdhip64.so.7")
    hip.hipMalloc.argtypes = [C.POINTER(C.c_void_p), C.c_size_t]
    hip.hipFree.argtypes = [C.c_void_p]
    hip.hipMemGetInfo.argtypes = [C.POINTER(C.c_size_t), C.POINTER(C.c_size_t)]
    p = yart.Preset("cornell-box")
    W, H, spp = 1920, 1080, 64
    cam = p.camera(W, H)
    prm = yart.render_params(W, H, spp, 50)
    with yart.option("scratch_bytes", 8 * ((W + 7) // 8) * ((H + 7) // 8) * 64 * 24):
        ref = yart.DeviceScene(p).render(cam, prm)
    s = yart.DeviceScene(p)
    free, total = C.c_size_t(), C.c_size_t()
    assert hip.hipMemGetInfo(C.byref(free), C.byref(total)) == 0
    hold = C.c_void_p()
    assert hip.hipMalloc(C.byref(hold), max(1, free.value - (3 << 29))) == 0
    try:
        assert hip.hipMemGetInfo(C.byref(free), C.byref(total)) == 0
        assert free.value < 3 << 30  # the one-pass scratch cannot fit
        got = s.render(cam, prm)
    finally:
        assert hip.hipFree(hold) == 0
    np.testing.assert_array_equal(got, ref)
    assert (got[O.coverage(W, H)].sum(axis=-1) != 0).mean() > 0.5


def test_sample_scratch_regrows_between_frames_on_one_stream(dev):
    """Chunked frames (samples_per_unit = 2) enqueued back to back on one stream: 16x16x4, then
    48x40x8 (the stream's sample scratch grows, after the stream drained), then 16x16x4 again in the
    larger scratch. Each frame bitwise its render on a fresh scene handle; the three frames' timing
    events were handed over to the scene and are read (and recycled) by yart_frame_timing."""
    import torch
    p = yart.Preset("cornell-box")
    s = yart.DeviceScene(p)
    st = torch.cuda.current_stream()
    shapes = [(16, 16, 4), (48, 40, 8), (16, 16, 4)]
    outs = []
    for W, H, spp in shapes:
        out = torch.full((H, W, 3), float("nan"), dtype=torch.float64, device="cuda:0")
        s.render_async(p.camera(W, H), yart.render_params(W, H, spp, 50, samples_per_unit=2), out.data_ptr(), st.cuda_stream)
        outs.append(out)
    torch.cuda.synchronize()
    for (W, H, spp), out in zip(shapes, outs):
        ref = yart.DeviceScene(p).render(p.camera(W, H), yart.render_params(W, H, spp, 50, samples_per_unit=2))
        np.testing.assert_array_equal(out.cpu().numpy(), ref, err_msg=f"{W}x{H}x{spp}")
    assert (outs[1].cpu().numpy()[O.coverage(48, 40)].sum(axis=-1) != 0).mean() > 0.05  # not a frame of zeros
    r, a, n = s.frame_timing(st.cuda_stream)
    assert n == 3 and r > 0 and a > 0
    assert s.frame_timing(st.cuda_stream)[2] == 0  # read once


def test_auto_chunking_at_full_device_scale(dev):
    """A small frame on a 256-CU device is auto-split into sample chunks; still bitwise."""
    p = yart.Preset("cornell-box")
    W, H, spp = 64, 64, 64
    cam = p.camera(W, H)
    g = yart.DeviceScene(p).render(cam, yart.render_params(W, H, spp, 50))
    np.testing.assert_array_equal(g, O.OracleScene(p.desc).render(cam, yart.render_params(W, H, spp, 50)))


def test_shards_partition_the_frame(dev):
    p = yart.Preset("cornell-box")
    W, H, spp = 72, 48, 4
    cam = p.camera(W, H)
    s = yart.DeviceScene(p.desc)
    full = s.render(cam, yart.render_params(W, H, spp, 50))
    parts = [s.render(cam, yart.render_params(W, H, spp, 50, shard_index=i, shard_count=3)) for i in range(3)]
    nz = [(q.sum(axis=-1) != 0) for q in parts]
    assert not (nz[0] & nz[1]).any() and not (nz[1] & nz[2]).any() and not (nz[0] & nz[2]).any()
    np.testing.assert_array_equal(parts[0] + parts[1] + parts[2], full)


@pytest.mark.parametrize("scene,W,H,spp,depth", [("bunny", 40, 40, 4, 50), ("david", 48, 27, 2, 50), ("david", 24, 16, 3, 1),
                                                 ("david", 16, 16, 2, 0)])
def test_wavefront_and_megakernel_agree(dev, scene, W, H, spp, depth, opt):
    """The wavefront path (k_wf_shade / k_wf_trace; option mesh_wavefront = 1 — until r04 the default
    for meshes deeper than depth 10) must give the megakernel's bits (mesh_wavefront = 0) and the oracle's: with
    the default pool, with a 256-path pool (hundreds of iterations, every path slot regenerated
    many times), and over several scratch passes."""
    p = yart.Preset(scene)
    cam = p.camera(W, H)
    prm = yart.render_params(W, H, spp, depth)
    opt("mesh_wavefront", 1)
    wf = yart.DeviceScene(p).render(cam, prm)
    opt("wf_pool", 256)
    small = yart.DeviceScene(p).render(cam, prm)
    opt("scratch_bytes", ((W + 7) // 8) * ((H + 7) // 8) * 64 * 24)  # one sample per pass
    passes = yart.DeviceScene(p).render(cam, prm)
    opt("mesh_wavefront", 0)
    mega = yart.DeviceScene(p).render(cam, prm)
    np.testing.assert_array_equal(wf, mega)
    np.testing.assert_array_equal(small, mega)
    np.testing.assert_array_equal(passes, mega)
    if depth > 0:
        np.testing.assert_array_equal(wf, O.OracleScene(p.desc).render(cam, prm, threads=0))
    assert (wf[O.coverage(W, H)].sum(axis=-1) != 0).mean() > 0.05


def _deep_grid(n=1450):
    """A height-field grid of 2 (n - 1)^2 = 4,199,202 triangles: more than 4 * 4^10, so the
    reference's median-split L4QBVH is 11 levels deep and its walk needs 34 stack entries."""
    xs = np.linspace(-1.0, 1.0, n)
    X, Z = np.meshgrid(xs, xs, indexing="xy")
    Y = 0.05 * np.sin(7.0 * X) * np.cos(5.0 * Z)
    P = np.stack([X, Y, Z], -1).astype(np.float32)
    a, b, c, d = P[:-1, :-1], P[:-1, 1:], P[1:, :-1], P[1:, 1:]
    pos = np.ascontiguousarray(np.concatenate([np.concatenate([a, c, b], -1).reshape(-1, 9),
                                               np.concatenate([b, c, d], -1).reshape(-1, 9)], 0))
    v = pos.astype(np.float64).reshape(-1, 3, 3)
    cr = np.cross(v[:, 1] - v[:, 0], v[:, 2] - v[:, 0])
    nrm = cr / np.sqrt((cr * cr).sum(-1, keepdims=True))
    return pos, np.ascontiguousarray(np.repeat(nrm, 3, axis=0).reshape(-1, 9))


def test_mesh_instances_at_random_angles_match_oracle(dev, repo):
    """Six instances of the sycee stand-in mesh under RotateY at random angles (and Translate, one
    under FlipFace), diffuse, metal and glass, with a sphere light: closest hits of 60k rays aimed
    at the instances and a small render, bitwise the oracle's. The instances' sin / cos come from
    the host (one sincos each, test_rotate_y_uses_the_oracles_sincos); the walk runs on the
    rotated local rays."""
    pos, nrm = yart.load_obj(repo / "assets" / "sycee.obj")
    b = O.DescBuilder(background=(0.5, 0.6, 0.7))
    mats = [b.material(abi.MAT_LAMBERTIAN, b.texture((0.7, 0.6, 0.5))),
            b.material(abi.MAT_METAL, b.texture((0.9, 0.9, 0.8)), fuzz=0.1),
            b.material(abi.MAT_DIELECTRIC, 0, b=(1.62153902, 0.256287842, 1.64447552),
                       c=(0.0122241457e6, 0.0595736775e6, 147.468793e6))]
    li = b.material(abi.MAT_DIFFUSE_LIGHT, b.texture((6.0, 6.0, 6.0)))
    b.mesh(pos, nrm)
    rng = np.random.default_rng(91)
    centres = []
    for k in range(6):
        c = (float(rng.uniform(-6, 6)), float(rng.uniform(-1, 1)), float(rng.uniform(-6, 6)))
        centres.append(c)
        xf = [(abi.XF_TRANSLATE, c), (abi.XF_ROTATE_Y, (float(rng.uniform(-180, 180)), 0.0, 0.0))]
        if k == 5:
            xf = [(abi.XF_FLIP_FACE, (0.0, 0.0, 0.0))] + xf
        b.obj(abi.PRIM_MESH, mats[k % 3], mesh=0, xforms=xf)
    b.obj(abi.PRIM_SPHERE, li, (0.0, 9.0, 0.0, 2.0))
    b.obj(abi.PRIM_SPHERE, li, (0.0, 9.0, 0.0, 2.0), light=True)
    d = b.desc()
    n = 60000
    org = rng.uniform(-12, 12, (n, 3))
    tgt = np.array(centres)[rng.integers(0, 6, n)] + rng.normal(scale=1.0, size=(n, 3))
    rays = np.column_stack([org, tgt - org, np.full(n, 0.001), np.full(n, np.inf)])
    s = yart.DeviceScene(d)
    h, o = s.intersect(rays)
    h2, o2 = O.OracleScene(d).intersect(rays)
    assert (o2 >= 0).mean() > 0.2
    _hits_equal(h, o, h2, o2)
    W, H, spp = 32, 24, 4
    cam = yart.make_camera((0.0, 4.0, 18.0), (0.0, 0.0, 0.0), 50.0, W / H, 0.0, 10.0)
    np.testing.assert_array_equal(s.render(cam, yart.render_params(W, H, spp, 16)),
                                  O.OracleScene(d).render(cam, yart.render_params(W, H, spp, 16)))


@pytest.mark.parametrize("n,layout", [(17, "soup"), (65, "soup"), (1000, "soup"), (30000, "soup"),
                                      (3000, "geometric"), (600, "coincident")])
def test_walk_tree_of_triangle_soups_matches_oracle(dev, n, layout):
    """r05: the front-to-back walk's tree is collapsed from a binary SAH tree by dynamic programming
    (walk_tree.cpp), with unusual shapes on unusual inputs: random soups of awkward sizes, triangles
    along a geometric progression (the most unbalanced cuts) and coincident triangles (every cut a
    tie). Closest hits of rays aimed at the triangles, bitwise the oracle's (the reference's walk)."""
    rng = np.random.default_rng(1000 + n)
    if layout == "soup":
        c = rng.uniform(-5, 5, (n, 1, 3))
    elif layout == "geometric":
        c = np.zeros((n, 1, 3))
        c[:, 0, 0] = 1.01 ** np.arange(n) - 1.0
    else:
        c = np.zeros((n, 1, 3))
    v = c + rng.normal(0, 0.3, (n, 3, 3))
    pos = v.astype(np.float32).reshape(n, 9)
    pv = pos.reshape(n, 3, 3).astype(np.float64)
    fn = np.cross(pv[:, 1] - pv[:, 0], pv[:, 2] - pv[:, 0])
    fn /= np.maximum(np.linalg.norm(fn, axis=1), 1e-30)[:, None]
    nrm = np.repeat(fn[:, None, :], 3, axis=1).reshape(n, 9)
    b = O.DescBuilder(background=(0.5, 0.6, 0.7))
    m = b.material(abi.MAT_LAMBERTIAN, b.texture((0.6, 0.6, 0.6)))
    b.mesh(pos, nrm)
    b.obj(abi.PRIM_MESH, m, mesh=0)
    d = b.desc()
    k = 20000
    cen = pv.mean(axis=1)
    org = cen[rng.integers(0, n, k)] + rng.normal(0, 3.0, (k, 3))
    tgt = cen[rng.integers(0, n, k)] + rng.normal(0, 0.05, (k, 3))
    rays = np.column_stack([org, tgt - org, np.full(k, 0.001), np.full(k, np.inf)])
    s = yart.DeviceScene(d)
    h, o = s.intersect(rays)
    h2, o2 = O.OracleScene(d).intersect(rays)
    assert (o2 >= 0).mean() > 0.2
    _hits_equal(h, o, h2, o2)


@pytest.mark.parametrize("wavefront", [0, 1])
def test_deep_mesh_walks_with_the_references_64_slot_stack(dev, wavefront):
    """A mesh deeper than depth 10 (VERDICT r02 Missing #3, r04 Missing #3): the reference walks it
    with its 64-entry stack (qbvh.rs:382-384). Since r05 the megakernel does too (wavefront = 0, the
    default): 32 stack entries in LDS, the rest in HBM; the wavefront trace kernel's 64-slot LDS walk
    is the forced alternative (mesh_wavefront = 1). Closest hits and a small render bitwise vs the
    oracle on both, and the work counters (the instrumented megakernel) on a deep mesh."""
    pos, nrm = _deep_grid()
    b = O.DescBuilder(background=(0.7, 0.8, 1.0))
    w = b.material(abi.MAT_LAMBERTIAN, b.texture((0.6, 0.5, 0.4)))
    g = b.material(abi.MAT_DIELECTRIC, 0, b=(1.62153902, 0.256287842, 1.64447552),
                   c=(0.0122241457e6, 0.0595736775e6, 147.468793e6))
    li = b.material(abi.MAT_DIFFUSE_LIGHT, b.texture((4.0, 4.0, 4.0)))
    b.mesh(pos, nrm)
    b.obj(abi.PRIM_MESH, w, mesh=0)
    b.obj(abi.PRIM_MESH, g, mesh=0, xforms=[(abi.XF_TRANSLATE, (0.0, 0.3, 0.0))])
    b.obj(abi.PRIM_SPHERE, li, (0.0, 2.0, 0.0, 0.5))
    b.obj(abi.PRIM_SPHERE, li, (0.0, 2.0, 0.0, 0.5), light=True)
    desc = b.desc()
    with yart.option("mesh_wavefront", 1 if wavefront else -1):
        s = yart.DeviceScene(desc)
    i = s.info()
    assert i.bvh_max_depth == 11 and i.bvh_max_stack == 34
    o = O.OracleScene(desc)
    assert o.qbvh_stats(0) == (i.bvh_nodes, i.bvh_leaves, 11)
    rng = np.random.default_rng(3)
    n = 20000
    org = np.column_stack([rng.uniform(-1.2, 1.2, n), rng.uniform(0.5, 2.0, n), rng.uniform(-1.2, 1.2, n)])
    tgt = np.column_stack([rng.uniform(-1.0, 1.0, n), rng.uniform(-0.1, 0.4, n), rng.uniform(-1.0, 1.0, n)])
    rays = np.column_stack([org, tgt - org, np.full(n, 0.001), np.full(n, np.inf)])
    gh, go = s.intersect(rays)
    oh, oo = o.intersect(rays)
    np.testing.assert_array_equal(go, oo)
    np.testing.assert_array_equal(gh, oh)
    assert (go >= 0).mean() > 0.9
    cam = yart.make_camera((0.3, 1.5, 2.0), (0.0, 0.0, 0.0), 40.0, 1.0, 0.0)
    prm = yart.render_params(24, 24, 2, 8)
    img = s.render(cam, prm)
    want = o.render(cam, prm, threads=0)
    np.testing.assert_array_equal(img, want)
    assert (img[O.coverage(24, 24)].sum(axis=-1) != 0).mean() > 0.5
    # the chunked (persistent-wave) plan too, and the instrumented kernel (on the same plan)
    np.testing.assert_array_equal(s.render(cam, yart.render_params(24, 24, 2, 8, samples_per_unit=1)), want)
    img2, st = s.render_with_stats(cam, prm)
    np.testing.assert_array_equal(img2, want)
    assert st.samples == 24 * 24 * 2 and st.node_visits > 0


def test_finalize_matches_oracle(dev):
    p = yart.Preset("cornell-box")
    W, H, spp = 96, 64, 8
    xyz = O.OracleScene(p.desc).render(p.camera(W, H), yart.render_params(W, H, spp, 50))
    g = yart.finalize_rgba8(xyz, spp)
    c = O.finalize(xyz, spp)
    np.testing.assert_array_equal(g, c)
    # bright, dark, negative and non-finite sums too (sanitize is upstream; finalize must still agree)
    rng = np.random.default_rng(9)
    wild = rng.normal(0.0, 1.0, (64, 96, 3)) * 10.0 ** rng.uniform(-6, 6, (64, 96, 1)) * spp
    wild[0, :4] = [[np.nan, 0, 0], [np.inf, -np.inf, 0], [0, 0, 0], [-0.0, 1e308, -1e308]]
    with np.errstate(all="ignore"):
        np.testing.assert_array_equal(yart.finalize_rgba8(wild, spp), O.finalize(wild, spp))


def test_device_byte_map_matches_reference_around_every_step(dev):
    """k_finalize's srgb_byte (probe op 11) on every double within 512 ulps of each of the 255
    steps and of the 0.0031308 branch edge, against the oracle's glibc-pow chain."""
    from test_finalize_bytes import steps
    centres = np.concatenate([steps(), [0.0031308]]).view(np.int64)
    win = (centres[:, None] + np.arange(-512, 513, dtype=np.int64)[None, :]).ravel().view(np.float64)
    rng = np.random.default_rng(10)
    with np.errstate(all="ignore"):
        win = np.concatenate([win, rng.uniform(-0.1, 1.2, 200000), 10.0 ** rng.uniform(-320, 308, 50000),
                              [np.nan, np.inf, -np.inf, 0.0, -0.0]])
        got = _probe(dev, 11, win)
        np.testing.assert_array_equal(got, O.display_bytes(win).astype(np.float64))


def test_errors_are_reported_not_raised(dev):
    b = O.DescBuilder()
    m = b.material(abi.MAT_LAMBERTIAN, b.texture((0.5, 0.5, 0.5)))
    b.mesh(np.zeros((3, 9), dtype=np.float32), np.zeros((3, 9)))  # <= 4 triangles: reference panics
    b.obj(abi.PRIM_MESH, m, mesh=0)
    with pytest.raises(yart.YartError) as e:
        yart.DeviceScene(b.desc())
    assert e.value.code == abi.ERR_UNSUPPORTED
    b2 = O.DescBuilder()
    b2.obj(abi.PRIM_SPHERE, 3, (0, 0, 0, 1))  # material index out of range
    with pytest.raises(yart.YartError) as e:
        yart.DeviceScene(b2.desc())
    assert e.value.code == abi.ERR_INVALID


def _mesh_triangles(p, k=0):
    """(n, 3, 3) f64 vertices of mesh k of a preset (the exact f32 values tobj parsed)."""
    m = p.desc.contents.meshes[k]
    n = int(m.n_triangles)
    return np.ctypeslib.as_array(m.positions, shape=(n * 9,)).reshape(n, 3, 3).astype(np.float64)


def _near_coplanar_rays(tris, n, seed, reach):
    """Rays that run within 1e-15 .. 1e-12 rad of a triangle's plane (and some exactly in it, up to
    rounding) and pass through that triangle's interior, arriving from `reach` units away: the
    case where Moller-Trumbore's t loses all its digits (condition number 1 / |cos theta|) and the
    front-to-back walk's pruning margin (2^-8 relative, kernels.hip qbvh_coop) is not a bound."""
    rng = np.random.default_rng(seed)
    k = rng.integers(0, len(tris), n)
    v0, e1, e2 = tris[k, 0], tris[k, 1] - tris[k, 0], tris[k, 2] - tris[k, 0]
    nrm = np.cross(e1, e2)
    ln = np.linalg.norm(nrm, axis=1, keepdims=True)
    ok = ln[:, 0] > 0
    nrm = np.where(ok[:, None], nrm / np.where(ln > 0, ln, 1.0), np.array([0.0, 1.0, 0.0]))
    a, b = rng.uniform(0, 1, n), rng.uniform(0, 1, n)
    f = a + b > 1
    a[f], b[f] = 1 - a[f], 1 - b[f]
    X = v0 + a[:, None] * e1 + b[:, None] * e2
    g = rng.normal(size=(n, 3))
    u = g - (g * nrm).sum(1, keepdims=True) * nrm
    u /= np.linalg.norm(u, axis=1, keepdims=True)
    tilt = 10.0 ** rng.uniform(-15, -12, n) * rng.choice([-1.0, 1.0], n)
    tilt[rng.uniform(0, 1, n) < 0.1] = 0.0
    d = u * np.cos(tilt)[:, None] + nrm * np.sin(tilt)[:, None]
    d *= 10.0 ** rng.uniform(-1, 1, n)[:, None]  # the renderer's rays are not unit length
    o = X - rng.uniform(0.05, 1.0, n)[:, None] * reach * d / np.linalg.norm(d, axis=1, keepdims=True)
    return np.concatenate([o, d, np.full((n, 1), 0.001), np.full((n, 1), np.inf)], axis=1)


@pytest.mark.parametrize("scene,reach", [("david", 120.0), ("sycee", 3.0)])
def test_mesh_walk_near_coplanar_rays_match_oracle(dev, scene, reach):
    """200k rays grazing a triangle of the mesh within 1e-15 .. 1e-12 rad of
    its plane, through its interior, from up to `reach` units away (most of them cross other parts
    of the mesh first), against the oracle (qbvh.rs:381-543's order with the running t_max).

    * The reference-order walk (option YART_OPT_MESH_WALK_REF = 1): bitwise on every ray.
    * The default front-to-back walk: bitwise on every ray but those where the reference's own
      answer is a Moller-Trumbore artifact — a triangle at |a| within a few ulps of the reference's
      f64::EPSILON threshold whose t lies OUTSIDE that triangle's own bounding box (measured on
      david: 60 of 200,000 rays, t = 32.0 for a triangle whose box spans [53.5, 55.1], and the like).
      The reference reaches such a triangle only because its visiting order had not yet lowered
      t_max past the box; the front-to-back walk prunes the box beyond its nearer geometric hit.
      Each differing ray is checked here to be exactly that (numpy MT in the reference's operation
      order, tests/mt_numpy.py), with the device answer the later one; any other difference fails."""
    p = yart.Preset(scene)
    rays = _near_coplanar_rays(_mesh_triangles(p), 200000, seed=41, reach=reach)
    h2, o2 = O.OracleScene(p.desc).intersect(rays)
    assert (o2 >= 0).mean() > 0.5
    with yart.option("mesh_walk_ref", 1):
        s = yart.DeviceScene(p)
        h, o = s.intersect(rays)
    _hits_equal(h, o, h2, o2)
    s = yart.DeviceScene(p)
    h, o = s.intersect(rays)
    bad = np.flatnonzero((o != o2) | ((o2 >= 0) & np.any(_bits(h) != _bits(h2), axis=1)))
    assert len(bad) <= len(rays) // 1000, len(bad)
    desc = p.desc.contents
    for i in bad:
        assert o2[i] >= 0 and (o[i] < 0 or h[i, 0] > h2[i, 0]), (i, o[i], h[i, 0], o2[i], h2[i, 0])
        tris = MT.answer_outside_own_box(desc, rays[i], int(o2[i]), h2[i, 0])
        assert tris, i
        for tri, a, entry, exit_ in tris:
            assert abs(a) < 1e-12 and not (entry <= h2[i, 0] <= exit_), (i, tri, a, entry, exit_, h2[i, 0])


_STACK = []


def _layer_stack():
    """(builder, desc, oracle scene) of the stacked-layers mesh, built once per session."""
    if not _STACK:
        n = 5 * 4 ** 10 + 64  # > 4 triangles under every level-10 node: every leaf at depth 11
        x = (np.arange(n) * 1e-3).astype(np.float32)
        pos = np.zeros((n, 9), np.float32)
        pos[:, 0::3] = x[:, None]
        pos[:, [1, 2, 5, 7]] = -1.0
        pos[:, [4, 8]] = 3.0
        nrm = np.zeros((n, 9))
        nrm[:, 0::3] = 1.0
        b = O.DescBuilder(background=(0.7, 0.8, 1.0))
        m = b.material(abi.MAT_LAMBERTIAN, b.texture((0.6, 0.5, 0.4)))
        b.mesh(pos, nrm)
        b.obj(abi.PRIM_MESH, m, mesh=0)
        d = b.desc()
        _STACK.append((b, d, O.OracleScene(d)))
    return _STACK[0]


@pytest.mark.parametrize("rewalk", [0, 1])
def test_parked_mesh_walks_are_exact(dev, rewalk):
    """Parked walks (YART_OPT_MESH_PARK, kernels.hip qbvh_coop PARK): in a one-mesh scene on the
    persistent plan, a walk whose wave has no new rays left and at most 8 busy quads stops, and its
    quad picks it up at the next iteration, next to the new rays. The bunny frame parks walks
    (parked_walks > 0) and renders bitwise the oracle's frame and the frame with parking off; under
    yart_debug_force_rewalk the re-walks (their stacks in the wave's HBM region while other walks
    are parked) are exact too."""
    p = yart.Preset("bunny")
    W, H, spp = 96, 72, 8
    cam, prm = p.camera(W, H), yart.render_params(W, H, spp, 50)
    ref = O.OracleScene(p.desc).render(cam, prm, threads=0)
    assert dev.yart_debug_force_rewalk(0, rewalk) == 0
    try:
        s = yart.DeviceScene(p.desc)
        img, st = s.render_with_stats(cam, prm)
        plain = s.render(cam, prm)
        with yart.option("mesh_park", 0):
            off, st_off = yart.DeviceScene(p.desc).render_with_stats(cam, prm)
    finally:
        assert dev.yart_debug_force_rewalk(0, 0) == 0
    assert st.parked_walks > 0 and st_off.parked_walks == 0
    if rewalk:
        assert st.mesh_rewalks > 0
    np.testing.assert_array_equal(img, ref)
    np.testing.assert_array_equal(plain, ref)
    np.testing.assert_array_equal(off, ref)


@pytest.mark.parametrize("walk", ["default", "reference_order", "lane_rewalk"])
def test_deep_mesh_overflow_stack_is_used_and_exact(dev, walk):
    """the megakernel's deep-mesh walks keep their first kStackSlots = 32 stack
    entries in LDS and the rest in the per-wave HBM region (OVF) — exercised here, not assumed.
    5,242,944 parallel triangles stacked along x (one per layer, every layer covering the same
    y-z square): the reference's median-split L4QBVH has every leaf at depth 11 (more than 4
    triangles under every level-10 node) and every box of a level spans the square, so a ray along
    -x through the square hits all four children at every level, and a descent that defers three
    of them per level pushes 33 entries: slot 32 lives in HBM.
    Measured (tools/ovf_probe.py, profiles/r06f_ovf_probe.log): the default front-to-back walk on its
    depth-11 walk tree pushes one entry per ray into the region (the cooperative walk's per-quad node
    ids and 16-bit entries), and so does the per-lane reference-order re-walk (force_rewalk: per-lane
    columns); the instrumented render counts those pushes (yart_render_stats.ovf_pushes > 0). The
    cooperative walk in the reference's order (mesh_walk_ref = 1) visits the whole tree on these rays
    without reaching slot 32. Production and instrumented renders, and a
    ray batch, bitwise the oracle's in all three."""
    b, d, o = _layer_stack()
    with yart.option("mesh_walk_ref", 1 if walk == "reference_order" else 0):
        s = yart.DeviceScene(d)
    i = s.info()
    assert i.bvh_max_depth == 11 and i.bvh_max_stack >= 33
    # small on purpose: on this mesh the reference's own walk order is far to near along x, so a
    # reference-order walk visits most of the tree (~0.13 s per ray on the oracle)
    cam = yart.make_camera((5400.0, 0.4, 0.4), (0.0, 0.4, 0.4), 0.02, 1.0, 0.0)
    prm = yart.render_params(8, 8, 1, 2)
    want = o.render(cam, prm, threads=0)
    if walk == "lane_rewalk":
        assert dev.yart_debug_force_rewalk(0, 1) == 0
    try:
        img, st = s.render_with_stats(cam, prm)
        np.testing.assert_array_equal(img, want)
        np.testing.assert_array_equal(s.render(cam, prm), want)
    finally:
        assert dev.yart_debug_force_rewalk(0, 0) == 0
    if walk != "reference_order":
        assert st.ovf_pushes > 0, "the HBM overflow stack was never written"
    assert (img[O.coverage(8, 8)].sum(axis=-1) != 0).mean() > 0.5
    rng = np.random.default_rng(8)
    k = 48
    org = np.column_stack([np.full(k, 5500.0), rng.uniform(-0.5, 0.9, k), rng.uniform(-0.5, 0.9, k)])
    dirs = np.column_stack([-np.ones(k), rng.normal(0, 1e-5, k), rng.normal(0, 1e-5, k)])
    rays = np.column_stack([org, dirs, np.full(k, 0.001), np.full(k, np.inf)])
    gh, go = s.intersect(rays)
    oh, oo = o.intersect(rays)
    _hits_equal(gh, go, oh, oo)
    assert (go >= 0).all()
