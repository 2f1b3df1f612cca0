"""Seeded inputs of the IPPE edge certificates (tests/test_ippe_reference_host.py, tests/test_gpu_ippe_edges.py) -- TEST INFRASTRUCTURE ONLY.
Built once per session (functools.lru_cache), never modified by a test.

Every family is a set of noise-free detections of one 0.05 m marker by the camera K = (900, 900, 640, 360), 1280 x 720: the true marker ->
camera transforms and their corners projected in float64 and rounded to float32, all four inside the image.  A marker that faces the camera
has its z axis towards it, so a fronto-parallel ("head-on") pose is a rotation by exactly pi about an axis in the image plane.

    fronto       head-on, random in-plane angle and position, 15 to 150 pixels
    integer      axis-aligned squares on integer pixels (rendered data) in the four corner orders, a tenth of them centred on the principal point
    near_pi      pi - delta about an in-plane axis, delta log-uniform in [1e-9, 1e-2]
    on_axis      the centre exactly on the principal point: in-plane rotated squares whose pixel offsets are multiples of 1/8 (exactly symmetric
                 floats: p = q = 0 in d_ippe_square), and tilted poses with t = (0, 0, z) (p, q at rounding level)
    one_axis     the centre on one axis only: integer squares on the principal column (p = 0 exactly, q != 0) and row (the reverse), and
                 tilted poses with t_x = 0 or t_y = 0
    generic      tilted 0-60 degrees against the viewing ray
    oblique      60-85 degrees
    grazing      85-89 degrees
    small        5-pixel markers (9 m), tilted 0-60
    large        200-pixel markers (0.225 m), tilted 0-60
    far          20 m away (2.25 pixels), tilted 0-60

Bars.  RESID is the project's own bar on the two defining equations (tests/test_initializer.py), for every family but `grazing`, where J^-1
amplifies the float rounding of the stored rotation: its bar, and every family's bar on |T1 - truth| (set by the conditioning of the pose in
the float-rounded corners, so per family), is the worst value of the oracle (oracle/init_oracle.cpp, this CPU's libm) over the family as
generated here, times 4 for libm and seed variation, rounded up to two digits.  The measured worsts stand beside the bars.  The distorted
variant (corners through the forward model with DIST5, undone by the kernel's five fixed-point iterations, which do not converge to float
accuracy) has bars of its own, measured the same way.
"""
import functools
from types import SimpleNamespace

import numpy as np

import aar

MS = 0.05
K = np.array([[900.0, 0, 640.0], [0, 900.0, 360.0], [0, 0, 1.0]])
SIZE = (1280, 720)
N = 500
RESID = 2e-5
DELTA0 = 1e-3                                   # the seam of the pi guard: c0 = DELTA0^2 / 2 = 5e-7 in d_store_pose / rt_matrix_f32

#   family            bar on the residuals (worst)      bar on |T1 - truth| (worst)    the same with DIST5 (worst)
BARS = {
    "fronto":   dict(resid_bar=RESID,                truth_bar=1.6e-3,  # 3.878e-4
                     truth_bar_dist=6.1e-4),                            # 1.507e-4
    "integer":  dict(resid_bar=RESID,                truth_bar=4.8e-5,  # 1.192e-5
                     truth_bar_dist=8.6e-3),                            # 2.134e-3
    "near_pi":  dict(resid_bar=RESID,                truth_bar=1.5e-4,  # 3.524e-5
                     truth_bar_dist=1.6e-4),                            # 3.771e-5
    "on_axis":  dict(resid_bar=RESID,                truth_bar=8.6e-3,  # 2.140e-3
                     truth_bar_dist=1.1e-2),                            # 2.725e-3
    "one_axis": dict(resid_bar=RESID,                truth_bar=8.5e-4,  # 2.120e-4
                     truth_bar_dist=1.6e-3),                            # 3.911e-4
    "generic":  dict(resid_bar=RESID,                truth_bar=1.2e-3,  # 2.920e-4
                     truth_bar_dist=1.2e-3),                            # 2.956e-4
    "oblique":  dict(resid_bar=RESID,                truth_bar=4.5e-5,  # 1.121e-5
                     truth_bar_dist=6.2e-5),                            # 1.528e-5
    "grazing":  dict(resid_bar=6.0e-6,               truth_bar=8.1e-6,  # residual 1.37e-6 (1.49e-6 with DIST5); truth 2.007e-6
                     truth_bar_dist=8.5e-6),                            # 2.122e-6
    "small":    dict(resid_bar=RESID,                truth_bar=1.7e-2,  # 4.146e-3
                     truth_bar_dist=1.2e-2),                            # 2.765e-3
    "large":    dict(resid_bar=RESID,                truth_bar=2.2e-4,  # 5.301e-5
                     truth_bar_dist=2.3e-4),                            # 5.698e-5
    "far":      dict(resid_bar=RESID,                truth_bar=8.5e-2,  # 2.106e-2
                     truth_bar_dist=8.6e-2),                            # 2.130e-2
}
# (over the other ten families the oracle's worst residual is 3.1e-7, in `oblique`: RESID is not what limits them.  In `on_axis`, `small` and `far`
# the two solutions all but coincide and a few detections, 1, 1 and 3 of 500, put the reflected one first: they are in the worsts above.)
SEAM_TRUTH = 9.0e-5     # both sides of the pi guard's seam: 2.234e-5 on the guarded side, 2.150e-5 on the other (the conditioning of a pose 1e-3 off head-on)
BOARD_TRUTH = 7.6e-6    # the board scene through the oracle's whole Initializer: 1.890e-6 (a marker), 1.42e-6 (camera 1), 1.24e-6 (a frame)
FAMILIES = tuple(BARS)


# ---- rotations, in plain numpy ----
def axis_angle(axis, angle):
    a = np.asarray(axis, dtype=np.float64)
    a = a / np.linalg.norm(a)
    S = np.array([[0, -a[2], a[1]], [a[2], 0, -a[0]], [-a[1], a[0], 0]])
    return np.cos(angle) * np.eye(3) + (1 - np.cos(angle)) * np.outer(a, a) + np.sin(angle) * S


def face(phi):
    """the half turn about the in-plane axis (cos phi, sin phi, 0): the marker looks back at the camera, turned in the plane by 2 phi"""
    a = np.array([np.cos(phi), np.sin(phi), 0.0])
    return 2 * np.outer(a, a) - np.eye(3)


def to_ray(t):
    """the rotation that takes the optical axis onto the ray through t"""
    d = np.asarray(t, dtype=np.float64) / np.linalg.norm(t)
    ax = np.cross([0, 0, 1.0], d)
    s = np.linalg.norm(ax)
    return np.eye(3) if s < 1e-300 else axis_angle(ax, np.arctan2(s, d[2]))


def rigid(R, t):
    T = np.eye(4)
    T[:3, :3] = R
    T[:3, 3] = t
    return T


def corners(T, Kc=K, ms=MS):
    """float64 pixel corners [4, 2] of the marker at T, aruco's corner order"""
    h = ms / 2
    X = np.array([[-h, h, 0, 1], [h, h, 0, 1], [h, -h, 0, 1], [-h, -h, 0, 1.0]]).T
    P = Kc @ (T @ X)[:3]
    return (P[:2] / P[2]).T


def visible(uv, margin=2.0):
    return bool(np.all(uv[:, 0] > margin) and np.all(uv[:, 0] < SIZE[0] - margin) and np.all(uv[:, 1] > margin) and np.all(uv[:, 1] < SIZE[1] - margin))


def _family(name, poses):
    T = np.array(poses)
    uv = np.array([corners(t) for t in T])
    assert len(T) <= N and all(visible(c) for c in uv), name
    return SimpleNamespace(name=name, truth=T, uv=uv.reshape(-1, 8).astype(np.float32), **BARS[name])


def _centre(rng, z, margin):
    u, v = rng.uniform(margin, SIZE[0] - margin), rng.uniform(margin, SIZE[1] - margin)
    return z * np.array([(u - K[0, 2]) / K[0, 0], (v - K[1, 2]) / K[1, 1], 1.0])


def _tilted(rng, n, tilt_deg, depth, margin=40, centre=None):
    """n visible poses tilted by an angle in tilt_deg against the viewing ray, about a random in-plane axis"""
    out = []
    while len(out) < n:
        z = rng.uniform(*depth)
        t = _centre(rng, z, margin) if centre is None else centre(rng, z)
        alpha = np.deg2rad(rng.uniform(*tilt_deg))
        ax = rng.uniform(0, 2 * np.pi)
        T = rigid(to_ray(t) @ axis_angle([np.cos(ax), np.sin(ax), 0], alpha) @ face(rng.uniform(0, np.pi)), t)
        if visible(corners(T)):
            out.append(T)
    return out


def _integer_square(u, v, s, turn):
    """the square with half side s pixels centred on pixel (u, v), its corner order turned by `turn` quarter turns: corners and true pose"""
    z = K[0, 0] * (MS / 2) / s
    R = face(0.0) @ axis_angle([0, 0, 1.0], turn * np.pi / 2)
    R = np.round(R)                                              # quarter turns: entries are exactly 0 and +-1
    return rigid(R, z * np.array([(u - K[0, 2]) / K[0, 0], (v - K[1, 2]) / K[1, 1], 1.0]))


@functools.lru_cache(maxsize=None)
def family(name):
    rng = np.random.default_rng(sum(map(ord, name)) + 20240)
    if name == "fronto":
        out = []
        while len(out) < N:
            z = rng.uniform(0.3, 3.0)
            T = rigid(face(rng.uniform(0, np.pi)), _centre(rng, z, 40))
            if visible(corners(T)):
                out.append(T)
        return _family(name, out)
    if name == "integer":
        out = []
        for i in range(N):
            s = int(rng.integers(3, 100))
            u, v = int(rng.integers(s + 3, SIZE[0] - s - 3)), int(rng.integers(s + 3, SIZE[1] - s - 3))
            if i % 10 == 0:
                u, v = 640, 360
            out.append(_integer_square(u, v, s, i % 4))
        f = _family(name, out)
        assert np.array_equal(f.uv, np.round(f.uv))
        return f
    if name == "near_pi":
        out = []
        while len(out) < N:
            delta = 10 ** rng.uniform(-9, -2)
            ax = rng.uniform(0, 2 * np.pi)
            T = rigid(axis_angle([np.cos(ax), np.sin(ax), 0], np.pi - delta), _centre(rng, rng.uniform(0.3, 3.0), 40))
            if visible(corners(T)):
                out.append(T)
        return _family(name, out)
    if name == "on_axis":
        out, exact = [], []
        for i in range(N // 2):
            # exact: face(phi) = [[c, s], [s, -c]] (c, s of 2 phi) takes corner 1 (h, h) to the pixel offset (a, b) and the others to
            # (b, -a), (-b, a), (-a, -b); a, b in eighths of a pixel, so the float corners are symmetric about the principal point
            a, b = rng.integers(8, 800, 2) / 8.0
            z = K[0, 0] * (MS / 2) * np.sqrt(2) / np.hypot(a, b)
            out.append(rigid(face(0.5 * np.arctan2(a + b, a - b)), [0, 0, z]))
            exact.append(np.array([[b, -a], [a, b], [-b, a], [-a, -b]]) + K[:2, 2])
        out += _tilted(rng, N - len(out), (0, 70), (0.3, 3.0), centre=lambda rng, z: np.array([0, 0, z]))
        f = _family(name, out)
        exact = np.array(exact).reshape(-1, 8)
        assert np.abs(np.array([corners(T) for T in f.truth[:N // 2]]).reshape(-1, 8) - exact).max() < 1e-9
        f.uv[:N // 2] = exact.astype(np.float32)
        assert np.array_equal(f.uv[:N // 2], exact)
        return f
    if name == "one_axis":
        out = []
        for i in range(N // 2):
            s = int(rng.integers(3, 100))
            if i % 2:
                out.append(_integer_square(640, int(rng.integers(s + 3, SIZE[1] - s - 3)), s, i % 4))
            else:
                out.append(_integer_square(int(rng.integers(s + 3, SIZE[0] - s - 3)), 360, s, i % 4))
        k = [0]

        def centre(rng, z):
            k[0] += 1
            c = _centre(rng, z, 60)
            c[k[0] % 2] = 0.0
            return c
        out += _tilted(rng, N - len(out), (0, 70), (0.3, 3.0), centre=centre)
        f = _family(name, out)
        assert not np.any(np.all(f.truth[:, :2, 3] == 0, axis=1))
        return f
    if name == "generic":
        return _family(name, _tilted(rng, N, (0, 60), (0.3, 3.0)))
    if name == "oblique":
        return _family(name, _tilted(rng, N, (60, 85), (0.3, 3.0)))
    if name == "grazing":
        return _family(name, _tilted(rng, N, (85, 89), (0.3, 1.0)))
    if name == "small":
        return _family(name, _tilted(rng, N, (0, 60), (9.0, 9.0), margin=10))
    if name == "large":
        return _family(name, _tilted(rng, N, (0, 60), (0.225, 0.225), margin=150))
    if name == "far":
        return _family(name, _tilted(rng, N, (0, 60), (20.0, 20.0), margin=10))
    raise KeyError(name)


def regular(n):
    """n ordinary detections (the generic family, cycled): the lanes that sit beside the edge cases in a wavefront"""
    g = family("generic")
    idx = np.arange(n) % N
    return g.uv[idx], g.truth[idx]


LAUNCH_SHAPES = (1, 63, 64, 65, 130)             # one detection, one short of a wavefront, a wavefront, one more, two and a partial third


def interleaved(f, n, start=0):
    """a launch of n detections, the family's (from index `start` on) on the even places and ordinary ones on the odd, so that a guard lane sits
    beside an ordinary one in a wavefront: (uv [n, 8], truth [n, 4, 4], edge mask [n])"""
    ne = (n + 1) // 2
    assert start + ne <= len(f.uv)
    uv = np.zeros((n, 8), dtype=np.float32); T = np.zeros((n, 4, 4)); edge = np.arange(n) % 2 == 0
    ruv, rT = regular(n - ne)
    uv[edge], T[edge] = f.uv[start:start + ne], f.truth[start:start + ne]
    uv[~edge], T[~edge] = ruv, rT
    return uv, T, edge


# ---- the seam of the pi guard ----
@functools.lru_cache(maxsize=None)
def seam():
    """groups of four true poses pi - delta about the same in-plane axis at the same place, delta = 0.9, 0.999, 1.001 and 1.1 times DELTA0:
    (truth [n, 4, 4], uv [n, 8], guarded [n]: the side of the seam the TRUE rotation is on).  The rotation IPPE recovers from the float corners
    differs from the true one by up to the conditioning of a head-on pose (SEAM_TRUTH), so a case may be stored by the other branch than its
    truth suggests; the set as a whole sits on the seam and feeds both."""
    rng = np.random.default_rng(77)
    T, g = [], []
    while len(T) < 200:
        ax = rng.uniform(0, 2 * np.pi)
        t = _centre(rng, rng.uniform(0.3, 3.0), 40)
        for f in (0.9, 0.999, 1.001, 1.1):
            T.append(rigid(axis_angle([np.cos(ax), np.sin(ax), 0], np.pi - f * DELTA0), t))
            g.append(f < 1)
        if not all(visible(corners(x)) for x in T[-4:]):
            del T[-4:], g[-4:]
    T = np.array(T)
    return T, np.array([corners(x) for x in T]).reshape(-1, 8).astype(np.float32), np.array(g)


# ---- the board scene ----
@functools.lru_cache(maxsize=None)
def board():
    """2 cameras, 6 coplanar markers at 0.1 m pitch, 5 frames, 60 detections.  Camera 0 looks straight at the board from 0.9 m in every frame
    (the board slides and turns in its own plane), camera 1 sees it from the side.  Returns det (aar.Detections), Ks, dists, and the true
    transforms in the Initializer's gauge (root camera 0, root marker 0): T_cam [2], T_marker [6], T_object [5], and per detection T_det."""
    Ks = np.array([K, K])
    dists = [np.zeros(5)] * 2
    T_marker = np.array([rigid(np.eye(3), [0.1 * (m % 3), 0.1 * (m // 3), 0.0]) for m in range(6)])
    eye1 = np.array([0.75, 0.05, 0.0])                                         # camera 1 in camera 0's frame, looking at the board's middle
    z1 = np.array([0.0, 0.0, 0.9]) - eye1
    z1 /= np.linalg.norm(z1)
    x1 = np.cross([0, 1.0, 0], z1); x1 /= np.linalg.norm(x1)
    T_cam = np.array([np.eye(4), rigid(np.array([x1, np.cross(z1, x1), z1]).T, eye1)])
    T_object = []
    for f in range(5):
        R = face(0.05 + 0.11 * f)                                              # head-on to camera 0: a half turn about an in-plane axis
        c = np.array([0.02 * f - 0.04, 0.015 * f - 0.03, 0.9])                 # where the board's middle (0.1, 0.05, 0) goes
        T_object.append(rigid(R, c - R @ np.array([0.1, 0.05, 0.0])))
    T_object = np.array(T_object)
    fr, cam, mk, uv, Td = [], [], [], [], []
    for f in range(5):
        for c in range(2):
            for m in range(6):
                T = np.linalg.inv(T_cam[c]) @ T_object[f] @ T_marker[m]
                p = corners(T)
                assert visible(p) and T[2, 3] > 0
                fr.append(f); cam.append(c); mk.append(m); uv.append(p.reshape(8)); Td.append(T)
    det = aar.Detections(2, 5, np.array(fr, dtype=np.int32), np.array(cam, dtype=np.int32), np.array(mk, dtype=np.int32),
                         np.array(uv).astype(np.float32))
    return SimpleNamespace(det=det, Ks=Ks, dists=dists, ms=MS, T_cam=T_cam, T_marker=T_marker, T_object=T_object, T_det=np.array(Td),
                           truth_bar=BOARD_TRUTH)


# ---- the distorted variant ----
DIST5 = np.array([-0.11, 0.085, 0.0012, -0.0007, -0.019])


@functools.lru_cache(maxsize=None)
def distorted(name):
    """the family's corners through the forward distortion model (fp64), rounded to float32: what d_undistort4 has to undo"""
    import oracle_lib as O
    f = family(name)
    return O.distort_points(K, DIST5, f.uv.astype(np.float64).reshape(-1, 2)).reshape(-1, 8).astype(np.float32)


@functools.lru_cache(maxsize=None)
def board_solution():
    """the board scene as a solved map (an aar.Dataset at the truth), for the live tracker: cameras, markers, the five frames and all 60 detections"""
    import oracle_lib as O
    b = board()
    vec = lambda T: np.concatenate([O.rodrigues_mat2vec(T[:3, :3]), T[:3, 3]])
    ds = aar.Dataset()
    ds.num_cams, ds.num_markers, ds.num_frames, ds.root_cam, ds.root_marker = 2, 6, 5, 0, 0
    ds.marker_size = np.float32(MS)
    ds.cam_ids, ds.marker_ids, ds.frame_ids = np.arange(2, dtype=np.int32), np.arange(6, dtype=np.int32), np.arange(5, dtype=np.int32)
    ds.image_sizes = np.array([SIZE, SIZE], dtype=np.int32)
    ds.cam_mats = b.Ks.reshape(2, 9).copy()
    ds.dist_coeffs = np.zeros((2, 5))
    ds.obs_frame, ds.obs_cam, ds.obs_marker, ds.obs_uv = b.det.det_frame, b.det.det_cam, b.det.det_id, b.det.det_uv
    ds.num_obs = len(ds.obs_frame)
    ds.x_full = np.concatenate([vec(b.T_cam[1])] + [vec(T) for T in b.T_marker[1:]] + [vec(T) for T in b.T_object])
    ds.x_truth = ds.x_full.copy()
    ds.optimize_cam_poses = ds.optimize_marker_poses = ds.optimize_object_poses = True
    ds.optimize_cam_intrinsics = False
    return ds
