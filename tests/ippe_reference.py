"""An independent checker of one square-marker IPPE pose -- TEST INFRASTRUCTURE ONLY, numpy float64, nothing shared with oracle/init_oracle.cpp
or csrc/ippe_vote.hpp.  It is the defining-equation check of tests/test_initializer.py
(test_oracle_ippe_satisfies_the_defining_equations_of_ippe), lifted into a function and vectorised over detections.

IPPE (Collins & Bartoli, IJCV 2014) is defined by two equations.  With H the homography marker plane -> normalised image (DLT by SVD; exact for
four corners), v = H(0, 0) and J the 2x2 Jacobian of H at the origin:
  (1) rotation:     [I2 | -v] R[:, :2] = gamma J with gamma > 0, for BOTH returned rotations;
  (2) translation:  t is the linear least-squares solution of the four corners' projection equations, given R.
On top of those, check() measures what a pose that satisfies neither can still hide from: the distance of R from a rotation, and the float64
reprojection error e64 of the matrix AS STORED, to be held against the float error the kernel reports for the matrix before it was stored.

The corners are normalised exactly as the kernel does it (d_undistort4): double arithmetic in the kernel's order, five fixed-point iterations
of the inverse distortion model, rounded to float.
"""
from types import SimpleNamespace

import numpy as np


def model_corners(marker_size):
    """[4, 2] float64: the corner order of aruco::Marker, half side rounded to float as the kernel's hf"""
    h = float(np.float32(marker_size) / np.float32(2.0))
    return np.array([[-h, h], [h, h], [h, -h], [-h, -h]])


def normalise(K, dist, uv):
    """q [n, 4, 2] float64 holding float32 values: the kernel's normalised corners of the raw float32 pixel corners uv [n, 8]"""
    K = np.asarray(K, dtype=np.float64).reshape(3, 3)
    k = np.zeros(12)
    d = np.asarray(dist, dtype=np.float64).reshape(-1)
    k[:len(d)] = d
    uv = np.asarray(uv, dtype=np.float32).astype(np.float64).reshape(-1, 4, 2)
    ifx, ify = 1.0 / K[0, 0], 1.0 / K[1, 1]
    x0, y0 = (uv[..., 0] - K[0, 2]) * ifx, (uv[..., 1] - K[1, 2]) * ify
    x, y = x0, y0
    for _ in range(5):
        r2 = x * x + y * y
        icdist = (1.0 + ((k[7] * r2 + k[6]) * r2 + k[5]) * r2) / (1.0 + ((k[4] * r2 + k[1]) * r2 + k[0]) * r2)
        dx = 2.0 * k[2] * x * y + k[3] * (r2 + 2.0 * x * x) + k[8] * r2 + k[9] * r2 * r2
        dy = k[2] * (r2 + 2.0 * y * y) + 2.0 * k[3] * x * y + k[10] * r2 + k[11] * r2 * r2
        x, y = (x0 - dx) * icdist, (y0 - dy) * icdist
    return np.stack([x, y], axis=-1).astype(np.float32).astype(np.float64)


def homography(model, q):
    """H [n, 3, 3], H[2, 2] = 1: DLT rows of q ~ H (x, y, 1) for the four corners, null vector by SVD"""
    n = len(q)
    A = np.zeros((n, 8, 9))
    for c, (x, y) in enumerate(model):
        a, b = q[:, c, 0], q[:, c, 1]
        A[:, 2 * c, 0:3] = [x, y, 1]
        A[:, 2 * c, 6], A[:, 2 * c, 7], A[:, 2 * c, 8] = -a * x, -a * y, -a
        A[:, 2 * c + 1, 3:6] = [x, y, 1]
        A[:, 2 * c + 1, 6], A[:, 2 * c + 1, 7], A[:, 2 * c + 1, 8] = -b * x, -b * y, -b
    # columns scaled to unit norm first: the marker's coordinates (centimetres) and the constant column differ by orders of magnitude
    s = np.linalg.norm(A, axis=1, keepdims=True)
    h = np.linalg.svd(A / s)[2][:, -1, :] / s[:, 0, :]
    H = h.reshape(n, 3, 3)
    return H / H[:, 2:3, 2:3]


def reprojection_error(model, q, T):
    """sum over the corners of |proj(R X + t) - q| [n], float64"""
    X = np.concatenate([model, np.zeros((4, 1))], axis=1)
    P = np.einsum("nij,cj->nci", T[:, :3, :3], X) + T[:, None, :3, 3]
    return np.linalg.norm(P[..., :2] / P[..., 2:3] - q, axis=-1).sum(axis=1)


def check(marker_size, q, T):
    """marker_size; q [n, 4, 2] from normalise(); T [n, 4, 4] returned poses (either solution).  Returns arrays [n]:
         gamma     of equation (1); must be > 0
         rot       max |G - gamma I| / gamma with G = [I2 | -v] R[:, :2] J^-1
         trans     max |t - t_ls| / max |t_ls|, t_ls by an SVD least-squares solve
         ortho     max |R R^T - I|
         det       |det R - 1|
         e64       float64 reprojection error of the stored matrix
         last_row  max |T[3] - (0, 0, 0, 1)|
       Non-finite input gives non-finite (never small) output."""
    q = np.asarray(q, dtype=np.float64).reshape(-1, 4, 2)
    T = np.asarray(T, dtype=np.float64).reshape(-1, 4, 4)
    model = model_corners(marker_size)
    n = len(q)
    bad = ~np.isfinite(T).all(axis=(1, 2))
    Tw = np.where(bad[:, None, None], np.eye(4), T)                  # (so that the batched SVDs run; the results are overwritten below)
    H = homography(model, q)
    v = H[:, :2, 2]
    J = H[:, :2, :2] - v[:, :, None] * H[:, 2:3, :2]
    R, t = Tw[:, :3, :3], Tw[:, :3, 3]
    M = R[:, :2, :2] - v[:, :, None] * R[:, 2:3, :2]
    G = M @ np.linalg.inv(J)
    gamma = 0.5 * (G[:, 0, 0] + G[:, 1, 1])
    with np.errstate(divide="ignore", invalid="ignore"):
        rot = np.abs(G - gamma[:, None, None] * np.eye(2)).max(axis=(1, 2)) / gamma
    # (R X + t)_xy = q (R X + t)_z, eight rows in t
    X = np.concatenate([model, np.zeros((4, 1))], axis=1)
    RX = np.einsum("nij,cj->nci", R, X)
    A = np.zeros((n, 8, 3)); b = np.zeros((n, 8))
    A[:, 0::2, 0] = 1; A[:, 0::2, 2] = -q[:, :, 0]
    A[:, 1::2, 1] = 1; A[:, 1::2, 2] = -q[:, :, 1]
    b[:, 0::2] = q[:, :, 0] * RX[:, :, 2] - RX[:, :, 0]
    b[:, 1::2] = q[:, :, 1] * RX[:, :, 2] - RX[:, :, 1]
    t_ls = (np.linalg.pinv(A) @ b[:, :, None])[:, :, 0]
    with np.errstate(divide="ignore", invalid="ignore"):
        trans = np.abs(t - t_ls).max(axis=1) / np.abs(t_ls).max(axis=1)
    ortho = np.abs(R @ R.transpose(0, 2, 1) - np.eye(3)).max(axis=(1, 2))
    det = np.abs(np.linalg.det(R) - 1)
    with np.errstate(divide="ignore", invalid="ignore"):
        e64 = reprojection_error(model, q, Tw)
    last = np.abs(Tw[:, 3] - np.array([0, 0, 0, 1.0])).max(axis=1)
    out = SimpleNamespace(gamma=gamma, rot=rot, trans=trans, ortho=ortho, det=det, e64=e64, last_row=last)
    for k in vars(out):
        getattr(out, k)[bad] = np.nan
    return out


ORTHO_BAR = 1e-6        # a float-rounded rotation: tests/test_initializer.py's bar (test_oracle_ippe_recovers_exact_planar_poses)
ERR_BAR = 1e-6          # |e - e64|: the float chain sums four terms of magnitude <~ 0.5 (6e-8 each) and t is rounded to float


def failures(marker_size, q, T, e, resid_bar):
    """the indices at which a pose with reported float error e misses the checker: list of (index, what, value)"""
    r = check(marker_size, q, T)
    e = np.asarray(e, dtype=np.float64)
    out = []
    for name, val, bar in (("rot", r.rot, resid_bar), ("trans", r.trans, resid_bar), ("ortho", r.ortho, ORTHO_BAR), ("det", r.det, ORTHO_BAR),
                           ("last_row", r.last_row, 0.0), ("e-e64", np.abs(e - r.e64), ERR_BAR)):
        for i in np.nonzero(~(val <= bar))[0]:
            out.append((int(i), name, float(val[i])))
    for i in np.nonzero(~(r.gamma > 0))[0]:
        out.append((int(i), "gamma", float(r.gamma[i])))
    return out
