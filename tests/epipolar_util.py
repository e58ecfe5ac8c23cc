"""What the epipolar-matching tests share (test_epipolar_cpu, test_gpu_epipolar_match): planted two-view geometry and
the numpy float32 restatement of misift_match_epipolar_batch's gate, op by op in the order include/misift.h gives.  A
plain module: no fixtures, no hooks."""
import numpy as np

f32 = np.float32
STEREO = np.array([[0, 0, 0], [0, 0, -1], [0, 1, 0]], f32)        # rectified stereo: the line of (x, y) is y2 = y
STEREO_V = np.array([[0, 0, -1], [0, 0, 0], [1, 0, 0]], f32)      # its vertical counterpart: x2 = x


def planted_F(i, w=1920.0, h=1080.0):
    """F = K^-T [t]x R K^-1 of a planted camera motion (a small rotation and a translation that vary with i), float32,
    in the convention (x2, y2, 1) F (x1, y1, 1)^T = 0."""
    K = np.array([[1.1 * w, 0, w / 2], [0, 1.1 * w, h / 2], [0, 0, 1]])
    ax, ay, az = 0.02 + 0.01 * (i % 3), -0.03 + 0.012 * (i % 5), 0.05 * ((i % 4) - 1.5)
    Rx = np.array([[1, 0, 0], [0, np.cos(ax), -np.sin(ax)], [0, np.sin(ax), np.cos(ax)]])
    Ry = np.array([[np.cos(ay), 0, np.sin(ay)], [0, 1, 0], [-np.sin(ay), 0, np.cos(ay)]])
    Rz = np.array([[np.cos(az), -np.sin(az), 0], [np.sin(az), np.cos(az), 0], [0, 0, 1]])
    t = np.array([1.0, 0.3 * ((i % 3) - 1), 0.2 * ((i % 2) - 0.5)])
    tx = np.array([[0, -t[2], t[1]], [t[2], 0, -t[0]], [-t[1], t[0], 0]])
    Ki = np.linalg.inv(K)
    F = Ki.T @ tx @ (Rz @ Ry @ Rx) @ Ki
    return (F / np.abs(F).max()).astype(f32)


def finite(v):
    return np.abs(v) <= f32(3.402823466e+38)


def lines_np(F, x, y):
    """a0, a1, a2, n2 and ok of the rows (x, y), float32, sums left to right."""
    F = np.asarray(F, f32).reshape(9)
    x, y = np.asarray(x, f32), np.asarray(y, f32)
    with np.errstate(all="ignore"):
        a0 = F[0] * x + F[1] * y + F[2]
        a1 = F[3] * x + F[4] * y + F[5]
        a2 = F[6] * x + F[7] * y + F[8]
        n2 = a0 * a0 + a1 * a1
    return a0, a1, a2, n2, finite(a0) & finite(a1) & finite(a2) & finite(n2)


def gate_np(F, x1, y1, x2, y2, radius):
    """(n1, n2) bool: record j is a candidate of row i."""
    a0, a1, a2, n2, ok = lines_np(F, x1, y1)
    x2, y2 = np.asarray(x2, f32), np.asarray(y2, f32)
    with np.errstate(all="ignore"):
        r2 = f32(radius) * f32(radius)
        e = x2[None, :] * a0[:, None] + y2[None, :] * a1[:, None] + a2[:, None]
        return ok[:, None] & (e * e < (r2 * n2)[:, None])


def points_on_lines(F, x1, y1, rng, across, w=1920.0, h=1080.0):
    """For each row a point of image 2 on its epipolar line (float64 geometry), at a random position along it inside
    the w x h frame where the line crosses it, and `across` (per row) pixels off the line.  Returns x2, y2 (float64)
    and whether the row's line crosses the frame."""
    F = np.asarray(F, np.float64).reshape(3, 3)
    p = np.stack([np.asarray(x1, np.float64), np.asarray(y1, np.float64), np.ones(len(x1))])
    a = F @ p
    n = np.hypot(a[0], a[1])
    n = np.where(n > 0, n, 1.0)
    nx, ny = a[0] / n, a[1] / n                                    # unit normal; direction (-ny, nx)
    # the point of the line nearest the frame centre, then a random step along the line
    d0 = (a[0] * w / 2 + a[1] * h / 2 + a[2]) / n
    cx, cy = w / 2 - d0 * nx, h / 2 - d0 * ny
    s = rng.uniform(-0.45, 0.45, len(n)) * min(w, h)
    x = cx - s * ny + across * nx
    y = cy + s * nx + across * ny
    inside = (x > 0) & (x < w) & (y > 0) & (y < h)
    return x, y, inside
