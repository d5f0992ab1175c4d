"""CPU restatement of the float32 screen of the screened 2-opt (difusco_amd/csrc/two_opt.hip: ``change32``,
``two_opt_screen_kernel``, ``two_opt_screened_best_kernel``) in numpy, every float32 operation rounded where the kernel rounds it.

``c64`` is the change matrix of ``oracle.tsp_decode_oracle.batched_two_opt`` (its formula, restated for one tour).  ``c32`` is the
kernel's float32 value of the same entry: coordinates and edge lengths rounded to float32, float32 subtract, the sum of squares
either as the kernel writes it (one fused multiply-add: evaluated in float64 and rounded once) or as two products and a sum, a
float32 square root (numpy's is correctly rounded; ``sqrt_ulps`` moves every root by that many ulps, the v_sqrt_f32 tolerance),
and the three additions left to right.  ``screened_best`` is the skip rule and the float64 argmin over the survivors."""
import numpy as np

F32 = np.float32


def valid_mask(n):
    return np.triu(np.ones((n, n), dtype=bool), k=2)


def c64_matrix(points, tour):
    """tsp_decode_oracle.batched_two_opt, lines 115-123, for one closed tour: change[i, j] in float64."""
    pts = np.asarray(points, dtype=np.float64)
    tour = np.asarray(tour, dtype=np.int64)
    pi, pi1 = pts[tour[:-1]], pts[tour[1:]]

    def dmat(a, b):
        d = a[:, None, :] - b[None, :, :]
        return np.sqrt((d ** 2).sum(-1))
    d_i = np.sqrt(((pi - pi1) ** 2).sum(-1))
    return dmat(pi, pi) + dmat(pi1, pi1) - d_i[:, None] - d_i[None, :]


def oracle_best(c64):
    """(min, first flat index) of triu(change, 2), as the oracle takes it (invalid entries are zeros)."""
    v = np.triu(c64, k=2)
    return float(v.min()), int(v.reshape(-1).argmin())


def c32_matrix(points, tour, contracted=True, sqrt_ulps=0):
    pts = np.asarray(points, dtype=np.float64)
    tour = np.asarray(tour, dtype=np.int64)
    pi, pi1 = pts[tour[:-1]], pts[tour[1:]]
    d32 = np.sqrt(((pi - pi1) ** 2).sum(-1)).astype(F32)          # dlen in float64, rounded once
    qi, qi1 = pi.astype(F32), pi1.astype(F32)

    def dist(a):
        dx = a[:, None, 0] - a[None, :, 0]                         # float32 - float32 -> float32
        dy = a[:, None, 1] - a[None, :, 1]
        yy = dy * dy                                               # float32 product
        if contracted:                                             # fma(dx, dx, yy): exact in float64, one rounding
            s = (dx.astype(np.float64) * dx.astype(np.float64) + yy.astype(np.float64)).astype(F32)
        else:
            s = dx * dx + yy
        r = np.sqrt(s)
        for _ in range(abs(sqrt_ulps)):
            r = np.nextafter(r, F32(np.inf if sqrt_ulps > 0 else 0.0))
        return r
    c = ((dist(qi) + dist(qi1)) - d32[:, None]) - d32[None, :]
    assert c.dtype == F32
    return c


def float32_at_or_above(x):
    """The kernel's __double2float_ru: the smallest float32 >= x."""
    f = F32(x)
    return f if float(f) >= x else np.nextafter(f, F32(np.inf))


def screened_best(c32, c64, eps):
    """-> ((min, first flat index), exact pair count, upper bound U, survivor mask).  m32 = min(0, min c32) over the valid pairs, U = min(0, m32 +
    eps), thr = the float32 at or above U + eps; a pair is skipped only if c32 > thr, the others are evaluated exactly."""
    n = c32.shape[0]
    valid = valid_mask(n)
    m32 = min(F32(0.0), c32[valid].min()) if valid.any() else F32(0.0)
    upper = min(0.0, float(m32) + eps)
    thr = float32_at_or_above(upper + eps)
    survive = valid & ~(c32 > thr)
    best_v, best_idx = 0.0, 0                                      # the kernel's running best starts at the no-op move
    for flat in np.flatnonzero(survive.reshape(-1)):               # increasing flat index: strict < keeps the first
        v = c64.reshape(-1)[flat]
        if v < best_v:
            best_v, best_idx = float(v), int(flat)
    return (best_v, best_idx), int(survive.sum()), upper, survive
