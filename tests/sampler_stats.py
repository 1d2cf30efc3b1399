"""Acceptance statistics for the sampler tests, every threshold derived from the sample size and ALPHA -- none tuned.

ALPHA = 1e-9 per statistic: the suite holds fewer than 1000 of them, so the family-wise error stays below 1e-6.  Seeds are fixed, so
a pass is reproducible; a correct sampler fails a NEW seed with probability below 1e-6.

* Kolmogorov-Smirnov distance against an analytic CDF; threshold from the Dvoretzky-Kiefer-Wolfowitz inequality with Massart's
  constant, P(D_n > d) <= 2 exp(-2 n d^2): d(n, alpha) = sqrt(ln(2 / alpha) / (2 n)).  Holds for every n, no asymptotics.
* sample correlation of independent columns: |r| <= z(alpha / 2) / sqrt(n) (r sqrt(n) -> N(0, 1); n >= 2^17 here).
* sample mean against an analytic one: |mean - mu| <= z(alpha / 2) std / sqrt(n).
"""
import numpy as np
from scipy import special

ALPHA = 1e-9
Z = float(special.ndtri(1.0 - ALPHA / 2.0))          # 6.109...


def dkw(n, alpha=ALPHA):
    return float(np.sqrt(np.log(2.0 / alpha) / (2.0 * n)))


def corr_bound(n):
    return Z / float(np.sqrt(n))


def ks_stat(x, cdf):
    """One-sample KS distance sup |F_n - F|.  Non-finite samples are an error, never averaged away."""
    x = np.asarray(x, dtype=np.float64).ravel()
    if not np.isfinite(x).all():
        return float("inf")
    x = np.sort(x)
    n = x.size
    F = cdf(x)
    i = np.arange(1, n + 1, dtype=np.float64)
    return float(max(np.max(i / n - F), np.max(F - (i - 1) / n)))


def corr(a, b):
    a, b = np.asarray(a, dtype=np.float64).ravel(), np.asarray(b, dtype=np.float64).ravel()
    if not (np.isfinite(a).all() and np.isfinite(b).all()):
        return float("inf")
    a, b = a - a.mean(), b - b.mean()
    return float((a * b).sum() / np.sqrt((a * a).sum() * (b * b).sum()))


def cross_corr_max(X, Y):
    """max |corr| over the columns of X (n, p) against the columns of Y (n, q)."""
    return max(abs(corr(X[:, i], Y[:, j])) for i in range(X.shape[1]) for j in range(Y.shape[1]))


# ---- analytic CDFs ----------------------------------------------------------------------------------------------------------------

def cdf_uniform(lo, hi):
    return lambda x: np.clip((x - lo) / (hi - lo), 0.0, 1.0)


def cdf_s3_component(x):
    """One coordinate of a uniform point on S^3: density (2 / pi) sqrt(1 - x^2)."""
    x = np.clip(x, -1.0, 1.0)
    return 0.5 + (x * np.sqrt(1.0 - x * x) + np.arcsin(x)) / np.pi


def s3_uniformity(x):
    """The eight statistics of a uniform point x (n, 4) on S^3: four coordinate marginals, x0^2 + x1^2 ~ U(0, 1), and the three
    angles atan2(x1, x0), atan2(x3, x2), atan2(x2, x1) ~ U(-pi, pi).  Returns {name: KS distance}."""
    out = {"x%d" % i: ks_stat(x[:, i], cdf_s3_component) for i in range(4)}
    out["x0^2+x1^2"] = ks_stat(x[:, 0] ** 2 + x[:, 1] ** 2, cdf_uniform(0.0, 1.0))
    for i, j in ((0, 1), (2, 3), (1, 2)):
        out["atan2(x%d,x%d)" % (j, i)] = ks_stat(np.arctan2(x[:, j], x[:, i]), cdf_uniform(-np.pi, np.pi))
    return out


def cdf_rotation_angle(s, nodes=400001):
    """CDF of the rotation angle of R ~ matrix-Fisher(F = s I): tr(F^T R) = s (1 + 2 cos t) and the Haar density of the angle is
    (1 - cos t) / pi, so p(t) ~ (1 - cos t) exp(2 s cos t) on [0, pi].  Float64 trapezoid, exponent shifted by its maximum.
    s = 0 (Haar) is the closed form (t - sin t) / pi."""
    if s == 0:
        return lambda t: np.clip((t - np.sin(t)) / np.pi, 0.0, 1.0)
    t = np.linspace(0.0, np.pi, nodes)
    p = (1.0 - np.cos(t)) * np.exp(2.0 * s * (np.cos(t) - 1.0))
    F = np.concatenate([[0.0], np.cumsum(0.5 * (p[1:] + p[:-1]))])
    F /= F[-1]
    return lambda x: np.interp(x, t, F)


def angle_axis_from_quat(q):
    """Rotation angle in [0, pi] and unit axis of unit quaternions (w, x, y, z), float64."""
    q = np.asarray(q, dtype=np.float64)
    v = q[:, 1:] * np.where(q[:, :1] < 0, -1.0, 1.0)
    nv = np.linalg.norm(v, axis=1)
    return 2.0 * np.arctan2(nv, np.abs(q[:, 0])), v / nv[:, None]


def angle_axis_from_rotmat(R):
    R = np.asarray(R, dtype=np.float64)
    v = np.stack([R[:, 2, 1] - R[:, 1, 2], R[:, 0, 2] - R[:, 2, 0], R[:, 1, 0] - R[:, 0, 1]], axis=1)
    nv = np.linalg.norm(v, axis=1)
    return np.arctan2(0.5 * nv, 0.5 * (np.trace(R, axis1=1, axis2=2) - 1.0)), v / nv[:, None]


def axis_uniformity(axis):
    """A uniform direction on S^2: every coordinate ~ U(-1, 1) (Archimedes), azimuth ~ U(-pi, pi).  {name: KS distance}."""
    out = {"axis%d" % i: ks_stat(axis[:, i], cdf_uniform(-1.0, 1.0)) for i in range(3)}
    out["azimuth"] = ks_stat(np.arctan2(axis[:, 1], axis[:, 0]), cdf_uniform(-np.pi, np.pi))
    return out


# ---- first moment of the matrix-Fisher distribution -----------------------------------------------------------------------------

_PANELS, _ORDER = 128, 64                              # composite Gauss-Legendre: 8192 nodes on [-1, 1]


def _gl_nodes():
    x, w = np.polynomial.legendre.leggauss(_ORDER)
    edges = np.linspace(-1.0, 1.0, _PANELS + 1)
    h = 0.5 * (edges[1:] - edges[:-1])
    mid = 0.5 * (edges[1:] + edges[:-1])
    return (mid[:, None] + h[:, None] * x[None, :]).ravel(), (h[:, None] * w[None, :]).ravel()


def mf_first_moment(S_proper):
    """E[(U_p^T R V_p)_kk], k = 0, 1, 2, of R ~ matrix-Fisher(U_p diag(S_proper) V_p^T) with PROPER factors (s_2 may be negative):
    d log c / d s_k with  c(S) = int_{-1}^{1} 1/2 I0(1/2 (s_i - s_j)(1 - u)) I0(1/2 (s_i + s_j)(1 + u)) exp(s_k u) du,  (i, j, k)
    cyclic (Lee, "Bayesian attitude estimation with the matrix Fisher distribution on SO(3)", 2018) -- for each k the form whose
    exponential carries s_k, so the derivative is the mean of u under the integrand.  Bessel functions exponentially scaled
    (scipy.special.ive), the exponents carried in logs and shifted by their maximum."""
    s = np.asarray(S_proper, dtype=np.float64)
    u, wq = _gl_nodes()
    out = np.zeros(3)
    for k in range(3):
        i, j = (k + 1) % 3, (k + 2) % 3
        a = 0.5 * (s[i] - s[j]) * (1.0 - u)
        c = 0.5 * (s[i] + s[j]) * (1.0 + u)
        lf = np.log(special.ive(0, a)) + np.abs(a) + np.log(special.ive(0, c)) + np.abs(c) + s[k] * u
        f = np.exp(lf - lf.max()) * wq
        out[k] = (f * u).sum() / f.sum()
    return out


def mean_within(x, mu, n=None):
    """(|mean - mu|, z(alpha/2) std / sqrt(n)) of a sample column."""
    x = np.asarray(x, dtype=np.float64)
    if not np.isfinite(x).all():
        return float("inf"), 0.0
    n = x.size if n is None else n
    return abs(float(x.mean()) - mu), Z * float(x.std(ddof=1)) / float(np.sqrt(n))


def failures(stats):
    """The entries of {name: (value, bound)} that miss their bound (a NaN value misses it)."""
    return {k: v for k, v in stats.items() if not v[0] <= v[1]}


def moment_statistics(R, U, S, V):
    """{name: (|mean - analytic|, bound)} of D = U_p^T R V_p for rotations R (n, 3, 3) drawn for the RAW factors U, S, V of one
    call (the proper-SVD fix of utils/sampling_utils.py:104-111 is applied here): diagonal against mf_first_moment at
    z std / sqrt(n), off-diagonal (zero by symmetry; an entry of a rotation has |D_ij| <= 1, so std <= 1) at z / sqrt(n)."""
    R, U, S, V = (np.array(a, dtype=np.float64) for a in (R, U, S, V))
    dU, dV = np.linalg.det(U), np.linalg.det(V)
    S[2] *= dU * dV
    U[:, 2] *= dU
    V[:, 2] *= dV
    n = R.shape[0]
    D = np.matmul(U.T[None], np.matmul(R, V[None]))
    want = mf_first_moment(S)
    out = {}
    for i in range(3):
        for j in range(3):
            if i == j:
                out["E[D%d%d]" % (i, j)] = mean_within(D[:, i, j], want[i])
            else:
                out["E[D%d%d]" % (i, j)] = (abs(float(D[:, i, j].mean())) if np.isfinite(D[:, i, j]).all() else float("inf"),
                                            corr_bound(n))
    return out
