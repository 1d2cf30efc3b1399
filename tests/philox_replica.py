"""Host replica of the noise hps_mf_sample draws inside the kernel (csrc/mf_sample.hip, eps == NULL), in NumPy.

Philox4x32-10 is written from the published algorithm (Salmon, Moraes, Dror, Shaw: "Parallel random numbers: as easy as 1, 2, 3",
SC'11): two 32 x 32 -> 64 bit multiplies per round by 0xD2511F53 / 0xCD9E8D57, the key bumped by the Weyl constants 0x9E3779B9 /
0xBB67AE85 after every round, ten rounds.  The counter / key layout and the maps from words to noise are the kernel's
(include/hps.h, hps_mf_sample):

    key      = (seed bits 0..31, seed bits 32..63)
    counter  = (proposal, round, gcall bits 0..31, gcall bits 32..62 | block << 31)        gcall = call_offset + call
    block 0  : words (x, y) -> Box-Muller pair (e0, e1), words (z, w) -> (e2, e3)
               radius sqrt(-2 ln(((a >> 8) + 1) / 2^24)), angle 2 pi (b >> 8) / 2^24, (cos, sin)
    block 1  : word x -> w = (x >> 8) / 2^24, the acceptance uniform

`replay` is the rejection loop of the reference (utils/sampling_utils.py:48-69) in float64 on that noise.  Nothing here imports
the package under test.
"""
import numpy as np

_M0, _M1 = np.uint64(0xD2511F53), np.uint64(0xCD9E8D57)
_W0, _W1 = np.uint64(0x9E3779B9), np.uint64(0xBB67AE85)
_LO = np.uint64(0xFFFFFFFF)
_S32 = np.uint64(32)
MASK64 = (1 << 64) - 1


def philox4x32_10(c0, c1, c2, c3, k0, k1, rounds=10):
    """Philox4x32 on 32-bit words held in uint64 arrays (broadcast together); returns the four output words."""
    c0, c1, c2, c3, k0, k1 = (np.asarray(a, dtype=np.uint64) & _LO for a in (c0, c1, c2, c3, k0, k1))
    c0, c1, c2, c3 = np.broadcast_arrays(c0, c1, c2, c3)
    for _ in range(rounds):
        p0 = _M0 * c0                       # < 2^64: both factors are below 2^32
        p1 = _M1 * c2
        c0, c1, c2, c3 = (p1 >> _S32) ^ c1 ^ k0, p1 & _LO, (p0 >> _S32) ^ c3 ^ k1, p0 & _LO
        k0 = (k0 + _W0) & _LO
        k1 = (k1 + _W1) & _LO
    return c0, c1, c2, c3


def _box_muller(a, b, dtype, open_radius=True):
    """The kernel's chain in ``dtype``.  ``open_radius=False`` is the WRONG half-open radius map ((a >> 8) / 2^24, which can be 0);
    it exists only for the power check of tests/test_philox_replica.py."""
    dt = np.dtype(dtype).type
    ua = ((a >> np.uint64(8)).astype(dtype) + dt(1.0 if open_radius else 0.0)) * dt(1.0 / 16777216.0)
    ub = (b >> np.uint64(8)).astype(dtype) * dt(1.0 / 16777216.0)
    with np.errstate(divide="ignore"):
        r = np.sqrt(dt(-2.0) * np.log(ua))
    t = dt(6.28318530717958647692) * ub
    return r * np.cos(t), r * np.sin(t)


def kernel_words(seed, gcall, rnd, proposals):
    """The eight 32-bit words of one proposal: (block 0: x, y, z, w), (block 1: x, y, z, w).  gcall / rnd / proposals broadcast."""
    seed = int(seed) & MASK64
    k0, k1 = seed & 0xFFFFFFFF, seed >> 32
    g = np.asarray(gcall, dtype=np.uint64)
    c2 = g & _LO
    c3 = (g >> _S32) & np.uint64(0x7FFFFFFF)
    p = np.asarray(proposals, dtype=np.uint64)
    r = np.asarray(rnd, dtype=np.uint64)
    return philox4x32_10(p, r, c2, c3, k0, k1), philox4x32_10(p, r, c2, c3 | np.uint64(0x80000000), k0, k1)


def kernel_noise(seed, gcall, rnd, proposals, dtype=np.float64):
    """eps (..., 4) and w (...) of the proposals ``proposals`` (an int n means arange(n)) of round ``rnd`` of global call ``gcall``
    under ``seed``.  gcall / rnd / proposals broadcast against each other.  ``dtype=np.float32`` evaluates the same chain in
    single precision (the measure of what fp32 libm-class functions may differ by, not a reference)."""
    if np.isscalar(proposals):
        proposals = np.arange(int(proposals), dtype=np.uint64)
    (x, y, z, w4), (x1, _, _, _) = kernel_words(seed, gcall, rnd, proposals)
    e0, e1 = _box_muller(x, y, dtype)
    e2, e3 = _box_muller(z, w4, dtype)
    dt = np.dtype(dtype).type
    w = (x1 >> np.uint64(8)).astype(dtype) * dt(1.0 / 16777216.0)
    return np.stack([e0, e1, e2, e3], axis=-1), w


# raw factors (S, det U, det V) with generic U, V: the improper ones are what the head can emit (utils/sampling_utils.py:104-111)
IMPROPER_ROWS = [((1.0, 0.5, 0.2), 1, 1), ((20.0, 10.0, 5.0), -1, 1), ((50.0, 2.0, 1.5), 1, -1), ((500.0, 400.0, 300.0), 1, 1)]


def generic_rotation(seed, det):
    """A seeded orthogonal matrix far from the identity with the given determinant (+1 / -1), rounded to fp32 values."""
    q, _ = np.linalg.qr(np.random.default_rng(seed).standard_normal((3, 3)))
    if np.linalg.det(q) * det < 0:
        q[:, 2] = -q[:, 2]
    return q.astype(np.float32).astype(np.float64)


def improper_row(row):
    S, dU, dV = IMPROPER_ROWS[row]
    return generic_rotation(100 + row, dU), np.array(S), generic_rotation(200 + row, dV)


# ---- the rejection loop ---------------------------------------------------------------------------------------------------------

def m_star_of(b):
    return float(np.exp(-(4 - b) / 2) * ((4 / b) ** 2))         # utils/sampling_utils.py:46


def proper_svd(U, S, V):
    """utils/sampling_utils.py:104-111 in float64."""
    U, S, V = (np.array(a, dtype=np.float64) for a in (U, S, V))
    dU, dV = np.linalg.det(U), np.linalg.det(V)
    S[..., 2] *= dU * dV
    U[..., :, 2] *= dU[..., None]
    V[..., :, 2] *= dV[..., None]
    return U, S, V


def envelope(S_proper, b, bingham_a=None, acg_override=None):
    """A, Omega, Gaussian std of every call (C, 4) (:42-45, :118-124)."""
    S = np.asarray(S_proper, dtype=np.float64)
    A = np.zeros(S.shape[:-1] + (4,))
    A[..., 1] = 2 * (S[..., 1] + S[..., 2])
    A[..., 2] = 2 * (S[..., 0] + S[..., 2])
    A[..., 3] = 2 * (S[..., 0] + S[..., 1])
    if bingham_a is not None:
        A = np.array(bingham_a, dtype=np.float64).reshape(A.shape)
    Om = 1.0 + 2.0 * A / b
    sd = Om ** -0.5
    if acg_override is not None:
        o = np.asarray(acg_override, dtype=np.float64).reshape(A.shape[:-1] + (8,))
        Om, sd = o[..., :4], o[..., 4:]
    return A, Om, sd


def accept_ratio(x, A, Om, ms, with_exponent=False):
    """rho = p_Bing* / (M* p_ACG*) of unit quaternions x (..., n, 4) for per-call A, Omega (..., 4)   (:56-61)."""
    qa = np.einsum("...ni,...i,...ni->...n", x, A, x)
    qo = np.einsum("...ni,...i,...ni->...n", x, Om, x)
    rho = np.exp(-qa) * qo * qo / ms
    return (rho, qa) if with_exponent else rho


def amplification(qa):
    """What the exponent x^T A x costs an fp32 evaluation of rho: its rounding (a four-term sum of products, a few 2^-24 qa)
    becomes a RELATIVE error of exp(-qa).  The sampler module's "fp32 rounding tie" of 1e-6 is the figure at an exponent of about
    2; beyond that the margin a decision needs grows in proportion."""
    return np.maximum(1.0, 0.5 * np.abs(qa))


def quat_to_rotmat(q):
    """utils/rigid_transform_utils.py:113-133, (w, x, y, z), in q's dtype."""
    q = q / np.linalg.norm(q, axis=-1, keepdims=True)
    w, x, y, z = (q[..., i] for i in range(4))
    R = np.stack([w * w + x * x - y * y - z * z, 2 * x * y - 2 * w * z, 2 * w * y + 2 * x * z,
                  2 * w * z + 2 * x * y, w * w - x * x + y * y - z * z, 2 * y * z - 2 * w * x,
                  2 * x * z - 2 * w * y, 2 * w * x + 2 * y * z, w * w - x * x - y * y + z * z], axis=-1)
    return R.reshape(q.shape[:-1] + (3, 3))


def rotations(Up, Vp, sd, eps):
    """U_p quat_to_rotmat(normalise(sd eps)) V_p^T for eps (C, N, 4) in eps's dtype (:52-53, :139-141) -> (C, N, 3, 3)."""
    dt = eps.dtype
    y = sd.astype(dt)[:, None, :] * eps
    x = y / np.linalg.norm(y, axis=-1, keepdims=True)
    Rq = quat_to_rotmat(x)
    return np.matmul(Up.astype(dt)[:, None], np.matmul(Rq, np.swapaxes(Vp.astype(dt), -1, -2)[:, None])), x


class Replay:
    """What `replay` found, per call c of C:
    quat (C, N, 4) float64 unit quaternions, the first N accepted of the round that succeeded, in proposal order (NaN: no round did);
    R (C, N, 3, 3) float64 = U_p R(quat) V_p^T; eps (C, n_prop, 4) / w (C, n_prop) / accept (C, n_prop) of that round;
    idx (C, N) the accepted proposals' indices; round (C,) (-1: max_rounds exhausted); n_eval (C,) = index of the N-th accept + 1;
    total (C,) the round's accepts over all n_prop; discarded = round summed over the calls;
    margins are |w - rho| / rho, rho = p_Bing / (M* p_ACG), divided by amplification(x^T A x) (1 for exponents up to 2);
    min_margin (C,): the smallest margin over every proposal of the discarded rounds and the proposals up to the N-th
    accept of the round that succeeded; margin (C, n_prop): that of the final round, every proposal."""

    def accepted_at(self, waves):
        """accepted[c] as the kernel reports it without quat_out: accepts up to the end of the 64 * waves super-block that
        reached N."""
        blk = 64 * waves
        end = np.minimum(-(-self.n_eval // blk) * blk, self.accept.shape[1])
        return np.array([int(self.accept[c, :end[c]].sum()) for c in range(len(end))])

    def margin_at(self, waves):
        """Smallest margin over what `accepted_at(waves)` depends on."""
        blk = 64 * waves
        end = np.minimum(-(-self.n_eval // blk) * blk, self.accept.shape[1])
        return np.array([min(self.min_margin[c], self.margin[c, :end[c]].min()) for c in range(len(end))])


def replay(U, S, V, N, n_prop, seed, call_offset, b=1.5, max_rounds=64, bingham_a=None, acg_override=None, m_star=None):
    """The sampler on replica noise in float64.  U, V (C, 3, 3), S (C, 3): call c is global call call_offset + c."""
    U, S, V = (np.asarray(a, dtype=np.float64) for a in (U, S, V))
    U, S, V = U.reshape(-1, 3, 3), S.reshape(-1, 3), V.reshape(-1, 3, 3)
    C = S.shape[0]
    Up, Sp, Vp = proper_svd(U, S, V)
    A, Om, sd = envelope(Sp, b, bingham_a, acg_override)
    ms = m_star_of(b) if m_star is None else float(m_star)
    out = Replay()
    out.eps = np.zeros((C, n_prop, 4))
    out.w = np.zeros((C, n_prop))
    out.accept = np.zeros((C, n_prop), dtype=bool)
    out.margin = np.full((C, n_prop), np.inf)
    out.idx = np.zeros((C, N), dtype=np.int64)
    out.round = np.full(C, -1, dtype=np.int64)
    out.n_eval = np.full(C, n_prop, dtype=np.int64)
    out.total = np.zeros(C, dtype=np.int64)
    out.min_margin = np.full(C, np.inf)
    gcall = (int(call_offset) + np.arange(C, dtype=object)) & MASK64
    gcall = np.array([int(g) for g in gcall], dtype=np.uint64)
    todo = np.arange(C)
    for rnd in range(max_rounds):
        if todo.size == 0:
            break
        eps, w = kernel_noise(seed, gcall[todo, None], rnd, np.arange(n_prop, dtype=np.uint64)[None, :])
        y = sd[todo, None, :] * eps
        x = y / np.linalg.norm(y, axis=-1, keepdims=True)
        rho, qa = accept_ratio(x, A[todo], Om[todo], ms, with_exponent=True)
        acc = w < rho
        with np.errstate(invalid="ignore", divide="ignore", over="ignore"):
            margin = np.abs(w - rho) / (rho * amplification(qa))
        margin = np.where(np.isfinite(margin), margin, np.inf)
        tot = acc.sum(1)
        ok = tot >= N
        out.eps[todo], out.w[todo], out.accept[todo], out.margin[todo], out.total[todo] = eps, w, acc, margin, tot
        for i in np.nonzero(ok)[0]:
            c = todo[i]
            out.idx[c] = np.nonzero(acc[i])[0][:N]
            out.n_eval[c] = out.idx[c, -1] + 1
            out.round[c] = rnd
            out.min_margin[c] = min(out.min_margin[c], margin[i, :out.n_eval[c]].min())
        for i in np.nonzero(~ok)[0]:
            out.min_margin[todo[i]] = min(out.min_margin[todo[i]], margin[i].min())
        todo = todo[~ok]
    done = out.round >= 0
    sel = np.take_along_axis(out.eps, out.idx[:, :, None], axis=1)
    out.R, out.quat = rotations(Up, Vp, sd, sel)
    out.R[~done] = np.nan
    out.quat[~done] = np.nan
    out.discarded = int(out.round[done].sum())
    out.Up, out.Vp, out.sd = Up, Vp, sd
    return out
