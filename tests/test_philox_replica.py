"""CPU tests of the sampler's DESIGN on the host replica of the kernel's noise (tests/philox_replica.py): is Philox transcribed
right (known-answer vectors), is the noise it feeds the rejection loop what the loop assumes (independent N(0,1)^4 and U(0,1),
independent between neighbouring counters), and does the loop on that noise draw from the matrix-Fisher distribution (analytic
float64 answers: rotation angle / axis for F = s I, first moment from the normalising constant).  Whether the KERNEL computes this
replica is tests/test_gpu_philox.py's question.

Every threshold is derived (tests/sampler_stats.py: DKW, normal tail, alpha = 1e-9 per statistic); the power checks at the end show
each statistic failing on the corruption it is there to catch.
"""
import numpy as np
import pytest
import torch
from scipy import special

from oracle import ref_cpu as O
import philox_replica as P
import sampler_stats as T

SEED, CALL, ROUND = 11, 3, 0
N_NOISE = 1 << 21
N_NEIGH = 1 << 19
N_DIST = 1 << 17


def test_philox_known_answer_vectors():
    """The three Philox4x32-10 vectors of Random123's kat_vectors."""
    kat = (((0, 0, 0, 0), (0, 0), (0x6627e8d5, 0xe169c58d, 0xbc57ac4c, 0x9b00dbd8)),
           ((0xffffffff,) * 4, (0xffffffff,) * 2, (0x408f276d, 0x41c83b0e, 0xa20bc7c6, 0x6d5451fd)),
           ((0x243f6a88, 0x85a308d3, 0x13198a2e, 0x03707344), (0xa4093822, 0x299f31d0),
            (0xd16cfe09, 0x94fdcceb, 0x5001e420, 0x24126ea1)))
    for ctr, key, want in kat:
        assert tuple(int(v) for v in P.philox4x32_10(*ctr, *key)) == want
    # vectorised = element by element
    c = np.array([k[0] for k in kat], dtype=np.uint64).T
    k = np.array([k[1] for k in kat], dtype=np.uint64).T
    got = np.stack(P.philox4x32_10(*c, *k), axis=1)
    assert (got == np.array([k[2] for k in kat], dtype=np.uint64)).all()


def test_counter_layout_of_the_replica():
    """kernel_noise puts (proposal, round, gcall low, gcall bits 32..62 | block bit) into the counter and the seed into the key."""
    (x, y, z, w), (x1, _, _, _) = P.kernel_words((0x299f31d0 << 32) | 0xa4093822, (0x03707344 << 32) | 0x13198a2e, 0x85a308d3,
                                                  np.array([0x243f6a88], dtype=np.uint64))
    assert (int(x[0]), int(y[0]), int(z[0]), int(w[0])) == (0xd16cfe09, 0x94fdcceb, 0x5001e420, 0x24126ea1)
    want = P.philox4x32_10(0x243f6a88, 0x85a308d3, 0x13198a2e, 0x83707344, 0xa4093822, 0x299f31d0)
    assert int(x1[0]) == int(want[0])
    # bit 63 of the call index does not reach the counter (bit 31 of the last word is the block bit)
    a = P.kernel_noise(1, 5, 0, 8)
    b = P.kernel_noise(1, 5 + (1 << 63), 0, 8)
    assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1])


# ---- statistics of one noise block ------------------------------------------------------------------------------------------------

def noise_statistics(eps, w):
    """{name: (value, bound)} for eps (n, 4), w (n,): what the rejection loop assumes of its noise."""
    n = w.size
    d, r = T.dkw(n), T.corr_bound(n)
    nrm = np.linalg.norm(eps, axis=1, keepdims=True)
    with np.errstate(invalid="ignore", divide="ignore"):
        x = eps / nrm
    out = {"S3 " + k: (v, d) for k, v in T.s3_uniformity(x).items()}
    out["|eps|^2 ~ chi2(4)"] = (T.ks_stat(nrm ** 2, lambda t: special.gammainc(2.0, t / 2.0)), d)
    for i in range(4):
        out["eps%d ~ N(0,1)" % i] = (T.ks_stat(eps[:, i], special.ndtr), d)
    out["w ~ U(0,1)"] = (T.ks_stat(w, T.cdf_uniform(0.0, 1.0)), d)
    for i in range(4):
        for j in range(i + 1, 4):
            out["corr(eps%d, eps%d)" % (i, j)] = (abs(T.corr(eps[:, i], eps[:, j])), r)
        for j in range(4):
            out["lag-1 corr(eps%d[k], eps%d[k+1])" % (i, j)] = (abs(T.corr(eps[:-1, i], eps[1:, j])), T.corr_bound(n - 1))
        out["corr(w, eps%d)" % i] = (abs(T.corr(w, eps[:, i])), r)
        out["corr(w, eps%d^2)" % i] = (abs(T.corr(w, eps[:, i] ** 2)), r)
    out["lag-1 corr(w[k], w[k+1])"] = (abs(T.corr(w[:-1], w[1:])), T.corr_bound(n - 1))
    return out


failures = T.failures


@pytest.fixture(scope="module")
def noise():
    return P.kernel_noise(SEED, CALL, ROUND, N_NOISE)


def test_replica_noise_is_standard_normal_and_uniform(noise):
    eps, w = noise
    assert eps.shape == (N_NOISE, 4) and np.isfinite(eps).all()
    assert w.min() >= 0.0 and w.max() < 1.0
    stats = noise_statistics(eps, w)
    for k, (v, bound) in sorted(stats.items()):
        print("%-40s %.3e  (<= %.3e)" % (k, v, bound))
    assert not failures(stats)


# ---- neighbouring counters --------------------------------------------------------------------------------------------------------

def neighbour_statistics(a, b):
    """Two noise blocks (eps, w) of equal length: number of identical proposals and the largest cross-correlation."""
    ea, wa = a
    eb, wb = b
    n = wa.size
    same = int((ea == eb).all(1).sum())
    # w has 24 bits: independent blocks agree in Poisson(n / 2^24) places; the smallest k with P(count > k) < ALPHA
    lam = n / 16777216.0
    k = 0
    while special.pdtrc(k, lam) >= T.ALPHA:
        k += 1
    X, Y = np.column_stack([ea, wa]), np.column_stack([eb, wb])
    return {"equal rows": (same, 0), "equal w": (int((wa == wb).sum()), k),
            "max 5x5 cross-correlation": (T.cross_corr_max(X, Y), T.corr_bound(n))}


NEIGHBOURS = {"call + 1": dict(gcall=CALL + 1), "round + 1": dict(rnd=ROUND + 1), "seed + 1": dict(seed=SEED + 1),
              "call + 2^32": dict(gcall=CALL + (1 << 32)), "seed + 2^32": dict(seed=SEED + (1 << 32))}


@pytest.mark.parametrize("which", sorted(NEIGHBOURS))
def test_neighbouring_counters_are_independent(which):
    kw = dict(seed=SEED, gcall=CALL, rnd=ROUND)
    a = P.kernel_noise(kw["seed"], kw["gcall"], kw["rnd"], N_NEIGH)
    kw.update(NEIGHBOURS[which])
    b = P.kernel_noise(kw["seed"], kw["gcall"], kw["rnd"], N_NEIGH)
    stats = neighbour_statistics(a, b)
    print(which, stats)
    assert not failures(stats)


def test_the_two_blocks_of_one_proposal_differ_from_the_next_calls():
    """Block 1 of call g is counter word 3 | 2^31: it must not be block 0 of another reachable call (gcall bits 32..62 only)."""
    (x0, _, _, _), (x1, _, _, _) = P.kernel_words(SEED, CALL, ROUND, np.arange(1 << 16, dtype=np.uint64))
    assert not (x0 == x1).any()


# ---- the rejection loop on replica noise ------------------------------------------------------------------------------------------

def _oracle_rotations(r, U, S, V):
    """R = U_p quat_to_rotmat(q) V_p^T through the oracle's own functions, float64."""
    Up, Sp, Vp = O.proper_svd(torch.from_numpy(U)[None], torch.from_numpy(S)[None], torch.from_numpy(V)[None])
    Rq = O.quat_to_rotmat(torch.from_numpy(r.quat[0]))
    return torch.matmul(Up, torch.matmul(Rq, Vp.transpose(-1, -2))).numpy(), Up[0].numpy(), Sp[0].numpy(), Vp[0].numpy()


@pytest.mark.parametrize("s", [0.0, 0.5, 5.0, 50.0])
def test_rotation_angle_and_axis_of_isotropic_matrix_fisher(s):
    eye = np.eye(3)
    S = np.full(3, s)
    r = P.replay(eye, S, eye, N_DIST, 8 * N_DIST, SEED, CALL)
    assert r.round[0] == 0
    R, _, _, _ = _oracle_rotations(r, eye, S, eye)
    assert np.abs(R - r.R[0]).max() <= 1e-12
    angle, axis = T.angle_axis_from_rotmat(R)
    stats = {"angle": (T.ks_stat(angle, T.cdf_rotation_angle(s)), T.dkw(N_DIST))}
    stats.update({k: (v, T.dkw(N_DIST)) for k, v in T.axis_uniformity(axis).items()})
    a2, _ = T.angle_axis_from_quat(r.quat[0])
    stats["angle (from the quaternion)"] = (T.ks_stat(a2, T.cdf_rotation_angle(s)), T.dkw(N_DIST))
    print(s, stats)
    assert not failures(stats)


@pytest.mark.parametrize("row", range(len(P.IMPROPER_ROWS)))
def test_first_moment_matches_the_normalising_constant(row):
    U, S, V = P.improper_row(row)
    dU, dV = P.IMPROPER_ROWS[row][1:]
    r = P.replay(U, S, V, N_DIST, 8 * N_DIST, SEED, CALL + row)
    assert r.round[0] == 0
    R, Up, Sp, Vp = _oracle_rotations(r, U, S, V)
    assert np.abs(R - r.R[0]).max() <= 1e-12
    assert np.sign(Sp[2]) == dU * dV
    stats = T.moment_statistics(R, U, S, V)
    print(S, T.mf_first_moment(Sp), stats)
    assert not failures(stats)


def test_first_moment_integral_against_closed_forms():
    """mf_first_moment: S = 0 -> 0; S = s I -> (E[1 + 2 cos t] / 3 from the angle density); a small S -> S_k / 3 ... first order."""
    assert np.abs(T.mf_first_moment(np.zeros(3))).max() <= 1e-14
    for s in (0.5, 5.0, 50.0):
        t = np.linspace(0.0, np.pi, 2000001)
        p = (1.0 - np.cos(t)) * np.exp(2.0 * s * (np.cos(t) - 1.0))
        p[-1] *= 0.5                                      # trapezoid (p[0] = 0)
        want = float(((1.0 + 2.0 * np.cos(t)) * p).sum() / p.sum() / 3.0)
        assert np.abs(T.mf_first_moment(np.full(3, s)) - want).max() <= 1e-9, s
    # small concentration: c(S) = 1 + |S|^2 / 6 + s0 s1 s2 / 6 + O(|S|^4)  (E[R_ij R_kl] = delta_ik delta_jl / 3 and
    # E[R_00 R_11 R_22] = 1 / 6 under Haar), so d log c / d s_k = s_k / 3 + s_i s_j / 6 + O(|S|^3)
    S = np.array([3e-4, 2e-4, -1e-4])
    want = S / 3.0 + np.array([S[1] * S[2], S[0] * S[2], S[0] * S[1]]) / 6.0
    assert np.abs(T.mf_first_moment(S) - want).max() <= 1e-10


# ---- power: each corruption of otherwise correct noise must FAIL its statistic ----------------------------------------------------

def test_statistics_catch_a_scaled_component(noise):
    eps, w = noise
    bad = eps.copy()
    bad[:, 0] *= 1.02
    f = failures(noise_statistics(bad, w))
    print(f)
    assert "S3 x0" in f and "eps0 ~ N(0,1)" in f


def test_statistics_catch_correlated_components(noise):
    eps, w = noise
    bad = eps.copy()
    bad[:, 1] = 0.05 * eps[:, 0] + np.sqrt(1.0 - 0.05 ** 2) * eps[:, 1]
    f = failures(noise_statistics(bad, w))
    print(f)
    assert "corr(eps0, eps1)" in f and "S3 atan2(x1,x0)" in f


def test_statistics_catch_an_acceptance_uniform_taken_from_a_normals_word():
    (x, _, _, _), _ = P.kernel_words(SEED, CALL, ROUND, np.arange(N_NOISE, dtype=np.uint64))
    eps, _ = P.kernel_noise(SEED, CALL, ROUND, N_NOISE)
    w_bad = (x >> np.uint64(8)).astype(np.float64) / 16777216.0
    stats = noise_statistics(eps, w_bad)
    assert stats["w ~ U(0,1)"][0] <= stats["w ~ U(0,1)"][1]          # still a perfect uniform on its own
    f = failures(stats)
    print(f)
    assert "corr(w, eps0^2)" in f and "corr(w, eps1^2)" in f


def test_statistics_catch_a_counter_without_the_call_index():
    a = P.kernel_noise(SEED, 0, ROUND, N_NEIGH)          # call 3 and call 4 with the call index dropped: both draw call 0
    b = P.kernel_noise(SEED, 0, ROUND, N_NEIGH)
    f = failures(neighbour_statistics(a, b))
    assert f["equal rows"][0] == N_NEIGH and "max 5x5 cross-correlation" in f


def test_statistics_catch_fewer_philox_rounds():
    """Seven rounds is the weakest Philox4x32 that still passes BigCrush, so a round COUNT that is off is a question for the
    known-answer vectors, not for statistics; what statistics must catch is a generator that is visibly not random: 2 rounds."""
    p = np.arange(N_NEIGH, dtype=np.uint64)
    words = P.philox4x32_10(p, ROUND, CALL, 0, SEED, 0, rounds=2)
    e0, e1 = P._box_muller(words[0], words[1], np.float64)
    e2, e3 = P._box_muller(words[2], words[3], np.float64)
    w = (P.philox4x32_10(p, ROUND, CALL, 0x80000000, SEED, 0, rounds=2)[0] >> np.uint64(8)).astype(np.float64) / 16777216.0
    assert failures(noise_statistics(np.stack([e0, e1, e2, e3], 1), w))
    assert tuple(int(v) for v in P.philox4x32_10(0, 0, 0, 0, 0, 0, rounds=9)) != (0x6627e8d5, 0xe169c58d, 0xbc57ac4c, 0x9b00dbd8)


def test_statistics_report_non_finite_noise_from_a_half_open_radius():
    """A word whose top 24 bits are zero (one draw in 2^24) gives radius sqrt(-2 ln 0) = inf under the half-open map u = (a >> 8) / 2^24;
    the kernel's map ((a >> 8) + 1) / 2^24 keeps it finite.  One such proposal among 2^19 must fail the statistics, not be
    averaged away."""
    (x, y, z, w4), (x1, _, _, _) = P.kernel_words(SEED, CALL, ROUND, np.arange(N_NEIGH, dtype=np.uint64))
    x = x.copy()
    x[12345] = 0x000000C7
    w = (x1 >> np.uint64(8)).astype(np.float64) / 16777216.0
    for open_radius, must_fail in ((True, False), (False, True)):
        e0, e1 = P._box_muller(x, y, np.float64, open_radius)
        e2, e3 = P._box_muller(z, w4, np.float64, open_radius)
        eps = np.stack([e0, e1, e2, e3], 1)
        assert np.isfinite(eps).all() == (not must_fail)
        f = failures(noise_statistics(eps, w))
        assert bool(f) == must_fail, f
        if must_fail:
            assert "S3 x0" in f and "corr(w, eps0)" in f
    # and the first moment refuses it too
    assert T.mean_within(eps[:, 0], 0.0)[0] == float("inf")


def test_moment_statistic_catches_a_wrong_distribution():
    """The loop with the accept test ignored (proposals straight from the envelope) misses the first moment at S = (20, 10, -5)."""
    U, S, V = P.improper_row(1)
    r = P.replay(U, S, V, N_DIST, 8 * N_DIST, SEED, CALL + 1)
    x = r.sd[0] * r.eps[0, :N_DIST]
    x /= np.linalg.norm(x, axis=1, keepdims=True)
    R = np.matmul(r.Up, np.matmul(P.quat_to_rotmat(x), r.Vp[0].T))
    assert failures(T.moment_statistics(R, U, S, V))
