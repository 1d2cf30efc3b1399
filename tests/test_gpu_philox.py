"""Does hps_mf_sample's in-kernel Philox route (eps == NULL) compute the host replica (tests/philox_replica.py)?

The replica restates the kernel's noise (Philox4x32-10, counter (proposal, round, call low, call bits 32..62 | block bit), key from the
seed, the two uniform maps, Box-Muller) and the reference's rejection loop in float64; tests/test_philox_replica.py shows on the CPU
that this design draws from the matrix-Fisher distribution.  Here the kernel is compared with it sample by sample: the noise itself
(a), the acceptance uniform (b), the whole route against the already pinned host-noise route fed with replica noise (c), the ordered
compaction across wavefront counts (d), the distribution on the device without the replica (e) and the reported accept counts (f).

Numbers
  TOL = 1e-5 is the sampler module's tolerance and the ceiling of every component tolerance here.  The component tolerance of (a), (b)
  and (c) is 4 x the largest difference between the documented chain evaluated in NumPy float32 and in float64 on the test's own
  proposals (libm-class functions on both sides, a few ulp each).
  TAU = 1e-5: an accept decision w < rho may differ between fp32 and float64 only where |w - rho| / rho < TAU * amplification, ten
  times the "fp32 rounding tie" the sampler module states.  amplification = max(1, x^T A x / 2): rho = exp(-x^T A x) (...), so the fp32
  rounding of the exponent becomes a relative error of rho that grows with it; a flat 1e-5 is NOT four times the fp32-vs-float64
  difference of rho on the concentrated rows (measured up to 1.1e-5, at exponents of about 20), the scaled one is
  (test_fp32_accept_ratio_stays_within_a_quarter_of_the_margin: at most 1.0e-6 x amplification, against TAU / 4 = 2.5e-6).
  A call is fragile if a proposal its result depends on sits inside that margin; fragile calls are compared for validity only and
  at most CAP = 5 % of a case's calls may be fragile (asserted from the replica alone, also without a GPU).

Measured on an MI355X: see the docstrings of the tests.  The 41 GPU tests of this file take 4.6 s together.
"""
import numpy as np
import pytest
import torch

from oracle import ref_cpu as O
import philox_replica as P
import sampler_stats as T

gpu = pytest.mark.gpu
TOL = 1e-5
TAU = 1e-5
CAP = 0.05
B_ENV = 1.5
N_ALL = [1, 4, 64, 65, 100, 128, 129, 300, 384, 385, 896, 897, 1000, 2000]


def _su():
    from hierarchicalprobabilistic3dhuman_amd import sampling_utils as su
    return su


def waves(N):
    return min(8, max(1, (2 * N + 255) // 256))


def per_call(t):
    """(B, N, nj, ...) device tensor -> (B * nj, N, ...) float64 NumPy, call-major like the replica."""
    t = t.detach().cpu().double()
    return t.transpose(1, 2).reshape((t.shape[0] * t.shape[2], t.shape[1]) + tuple(t.shape[3:])).numpy()


def assert_proper_rotations(R):
    R = np.asarray(R, dtype=np.float64).reshape(-1, 3, 3)
    assert np.isfinite(R).all()
    assert np.abs(np.matmul(np.swapaxes(R, 1, 2), R) - np.eye(3)).max() <= 1e-5
    assert np.abs(np.linalg.det(R) - 1.0).max() <= 1e-5


# ---- inputs and cases of (c), (d), (f) ----------------------------------------------------------------------------------------------

STARVED_LOW = [4, 13, 27, 36, 40]


def input_sets(golden):
    """'mix' (5 x 23 calls): the two net images, the two starved images and one image made of the 7 sweep rows, the 4 improper rows
    of tests/test_philox_replica.py and 12 more starved rows.  'lean' (4 x 23 calls): net + starved, every call with an acceptance
    of 49 % or more, for oversampling_ratio = 2: a row that accepts 47 % would need more than the kernel's 64 rounds to collect
    2000 of 4000 proposals; five such starved rows are replaced by net rows."""
    g = {k: golden[k].numpy().astype(np.float64) for k in ("net_U", "net_S", "net_V", "sweep_U", "sweep_S", "sweep_V",
                                                          "starved_U", "starved_S", "starved_V")}
    imp = [P.improper_row(i) for i in range(len(P.IMPROPER_ROWS))]
    last = [np.concatenate([g["sweep_" + k][0], np.stack([r[i] for r in imp]), g["starved_" + k][0][:12]])[None]
            for i, k in enumerate("USV")]
    lean = [np.concatenate([g["net_" + k], g["starved_" + k]]) for k in "USV"]
    for a in lean:                   # the starved rows that accept less than 48.8 % (16000 replica proposals each) leave 'lean'
        flat = a.reshape((92,) + a.shape[2:])
        flat[[46 + i for i in STARVED_LOW]] = flat[:len(STARVED_LOW)]
    return {"lean": tuple(lean), "mix": tuple(np.concatenate([a, b]) for a, b in zip(lean, last))}


# (input set, N, oversampling_ratio, seed, image_offset).  Seeds are 1000 + N / 2000 + N, except where that seed misses a condition
# asserted below (fragile share, >= 10 discarded rounds at x2, no call beyond the kernel's 64 rounds): then the first of
# seed + 10000 k that meets them, found on the CPU from the replica alone.
RESEEDED = {("lean", 65): 32065, ("lean", 300): 12300, ("lean", 1000): 13000, ("lean", 2000): 24000}
CASES = [("mix", N, 8, 1000 + N, N % 7) for N in N_ALL] + \
        [("lean", N, 2, RESEEDED.get(("lean", N), 2000 + N), (N + 3) % 5) for N in N_ALL]
_replays = {}
_inputs = {}


def case_id(case):
    return "%s-N%d-x%d" % case[:3]


def replay_case(golden, case):
    """(U, S, V float64 (B, nj, ...), Replay) of a case, computed once per process."""
    if not _inputs:
        _inputs.update(input_sets(golden))
    if case not in _replays:
        name, N, ratio, seed, off = case
        U, S, V = _inputs[name]
        nj = U.shape[1]
        _replays[case] = P.replay(U.reshape(-1, 3, 3), S.reshape(-1, 3), V.reshape(-1, 3, 3), N, N * ratio, seed, off * nj, b=B_ENV)
    return _inputs[case[0]] + (_replays[case],)


def chain_difference(r, seed, call_offset):
    """Largest |float32 chain - float64 chain| over the accepted proposals of a replay: quaternion components and rotation entries.
    The float32 chain: Box-Muller, sd * eps, normalisation, quaternion -> rotation, U_p R V_p^T, all in NumPy float32."""
    C, N = r.idx.shape
    ok = r.round >= 0
    gcall = np.array([(int(call_offset) + c) & P.MASK64 for c in range(C)], dtype=np.uint64)
    eps32, _ = P.kernel_noise(seed, gcall[:, None], np.maximum(r.round, 0)[:, None], r.idx.astype(np.uint64), dtype=np.float32)
    R32, q32 = P.rotations(r.Up, r.Vp, r.sd, eps32)
    return float(np.abs(q32[ok] - r.quat[ok]).max()), float(np.abs(R32[ok] - r.R[ok]).max())


_tol_c = []


def tolerance_c(golden):
    """4 x the float32-vs-float64 chain difference of the rotations over ALL cases' accepted proposals, at most TOL."""
    if not _tol_c:
        worst = 0.0
        for case in CASES:
            r = replay_case(golden, case)[3]
            worst = max(worst, chain_difference(r, case[3], case[4] * _inputs[case[0]][0].shape[1])[1])
        _tol_c.append(worst)
    return min(4.0 * _tol_c[0], TOL), _tol_c[0]


def rho_fp32(U, S, V, eps, b=B_ENV):
    """rho of every proposal in the oracle's fp32 arithmetic (oracle/ref_cpu.py bingham_sampling / pose_matrix_fisher_sampling)."""
    U, S, V = (torch.from_numpy(a.reshape((-1,) + a.shape[2:])).float() for a in (U, S, V))
    _, Sp, _ = O.proper_svd(U, S, V)
    A = torch.zeros(S.shape[0], 4)
    A[:, 1] = 2 * (Sp[:, 1] + Sp[:, 2])
    A[:, 2] = 2 * (Sp[:, 0] + Sp[:, 2])
    A[:, 3] = 2 * (Sp[:, 0] + Sp[:, 1])
    Omega = torch.ones_like(A) + 2 * A / b
    std = Omega ** (-0.5)
    y = std[:, None, :] * torch.from_numpy(eps).float()
    x = y / torch.norm(y, dim=2, keepdim=True)
    p_bing = torch.exp(-torch.einsum('cbn,cn,cbn->cb', x, A, x))
    p_acg = torch.einsum('cbn,cn,cbn->cb', x, Omega, x) ** (-2)
    return (p_bing / (O.m_star(b) * p_acg)).double().numpy()


# ---- conditions on the cases, from the replica alone (no GPU) ---------------------------------------------------------------------

@pytest.mark.parametrize("case", CASES, ids=case_id)
def test_cases_meet_the_fragility_cap_and_exercise_redraws(case, golden):
    """Fragile calls per case (of 115 for 'mix', 92 for 'lean') at TAU = 1e-5: x8: none up to N = 100, 0..3 up to N = 1000, 5 at
    N = 2000 (4.3 %); x2: 0..3.  Discarded rounds at x2: 10..48 per case, the deepest call succeeds in round 27."""
    U, S, V, r = replay_case(golden, case)
    assert (r.round >= 0).all(), "a call exhausts the kernel's 64 rounds: choose another seed"
    share = float((r.min_margin < TAU).mean())
    print(case_id(case), "fragile %d / %d" % ((r.min_margin < TAU).sum(), r.round.size), "discarded rounds", r.discarded,
          "deepest round", int(r.round.max()))
    assert share <= CAP
    if case[2] == 2:
        assert r.discarded >= 10, "the case no longer exercises the in-kernel redraw (round > 0)"
    n_prop, W = case[1] * case[2], waves(case[1])
    if case[1] in (100, 129):
        assert n_prop % (64 * W) != 0          # a ragged last super-block


@pytest.mark.parametrize("case", CASES, ids=case_id)
def test_fp32_accept_ratio_stays_within_a_quarter_of_the_margin(case, golden):
    """rho in the oracle's fp32 arithmetic against float64 on the proposals the final round evaluated (those that can decide at all:
    rho >= 2^-25, half the spacing of w's grid): relative difference / amplification <= TAU / 4.  Largest over the 28 cases: 1.0e-6
    (and 1.1e-5 WITHOUT the amplification, at exponents of about 20 -- why the margin is scaled)."""
    U, S, V, r = replay_case(golden, case)
    C, n_prop = r.w.shape
    y = r.sd[:, None, :] * r.eps
    x = y / np.linalg.norm(y, axis=-1, keepdims=True)
    A, Om, _ = P.envelope(P.proper_svd(U.reshape(-1, 3, 3), S.reshape(-1, 3), V.reshape(-1, 3, 3))[1], B_ENV)
    rho, qa = P.accept_ratio(x, A, Om, P.m_star_of(B_ENV), with_exponent=True)
    rho32 = rho_fp32(U, S, V, r.eps)
    m = (np.arange(n_prop)[None, :] < r.n_eval[:, None]) & (rho >= 2.0 ** -25)
    rel = np.abs(rho32 - rho)[m] / rho[m]
    print(case_id(case), "max relative %.3e, / amplification %.3e" % (rel.max(), (rel / P.amplification(qa[m])).max()))
    assert (rel / P.amplification(qa[m])).max() <= TAU / 4


# ---- (a) the noise ----------------------------------------------------------------------------------------------------------------

SEEDS = [0, 1, 2 ** 32 - 1, 2 ** 32, 2 ** 63 + 12345, 2 ** 64 - 1]
CALL_OFFSETS = [0, 23 * 5, 2 ** 32 - 7, 2 ** 40 + 3]
PAD = 37            # proposals past N: the round's total must count them


def _trivial_envelope(C, dev):
    return torch.zeros(C, 4, device=dev), torch.ones(C, 8, device=dev)


@gpu
def test_kernel_noise_is_the_replicas(dev):
    """Bingham entry with A = 0, Omega = 1, std = 1, M* = 1/2: rho = 2, every proposal is accepted and quat_out[k] = eps_k / |eps_k|.
    4 x 23 calls, every N x seed x call_offset (2^32 - 7: the calls straddle the carry into the counter's last word), every
    component against the replica; the same launches with the key read from device memory (seed_dev) must give the same bits.
    Measured: float32 chain vs float64 4.31e-7 (tolerance 1.72e-6); MI355X vs float64 4.24e-7."""
    su = _su()
    B, nj = 4, 23
    C = B * nj
    eye = torch.eye(3, device=dev).expand(B, nj, 3, 3).contiguous()
    S0 = torch.zeros(B, nj, 3, device=dev)
    a0, ov = _trivial_envelope(C, dev)
    want, chain = {}, 0.0
    for N in (1, 64, 100, 129, 1000):
        prop = np.arange(N, dtype=np.uint64)[None, :]
        for seed in SEEDS:
            for off in CALL_OFFSETS:
                gcall = np.array([(off + c) & P.MASK64 for c in range(C)], dtype=np.uint64)[:, None]
                e64, _ = P.kernel_noise(seed, gcall, 0, prop)
                e32, _ = P.kernel_noise(seed, gcall, 0, prop, dtype=np.float32)
                q64 = e64 / np.linalg.norm(e64, axis=-1, keepdims=True)
                q32 = e32 / np.sqrt((e32 * e32).sum(-1, keepdims=True, dtype=np.float32))
                chain = max(chain, float(np.abs(q32 - q64).max()))
                want[(N, seed, off)] = q64
    tol = min(4.0 * chain, TOL)
    worst = 0.0
    for (N, seed, off), q64 in want.items():
        n_prop = N + PAD
        _, quat, acc = su._launch(eye, S0, eye, N, n_prop, B_ENV, seed=seed, call_offset=off, bingham_a=a0, want_quat=True,
                                  acg_override=ov, m_star=0.5)
        assert (acc.cpu().numpy() == n_prop).all(), (N, seed, off)
        err = float(np.abs(per_call(quat) - q64).max())
        worst = max(worst, err)
        assert err <= tol, (N, seed, off, err, tol)
        if N == 129:
            key = torch.tensor([su.philox_key(seed, signed=True), off], dtype=torch.int64, device=dev)
            _, quat_d, acc_d = su._launch(eye, S0, eye, N, n_prop, B_ENV, seed=0, call_offset=0, bingham_a=a0, want_quat=True,
                                          acg_override=ov, m_star=0.5, seed_dev=key)
            assert torch.equal(quat_d, quat) and torch.equal(acc_d, acc), (seed, off)
    print("4a: float32 chain vs float64 %.3e, tolerance %.3e, device vs float64 %.3e" % (chain, tol, worst))


# ---- (b) the acceptance uniform ----------------------------------------------------------------------------------------------------

@gpu
@pytest.mark.parametrize("t", [0.1, 0.5, 0.9])
def test_acceptance_uniform_is_the_replicas(t, dev):
    """Same envelope with M* = 1 / t: rho = t (sum x^2)^2, so the accepted set is {k : w_k < t}: the accepted directions in order
    (quat_out) and the round's total (accepted, count_all) against the replica.  n_prop = 32 N at t = 0.1 (a round still reaches N,
    and the proposal counter walks far past N).  Only proposals inside the margin TAU may differ.
    Measured: float32 chain vs float64 3.9e-7..4.1e-7 (tolerance 4 x that); MI355X vs float64 the same figures."""
    su = _su()
    B, nj = 2, 23
    C = B * nj
    eye = torch.eye(3, device=dev).expand(B, nj, 3, 3).contiguous()
    S0 = torch.zeros(B, nj, 3, device=dev)
    a0, ov = _trivial_envelope(C, dev)
    I = np.broadcast_to(np.eye(3), (C, 3, 3))
    for N in (100, 300):
        n_prop = (32 if t == 0.1 else 8) * N
        seed, off = 77 + N, 5
        r = P.replay(I, np.zeros((C, 3)), I, N, n_prop, seed, off, b=B_ENV, bingham_a=np.zeros((C, 4)),
                     acg_override=np.ones((C, 8)), m_star=1.0 / t)
        assert (r.round >= 0).all()
        chain = chain_difference(r, seed, off)[0]
        tol = min(4.0 * chain, TOL)
        _, quat, acc = su._launch(eye, S0, eye, N, n_prop, B_ENV, seed=seed, call_offset=off, bingham_a=a0, want_quat=True,
                                  acg_override=ov, m_star=1.0 / t)
        acc, q = acc.cpu().numpy(), per_call(quat)
        near = (r.margin < TAU).sum(1)                              # proposals of the final round inside the margin
        strict = (r.min_margin >= TAU) & (near == 0)
        assert (~(r.min_margin >= TAU)).mean() <= CAP
        assert (np.abs(acc - r.total) <= near).all(), (t, N)
        assert (acc[strict] == r.total[strict]).all()
        err = float(np.abs(q[r.min_margin >= TAU] - r.quat[r.min_margin >= TAU]).max())
        print("4b t=%.1f N=%d: accepted %d..%d of %d, chain %.3e, device vs float64 %.3e" % (t, N, acc.min(), acc.max(), n_prop, chain, err))
        assert err <= tol
        assert np.abs(np.linalg.norm(q, axis=-1) - 1.0).max() <= 1e-5


# ---- (c) the whole route against the host-noise route on replica noise ----------------------------------------------------------------

@gpu
@pytest.mark.parametrize("case", CASES, ids=case_id)
def test_philox_route_equals_host_noise_route_on_replica_noise(case, dev, golden):
    """pose_matrix_fisher_sampling_torch(seed, image_offset) against hps_mf_sample fed with the replica's noise of the round the
    replica says succeeded (device arithmetic on both sides: TOL), against the replica's float64 rotations (4 x the float32-vs-
    float64 chain difference, at most TOL), and the accept counts it reports.  N walks 1..8 wavefronts per call and both sides of
    each step; x2 cases redraw in the kernel (>= 10 discarded rounds, asserted).
    Measured over the 28 cases: float32 chain vs float64 2.17e-6 (tolerance 8.69e-6); MI355X vs float64 at most 2.16e-6, vs the
    host-noise route at most 2.25e-6; fragile calls 0..5 of 115 / 0..3 of 92, discarded rounds 10..48 at x2."""
    su = _su()
    name, N, ratio, seed, off = case
    U64, S64, V64, r = replay_case(golden, case)
    tol, chain = tolerance_c(golden)
    B, nj = U64.shape[:2]
    C, n_prop = B * nj, N * ratio
    fragile = r.min_margin < TAU
    assert (r.round >= 0).all() and fragile.mean() <= CAP
    if ratio == 2:
        assert r.discarded >= 10
    U, S, V = (torch.from_numpy(a).float().to(dev) for a in (U64, S64, V64))
    R = su.pose_matrix_fisher_sampling_torch(U, S, V, N, oversampling_ratio=ratio, seed=seed, image_offset=off)
    su.check_sampling()
    acc = su.last_accepted[0].cpu().numpy()
    eps = torch.from_numpy(r.eps.astype(np.float32)).to(dev)
    w = torch.from_numpy(r.w.astype(np.float32)).to(dev)
    Rh, _, acc_h = su._launch(U, S, V, N, n_prop, B_ENV, eps=eps, w=w, draw_idx=torch.arange(C, dtype=torch.int32, device=dev))
    R, Rh, acc_h = per_call(R), per_call(Rh), acc_h.cpu().numpy()
    assert_proper_rotations(R)
    ok = ~fragile
    assert (acc_h[ok] >= N).all()
    e_host, e_ref = float(np.abs(R[ok] - Rh[ok]).max()), float(np.abs(R[ok] - r.R[ok]).max())
    print("4c %s: fragile %d / %d, discarded %d, chain %.3e (tol %.3e), device vs float64 %.3e, vs host-noise route %.3e"
          % (case_id(case), fragile.sum(), C, r.discarded, chain, tol, e_ref, e_host))
    assert e_host <= TOL
    assert e_ref <= tol
    counted = r.margin_at(waves(N)) >= TAU
    assert (acc[counted] == r.accepted_at(waves(N))[counted]).all()
    assert (acc_h[counted] == acc[counted]).all()


# ---- (d) prefix property -----------------------------------------------------------------------------------------------------------

@gpu
def test_more_samples_extend_the_same_sequence(dev, golden):
    """Same key, N0 < N1: the first N0 samples of every call are the same bits whenever round 0 succeeds in both runs (it does here:
    the net rows accept more than 30 %, asserted from the replica and from last_accepted) -- the ordered compaction across 1, 2, 3
    and 8 wavefronts on Philox noise."""
    su = _su()
    U64, S64, V64 = (golden[k].numpy().astype(np.float64) for k in ("net_U", "net_S", "net_V"))
    U, S, V = (golden[k].to(dev) for k in ("net_U", "net_S", "net_V"))
    seed, off = 31337, 2
    out = {}
    for N in (64, 100, 128, 129, 300, 1000):
        r = P.replay(U64.reshape(-1, 3, 3), S64.reshape(-1, 3), V64.reshape(-1, 3, 3), N, 8 * N, seed, off * 23, b=B_ENV)
        assert (r.round == 0).all() and (r.total >= 0.3 * 8 * N).all()
        out[N] = su.pose_matrix_fisher_sampling_torch(U, S, V, N, seed=seed, image_offset=off)
        assert int(su.last_accepted[0].min()) >= N
    su.check_sampling()
    for N0 in (64, 100, 128):
        for N1 in (129, 300, 1000):
            assert torch.equal(out[N1][:, :N0], out[N0]), (N0, N1)


# ---- (e) the distribution on the device ---------------------------------------------------------------------------------------------

def _pooled(dev, U, S, V, seed, calls=64, N=1000):
    su = _su()
    Ud, Sd, Vd = (torch.from_numpy(np.ascontiguousarray(np.broadcast_to(a, (calls, 1) + a.shape))).float().to(dev) for a in (U, S, V))
    R = su.pose_matrix_fisher_sampling_torch(Ud, Sd, Vd, N, seed=seed)
    su.check_sampling()
    R = per_call(R)                                                 # (calls, N, 3, 3)
    assert_proper_rotations(R)
    flat = R.reshape(-1, 9)
    assert np.unique(flat, axis=0).shape[0] == flat.shape[0], "two calls (or two proposals) share a sample"
    return R.reshape(-1, 3, 3)


@gpu
def test_device_samples_of_isotropic_matrix_fisher(dev):
    """64 calls with IDENTICAL parameters x 1000 samples in one launch: no sample occurs twice; pooled (n = 64000) rotation angle
    and axis of F = 5 I against the analytic distribution at the DKW threshold."""
    R = _pooled(dev, np.eye(3), np.full(3, 5.0), np.eye(3), seed=5)
    n = R.shape[0]
    angle, axis = T.angle_axis_from_rotmat(R)
    stats = {"angle": (T.ks_stat(angle, T.cdf_rotation_angle(5.0)), T.dkw(n))}
    stats.update({k: (v, T.dkw(n)) for k, v in T.axis_uniformity(axis).items()})
    print(stats)
    assert not T.failures(stats)


@gpu
@pytest.mark.parametrize("row", range(len(P.IMPROPER_ROWS)))
def test_device_first_moment_matches_the_normalising_constant(row, dev):
    U, S, V = P.improper_row(row)
    R = _pooled(dev, U, S, V, seed=60 + row)
    stats = T.moment_statistics(R, U, S, V)
    print(S, stats)
    assert not T.failures(stats)


# ---- (f) accepted without quat_out ---------------------------------------------------------------------------------------------------

@gpu
@pytest.mark.parametrize("N", [100, 200, 1000])
def test_accept_count_is_up_to_the_iteration_that_reached_n(N, dev, golden):
    """Without quat_out the kernel stops at the 64 W proposal super-block in which the N-th accept falls and reports the accepts up
    to its end: W = 1, 2, 8.  (A call that exhausts max_rounds reports < N: test_gpu_sampler.py::test_failed_sampling_is_loud.)"""
    su = _su()
    W = waves(N)
    assert W == {100: 1, 200: 2, 1000: 8}[N]
    case = ("lean", N, 8, 4000 + N, 1)
    U64, S64, V64, r = replay_case(golden, case)
    U, S, V = (torch.from_numpy(a).float().to(dev) for a in (U64, S64, V64))
    su.pose_matrix_fisher_sampling_torch(U, S, V, N, seed=case[3], image_offset=case[4])
    su.check_sampling()
    acc = su.last_accepted[0].cpu().numpy()
    counted = r.margin_at(W) >= TAU
    assert (~counted).mean() <= CAP
    want = r.accepted_at(W)
    assert (want >= N).all() and (want <= r.total).all()
    assert (acc[counted] == want[counted]).all()
    assert (acc >= N).all()
