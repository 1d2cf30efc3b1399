"""GPU parity: matrix-Fisher sampling kernel against the golden vectors the imported reference produced
(same torch seed, sample_on_cpu route), against the oracle with forced discarded rounds, and the Philox
route through seed-independent properties (first moment, orthonormality, sharding invariance).  The Philox route is pinned
sample by sample in tests/test_gpu_philox.py, against the host replica of the kernel's noise (tests/philox_replica.py).

Stated tolerance: rotation matrices <= 1e-5 given identical (U,S,V, eps, w); an accept decision may flip only
on an fp32 rounding tie (<= 1e-6 of proposals) -- a flip would change every later sample of that call."""
import pytest
import torch

from oracle import ref_cpu as O
from hierarchicalprobabilistic3dhuman_amd import sampling_utils as su
from hierarchicalprobabilistic3dhuman_amd import rigid_transform_utils as rtu
from conftest import maxerr
import sampler_stats

pytestmark = pytest.mark.gpu
TOL = 1e-5


@pytest.mark.parametrize("N", [1, 4, 100])
def test_host_stream_route_reproduces_reference_samples(N, dev, golden):
    U, S, V = (golden[k].to(dev) for k in ("net_U", "net_S", "net_V"))
    torch.manual_seed(0)
    R = su.pose_matrix_fisher_sampling_torch(U, S, V, N, sample_on_cpu=True)
    assert R.shape == (2, N, 23, 3, 3)
    assert maxerr(R, golden["sampler_R_N%d" % N]) <= TOL


@pytest.mark.parametrize("N", [129, 300, 1000])
def test_multi_wavefront_sizes_reproduce_reference_samples(N, dev, golden):
    """hps_mf_sample runs ceil(2N / 256) wavefronts per (image, joint) call: 2, 3 and 8 here (N = 1000 is BASELINE configs[4]).
    "The first N accepted, in proposal order" (utils/sampling_utils.py:61-66) across wavefront boundaries: the kept samples of the
    reference's run (tests/golden/make_golden.py) and the float64 sum over ALL of its samples."""
    U, S, V = (golden[k].to(dev) for k in ("net_U", "net_S", "net_V"))
    torch.manual_seed(40 + N)
    R = su.pose_matrix_fisher_sampling_torch(U, S, V, N, sample_on_cpu=True)
    assert R.shape == (2, N, 23, 3, 3)
    assert maxerr(R[:, golden["sampler_R_N%d_keep" % N].to(dev)], golden["sampler_R_N%d_sub" % N]) <= TOL
    assert maxerr(R.double().sum(1), golden["sampler_R_N%d_sum" % N]) <= TOL * N


def test_starved_multi_wavefront_rounds_follow_the_reference(dev, golden):
    """oversampling_ratio = 2, N = 200 (two wavefronts, 400 proposals = three whole super-blocks and a ragged one) on broad
    concentrations: the reference discards 23 rounds here, up to 9 for one call (utils/sampling_utils.py:68-69); every later call
    shifts along the host stream.  Samples and the generator's final state must equal the reference's."""
    U, S, V = (golden[k].to(dev) for k in ("starved_U", "starved_S", "starved_V"))
    assert int(golden["starved_discarded"].sum()) >= 10
    torch.manual_seed(9)
    R = su.pose_matrix_fisher_sampling_torch(U, S, V, 200, oversampling_ratio=2, sample_on_cpu=True)
    assert maxerr(R, golden["starved_R_N200"]) <= TOL
    assert torch.equal(torch.rand(1), golden["starved_next_rand"])
    # the Philox route with the same starved budget: N proper rotations per call, and the same bits whatever the batch split
    Rp = su.pose_matrix_fisher_sampling_torch(U, S, V, 200, oversampling_ratio=2, seed=3)
    su.check_sampling()
    assert float((torch.matmul(Rp.transpose(-1, -2), Rp) - torch.eye(3, device=dev)).abs().max()) <= 1e-5
    Rq = su.pose_matrix_fisher_sampling_torch(U[1:], S[1:], V[1:], 200, oversampling_ratio=2, seed=3, image_offset=1)
    assert torch.equal(Rq[0], Rp[1])


def test_concentration_sweep_reproduces_reference(dev, golden):
    torch.manual_seed(1)
    R = su.pose_matrix_fisher_sampling_torch(golden["sweep_U"].to(dev), golden["sweep_S"].to(dev),
                                             golden["sweep_V"].to(dev), 50, sample_on_cpu=True)
    assert maxerr(R, golden["sweep_R_N50"]) <= TOL


def test_bingham_entry_point_reproduces_reference(dev, golden):
    torch.manual_seed(2)
    q, ratio = su.bingham_sampling_for_matrix_fisher_torch(golden["bingham_A"].to(dev), 16, sample_on_cpu=True)
    assert maxerr(q, golden["bingham_q_N16"]) <= TOL and ratio > 0


def test_discarded_rounds_follow_the_reference_stream(dev):
    """A round with fewer than N accepted proposals is discarded and redrawn (utils/sampling_utils.py:68-69),
    which shifts every later call along the host random stream.  oversampling_ratio=2 with N=1 makes that
    happen for ~10 % of the calls (including double discards); results must still match the sequential loop."""
    g = torch.Generator().manual_seed(5)
    F = torch.randn(8, 23, 3, 3, generator=g) * 0.3 + torch.eye(3)
    U, S, Vh = torch.linalg.svd(F)
    V = Vh.transpose(-1, -2).contiguous()
    torch.manual_seed(9)
    Rref, (_, _, disc) = O.pose_matrix_fisher_sampling(U, S, V, 1, oversampling_ratio=2, return_noise=True)
    assert int(disc.sum()) >= 5 and int(disc.max()) >= 2, "test input no longer exercises discarded rounds"
    torch.manual_seed(9)
    R = su.pose_matrix_fisher_sampling_torch(U.to(dev), S.to(dev), V.to(dev), 1, oversampling_ratio=2, sample_on_cpu=True)
    assert maxerr(R, Rref) <= TOL
    # the host generator must end in the same state as after the reference loop
    a = torch.rand(1)
    torch.manual_seed(9)
    O.pose_matrix_fisher_sampling(U, S, V, 1, oversampling_ratio=2)
    assert torch.equal(a, torch.rand(1))
    # Philox route with the same starved proposal budget still returns N valid rotations per call
    Rp = su.pose_matrix_fisher_sampling_torch(U.to(dev), S.to(dev), V.to(dev), 1, oversampling_ratio=2, seed=3)
    assert float((torch.matmul(Rp.transpose(-1, -2), Rp) - torch.eye(3, device=dev)).abs().max()) <= 1e-5


def test_philox_route_properties(dev, golden):
    U, S, V = (golden[k].to(dev) for k in ("sweep_U", "sweep_S", "sweep_V"))
    N = 20000
    R = su.pose_matrix_fisher_sampling_torch(U, S, V, N, seed=2024)
    # proper rotations
    eye = torch.eye(3, device=dev)
    assert float((torch.matmul(R.transpose(-1, -2), R) - eye).abs().max()) <= 1e-5
    assert float((torch.det(R.cpu()) - 1).abs().max()) <= 1e-5
    # E[R] = U diag(dlogc/ds) V^T, gradient from the reference's LogMFNormConstant (golden)
    # (row 5, S = (500,400,300), is left out: there the reference's 512-point trapezoid integral is itself off by
    #  ~0.09 against a 20000-sample Monte-Carlo mean of the reference's own sampler; the other rows agree to 0.01)
    D = torch.matmul(U[0].transpose(-1, -2), torch.matmul(R[0].mean(0), V[0])).cpu()
    rows = [0, 1, 2, 3, 4, 6]
    assert maxerr(D[rows], torch.diag_embed(golden["sweep_dlogc_dS"])[rows]) <= 0.025
    # ... and every row, row 5 included, against the float64 first moment (tests/sampler_stats.py: Gauss-Legendre on the
    # one-dimensional form of c(S), not the reference's trapezoid rule) at the normal-tail bound z(alpha/2) std / sqrt(N)
    for row in range(7):
        stats = sampler_stats.moment_statistics(R[0, :, row].cpu().numpy(), U[0, row].cpu().numpy(), S[0, row].cpu().numpy(),
                                                V[0, row].cpu().numpy())
        assert not sampler_stats.failures(stats), (row, stats)
    # same seed -> same samples; different seed -> different samples
    assert torch.equal(R, su.pose_matrix_fisher_sampling_torch(U, S, V, N, seed=2024))
    assert not torch.equal(R, su.pose_matrix_fisher_sampling_torch(U, S, V, N, seed=2025))


def test_philox_is_sharding_invariant(dev):
    g = torch.Generator().manual_seed(8)
    F = torch.randn(8, 23, 3, 3, generator=g) * 2 + torch.eye(3)
    U, S, Vh = torch.linalg.svd(F)
    U, S, V = U.to(dev), S.to(dev), Vh.transpose(-1, -2).contiguous().to(dev)
    whole = su.pose_matrix_fisher_sampling_torch(U, S, V, 10, seed=7)
    for world in (2, 4, 8):
        step = 8 // world
        parts = [su.pose_matrix_fisher_sampling_torch(U[r * step:(r + 1) * step], S[r * step:(r + 1) * step],
                                                      V[r * step:(r + 1) * step], 10, seed=7, image_offset=r * step)
                 for r in range(world)]
        assert torch.equal(whole, torch.cat(parts)), world


def test_torch_manual_seed_controls_default_philox_seed(dev, golden):
    U, S, V = (golden[k].to(dev) for k in ("net_U", "net_S", "net_V"))
    torch.manual_seed(3)
    a = su.pose_matrix_fisher_sampling_torch(U, S, V, 5)
    torch.manual_seed(3)
    assert torch.equal(a, su.pose_matrix_fisher_sampling_torch(U, S, V, 5))


def test_stress_config_1000_samples(dev, golden):
    """BASELINE configs[4] sampler size (num_samples=1000) -- properties only."""
    U, S, V = (golden[k].to(dev) for k in ("net_U", "net_S", "net_V"))
    R = su.pose_matrix_fisher_sampling_torch(U, S, V, 1000, seed=1)
    assert R.shape == (2, 1000, 23, 3, 3) and torch.isfinite(R).all()
    assert float((torch.matmul(R.transpose(-1, -2), R) - torch.eye(3, device=dev)).abs().max()) <= 1e-5


def test_rotation_conversions_reproduce_reference(dev, golden):
    assert maxerr(rtu.rot6d_to_rotmat(golden["rot6d_in"].to(dev)), golden["rot6d_out"]) <= 1e-6
    assert maxerr(rtu.quat_to_rotmat(golden["quat_in"].to(dev)), golden["quat_out"]) <= 1e-6
    aa = torch.randn(11, 3, generator=torch.Generator().manual_seed(1))
    aa[0] = 0
    assert maxerr(rtu.batch_rodrigues(aa.to(dev)), O.batch_rodrigues(aa)) <= 1e-6
    x3 = torch.randn(3, 6, generator=torch.Generator().manual_seed(2))      # the reference is wrong at exactly B == 3
    assert maxerr(rtu.rot6d_to_rotmat(x3.to(dev)), O.rot6d_to_rotmat(x3)) <= 1e-6


def test_vertex_uncertainty_sampling_reproduces_reference(dev, golden, smpl_gpu):
    """SURVEY 8 row A9 on the GPU: compute_vertex_uncertainties_by_poseMF_shapeGaussian_sampling (sample_on_cpu=True: the
    reference's random stream) against the outputs of the REFERENCE function (utils/sampling_utils.py:146-192, oracle SMPL
    injected; tests/golden/make_golden.py), both use_mean_shape routes.  Tolerance: SMPL's 2e-5 m (vertices, joints),
    1e-5 on the uncertainty."""
    from torch.distributions import Normal
    U, S, V = (golden[k][:1].to(dev) for k in ("net_U", "net_S", "net_V"))
    dist = Normal(golden["net_shape_loc"][:1].to(dev), golden["net_shape_scale"][:1].to(dev))
    glob_R = golden["a9_glob_rotmats"].to(dev)
    for tag, mean_shape in (("mean", True), ("samp", False)):
        torch.manual_seed(5)
        unc, verts, joints = su.compute_vertex_uncertainties_by_poseMF_shapeGaussian_sampling(
            U, S, V, dist, glob_R, 4, smpl_gpu, use_mean_shape=mean_shape, sample_on_cpu=True)
        assert unc.shape == (6890,) and verts.shape == (4, 6890, 3) and joints.shape == (4, 90, 3)
        assert maxerr(verts[:, ::10], golden["a9_%s_verts_sub" % tag]) <= 2e-5, tag
        assert maxerr(joints, golden["a9_%s_joints" % tag]) <= 2e-5, tag
        assert maxerr(unc, golden["a9_%s_unc" % tag]) <= 1e-5, tag


def test_bingham_entry_accepts_caller_parameters(dev):
    """utils/sampling_utils.py:10-46: Omega / Gaussian_std / M_star are ARGUMENTS of the reference's entry point (their
    derivation from A and b is only the default).  Same host random stream, caller's envelope -> the oracle's samples."""
    A = torch.tensor([0.0, 2.76, 5.0, 5.36])
    b = 1.5
    for omega_scale, m_scale in ((1.0, 1.0), (0.7, 1.6)):
        Omega = (1.0 + 2.0 * A / b) * omega_scale
        std = Omega ** (-0.5)
        M_star = O.m_star(b) * m_scale
        torch.manual_seed(9)
        want = O.bingham_sampling(A, 16, Omega, std, M_star)
        torch.manual_seed(9)
        got, _ = su.bingham_sampling_for_matrix_fisher_torch(A.to(dev), 16, Omega=Omega.to(dev), Gaussian_std=std.to(dev), b=b,
                                                              M_star=M_star, sample_on_cpu=True)
        assert maxerr(got, want) <= 1e-6, (omega_scale, m_scale)
    # Philox route with an override: unit quaternions, finite
    q, _ = su.bingham_sampling_for_matrix_fisher_torch(A.to(dev), 64, Omega=(1.0 + 2.0 * A / b).to(dev) * 0.8, b=b, seed=4)
    assert torch.isfinite(q).all() and maxerr(q.norm(dim=-1), torch.ones(64)) <= 1e-5


def test_failed_sampling_is_loud(dev):
    """NaN concentrations make every accept test false; the Philox route must not hand back uninitialised memory."""
    from hierarchicalprobabilistic3dhuman_amd import _capi
    eye = torch.eye(3, device=dev).expand(1, 23, 3, 3).contiguous()
    S = torch.full((1, 23, 3), float("nan"), device=dev)
    R = su.pose_matrix_fisher_sampling_torch(eye, S, eye, 4, seed=1)
    assert torch.isnan(R).all()
    with pytest.raises(_capi.HpsError):
        su.check_sampling()
    R = su.pose_matrix_fisher_sampling_torch(eye, torch.ones(1, 23, 3, device=dev), eye, 4, seed=1)
    su.check_sampling()
    assert torch.isfinite(R).all()
