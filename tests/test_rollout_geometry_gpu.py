"""The kernels that move the Gaussians during a rollout (gsr_dynamics.hip: fit_bones_kernel, fit_rotations_kernel, mat2quat_unit,
lbs_kernel) through the C ABI, against the plain fp64 references of tests/dynamics_ref.py (pinned to the host path by
tests/test_dynamics_ref_cpu.py) at every size edge and every branch: both summation paths of the rotation fit, one and two workgroups,
both ballot halves, every class of degenerate neighbourhood, the half-turn branches of the quaternion conversion, the skinning's
two-Gaussians-per-thread indexing, its LDS rounds of 256 bones, its distance clamp, and the bone count read from the device.

Every bound is one the project already uses for the same comparison, named where it is used; the one new rule (half-turns) is the
project's referee rule: the device's error against fp64 is at most twice the host's on the same input.  Each test prints its worst
error next to its bound (pytest -s)."""
import numpy as np
import pytest
import torch

import dynamics_ref as ref

pytestmark = pytest.mark.gpu

# test_device_rotation_fit_matches_the_literal_decision_tree's bounds
FIT_ERR, FIT_DET, QUAT_ERR, QUAT_NORM = 2e-5, 1e-4, 3e-7, 1e-6
# test_lbs_kernel_matches_torch_path_and_goldens' bound for the skinning against fp64
LBS_RTOL, LBS_ATOL = 2e-5, 2e-6
# the end-to-end comparison of test_device_rotation_fit_matches_the_literal_decision_tree (positions, quaternions)
E2E_XYZ, E2E_QUAT = 1e-4, 5e-4


def _say(what, err, bound):
    print(f"[rollout-geometry] {what}: {err:.3g} / {bound:.3g} = {err / bound:.3f}")


def _eye(n):
    return torch.eye(3).expand(n, 3, 3)


@pytest.fixture(scope="module")
def fit_refs():
    """Per bone count: the scene, the literal host fit, the fp64 moment matrices and the expected codes -- computed once, never changed."""
    from gsdyn.dynamics import _fit_bone_rotations_loop
    cache = {}

    def get(nb):
        if nb not in cache:
            s = ref.bone_scene(nb)
            F64, n = ref.moments_ref64(s["bones"], s["motions"], s["rel"])
            cache[nb] = dict(s, want=_fit_bone_rotations_loop(s["bones"], s["motions"], s["rel"]), code=ref.classify_ref(F64.astype(np.float32), n))
        return cache[nb]
    return get


def _check_fit(tag, s, R, q, code):
    """Rotations, quaternions and codes of one gsr_fit_bones call against the scene's references."""
    from gsdyn.dynamics import mat2quat
    nb = s["bones"].shape[0]
    R, q, code = R.cpu(), q.cpu(), code.cpu()
    assert R.shape == (nb, 3, 3) and q.shape == (nb, 4) and code.shape == (nb,) and code.dtype == torch.int32
    assert torch.isfinite(R).all() and torch.isfinite(q).all()
    assert code.tolist() == s["code"].tolist(), (tag, [(i, int(a), int(b)) for i, (a, b) in enumerate(zip(code, s["code"])) if a != b])
    solved = code != 1                                    # a code 1 bone holds the identity and is the caller's to resolve
    err = (R - s["want"]).abs().amax(dim=(1, 2))[solved]
    det = (torch.linalg.det(R.double()) - 1).abs()
    _say(f"{tag} rotation vs the literal host form", float(err.max()), FIT_ERR)
    assert float(err.max()) < FIT_ERR, (tag, int(err.argmax()), float(err.max()))
    assert float(det.max()) < FIT_DET, tag
    for name in ref.IDENTITY_CLASSES + ("code1",):
        idx = ref.class_indices(s, name)
        assert torch.equal(R[idx], _eye(len(idx))), (tag, name)
        assert torch.equal(q[idx], torch.tensor([1.0, 0.0, 0.0, 0.0]).expand(len(idx), 4)), (tag, name)
    q_ref = torch.nn.functional.normalize(mat2quat(R), dim=-1)       # the host's torch expressions on the device's matrices
    _say(f"{tag} quaternion vs the host's of the same matrix", float((q - q_ref).abs().max()), QUAT_ERR)
    assert float((q - q_ref).abs().max()) < QUAT_ERR and float((q.norm(dim=-1) - 1).abs().max()) < QUAT_NORM, tag


# ------------------------------------------------------------------------------------------ 1. rotation fit at every size edge
@pytest.mark.parametrize("strided", [False, True], ids=["contiguous", "view"])
@pytest.mark.parametrize("nb", ref.FIT_SIZES_MASK + ref.FIT_SIZES_ROWS)
def test_rotation_fit_at_every_size_edge(dev, fit_refs, nb, strided):
    from diff_gaussian_rasterization import _hip
    from gsdyn.dynamics import _bone_moment_matrices, bone_transforms
    s = fit_refs(nb)
    bones, motions = s["bones"].to(dev), s["motions"].to(dev)
    if strided:                       # a window of a larger matrix whose other entries are all set: a read outside the window shows
        big = torch.ones((nb + 5, nb + 7), dtype=torch.long)
        big[2:nb + 2, 3:nb + 3] = s["rel"]
        big = big.to(dev)
        rel = big[2:nb + 2, 3:nb + 3]
        assert rel.stride(0) == nb + 7 and rel.data_ptr() != big.data_ptr() and (nb == 1 or not rel.is_contiguous())
    else:
        rel = s["rel"].to(dev)
    R, q, code = _hip.fit_bones(bones, motions, rel)
    tag = f"nb={nb} {'view' if strided else 'contiguous'}"
    _check_fit(tag, s, R, q, code)
    # code 1 bones: bone_transforms hands them to the host, and equals the literal form on EVERY bone
    R2, q2 = bone_transforms(bones, motions, rel)
    err = float((R2.cpu() - s["want"]).abs().max())
    _say(f"{tag} bone_transforms vs the literal host form", err, FIT_ERR)
    assert err < FIT_ERR and float((q2.norm(dim=-1) - 1).abs().max()) < QUAT_NORM
    if not strided:                   # gsr_fit_rotations on the HOST's moment matrices: same codes, same rotations
        F, n = _bone_moment_matrices(s["bones"], s["motions"], s["rel"])
        R3, code3 = _hip.fit_rotations(F.to(dev), n.to(dev))
        assert code3.cpu().tolist() == s["code"].tolist()
        solved = code3.cpu() != 1
        err = float((R3.cpu() - s["want"]).abs().amax(dim=(1, 2))[solved].max())
        _say(f"{tag} gsr_fit_rotations vs the literal host form", err, FIT_ERR)
        assert err < FIT_ERR


def test_rotation_fit_of_no_bones(dev):
    from diff_gaussian_rasterization import _hip
    e = lambda *sh, dt=torch.float32: torch.empty(sh, dtype=dt, device=dev)     # noqa: E731
    R, q, code = _hip.fit_bones(e(0, 3), e(0, 3), e(0, 0, dt=torch.long))
    assert R.shape == (0, 3, 3) and q.shape == (0, 4) and code.shape == (0,)
    R, code = _hip.fit_rotations(e(0, 3, 3), e(0))
    assert R.shape == (0, 3, 3) and code.shape == (0,)
    torch.cuda.synchronize(dev)


# ------------------------------------------------------------------------------------------ 2. both summation paths, the same bits
def test_mask_path_and_row_walk_give_the_same_bits(dev, fit_refs):
    """128 bones take the bit-mask path; the same bones plus a 129th, far away and related to nobody, take the row walk.  Both sum a
    bone's neighbours in ascending order: the first 128 rows are equal bit for bit."""
    from diff_gaussian_rasterization import _hip
    s = fit_refs(128)
    a = _hip.fit_bones(s["bones"].to(dev), s["motions"].to(dev), s["rel"].to(dev))
    bones = torch.cat([s["bones"], torch.tensor([[40.0, -30.0, 20.0]])])
    motions = torch.cat([s["motions"], torch.tensor([[0.25, 0.5, -0.125]])])
    rel = torch.zeros((129, 129), dtype=torch.long)
    rel[:128, :128] = s["rel"]
    b = _hip.fit_bones(bones.to(dev), motions.to(dev), rel.to(dev))
    for x, y, what in zip(a, b, ("rotations", "quaternions", "codes")):
        assert torch.equal(x, y[:128]), what
    assert torch.equal(b[0][128].cpu(), torch.eye(3)) and int(b[2][128]) == 0


# ------------------------------------------------------------------------------------------ 3. half-turns
def _check_half_turn_family(dev, fam, tag):
    """One family of stars: rotation against the literal host form, quaternion against the host's for the SAME matrix, and the referee
    rule -- the matrix of the device's quaternion is at most twice as far (+ 1e-6) from the device's matrix, in fp64, as the host's
    quaternion's is.  -> (branches the matrices take, worst device / host error ratio)."""
    from diff_gaussian_rasterization import _hip
    from gsdyn.dynamics import _fit_bone_rotations_loop, mat2quat
    R, q, code = _hip.fit_bones(fam["bones"].to(dev), fam["motions"].to(dev), fam["rel"].to(dev))
    stars = fam["stars"]
    R, q = R.cpu()[stars], q.cpu()[stars]
    assert code.cpu()[stars].tolist() == [2] * len(stars)
    want = _fit_bone_rotations_loop(fam["bones"], fam["motions"], fam["rel"])[stars]
    err = float((R - want).abs().max())
    _say(f"{tag}: rotation vs the literal host form", err, FIT_ERR)
    assert err < FIT_ERR and float((torch.linalg.det(R.double()) - 1).abs().max()) < FIT_DET
    q_host = torch.nn.functional.normalize(mat2quat(R), dim=-1)
    _say(f"{tag}: quaternion vs the host's of the same matrix", float((q - q_host).abs().max()), QUAT_ERR)
    assert float((q - q_host).abs().max()) < QUAT_ERR and float((q.norm(dim=-1) - 1).abs().max()) < QUAT_NORM
    R64 = R.double().numpy()
    e_dev = np.abs(ref.quat_to_mat64(q.numpy()) - R64).max(axis=(1, 2))
    e_host = np.abs(ref.quat_to_mat64(q_host.numpy()) - R64).max(axis=(1, 2))
    branch = ref.mat2quat_branch(R.numpy())
    worst = 0.0
    for (axis, gap), d, h, b in zip(fam["labels"], e_dev, e_host, branch):
        print(f"[rollout-geometry] {tag} axis ({axis[0]:.2f}, {axis[1]:.2f}, {axis[2]:.2f}) pi - {gap:g} branch {b}: device {d:.3g} host {h:.3g}")
        worst = max(worst, (d - 1e-6) / max(h, 1e-30))
        assert d <= 2 * h + 1e-6, (tag, axis, gap, d, h)
    print(f"[rollout-geometry] {tag}: worst (device error - 1e-6) / host error = {worst:.3f} (bound 2)")
    return branch, worst


def test_half_turns_take_their_own_branches(dev):
    """Exact half-turns about the coordinate axes: the fit returns diag(1,-1,-1), diag(-1,1,-1), diag(-1,-1,1) exactly and mat2quat_unit
    its second, third and fourth branch: (0,1,0,0), (0,0,1,0), (0,0,0,1) exactly.
    Near half-turns (pi - 1e-1 .. 3e-4 about five axes) and exact half-turns about 30 tilted axes (the half-turn branches with non-zero
    off-diagonal sums): the device's quaternion within 3e-7 of the host's for the same matrix, and the referee rule of
    _check_half_turn_family, which prints both errors per star and the worst ratio.
    Measured on the MI355X: worst (device error - 1e-6) / host error = 1.000 in both families (bound 2); the quaternions differ from the
    host's by 0 (near) and 6e-8 (tilted: one rounding of the norm).  The error itself reaches 2.0 in the half-turn branches, on the host
    as on the device: the reference's formulas there are not the rotation's quaternion, and the project reproduces them."""
    from diff_gaussian_rasterization import _hip
    exact, near, tilted = ref.half_turn_stars()
    R, q, code = _hip.fit_bones(exact["bones"].to(dev), exact["motions"].to(dev), exact["rel"].to(dev))
    stars = exact["stars"]
    assert code.cpu()[stars].tolist() == [2, 2, 2]
    assert torch.equal(R.cpu()[stars], exact["rotations"]), R.cpu()[stars]
    assert torch.equal(q.cpu()[stars], exact["quats"]), q.cpu()[stars]
    others = [i for i in range(exact["bones"].shape[0]) if i not in stars]
    assert torch.equal(R.cpu()[others], _eye(len(others))) and code.cpu()[others].tolist() == [0] * len(others)
    _check_half_turn_family(dev, near, "near half-turns")
    branch, _ = _check_half_turn_family(dev, tilted, "tilted half-turns")
    # the signed permutations are exact; among the others every half-turn branch is taken (which star takes which hangs on the last bit
    # of its trace: the host's matrices take them 4, 7 and 6 times, tests/test_dynamics_ref_cpu.py asserts at least twice each)
    assert branch[:3].tolist() == [1, 2, 1] and all((branch[3:] == k).any() for k in (1, 2, 3)), branch


# ------------------------------------------------------------------------------------------ 4. skinning at every size edge
def _skin(dev, c, quat=True, **kw):
    from diff_gaussian_rasterization import _hip
    return _hip.linear_blend_skinning(c["bones"].to(dev), c["R"].to(dev), c["t"].to(dev), c["bq"].to(dev), c["xyz"].to(dev),
                                      c["quat"].to(dev) if quat else None, **kw)


def _close(tag, got, want):
    got = got.cpu().numpy()
    assert np.isfinite(got).all(), tag
    excess = np.abs(got - want) / (LBS_ATOL + LBS_RTOL * np.abs(want))
    _say(tag, float(excess.max()), 1.0)
    np.testing.assert_allclose(got, want, rtol=LBS_RTOL, atol=LBS_ATOL, err_msg=tag)


@pytest.mark.parametrize("P,nb", ref.SKIN_SIZES)
def test_skinning_at_every_size_edge(dev, P, nb):
    c = ref.skinning_case(P, nb)
    want_x, want_q = ref.lbs_ref64(c["bones"], c["R"], c["t"], c["bq"], c["xyz"], c["quat"])
    x, q, _ = _skin(dev, c)
    assert x.shape == (P, 3) and q.shape == (P, 4)
    for name, (a, b) in c["ranges"].items():          # group by group: on a bone, inside / across the clamp, underflow, free
        if a < b:
            _close(f"P={P} nb={nb} {name} xyz", x[a:b], want_x[a:b])
            _close(f"P={P} nb={nb} {name} quat", q[a:b], want_q[a:b])
    x2, q2, _ = _skin(dev, c, quat=False)
    assert q2 is None and torch.equal(x2, x)


# ------------------------------------------------------------------------------------------ 5. the bone count read from the device
@pytest.fixture(scope="module")
def case300():
    return ref.skinning_case(700, 300)


@pytest.mark.parametrize("n_valid", [300, 299, 257, 256, 255, 1])
def test_skinning_with_a_device_bone_count(dev, case300, n_valid):
    c = case300
    x, q, _ = _skin(dev, c, n_valid=torch.tensor([n_valid], dtype=torch.int32, device=dev))
    head = dict(c, **{k: c[k][:n_valid] for k in ("bones", "R", "t", "bq")})
    x1, q1, _ = _skin(dev, head)
    assert torch.equal(x, x1) and torch.equal(q, q1)
    want_x, want_q = ref.lbs_ref64(c["bones"], c["R"], c["t"], c["bq"], c["xyz"], c["quat"], n_valid=n_valid)
    _close(f"n_valid={n_valid} xyz", x, want_x)
    _close(f"n_valid={n_valid} quat", q, want_q)


def test_a_bone_count_above_the_array_means_all_of_it(dev, case300):
    a = _skin(dev, case300, n_valid=torch.tensor([400], dtype=torch.int32, device=dev))
    b = _skin(dev, case300, n_valid=torch.tensor([300], dtype=torch.int32, device=dev))
    c = _skin(dev, case300)
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1]) and torch.equal(a[0], c[0]) and torch.equal(a[1], c[1])


def test_no_valid_bone_means_nobody_moves(dev):
    """*n_valid = 0: the inputs pass through bit for bit (gsr.h), out of place and in place -- not the NaN of 0 * (1 / 0)."""
    c = ref.skinning_case(513, 100)
    zero = torch.tensor([0], dtype=torch.int32, device=dev)
    xyz, quat = c["xyz"].to(dev), c["quat"].to(dev)
    x, q, _ = _skin(dev, c, n_valid=zero)
    assert torch.isfinite(x).all() and torch.isfinite(q).all()
    assert torch.equal(x, xyz) and torch.equal(q, quat) and x.data_ptr() != xyz.data_ptr()
    x2, q2, _ = _skin(dev, c, quat=False, n_valid=zero)
    assert q2 is None and torch.equal(x2, xyz)
    from diff_gaussian_rasterization import _hip
    xi, qi = xyz.clone(), quat.clone()
    _hip.linear_blend_skinning(c["bones"].to(dev), c["R"].to(dev), c["t"].to(dev), c["bq"].to(dev), xi, qi, n_valid=zero, in_place=True)
    assert torch.equal(xi, xyz) and torch.equal(qi, quat)


# ------------------------------------------------------------------------------------------ 6. a Gaussian's result is its own
def test_a_gaussians_result_does_not_depend_on_its_row(dev):
    """513 Gaussians alone and as rows 100 .. 612 of a 1025-row call: other threads, other halves of the two-per-thread pairs, the same
    bits.  In place and into given outputs: the same bits as out of place."""
    from diff_gaussian_rasterization import _hip
    c = ref.skinning_case(513, 100)
    x, q, _ = _skin(dev, c)
    g = torch.Generator().manual_seed(9)
    big_x = torch.rand(1025, 3, generator=g)
    big_q = torch.nn.functional.normalize(torch.randn(1025, 4, generator=g), dim=-1)
    big_x[100:613], big_q[100:613] = c["xyz"], c["quat"]
    bx, bq_, _ = _skin(dev, dict(c, xyz=big_x, quat=big_q))
    assert torch.equal(bx[100:613], x) and torch.equal(bq_[100:613], q)
    args = [c[k].to(dev) for k in ("bones", "R", "t", "bq")]
    xi, qi = c["xyz"].to(dev).clone(), c["quat"].to(dev).clone()
    ri = _hip.linear_blend_skinning(*args, xi, qi, in_place=True)
    assert ri[0].data_ptr() == xi.data_ptr() and torch.equal(xi, x) and torch.equal(qi, q)
    ox, oq = torch.full((513, 3), float("nan"), device=dev), torch.full((513, 4), float("nan"), device=dev)
    ro = _hip.linear_blend_skinning(*args, c["xyz"].to(dev), c["quat"].to(dev), out=(ox, oq))
    assert ro[0].data_ptr() == ox.data_ptr() and torch.equal(ox, x) and torch.equal(oq, q)


# ------------------------------------------------------------------------------------------ 7. as production calls it
def test_interpolate_motions_with_bones_sampled_from_the_gaussians(dev):
    """100 bones picked from 3000 Gaussians by farthest point sampling (every bone has a Gaussian at distance exactly 0), relations by
    distance: gsr_fit_bones + gsr_lbs on the device against fp64 skinning with the literal host form's rotations."""
    from gsdyn.dynamics import _fit_bone_rotations_loop, farthest_point_sampler, interpolate_motions, mat2quat
    g = torch.Generator().manual_seed(21)
    P = 3000
    xyz = torch.rand(P, 3, generator=g) * torch.tensor([0.6, 0.4, 0.1])
    quat = torch.nn.functional.normalize(torch.randn(P, 4, generator=g), dim=-1)
    idx = farthest_point_sampler(xyz[None], 100, start_idx=0)[0]
    assert idx.unique().numel() == 100
    bones = xyz[idx].clone()
    Rz = torch.tensor(ref.axis_angle64([0.2, 0.1, 1.0], 0.3), dtype=torch.float32)
    motions = (bones - 0.3) @ Rz.T + 0.3 + 0.002 * torch.randn(100, 3, generator=g) - bones
    rel = (torch.cdist(bones.double(), bones.double()) < 0.3).long()
    # the scene's own precondition: every bone a clear rank 3 (no decision of this test hangs on rounding)
    F64, n = ref.moments_ref64(bones, motions, rel)
    S = ref.singular_values64(F64.astype(np.float32))
    assert (n >= 4).all() and (S[:, 2] > ref.RANK_CLEAR * S[:, 0]).all() and (np.linalg.det(F64) > 0).all()
    x, q, _ = interpolate_motions(bones.to(dev), motions.to(dev), rel.to(dev), xyz.to(dev), quat=quat.to(dev))
    R = _fit_bone_rotations_loop(bones, motions, rel)
    bq = torch.nn.functional.normalize(mat2quat(R), dim=-1)
    want_x, want_q = ref.lbs_ref64(bones, R, motions, bq, xyz, quat)
    assert torch.isfinite(x).all() and torch.isfinite(q).all()
    ex, eq = float(np.abs(x.cpu().numpy() - want_x).max()), float(np.abs(q.cpu().numpy() - want_q).max())
    _say("production shape xyz", ex, E2E_XYZ)
    _say("production shape quat", eq, E2E_QUAT)
    assert ex < E2E_XYZ and eq < E2E_QUAT
    on = np.abs(x.cpu().numpy()[idx] - want_x[idx]).max()          # the Gaussians that ARE bones
    _say("production shape xyz, Gaussians on a bone", float(on), E2E_XYZ)
