"""The yardstick of tests/test_rollout_geometry_gpu.py, checked without a GPU: the fp64 references and the scene builders of
tests/dynamics_ref.py against the host path of gsdyn/dynamics.py (which tests/test_dynamics_cpu.py pins to the reference's goldens)."""
import numpy as np
import pytest
import torch

import dynamics_ref as ref


@pytest.fixture(scope="module")
def scenes():
    return {nb: ref.bone_scene(nb) for nb in ref.FIT_SIZES_MASK + ref.FIT_SIZES_ROWS}


@pytest.mark.parametrize("nb", ref.FIT_SIZES_MASK + ref.FIT_SIZES_ROWS)
def test_bone_scene_classes_are_what_they_claim(scenes, nb):
    from gsdyn.dynamics import _bone_moment_matrices, _fit_bone_rotations_loop, fit_bone_rotations
    s = scenes[nb]
    bones, motions, rel = s["bones"], s["motions"], s["rel"]
    assert bones.shape == (nb, 3) and rel.shape == (nb, nb) and bones.dtype == torch.float32
    covered = sorted(i for name in s["ranges"] for i in ref.class_indices(s, name))
    assert covered == list(range(nb))                     # every bone belongs to exactly one class
    if nb >= 63:
        assert set(s["ranges"]) == set(ref.CLASS_CODE)    # all eight classes
        for name in ref.CLASS_CODE:
            if name != "generic":
                assert len(s["ranges"][name]) == 2        # one group at the low indices, one at the high ones
        assert max(ref.class_indices(s, "generic")) < nb - 1
    if nb >= 100:
        for name in ref.CLASS_CODE:
            assert max(ref.class_indices(s, name)) >= 64, name          # the second ballot half / the second workgroup sees every class
            assert min(ref.class_indices(s, name)) < 64, name
    want = _fit_bone_rotations_loop(bones, motions, rel)
    got = fit_bone_rotations(bones, motions, rel)
    assert float((got - want).abs().max()) <= 1e-6        # (test_fit_bone_rotations_vectorised_equals_literal_form's bound)
    # the fp64 moment matrices against the host's fp32 ones; exactly equal where the class is exactly degenerate
    F64, n = ref.moments_ref64(bones, motions, rel)
    F_host, n_host = _bone_moment_matrices(bones, motions, rel)
    assert np.array_equal(n, n_host.numpy())
    assert np.abs(F64 - F_host.double().numpy()).max() <= 8 * 4 * ref.EPS32 * max(1.0, np.abs(F64).max())   # <= 8 fp32 terms of size <= max|F|
    F32 = F64.astype(np.float32)
    code = ref.classify_ref(F32, n)
    assert np.array_equal(code, ref.classify_ref(F_host.numpy(), n_host.numpy()))
    eye = torch.eye(3)
    S = ref.singular_values64(F32)
    for name, expect in ref.CLASS_CODE.items():
        idx = ref.class_indices(s, name)
        if not idx:
            continue
        assert (code[idx] == expect).all(), (name, code[idx])
        if name in ("one_neighbour", "collinear", "coincident", "code1"):
            assert np.array_equal(F32[idx], F_host.numpy()[idx]), name
        if name == "code1":                               # rank 1 with a zero first column: whatever the host's LAPACK makes of it
            assert (F32[idx][:, :, 0] == 0).all() and (S[idx, 0] > 0).all() and (S[idx, 1] < ref.SVD_ZERO * S[idx, 0]).all()
            continue
        R = want[idx]
        if name in ref.IDENTITY_CLASSES:
            assert torch.equal(R, eye.expand(len(idx), 3, 3)), name
            continue
        Rd = R.double()
        assert float((Rd @ Rd.transpose(1, 2) - torch.eye(3, dtype=torch.float64)).abs().max()) < 1e-5, name
        assert float((torch.linalg.det(Rd) - 1).abs().max()) < 1e-5, name
        if expect == 3:                                   # the x axis lands on the line the neighbours end up on
            for i, Ri in zip(idx, Rd):
                u, _, _ = np.linalg.svd(F64[i])
                assert abs(abs(float(Ri[:, 0] @ torch.tensor(u[:, 0]))) - 1) < 1e-6, (name, i)
        if name == "coplanar":
            assert (S[idx, 2] < ref.SVD_ZERO * S[idx, 0]).all() and (S[idx, 1] > ref.RANK_CLEAR * S[idx, 0]).all()
        if name == "generic":
            assert (S[idx, 2] > ref.RANK_CLEAR * S[idx, 0]).all() and (np.linalg.det(F64[idx]) > 0).all()
    if "mirrored" in s["ranges"]:
        idx = ref.class_indices(s, "mirrored")
        assert (S[idx, 2] > ref.RANK_CLEAR * S[idx, 0]).all() and (np.linalg.det(F64[idx]) < 0).all()


def test_classify_ref_on_hand_made_matrices():
    F = np.zeros((6, 3, 3), dtype=np.float32)
    F[0] = np.diag([1, 2, 3])                            # full rank, det > 0
    F[1] = np.diag([1, 2, -3])                           # full rank, det < 0
    F[2] = np.diag([1, 2, 0])                            # rank 2
    F[3] = np.outer([1, 2, 3], [1, 0, 0])                # rank 1
    F[4] = np.outer([1, 2, 3], [0, 1, 0])                # rank 1, first column zero
    F[5] = np.diag([1, 2, 3])                            # no neighbour
    assert ref.classify_ref(F, [3, 3, 3, 1, 1, 0]).tolist() == [2, 0, 2, 3, 1, 0]
    assert ref.classify_ref(np.zeros((1, 3, 3), np.float32), [2]).tolist() == [0]
    # the rank rule is the reference's: a third singular value of 2 eps_fp32 of the first does not count, one of 6 eps_fp32 does
    assert ref.classify_ref(np.diag([1, 1, -2 * ref.EPS32])[None], [3]).tolist() == [2]
    assert ref.classify_ref(np.diag([1, 1, -6 * ref.EPS32])[None], [3]).tolist() == [0]


@pytest.mark.parametrize("P,nb", ref.SKIN_SIZES)
def test_lbs_ref64_against_the_host_skinning(P, nb):
    from gsdyn.dynamics import blend_skinning
    c = ref.skinning_case(P, nb)
    assert c["xyz"].shape == (P, 3) and c["bones"].shape == (nb, 3)
    r = c["ranges"]
    assert list(r) == list(ref.GAUSSIAN_GROUPS) and r["on_bone"][0] == 0 and r["free"][1] == P
    assert all(r[a][1] == r[b][0] for a, b in zip(ref.GAUSSIAN_GROUPS, ref.GAUSSIAN_GROUPS[1:]))
    if P >= 255:                                          # every group is there, and is what it says
        X, B = c["xyz"].double(), c["bones"].double()
        dmin = (X[:, None] - B[None]).norm(dim=-1).min(1).values
        seg = lambda k: dmin[r[k][0]:r[k][1]]            # noqa: E731
        assert len(seg("on_bone")) >= 2 and bool((seg("on_bone") == 0).all())
        assert len(seg("inside_clamp")) >= 2 and bool(((seg("inside_clamp") > 2e-5) & (seg("inside_clamp") < 4e-5)).all())
        assert len(seg("across_clamp")) >= 2 and bool(((seg("across_clamp") - 1e-4).abs() < 4e-7).all())
        assert len(seg("underflow")) >= 1 and bool(((seg("underflow") > 0) & (seg("underflow") < 1e-24)).all())
    want_x, want_q = ref.lbs_ref64(c["bones"], c["R"], c["t"], c["bq"], c["xyz"], c["quat"])
    got_x, got_q, _ = blend_skinning(c["bones"], c["R"], c["t"], c["bq"], c["xyz"], c["quat"])
    for name, (a, b) in r.items():
        if a == b:
            continue
        # test_lbs_kernel_matches_torch_path_and_goldens' bound for this comparison
        np.testing.assert_allclose(got_x[a:b].numpy(), want_x[a:b], rtol=2e-5, atol=2e-6, err_msg=name)
        np.testing.assert_allclose(got_q[a:b].numpy(), want_q[a:b], rtol=2e-5, atol=2e-6, err_msg=name)
    # n_valid = a prefix of the bones; without quaternions the positions are the same
    k = max(1, nb // 2)
    cut_x, _ = ref.lbs_ref64(c["bones"], c["R"], c["t"], c["bq"], c["xyz"], None, n_valid=k)
    pre_x, pre_q = ref.lbs_ref64(c["bones"][:k], c["R"][:k], c["t"][:k], c["bq"][:k], c["xyz"], c["quat"])
    assert pre_q is not None and np.array_equal(cut_x, pre_x)
    assert np.array_equal(ref.lbs_ref64(c["bones"], c["R"], c["t"], c["bq"], c["xyz"], None, n_valid=nb + 7)[0], want_x)


def test_half_turn_stars_on_the_host():
    from gsdyn.dynamics import _fit_bone_rotations_loop, bone_transforms, mat2quat
    exact, near, tilted = ref.half_turn_stars()
    F, n = ref.moments_ref64(exact["bones"], exact["motions"], exact["rel"])
    for k, c in enumerate(exact["stars"]):
        assert np.array_equal(F[c], 0.125 * np.diag(ref.HALF_TURN_DIAGS[k])) and n[c] == 6
    R, q = bone_transforms(exact["bones"], exact["motions"], exact["rel"])
    assert torch.equal(R[exact["stars"]], exact["rotations"])
    assert torch.equal(q[exact["stars"]], exact["quats"])
    assert torch.equal(_fit_bone_rotations_loop(exact["bones"], exact["motions"], exact["rel"])[exact["stars"]], exact["rotations"])
    others = [i for i in range(exact["bones"].shape[0]) if i not in exact["stars"]]
    assert torch.equal(R[others], torch.eye(3).expand(len(others), 3, 3))
    # each of the three takes a half-turn branch of its own: trace = -1, and the largest diagonal element is a different one
    d = torch.diagonal(exact["rotations"], dim1=1, dim2=2)
    assert d.sum(1).tolist() == [-1.0] * 3 and d.argmax(1).tolist() == [0, 1, 2]
    # the near half-turns: the fit returns the rotation the star was turned by, and the quaternion is that rotation's
    assert len(near["stars"]) == len(ref.NEAR_HALF_TURN_AXES) * len(ref.NEAR_HALF_TURN_GAPS) and near["bones"].shape[0] <= 128
    Rn, qn = bone_transforms(near["bones"], near["motions"], near["rel"])
    Rn, qn = Rn[near["stars"]], qn[near["stars"]]
    assert float((Rn.double() - near["rotations"]).abs().max()) < 2e-6
    tr = torch.diagonal(Rn, dim1=1, dim2=2).sum(1)
    assert float(tr.max()) < -0.98 and int((mat2quat(Rn)[:, 0].abs() < 0.06).sum()) == len(near["stars"])     # w = cos(angle / 2) is tiny
    for (ax, gap), Ri, qi in zip(near["labels"], Rn, qn):
        err = np.abs(ref.quat_to_mat64(qi.numpy()) - Ri.double().numpy()).max()
        # mat2quat near a half-turn is ill-conditioned: w = sqrt(trace + 1) / 2, and the fitted matrix's entries are known to E = 2e-6
        # (asserted above), its trace to 3 E: w is off by at most sqrt(3 E) / 2, the matrix of the quaternion (terms 2 w x) by sqrt(3 E)
        assert err < 1e-5 + np.sqrt(3 * 2e-6), (ax, gap, err)


def test_quat_to_mat64_and_axis_angle64():
    from gsdyn.dynamics import quat2mat
    g = torch.Generator().manual_seed(0)
    q = torch.nn.functional.normalize(torch.randn(50, 4, generator=g, dtype=torch.float64), dim=-1)
    assert np.abs(ref.quat_to_mat64(q.numpy()) - quat2mat(q).numpy()).max() < 1e-14
    R = ref.axis_angle64([0.0, 0.0, 2.0], 0.3)
    assert np.allclose(R, [[np.cos(0.3), -np.sin(0.3), 0], [np.sin(0.3), np.cos(0.3), 0], [0, 0, 1]], atol=1e-15)
    assert np.allclose(ref.quat_to_mat64([np.cos(0.15), 0, 0, np.sin(0.15)]), R, atol=1e-15)


def test_tilted_half_turns_reach_every_half_turn_branch():
    """The exact half-turns about tilted axes: on the host the fitted matrices take each of mat2quat's three half-turn branches several
    times (which ones exactly hangs on the last bit of the trace; the GPU file asserts the same of the device's matrices)."""
    from gsdyn.dynamics import bone_transforms, mat2quat
    _, _, tilted = ref.half_turn_stars()
    assert tilted["bones"].shape[0] <= 128                # the bit-mask path
    R, q = bone_transforms(tilted["bones"], tilted["motions"], tilted["rel"])
    R, q = R[tilted["stars"]], q[tilted["stars"]]
    assert float((R.double() - tilted["rotations"]).abs().max()) < 2e-6
    br = ref.mat2quat_branch(R.numpy())
    # the three signed permutations are exact: trace = -1, branches x, y, x
    assert br[:3].tolist() == [1, 2, 1] and torch.equal(R[:3], tilted["rotations"][:3].round().float())
    assert all(int((br[3:] == k).sum()) >= 2 for k in (1, 2, 3)), br
    # mat2quat_branch is the host's decision: the host's quaternion is the branch's formula
    m = R[br == 2]
    h = 0.5 / torch.sqrt(1 + m[:, 1, 1] - m[:, 0, 0] - m[:, 2, 2])
    want = torch.stack([(m[:, 0, 2] - m[:, 2, 0]) * h, (m[:, 2, 1] + m[:, 1, 2]) * h, 0.5 * h, (m[:, 0, 1] + m[:, 1, 0]) * h], -1)
    assert torch.equal(mat2quat(m), want) and float(want[:, 1].abs().min()) > 0.05
