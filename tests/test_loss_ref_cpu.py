"""Pins tests/loss_ref.py, the fp64 reference of the image-loss kernels, without a GPU: against the package's torch formulas
(calc_ssim, l1_loss_v1: another implementation, conv2d with a 2-D window), against the vectors stored from the imported reference,
against a brute-force 2-D window sum; and checks the precondition of the GPU file's referee rule -- the same statements in fp32 meet
the plain bounds on every random-content case, so a HIP result that misses them there is a finding about the kernel."""
import os

import numpy as np
import pytest
import torch

import loss_ref as R

TOL = 1e-4       # gradients and moments: of the tensor's (per-image) maximum, as tests/hipcheck.py


def _package_total(s, dtype=torch.float64):
    from gsdyn import losses as L
    r = s["renders"].to(dtype).requires_grad_(True)
    m, c = s["cam_m"].to(dtype).requires_grad_(True), s["cam_c"].to(dtype).requires_grad_(True)
    per = []
    for i, (t, row) in enumerate(zip(s["targets"], s["rows"])):
        pred = r[i] if row < 0 else torch.exp(m[row])[:, None, None] * r[i] + c[row][:, None, None]
        per.append(0.8 * L.l1_loss_v1(pred, t.to(dtype)) + 0.2 * (1.0 - L.calc_ssim(pred, t.to(dtype))))
    total = sum(w * l for w, l in zip(s["weights"], per))
    grads = torch.autograd.grad(total, (r, m, c))
    return total.detach(), torch.stack(per).detach(), grads


@pytest.mark.parametrize("H,W", [(1, 1), (5, 6), (11, 33), (55, 37), (60, 65)])
def test_reference_equals_the_package_formulas_in_fp64(H, W):
    s = R.views_scene(H, W, n=3, rows=[1, -1, 1])
    total, per, grads = _package_total(s)
    ref = R.reference_of(s)
    # the package's 2-D window is the outer product ROUNDED to fp32, the reference applies the fp32 taps twice in fp64: 6e-8 per weight
    assert abs(float(total) - float(ref["total"])) <= 1e-6 * abs(float(ref["total"]))
    assert float((per - ref["per"]).abs().max()) <= 1e-6 * float(ref["per"].abs().max())
    for a, k in zip(grads, ("d_renders", "d_cam_m", "d_cam_c")):
        assert R.grad_err(a, ref[k]) <= 1e-5, k
    assert float(ref["d_cam_m"][0].abs().max()) == 0.0 and float(ref["d_cam_m"][1].abs().max()) > 0.0


def test_reference_equals_the_stored_vectors_of_the_imported_reference(golden_dir):
    g = np.load(os.path.join(golden_dir, "reference_host.npz"))
    x, y = torch.tensor(g["ssim_im1"]), torch.tensor(g["ssim_im2"])
    ssim = R.views_reference(x[None], [y], [-1], [1.0], w_l1=0.0, w_ssim=1.0)
    np.testing.assert_allclose(1.0 - float(ssim["total"]), float(g["ssim"]), rtol=2e-5)
    assert R.grad_err(-ssim["d_renders"][0], torch.tensor(g["ssim_grad"])) <= TOL
    both = R.views_reference(x[None], [y], [-1], [1.0])
    np.testing.assert_allclose(float(both["total"]), float(g["im_term"]), rtol=2e-5)


def test_separable_window_equals_the_brute_force_2d_sum():
    rng = np.random.default_rng(5)
    for H, W in ((13, 7), (4, 12), (1, 1)):
        x, y = rng.uniform(0, 1, (H, W)), rng.uniform(0, 1, (H, W))
        for img in (x, x * x, x * y):
            got = R.blur(torch.tensor(img)).numpy()
            np.testing.assert_allclose(got, R.blur_brute(img), rtol=1e-13, atol=1e-15)
        # ... and the whole SSIM map from brute-force moments
        A, B = R.blur_brute(x), R.blur_brute(y)
        sxx, syy, sxy = R.blur_brute(x * x) - A * A, R.blur_brute(y * y) - B * B, R.blur_brute(x * y) - A * B
        m = ((2 * A * B + R.C1) * (2 * sxy + R.C2)) / ((A * A + B * B + R.C1) * (sxx + syy + R.C2))
        np.testing.assert_allclose(R.ssim_map(torch.tensor(x)[None], torch.tensor(y)[None])[0].numpy(), m, rtol=1e-10)


def test_target_moments_and_l1_ties():
    y = torch.tensor(np.random.default_rng(2).uniform(0, 1, (2, 12, 9)).astype(np.float32))
    B, D = R.target_moments(y)
    np.testing.assert_allclose(B[1].numpy(), R.blur_brute(y[1].double().numpy()), rtol=1e-13)
    np.testing.assert_allclose(D[0].numpy(), R.blur_brute((y[0].double() ** 2).numpy()), rtol=1e-13)
    render, target, tie = R.tie_scene()
    assert bool((render[0][tie] == target[tie]).all()) and bool((render[0][~tie] != target[~tie]).all())
    W = render.shape[-1]
    assert bool((render[0] >= target)[..., : W // 2].all()) and bool((render[0] <= target)[..., W // 2:].all())
    g = R.views_reference(render, [target], [-1], [1.0], w_l1=0.8, w_ssim=0.0, dtype=torch.float32)["d_renders"][0]
    n = float(render[0].numel())
    assert bool((g[tie] == 0).all()) and set(np.unique(g[~tie].numpy()).tolist()) == {-float(np.float32(0.8)) / n, float(np.float32(0.8)) / n}


def test_scene_tables_hit_the_sizes_they_are_named_for():
    assert sorted(R.SLOT_CASES) == [1, 7, 8, 9, 15, 16, 17]
    for N in R.SLOT_CASES:
        s = R.slot_scene(N)
        n, C, H, W = s["renders"].shape
        assert R.tiles_times_planes(H, W, C, n) == N
        flat = s["renders"].reshape(n * C, -1)
        assert len({tuple(p.tolist()) for p in flat}) == n * C                  # every plane distinct
    for k in R.FINISH_K1:
        assert R.tiles_times_planes(3, 32 * k - 5, 1, 1) == k
    assert max(32 * k - 5 for k in R.FINISH_K1) == 16411
    t = R.table_cases()
    assert t["full-32x4"][0] * t["full-32x4"][1] == 128 and set(t["one-row"][2]) == {0} and t["descending"][2] == sorted(t["descending"][2], reverse=True)
    assert all(r == -1 for r in t["no-rows"][2]) and all(4 not in c[2] for k, c in t.items() if k.startswith("n"))
    w = R.table_scene("n17")["weights"]
    assert min(w) < 0 < max(w) and 0.0 in w
    for N, C in R.BATCH_CASES:
        w = R.batch_scene(N, C)["weights"]
        assert len(set(w)) == N


def test_fp32_yardstick_meets_the_plain_bounds_on_every_random_case():
    """The referee rule's precondition: the reference's statements in fp32 on the CPU are inside the value bound and inside TOL of the
    per-image maximum on every random-content case that the GPU file holds to the plain bounds."""
    worst_v, worst_g, over = 0.0, 0.0, []
    for tag, build in R.random_cases():
        s = build()
        r64, r32 = R.reference_of(s, upstream=0.7), R.reference_of(s, upstream=0.7, dtype=torch.float32)
        ev = max(abs(float(a) - float(b)) / max(abs(float(b)), 1e-300) for a, b in zip(r32["per"], r64["per"]))
        scale = r64["d_renders"].abs().amax(dim=(1, 2, 3)).clamp_min(1e-300)
        eg = float(((r32["d_renders"] - r64["d_renders"]).abs().amax(dim=(1, 2, 3)) / scale).max())
        for k in ("d_cam_m", "d_cam_c"):
            if float(r64[k].abs().max()) > 0:
                eg = max(eg, R.grad_err(r32[k], r64[k]))
        ok_v = all(R.value_ok(float(a), float(b)) for a, b in zip(r32["per"], r64["per"])) and R.value_ok(float(r32["total"]), float(r64["total"]))
        if not ok_v or eg > TOL:
            over.append((tag, ev, eg))
        worst_v, worst_g = max(worst_v, ev), max(worst_g, eg)
    print(f"fp32 yardstick over {len(R.random_cases())} cases: worst value {worst_v:.2e} relative, worst gradient {worst_g:.2e} of max |g|")
    assert not over, over
