"""The reference of the propagation network's GPU suite (tests/gnn_ref.py) is itself checked here, without a GPU: against the torch module
in fp64 at every configuration of the matrix, against the committed goldens, and its fp32 statement of the aggregation kernel against the
derived bound.  The yardstick y_c of tests/test_gnn_kernels_gpu.py -- the host fp32 network's own distance from fp64 -- is printed per
configuration and capped."""
import copy
import os

import numpy as np
import pytest
import torch

import gnn_ref


@pytest.mark.parametrize("name", list(gnn_ref.CONFIGS))
def test_reference_equals_the_fp64_module(name):
    c = gnn_ref.case(name)
    m64 = copy.deepcopy(c["model"]).double()
    with torch.no_grad():
        for s, (ref_pos, ref_mot) in zip(c["sets"], c["refs"]):
            assert s["recv"].shape[0] > s["a"].shape[0]
            pos, mot = m64._propagate(s["state_t"].double(), s["a"].double(), s["g"].double(), s["act"].double(), s["recv"], s["send"])
            assert ref_pos.shape == (gnn_ref.N_OBJ + 1, 3) and ref_mot.shape == ref_pos.shape and np.abs(ref_mot).max() > 0
            for got, want in ((ref_mot, mot.numpy()), (ref_pos, pos.numpy())):
                assert np.abs(got - want).max() <= 1e-12 * np.abs(want).max(), name


@pytest.mark.parametrize("name", list(gnn_ref.CONFIGS))
def test_yardstick_is_capped(name):
    """y_c <= 1e-6 caps the conditioning of the seeded case (a badly conditioned one would make 4 y_c a loose bound); it is no measurement."""
    c = gnn_ref.case(name)
    print(f"{name}: y_c = {c['y']:.3e} of the largest motion, positions {c['p_y']:.3e} absolute "
          f"(relations per set: {[int(s['recv'].shape[0]) for s in c['sets']]})")
    assert 0.0 < c["y"] <= 1e-6, (name, c["y"])


def test_reference_equals_the_goldens(golden_dir):
    from gsdyn.dynamics import construct_edges
    gold = np.load(os.path.join(golden_dir, "dynamics_host.npz"))
    cfg = {str(k): int(v) for k, v in zip(gold["gnn_cfg_keys"], gold["gnn_cfg_vals"])}
    w = {k[len("gnn_w_"):]: gold[k] for k in gold.files if k.startswith("gnn_w_")}
    states = torch.tensor(gold["edge_states"])
    N = states.shape[0]
    mask, tool = torch.ones(N, dtype=torch.bool), torch.zeros(N, dtype=torch.bool)
    tool[N - 1] = True
    recv, send = construct_edges(states, 0.08, mask, tool, topk=5, connect_all=False)
    state = gold["gnn_state"][0]                                            # [n_his, N, 3]
    state_t = state.transpose(1, 0, 2).reshape(N, -1)
    g = np.concatenate([np.ones((N - 1, 1)), np.zeros((1, 1))], 0)
    pos, mot = gnn_ref.propagate(w, cfg, state_t, gold["gnn_attrs"][0], g, gold["gnn_action"][0], recv.numpy(), send.numpy())
    np.testing.assert_allclose(pos[:N - 1], gold["gnn_pred_pos"][0], rtol=1e-5, atol=1e-6)
    np.testing.assert_allclose(mot[:N - 1], gold["gnn_pred_motion"][0], rtol=1e-4, atol=1e-6)


def test_aggregate_f32_stays_inside_the_derived_bound():
    rng = np.random.default_rng(0)
    H, worst = 8, 0.0
    for n in (0, 1, 2, 3, 10, 100, 500, 2000):
        E = n + 5
        rew1 = rng.standard_normal((E, H)).astype(np.float32)
        a23 = rng.standard_normal((4, 2 * H)).astype(np.float32)
        send = rng.integers(0, 4, E)
        row_start = np.array([0, n, n, n + 5, E])                          # rows of n, 0, 5 and 0 entries
        want = gnn_ref.aggregate(rew1, a23, send, row_start, 4)
        got = gnn_ref.aggregate_f32(rew1, a23, send, row_start, 4)
        bound = gnn_ref.aggregate_bound(rew1, a23, send, row_start, 4)
        assert got.dtype == np.float32 and want.dtype == np.float64
        direct = sum(np.maximum(rew1[e].astype(np.float64) + a23[2, :H] + a23[send[e], H:], 0) for e in range(n, n + 5))
        np.testing.assert_allclose(want[2], direct, rtol=1e-14)
        assert not want[1].any() and not want[3].any() and not got[1].any()
        err = np.abs(got - want)
        assert (err <= bound).all(), n
        worst = max(worst, float((err[bound > 0] / bound[bound > 0]).max()))
        assert not gnn_ref.aggregate(rew1, a23, send, row_start, 2)[2:].any()            # rows >= n_sum are zero
    print(f"aggregate_f32 used at most {worst:.2f} of the bound")


def test_aggregate_statement_keeps_a_nan_as_torch_does():
    rew1 = np.array([[1.0, np.nan, -3.0, np.inf]], dtype=np.float32)
    a23 = np.zeros((1, 8), dtype=np.float32)
    got = gnn_ref.aggregate_f32(rew1, a23, np.array([0]), np.array([0, 1]), 1)
    want = torch.relu(torch.tensor(rew1)).numpy()
    assert np.array_equal(got, want, equal_nan=True) and np.isnan(got[0, 1]) and got[0, 2] == 0 and np.isinf(got[0, 3])
