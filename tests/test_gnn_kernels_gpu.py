"""GPU tests of the propagation network's device path (gsdyn.dynamics.DynamicsPredictor._propagate_split and its three callers) against
the fp64 restatement of tests/gnn_ref.py.

Part one: the two kernels of csrc/gsr_gnn.hip alone -- gsr_gnn_rel_inputs and gsr_gnn_aggregate[_res] bit for bit against their fp32
statements and within derived bounds of fp64, at every shape edge, segment layout and non-finite input -- and the wrappers' contract.
Part two: the whole network at every configuration the device path accepts (gnn_ref.CONFIGS), through the eager split path, the graphed
propagation and the planner's batch; the bound is 4 x the HOST fp32 network's own distance from fp64 on the same inputs (gnn_ref.yardstick).
The measured distances are appended to gnn_parity.log next to plan_rollout_parity.log (``GSR_GNN_PARITY_LOG`` names another file);
profiles/gnn_parity.txt is that log of one run, copied by hand under a one-line header."""
import os

import numpy as np
import pytest
import torch

import gnn_ref
from gnn_ref import U24
from hipcheck import _ROW_LOG

pytestmark = pytest.mark.gpu

_LOG = os.environ.get("GSR_GNN_PARITY_LOG", os.path.join(os.path.dirname(_ROW_LOG), "gnn_parity.log"))


def _log(line):
    print(line)
    try:
        os.makedirs(os.path.dirname(_LOG), exist_ok=True)
        with open(_LOG, "a") as f:
            f.write(line + "\n")
    except OSError as e:
        print(f"(gnn_parity.log not written: {e})")


def _bits(x):
    return np.ascontiguousarray(x, dtype=np.float32).view(np.uint32)


def _same_bits(got, want):
    """Bit equality, except that any NaN equals any NaN (the payload is not pinned)."""
    got, want = np.asarray(got, dtype=np.float32), np.asarray(want, dtype=np.float32)
    nan = np.isnan(want)
    return got.shape == want.shape and np.array_equal(np.isnan(got), nan) and np.array_equal(_bits(got)[~nan], _bits(want)[~nan])


# ========================================================================================== part one: gsr_gnn_rel_inputs
@pytest.mark.parametrize("A,G,S", [(2, 1, 9), (0, 1, 3), (3, 2, 9), (2, 4, 3), (2, 1, 0)])
def test_rel_inputs_kernel_bit_for_bit(dev, A, G, S):
    """Bit-equal to the fp32 statement (a gather is exact, a difference column one fp32 subtraction, the group column an ascending-k fp32
    sum of |a - b|), and within 2^-24 relative of fp64 per column: the gathers are exact and a difference of two fp32 numbers is rounded
    once.  The group column of G > 1 columns is a sum of G rounded terms, which no fp32 evaluation holds to ONE rounding for arbitrary
    inputs: the fp64 comparison of that column runs on instance values that are multiples of 2^-10 (every term and the sum exact), the
    bit comparison on full-mantissa values as well (there the order of the sum shows)."""
    from diff_gaussian_rasterization import _hip
    Dr, F, N = 2 * A + 1 + S, A + G + S, 37
    rng = np.random.default_rng(1000 * A + 100 * G + S)
    for E in (1, 256 // Dr, 256 // Dr + 1, 1000):          # around 256 / Dr a row of ``out`` straddles two workgroups
        for dyadic in (False, True):
            nodes = rng.standard_normal((N, F)).astype(np.float32)
            if dyadic:
                nodes[:, A:A + G] = rng.integers(0, 1024, (N, G)).astype(np.float32) / 1024.0
            nodes[N - 1] = 0.0                                 # the padding's dummy row
            recv, send = rng.integers(0, N, E), rng.integers(0, N, E)
            send[1::7] = N - 1                                 # senders at the dummy row
            send[::5] = recv[::5]                              # recv == send: exact zeros
            recv[E - 1], send[E - 1] = N - 1, N - 1            # ... and a padding relation
            got = _hip.gnn_rel_inputs(torch.from_numpy(nodes).to(dev), torch.from_numpy(recv).to(dev), torch.from_numpy(send).to(dev), A, G).cpu().numpy()
            want32 = gnn_ref.rel_inputs(nodes, recv, send, A, G, dtype=np.float32)
            want64 = gnn_ref.rel_inputs(nodes, recv, send, A, G)
            tag = (A, G, S, E, dyadic)
            assert got.shape == (E, Dr) and want32.dtype == np.float32, tag
            assert np.array_equal(_bits(got), _bits(want32)), tag
            assert not got[::5, 2 * A:].any() and np.array_equal(got[::5, :A], got[::5, A:2 * A]), tag
            cols = np.ones(Dr, dtype=bool)
            cols[2 * A] = dyadic or G == 1
            assert (np.abs(got - want64)[:, cols] <= U24 * np.abs(want64)[:, cols]).all(), tag


# ========================================================================================== part one: gsr_gnn_aggregate[_res]
PAD = 5          # the dummy row's own segment: padding relations that connect it to itself


def _segments(layout, N, rng):
    """Degrees of the N - 1 real rows (the last row is the padding's dummy row and owns PAD entries)."""
    n = N - 1
    deg = np.zeros(n, dtype=np.int64)
    if n == 0 or layout == "none":
        return deg
    if layout == "random":
        deg = rng.integers(0, 10, n)
    elif layout == "alternate":
        deg = rng.integers(1, 10, n)
        deg[1::2] = 0
    elif layout == "ends_empty":
        deg = rng.integers(1, 10, n)
        deg[0] = deg[n - 1] = 0
    elif layout == "first":
        deg[0] = 97
    elif layout == "last":
        deg[n - 1] = 97
    return deg


def _aggregate_case(N, H, layout, rng, scale=1.0):
    deg = _segments(layout, N, rng)
    deg = np.concatenate([deg, [0 if layout == "none" else PAD]])
    row_start = np.concatenate([[0], np.cumsum(deg)]).astype(np.int64)
    E = int(row_start[-1])
    send = rng.integers(0, N, E).astype(np.int64)
    if E:
        send[E - int(deg[-1]):] = N - 1
    rew1 = (rng.standard_normal((E, H)) * scale).astype(np.float32)
    a23 = (rng.standard_normal((N, 2 * H)) * scale).astype(np.float32)
    ra, rb = rng.standard_normal((N, H)).astype(np.float32), rng.standard_normal((N, H)).astype(np.float32)
    return rew1, a23, send, row_start, ra, rb


def _run_aggregate(dev, rew1, a23, send, row_start, n_sum, ra, rb):
    from diff_gaussian_rasterization import _hip
    t = lambda x: torch.from_numpy(x).to(dev)  # noqa: E731
    rew1, a23, send, row_start, ra, rb = t(rew1), t(a23), t(send), t(row_start), t(ra), t(rb)
    agg = _hip.gnn_aggregate(rew1, a23, send, row_start, n_sum)
    agg2, base = _hip.gnn_aggregate(rew1, a23, send, row_start, n_sum, res=(ra, rb))
    return agg.cpu().numpy(), agg2.cpu().numpy(), base.cpu().numpy()


def _check_aggregate(dev, case, n_sum, tag):
    rew1, a23, send, row_start, ra, rb = case
    N = a23.shape[0]
    agg, agg2, base = _run_aggregate(dev, rew1, a23, send, row_start, n_sum, ra, rb)
    want32 = gnn_ref.aggregate_f32(rew1, a23, send, row_start, n_sum)
    want64 = gnn_ref.aggregate(rew1, a23, send, row_start, n_sum)
    bound = gnn_ref.aggregate_bound(rew1, a23, send, row_start, n_sum)
    assert agg.shape == want32.shape and np.array_equal(_bits(agg), _bits(want32)), tag
    assert np.array_equal(_bits(agg2), _bits(agg)) and np.array_equal(_bits(base), _bits(ra + rb)), tag
    assert (np.abs(agg - want64) <= bound).all(), tag
    assert not agg[n_sum:].any(), tag                                  # rows >= n_sum: zero (the dummy row's padding included)
    if n_sum == N and row_start[-1]:
        assert agg[N - 1].any(), tag                                   # ... and summed like any other row when it is asked for


@pytest.mark.parametrize("N,H", [(1, 4), (2, 8), (63, 12), (64, 12), (65, 12), (257, 20), (128, 64), (22, 512)])
def test_aggregate_kernel_bit_for_bit(dev, N, H):
    """gsr_gnn_aggregate and _res against ``aggregate_f32`` (bit for bit) and fp64 ``aggregate`` (|err| <= (n_e + 2) 2^-24 sum_e(|r1_e| + |a2|
    + |a3_e|), gnn_ref.aggregate_bound).  With H / 4 = 3 or 5 a row's threads straddle the 256-thread workgroups."""
    rng = np.random.default_rng(N * 1000 + H)
    for layout in ("random", "alternate", "ends_empty", "first", "last", "none"):
        case = _aggregate_case(N, H, layout, rng)
        for n_sum in sorted({N, N - 1, 0}):
            _check_aggregate(dev, case, n_sum, (N, H, layout, n_sum))


def test_aggregate_kernel_long_segment(dev):
    rng = np.random.default_rng(7)
    N, H, n = 4, 4, 2000
    row_start = np.array([0, 3, 3 + n, 3 + n, 3 + n + PAD], dtype=np.int64)          # rows of 3, 2000, 0 entries and the dummy's padding
    E = int(row_start[-1])
    send = rng.integers(0, N, E).astype(np.int64)
    case = ((rng.standard_normal((E, H))).astype(np.float32), rng.standard_normal((N, 2 * H)).astype(np.float32), send, row_start,
            rng.standard_normal((N, H)).astype(np.float32), rng.standard_normal((N, H)).astype(np.float32))
    for n_sum in (N, N - 1, 0):
        _check_aggregate(dev, case, n_sum, ("long", n_sum))


def _torch_statement(rew1, a23, send, row_start, n_sum):
    """torch.relu, then a list-order sum per receiver, on the host."""
    r1, nb = torch.from_numpy(rew1), torch.from_numpy(a23)
    N, H = nb.shape[0], nb.shape[1] // 2
    recv = torch.repeat_interleave(torch.arange(N), torch.from_numpy(np.diff(row_start)))
    terms = torch.relu((r1 + nb[recv, :H]) + nb[torch.from_numpy(send), H:])
    out = torch.zeros((N, H))
    for e in range(int(row_start[n_sum])):
        out[recv[e]] = out[recv[e]] + terms[e]
    return out.numpy()


def test_aggregate_kernel_non_finite_values_as_torch(dev):
    """NaN and inf are ordinary data: the result equals the torch statement (torch.relu keeps a NaN; fmaxf(NaN, 0) would not), the touched
    elements are NaN / inf exactly where the statement's are, and nothing else moves."""
    rng = np.random.default_rng(11)
    N, H = 9, 8
    deg = np.array([3, 0, 4, 2, 5, 1, 3, 2, PAD])
    row_start = np.concatenate([[0], np.cumsum(deg)]).astype(np.int64)
    E = int(row_start[-1])
    send = rng.integers(0, N - 1, E).astype(np.int64)
    send[E - PAD:] = N - 1
    send[int(row_start[4]) + 1] = 6                      # row 4's second relation sends from row 6 ...
    send[int(row_start[0])] = 6                          # ... and so does row 0's first
    clean = (rng.standard_normal((E, H)).astype(np.float32), rng.standard_normal((N, 2 * H)).astype(np.float32), send, row_start,
             rng.standard_normal((N, H)).astype(np.float32), rng.standard_normal((N, H)).astype(np.float32))
    rew1, a23 = clean[0].copy(), clean[1].copy()
    rew1[int(row_start[2]) + 1, 1] = np.nan              # a NaN in rew1: row 2, column 1
    rew1[int(row_start[3]), 2] = np.inf                  # + inf in rew1: row 3, column 2
    a23[6, H + 3] = np.nan                               # a NaN in a sender's a3 half: rows 0 and 4 (and whoever else row 6 sends to), column 3
    a23[7, 0] = np.nan                                   # a NaN in a receiver's a2 half: row 7, column 0
    a23[5, 5] = -np.inf                                  # - inf in a receiver's a2 half: relu gives 0, row 5 column 5 is exactly 0
    for n_sum in (N, N - 1):
        agg_clean = _run_aggregate(dev, *clean[:4], n_sum, *clean[4:])[0]
        agg, agg2, base = _run_aggregate(dev, rew1, a23, send, row_start, n_sum, *clean[4:])
        want = _torch_statement(rew1, a23, send, row_start, n_sum)
        want_clean = _torch_statement(*clean[:4], n_sum)
        assert _same_bits(want, gnn_ref.aggregate_f32(rew1, a23, send, row_start, n_sum))           # the two statements agree
        for r, c in ((2, 1), (0, 3), (4, 3), (7, 0)):
            assert np.isnan(want[r, c]), (r, c)
        assert want[3, 2] == np.inf and want[5, 5] == 0.0
        assert _same_bits(agg, want) and _same_bits(agg2, want), (n_sum, agg, want)
        assert np.array_equal(_bits(base), _bits(clean[4] + clean[5]))
        touched = ~((_bits(want) == _bits(want_clean)) | (np.isnan(want) & np.isnan(want_clean)))
        assert 6 <= int(touched.sum()) <= 16
        assert np.array_equal(_bits(agg)[~touched], _bits(agg_clean)[~touched])
        assert np.isfinite(agg[~touched]).all()


# ========================================================================================== part one: the wrappers' contract
def _wrapper_inputs(dev, N=6, H=8, E=10):
    g = torch.Generator().manual_seed(3)
    rew1, a23 = torch.randn((E, H), generator=g).to(dev), torch.randn((N, 2 * H), generator=g).to(dev)
    send = torch.randint(0, N, (E,), generator=g).to(dev)
    rows = torch.tensor([0, 2, 2, 5, 7, 9, 10][:N + 1], dtype=torch.int64, device=dev)
    return rew1, a23, send, rows


def test_wrappers_without_relations(dev):
    """E = 0: zeros [N, H] (and a + b), an empty [0, Dr] -- no library call (an empty tensor has no address to hand over)."""
    from diff_gaussian_rasterization import _hip
    N, H = 6, 8
    g = torch.Generator().manual_seed(4)
    a23 = torch.randn((N, 2 * H), generator=g).to(dev)
    ra, rb = torch.randn((N, H), generator=g).to(dev), torch.randn((N, H), generator=g).to(dev)
    rew1 = torch.zeros((0, H), device=dev)
    send = torch.zeros((0,), dtype=torch.int64, device=dev)
    rows = torch.zeros((N + 1,), dtype=torch.int64, device=dev)
    for n_sum in (None, N - 1, 0):
        agg = _hip.gnn_aggregate(rew1, a23, send, rows, n_sum)
        agg2, base = _hip.gnn_aggregate(rew1, a23, send, rows, n_sum, res=(ra, rb))
        for x in (agg, agg2):
            assert x.shape == (N, H) and x.dtype == torch.float32 and x.device == a23.device and not bool(x.any())
        assert torch.equal(base, ra + rb)
    nodes = torch.randn((N, 2 + 1 + 9), generator=g).to(dev)
    out = _hip.gnn_rel_inputs(nodes, send, send, 2, 1)
    assert out.shape == (0, 14) and out.dtype == torch.float32 and out.device == nodes.device


def test_aggregate_wrapper_rejects_what_the_kernel_would_misread(dev):
    from diff_gaussian_rasterization import _hip
    rew1, a23, send, rows = _wrapper_inputs(dev)
    N, H, E = 6, 8, 10
    ra, rb = torch.zeros((N, H), device=dev), torch.zeros((N, H), device=dev)
    assert _hip.gnn_aggregate(rew1, a23, send, rows).shape == (N, H)                    # the inputs as they should be
    wide = torch.zeros((E, 2 * H), device=dev)
    bad = {
        "rel_part not contiguous": (wide[:, :H], a23, send, rows),
        "rel_part not float32": (rew1.double(), a23, send, rows),
        "node_parts not contiguous": (rew1, torch.zeros((N, 4 * H), device=dev)[:, :2 * H], send, rows),
        "node_parts not float32": (rew1, a23.half(), send, rows),
        "node_parts width != 2 H": (rew1, a23[:, :H].contiguous(), send, rows),
        "H % 4 != 0": (rew1[:, :6].contiguous(), a23[:, :12].contiguous(), send, rows),
        "senders int32": (rew1, a23, send.int(), rows),
        "senders not contiguous": (rew1, a23, torch.stack([send, send], 1)[:, 0], rows),
        "senders on the host": (rew1, a23, send.cpu(), rows),
        "senders length != E": (rew1, a23, send[:E - 1], rows),
        "row_start int32": (rew1, a23, send, rows.int()),
        "row_start not contiguous": (rew1, a23, send, torch.stack([rows, rows], 1)[:, 0]),
        "row_start on the host": (rew1, a23, send, rows.cpu()),
        "row_start length != N + 1": (rew1, a23, send, rows[:N]),
    }
    for why, args in bad.items():
        with pytest.raises(ValueError):
            _hip.gnn_aggregate(*args)
            pytest.fail(f"accepted: {why}")
        with pytest.raises(ValueError):
            _hip.gnn_aggregate(*args, res=(ra, rb))
            pytest.fail(f"accepted with res: {why}")
    for res in ((ra[:, :4], rb), (ra.double(), rb.double()), (ra, torch.zeros((N, 2 * H), device=dev)[:, :H])):
        with pytest.raises(ValueError):
            _hip.gnn_aggregate(rew1, a23, send, rows, res=res)


def test_rel_inputs_wrapper_rejects_what_the_kernel_would_misread(dev):
    from diff_gaussian_rasterization import _hip
    g = torch.Generator().manual_seed(5)
    N, E, A, G, S = 6, 10, 2, 1, 9
    nodes = torch.randn((N, A + G + S), generator=g).to(dev)
    recv, send = torch.randint(0, N, (E,), generator=g).to(dev), torch.randint(0, N, (E,), generator=g).to(dev)
    assert _hip.gnn_rel_inputs(nodes, recv, send, A, G).shape == (E, 2 * A + 1 + S)
    bad = {
        "rel_nodes not contiguous": (torch.zeros((N, 2 * (A + G + S)), device=dev)[:, :A + G + S], recv, send),
        "rel_nodes not float32": (nodes.double(), recv, send),
        "rel_nodes narrower than attr + group": (nodes[:, :2].contiguous(), recv, send),
        "receivers int32": (nodes, recv.int(), send),
        "senders int32": (nodes, recv, send.int()),
        "receivers not contiguous": (nodes, torch.stack([recv, recv], 1)[:, 0], send),
        "senders not contiguous": (nodes, recv, torch.stack([send, send], 1)[:, 0]),
        "receivers on the host": (nodes, recv.cpu(), send),
        "senders on the host": (nodes, recv, send.cpu()),
        "senders length != E": (nodes, recv, send[:E - 1]),
    }
    for why, args in bad.items():
        with pytest.raises(ValueError):
            _hip.gnn_rel_inputs(*args, A, G)
            pytest.fail(f"accepted: {why}")


# ========================================================================================== part two: the whole network
FACTOR = 4.0
"""A device path may be 4 y_c from fp64, y_c = the host fp32 ``_propagate``'s distance on the same 8 input sets: both are fp32 evaluations of
one network; the device side sums the products in another order and forms each relation effect from three separately rounded partial
products, (r1 + a2) + a3, instead of one -- two more roundings at the partials' magnitude.  (The planner path recorded ratios up to 1.6
against its own yardstick: profiles/plan_rollout_parity.txt.)"""


def _dev_set(s, dev):
    return {k: v.to(dev) for k, v in s.items()}


def _assert_within(tag, c, e_m, e_p):
    _log(f"{tag}: motions {e_m:.3e} of the largest motion = {e_m / c['y']:.2f} y_c ({c['y']:.3e}); positions {e_p:.3e} absolute = "
         f"{e_p / c['p_y']:.2f} p_y ({c['p_y']:.3e})")
    assert e_m <= FACTOR * c["y"] and e_p <= FACTOR * c["p_y"], (tag, e_m, c["y"], e_p, c["p_y"])


def _fresh_model(c, dev):
    from gsdyn.dynamics import DynamicsPredictor
    m = DynamicsPredictor(c["cfg"]).eval()
    m.load_state_dict(c["model"].state_dict())
    return m.to(dev)


@pytest.mark.parametrize("name", list(gnn_ref.CONFIGS))
def test_split_propagation_against_fp64(dev, name):
    """P1: ``_propagate_split``, eager, on the host-built ascending list."""
    c = gnn_ref.case(name)
    model = _fresh_model(c, dev)
    e_m = e_p = 0.0
    with torch.no_grad():
        for s, ref in zip(c["sets"], c["refs"]):
            d = _dev_set(s, dev)
            assert model._split_ok(d["a"])
            pos, mot = model._propagate_split(d["state_t"], d["a"], d["g"], d["act"], d["recv"], d["send"])
            assert pos.shape == (gnn_ref.N_OBJ + 1, 3)
            m, p = gnn_ref.errors(pos.cpu().numpy(), mot.cpu().numpy(), *ref)
            e_m, e_p = max(e_m, m), max(e_p, p)
    _assert_within(f"P1 split      {name:>3}", c, e_m, e_p)


def _call_model(model, c, d, recv, send):
    n_obj = gnn_ref.N_OBJ
    action = d["act"][None] if c["cfg"]["action_dim"] > 0 else None
    pos, mot = model(state=d["state"][None], attrs=d["a"][None], p_instance=d["g"][None, :n_obj], action=action, receivers=recv, senders=send)
    assert pos.shape == (1, n_obj, 3) and mot.shape == (1, n_obj, 3)
    return pos[0], mot[0]


@pytest.mark.parametrize("name", list(gnn_ref.CONFIGS))
def test_graphed_propagation_against_fp64(dev, name):
    """P2: ``model(...)`` with one graph under no_grad = ``_forward_index`` -> ``_propagate_graphed`` (padding, capture, replay), the list
    handed over SHUFFLED: the stable sort inside restores the receiver order (a receiver's relations stay in the order given, which moves
    the fp64 reference by 1e-16 only: it is the one of the ascending list)."""
    c = gnn_ref.case(name)
    model = _fresh_model(c, dev)
    gen = torch.Generator().manual_seed(17)
    e_m = e_p = 0.0
    with torch.no_grad():
        for s, ref in zip(c["sets"], c["refs"]):
            d = _dev_set(s, dev)
            perm = torch.randperm(s["recv"].shape[0], generator=gen)
            assert not torch.equal(s["recv"][perm], s["recv"])
            pos, mot = _call_model(model, c, d, s["recv"][perm].to(dev), s["send"][perm].to(dev))
            m, p = gnn_ref.errors(pos.cpu().numpy(), mot.cpu().numpy(), *ref)
            e_m, e_p = max(e_m, m), max(e_p, p)
    assert len(model._graphs) == 1                       # one padded shape: the sets were replays of one captured graph
    _assert_within(f"P2 graphed    {name:>3}", c, e_m, e_p)


@pytest.mark.parametrize("name", ["C0", "C1"])
def test_graphed_propagation_replay_carries_nothing_over(dev, name):
    """A second call of the same padded shape with FEWER relations and other positions gives, bit for bit, what a model with the same
    weights and an empty graph cache gives on its first call: stale buffer contents reach no result."""
    c = gnn_ref.case(name)
    s0, s1 = c["sets"][0], c["sets"][1]
    gen = torch.Generator().manual_seed(23)
    keep = torch.randperm(s1["recv"].shape[0], generator=gen)[:60]          # a shuffled subset: 60 of ~100 relations, the same 128-entry list
    recv1, send1 = s1["recv"][keep].to(dev), s1["send"][keep].to(dev)
    with torch.no_grad():
        used, fresh = _fresh_model(c, dev), _fresh_model(c, dev)
        _call_model(used, c, _dev_set(s0, dev), s0["recv"].to(dev), s0["send"].to(dev))
        got = _call_model(used, c, _dev_set(s1, dev), recv1, send1)
        want = _call_model(fresh, c, _dev_set(s1, dev), recv1, send1)
    assert len(used._graphs) == 1 and len(fresh._graphs) == 1
    assert torch.equal(got[0], want[0]) and torch.equal(got[1], want[1])
    order = torch.sort(s1["recv"][keep], stable=True)[1]                     # and the result is the subset's: against fp64 on the sorted subset
    r, sd = s1["recv"][keep][order].numpy(), s1["send"][keep][order].numpy()
    ref = gnn_ref.propagate(c["weights"], c["cfg"], s1["state_t"].numpy(), s1["a"].numpy(), s1["g"].numpy(), s1["act"].numpy(), r, sd)
    e_m, e_p = gnn_ref.errors(got[0].cpu().numpy(), got[1].cpu().numpy(), *ref)
    assert e_m <= FACTOR * c["y"] and e_p <= FACTOR * c["p_y"], (e_m, e_p)


@pytest.mark.parametrize("B", [1, 2, 65])
@pytest.mark.parametrize("name", ["C0", "C1", "C6"])
def test_planner_batch_against_fp64(dev, name, B):
    """P3: the planner's batch (gsr_plan_step_head + gsr_construct_edges_batch + ``_propagate_split`` on B R + 1 rows); sample b carries
    input set b mod 8, and is compared with the reference on ITS OWN relation segment of the device's list."""
    from diff_gaussian_rasterization import _hip
    c = gnn_ref.case(name)
    cfg, n_obj, sets = c["cfg"], gnn_ref.N_OBJ, c["sets"]
    model = _fresh_model(c, dev)
    R, n_his = n_obj + 1, cfg["n_his"]
    pick = [b % len(sets) for b in range(B)]
    hist = torch.stack([sets[k]["state"][:, :n_obj] for k in pick]).contiguous().to(dev)            # [B, n_his, n_obj, 3]
    eef_hist = torch.stack([sets[k]["state"][:, n_obj] for k in pick]).contiguous().to(dev)         # [B, n_his, 3]
    delta = torch.stack([sets[k]["act"][n_obj] for k in pick]).contiguous().to(dev)                 # [B, 3]
    a1, g1 = sets[0]["a"], sets[0]["g"]
    a = torch.cat([a1.repeat(B, 1), torch.zeros((1, a1.shape[1]))], 0).contiguous().to(dev)
    g = torch.cat([g1.repeat(B, 1), torch.zeros((1, 1))], 0).contiguous().to(dev)
    with torch.no_grad():
        st, p_in, nodes, last = _hip.plan_step_head(hist, eef_hist, delta, a, g.view(-1), cfg["state_dim"] == 3)
        recv, send, cnt, rows = _hip.construct_edges_batch(last, torch.tensor([n_obj], dtype=torch.int32, device=dev), gnn_ref.THR, gnn_ref.TOPK)
        _, mot = model._propagate_split(None, a, g, None, recv, send, dummy_last_row=True, p_in=p_in, nodes=nodes, row_start=rows, motion_only=True)
        pos = st[:, -3:] + torch.clamp(mot, -model.motion_clamp, model.motion_clamp)                 # gsr_plan_step_tail's arithmetic
    rows_h, recv_h, send_h, mot_h, pos_h = rows.cpu(), recv.cpu(), send.cpu(), mot.cpu().numpy(), pos.cpu().numpy()
    assert int(cnt.item()) > B * R
    e_m = e_p = 0.0
    refs = {}
    for b, k in enumerate(pick):
        lo, hi = int(rows_h[b * R]), int(rows_h[(b + 1) * R])
        r_b, s_b = (recv_h[lo:hi] - b * R).numpy(), (send_h[lo:hi] - b * R).numpy()
        assert hi - lo > R and r_b.min() >= 0 and max(r_b.max(), s_b.max()) < R
        key = (k, r_b.tobytes(), s_b.tobytes())
        if key not in refs:
            s = sets[k]
            refs[key] = gnn_ref.propagate(c["weights"], cfg, s["state_t"].numpy(), s["a"].numpy(), s["g"].numpy(), s["act"].numpy(), r_b, s_b)
        m, p = gnn_ref.errors(pos_h[b * R:(b + 1) * R], mot_h[b * R:(b + 1) * R], *refs[key])
        e_m, e_p = max(e_m, m), max(e_p, p)
    _assert_within(f"P3 planner    {name:>3} B={B:2d}", c, e_m, e_p)


# ------------------------------------------------------------------------------------------ the fused rollout step with the state columns
@pytest.mark.parametrize("name", ["C1", "C6"])
def test_graphed_step_with_fused_glue_equals_the_torch_glue_at(dev, name):
    """test_graphed_step_with_fused_glue_equals_the_torch_glue (tests/test_dynamics_gpu.py, C0) at state_dim = 3 and at attr_dim = 3: four
    steps with the glue as kernels and as torch ops, the same packets, positions, rotations, histories, predicted bones and bone count."""
    import gsdyn.dynamics as D
    from gsdyn import synth_scene_params
    c = gnn_ref.case(name)
    model = _fresh_model(c, dev)
    P, n_track = 3000, 200
    params = {k: v.detach() for k, v in synth_scene_params(P, device=dev).items()}
    xyz, quat = params["means3D"], torch.nn.functional.normalize(params["unnorm_rotations"])
    with torch.no_grad():
        track = D.farthest_point_sampler(xyz[None], n_track)[0]
        runs, bodies = {}, {}
        for fused in (True, False):
            D._STEP_FUSED_GLUE = fused
            model.__dict__.pop("_step_graphs", None)
            try:
                gs = D._graphed_step_for(model, P, n_track, 3, 40, 0.3, 0, 0.6, 5, dev)
                bodies[fused] = gs._body.__name__
                gs.load(track, xyz[track], xyz[track][None].repeat(3, 1, 1), torch.zeros((3, 1, 3), device=dev), xyz, quat)
                out = []
                for i in range(4):
                    gs.step(torch.tensor([[0.03 * (i + 1), 0.0, 0.01 * (i + 1)]], device=dev))
                    out.append([t.clone() for t in (gs.skin, gs.all_pos, gs.all_rot, gs.hist, gs.eef_hist, gs.pred, gs.n_valid)])
                torch.cuda.synchronize()
                runs[fused] = out
            finally:
                D._STEP_FUSED_GLUE = True
                model.__dict__.pop("_step_graphs", None)
    assert bodies == {True: "body_fused", False: "body"}
    assert 2 <= int(runs[True][0][6]) <= 40 and not torch.equal(runs[True][-1][1], xyz) and torch.isfinite(runs[True][-1][1]).all()
    for i, (a, b) in enumerate(zip(runs[True], runs[False])):
        for j, (x, y) in enumerate(zip(a, b)):
            assert torch.equal(x, y), (name, i, j, float((x.float() - y.float()).abs().max()))


# ------------------------------------------------------------------------------------------ a whole planner rollout with the state columns
ROLL_SEED_C1 = 20          # found on the host: with this seed the fp64 reference keeps both relation margins >= 1e-3 (asserted below)


def test_whole_rollout_with_state_columns_against_the_fp64_fallback(dev):
    """tests/test_plan_gpu.py's whole rollout at state_dim = 3 (C1): the relation lists of every call equal the fp64 fallback's, the
    positions lie within 2 p_y per model call behind a state, p_y = the host fp32 network's position distance from fp64 for THIS model
    on the case shape of this file."""
    from gsdyn.plan import rollout_actions
    from test_plan_gpu import ROLL, ROLL_REPEATS, _model, _relation_margins, _roll_case
    _, state, actions = _roll_case(ROLL_SEED_C1)
    make = lambda: _model(ROLL["width"], seed=ROLL_SEED_C1, motion_scale=ROLL["motion_scale"], state_dim=3)  # noqa: E731
    kw = dict(push_length=ROLL["push"], adj_thresh=ROLL["thr"], topk=ROLL["topk"], n_his=3)
    host = make()
    _, p_y, _ = gnn_ref.yardstick(host, gnn_ref.input_sets(host.model_config, 1, 300))
    trace = []
    ref = rollout_actions(make().double(), state.double(), actions.double(), _trace=trace, **kw)["state_seqs"]
    calls = {(s + b, li, ai): (pts, recv, send) for s, e, tr in trace for b, li, ai, pts, recv, send in tr}
    n_calls = sum(sum(r) for r in ROLL_REPEATS)
    assert len(calls) == n_calls
    margins = [_relation_margins(p, ROLL["thr"], ROLL["topk"]) for p, _, _ in calls.values()]
    m_thr, m_k = min(m[0] for m in margins), min(m[1] for m in margins)
    assert m_thr >= 1e-3 and m_k >= 1e-3, (m_thr, m_k)
    trace = []
    got = rollout_actions(make().to(dev), state.to(dev), actions.to(dev), _trace=trace, **kw)["state_seqs"]
    (s, e, tr), = trace
    R, seen = ROLL["n_obj"] + 1, 0
    for li, ai, last, recv, send, cnt in tr:
        m = int(cnt.item())
        recv, send = recv[:m].cpu(), send[:m].cpu()
        for b in range(ROLL["B"]):
            if (b, li, ai) not in calls:
                continue
            sel = (recv >= b * R) & (recv < (b + 1) * R)
            _, w_recv, w_send = calls[(b, li, ai)]
            assert torch.equal(recv[sel] - b * R, w_recv) and torch.equal(send[sel] - b * R, w_send), (b, li, ai)
            seen += 1
    assert seen == n_calls
    disp = float((ref - state.double()[None, None]).abs().max())
    err = float((got.double().cpu() - ref).abs().max())
    depth = max(sum(r) for r in ROLL_REPEATS)
    bound = 2.0 * p_y * depth
    _log(f"whole rollout C1 B={ROLL['B']} T={ROLL['T']} n_obj={ROLL['n_obj']}: margins thr {m_thr:.2e} k {m_k:.2e}; largest displacement {disp:.3e}, "
         f"max abs error {err:.3e}, bound {bound:.3e} (= 2 x {p_y:.3e} x {depth} calls)")
    assert disp > 1e-3 and err <= bound, (err, bound)
