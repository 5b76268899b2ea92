"""The device tree search (acme_mcts_search_run) at its edges, on the cases of
tests/mcts_search_cases.py: fewer simulations than the handle holds and a reused handle, ties
among all 64 lanes, a tree that is one chain, terminals everywhere and nowhere, the widths and
depths create() accepts, the LDS residency boundary, non-finite scores, and the call surface.

Counts (root visits, every node's edge visits, nodes, deepest) equal those of the float64
search of tests/mcts_search_oracle.py; prior, root value and child values meet
tests/test_az_gpu.py::_close; runs that must agree (a repeated call, a fresh handle, resident
and streamed weights) agree bit for bit.  tests/test_mcts_search_cases_cpu.py proves on the
reference alone that every case keeps clear of ties and has the property it is here for."""

import numpy as np
import pytest
import torch

from acme_amd import _lib
from tests import mcts_search_cases as C
from tests.mcts_search_oracle import _setup
from tests.test_az_gpu import _close

pytestmark = pytest.mark.gpu


def _networks(c):
    from acme_amd.native import NativeAZ, NativeMLPModel
    _, _, mp, zp, root = _setup(c.D, c.mh, c.zh, c.A, c.seed, c.zero, c.override)
    az = NativeAZ(obs_dim=c.D, hidden=c.zh, num_actions=c.A, max_batch=4)
    model = NativeMLPModel(obs_dim=c.D, hidden=c.mh, num_actions=c.A, max_batch=4)
    az.set_params(zp)
    model.set_params(mp)
    return az, model, torch.from_numpy(root).cuda()


def _search(c, nets, stream=None):
    from acme_amd.native import NativeMCTSSearch
    return NativeMCTSSearch(nets[0], nets[1], c.cap,
                            stream_weights=c.stream if stream is None else stream)


def _run(n, root, c, **kw):
    """(packed row, visits table [S + 1, A]) of one run of the case, on the host."""
    row = n.run(root, c.S, c.discount, sigmoid=c.activation == "sigmoid", terminal_tol=c.tol,
                seed=c.philox_seed, call_counter=c.call_counter, **kw)
    if kw.get("stream") is not None:
        kw["stream"].synchronize()
    return row.cpu().numpy(), n.debug_buffer("visits").reshape(c.S + 1, -1).copy()


def _same_bits(x, y):
    return all(np.array_equal(a.view(np.uint32), b.view(np.uint32)) for a, b in zip(x, y))


def _check(n, c, run, floats=True):
    """One run against the case's float64 reference."""
    ref, (row, table) = C.reference(c), run
    got = n.unpack(row)
    print(c, {k: got[k] for k in ("nodes", "deepest", "status")})
    assert got["status"] == 0 and got["visits"].sum() == c.S
    np.testing.assert_array_equal(got["visits"], ref["visits"])
    assert (got["nodes"], got["deepest"]) == (ref["nodes"], ref["deepest"])
    np.testing.assert_array_equal(table[:got["nodes"]], ref["tree"])
    assert not table[got["nodes"]:].any()
    if floats:
        _close(got["prior"], ref["prior"], name="root prior")
        _close([got["root_value"]], [ref["root_value"]], name="root value")
        _close(got["values"], ref["values"], name="root child values")
    return got


def _both_sources(c):
    """The case with its weights where create() puts them and streamed: the same bits."""
    nets = _networks(c)
    handles = [_search(c, nets, stream) for stream in (False, True)]
    runs = [_run(n, nets[2], c) for n in handles]
    assert _same_bits(*runs)
    return nets, handles[0], runs[0]


# a. -------------------------------------------------------------------------------------------
def test_fewer_simulations_than_the_handle_holds_and_reuse():
    nets = _networks(C.SMALL)
    n, runs = _search(C.SMALL, nets), []
    for c in C.REUSE:
        runs.append(_run(n, nets[2], c))
        _check(n, c, runs[-1])
    assert _same_bits(runs[0], runs[3])
    seven = C.REUSE[2].but(max_sim=0)
    assert (seven.S, seven.cap) == (7, 7)
    assert _same_bits(runs[2], _run(_search(seven, nets), nets[2], seven))  # cap does not enter
    # With terminals the table has rows past `nodes`, over what the 24-simulation runs left.
    for c in C.REUSE_SIGMOID:
        got = _check(n, c, _run(n, nets[2], c))
        assert got["nodes"] < c.S + 1
    assert _same_bits(runs[0], _run(n, nets[2], C.REUSE[0]))


# b. -------------------------------------------------------------------------------------------
def test_ties_among_all_lanes():
    nets = _networks(C.TIES[0])
    n = _search(C.TIES[0], nets)
    for c in C.TIES:
        got = _check(n, c, _run(n, nets[2], c), floats=False)
        assert (got["prior"] == np.float32(1 / 64)).all() and not got["values"].any()


# c. -------------------------------------------------------------------------------------------
def test_chain_as_deep_as_the_simulations():
    nets = _networks(C.CHAIN)
    n = _search(C.CHAIN, nets)
    run = _run(n, nets[2], C.CHAIN)
    got = _check(n, C.CHAIN, run)
    assert (got["deepest"], got["nodes"]) == (128, 129)
    np.testing.assert_array_equal(run[1][:, 0], np.arange(128, -1, -1))


# d. -------------------------------------------------------------------------------------------
def test_every_edge_terminal():
    c = C.ALL_TERMINAL
    nets = _networks(c)
    n = _search(c, nets)
    got = _check(n, c, _run(n, nets[2], c))
    assert (got["nodes"], got["deepest"]) == (1, 1)
    _close(got["values"], C.reference(c)["root_rewards"], name="cached rewards")


def test_no_edge_terminal_is_the_softmax_search():
    c = C.NONE_TERMINAL
    nets = _networks(c)
    n = _search(c, nets)
    sig, soft = _run(n, nets[2], c), _run(n, nets[2], c.but(activation="softmax"))
    _check(n, c, sig)
    assert _same_bits(sig, soft)


@pytest.mark.parametrize("name", ["mixed", "discount0", "deep"])
def test_case_matches_f64(name):
    c = C.COMPARED[name]
    assert C.resident(c)
    nets = _networks(c)
    n = _search(c, nets)
    got = _check(n, c, _run(n, nets[2], c))
    if name == "discount0":
        _close(got["values"], C.reference(c)["root_rewards"], name="the edges' rewards")


# e. -------------------------------------------------------------------------------------------
def test_widths_at_the_limits():
    c = C.WIDE
    nets = _networks(c)
    assert not C.resident(c, nets[1].flat_size, nets[0].flat_size)
    n = _search(c, nets)
    _check(n, c, _run(n, nets[2], c))


# f. -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["fits", "spills"])
def test_residency_boundary(name):
    c = C.COMPARED[name]
    nets, n, run = _both_sources(c)
    total = C.lds_bytes(c, nets[1].flat_size, nets[0].flat_size)
    assert total == C.lds_bytes(c)
    if name == "fits":
        assert total == _lib.MCTS_SEARCH_LDS_BYTES and C.resident(c)
    else:
        assert total == _lib.MCTS_SEARCH_LDS_BYTES + 256 and not C.resident(c)
    _check(n, c, run)


def test_resident_and_streamed_sigmoid_search_agree():
    c = C.SIGMOID
    nets, n, run = _both_sources(c)
    assert C.resident(c, nets[1].flat_size, nets[0].flat_size)
    _check(n, c, run, floats=False)  # floats: test_search_matches_f64


# g. -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(C.BAD))
def test_bad_score_sets_the_status_and_leaves_the_handle_usable(name):
    c = C.BAD[name]
    ref = C.reference(c)
    assert ref["bad_at"] == ref["simulations"] == ref["nodes"] - 1
    nets = _networks(c)
    n = _search(c, nets)
    row, table = _run(n, nets[2], c)
    got = n.unpack(row)
    print(got)
    assert got["status"] == 1 and got["nodes"] == ref["nodes"]
    assert got["visits"].sum() == ref["simulations"] == table.sum()
    # The same handle on clean networks is a fresh handle's search.
    _, _, mp, zp, root = _setup(c.D, c.mh, c.zh, c.A, c.seed)
    nets[0].set_params(zp)
    nets[1].set_params(mp)
    root = torch.from_numpy(root).cuda()
    clean = c.but(override=())
    again = _run(n, root, clean)
    _check(n, clean, again)
    assert _same_bits(again, _run(_search(clean, nets), root, clean))


def test_actor_raises_check_numerics_and_acts_again():
    from acme_amd import networks, optimizers, specs
    from acme_amd.agents.mcts import MCTS
    from acme_amd.agents.mcts.models import MLPModel
    from acme_amd.environments.catch import Catch
    env = Catch(rows=4, columns=3, seed=0)
    spec = specs.make_environment_spec(env)
    model = MLPModel(spec, replay_capacity=16, batch_size=4, hidden_sizes=(9,))
    agent = MCTS(networks.PolicyValueMLP(12, (9,), 3), model, optimizer=optimizers.Adam(1e-3),
                 n_step=1, discount=0.99, replay_capacity=16, num_simulations=8,
                 environment_spec=spec, batch_size=4, search="native")
    observation = env.reset().observation
    np.random.seed(0)
    assert 0 <= agent.select_action(observation) < 3
    az = agent._learner.native  # noqa: SLF001
    w = az.views(az.params)["mlp/linear_0/w"]
    kept = w[1, 2].item()
    w[1, 2] = float("nan")
    with pytest.raises(ValueError, match="check_numerics failed"):
        agent.select_action(observation)
    w[1, 2] = kept
    assert 0 <= agent.select_action(observation) < 3


# h. -------------------------------------------------------------------------------------------
def test_out_slice_unaligned_root_and_side_stream():
    c = C.SMALL
    nets = _networks(c)
    az, model, root = nets
    n = _search(c, nets)
    plain = _run(n, root, c)
    _check(n, c, plain)
    width = 3 * c.A + 4
    # out= inside a larger buffer: the guards keep their bits.
    big = torch.full((width + 10,), float("nan"), device="cuda")
    nan_bits = big.cpu().numpy().view(np.uint32).copy()
    row, table = _run(n, root, c, out=big[3:3 + width])
    host = big.cpu().numpy()
    assert _same_bits(plain, (host[3:3 + width], table)) and _same_bits((row,), (plain[0],))
    for guard in (slice(0, 3), slice(3 + width, None)):
        np.testing.assert_array_equal(host.view(np.uint32)[guard], nan_bits[guard])
    # A root one float into an allocation: 4-byte aligned, not 16.
    shifted = torch.zeros(c.D + 1, device="cuda")
    shifted[1:] = root
    assert shifted[1:].data_ptr() % 16 == 4 and shifted[1:].is_contiguous()
    assert _same_bits(plain, _run(n, shifted[1:], c))
    # A side stream ordered by an event behind a model step on the default stream.
    rng = np.random.default_rng(0)
    ring = torch.as_tensor(rng.standard_normal((8, 2 * c.D + 3)).astype(np.float32)).cuda()
    ring[:, c.D] = 1.0
    side, event = torch.cuda.Stream(), torch.cuda.Event()
    model.step(ring, torch.arange(4, dtype=torch.int32, device="cuda"))
    event.record()
    side.wait_event(event)
    on_side = _run(n, root, c, stream=side)
    torch.cuda.synchronize()
    assert _same_bits(on_side, _run(n, root, c)) and not _same_bits(on_side, plain)


def test_run_refusals():
    c = C.SMALL
    nets = _networks(c)
    n, root, width = _search(c, nets), nets[2], 3 * c.A + 4
    for S in (0, c.cap + 1):
        with pytest.raises(ValueError, match="num_simulations must be in"):
            n.run(root, S)
    for discount in (float("nan"), float("inf")):
        with pytest.raises(ValueError, match="discount must be finite"):
            n.run(root, c.S, discount)
    wide = torch.zeros(2 * (c.D + 1), device="cuda")
    for bad in (wide[:c.D + 1], wide[:c.D - 1], wide[::2][:c.D], root.double(), root.cpu()):
        with pytest.raises(ValueError, match="root_state must be contiguous float32"):
            n.run(bad, c.S)
    out = torch.zeros(2 * (width + 1), device="cuda")
    for bad in (out[:width + 1], out[:width - 1], out[::2][:width]):
        with pytest.raises(ValueError, match="out must be contiguous float32"):
            n.run(root, c.S, out=bad)
    _check(n, c, _run(n, root, c))  # and the handle still serves
