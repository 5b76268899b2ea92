"""The float64 reference of the device tree search (acme_mcts_search_*): search.mcts itself on
the float64 forwards of tests/mlp_model_oracle.py and tests/az_oracle.py, with a search policy
that computes search.puct's scores and an `rng` stand-in that breaks ties by the device's Philox
rule (include/acme_hip.h).  Shared by tests/test_mcts_native_search_gpu.py,
tests/test_mcts_native_search_edges_gpu.py and tests/test_mcts_search_cases_cpu.py; needs no
GPU.  Test infrastructure only.

Besides the tree, the reference logs what makes a float32 comparison meaningful: `gap`, the
smallest distance between the best and the best non-tied PUCT score, with `scale`, the largest
|score|; and `tol_gap`, the smallest |sigmoid(logit) - terminal_tol| over every model step."""

import functools

import numpy as np

from acme_amd import dm_env
from acme_amd.agents.mcts import search
from tests import _oracle, az_oracle as AO, mlp_model_oracle as MO
from tests.test_az_gpu import _params as _az_params
from tests.test_mlp_model_gpu import _params as _model_params

TAG, M32 = 0x4D435453, 0xFFFFFFFF  # "MCTS"


class _Rng:
    """search.argmax's rng: selection k of the call picks the ((r.x n) >> 32)-th maximum.
    widest: the most candidates of one selection; high_pick: a selection among more than 32
    candidates chose an action at or above 32 (both halves of the device's 64-bit tie mask)."""

    def __init__(self, seed, call_counter):
        self.k, self.seed, self.cc = 0, seed, call_counter
        self.widest, self.high_pick = 0, False

    dirichlet = staticmethod(lambda alpha: np.zeros(len(alpha)))  # drawn, then multiplied by 0

    def choice(self, best):
        r = _oracle.philox([self.k, self.cc & M32, self.cc >> 32, TAG],
                           [self.seed & M32, self.seed >> 32])
        self.k += 1
        pick = best[(int(r[0]) * len(best)) >> 32]
        self.widest = max(self.widest, len(best))
        self.high_pick |= len(best) > 32 and pick >= 32
        return pick


class _Model:
    """step / checkpoint / reload on the float64 model forward; counts what the tests assert."""
    def __init__(self, cfg, params, state, sigmoid, terminal_tol=0.5):
        self.cfg, self.params, self.sigmoid, self.tol = cfg, params, sigmoid, terminal_tol
        self.state, self.actions = np.asarray(state, np.float64), []
        self.deepest, self.terminal_edges, self.revisits = 0, set(), 0
        self.tol_gap, self.simulations = np.inf, 0

    def save_checkpoint(self):
        self.ckpt = self.state.copy()

    def load_checkpoint(self):
        self.deepest = max(self.deepest, len(self.actions))
        self.state, self.actions = self.ckpt.copy(), []
        self.simulations += 1

    def step(self, action):
        s, r, x, _ = MO.forward(self.cfg, self.params, self.state[None], [action])
        self.state = s[0]
        self.actions.append(int(action))
        if self.sigmoid:
            p = 1 / (1 + np.exp(-x[0]))
            self.tol_gap = min(self.tol_gap, abs(p - self.tol))
            if p < self.tol:
                self.revisits += tuple(self.actions) in self.terminal_edges
                self.terminal_edges.add(tuple(self.actions))
                return dm_env.termination(reward=r[0], observation=s[0])
        return dm_env.transition(reward=r[0], observation=s[0])


def _setup(D, mh, zh, A, seed, zero=False, override=()):
    """The two networks' float32 parameters and the root state of a case.  zero: True zeroes
    every tensor, a tuple zeroes the tensors it names; override: (where, index, value) triples
    written last, where = "root", "model:<tensor>" or "az:<tensor>" and index is flat."""
    mcfg, zcfg = MO.Config(D, tuple(mh), A), AO.AZConfig(D, tuple(zh), A)
    nets = {"model": _model_params(mcfg, seed + 1), "az": _az_params(zcfg, seed + 2)}
    root = np.random.default_rng(seed + 3).standard_normal(D).astype(np.float32)
    for net, p in nets.items():
        for k in p:
            if zero is True or (zero and f"{net}:{k}" in zero):
                p[k] = np.zeros_like(p[k])
    for where, index, value in override:
        net, _, k = where.partition(":")
        (root if where == "root" else nets[net][k]).reshape(-1)[index] = value
    return mcfg, zcfg, nets["model"], nets["az"], root


@functools.lru_cache(maxsize=None)
def _reference(D, mh, zh, A, S, activation, discount, seed, call_counter=0, zero=False,
               terminal_tol=0.5, tie_seed=None, override=()):
    """The search of S simulations (the handle's max_simulations does not enter).  tie_seed:
    the Philox seed where it is not the parameters' seed.  A search that search.check_numerics
    stops returns what it had reached: `bad_at`, the index of the selection that raised,
    `nodes` and `simulations` (the completed ones); otherwise bad_at is None."""
    mcfg, zcfg, mp, zp, root_state = _setup(D, mh, zh, A, seed, zero, override)
    model = _Model(mcfg, mp, root_state, activation == "sigmoid", terminal_tol)
    rng = _Rng(seed if tie_seed is None else tie_seed, call_counter)
    order, log = [], dict(gap=np.inf, scale=0.0)

    def evaluation(obs):
        p, v = AO.evaluate(zcfg, zp, np.asarray(obs)[None])
        order.append(tuple(model.actions))  # nodes in order of expansion, by their action path
        return p[0], float(v[0])

    def puct(node, rng):
        ch = list(node.children.values())
        scores = np.array([c.value for c in ch]) + 1.0 * np.array([c.prior for c in ch]) * \
            np.array([np.sqrt(node.visit_count) / (c.visit_count + 1) for c in ch])
        rest = scores[scores < scores.max()]
        if rest.size:
            log["gap"] = min(log["gap"], scores.max() - rest.max())
        log["scale"] = max(log["scale"], np.abs(scores).max())
        return search.argmax(scores, rng=rng)

    try:
        with np.errstate(all="ignore"):
            root = search.mcts(root_state.astype(np.float64), model, puct, evaluation, S, A,
                               discount, rng=rng)
    except ValueError as e:
        assert "check_numerics" in str(e)
        return dict(bad_at=rng.k, nodes=len(order), simulations=model.simulations)
    tree = []
    for path in order:
        node = root
        for a in path:
            node = node.children[a]
        tree.append(node.children_visits)
    prior, value, acts = AO.forward(zcfg, zp, root_state[None].astype(np.float64))
    prior = np.exp(AO.log_softmax(prior))
    # sum_k |h_k wv_k| + |bv| of the root value: what bounds its float32 rounding error.
    terms = float(np.abs(acts[-1][0] * zp[AO.VW].astype(np.float64)[:, 0]).sum()
                  + abs(float(zp[AO.VB][0])))
    return dict(visits=root.children_visits, values=root.children_values, prior=prior[0],
                root_value=value[0], tree=np.array(tree), nodes=len(order),
                deepest=model.deepest, gap=log["gap"], scale=log["scale"],
                terminal_edges=len(model.terminal_edges), revisits=model.revisits,
                tol_gap=model.tol_gap, widest_tie=rng.widest, high_pick=rng.high_pick,
                selections=rng.k, root_value_terms=terms, bad_at=None,
                simulations=model.simulations,
                root_rewards=np.array([c.reward for c in root.children.values()], np.float64))
