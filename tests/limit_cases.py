"""Case tables and data-edge inputs of the declared-limit tests: every learner at the ends of
the ranges its create() accepts (include/acme_hip.h), and the inputs that random data never
produces (argmax ties, TD targets on an atom or clipped at either end, importance ratios
past f32 exp's range, rewards on both sides of the clip).

tests/test_limits_gpu.py runs each case on the kernels against the float64 oracles at the
bars the per-learner modules state; tests/test_limits_cpu.py checks on the oracle alone that
each data-edge input still exercises its edge and that every oracle runs every shape.  The
builders here are numpy only; the batches and parameters come from the per-learner modules'
own helpers.
"""

import numpy as np

from oracle import d4pg_oracle as D4
from oracle import dqn_oracle as DQ
from oracle import impala_oracle as IM
from oracle import r2d2_oracle as R2
from tests import ddpg_oracle as DD
from tests import dmpo_oracle as DM
from tests import mpo_oracle as MP
from tests import test_d4pg_gpu as d4pg_t
from tests import test_dqn_gpu as dqn_t
from tests import test_impala_gpu as impala_t
from tests import test_r2d2_learner_gpu as r2d2_t
from tests import test_step_guard_gpu as guard_t

# ------------------------------------------------------------------ DQN

# id -> (obs_dim, hidden, num_actions, batch).  loss_row's argmax reads the selector row 8
# entries at a time: A = 1 (one clamped group), 8 (one full group), 9 (one entry in the
# second), 63 (the largest, 7 of the last group).  0 and 8 hidden layers are the ends of
# ACME_MAX_MLP_LAYERS; the deep net has a layer of width 1.
DQN_MLP = {
    "a1": (12, [32], 1, 37),
    "a8": (12, [32], 8, 37),
    "a9": (12, [32], 9, 37),
    "a63": (12, [32], 63, 37),
    "linear_q": (12, [], 5, 37),
    "hidden8": (12, [20, 1, 7, 33, 64, 5, 12, 3], 5, 37),
}
DQN_ATARI = {"atari_a63": (63, 4), "atari_a1": (1, 4)}
DQN_TIES = ("tie_row", "tie_pair")
DQN_TIE_PAIR = (2, 8)  # j < k, in different 8-entry groups of the 9-action row


def dqn_params(net, seed):
    """net.init with random biases (init's are zero)."""
    p = net.init(seed)
    rng = np.random.default_rng(1000 + seed)
    for k in p:
        if k.endswith("/b"):
            p[k] = (0.1 * rng.standard_normal(p[k].shape)).astype(np.float32)
    return p


def dqn_mlp_case(name):
    """-> net, params, target, batch."""
    from acme_amd.networks import MLP
    obs_dim, hidden, A, B = DQN_MLP[name]
    net = MLP(obs_dim, hidden, A)
    batch = dqn_t._batch(np.random.default_rng(B + A), B, net.obs_shape, A, u8=False)
    return net, dqn_params(net, 1), dqn_params(net, 2), batch


def dqn_atari_case(name):
    from acme_amd.networks import DQNAtariNetwork
    A, B = DQN_ATARI[name]
    net = DQNAtariNetwork(A)
    batch = dqn_t._batch(np.random.default_rng(B + A), B, net.obs_shape, A, u8=True)
    return net, dqn_params(net, 1), dqn_params(net, 2), batch


def _raise_pair(q, j, k):
    """How much to add to columns j and k of q so that they exceed every other column of
    every row by at least 1."""
    others = np.delete(q, [j, k], axis=1)
    return float(np.max(others.max(axis=1) - q[:, j])) + 1.0


def dqn_tie_case(name):
    """-> net, params, target, batch, (j, k): the online net's selector rows tie between j
    and k (tie_pair: two identical columns raised above the rest; tie_row: a zero last layer
    with equal biases, every entry ties and j = 0, k = 1); the target's columns differ.
    The pair's identical weights are zero: a BLAS does not sum two equal columns in the same
    order (float64 dgemm gave 2 of 37 rows a last-bit difference between columns 2 and 8 of
    random equal weights), and 0 x + b is b in any order and any format."""
    from acme_amd.networks import MLP
    net = MLP(12, [32], 9)
    B = 37
    batch = dqn_t._batch(np.random.default_rng(77), B, net.obs_shape, 9, u8=False)
    params, target = dqn_params(net, 3), dqn_params(net, 4)
    w, b = params["mlp/linear_1/w"].copy(), params["mlp/linear_1/b"].copy()
    if name == "tie_row":
        j, k = 0, 1
        w[:] = 0.0
        b[:] = 0.3
    else:
        j, k = DQN_TIE_PAIR
        w[:, j] = w[:, k] = 0.0
        b[k] = b[j]
        params["mlp/linear_1/w"], params["mlp/linear_1/b"] = w, b
        q, _ = DQ.forward(dqn_t._cfg(net), params, batch["o_t"], np.float64)
        b[j] = b[k] = np.float32(b[j] + _raise_pair(q, j, k))
    params["mlp/linear_1/w"], params["mlp/linear_1/b"] = w, b
    return net, params, target, batch, (j, k)


def swap_columns(params, names, j, k):
    """params with columns j and k of the named tensors exchanged: the oracle on a target
    network so changed computes what a kernel breaking the tie towards k would."""
    out = dict(params)
    for n in names:
        x = params[n].copy()
        x[..., [j, k]] = x[..., [k, j]]
        out[n] = x
    return out


# ------------------------------------------------------------------ DQN acting (q_values)

# Frames an actor really sends (tests/test_acting_gpu.py; shown to produce their edge, or not,
# on the oracle alone by tests/test_acting_cpu.py).  id -> (frames, value, biased):
# black frames under net.init's zero biases (every torso activation and the hidden layer are
# identically zero, so the target activations' scale records see a maximum of 0), the same
# frames under dqn_params' non-zero biases (no activation tensor is zero), and one saturated
# frame.
DQN_ACTING_EDGES = {"black_zero_bias": (3, 0, False), "black_biased": (3, 0, True),
                    "saturated": (1, 255, True)}


def dqn_acting_edge(name):
    """-> net, params, target, frames (uint8 [n, 84, 84, 4])."""
    from acme_amd.networks import DQNAtariNetwork
    n, value, biased = DQN_ACTING_EDGES[name]
    net = DQNAtariNetwork(18)
    draw = dqn_params if biased else (lambda net_, seed: net_.init(seed))
    return net, draw(net, 1), draw(net, 2), np.full((n,) + net.obs_shape, value, np.uint8)


# ------------------------------------------------------------------ DQN plane-engine inputs

# Batch schedules of the learner step on frames that i.i.d. uniform bytes never produce
# (tests/test_plane_inputs_gpu.py; shown to produce their edge on the oracle alone by
# tests/test_plane_inputs_cpu.py).  id -> (biased, the frames of each batch in turn, the
# learner's learning rate).  Every batch is test_step_guard_gpu._batch's draw (actions,
# N(0, 1.5) rewards, discounts, probabilities) with its frames replaced, B = 5: conv2_fwd's
# last two-frame block half empty, the fc tile partial.
#   black   every byte 0 (under net.init's zero biases every activation, every input
#           gradient below the head and every weight gradient is identically zero);
#   random  _batch's own uniform bytes;
#   dark    bytes drawn from {0, 1};  saturated  every byte 255 (x1's maximum moves about
#           255-fold between the two);
#   sparse  an Atari-like stack: black background and a few rectangles of bytes in
#           128..255, o_t the stack of o_tm1 one position on (plane_sparse_frames).
DQN_PLANE_B = 5
# learning rate 0 where the schedule needs the biases to stay zero past the first update;
# black_after_update is black_between at the default rate: the update of the first batch
# leaves biases of about the learning rate, so the black batch's activations are those
# biases alone, about 2^-10 of the first batch's, and the third batch's 2^10 above them.
DQN_PLANE_SCHEDULES = {
    "black_first": (False, ("black", "random", "random"), 1e-3),
    "black_between": (False, ("random", "black", "random"), 0.0),
    "black_after_update": (False, ("random", "black", "random"), 1e-3),
    "black_biased": (True, ("black", "random", "random"), 1e-3),
    "dark_then_saturated": (False, ("dark", "saturated", "dark"), 1e-3),
    "sparse": (False, ("sparse", "sparse", "sparse"), 1e-3),
}


def plane_sparse_frames(rng, B):
    """-> o_tm1, o_t (uint8 [B, 84, 84, 4]).  Five 84 x 84 screens per row, each black but
    for three rectangles (3..10 pixels a side, bytes in 128..255, redrawn per screen as a
    sprite that moves); o_tm1 stacks screens 0..3 and o_t screens 1..4."""
    screens = np.zeros((B, 5, 84, 84), np.uint8)
    for b in range(B):
        for s in range(5):
            for _ in range(3):
                h, w = rng.integers(3, 11, 2)
                y, x = rng.integers(0, 84 - h), rng.integers(0, 84 - w)
                screens[b, s, y:y + h, x:x + w] = rng.integers(128, 256, (h, w), dtype=np.uint8)
    stack = lambda lo: np.ascontiguousarray(np.moveaxis(screens[:, lo:lo + 4], 1, -1))  # noqa: E731
    return stack(0), stack(1)


def _plane_frames(kind, rng, b):
    shape = b["o_tm1"].shape
    if kind == "random":
        return b["o_tm1"], b["o_t"]
    if kind == "sparse":
        return plane_sparse_frames(rng, shape[0])
    if kind == "dark":
        return (rng.integers(0, 2, shape, dtype=np.uint8), rng.integers(0, 2, shape, dtype=np.uint8))
    value = {"black": 0, "saturated": 255}[kind]
    return np.full(shape, value, np.uint8), np.full(shape, value, np.uint8)


def dqn_plane_schedule(name):
    """-> net, params, target, batches (a list of transition batches), learning rate."""
    from acme_amd.networks import DQNAtariNetwork
    biased, kinds, lr = DQN_PLANE_SCHEDULES[name]
    net = DQNAtariNetwork(18)
    draw = dqn_params if biased else (lambda net_, seed: net_.init(seed))
    rng = np.random.default_rng(list(name.encode()))
    batches = []
    for kind in kinds:
        b = guard_t._batch(rng, DQN_PLANE_B, 18)
        b["o_tm1"], b["o_t"] = _plane_frames(kind, rng, b)
        batches.append(b)
    return net, draw(net, 1), draw(net, 2), batches, lr


# The step guard's window (rescale.h): a rescale leaves a tensor's maximum times its write
# scale in [2^7, 2^8), and the next step is applied while that product stays in [1, 65520).
# A g-fold jump of the tensor therefore must apply when [2^7 g, 2^8 g) lies inside
# [1, 65520) (2^-7 <= g <= 2^7) and must skip when it lies outside whatever the mantissa
# (g >= 2^9: overflow; g <= 2^-8: underflow).  id -> (log2 g, log2 r0, log2 r1 = log2 g r0,
# skips, overflow): the innermost power of two that must apply and, with a binade to spare,
# one that must skip, on either side.
DQN_WINDOW_JUMPS = {
    "up7_applies": (7, -8, -1, 0, False),
    "down6_applies": (-6, -1, -7, 0, False),
    "up10_skips": (10, -11, -1, 1, True),
    "down9_skips": (-9, -1, -10, 1, False),
}
# The parameter planes share one scale record (the largest parameter, 0.125, at 2^7), so a
# tensor far below it loses its low plane: test_step_guard_gpu's head scale 1e-4 is kept,
# and the remaining factor (q must be below 2^-7 of the smaller reward, 2^-18) comes from
# the hidden layer's weights, an exact power of two 2^-4.  With zero biases q is linear in
# each: max |q| falls from 0.14 to 8.6e-7.
DQN_WINDOW_HEAD_SCALE = 1e-4
DQN_WINDOW_HIDDEN_SCALE = 2.0 ** -4


def dqn_window_case(name):
    """-> net, params, target, first, second, g: two batches on the same frames, actions,
    discounts (0) and probabilities whose constant rewards are r0 and g r0.  Every |TD| is
    below 1 (Huber's quadratic zone) and q is negligible beside either reward, so the head dZ
    and with it the whole input-gradient chain and every weight gradient scale by g, while
    the forward activations do not move."""
    from acme_amd.networks import DQNAtariNetwork
    lg, l0, l1, _, _ = DQN_WINDOW_JUMPS[name]
    assert l0 + lg == l1
    net = DQNAtariNetwork(18)
    params, target = guard_t._head_scaled_params(net, DQN_WINDOW_HEAD_SCALE)
    for p in (params, target):
        k = "duelling_q_network/hidden/w"
        p[k] = p[k] * np.float32(DQN_WINDOW_HIDDEN_SCALE)
    first = guard_t._batch(np.random.default_rng(20), DQN_PLANE_B, 18, r=2.0 ** l0, d=0.0)
    second = dict(first, r_t=np.full(DQN_PLANE_B, 2.0 ** l1, np.float32))
    return net, params, target, first, second, 2.0 ** lg


def dqn_uncalibrated_case():
    """-> net, params, target, batch: one of _batch's random batches for a learner whose
    scale records are restored at 1 (the scale state of a checkpoint taken before its first
    step), so its first step is not calibrated.  x3's maximum is below 1: at scale 1 its
    planes underflow, and that first step, the learner's verdict 0, must be skipped."""
    from acme_amd.networks import DQNAtariNetwork
    net = DQNAtariNetwork(18)
    batch = guard_t._batch(np.random.default_rng(30), DQN_PLANE_B, 18)
    return net, net.init(1), net.init(2), batch


# ------------------------------------------------------------------ recurrent plane inputs

# The recurrent learners' first (calibrating) plane step on black frames under zero biases
# (the torso's activations and input gradients all zero), then two steps on the modules' own
# random batches.  IMPALA at 4 x 16 = 64 frames, the fewest that take the plane path; R2D2's
# Atari network at 3 x 6.


def zero_biases(params):
    return {k: (np.zeros_like(v) if k.endswith("/b") else v) for k, v in params.items()}


def impala_plane_black():
    """-> cfg, B, T, params, batches."""
    cfg = IM.IMPALAConfig(num_actions=18, torso="atari", lstm_size=256, head_size=64,
                          entropy_cost=0.01, baseline_cost=0.5)
    B, T = 4, 16
    batches = [impala_t._batch(cfg, B, T, 40 + k) for k in range(3)]
    batches[0]["obs"] = np.zeros_like(batches[0]["obs"])
    return cfg, B, T, zero_biases(impala_t._params(cfg, 9)), batches


def r2d2_plane_black():
    """-> cfg, B, T, params, target, batches."""
    cfg = r2d2_t._cfg(torso="atari", num_actions=18, lstm_size=512, head_size=512, obs_dim=0,
                      burn_in_length=2, n_step=2)
    B, T = 3, 6
    batches = [r2d2_t._batch(cfg, B, T, 50 + k) for k in range(3)]
    batches[0]["obs"] = np.zeros_like(batches[0]["obs"])
    return (cfg, B, T, zero_biases(r2d2_t._params(cfg, 14)), zero_biases(r2d2_t._params(cfg, 24)),
            batches)


# ------------------------------------------------------------------ IMPALA

# Flat torso, obs_dim 12.  B, T, H (lstm_size), A; head: head_size (default 16); kw: learner
# options; edit: a change to the module's random batch / parameters (impala_case).
IMPALA = {
    # B > 64 (the vs scan's second 64-sequence pass) and 2600 rows > kVtraceLdsRows.
    "global_scan": dict(B=130, T=20, H=16, A=5),
    # The longest unroll with the value in lane 63.
    "t64_a63": dict(B=3, T=64, H=16, A=63),
    # The one-launch unroll across 63 hand-offs (7-bit tag window).
    "t64_one_launch": dict(B=3, T=64, H=256, A=5, head=64, one_launch=True),
    "a1": dict(B=4, T=6, H=16, A=1),
    "head4": dict(B=4, T=6, H=16, A=5, head=4),
    # (8 x 10: at 4 x 6 this batch's three loss terms cancel to 0.013, a hundredth of each.)
    "reward_clip": dict(B=8, T=10, H=16, A=5, kw=dict(max_abs_reward=1.0)),
    "discount_rows": dict(B=4, T=6, H=16, A=5, edit="discount_rows"),
    "rho_overflow": dict(B=8, T=10, H=16, A=5, edit="rho_overflow"),
    "rho_underflow": dict(B=8, T=10, H=16, A=5, edit="rho_underflow"),
}


def impala_case(name):
    """-> cfg, B, T, params, batch, learner kwargs."""
    c = IMPALA[name]
    kw = dict(c.get("kw", {}))
    cfg = IM.IMPALAConfig(num_actions=c["A"], torso="flat", obs_dim=12, lstm_size=c["H"],
                          head_size=c.get("head", 16), entropy_cost=0.01, baseline_cost=0.5,
                          **kw)
    B, T, A = c["B"], c["T"], c["A"]
    params = impala_t._params(cfg, 1)
    batch = impala_t._batch(cfg, B, T, 2)
    edit = c.get("edit")
    if edit == "discount_rows":  # sequence 0 ends at every step, sequence 1 never
        batch["discount"][0] = 0.0
        batch["discount"][1] = 1.0
    if edit in ("rho_overflow", "rho_underflow"):
        # Behaviour logits x 60: log mu(a) of an unlikely action is far below -89, so
        # rho = pi / mu overflows f32 exp and min(1, inf) must be 1.
        batch["behaviour_logits"] = batch["behaviour_logits"] * np.float32(60.0)
    if edit == "rho_underflow":
        # A peaked policy as well: log pi(a) far below -104 on other rows, rho underflows to 0.
        w = params[f"{IM.PREFIX}/policy_value/w"].copy()
        w[:, :A] *= np.float32(100.0)
        params[f"{IM.PREFIX}/policy_value/w"] = w
    return cfg, B, T, params, batch, kw


# ------------------------------------------------------------------ R2D2

# Flat torso through test_r2d2_learner_gpu._compare (its _cfg defaults: A 5, obs 12, LSTM 16,
# head 8, burn-in 2, n-step 3).  cfg: overrides; B, T; one_launch: assert no spin timeout.
R2D2 = {
    "a1": dict(cfg=dict(num_actions=1), B=3, T=9),
    "a63": dict(cfg=dict(num_actions=63), B=3, T=9),
    # Past one wave of head outputs (A + 1 > 64): the head epilogue strides.
    "a64": dict(cfg=dict(num_actions=64), B=3, T=9),
    "a70": dict(cfg=dict(num_actions=70), B=3, T=9),
    "a1024": dict(cfg=dict(num_actions=1024), B=2, T=5),
    # The Atari torso's plane path: the embedding tail of dW_i (lstm.h oar_wgrad_tail_kernel)
    # takes the A + 1 = 71 rows in two chunks of LDS accumulators.
    "atari_a70": dict(cfg=dict(torso="atari", obs_dim=0, num_actions=70, burn_in_length=1,
                               n_step=2), B=2, T=4),
    # 67 loss steps: the loss kernel's second t += 64 stride, per-step LSTM launches.
    "t70_per_step": dict(cfg=dict(burn_in_length=2, lstm_size=16), B=3, T=70),
    "t70_one_launch": dict(cfg=dict(burn_in_length=2, lstm_size=256, head_size=64,
                                    num_actions=18, obs_dim=24), B=5, T=70, one_launch=True),
    # kMaxSeq: the last tag of the 8-bit window.
    # f32_errors_bar: among ~500 TD errors one lies within 1.3e-4 of zero, where one f32 ulp
    # of q (6e-8) is already past the module's relative bar of 1e-4 and the float32 oracle
    # itself is 2.8e-4 (per-step shape) and 6.9e-4 (one-launch shape) from float64.  The
    # relative bar of these two cases is 4x that error, measured by r2d2_errors_rtol on the
    # case's own inputs; the absolute bar (2.5e-4), the bitwise loss checks and every other
    # bar of _compare stay.  The kernels measured 5.7e-4 and 2.3e-4.
    "t256_per_step": dict(cfg=dict(burn_in_length=0, lstm_size=16), B=2, T=256,
                          f32_errors_bar=True),
    "t256_one_launch": dict(cfg=dict(burn_in_length=3, lstm_size=256), B=2, T=256,
                            one_launch=True, f32_errors_bar=True),
}
R2D2_SEED = 0  # _compare's seed for the table above
R2D2_TIE = dict(cfg=dict(num_actions=9), B=3, T=9, seed=0, pair=(2, 8))
R2D2_ADV = ("r2d2_atari_network/duelling_q_network/mlp_1/linear_1/w",
            "r2d2_atari_network/duelling_q_network/mlp_1/linear_1/b")


def r2d2_cfg(case):
    return r2d2_t._cfg(**case["cfg"])


def r2d2_errors_rtol(case):
    """The end-to-end errors' relative bar of a case: the module's 1e-4, or with
    f32_errors_bar 4x the float32 oracle's largest relative error against float64 on the
    inputs _compare draws for its first step (never below 1e-4)."""
    if not case.get("f32_errors_bar"):
        return 1e-4
    cfg, B, T = r2d2_cfg(case), case["B"], case["T"]
    batch = r2d2_t._batch(cfg, B, T, 100 * R2D2_SEED)
    p, t = r2d2_t._params(cfg, 10 + R2D2_SEED), r2d2_t._params(cfg, 20 + R2D2_SEED)
    e64 = R2.loss_and_grads(cfg, p, t, batch, np.float64)[0]["errors"]
    e32 = np.asarray(R2.loss_and_grads(cfg, p, t, batch, np.float32)[0]["errors"], np.float64)
    return max(1e-4, 4.0 * float(np.max(np.abs(e32 - e64) / np.abs(e64))))


def r2d2_tie_inputs():
    """-> cfg, B, T, params_fn, batch, (j, k).  params_fn(cfg, seed) is _params with, for the
    online network's seed, advantage columns j and k identical (zero weights, as
    dqn_tie_case) and raised until q[j] = q[k] is the maximum of every row of the batch
    _compare draws for its one step."""
    c = R2D2_TIE
    cfg = r2d2_cfg(c)
    B, T, seed, (j, k) = c["B"], c["T"], c["seed"], c["pair"]
    batch = r2d2_t._batch(cfg, B, T, 100 * seed)
    online = r2d2_t._params(cfg, 10 + seed)
    w, b = online[R2D2_ADV[0]].copy(), online[R2D2_ADV[1]].copy()
    w[:, j] = w[:, k] = 0.0
    b[k] = b[j]
    online[R2D2_ADV[0]], online[R2D2_ADV[1]] = w, b
    q, _ = R2.forward(cfg, online, batch, np.float64)
    # Raising two of A advantages by d raises their q by d (1 - 2 / A) and lowers the rest by
    # 2 d / A: the gap grows by d, as for a plain head.
    b[j] = b[k] = np.float32(b[j] + _raise_pair(q.reshape(-1, cfg.num_actions), j, k))
    online[R2D2_ADV[1]] = b

    # The target's advantage of k is 4 above what it drew: a bootstrap from k is O(1) away.
    target = r2d2_t._params(cfg, 20 + seed)
    tb = target[R2D2_ADV[1]].copy()
    tb[k] += np.float32(4.0)
    target[R2D2_ADV[1]] = tb

    draw = r2d2_t._params  # bound now: the caller puts params_fn in its place

    def params_fn(cfg_, s):
        fixed = {10 + seed: online, 20 + seed: target}
        return dict(fixed[s]) if s in fixed else draw(cfg_, s)

    return cfg, B, T, params_fn, batch, (j, k)


# ------------------------------------------------------------------ D4PG / DDPG


def _ac(mod, obs, act, policy, critic, **kw):
    return mod(obs_dim=obs, act_dim=act, policy_sizes=policy, critic_sizes=critic,
               action_min=(-1.0,) * act, action_max=(1.0,) * act, target_update_period=2, **kw)


# id -> (config, batch rows).  obs + act = 64 and act = 16 (kMaxIn, ACME_D4PG_MAX_ACT) on the
# narrowest layers with every lane an atom; the smallest inputs and support on four layers
# each; the largest batch.
D4PG = {
    "in64_k64": (_ac(D4.D4PGConfig, 48, 16, (4,), (4,), num_atoms=64, vmin=-1.0, vmax=1.0), 9),
    "in2_k2_layers4": (_ac(D4.D4PGConfig, 1, 1, (8, 12, 16, 20), (20, 16, 12, 8), num_atoms=2), 9),
    "rows65536": (_ac(D4.D4PGConfig, 3, 2, (8,), (8,), num_atoms=5), 65536),
}
# dq/da of a few of the 65536 rows is ill-conditioned in f32 whatever computes it: the float32
# oracle is 1.20e-5 from float64 there (1.5x the bar: rtol 1e-4 + 2e-6 of the scale, 1), the
# kernel 1.25e-5 on 3 of 131072 elements.  That case's dqda may miss the bar by 4x the float32
# oracle's error on the same inputs (d4pg_dqda_allowance); no other quantity has an allowance.
D4PG_F32_DQDA = ("rows65536",)
D4PG_PROJECTION = _ac(D4.D4PGConfig, 3, 2, (8,), (8,), num_atoms=21, vmin=-10.0, vmax=10.0)
# Atom spacing exactly 1.  Terminal rows (d = 0): on an atom at both ends and in the middle
# (rows 0-3), mid-way between atoms (4, 7), clipped on both sides (5, 6); bootstrapped rows
# with the whole support clipped at either end (8-11: 3 + 0.96 z and 7 + 0.96 z cross 10,
# -3 + 0.96 z crosses -10) and an atom's width from an atom and from the ends (12-15).
PROJECTION_R = [-10, 10, 0, 1, 0.5, -25, 25, -9.5, 3, -3, 7, 7, 1e-3, -1e-3, 9.999, -9.999]
PROJECTION_D = [0, 0, 0, 0, 0, 0, 0, 0, 1, 1, 1, 0.5, 1, 1, 1, 1]

DDPG = {
    "in64": (_ac(DD.DDPGConfig, 48, 16, (4,), (4,)), 9),
    "in2_layers4": (_ac(DD.DDPGConfig, 1, 1, (8, 12, 16, 20), (20, 16, 12, 8)), 9),
    "rows65536": (_ac(DD.DDPGConfig, 3, 2, (8,), (8,)), 65536),
}


def d4pg_dqda_allowance(cfg, params, target, batch):
    """4x the float32 oracle's largest dqda error against float64."""
    o64, _ = D4.d4pg_loss_and_grads(cfg, params, target, batch, np.float64)
    o32, _ = D4.d4pg_loss_and_grads(cfg, params, target, batch, np.float32)
    return 4.0 * float(np.abs(np.asarray(o32["dqda"], np.float64) - o64["dqda"]).max())


def d4pg_projection_batch():
    cfg = D4PG_PROJECTION
    b = d4pg_t._batch(cfg, len(PROJECTION_R), 5)
    b["r_t"] = np.asarray(PROJECTION_R, np.float32)
    b["d_t"] = np.asarray(PROJECTION_D, np.float32)
    return cfg, b


# ------------------------------------------------------------------ MPO / DMPO


def _mpo(mod, obs, act, N, **kw):
    base = dict(obs_dim=obs, act_dim=act, policy_sizes=(8,), critic_sizes=(8,), num_samples=N,
                target_policy_update_period=2, target_critic_update_period=3)
    base.update(kw)
    return mod(**base)


# id -> (config, max_batch = batch rows).  obs + act = 64 with the widest action; 64 samples
# of 2048 states = ACME_MPO_MAX_ROWS sampled rows; DMPO also at both ends of num_atoms.
MPO = {
    "in64": (_mpo(MP.MPOConfig, 48, 16, 3), 5),
    "rows131072": (_mpo(MP.MPOConfig, 3, 2, 64), 2048),
}


def mpo_target(name, cfg, target):
    """The target parameters of an MPO case.  loss_temperature = T (epsilon + mean_b
    logmeanexp_n(q / T)) moves one for one with the mean sampled q and has no allowance
    (test_dmpo_gpu's docstring): at rows131072 the drawn critic leaves it at 0.014, where
    f32 rounding of its O(1) terms is all that is left, so that case's target critic's
    output bias is one higher (loss_temperature 1.01)."""
    if name != "rows131072":
        return target
    out = dict(target)
    bias = MP.critic_tensor_shapes(cfg)[-1][0]
    assert bias.endswith("/b")
    out[bias] = target[bias] + np.float32(1.0)
    return out


_DM = dict(vmin=-1.0, vmax=5.0, init_scale=1.0)  # test_dmpo_gpu's narrow support
DMPO = {
    "in64_k64": (_mpo(DM.DMPOConfig, 48, 16, 3, num_atoms=64, **_DM), 5),
    "in64_k2": (_mpo(DM.DMPOConfig, 48, 16, 3, num_atoms=2, **_DM), 5),
    "rows131072_k64": (_mpo(DM.DMPOConfig, 3, 2, 64, num_atoms=64, **_DM), 2048),
    "rows131072_k2": (_mpo(DM.DMPOConfig, 3, 2, 64, num_atoms=2, **_DM), 2048),
}
