"""Batch schedules: one learner created once at its maxima, then stepped through a list of
shapes below and across the shapes its workspaces were sized for, as data-parallel shares,
short last batches of a sequence dataset and a long-lived learner see them.

tests/test_batch_schedule_gpu.py runs each schedule on the kernels: every step against the
float64 oracle at the bars of the per-learner modules, teacher-forced, and one small step
bit for bit against a fresh learner restored to the same state.
tests/test_batch_schedule_cpu.py shows on the oracles alone that every shape is valid and
that one leaked row of an earlier, larger batch would be caught.  The builders here are numpy
only; batches and parameters come from the per-learner modules' own helpers (the same draws
their _run_steps / _compare make, so the CPU tests see the GPU tests' inputs).

Every schedule begins at the maxima (but for the data-parallel shares); the sizes after it
are the smallest that cross each boundary named in the table's comment.  Neighbouring batch sizes of the plane
learners differ by at most 37-fold, inside the step guard's apply window (2^-7 .. 2^7,
limit_cases.DQN_WINDOW_JUMPS), so no step of any schedule may be skipped.
"""

import numpy as np

from oracle import d4pg_oracle as D4
from oracle import impala_oracle as IM
from tests import ddpg_oracle as DD
from tests import dmpo_oracle as DM
from tests import limit_cases as C
from tests import mpo_oracle as MP
from tests import test_d4pg_gpu as d4pg_t
from tests import test_ddpg_gpu as ddpg_t
from tests import test_dmpo_gpu as dmpo_t
from tests import test_dqn_gpu as dqn_t
from tests import test_impala_gpu as impala_t
from tests import test_mpo_gpu as mpo_t
from tests import test_r2d2_learner_gpu as r2d2_t

# ------------------------------------------------------------------ DQN

# id -> net: ("mlp", obs_dim, hidden, A) | ("nature", A); max_batch; steps: the rows of each
# step; mean_over: the batch mean's denominator passed with every share (None: the rows).
#   dqn_mlp     37 rows are ragged against every tile; 1 and 5 leave 36 and 32 stale rows
#               in every workspace.
#   dqn_nature  the plane path: the fc tile partial, conv2_fwd's last two-frame block half
#               empty (1, 5, 37 are odd), the priority write-back riding conv1's weight
#               gradient (the step is given a table and keys), the plane scales moving with
#               the batch.
#   dqn_nature_mean_over  shares of a nominal 16-row rank batch, as replay/sharding hands
#               them out: the staged step with mean_over = 16.
DQN = {
    "dqn_mlp": dict(net=("mlp", 12, [32], 9), max_batch=37, steps=(37, 1, 5, 37)),
    "dqn_nature": dict(net=("nature", 18), max_batch=37, steps=(37, 1, 5, 37), rider=True),
    "dqn_nature_mean_over": dict(net=("nature", 18), max_batch=37, steps=(16, 9, 23, 16),
                                 mean_over=16),
}


def dqn_schedule(name):
    """-> net, params, target, batches (one transition batch per step)."""
    from acme_amd.networks import MLP, DQNAtariNetwork
    c = DQN[name]
    net = MLP(*c["net"][1:]) if c["net"][0] == "mlp" else DQNAtariNetwork(c["net"][1])
    rng = np.random.default_rng(list(name.encode()))
    batches = [dqn_t._batch(rng, B, net.obs_shape, net.num_actions, u8=net.obs_dtype == "uint8")
               for B in c["steps"]]
    return net, C.dqn_params(net, 1), C.dqn_params(net, 2), batches


# ------------------------------------------------------------------ IMPALA

# id -> cfg: IMPALAConfig fields; max: the creation's (max_batch, max_sequence_length);
# steps: (B, T) of each step; per_step: set_lstm_unroll(True).
#   impala_rg   the one-launch LSTM takes rg_single for B <= 16, rg_pairs for B <= 32 and
#               groups of 4 above: 40, 16, 17, 33, 3, 40 sequences visit quads, single,
#               pairs, quads, single, quads over one granule buffer sized for 40 sequences
#               and never cleared (lstm.h next_lstm_tags), at four unroll lengths.
#   impala_rg_per_step  the per-step kernels (set_lstm_unroll(True)).  They cannot run
#               impala_rg's shapes: the per-step forward holds every row's h in LDS
#               (lstm.h lstm_fwd_smem at the creation's max_batch must fit 64 KB, which
#               acme_impala_set_lstm_unroll checks), at H = 256 at most 30 sequences, so a
#               learner created for 40 refuses the per-step mode.  The schedule is impala_rg's
#               with 30 in place of 40 and 33: 16 and 17 sequences lie on either side of the
#               forward's 16-row chunk (kRowChunk), 30 is the largest creation.
#   impala_scan 70 > 64 sequences take the v-trace scan's second 64-sequence pass; 3 x 4
#               then leaves 67 sequences of stale LDS-staged rows, 65 x 3 has one sequence
#               in the second pass at another T.
#   impala_atari 64 frames are the fewest on the f16 plane path (use_p3: B * T >= 64);
#               3 x 16 = 48 and 2 x 5 = 10 frames run the f32 path on the same learner while
#               the parameter planes and their scale lag the parameters, then 64 again.
_IMPALA_RG = dict(torso="flat", obs_dim=12, lstm_size=256, head_size=64, num_actions=5)
_IMPALA_RG_STEPS = ((40, 8), (16, 8), (17, 5), (33, 2), (3, 8), (40, 8))
IMPALA = {
    "impala_rg": dict(cfg=_IMPALA_RG, max=(40, 8), steps=_IMPALA_RG_STEPS, one_launch=True),
    "impala_rg_per_step": dict(cfg=_IMPALA_RG, max=(30, 8), per_step=True,
                               steps=((30, 8), (16, 8), (17, 5), (30, 2), (3, 8), (30, 8))),
    "impala_scan": dict(cfg=dict(torso="flat", obs_dim=12, lstm_size=16, head_size=16,
                                 num_actions=5),
                        max=(70, 4), steps=((70, 4), (3, 4), (65, 3))),
    "impala_atari": dict(cfg=dict(torso="atari", lstm_size=256, head_size=64, num_actions=18),
                         max=(4, 16), steps=((4, 16), (3, 16), (2, 5), (4, 16)),
                         one_launch=True, planes=True),
}


def impala_schedule(name):
    """-> cfg, params, batches."""
    c = IMPALA[name]
    cfg = IM.IMPALAConfig(entropy_cost=0.01, baseline_cost=0.5, **c["cfg"])
    batches = [impala_t._batch(cfg, B, T, 60 + k) for k, (B, T) in enumerate(c["steps"])]
    return cfg, impala_t._params(cfg, 9), batches


# ------------------------------------------------------------------ R2D2

# id -> cfg: overrides of test_r2d2_learner_gpu._cfg; max; steps: (B, T); seed: _compare's.
#   r2d2_rg     the one-launch LSTM's row groups of 4: 9 = 2 groups + 1, 4 = one full group,
#               5 = one group + 1, 1 row; T from 10 down to 5 = burn_in + 2, the shortest
#               accepted: the time-major workspaces (h [T * B, H], q, g) re-laid at each
#               step's T and B inside allocations sized for 9 x 10.
#   r2d2_switch at H = 512 the one-launch kernels take B <= 32 (rg_shape: 256 workgroups),
#               but the boundary is not where the actual B crosses 32: acme_r2d2_create
#               allocates the granule buffers only when rg_shape(H, max_batch) holds, and
#               lstm_persistent needs them, so a learner created for 80 sequences runs the
#               per-step kernels at every B, and one created for B <= 32 the one-launch
#               kernels at every B (rg_shape is monotone in B).  No R2D2 learner switches
#               kernels on the actual B.  What 80 -> 32 -> 80 does cross is the per-step
#               forward's split of the batch over grid.y (h_prev of 80 rows exceeds one
#               workgroup's LDS, that of 32 does not), on workspaces laid out for 80.
#   r2d2_rg512  the one-launch kernels at H = 512 on their largest grid (32 sequences, 256
#               workgroups), then 5 (one row group + 1) and 32 again.
#   r2d2_atari  the plane path on 18, 4, 12, 18 frames.
R2D2 = {
    "r2d2_rg": dict(cfg=dict(lstm_size=256, head_size=64, num_actions=18, obs_dim=24,
                             burn_in_length=3),
                    max=(9, 10), steps=((9, 10), (4, 10), (5, 6), (1, 5), (9, 10)), seed=7),
    "r2d2_switch": dict(cfg=dict(lstm_size=512, head_size=64, num_actions=18, obs_dim=24,
                                 burn_in_length=2),
                        max=(80, 6), steps=((80, 6), (32, 6), (80, 6)), seed=8),
    "r2d2_rg512": dict(cfg=dict(lstm_size=512, head_size=64, num_actions=18, obs_dim=24,
                                burn_in_length=2),
                       max=(32, 6), steps=((32, 6), (5, 6), (32, 6)), seed=10),
    "r2d2_atari": dict(cfg=dict(torso="atari", num_actions=18, lstm_size=512, head_size=512,
                                obs_dim=0, burn_in_length=2, n_step=2),
                       max=(3, 6), steps=((3, 6), (1, 4), (2, 6), (3, 6)), seed=9),
}


def r2d2_cfg(name):
    return r2d2_t._cfg(**R2D2[name]["cfg"])


def r2d2_one_launch(name):
    """Whether the schedule's learner has the one-launch LSTM kernels (r2d2_learner.hip
    rg_shape at the creation's max_batch): rows in groups of 4, 16 units per workgroup, at
    most 256 workgroups."""
    H, B = R2D2[name]["cfg"]["lstm_size"], R2D2[name]["max"][0]
    return H in (256, 512) and -(-B // 4) * (H // 16) <= 256


def r2d2_schedule(name):
    """-> cfg, params, target, batches: the draws _compare makes for seed and steps."""
    c = R2D2[name]
    cfg, seed = r2d2_cfg(name), c["seed"]
    batches = [r2d2_t._batch(cfg, B, T, 100 * seed + k) for k, (B, T) in enumerate(c["steps"])]
    return cfg, r2d2_t._params(cfg, 10 + seed), r2d2_t._params(cfg, 20 + seed), batches


# ------------------------------------------------------------------ D4PG / DDPG / MPO / DMPO

# One schedule for the four: 45 rows are ragged against the row kernels' 4 and the 32-row
# tiles (one full tile + 13), 1 is the smallest batch, 37 = 32 + 5 follows it, 4 is exactly
# one row block.  MPO and DMPO pack num_samples x B sampled rows densely (row n * B + b)
# inside buffers sized 3 x 45.  Target periods of 2 (and 2 / 3) put copies inside the
# schedule.  pseed, bseed: the modules' _run_steps seeds (parameters pseed and pseed + 1,
# batch bseed + s, noise bseed + 100 + s).
# MPO's mean layer is scaled 3x, as in test_mpo_gpu.test_loss_options, so that samples leave
# [-1, 1] and the action penalty is not a near-total cancellation: at scale 1 the penalty
# temperature's gradient is 4.1e-4 at the one-row step, formed from O(1) terms, and one f32
# ulp of those (6.0e-8) is past its bar of 4.9e-8 whatever computes it (float32 oracle
# against float64 on that step: 5.6e-8; the kernel: 5.96e-8).  At scale 3 the gradient is
# 1.6e-2 and the float32 oracle is within a ninetieth of the bar at every step; no
# allowance is needed or made.
AC_STEPS = (45, 1, 37, 4, 45)
AC_MAX = 45
_MPO = dict(obs_dim=7, act_dim=3, policy_sizes=(36, 100), critic_sizes=(64, 44), num_samples=3,
            per_dim_constraining=True, action_penalization=True,
            target_policy_update_period=2, target_critic_update_period=3)
AC = {
    "d4pg": dict(cfg=D4.D4PGConfig(target_update_period=2), pseed=1, bseed=10),
    "ddpg": dict(cfg=DD.DDPGConfig(target_update_period=2), pseed=1, bseed=10),
    "mpo": dict(cfg=MP.MPOConfig(**_MPO), pseed=1, bseed=10, mean_scale=3.0),
    "dmpo": dict(cfg=DM.DMPOConfig(num_atoms=9, vmin=-1.0, vmax=5.0, init_scale=1.0, **_MPO),
                 pseed=1, bseed=10, critic_scale=4.0),
}
AC_MODULES = {"d4pg": d4pg_t, "ddpg": ddpg_t, "mpo": mpo_t, "dmpo": dmpo_t}


def dmpo_batch(cfg, B, seed):
    """test_dmpo_gpu._batch, whose pinned rewards need two rows: a one-row batch is row 0
    (reward -2.5, not terminal) of that seed's two-row draw.  From two rows on the batch
    takes every branch of the projection, which is asserted here."""
    if B >= 2:
        b = dmpo_t._batch(cfg, B, seed)
        dmpo_t._assert_projection_branches(cfg, b)
        return b
    return {k: v[:1].copy() for k, v in dmpo_t._batch(cfg, 2, seed).items()}


def ac_params(name):
    """-> params, target: the draws of the module's _run_steps."""
    c = AC[name]
    kw = {k: c[k] for k in ("mean_scale", "critic_scale") if k in c}
    draw = AC_MODULES[name]._random_params
    return draw(c["cfg"], c["pseed"], **kw), draw(c["cfg"], c["pseed"] + 1, **kw)


def ac_batch(name, s):
    """-> batch, noise (None for D4PG / DDPG) of step s."""
    c = AC[name]
    cfg, B = c["cfg"], AC_STEPS[s]
    mod = AC_MODULES[name]
    batch = dmpo_batch(cfg, B, c["bseed"] + s) if name == "dmpo" else \
        mod._batch(cfg, B, c["bseed"] + s)
    eps = mod._eps(cfg, B, c["bseed"] + 100 + s) if name in ("mpo", "dmpo") else None
    return batch, eps


# ------------------------------------------------------------------ shared

ALL = {**DQN, **IMPALA, **R2D2, **{k: dict(steps=AC_STEPS) for k in AC}}


def shape(step):
    """(B, T) of a step entry (T = 1 for transition batches)."""
    return step if isinstance(step, tuple) else (step, 1)


def donor(steps, k):
    """The step whose rows could be left in step k's workspaces: the latest earlier step
    with more sequences or a longer unroll whose sequences are at least as long (so that one
    of them, cut to T, is a row of this step's form).  None: nothing larger came before.
    Where the preceding step is larger in B at the same T it is the donor."""
    B, T = shape(steps[k])
    for j in range(k - 1, -1, -1):
        Bj, Tj = shape(steps[j])
        if Tj >= T and (Bj > B or Tj > T):
            return j
    return None


def small_step(steps):
    """The first step smaller than its predecessor (fewer rows in all)."""
    for k in range(1, len(steps)):
        (B, T), (Bp, Tp) = shape(steps[k]), shape(steps[k - 1])
        if B * T < Bp * Tp:
            return k
    raise AssertionError("no step follows a larger one")
