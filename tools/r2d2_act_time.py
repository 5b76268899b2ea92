"""Cost of one R2D2 acting step (acme_r2d2_q_step) on the headline network: Atari torso,
LSTM 512, duelling [512], A = 18, at rows 1 (one actor) and rows 32 (max_batch).

Two learners in one process, the variants alternating round by round (ROUNDS rounds of
STEPS calls after WARMUP of each), so drift of the box hits both alike:

  unfused  launch_duel_head_finish followed by acme_epsilon_greedy's launch (the default);
  fused    the head's split-K finish and the epsilon-greedy selection in one launch
           (duel_head_act_kernel, ACME_V_R2ACT=1 at the learner's creation).

Per variant and row count:

  device   time per q_step from device events around STEPS calls (q, actions and the state
           in place all requested);
  actor    host wall time per RecurrentActor.select_action on an R2D2Policy (rows 1 only:
           upload of the observation, the q_step, download of the action and of the state
           that went into the step).

Prints one line per figure (median over the rounds, and the rounds' spread) and a JSON line.

    python tools/r2d2_act_time.py [--out FILE]      (needs the GPU)
"""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from acme_amd._lib import lib  # noqa: E402
from acme_amd.agents.actors import RecurrentActor  # noqa: E402
from acme_amd.agents.r2d2.learning import R2D2Policy  # noqa: E402
from acme_amd.native import NativeR2D2  # noqa: E402
from acme_amd.networks import R2D2AtariNetwork  # noqa: E402
from acme_amd.wrappers import OAR  # noqa: E402

A, H, MAX_BATCH, BURN, SEQ = 18, 512, 32, 2, 4
WARMUP, STEPS, ROUNDS = 20, 200, 5
VARIANTS = ("fused", "unfused")


def make_learner(variant, net):
    lib().acme_tune_set(b"R2ACT", 1 if variant == "fused" else 0)  # read at creation
    try:
        n = NativeR2D2(num_actions=A, max_batch=MAX_BATCH, max_sequence_length=SEQ,
                       burn_in_length=BURN, lstm_size=H, head_size=H)
    finally:
        lib().acme_tune_set(b"R2ACT", 0)
    n.set_params(net.init(1), net.init(2))
    return n


def device_us(n, rows, rng):
    dev = n.device
    obs = torch.as_tensor(rng.integers(0, 256, (rows, 84, 84, 4), dtype=np.uint8)).to(dev)
    pa = torch.as_tensor(rng.integers(0, A, rows).astype(np.int32)).to(dev)
    pr = torch.as_tensor(rng.standard_normal(rows).astype(np.float32)).to(dev)
    h = torch.zeros(rows, H, dtype=torch.float32, device=dev)
    c = torch.zeros(rows, H, dtype=torch.float32, device=dev)
    out = [torch.empty(rows, A, dtype=torch.float32, device=dev),
           torch.empty(rows, dtype=torch.int32, device=dev), h, c]

    def call(k):
        n.q_step(obs, pa, pr, h, c, epsilon=0.01, seed=0, step=k, out=out)

    for k in range(WARMUP):
        call(k)
    start, end = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize(dev)
    start.record()
    for k in range(STEPS):
        call(WARMUP + k)
    end.record()
    torch.cuda.synchronize(dev)
    return start.elapsed_time(end) * 1e3 / STEPS


def actor_us(n, net, rng):
    actor = RecurrentActor(R2D2Policy(n, net, 0.01, seed=0), net.initial_state)
    frames = rng.integers(0, 256, (8, 84, 84, 4), dtype=np.uint8)
    obs = [OAR(f, np.int32(1), np.float32(0.5)) for f in frames]
    for k in range(WARMUP):
        actor.select_action(obs[k % len(obs)])
    torch.cuda.synchronize(n.device)
    t0 = time.perf_counter()
    for k in range(STEPS):
        actor.select_action(obs[k % len(obs)])
    return (time.perf_counter() - t0) * 1e6 / STEPS


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out")
    args = ap.parse_args()
    net = R2D2AtariNetwork(A, lstm_size=H, head_size=H)
    learners = {v: make_learner(v, net) for v in VARIANTS}
    rng = np.random.default_rng(0)
    runs = {}
    for _ in range(ROUNDS):
        for v in VARIANTS:
            for rows in (1, MAX_BATCH):
                runs.setdefault(f"device_us_rows{rows}_{v}", []).append(
                    device_us(learners[v], rows, rng))
            runs.setdefault(f"actor_us_{v}", []).append(actor_us(learners[v], net, rng))
    result = {"network": f"atari H{H} A{A}", "warmup": WARMUP, "steps": STEPS, "rounds": ROUNDS}
    for key, xs in runs.items():
        result[key] = {"median": statistics.median(xs), "min": min(xs), "max": max(xs),
                       "rounds": xs}
        print(f"{key:28s} median {statistics.median(xs):9.2f} us   "
              f"(rounds {min(xs):.2f} .. {max(xs):.2f})")
    for rows in (1, MAX_BATCH):
        f, u = result[f"device_us_rows{rows}_fused"], result[f"device_us_rows{rows}_unfused"]
        spread = max(f["max"] - f["min"], u["max"] - u["min"])
        result[f"unfused_minus_fused_us_rows{rows}"] = u["median"] - f["median"]
        result[f"round_spread_us_rows{rows}"] = spread
        print(f"rows {rows}: unfused - fused {u['median'] - f['median']:+.2f} us, "
              f"round-to-round spread {spread:.2f} us")
    line = json.dumps(result)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as fh:
            fh.write(line + "\n")


if __name__ == "__main__":
    main()
