"""Cost of mixing demonstrations into the DQN batches (acme_amd.datasets.demonstrations):
the headline layout, B = 512 transitions of 84x84x4 uint8 frames, demonstration ratio 0.25,
prefetch 4, a Uniform table as the DQfD agent builds it.

Three measurements in one process, the variants alternating round by round (ROUNDS rounds
of STEPS after WARMUP of each), so drift of the box hits all alike.  Variants: `plain` (the
table's dataset as the DQN agent uses it: pipelined draws), `plain_unpipelined` (the same with
ACME_REPLAY_PIPE=0: the draw the mix is built on) and `mixed`; mixed - plain_unpipelined is
the overlay launch's share, plain_unpipelined - plain the share of giving up the pipeline:

  draw    next(iterator) alone, host clock around STEPS draws ending in a device synchronise
          (the draws run on the dataset's stream);
  step    DQNLearner.step() fed by each dataset (draw + learner step + priority write-back),
          the same clock;
  launch  acme_demo_mix alone on a drawn batch, device events around STEPS launches.

Prints one line per figure and a JSON line.

    python tools/dqfd_time.py [--out FILE]      (needs the GPU)
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
from acme_amd import replay, specs  # noqa: E402
from acme_amd.adders import reverb as adders  # noqa: E402
from acme_amd.agents.dqn import DQNLearner  # noqa: E402
from acme_amd.datasets import (DemonstrationStore, make_reverb_dataset,  # noqa: E402
                               mix_demonstrations)
from acme_amd.networks import DQNAtariNetwork  # noqa: E402
from acme_amd.utils import counting, loggers  # noqa: E402

B, A, RATIO, PREFETCH, N_STEP, DISCOUNT = 512, 18, 0.25, 4, 5, 0.99
REPLAY, EPISODES, EPISODE_STEPS = 16384, 32, 64
WARMUP, STEPS, ROUNDS = 30, 200, 5


def make_table(dev, seed):
    spec = specs.EnvironmentSpec(
        observations=specs.Array((84, 84, 4), np.uint8), actions=specs.DiscreteArray(A, np.int32),
        rewards=specs.Array((), np.float32), discounts=specs.BoundedArray((), np.float32, 0, 1))
    table = replay.Table(adders.DEFAULT_PRIORITY_TABLE, replay.selectors.Uniform(),
                         replay.selectors.Fifo(), REPLAY, replay.rate_limiters.MinSize(1),
                         signature=adders.NStepTransitionAdder.signature(spec), seed=seed,
                         device=dev)
    table.native.fill_synthetic(REPLAY, layout=0, num_actions=A, seed=0)
    return table


def make_store(table):
    rng = np.random.default_rng(0)
    eps = [(rng.integers(0, 256, (EPISODE_STEPS, 84, 84, 4), dtype=np.uint8),
            rng.integers(0, A, EPISODE_STEPS).astype(np.int32),
            rng.standard_normal(EPISODE_STEPS).astype(np.float32),
            np.ones(EPISODE_STEPS, np.float32)) for _ in range(EPISODES)]
    return DemonstrationStore(eps, table)


VARIANTS = ("plain", "plain_unpipelined", "mixed")


def first_draw(variant, fn):
    """The iterator reads ACME_REPLAY_PIPE when its first draw allocates the ring."""
    if variant == "plain_unpipelined":
        os.environ["ACME_REPLAY_PIPE"] = "0"
    try:
        fn()
    finally:
        os.environ.pop("ACME_REPLAY_PIPE", None)


def make_dataset(table, store):
    ds = make_reverb_dataset(replay.Server([table]), batch_size=B, prefetch_size=PREFETCH)
    if store is not None:
        ds = mix_demonstrations(ds, store, RATIO, N_STEP, DISCOUNT, seed=1, record_is_demo=False)
    return ds


def host_ms(fn, steps, dev):
    torch.cuda.synchronize(dev)
    t0 = time.perf_counter()
    for _ in range(steps):
        fn()
    torch.cuda.synchronize(dev)
    return (time.perf_counter() - t0) * 1e3 / steps


def alternate(fns, dev):
    for fn in fns.values():
        host_ms(fn, WARMUP, dev)
    ms = {k: [] for k in fns}
    for _ in range(ROUNDS):
        for name, fn in fns.items():
            ms[name].append(host_ms(fn, STEPS, dev))
    return ms


def summary(v):
    return {"median_ms": statistics.median(v), "min": min(v), "max": max(v), "rounds": v}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None, help="also write the JSON result here")
    args = ap.parse_args()
    dev = torch.device("cuda", 0)
    res = {"batch": B, "ratio": RATIO, "prefetch": PREFETCH, "n_step": N_STEP,
           "replay_size": REPLAY, "episodes": EPISODES, "episode_steps": EPISODE_STEPS,
           "warmup": WARMUP, "steps": STEPS, "rounds": ROUNDS}

    # draw alone
    tables = {k: make_table(dev, 11) for k in VARIANTS}
    store = make_store(tables["mixed"])
    its = {k: iter(make_dataset(t, store if k == "mixed" else None)) for k, t in tables.items()}
    for k, it in its.items():
        first_draw(k, lambda it=it: next(it))
    assert its["plain"]._pipe is not None and its["plain_unpipelined"]._pipe is None  # noqa: SLF001
    ms = alternate({k: (lambda it=it: next(it)) for k, it in its.items()}, dev)
    res["draw"] = {k: summary(v) for k, v in ms.items()}

    # the mix launch alone, on the batch handed out last
    it = its["mixed"]
    raw, ptrs = it._slots[0][:2]  # noqa: SLF001
    native = store.upload(dev)
    launch = []
    for _ in range(ROUNDS):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for s in range(STEPS):
            native.mix_transitions(RATIO, N_STEP, DISCOUNT, 1, s, B, ptrs, raw[1], raw[2], raw[3],
                                   raw[4])
        e1.record()
        e1.synchronize()
        launch.append(e0.elapsed_time(e1) / STEPS)
    res["mix_launch"] = summary(launch)
    # bytes the launch moves at this ratio: two observations and an action, read and written
    row = 2 * 28224 + 4
    res["mix_launch"]["expected_bytes"] = 2.0 * RATIO * B * row
    del its, it

    # the learner step fed by each
    learners = {}
    for k, t in tables.items():
        net = DQNAtariNetwork(A)
        server = replay.Server([t])
        learners[k] = DQNLearner(net, net, discount=DISCOUNT, importance_sampling_exponent=0.2,
                                 learning_rate=1e-3, target_update_period=100,
                                 dataset=make_dataset(t, store if k == "mixed" else None),
                                 replay_client=replay.Client(server), counter=counting.Counter(),
                                 logger=loggers.NoOpLogger(), seed=0, device=dev,
                                 checkpoint=False)
        first_draw(k, learners[k].step)
    ms = alternate({k: ln.step for k, ln in learners.items()}, dev)
    res["step"] = {k: summary(v) for k, v in ms.items()}
    for k, ln in learners.items():
        ln.get_variables([])  # settles the issued steps
        assert np.isfinite(ln.native.loss.item()), k
        res["step"][k]["reissued_or_skipped"] = int(ln.native.skipped_steps)

    for what in ("draw", "step"):
        p, u, m = (res[what][k]["median_ms"] for k in VARIANTS)
        res[what]["mixed_minus_plain_ms"] = m - p
        res[what]["mixed_minus_plain_unpipelined_ms"] = m - u
        print(f"{what}: plain {p:.4f} ms, plain unpipelined {u:.4f} ms, mixed {m:.4f} ms; "
              f"mixed - plain {m - p:+.4f} ms, of which the overlay {m - u:+.4f} ms "
              f"(medians of {ROUNDS} rounds of {STEPS})")
    print(f"acme_demo_mix alone: {res['mix_launch']['median_ms']:.4f} ms per launch "
          f"({res['mix_launch']['expected_bytes'] / 1e6:.1f} MB expected traffic)")
    line = json.dumps(res)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
