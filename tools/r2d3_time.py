"""Cost of mixing demonstration sequences into the R2D2 batches
(acme_amd.datasets.demonstrations.mix_sequence_demonstrations, csrc/demos.hip): the
headline layout, B = 32 sequences of T = 121 steps of an OAR observation with 84x84x4 uint8
frames (3.4 MB per row), demonstration ratio 0.25, a Uniform table as the R2D3 agent builds it.

Three measurements in one process:

  launch  acme_seq_demo_mix alone on a drawn batch, device events around STEPS launches, as
          ms per launch and bytes/s over the bytes the drawn demonstration rows move (rows
          written and windows read, counted per launch with tests/r2d3_oracle.py);
  gather  beside it, measured the same way in the same process and alternating with it round
          by round: the table's own acme_replay_sample_gather of the same batch (B rows read
          and written).  The overlay moves about a quarter of those bytes;
  step    R2D2Learner.step() (store_lstm_state=False) fed by the mixed and by the plain
          dataset, alternating round by round, host clock around steps ending in a device
          synchronise.

Prints one line per figure and a JSON line.

    python tools/r2d3_time.py [--out FILE]      (needs the GPU)
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
from acme_amd._lib import check, lib, stream_ptr  # noqa: E402
from acme_amd.adders import reverb as adders  # noqa: E402
from acme_amd.agents.r2d2.learning import R2D2Learner  # noqa: E402
from acme_amd.datasets import (SequenceDemonstrationStore, make_reverb_dataset,  # noqa: E402
                               mix_sequence_demonstrations)
from acme_amd.networks import LSTMState, R2D2AtariNetwork  # noqa: E402
from acme_amd.utils import counting, loggers  # noqa: E402
from acme_amd.wrappers import OAR  # noqa: E402
from tests import r2d3_oracle as oracle  # noqa: E402

B, A, RATIO, BURN_IN, TRACE, PERIOD, H = 32, 18, 0.25, 40, 80, 40, 512
T = BURN_IN + TRACE + 1
FRAME = (84, 84, 4)
REPLAY, EPISODES, EPISODE_STEPS = 64, 8, 300
LAUNCH_STEPS, LAUNCH_ROUNDS = 50, 5
WARMUP, STEPS, ROUNDS = 5, 20, 5
MIX_SEED = 1


def make_spec():
    action, reward = specs.DiscreteArray(A, np.int32), specs.Array((), np.float32)
    return specs.EnvironmentSpec(
        observations=OAR(specs.Array(FRAME, np.uint8), action, reward), actions=action,
        rewards=reward, discounts=specs.BoundedArray((), np.float32, 0, 1))


def make_table(dev, seed):
    extras = {"core_state": LSTMState(specs.Array((H,), np.float32),
                                      specs.Array((H,), np.float32))}
    table = replay.Table(adders.DEFAULT_PRIORITY_TABLE, replay.selectors.Uniform(),
                         replay.selectors.Fifo(), REPLAY, replay.rate_limiters.MinSize(1),
                         signature=adders.SequenceAdder.signature(make_spec(), extras),
                         seed=seed, device=dev, flush_every=4)
    rng = np.random.default_rng(0)
    frames = rng.integers(0, 256, (T + REPLAY,) + FRAME, dtype=np.uint8)
    for i in range(REPLAY):
        act = rng.integers(0, A, T).astype(np.int32)
        rew = rng.standard_normal(T).astype(np.float32)
        table.insert(adders.Step(
            observation=OAR(frames[i:i + T], act, rew), action=act, reward=rew,
            discount=np.ones(T, np.float32), start_of_episode=np.zeros(T, bool),
            extras={"core_state": LSTMState(np.zeros((T, H), np.float32),
                                            np.zeros((T, H), np.float32))}), 1.0)
    table.flush()
    return table


def make_store(table):
    rng = np.random.default_rng(1)
    eps = []
    for _ in range(EPISODES):
        act = rng.integers(0, A, EPISODE_STEPS).astype(np.int32)
        rew = rng.standard_normal(EPISODE_STEPS).astype(np.float32)
        obs = OAR(rng.integers(0, 256, (EPISODE_STEPS,) + FRAME, dtype=np.uint8), act, rew)
        eps.append((obs, act, rew, np.ones(EPISODE_STEPS, np.float32)))
    return SequenceDemonstrationStore(eps, table)


def make_dataset(table, store):
    ds = make_reverb_dataset(replay.Server([table]), batch_size=B, sequence_length=T)
    if store is not None:
        ds = mix_sequence_demonstrations(ds, store, RATIO, PERIOD, T, seed=MIX_SEED,
                                         record_is_demo=False)
    return ds


def event_ms(fn, steps):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for s in range(steps):
        fn(s)
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1) / steps


def host_ms(fn, steps, dev):
    torch.cuda.synchronize(dev)
    t0 = time.perf_counter()
    for _ in range(steps):
        fn()
    torch.cuda.synchronize(dev)
    return (time.perf_counter() - t0) * 1e3 / steps


def summary(v):
    return {"median_ms": statistics.median(v), "min": min(v), "max": max(v), "rounds": v}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None, help="also write the JSON result here")
    args = ap.parse_args()
    dev = torch.device("cuda", 0)
    res = {"batch": B, "sequence_length": T, "ratio": RATIO, "period": PERIOD,
           "replay_size": REPLAY, "episodes": EPISODES, "episode_steps": EPISODE_STEPS,
           "launch_steps": LAUNCH_STEPS, "launch_rounds": LAUNCH_ROUNDS, "warmup": WARMUP,
           "steps": STEPS, "rounds": ROUNDS}

    tables = {k: make_table(dev, 11) for k in ("plain", "mixed")}
    store = make_store(tables["mixed"])
    table = tables["mixed"]
    it = iter(make_dataset(table, store))
    next(it)
    raw, ptrs = it._slots[0][:2]  # noqa: SLF001
    launch = it._launch  # noqa: SLF001
    L, h, st = lib(), table.native.handle, stream_ptr()
    row_bytes = sum(f.nbytes for f in table.fields)           # a row written
    copied = sum(f.nbytes for f in store.step_fields)          # per step read
    res["row_bytes"] = row_bytes

    # Bytes the overlay moves, averaged over the timed launches (draw counters 0 ..
    # LAUNCH_STEPS - 1): per demonstration row the whole row written and the window's steps
    # read, the rows and windows being the oracle's (tests/r2d3_oracle.py).
    def mix_bytes():
        total = 0
        for s in range(LAUNCH_STEPS):
            _, rows = oracle.mix(store.lengths, MIX_SEED, s, RATIO, PERIOD, T, B)
            total += sum(row_bytes + (to - first) * copied for _, first, to in rows.values())
        return total / LAUNCH_STEPS

    res["mix_launch_bytes"] = mix_bytes()
    res["gather_bytes"] = 2.0 * B * row_bytes

    def do_mix(s):
        launch(s, B, ptrs, raw, 0, st)

    def do_gather(s):
        check(L.acme_replay_sample_gather(h, B, s, *raw, ptrs, st), "replay sample")

    for fn in (do_mix, do_gather):
        event_ms(fn, 10)
    ms = {"seq_demo_mix": [], "sample_gather": []}
    for _ in range(LAUNCH_ROUNDS):
        ms["seq_demo_mix"].append(event_ms(do_mix, LAUNCH_STEPS))
        ms["sample_gather"].append(event_ms(do_gather, LAUNCH_STEPS))
    res["launch"] = {k: summary(v) for k, v in ms.items()}
    res["launch"]["seq_demo_mix"]["bytes_per_s"] = (
        res["mix_launch_bytes"] / (res["launch"]["seq_demo_mix"]["median_ms"] * 1e-3))
    res["launch"]["sample_gather"]["bytes_per_s"] = (
        res["gather_bytes"] / (res["launch"]["sample_gather"]["median_ms"] * 1e-3))
    del it

    # the learner step fed by each
    learners = {}
    for k, t in tables.items():
        net = R2D2AtariNetwork(A)
        server = replay.Server([t])
        learners[k] = R2D2Learner(
            make_spec(), net, net, burn_in_length=BURN_IN, sequence_length=T,
            dataset=make_dataset(t, store if k == "mixed" else None),
            reverb_client=replay.Client(server), counter=counting.Counter(),
            logger=loggers.NoOpLogger(), store_lstm_state=False, max_replay_size=REPLAY,
            batch_size=B, seed=0, device=dev)
    for ln in learners.values():
        host_ms(ln.step, WARMUP, dev)
    ms = {k: [] for k in learners}
    for _ in range(ROUNDS):
        for k, ln in learners.items():
            ms[k].append(host_ms(ln.step, STEPS, dev))
    res["step"] = {k: summary(v) for k, v in ms.items()}
    for k, ln in learners.items():
        assert np.isfinite(ln.native.loss.item()), k
        res["step"][k]["skipped"] = int(ln.native.guard_state()["skipped"])
    p, m = (res["step"][k]["median_ms"] for k in ("plain", "mixed"))
    res["step"]["mixed_minus_plain_ms"] = m - p

    for k in ("seq_demo_mix", "sample_gather"):
        r = res["launch"][k]
        print(f"{k} alone: {r['median_ms']:.4f} ms per launch (min {r['min']:.4f}, max "
              f"{r['max']:.4f}), {r['bytes_per_s'] / 1e12:.3f} TB/s")
    print(f"bytes per launch: seq_demo_mix {res['mix_launch_bytes'] / 1e6:.1f} MB, "
          f"sample_gather {res['gather_bytes'] / 1e6:.1f} MB")
    print(f"step: plain {p:.3f} ms, mixed {m:.3f} ms, mixed - plain {m - p:+.3f} ms "
          f"(medians of {ROUNDS} rounds of {STEPS})")
    line = json.dumps(res)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
