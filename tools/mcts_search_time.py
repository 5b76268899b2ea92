"""Times of the MCTS actor's tree search on the learned model, host and device: observations
10 x 5 (Catch), hidden (50,), 3 actions, 50 simulations, the reference example's sizes.

  acting   MCTSActor.select_action with search="host" (search.mcts: a launch and a blocking
           copy per tree edge and per leaf) and search="native" (acme_mcts_search_run: one
           launch, one packed copy), on one model and one learner in one process: wall time per
           action, ROUNDS rounds of ACTIONS actions of each, alternating per round, after
           WARMUP actions of each.  The two actors see the same observations; the host actor's
           action drives the environment.
  device   the native call alone between device events, CALLS calls per window, with the
           weights staged into LDS and forced to stream from global memory / L2, alternating
           in ROUNDS rounds.

    python tools/mcts_search_time.py [--out FILE]      (needs the GPU)
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
from acme_amd import specs  # noqa: E402
from acme_amd.native import NativeMCTSSearch  # noqa: E402
from acme_amd.networks import PolicyValueMLP  # noqa: E402

OBS, HIDDEN, ACT, RING, SIMULATIONS = 50, (50,), 3, 1000, 50
WARMUP, ACTIONS, CALLS, ROUNDS = 3, 20, 200, 5
DEFAULT_OUT = os.path.join("profiles", "mcts_search", "mcts_search_time.json")


def _summary(v):
    return {"median": statistics.median(v), "min": min(v), "max": max(v), "rounds": v}


def _agent_parts(dev):
    from acme_amd.agents.mcts import AZLearner
    from acme_amd.agents.mcts.models import MLPModel
    from acme_amd.environments.catch import Catch
    from acme_amd.optimizers import Adam
    from acme_amd.utils import loggers
    env = Catch(rows=10, columns=5, seed=0)
    spec = specs.make_environment_spec(env)
    learner = AZLearner(PolicyValueMLP(OBS, HIDDEN, ACT), Adam(1e-3), iter(()), discount=1.0,
                        batch_size=16, logger=loggers.NoOpLogger(), device=dev)
    return env, spec, learner, MLPModel(spec, RING, 16, HIDDEN, device=dev)


def time_acting(env, spec, learner, model):
    from acme_amd.agents.mcts import MCTSActor
    np.random.seed(0)
    actors = {k: MCTSActor(spec, model, learner, discount=1.0, num_simulations=SIMULATIONS,
                           search=k) for k in ("host", "native")}
    ms = {k: [] for k in actors}
    ts = env.reset()

    def act(name, timed):
        """ACTIONS actions of one actor; the model follows the environment through the host
        actor's observe alone (both actors share it)."""
        nonlocal ts
        total = 0.0
        for _ in range(timed):
            t0 = time.perf_counter()
            action = actors[name].select_action(ts.observation)
            total += time.perf_counter() - t0
            prev, ts = ts, env.step(action)
            model.update(prev, action, ts)
            if ts.last():
                ts = env.reset()
        return total / timed * 1e3

    for name in actors:
        act(name, WARMUP)
    for _ in range(ROUNDS):
        for name in actors:
            ms[name].append(act(name, ACTIONS))
    return {"simulations": SIMULATIONS, "actions_per_round": ACTIONS,
            "ms_per_action": {k: _summary(v) for k, v in ms.items()}}


def time_device(dev, env, learner, model):
    model.reset(env.reset().observation)
    searches = {"lds_resident": NativeMCTSSearch(learner.native, model.native, SIMULATIONS),
                "streamed": NativeMCTSSearch(learner.native, model.native, SIMULATIONS,
                                             stream_weights=True)}
    out = torch.empty(3 * ACT + 4, dtype=torch.float32, device=dev)
    run = lambda n, i: n.run(model.state_row, SIMULATIONS, 1.0, call_counter=i, out=out)  # noqa
    rows = {}
    for name, n in searches.items():
        for i in range(WARMUP):
            run(n, i)
        rows[name] = run(n, 0).cpu().numpy()
    assert (rows["lds_resident"] == rows["streamed"]).all(), "the two weight sources differ"
    us = {k: [] for k in searches}
    for _ in range(ROUNDS):
        for name, n in searches.items():
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for i in range(CALLS):
                run(n, i)
            e1.record()
            e1.synchronize()
            us[name].append(e0.elapsed_time(e1) / CALLS * 1e3)
    return {"calls_per_window": CALLS, "us_per_call": {k: _summary(v) for k, v in us.items()}}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=DEFAULT_OUT, help="where the JSON result goes")
    args = ap.parse_args()
    dev = torch.device("cuda", 0)
    res = {"obs_dim": OBS, "hidden": list(HIDDEN), "num_actions": ACT, "warmup": WARMUP,
           "rounds": ROUNDS}
    env, spec, learner, model = _agent_parts(dev)
    res["acting"] = time_acting(env, spec, learner, model)
    res["device"] = time_device(dev, env, learner, model)
    for k, v in res["acting"]["ms_per_action"].items():
        print(f"select_action, {SIMULATIONS} simulations, {k} search: {v['median']:.3f} ms "
              f"(min {v['min']:.3f}, max {v['max']:.3f})")
    for k, v in res["device"]["us_per_call"].items():
        print(f"acme_mcts_search_run, {k}: {v['median']:.1f} us (min {v['min']:.1f}, "
              f"max {v['max']:.1f})")
    line = json.dumps(res)
    print(line)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as fh:
        fh.write(line + "\n")


if __name__ == "__main__":
    main()
