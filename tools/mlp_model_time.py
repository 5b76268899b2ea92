"""Times of the MCTS agent's learned MLP model beside the AlphaZero learner on a same-size trunk:
observations 10 x 5 (Catch), hidden (50,), 3 actions, the reference example's sizes.

  step      the two-launch model step (NativeMLPModel.step on a resident ring and resident
            indices) and the native AZ step on constant device batches, at B = 16 and B = 256:
            device events around each timed window, the learners timed alternately in one
            process, ROUNDS rounds of STEPS steps after WARMUP steps of each.
  one_row   host wall time of one MLPModel.step(action) (one launch, the action by value, one
            packed copy back) beside one AZLearner.evaluate of one row (upload, launch, copy
            back), alternating in ROUNDS rounds of EVALS calls.
  acting    MCTSActor.select_action at 50 simulations on Catch, planning on the MLPModel and
            on the Simulator: wall time per action over ACTIONS actions, alternating per
            action.
  launches  the profiled launch sections of one model step and one prediction.

    python tools/mlp_model_time.py [--out FILE]      (needs the GPU)
"""
import argparse
import ctypes
import json
import os
import statistics
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from acme_amd import _lib, specs  # noqa: E402
from acme_amd.native import NativeAZ, NativeMLPModel  # noqa: E402
from acme_amd.networks import MLPTransitionModel, PolicyValueMLP  # noqa: E402

OBS, HIDDEN, ACT, RING = 50, (50,), 3, 1000
BATCHES = (16, 256)
WARMUP, STEPS, ROUNDS = 20, 200, 5
EVALS, ACTIONS = 200, 20
DEFAULT_OUT = os.path.join("profiles", "mlp_model", "mlp_model_time.json")


def _summary(v):
    return {"median": statistics.median(v), "min": min(v), "max": max(v), "rounds": v}


def _ring(dev):
    rng = np.random.default_rng(0)
    ring = rng.standard_normal((RING, 2 * OBS + 3)).astype(np.float32)
    ring[:, OBS] = rng.integers(0, ACT, RING)
    ring[:, OBS + 2] = rng.random(RING) < 0.9
    return torch.as_tensor(ring).to(dev)


def time_steps(dev):
    rng = np.random.default_rng(1)
    f = lambda x: torch.as_tensor(np.asarray(x, np.float32)).to(dev).contiguous()  # noqa: E731
    ring, runs = _ring(dev), {}
    for B in BATCHES:
        model = NativeMLPModel(obs_dim=OBS, hidden=HIDDEN, num_actions=ACT, max_batch=B, device=dev)
        model.set_params(MLPTransitionModel((OBS,), ACT, HIDDEN).init(0))
        az = NativeAZ(obs_dim=OBS, hidden=HIDDEN, num_actions=ACT, max_batch=B, device=dev)
        az.set_params(PolicyValueMLP(OBS, HIDDEN, ACT).init(0))
        idx = [torch.as_tensor(rng.integers(0, RING, B).astype(np.int32)).to(dev) for _ in range(2)]
        batches = [[f(rng.standard_normal((B, OBS))), f(rng.uniform(-1, 1, B)), f(np.ones(B)),
                    f(rng.standard_normal((B, OBS))), f(rng.dirichlet(np.ones(ACT), B))]
                   for _ in range(2)]
        runs[f"mlp_model_b{B}"] = lambda s, m=model, i=idx: m.step(ring, i[s % 2])
        runs[f"az_b{B}"] = lambda s, a=az, b=batches: a.step(*b[s % 2])
    for run in runs.values():
        for s in range(WARMUP):
            run(s)
    torch.cuda.synchronize(dev)
    ms = {k: [] for k in runs}
    for _ in range(ROUNDS):
        for name, run in runs.items():
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for s in range(STEPS):
                run(s)
            e1.record()
            e1.synchronize()
            ms[name].append(e0.elapsed_time(e1) / STEPS)
    return {k: _summary(v) for k, v in ms.items()}


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


def time_one_row(dev, env, learner, model):
    obs = env.reset().observation
    model.reset(obs)
    model.save_checkpoint()

    def step():  # as the search does it: back to the checkpoint (a slot switch), one step
        model.load_checkpoint()
        return model.step(1)

    calls = {"mlp_model_step": step, "az_evaluate": lambda: learner.evaluate(obs)}
    for c in calls.values():
        for _ in range(WARMUP):
            c()
    us = {k: [] for k in calls}
    for _ in range(ROUNDS):
        for name, c in calls.items():
            torch.cuda.synchronize(dev)
            t0 = time.perf_counter()
            for _ in range(EVALS):
                c()
            us[name].append((time.perf_counter() - t0) / EVALS * 1e6)
    return {k: _summary(v) for k, v in us.items()}


def time_acting(env, spec, learner, model):
    from acme_amd.agents.mcts import MCTSActor
    from acme_amd.agents.mcts.models import Simulator
    np.random.seed(0)
    models = {"mlp_model": model, "simulator": Simulator(env)}  # copied before the reset below
    actors = {k: MCTSActor(spec, m, learner, discount=1.0, num_simulations=50)
              for k, m in models.items()}
    ms = {k: [] for k in actors}
    ts = env.reset()
    model.reset(ts.observation)
    for a in actors.values():
        a.observe_first(ts)
    for i in range(ACTIONS + 3):
        for name, actor in actors.items():
            t0 = time.perf_counter()
            action = actor.select_action(ts.observation)
            if i >= 3:
                ms[name].append((time.perf_counter() - t0) * 1e3)
        ts = env.step(action)  # the last actor's action drives the environment
        for a in actors.values():
            a.observe(action, ts)
        if ts.last():
            ts = env.reset()
            for a in actors.values():
                a.observe_first(ts)
    return {"simulations": 50, "ms_per_action": {k: _summary(v) for k, v in ms.items()}}


def count_launches(dev):
    model = NativeMLPModel(obs_dim=OBS, hidden=HIDDEN, num_actions=ACT, max_batch=16, device=dev)
    ring = _ring(dev)
    idx = torch.arange(16, dtype=torch.int32, device=dev)
    _lib.set_profiling(True)
    L = _lib.lib()
    L.acme_profile_reset()
    model.step(ring, idx)
    model.predict_packed(ring[:1], 1)
    torch.cuda.synchronize()
    out = {}
    for i in range(L.acme_profile_num_sections()):
        name, ms, n = ctypes.c_char_p(), ctypes.c_double(), ctypes.c_int64()
        fl, by = ctypes.c_double(), ctypes.c_double()
        L.acme_profile_query(i, ctypes.byref(name), ctypes.byref(ms), ctypes.byref(n),
                             ctypes.byref(fl), ctypes.byref(by))
        if n.value:
            out[name.value.decode()] = int(n.value)
    _lib.set_profiling(False)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=DEFAULT_OUT, help="where the JSON result goes")
    args = ap.parse_args()
    dev = torch.device("cuda", 0)
    res = {"obs_dim": OBS, "hidden": list(HIDDEN), "num_actions": ACT, "warmup": WARMUP,
           "steps": STEPS, "rounds": ROUNDS, "evals": EVALS}
    res["step_ms"] = time_steps(dev)
    env, spec, learner, model = _agent_parts(dev)
    res["one_row_us"] = time_one_row(dev, env, learner, model)
    res["acting"] = time_acting(env, spec, learner, model)
    res["launches"] = count_launches(dev)
    for k, v in res["step_ms"].items():
        print(f"step {k}: {v['median']:.4f} ms (min {v['min']:.4f}, max {v['max']:.4f})")
    for k, v in res["one_row_us"].items():
        print(f"one row {k}: {v['median']:.1f} us (min {v['min']:.1f}, max {v['max']:.1f})")
    for k, v in res["acting"]["ms_per_action"].items():
        print(f"select_action, 50 simulations, {k}: {v['median']:.2f} ms (min {v['min']:.2f}, "
              f"max {v['max']:.2f})")
    print("launches:", res["launches"])
    line = json.dumps(res)
    print(line)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as fh:
        fh.write(line + "\n")


if __name__ == "__main__":
    main()
