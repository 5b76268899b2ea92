"""Times of the AlphaZero learner and of the MCTS acting path beside the DQN MLP learner on the
same trunk: B = 256, obs 10, hidden (256, 256), 18 actions.

  step      the native AZ step and NativeDQN's MLP step on constant device batches (two
            alternating buffers), device events around each timed window, the two learners timed
            alternately in one process: ROUNDS rounds of STEPS steps after WARMUP steps of both.
  evaluate  host wall time of one `evaluate` of one row (upload, launch, results on the host):
            the fused kernel with its packed output (one copy back) and with probs and value
            copied back separately, the layered path on a trunk one column past the fused limit,
            and NativeDQN.q_values of one row, alternating in ROUNDS rounds of EVALS calls;
            and the device time of the fused and the layered path on a resident row (device
            events around EVALS back-to-back calls).
  acting    MCTSActor.select_action at 50 simulations on Catch (10 x 5) with the learner's
            evaluation: wall time per action over ACTIONS actions.
  launches  the profiled launch sections of one AZ step.

    python tools/az_time.py [--out FILE]      (needs the GPU)
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
from acme_amd import _lib, specs  # noqa: E402
from acme_amd.native import NativeAZ, NativeDQN  # noqa: E402
from acme_amd.networks import MLP, PolicyValueMLP  # noqa: E402

B, OBS, HIDDEN, ACT = 256, 10, (256, 256), 18
WARMUP, STEPS, ROUNDS = 20, 200, 5
EVALS, ACTIONS = 200, 20


def _summary(v):
    return {"median": statistics.median(v), "min": min(v), "max": max(v), "rounds": v}


def time_steps(dev, az, dqn):
    rng = np.random.default_rng(0)
    f = lambda x: torch.as_tensor(np.asarray(x, np.float32)).to(dev).contiguous()  # noqa: E731
    az_batches, dqn_batches = [], []
    for _ in range(2):
        o, o2 = rng.standard_normal((B, OBS)), rng.standard_normal((B, OBS))
        r, d = rng.uniform(-1, 1, B), np.full(B, 0.99)
        az_batches.append([f(o), f(r), f(d), f(o2), f(rng.dirichlet(np.ones(ACT), B))])
        a = torch.as_tensor(rng.integers(0, ACT, B).astype(np.int32)).to(dev)
        p = torch.full((B,), 1e-3, dtype=torch.float64, device=dev)
        dqn_batches.append([f(o), a, f(r), f(d), f(o2), p])
    runs = {"az": lambda s: az.step(*az_batches[s % 2]),
            "dqn_mlp": lambda s: dqn.step(*dqn_batches[s % 2])}
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
    assert np.isfinite(az.loss.item()) and np.isfinite(dqn.loss.item())
    return {k: _summary(v) for k, v in ms.items()}


def time_evaluate(dev, az, az_wide, dqn):
    x = np.random.default_rng(1).standard_normal((1, OBS)).astype(np.float32)
    up = lambda: torch.from_numpy(x).to(dev)  # noqa: E731

    def packed():
        return az.evaluate_packed(up()).cpu().numpy()

    def separate():
        probs, value = az.evaluate(up())
        return probs.cpu().numpy(), value.cpu().numpy()

    def layered():
        return az_wide.evaluate_packed(up()).cpu().numpy()

    def q_values():
        return dqn.q_values(up()).cpu().numpy()

    calls = {"az_fused_packed": packed, "az_fused_two_copies": separate,
             "az_layered_packed": layered, "dqn_q_values": q_values}
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


def time_evaluate_device(dev, az, az_wide):
    """Device time of one evaluate launch sequence on a resident row: device events around EVALS
    back-to-back calls, the fused and the layered path alternating."""
    x = torch.from_numpy(np.random.default_rng(1).standard_normal((1, OBS)).astype(np.float32)).to(dev)
    calls = {"az_fused": lambda: az.evaluate_packed(x), "az_layered": lambda: az_wide.evaluate_packed(x)}
    for c in calls.values():
        for _ in range(WARMUP):
            c()
    torch.cuda.synchronize(dev)
    us = {k: [] for k in calls}
    for _ in range(ROUNDS):
        for name, c in calls.items():
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(EVALS):
                c()
            e1.record()
            e1.synchronize()
            us[name].append(e0.elapsed_time(e1) / EVALS * 1e3)
    return {k: _summary(v) for k, v in us.items()}


def time_acting(dev):
    from acme_amd.agents.mcts import AZLearner, MCTSActor
    from acme_amd.agents.mcts.models import Simulator
    from acme_amd.environments.catch import Catch
    from acme_amd.optimizers import Adam
    from acme_amd.utils import loggers
    env = Catch(rows=10, columns=5, seed=0)
    learner = AZLearner(PolicyValueMLP(50, HIDDEN, 3), Adam(1e-3), iter(()), discount=1.0,
                        batch_size=16, logger=loggers.NoOpLogger(), device=dev)
    actor = MCTSActor(specs.make_environment_spec(env), Simulator(env), learner, discount=1.0,
                      num_simulations=50)
    np.random.seed(0)
    ms, ts = [], env.reset()
    actor.observe_first(ts)
    for i in range(ACTIONS + 3):
        t0 = time.perf_counter()
        action = actor.select_action(ts.observation)
        if i >= 3:
            ms.append((time.perf_counter() - t0) * 1e3)
        ts = env.step(action)
        actor.observe(action, ts)
        if ts.last():
            ts = env.reset()
            actor.observe_first(ts)
    return {"simulations": 50, "ms_per_action": _summary(ms)}


def count_launches(az, batch):
    _lib.set_profiling(True)
    L = _lib.lib()
    L.acme_profile_reset()
    az.step(*batch)
    torch.cuda.synchronize()
    import ctypes
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
    ap.add_argument("--out", default=None, help="also write the JSON result here")
    args = ap.parse_args()
    dev = torch.device("cuda", 0)
    az = NativeAZ(obs_dim=OBS, hidden=HIDDEN, num_actions=ACT, max_batch=B, max_eval_rows=1,
                  discount=0.99, device=dev)
    az.set_params(PolicyValueMLP(OBS, HIDDEN, ACT).init(0))
    wide = (HIDDEN[0] + 1, HIDDEN[1])
    az_wide = NativeAZ(obs_dim=OBS, hidden=wide, num_actions=ACT, max_batch=1, max_eval_rows=1,
                       device=dev)
    az_wide.set_params(PolicyValueMLP(OBS, wide, ACT).init(0))
    dqn = NativeDQN(network="mlp", num_actions=ACT, max_batch=B, obs_dtype="float32",
                    obs_dim=OBS, hidden=HIDDEN, device=dev)
    init = MLP(OBS, HIDDEN, ACT).init(0)
    dqn.set_params(init, init)
    res = {"batch": B, "obs_dim": OBS, "hidden": list(HIDDEN), "num_actions": ACT,
           "warmup": WARMUP, "steps": STEPS, "rounds": ROUNDS, "evals": EVALS}
    res["step_ms"] = time_steps(dev, az, dqn)
    res["evaluate_us"] = time_evaluate(dev, az, az_wide, dqn)
    res["evaluate_device_us"] = time_evaluate_device(dev, az, az_wide)
    res["acting"] = time_acting(dev)
    rng = np.random.default_rng(2)
    f = lambda x: torch.as_tensor(np.asarray(x, np.float32)).to(dev).contiguous()  # noqa: E731
    res["step_launches"] = count_launches(az, [
        f(rng.standard_normal((B, OBS))), f(rng.uniform(-1, 1, B)), f(np.ones(B)),
        f(rng.standard_normal((B, OBS))), f(rng.dirichlet(np.ones(ACT), B))])
    for k, v in res["step_ms"].items():
        print(f"step {k}: {v['median']:.4f} ms (min {v['min']:.4f}, max {v['max']:.4f})")
    for k, v in res["evaluate_us"].items():
        print(f"evaluate {k}: {v['median']:.1f} us (min {v['min']:.1f}, max {v['max']:.1f})")
    for k, v in res["evaluate_device_us"].items():
        print(f"evaluate, device {k}: {v['median']:.1f} us (min {v['min']:.1f}, max {v['max']:.1f})")
    a = res["acting"]["ms_per_action"]
    print(f"select_action, 50 simulations: {a['median']:.2f} ms (min {a['min']:.2f}, "
          f"max {a['max']:.2f})")
    print("step launches:", res["step_launches"], "total", sum(res["step_launches"].values()))
    line = json.dumps(res)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as fh:
            fh.write(line + "\n")


if __name__ == "__main__":
    main()
