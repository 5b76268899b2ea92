"""Times of the IMPALA step on IMPALAMLPNetwork (obs 10, MLP (50, 50), LSTM 20, 3 actions: the
network of examples/bsuite/run_impala.py) beside the nearest network the layered IMPALA path
runs: IMPALAAtariNetwork(torso="flat", obs_dim=10, lstm_size=24, head_size=52) on OAR inputs.
The two networks differ, so this is a record, not an equivalence.

  step      the three-launch step with the weights streamed through L2 ("mlp_l2") and staged in
            LDS ("mlp_lds", the IMPALA_MLP_W tuning key at creation) and the flat-torso step
            ("flat"), on constant device batches, device events around each timed window, the
            learners timed alternately in one process: ROUNDS rounds of STEPS steps after WARMUP
            steps of each, at (B, T) = (16, 3), (16, 20) and (256, 20).
  policy    the one-row policy step of both networks, device time of CALLS back-to-back calls.
  sections  the profiled sections of one step of each learner (one per launch for the MLP
            network; the layered path puts several launches into some of its sections).

    python tools/impala_mlp_time.py [--out FILE]      (needs the GPU)
"""
import argparse
import ctypes
import json
import os
import statistics
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from acme_amd import _lib  # noqa: E402
from acme_amd.native import NativeIMPALA, NativeIMPALAMLP  # noqa: E402
from acme_amd.networks import IMPALAAtariNetwork, IMPALAMLPNetwork  # noqa: E402

OBS, HIDDEN, LSTM, ACT = 10, (50, 50), 20, 3
FLAT_LSTM, FLAT_HEAD = 24, 52  # the layered path takes head sizes in multiples of 4
SHAPES = ((16, 3), (16, 20), (256, 20))
WARMUP, STEPS, ROUNDS, CALLS = 20, 200, 5, 200
COSTS = dict(discount=0.99, entropy_cost=0.01, baseline_cost=0.5)


def _summary(v):
    return {"median": statistics.median(v), "min": min(v), "max": max(v), "rounds": v}


def _device_rounds(runs, count):
    """Per-call device time of each run: device events around `count` back-to-back calls, the
    runs alternating in ROUNDS rounds after WARMUP calls of each."""
    for run in runs.values():
        for _ in range(WARMUP):
            run()
    torch.cuda.synchronize()
    out = {k: [] for k in runs}
    for _ in range(ROUNDS):
        for name, run in runs.items():
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(count):
                run()
            e1.record()
            e1.synchronize()
            out[name].append(e0.elapsed_time(e1) / count)
    return out


def make_mlp(dev, B, T, weights_lds):
    _lib.lib().acme_tune_set(b"IMPALA_MLP_W", 1 if weights_lds else 0)  # read at creation
    try:
        n = NativeIMPALAMLP(obs_dim=OBS, hidden=HIDDEN, lstm_size=LSTM, num_actions=ACT,
                            max_batch=B, max_sequence_length=T, device=dev, **COSTS)
    finally:
        _lib.lib().acme_tune_set(b"IMPALA_MLP_W", -1)
    n.set_params(IMPALAMLPNetwork(OBS, HIDDEN, LSTM, ACT).init(0))
    return n


def make_flat(dev, B, T):
    n = NativeIMPALA(num_actions=ACT, max_batch=B, max_sequence_length=T, torso="flat",
                     obs_dim=OBS, lstm_size=FLAT_LSTM, head_size=FLAT_HEAD, device=dev, **COSTS)
    n.set_params(IMPALAAtariNetwork(ACT, FLAT_LSTM, FLAT_HEAD, "flat", OBS).init(0))
    return n


def _batch(dev, B, T, H):
    rng = np.random.default_rng(0)
    f = lambda x, t=np.float32: torch.as_tensor(np.asarray(x, t)).to(dev).contiguous()  # noqa
    return dict(obs=f(rng.standard_normal((B, T, OBS))),
                action=f(rng.integers(0, ACT, (B, T)), np.int32),
                reward=f(rng.standard_normal((B, T))), discount=f(rng.random((B, T)) > 0.1),
                logits=f(rng.standard_normal((B, T, ACT))),
                h0=f(0.1 * rng.standard_normal((B, H))), c0=f(0.1 * rng.standard_normal((B, H))))


def _sections(step):
    _lib.set_profiling(True)
    L = _lib.lib()
    L.acme_profile_reset()
    step()
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


def time_steps(dev, B, T):
    b, bf = _batch(dev, B, T, LSTM), _batch(dev, B, T, FLAT_LSTM)
    mlp = {k: make_mlp(dev, B, T, k == "mlp_lds") for k in ("mlp_l2", "mlp_lds")}
    flat = make_flat(dev, B, T)
    runs = {k: (lambda n=n: n.step(b["obs"], b["action"], b["reward"], b["discount"],
                                   b["logits"], b["h0"], b["c0"])) for k, n in mlp.items()}
    runs["flat"] = lambda: flat.step(bf["obs"], bf["action"], bf["reward"], bf["action"],
                                     bf["reward"], bf["discount"], bf["logits"], bf["h0"],
                                     bf["c0"])
    ms = _device_rounds(runs, STEPS)
    for n in list(mlp.values()) + [flat]:
        assert np.isfinite(n.metrics.cpu().numpy()).all()
    return ({k: _summary(v) for k, v in ms.items()},
            {"mlp": _sections(runs["mlp_l2"]), "flat": _sections(runs["flat"])})


def time_policy(dev):
    mlp, flat = make_mlp(dev, 1, 2, False), make_flat(dev, 1, 2)
    z = lambda *s: torch.zeros(*s, device=dev)  # noqa: E731
    obs, pa, pr = z(1, OBS), torch.zeros(1, dtype=torch.int32, device=dev), z(1)
    hm, hf = z(1, LSTM), z(1, FLAT_LSTM)
    om, of = mlp._acting_outputs(1, torch.float32), flat._acting_outputs(1, torch.float32)  # noqa
    us = _device_rounds({"mlp": lambda: mlp.policy_step(obs, hm, hm, out=om),
                         "flat": lambda: flat.policy_step(obs, pa, pr, hf, hf, out=of)}, CALLS)
    return {k: _summary([1e3 * t for t in v]) for k, v in us.items()}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None, help="also write the JSON result here")
    args = ap.parse_args()
    dev = torch.device("cuda", 0)
    res = {"obs_dim": OBS, "hidden": list(HIDDEN), "lstm_size": LSTM, "num_actions": ACT,
           "flat": {"lstm_size": FLAT_LSTM, "head_size": FLAT_HEAD}, "warmup": WARMUP,
           "steps": STEPS, "rounds": ROUNDS, "calls": CALLS, "step_ms": {}, "sections": {}}
    for B, T in SHAPES:
        key = f"B{B}_T{T}"
        res["step_ms"][key], res["sections"][key] = time_steps(dev, B, T)
    res["policy_us"] = time_policy(dev)
    for key, r in res["step_ms"].items():
        for k, v in r.items():
            print(f"step {key} {k}: {v['median']:.4f} ms (min {v['min']:.4f}, max {v['max']:.4f})")
    for k, v in res["policy_us"].items():
        print(f"policy, one row, {k}: {v['median']:.1f} us (min {v['min']:.1f}, max {v['max']:.1f})")
    for key, r in res["sections"].items():
        print(f"sections {key}:", {k: sum(v.values()) for k, v in r.items()})
    line = json.dumps(res)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as fh:
            fh.write(line + "\n")


if __name__ == "__main__":
    main()
