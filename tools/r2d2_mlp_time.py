"""Times of the R2D2 step on R2D2MLPNetwork (obs 40, LSTM 20, MLP (50, 50), 5 actions: the
network of acme/agents/tf/r2d2/agent_test.py) beside the nearest network the layered R2D2 path
runs: R2D2AtariNetwork(torso="flat", obs_dim=40, lstm_size=24, head_size=56) on OAR inputs.
The two networks differ, so this is a record, not an equivalence.

  step      the three-launch step in its four variants, the target network on the online
            network's four waves or on four of its own ("w4" / "w8", the R2D2_MLP_WAVES tuning
            key at creation) and the weights streamed through L2 or staged in LDS ("l2" /
            "lds", R2D2_MLP_W), and the flat-torso step ("flat"), on constant device batches,
            device events around each timed window, the learners timed alternately in one
            process: ROUNDS rounds of STEPS steps after WARMUP steps of each, at (B, T, burn-in)
            = (10, 9, 2) (the reference test), (16, 20, 8) and (256, 20, 8).
  q_step    the one-row acting step of both networks, device time of CALLS back-to-back calls.
  sections  the profiled sections of one step of each learner (one per launch for the MLP
            network; the layered path puts several launches into some of its sections).

    python tools/r2d2_mlp_time.py [--out FILE]      (needs the GPU)
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
from acme_amd.native import NativeR2D2, NativeR2D2MLP  # noqa: E402
from acme_amd.networks import R2D2AtariNetwork, R2D2MLPNetwork  # noqa: E402

OBS, LSTM, HIDDEN, ACT = 40, 20, (50, 50), 5
FLAT_LSTM, FLAT_HEAD = 24, 56  # the layered path takes both sizes in multiples of 8
SHAPES = ((10, 9, 2), (16, 20, 8), (256, 20, 8))
VARIANTS = {"w8_lds": (8, 1), "w4_lds": (4, 1), "w8_l2": (8, 0), "w4_l2": (4, 0)}
DEFAULT_WAVES = 8  # csrc/r2d2_mlp.hip's default when the key is unset
WARMUP, STEPS, ROUNDS, CALLS = 20, 200, 5, 200


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


def make_mlp(dev, B, T, burn_in, waves=-1, weights_lds=-1):
    L = _lib.lib()
    if waves > 0:
        L.acme_tune_set(b"R2D2_MLP_WAVES", waves)  # both read at creation
    L.acme_tune_set(b"R2D2_MLP_W", weights_lds)
    try:
        n = NativeR2D2MLP(obs_dim=OBS, lstm_size=LSTM, hidden=HIDDEN, num_actions=ACT,
                          max_batch=B, max_sequence_length=T, burn_in_length=burn_in, device=dev)
    finally:
        L.acme_tune_set(b"R2D2_MLP_WAVES", DEFAULT_WAVES)
        L.acme_tune_set(b"R2D2_MLP_W", -1)
    net = R2D2MLPNetwork(OBS, LSTM, HIDDEN, ACT)
    n.set_params(net.init(0), net.init(1))
    return n


def make_flat(dev, B, T, burn_in):
    n = NativeR2D2(num_actions=ACT, max_batch=B, max_sequence_length=T, burn_in_length=burn_in,
                   torso="flat", obs_dim=OBS, lstm_size=FLAT_LSTM, head_size=FLAT_HEAD, device=dev)
    net = R2D2AtariNetwork(ACT, FLAT_LSTM, FLAT_HEAD, "flat", OBS)
    n.set_params(net.init(0), net.init(1))
    return n


def _batch(dev, B, T, H):
    rng = np.random.default_rng(0)
    f = lambda x, t=np.float32: torch.as_tensor(np.asarray(x, t)).to(dev).contiguous()  # noqa
    return dict(obs=f(rng.standard_normal((B, T, OBS))),
                action=f(rng.integers(0, ACT, (B, T)), np.int32),
                reward=f(rng.standard_normal((B, T))), discount=f(rng.random((B, T)) > 0.1),
                probs=f(rng.uniform(1e-4, 1e-2, B), np.float64),
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


def time_steps(dev, B, T, burn_in):
    b, bf = _batch(dev, B, T, LSTM), _batch(dev, B, T, FLAT_LSTM)
    mlp = {k: make_mlp(dev, B, T, burn_in, *v) for k, v in VARIANTS.items()}
    flat = make_flat(dev, B, T, burn_in)
    runs = {k: (lambda n=n: n.step(b["obs"], b["action"], b["reward"], b["discount"], b["probs"],
                                   b["h0"], b["c0"])) for k, n in mlp.items()}
    runs["flat"] = lambda: flat.step(bf["obs"], bf["action"], bf["reward"], bf["action"],
                                     bf["reward"], bf["discount"], bf["probs"], bf["h0"],
                                     bf["c0"])
    ms = _device_rounds(runs, STEPS)
    for n in list(mlp.values()) + [flat]:
        assert np.isfinite(n.loss.item())
    return ({k: _summary(v) for k, v in ms.items()},
            {"mlp": _sections(runs["w8_lds"]), "flat": _sections(runs["flat"])})


def time_q_step(dev):
    mlp, flat = make_mlp(dev, 1, 9, 2), make_flat(dev, 1, 9, 2)
    z = lambda *s: torch.zeros(*s, device=dev)  # noqa: E731
    obs, pa, pr = z(1, OBS), torch.zeros(1, dtype=torch.int32, device=dev), z(1)
    hm, cm, hf, cf = z(1, LSTM), z(1, LSTM), z(1, FLAT_LSTM), z(1, FLAT_LSTM)
    act = torch.zeros(1, dtype=torch.int32, device=dev)
    kw = dict(epsilon=0.01, seed=0, step=0)
    us = _device_rounds(
        {"mlp": lambda: mlp.q_step(obs, hm, cm, out=[None, act, hm, cm], **kw),
         "flat": lambda: flat.q_step(obs, pa, pr, hf, cf, out=[None, act, hf, cf], **kw)}, CALLS)
    return {k: _summary([1e3 * t for t in v]) for k, v in us.items()}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None, help="also write the JSON result here")
    args = ap.parse_args()
    dev = torch.device("cuda", 0)
    res = {"obs_dim": OBS, "lstm_size": LSTM, "hidden": list(HIDDEN), "num_actions": ACT,
           "flat": {"lstm_size": FLAT_LSTM, "head_size": FLAT_HEAD}, "warmup": WARMUP,
           "steps": STEPS, "rounds": ROUNDS, "calls": CALLS, "step_ms": {}, "sections": {}}
    for B, T, burn_in in SHAPES:
        key = f"B{B}_T{T}_burn{burn_in}"
        res["step_ms"][key], res["sections"][key] = time_steps(dev, B, T, burn_in)
    res["q_step_us"] = time_q_step(dev)
    for key, r in res["step_ms"].items():
        for k, v in r.items():
            print(f"step {key} {k}: {v['median']:.4f} ms (min {v['min']:.4f}, max {v['max']:.4f})")
    for k, v in res["q_step_us"].items():
        print(f"q_step, one row, {k}: {v['median']:.1f} us (min {v['min']:.1f}, max {v['max']:.1f})")
    for key, r in res["sections"].items():
        print(f"sections {key}:", {k: sum(v.values()) for k, v in r.items()}, r["mlp"])
    line = json.dumps(res)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as fh:
            fh.write(line + "\n")


if __name__ == "__main__":
    main()
