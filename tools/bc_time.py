"""Times of the BC learner and of its acting call: obs 10, hidden (64, 64), 3 actions, the
reference example's network.

  step      the native BC step beside the AZ step on the same trunk, constant device batches (two
            alternating buffers), device events around each timed window, the two learners timed
            alternately in one process: ROUNDS rounds of STEPS steps after WARMUP steps of both,
            at B = 16 and B = 256.
  act       one-row `act`, the one-launch kernel and the layered path (forced on a second handle
            of the same network with the BC_ACT tuning key): host wall time (upload, launch,
            actions on the host) and device time (device events around ACTS back-to-back calls
            on a resident row), alternating in ROUNDS rounds.
  widths    the same device time on both paths at hidden (w, w) for w = 32, 64, 128, 256: the
            measurement behind ACME_BC_FUSED_MAX_WIDTH.
  launches  the profiled launch sections of one BC step.

    python tools/bc_time.py [--out FILE]      (needs the GPU)
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
from acme_amd import _lib  # noqa: E402
from acme_amd.native import NativeAZ, NativeBC  # noqa: E402
from acme_amd.networks import MLP, PolicyValueMLP  # noqa: E402

OBS, HIDDEN, ACT = 10, (64, 64), 3
BATCHES, WIDTHS = (16, 256), (32, 64, 128, 256)
WARMUP, STEPS, ROUNDS, ACTS = 20, 200, 5, 200


def _summary(v):
    return {"median": statistics.median(v), "min": min(v), "max": max(v), "rounds": v}


def _device_rounds(runs, count):
    """Per-call device time of each run: device events around `count` back-to-back calls, the
    runs alternating in ROUNDS rounds after WARMUP calls of each."""
    for run in runs.values():
        for s in range(WARMUP):
            run(s)
    torch.cuda.synchronize()
    out = {k: [] for k in runs}
    for _ in range(ROUNDS):
        for name, run in runs.items():
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for s in range(count):
                run(s)
            e1.record()
            e1.synchronize()
            out[name].append(e0.elapsed_time(e1) / count)
    return out


def make_bc(dev, hidden, batch, layered=False):
    _lib.lib().acme_tune_set(b"BC_ACT", 1 if layered else 0)  # read at creation
    try:
        bc = NativeBC(obs_dim=OBS, hidden=hidden, num_actions=ACT, max_batch=batch, device=dev)
    finally:
        _lib.lib().acme_tune_set(b"BC_ACT", 0)
    bc.set_params(MLP(OBS, hidden, ACT).init(0))
    return bc


def time_steps(dev, B):
    bc = make_bc(dev, HIDDEN, B)
    az = NativeAZ(obs_dim=OBS, hidden=HIDDEN, num_actions=ACT, max_batch=B, discount=0.99,
                  device=dev)
    az.set_params(PolicyValueMLP(OBS, HIDDEN, ACT).init(0))
    rng = np.random.default_rng(0)
    f = lambda x: torch.as_tensor(np.asarray(x, np.float32)).to(dev).contiguous()  # noqa: E731
    bc_b, az_b = [], []
    for _ in range(2):
        o, o2 = rng.standard_normal((B, OBS)), rng.standard_normal((B, OBS))
        a = torch.as_tensor(rng.integers(0, ACT, B).astype(np.int32)).to(dev)
        bc_b.append([f(o), a])
        az_b.append([f(o), f(rng.uniform(-1, 1, B)), f(np.full(B, 0.99)), f(o2),
                     f(rng.dirichlet(np.ones(ACT), B))])
    ms = _device_rounds({"bc": lambda s: bc.step(*bc_b[s % 2]),
                         "az": lambda s: az.step(*az_b[s % 2])}, STEPS)
    assert np.isfinite(bc.loss.item()) and np.isfinite(bc.gradient_norm.item())
    return {k: _summary(v) for k, v in ms.items()}, count_launches(bc, bc_b[0])


def time_act(dev, hidden, host):
    x = np.random.default_rng(1).standard_normal((1, OBS)).astype(np.float32)
    paths = {"fused": make_bc(dev, hidden, 1), "layered": make_bc(dev, hidden, 1, layered=True)}
    res = {}
    xd = torch.from_numpy(x).to(dev)
    us = _device_rounds({k: (lambda s, n=n: n.act_packed(xd, 0.05, 1, s, with_logits=False))
                         for k, n in paths.items()}, ACTS)
    res["device_us"] = {k: _summary([1e3 * t for t in v]) for k, v in us.items()}
    if host:
        wall = {k: [] for k in paths}
        for _ in range(ROUNDS):
            for name, n in paths.items():
                torch.cuda.synchronize(dev)
                t0 = time.perf_counter()
                for s in range(ACTS):
                    n.act_packed(torch.from_numpy(x).to(dev), 0.05, 1, s,
                                 with_logits=False).cpu().numpy()
                wall[name].append((time.perf_counter() - t0) / ACTS * 1e6)
        res["host_wall_us"] = {k: _summary(v) for k, v in wall.items()}
    return res


def count_launches(bc, batch):
    _lib.set_profiling(True)
    L = _lib.lib()
    L.acme_profile_reset()
    bc.step(*batch)
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
    ap.add_argument("--out", default=None, help="also write the JSON result here")
    args = ap.parse_args()
    dev = torch.device("cuda", 0)
    res = {"obs_dim": OBS, "hidden": list(HIDDEN), "num_actions": ACT, "warmup": WARMUP,
           "steps": STEPS, "rounds": ROUNDS, "acts": ACTS,
           "fused_max_width": _lib.BC_FUSED_MAX_WIDTH, "step_ms": {}}
    for B in BATCHES:
        res["step_ms"][str(B)], res["step_launches"] = time_steps(dev, B)
    res["act"] = time_act(dev, HIDDEN, host=True)
    res["act_widths_device_us"] = {str(w): time_act(dev, (w, w), host=False)["device_us"]
                                   for w in WIDTHS}
    for B, r in res["step_ms"].items():
        for k, v in r.items():
            print(f"step B={B} {k}: {v['median']:.4f} ms (min {v['min']:.4f}, max {v['max']:.4f})")
    for kind, r in res["act"].items():
        for k, v in r.items():
            print(f"act {kind} {k}: {v['median']:.1f} (min {v['min']:.1f}, max {v['max']:.1f})")
    for w, r in res["act_widths_device_us"].items():
        print(f"act device, width {w}: " + ", ".join(f"{k} {v['median']:.1f} us" for k, v in r.items()))
    print("step launches:", res["step_launches"], "total", sum(res["step_launches"].values()))
    line = json.dumps(res)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as fh:
            fh.write(line + "\n")


if __name__ == "__main__":
    main()
