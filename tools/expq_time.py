"""Times of the exponentially Q-weighted acting call (acme_crr_act) at N = 16 on CRR's headline
networks: obs 24, act 6, policy (256, 256, 256), critic (512, 512, 256), 51 atoms.

  act       one-row `act`, the one-launch kernel and the layered path (forced on a second handle
            of the same networks with the EXPQ_ACT tuning key): host wall time (upload, launch,
            the action on the host) and device time (device events around ACTS back-to-back
            calls on a resident row), alternating in ROUNDS rounds.
  widths    the same device time on both paths with every layer w wide, w = 64, 128, 256: with
            the headline's 512 the measurement behind ACME_EXPQ_FUSED_MAX_WIDTH.
  rows      the same device time on both paths at rows = 1, 16, 256, on the headline networks
            and with every layer ACME_EXPQ_FUSED_MAX_WIDTH wide (the one-launch kernel is forced
            through the EXPQ_ACT key's value 2 whatever the limits say): the measurement behind
            ACME_EXPQ_FUSED_MAX_ROWS.

    python tools/expq_time.py [--out FILE]      (needs the GPU)
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
from acme_amd import _lib  # noqa: E402
from acme_amd.native import NativeCRR  # noqa: E402

OBS, ACT, ATOMS, N = 24, 6, 51, 16
POLICY, CRITIC = (256, 256, 256), (512, 512, 256)
WIDTHS, ROWS = (64, 128, 256), (1, 16, 256)
WARMUP, ROUNDS, ACTS = 20, 5, 1000


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
            out[name].append(1e3 * e0.elapsed_time(e1) / count)
    return out


def make(dev, policy, critic, key):
    """A CRR handle with random parameters; key: the EXPQ_ACT tuning value read at creation
    (0 the limits decide, 1 layered, 2 one launch at any row count)."""
    _lib.lib().acme_tune_set(b"EXPQ_ACT", key)
    try:
        n = NativeCRR(obs_dim=OBS, act_dim=ACT, max_batch=256, sequence_length=2,
                      policy_sizes=policy, critic_sizes=critic, num_atoms=ATOMS,
                      num_action_samples_policy_weight=16, device=dev)
    finally:
        _lib.lib().acme_tune_set(b"EXPQ_ACT", 0)
    rng = np.random.default_rng(0)
    with torch.no_grad():
        for name, t in n.views(n.params).items():
            v = (1.0 if name.endswith("/scale") else 0.0) + rng.standard_normal(tuple(t.shape)) * (
                0.1 if t.dim() == 1 else 1.0 / np.sqrt(t.shape[0]))
            t.copy_(torch.as_tensor(v.astype(np.float32)))
    return n


def time_act(dev, policy, critic, rows, host):
    x = np.random.default_rng(1).standard_normal((rows, OBS)).astype(np.float32)
    paths = {"fused": make(dev, policy, critic, 2), "layered": make(dev, policy, critic, 1)}
    xd = torch.from_numpy(x).to(dev)
    us = _device_rounds({k: (lambda s, n=n: n.act_packed(xd, N, 1.0, False, 1, s))
                         for k, n in paths.items()}, ACTS)
    res = {"device_us": {k: _summary(v) for k, v in us.items()}}
    a = {k: n.act(xd, N, 1.0, False, 1, 0, outputs=("index",)) for k, n in paths.items()}
    assert torch.equal(a["fused"]["index"], a["layered"]["index"])
    if host:
        wall = {k: [] for k in paths}
        for _ in range(ROUNDS):
            for name, n in paths.items():
                torch.cuda.synchronize(dev)
                t0 = time.perf_counter()
                for s in range(ACTS):
                    n.act_packed(torch.from_numpy(x).to(dev), N, 1.0, False, 1, s)[0].cpu().numpy()
                wall[name].append((time.perf_counter() - t0) / ACTS * 1e6)
        res["host_wall_us"] = {k: _summary(v) for k, v in wall.items()}
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None, help="also write the JSON result here")
    args = ap.parse_args()
    dev = torch.device("cuda", 0)
    res = {"obs_dim": OBS, "act_dim": ACT, "num_atoms": ATOMS, "num_samples": N,
           "policy": list(POLICY), "critic": list(CRITIC), "warmup": WARMUP, "rounds": ROUNDS,
           "acts": ACTS, "fused_max_width": _lib.EXPQ_FUSED_MAX_WIDTH,
           "fused_max_rows": _lib.EXPQ_FUSED_MAX_ROWS}
    res["act"] = time_act(dev, POLICY, CRITIC, 1, host=True)
    res["act_widths_device_us"] = {
        str(w): time_act(dev, (w,) * 3, (w,) * 3, 1, host=False)["device_us"] for w in WIDTHS}
    res["act_rows_device_us"] = {
        str(r): time_act(dev, POLICY, CRITIC, r, host=False)["device_us"] for r in ROWS}
    wl = (_lib.EXPQ_FUSED_MAX_WIDTH,) * 3
    res["act_rows_limit_width_device_us"] = {
        str(r): time_act(dev, wl, wl, r, host=False)["device_us"] for r in ROWS}
    for kind, r in res["act"].items():
        for k, v in r.items():
            print(f"act {kind} {k}: {v['median']:.1f} (min {v['min']:.1f}, max {v['max']:.1f})")
    for key, label in (("act_widths_device_us", "width"), ("act_rows_device_us", "rows"),
                       ("act_rows_limit_width_device_us", "limit width, rows")):
        for w, r in res[key].items():
            print(f"act device, {label} {w}: " +
                  ", ".join(f"{k} {v['median']:.1f} us" for k, v in r.items()))
    line = json.dumps(res)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as fh:
            fh.write(line + "\n")


if __name__ == "__main__":
    main()
