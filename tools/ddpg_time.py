"""Step time of the DDPG learner beside the D4PG learner: B = 256, full-size networks
(policy 256x3, critic 512/512/256), the native step on constant device batches (two
alternating buffers, as the dataset iterator hands them over), device events around each
timed window.  The two learners are timed alternately in one process — ROUNDS rounds of
STEPS steps each after WARMUP steps of both — so drift of the box hits both alike.  Prints
one line per learner (median, min and max ms/step over the rounds) and a JSON line.

    python tools/ddpg_time.py [--out FILE]      (needs the GPU)
"""
import argparse
import json
import os
import statistics
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from acme_amd.native import NativeD4PG, NativeDDPG  # noqa: E402
from acme_amd.networks import make_d4pg_networks, make_ddpg_networks  # noqa: E402
from acme_amd import specs  # noqa: E402

B, OBS, ACT = 256, 24, 6
WARMUP, STEPS, ROUNDS = 20, 200, 5


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None, help="also write the JSON result here")
    args = ap.parse_args()
    dev = torch.device("cuda", 0)
    rng = np.random.default_rng(0)
    batches = []
    for _ in range(2):
        b = (rng.standard_normal((B, OBS)), rng.uniform(-1, 1, (B, ACT)), rng.uniform(0, 5, B),
             np.full(B, 0.99 ** 4), rng.standard_normal((B, OBS)))
        batches.append([torch.as_tensor(x.astype(np.float32)).to(dev).contiguous() for x in b])
    spec = specs.BoundedArray((ACT,), np.float32, -1.0, 1.0)
    learners = {}
    for name, cls, nets in (("ddpg", NativeDDPG, make_ddpg_networks(OBS, spec)),
                            ("d4pg", NativeD4PG, make_d4pg_networks(OBS, spec))):
        n = cls(obs_dim=OBS, act_dim=ACT, max_batch=B, device=dev)
        init = dict(nets["policy"].init(0))
        init.update(nets["critic"].init(1))
        n.set_params(init, init)
        learners[name] = n

    def run(n, steps):
        for s in range(steps):
            n.step(*batches[s % 2])

    for n in learners.values():
        run(n, WARMUP)
    torch.cuda.synchronize(dev)
    ms = {k: [] for k in learners}
    for _ in range(ROUNDS):
        for name, n in learners.items():
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            run(n, STEPS)
            e1.record()
            e1.synchronize()
            ms[name].append(e0.elapsed_time(e1) / STEPS)
    res = {"batch": B, "warmup": WARMUP, "steps": STEPS, "rounds": ROUNDS}
    for name, v in ms.items():
        res[name] = {"ms_per_step_median": statistics.median(v), "min": min(v), "max": max(v),
                     "rounds": v}
        print(f"{name}: {statistics.median(v):.4f} ms/step (min {min(v):.4f}, max {max(v):.4f} "
              f"over {ROUNDS} rounds of {STEPS} steps)")
        assert np.isfinite(learners[name].critic_loss.item())
    line = json.dumps(res)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
