"""Step time of the DMPO learner beside the MPO learner: B = 256, N = 20 sampled actions per
state (5,120 target-critic rows), 24 observations, 6 actions, full-size networks (policy
256x3, critic 512/512/256), 51 atoms on [-150, 150] for DMPO, the native step on constant
device batches (two alternating buffers, as the dataset iterator hands them over) with the
sampling noise generated on the device, device events around each timed window.  The two
learners are timed alternately in one process — ROUNDS rounds of STEPS steps each after WARMUP
steps of both — so drift of the box hits both alike.  Prints one line per learner (median, min
and max ms/step over the rounds) and a JSON line.

    python tools/dmpo_time.py [--out FILE] [--steps K] [--rounds R]      (needs the GPU)

Under a kernel tracer (one run, no counters), --rounds 1 --steps 50 keeps the trace short; the
kernel DMPO adds is `dmpo_mix_loss_kernel`, and its N B-row head GEMM is the
`gemm_direct_kernel` launch over a two-problem DenseFwd set that follows the critic's last
hidden layer.
"""
import argparse
import json
import os
import statistics
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from acme_amd.native import NativeDMPO, NativeMPO  # noqa: E402
from acme_amd.networks import make_dmpo_networks, make_mpo_networks  # noqa: E402
from acme_amd import specs  # noqa: E402

B, N, OBS, ACT = 256, 20, 24, 6
ATOMS, VMIN, VMAX = 51, -150.0, 150.0
WARMUP = 20


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None, help="also write the JSON result here")
    ap.add_argument("--steps", type=int, default=200)
    ap.add_argument("--rounds", type=int, default=5)
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
    for name, make, nets in (
            ("dmpo", lambda: NativeDMPO(obs_dim=OBS, act_dim=ACT, max_batch=B, num_samples=N,
                                        num_atoms=ATOMS, vmin=VMIN, vmax=VMAX, device=dev),
             make_dmpo_networks(OBS, spec, vmin=VMIN, vmax=VMAX, num_atoms=ATOMS)),
            ("mpo", lambda: NativeMPO(obs_dim=OBS, act_dim=ACT, max_batch=B, num_samples=N,
                                      device=dev), make_mpo_networks(OBS, spec))):
        n = make()
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
    for _ in range(args.rounds):
        for name, n in learners.items():
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            run(n, args.steps)
            e1.record()
            e1.synchronize()
            ms[name].append(e0.elapsed_time(e1) / args.steps)
    res = {"batch": B, "num_samples": N, "num_atoms": ATOMS, "warmup": WARMUP,
           "steps": args.steps, "rounds": args.rounds}
    for name, v in ms.items():
        res[name] = {"ms_per_step_median": statistics.median(v), "min": min(v), "max": max(v),
                     "rounds": v}
        print(f"{name}: {statistics.median(v):.4f} ms/step (min {min(v):.4f}, max {max(v):.4f} "
              f"over {args.rounds} rounds of {args.steps} steps)")
        assert np.isfinite(learners[name].critic_loss.item())
        assert np.isfinite(learners[name].stats.cpu().numpy()).all()
    line = json.dumps(res)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
