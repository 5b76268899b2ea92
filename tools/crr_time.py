"""Step time of the CRR learner beside the DMPO learner: R = 256 transitions (B = 128 sequences
of T = 3), N_td = 1 and N_pw = 4 sampled actions per state for CRR (256 target-critic and
256 + 1,024 online-critic rows), N = 20 for DMPO (5,120 target-critic rows), 24 observations,
6 actions, full-size networks (policy 256x3, critic 512/512/256), 51 atoms on [-150, 150], the
native step on constant device batches (two alternating buffers, as the dataset iterator hands
them over) with the sampling noise generated on the device, device events around each timed
window.  The two learners are timed alternately in one process — ROUNDS rounds of STEPS steps
each after WARMUP steps of both — so drift of the box hits both alike.  Prints one line per
learner (median, min and max ms/step over the rounds), the sections of one eager CRR step (the
launch sequence: one launch per section, two for `d4pg_adam`) and a JSON line.

    python tools/crr_time.py [--out FILE] [--steps K] [--rounds R]      (needs the GPU)

Under a kernel tracer (one run, no counters), --rounds 1 --steps 50 keeps the trace short; the
kernels CRR adds are `crr_sample_kernel` and `crr_policy_loss_kernel`.
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
from acme_amd import _lib, specs  # noqa: E402
from acme_amd.native import NativeCRR, NativeDMPO  # noqa: E402
from acme_amd.networks import make_dmpo_networks  # noqa: E402

R, T, NTD, NPW, N, OBS, ACT = 256, 3, 1, 4, 20, 24, 6
ATOMS, VMIN, VMAX = 51, -150.0, 150.0
WARMUP = 20


def step_sections(n, batch):
    """(name, launches) of the profiler sections of one eager step."""
    L = _lib.lib()
    _lib.check(L.acme_profile_enable(1))
    try:
        _lib.check(L.acme_profile_reset())
        n.step(*batch)
        torch.cuda.synchronize()
        out = []
        for i in range(L.acme_profile_num_sections()):
            nm, ms, cnt = ctypes.c_char_p(), ctypes.c_double(), ctypes.c_int64()
            fl, by = ctypes.c_double(), ctypes.c_double()
            _lib.check(L.acme_profile_query(i, ctypes.byref(nm), ctypes.byref(ms),
                                            ctypes.byref(cnt), ctypes.byref(fl), ctypes.byref(by)))
            if cnt.value:
                out.append((nm.value.decode(), int(cnt.value)))
    finally:
        _lib.check(L.acme_profile_enable(0))
    return out


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
        b = (rng.standard_normal((R, OBS)), rng.uniform(-1, 1, (R, ACT)), rng.uniform(0, 5, R),
             np.full(R, 0.99), rng.standard_normal((R, OBS)))
        batches.append([torch.as_tensor(x.astype(np.float32)).to(dev).contiguous() for x in b])
    spec = specs.BoundedArray((ACT,), np.float32, -1.0, 1.0)
    nets = make_dmpo_networks(OBS, spec, vmin=VMIN, vmax=VMAX, num_atoms=ATOMS)
    learners = {
        "crr": NativeCRR(obs_dim=OBS, act_dim=ACT, max_batch=R, sequence_length=T,
                         num_action_samples_td_learning=NTD, num_action_samples_policy_weight=NPW,
                         num_atoms=ATOMS, vmin=VMIN, vmax=VMAX, device=dev),
        "dmpo": NativeDMPO(obs_dim=OBS, act_dim=ACT, max_batch=R, num_samples=N, num_atoms=ATOMS,
                           vmin=VMIN, vmax=VMAX, device=dev)}
    for n in learners.values():
        init = dict(nets["policy"].init(0))
        init.update(nets["critic"].init(1))
        n.set_params(init, init)

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
    res = {"rows": R, "sequence_length": T, "num_action_samples_td_learning": NTD,
           "num_action_samples_policy_weight": NPW, "dmpo_num_samples": N, "num_atoms": ATOMS,
           "warmup": WARMUP, "steps": args.steps, "rounds": args.rounds}
    for name, v in ms.items():
        res[name] = {"ms_per_step_median": statistics.median(v), "min": min(v), "max": max(v),
                     "rounds": v}
        print(f"{name}: {statistics.median(v):.4f} ms/step (min {min(v):.4f}, max {max(v):.4f} "
              f"over {args.rounds} rounds of {args.steps} steps)")
        assert np.isfinite(learners[name].critic_loss.item())
        assert np.isfinite(learners[name].policy_loss.item())
    # The launch sequence of a CRR step that copies no target.
    crr = learners["crr"]
    if crr.num_steps % crr.cfg.target_update_period == 0:
        crr.step(*batches[0])
    sections = step_sections(crr, batches[1])
    res["crr_sections"] = sections
    res["crr_launches"] = sum(c for _, c in sections) + sum(1 for s, _ in sections
                                                            if s == "d4pg_adam")
    print("crr step sections:", ", ".join(f"{s} x{c}" for s, c in sections))
    print(f"crr launches per step: {res['crr_launches']}")
    line = json.dumps(res)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
