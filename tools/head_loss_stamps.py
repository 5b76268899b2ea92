"""Phase stamps of the fused online head + loss + head dZ launch (kernels.hip
dqn_head_loss_dz_kernel, HEAD_STAMP; ACME_V_STAMPS=1): a B = 512 DQN learner runs a few steps,
then thread 0's stamps of every workgroup of the last step (s_memtime shader clocks, scaled by
the 100-MHz clock at entry and exit) are summarised: where one block's dependency chain goes.
Run on the GPU: python3 tools/head_loss_stamps.py"""
import os
import sys

import numpy as np

os.environ["ACME_V_STAMPS"] = "1"
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

PHASES = ("loads + partial dots (to barrier 1)", "reductions (to barrier 2)",
          "q rows (to barrier 3)", "loss row (to barrier 4)", "dZ planes + amax (to exit)")


def main():
    import torch
    from acme_amd.native import NativeDQN
    from acme_amd.networks import DQNAtariNetwork
    B = 512
    net = DQNAtariNetwork(18)
    d = NativeDQN(network="nature", num_actions=18, max_batch=B, obs_dtype="uint8")
    d.set_params(net.init(1), net.init(2))
    g = torch.Generator(device="cuda").manual_seed(0)
    o = torch.randint(0, 256, (B, 84, 84, 4), dtype=torch.uint8, device="cuda", generator=g)
    o2 = torch.randint(0, 256, (B, 84, 84, 4), dtype=torch.uint8, device="cuda", generator=g)
    a = torch.randint(0, 18, (B,), dtype=torch.int32, device="cuda", generator=g)
    r = torch.randn(B, device="cuda", generator=g)
    dd = torch.full((B,), 0.99, device="cuda")
    pr = torch.rand(B, dtype=torch.float64, device="cuda", generator=g) * 1e-3 + 1e-5
    for _ in range(5):
        d.step(o, a, r, dd, o2, pr)
    torch.cuda.synchronize()
    st = d.debug_buffer("gemm_stamps").view(np.int64).reshape(-1, 4096, 8)[5][:B].astype(np.float64)
    rt0, rt1, t = st[:, 0], st[:, 1], st[:, 2:8]
    mhz = np.median((t[:, 5] - t[:, 0]) / ((rt1 - rt0) * 10e-3))  # shader clocks per us
    print(f"head_loss_dz: {B} workgroups; s_memtime {mhz:.0f} ticks / us (median); launch span "
          f"{(rt1.max() - rt0.min()) * 0.01:.1f} us, entry spread {(rt0.max() - rt0.min()) * 0.01:.1f} "
          f"us, exit spread {(rt1.max() - rt1.min()) * 0.01:.1f} us")
    for i, ph in enumerate(PHASES):
        us = (t[:, i + 1] - t[:, i]) / mhz
        print(f"  {ph:38s} median {np.median(us):6.2f} us  min {us.min():6.2f}  max {us.max():6.2f}")
    us = (t[:, 5] - t[:, 0]) / mhz
    print(f"  {'total':38s} median {np.median(us):6.2f} us  min {us.min():6.2f}  max {us.max():6.2f}")


if __name__ == "__main__":
    main()
