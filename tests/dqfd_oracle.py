"""Numpy oracle of the demonstration mix (acme_demo_mix, acme_amd/csrc/demos.hip) — test
infrastructure, no GPU.

- draw(): the per-row mapping of one Philox4x32-10 call (tests/_oracle.philox, the C
  restatement of the published generator) to (demonstration?, episode, first step);
- nstep_f32(): the n-step return in f32, one rounding per operation in the kernel's order;
- nstep_f64(): the reference's expression as written (agents/tf/dqfd/agent.py:183-206),
  evaluated in f64;
- mix(): a whole batch overlaid the way the kernel does it.
"""

import numpy as np

from tests import _oracle

DEMO_TAG = 0x44454D4F  # "DEMO"
DEMO_KEY = np.uint64(0xFFFFFFFFFFFFFFFE)


def u01_53(a, b):
    """detmath.h u01_53: a 53-bit uniform in [0, 1) from two 32-bit words (exact)."""
    return float((int(a) >> 5) * 67108864 + (int(b) >> 6)) * (1.0 / 9007199254740992.0)


def draw(seed, step, j, ratio, lengths):
    """(is_demo, episode, first) of row j of draw `step`.  Episode and first step are
    reported for replay rows too (the kernel does not compute them there)."""
    seed, step = int(seed) & (2 ** 64 - 1), int(step) & (2 ** 64 - 1)
    r = _oracle.philox([j, step & 0xFFFFFFFF, step >> 32, DEMO_TAG],
                       [seed & 0xFFFFFFFF, seed >> 32])
    is_demo = u01_53(r[0], r[1]) < ratio
    e = (int(r[2]) * len(lengths)) >> 32
    first = (int(r[3]) * (int(lengths[e]) - 2)) >> 32
    return is_demo, e, first


def span(first, n_step, length):
    """(last, m) of a transition that starts at `first` in an episode of `length` steps."""
    last = min(first + n_step, length - 1)
    return last, last - first


def nstep_f32(rewards, discounts, first, n_step, discount):
    """(r_t, d_t) as float32, every operation rounded once, in the kernel's order:
    g_0 = c_0 = 1; g_k = g_{k-1} * discount; c_k = c_{k-1} * d[first + k - 1];
    disc_k = c_k * g_k; r_t = sum over k = 0..m-1 (left to right) of
    rewards[first + 1 + k] * disc_k; d_t = disc_{m-1}."""
    f = np.float32
    rewards, discounts = np.asarray(rewards, f), np.asarray(discounts, f)
    _, m = span(first, n_step, len(rewards))
    gamma = f(discount)
    g = c = disc = f(1.0)
    acc = f(0.0)
    for k in range(m):
        if k > 0:
            g = f(g * gamma)
            c = f(c * discounts[first + k - 1])
        disc = f(c * g)
        acc = f(acc + f(rewards[first + 1 + k] * disc))
    return acc, disc


def nstep_f64(rewards, discounts, first, n_step, discount):
    """(r_t, d_t, sum of |terms|) of the reference's expression in f64:
    discounts = concat([1], cumprod(d[first:last-1])) * discount ** arange(last - first);
    r_t = sum(rewards[first+1:last+1] * discounts); d_t = discounts[-1]."""
    rewards = np.asarray(rewards, np.float64)
    d = np.asarray(discounts, np.float64)
    last, m = span(first, n_step, len(rewards))
    disc = np.concatenate([[1.0], np.cumprod(d[first:last - 1])]) * \
        np.float64(np.float32(discount)) ** np.arange(m)
    terms = rewards[first + 1:last + 1] * disc
    return terms.sum(), disc[-1], np.abs(terms).sum()


def mix(episodes, lengths, seed, step, ratio, n_step, discount, batch):
    """The overlay of one batch: (is_demo bool [B], per demonstration row a dict of first /
    last global step index, r_t, d_t).  episodes: list of (obs rows, action rows, rewards,
    discounts)."""
    offsets = np.concatenate([[0], np.cumsum(lengths)])
    is_demo = np.zeros(batch, bool)
    rows = {}
    for j in range(batch):
        demo, e, first = draw(seed, step, j, ratio, lengths)
        is_demo[j] = demo
        if not demo:
            continue
        _, _, rew, dis = episodes[e]
        last, _ = span(first, n_step, lengths[e])
        r_t, d_t = nstep_f32(rew, dis, first, n_step, discount)
        rows[j] = dict(episode=e, first=first, last=last, gfirst=int(offsets[e] + first),
                       glast=int(offsets[e] + last), r_t=r_t, d_t=d_t)
    return is_demo, rows
