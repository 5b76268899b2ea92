"""The native behavioural-cloning step and acting call (acme_bc_*) against plain torch float64 on
the CPU: F.cross_entropy through autograd, and the snt.Adam formula.

Bars (those of tests/test_az_gpu.py):
  loss, gradient_norm, logits: rtol 1e-5 + 2e-6 x the tensor's largest magnitude
  gradients, per tensor: |g - g_ref| <= 1e-4 |g_ref| + 2e-5 max|g_ref|
  Adam applied to the kernel's own gradients: rtol 1e-6 (+ 1e-9 = 1e-6 lr, the rounding of the
      update's term, which p - update can cancel against: the project's Adam bar), against the
      formula in float32, as snt.Adam runs it: its 1 - beta^t is a float32 value, 3e-5 away from
      the float64 one at t = 2, and that difference is the optimizer's definition, not an error
  free-running parameters: all within 2 lr and 99% within 1e-5 relative.
"""

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from acme_amd import _lib
from acme_amd.networks import MLP

pytestmark = pytest.mark.gpu

LR, B1, B2, EPS = 1e-3, 0.9, 0.999, 1e-8

# (B, D, hidden, A): the loss exactly 0; the smallest hidden network; a second block and the
# ticket; the reference example; one full pass over the actions; a second pass of one lane; the
# limit on A.  The last element seeds the parameters and the batches: chosen on the CPU so that
# no float64 pre-activation of the six steps lies within 2e-6 x its layer's scale of 0.
SHAPES = [(1, 3, (), 1, 1), (2, 3, (5,), 3, 1), (5, 8, (50, 50), 5, 1), (16, 10, (64, 64), 3, 2),
          (33, 10, (36, 68), 64, 1), (33, 7, (36, 68), 65, 1), (9, 10, (64, 64), 1024, 1)]


def _native(D, hidden, A, B, rows=1):
    from acme_amd.native import NativeBC
    return NativeBC(obs_dim=D, hidden=hidden, num_actions=A, max_batch=B, max_act_rows=rows,
                    learning_rate=LR, adam_beta1=B1, adam_beta2=B2, adam_epsilon=EPS)


def _params(D, hidden, A, seed):
    rng = np.random.default_rng(seed)
    return {name: (0.1 * rng.standard_normal(shape) if name.endswith("/b") else
                   rng.standard_normal(shape) / np.sqrt(shape[0])).astype(np.float32)
            for name, shape in MLP(D, hidden, A).tensor_shapes()}


def _batch(B, D, A, seed):
    rng = np.random.default_rng(seed)
    return (rng.standard_normal((B, D)).astype(np.float32), rng.integers(0, A, B).astype(np.int32))


def _dev(obs, act):
    return torch.as_tensor(obs).cuda().contiguous(), torch.as_tensor(act).cuda().contiguous()


def _forward(p, obs):
    """(logits, hidden pre-activations) in float64."""
    x, pre = torch.as_tensor(np.asarray(obs, np.float64)), []
    nl = len(p) // 2 - 1
    for i in range(nl + 1):
        x = x @ p[f"mlp/linear_{i}/w"] + p[f"mlp/linear_{i}/b"]
        if i < nl:
            pre.append(x)
            x = torch.relu(x)
    return x, pre


def _adam(p, g, m, v, t, f=np.float64):
    """snt.optimizers.Adam in dtype f."""
    p, g, m, v = (np.asarray(x, f) for x in (p, g, m, v))
    b1, b2, lr, eps, one = f(B1), f(B2), f(LR), f(EPS), f(1)
    m = b1 * m + (one - b1) * g
    v = b2 * v + (one - b2) * (g * g)
    bc1, bc2 = one - np.power(b1, f(t)), one - np.power(b2, f(t))
    return p - (lr * (m / bc1)) / (np.sqrt(v / bc2) + eps), m, v


def _ref_step(state, obs, act, margin=True):
    """One float64 step from state = {params, m, v, num_steps}: out, grads, new state.  A row
    whose action is outside [0, A) is zeroed; the mean divides by B.  margin: assert that the
    seeds keep every hidden pre-activation clear of 0 (not at 4096 rows, where some lie there
    whatever the seed and one row's ReLU decision is far below the gradient bars)."""
    p = {k: torch.tensor(v, dtype=torch.float64, requires_grad=True)
         for k, v in state["params"].items()}
    logits, pre = _forward(p, obs)
    for z in pre if margin else ():  # no ReLU decision within float32 rounding of 0
        assert float(z.detach().abs().min()) > 2e-6 * float(z.detach().abs().max())
    a = torch.as_tensor(np.asarray(act, np.int64))
    ok = (a >= 0) & (a < logits.shape[1])
    per = F.cross_entropy(logits, a.clamp(0, logits.shape[1] - 1), reduction="none")
    loss = (per * ok).sum() / len(a)
    loss.backward()
    grads = {k: v.grad.numpy() for k, v in p.items()}
    norm = np.sqrt(sum(float((g * g).sum()) for g in grads.values()))
    t = state["num_steps"] + 1
    new = dict(params={}, m={}, v={}, num_steps=t)
    for k in grads:
        new["params"][k], new["m"][k], new["v"][k] = _adam(
            state["params"][k], grads[k], state["m"][k], state["v"][k], t)
    out = dict(loss=float(loss.detach()), gradient_norm=norm, logits=logits.detach().numpy())
    return out, grads, new


def _close(got, ref, name):
    ref = np.asarray(ref, np.float64)
    got = np.asarray(got, np.float64).reshape(ref.shape)
    scale = float(np.abs(ref).max()) if ref.size else 0.0
    print(f"{name}: max |err| {float(np.abs(got - ref).max()):.3e}, scale {scale:.3e}")
    np.testing.assert_allclose(got, ref, rtol=1e-5, atol=2e-6 * scale, err_msg=name)


def _check_params(got, ref):
    for k, r in ref.items():
        err = np.abs(got[k].reshape(r.shape).astype(np.float64) - r)
        assert err.max() <= 2 * LR + 1e-6, (k, float(err.max()))
        assert np.mean(err <= 1e-5 * np.abs(r) + 1e-7) >= 0.99, k


def _state_of(n):
    f = lambda w: {k: v.astype(np.float64) for k, v in n.get_params(w).items()}  # noqa: E731
    return dict(params=f("params"), m=f("m"), v=f("v"), num_steps=n.num_steps)


def _check_step(n, obs, act, tag="", margin=True):
    """One native step from the state the learner holds against the reference."""
    state = _state_of(n)
    n.step(*_dev(obs, act))
    torch.cuda.synchronize()
    out, grads, new = _ref_step(state, obs, act, margin)
    loss, norm = n.loss.item(), n.gradient_norm.item()
    assert np.isfinite(loss) and np.isfinite(norm)
    _close(loss, out["loss"], f"loss{tag}")
    _close(norm, out["gradient_norm"], f"gradient_norm{tag}")
    _close(n.debug_buffer("logits"), out["logits"], f"logits{tag}")
    got_g, got_p = n.get_params("grads"), n.get_params("params")
    for k, ref in grads.items():
        err = np.abs(got_g[k].astype(np.float64) - ref)
        assert (err <= 1e-4 * np.abs(ref) + 2e-5 * np.abs(ref).max() + 1e-30).all(), (k, tag)
        want = _adam(state["params"][k], got_g[k], state["m"][k], state["v"][k],
                     new["num_steps"], np.float32)[0]
        np.testing.assert_allclose(got_p[k], want, rtol=1e-6, atol=1e-9, err_msg=k + tag)
    _check_params(got_p, new["params"])
    return out, got_g


@pytest.mark.parametrize("B,D,hidden,A,seed", SHAPES)
def test_step_matches_f64(B, D, hidden, A, seed):
    n = _native(D, hidden, A, B)
    n.set_params(_params(D, hidden, A, seed))
    assert [(name, shape) for name, _, shape in n.tensors] == MLP(D, hidden, A).tensor_shapes()
    for s in range(3):  # teacher-forced: the reference continues from the kernel's state
        out, g = _check_step(n, *_batch(B, D, A, 100 * seed + 10 + s), tag=f" t={s + 1}")
        if A == 1:
            assert n.loss.item() == 0.0 and all((v == 0).all() for v in g.values())
    state = _state_of(n)
    for s in range(3):  # free-running: both continue from their own state
        obs, act = _batch(B, D, A, 100 * seed + 20 + s)
        n.step(*_dev(obs, act))
        _, _, state = _ref_step(state, obs, act)
    assert n.num_steps == 6
    _check_params(n.get_params("params"), state["params"])


@pytest.mark.parametrize("case", ["big_on_argmax", "big_off_argmax", "bad_actions", "one_action"])
def test_inputs_that_can_go_wrong(case):
    B, D, hidden, A = 9, 10, (50, 50), 5
    p = _params(D, hidden, A, 2)
    obs, act = _batch(B, D, A, 3)
    if case.startswith("big"):  # logits reach +-50
        p["mlp/linear_2/b"][:] = 0
        lg = _forward({k: torch.tensor(v, dtype=torch.float64) for k, v in p.items()}, obs)[0]
        p["mlp/linear_2/w"] *= np.float32(50.0 / float(lg.abs().max()))
        lg = _forward({k: torch.tensor(v, dtype=torch.float64) for k, v in p.items()}, obs)[0]
        assert float(lg.abs().max()) >= 49.0
        top = lg.argmax(dim=1).numpy().astype(np.int32)
        act = top if case == "big_on_argmax" else (top + 1) % A
    elif case == "bad_actions":
        act[2], act[6] = -1, A
    else:
        act[:] = 3
    n = _native(D, hidden, A, B)
    n.set_params(p)
    _check_step(n, obs, act, tag=f" {case}")
    if case == "bad_actions":
        dl, dh = n.debug_buffer("dlogits").reshape(B, A), n.debug_buffer("dh").reshape(B, -1)
        assert (dl[[2, 6]] == 0).all() and (dh[[2, 6]] == 0).all() and (dl[0] != 0).any()


def test_smaller_batches_repeat_and_resume_bit_for_bit():
    from acme_amd.agents.bc import BCLearner
    from acme_amd.replay import ReplaySample, SampleInfo
    from acme_amd.utils import loggers
    D, hidden, A = 10, (50, 50), 5
    n = _native(D, hidden, A, 8)
    n.set_params(_params(D, hidden, A, 4))
    for i, B in enumerate((3, 8)):
        _check_step(n, *_batch(B, D, A, 30 + i), tag=f" B={B}")
    with pytest.raises(ValueError, match="batch must be in"):
        n.step(*_dev(*_batch(9, D, A, 0)))
    batches = [_dev(*_batch(8, D, A, 40 + i)) for i in range(4)]

    def learner(order):
        data = (ReplaySample(info=SampleInfo(None, None, None, None),
                             data=batches[i] + (None, None, None)) for i in order)
        return BCLearner(MLP(D, hidden, A), LR, data, batch_size=8, seed=3,
                         logger=loggers.NoOpLogger())

    def bits(x):
        return [t.cpu().numpy().view(np.uint32) for t in (x.native.params, x.native._scalars)]

    a, b = learner([0, 1, 2, 3]), learner([0, 1, 2])
    for x in (a, b):
        for _ in range(3):
            x.step()
    for u, v in zip(bits(a), bits(b)):  # three steps, run twice
        np.testing.assert_array_equal(u, v)
    c = learner([0, 1, 2, 3])
    c.step(), c.step()
    saved = c.save()
    c.step(), c.step()
    d = learner([2, 3])
    d.restore(saved)
    d.step(), d.step()
    assert c.num_steps == d.num_steps == 4
    for w in ("params", "m", "v"):
        x, y = c.native.get_params(w), d.native.get_params(w)
        for k in x:
            np.testing.assert_array_equal(x[k].view(np.uint32), y[k].view(np.uint32), err_msg=k)


# The fused kernel takes rows <= 32 at widths <= ACME_BC_FUSED_MAX_WIDTH (at most 256).
@pytest.mark.parametrize("hidden,rows,path", [
    ((32, 32), 1, "fused"), ((32, 32), 2, "fused"), ((32, 32), 17, "fused"),
    ((32, 32), 32, "fused"), ((257,), 1, "layered"), ((257,), 17, "layered"),
    ((32, 32), 33, "layered")])
def test_act_matches_f64_and_epsilon_greedy(hidden, rows, path):
    from acme_amd.native import epsilon_greedy
    D, A = 10, 5
    assert (rows <= _lib.BC_FUSED_MAX_ROWS
            and max(hidden + (D, A)) <= _lib.BC_FUSED_MAX_WIDTH) == (path == "fused")
    n = _native(D, hidden, A, 4, rows=rows)
    p = _params(D, hidden, A, 7)
    n.set_params(p)
    before = [x.clone() for x in (n.params, n.m, n.v, n.grads)]
    obs = np.random.default_rng(8).standard_normal((33, D)).astype(np.float32)[:rows]
    ref = _forward({k: torch.tensor(v, dtype=torch.float64) for k, v in p.items()}, obs)[0]
    for eps, seed, step in ((0.0, 1, 0), (0.3, 2, 5), (1.0, 3, 2 ** 40)):
        logits, actions = n.act(torch.as_tensor(obs).cuda(), eps, seed, step)
        _close(logits.cpu().numpy(), ref.numpy(), f"logits eps={eps}")
        want = epsilon_greedy(logits.contiguous(), eps, seed, step)
        assert torch.equal(actions, want)
        only = n.act_packed(torch.as_tensor(obs).cuda(), eps, seed, step, with_logits=False)
        assert torch.equal(only, want)
    for x, y in zip(before, (n.params, n.m, n.v, n.grads)):
        assert torch.equal(x.view(torch.int32), y.view(torch.int32))
    with pytest.raises(ValueError, match="rows must be in"):
        n.act(torch.zeros(rows + 1, D, device="cuda"))


@pytest.mark.parametrize("hidden", [(32, 32), (257,)])
def test_act_ties_and_the_update(hidden):
    from acme_amd.native import epsilon_greedy
    D, A, B = 10, 5, 8
    n = _native(D, hidden, A, B, rows=B)
    n.set_params({k: np.zeros_like(v) for k, v in _params(D, hidden, A, 0).items()})
    obs, act = _batch(B, D, A, 11)
    draws = []
    for step in (0, 1):  # every action tied: the rule's draws under two counters
        logits, actions = n.act(torch.as_tensor(obs).cuda(), 0.0, 9, step)
        assert (logits == 0).all()
        assert torch.equal(actions, epsilon_greedy(logits.contiguous(), 0.0, 9, step))
        draws.append(actions.cpu().numpy())
    assert (draws[0] != draws[1]).any() and len(set(draws[0])) > 1
    n.set_params(_params(D, hidden, A, 9))
    state = _state_of(n)
    n.step(*_dev(obs, act))
    logits, _ = n.act(torch.as_tensor(obs).cuda())  # no synchronisation: the step's stream
    _, _, new = _ref_step(state, obs, act)
    f = lambda q: _forward({k: torch.as_tensor(v) for k, v in q.items()}, obs)[0].numpy()  # noqa
    assert np.abs(f(new["params"]) - f(state["params"])).max() > 1e-4
    _close(logits.cpu().numpy(), f(new["params"]), "logits after step")


def test_learner_on_a_replay_table():
    from acme_amd import datasets, replay
    from acme_amd.adders import reverb as adders
    from acme_amd.agents.actors import FeedForwardActor
    from acme_amd.agents.bc import BCLearner
    D, hidden, A, B = 4, (64, 64), 3, 8
    table = replay.Table(name=adders.DEFAULT_PRIORITY_TABLE, sampler=replay.selectors.Uniform(),
                         remover=replay.selectors.Fifo(), max_size=16,
                         rate_limiter=replay.rate_limiters.MinSize(1))
    server = replay.Server([table], port=None)
    rng = np.random.default_rng(0)
    for i in range(B):
        table.insert((rng.standard_normal(D).astype(np.float32), np.int32(i % A), np.float32(0),
                      np.float32(1), rng.standard_normal(D).astype(np.float32)), 1.0)
    dataset = datasets.make_reverb_dataset(server_address=f"localhost:{server.port}", batch_size=B)
    seen, logged = [], []

    class Data:  # the learner's iterator, recording what it hands out
        batch_size = B

        def __iter__(self):
            for s in dataset:
                seen.append(s)
                yield s

    class Log:
        write = staticmethod(logged.append)

    net = MLP(D, hidden, A)
    learner = BCLearner(net, LR, Data(), logger=Log(), seed=5)
    z = lambda q: {k: np.zeros_like(np.asarray(v, np.float64)) for k, v in q.items()}  # noqa
    p0 = {k: v.astype(np.float64) for k, v in net.init(5).items()}
    state = dict(params=p0, m=z(p0), v=z(p0), num_steps=0)
    for s in range(3):
        learner.step()
        o, a = (x.cpu().numpy() for x in seen[s].data[:2])
        out, _, state = _ref_step(state, o, a)
        _close(logged[s]["loss"].item(), out["loss"], f"loss {s}")
        _close(logged[s]["gradient_norm"].item(), out["gradient_norm"], f"gradient_norm {s}")
        assert logged[s]["steps"] == s + 1
    _check_params(learner.get_variables([])[0], state["params"])
    obs = seen[0].data[0].cpu().numpy()
    ref = _forward({k: torch.as_tensor(v) for k, v in state["params"].items()}, obs)[0].numpy()
    _close(learner.logits(obs), ref, "learner logits")
    actor = FeedForwardActor(learner.make_policy(epsilon=0.0))
    assert int(actor.select_action(obs[0])) == int(ref[0].argmax())


def test_limits():
    W, R, L = _lib.BC_MAX_WIDTH, _lib.BC_MAX_ROWS, _lib.MAX_MLP_LAYERS
    ok = dict(D=4, hidden=(4,), A=3, B=2, rows=2)
    for field, kw in (("obs_dim", dict(D=W + 1)), ("obs_dim", dict(D=0)),
                      ("hidden\\[1\\]", dict(hidden=(4, W + 1))), ("hidden\\[0\\]", dict(hidden=(0,))),
                      ("num_actions", dict(A=_lib.BC_MAX_ACTIONS + 1)), ("num_actions", dict(A=0)),
                      ("max_batch", dict(B=R + 1)), ("max_batch", dict(B=0)),
                      ("max_act_rows", dict(rows=R + 1)), ("max_act_rows", dict(rows=0)),
                      ("hidden", dict(hidden=(4,) * (L + 1)))):
        with pytest.raises(ValueError, match=field):
            _native(**{**ok, **kw})
    for B, D, hidden, A in ((2, W, (W, W), _lib.BC_MAX_ACTIONS), (R, 6, (12,) * L, 3)):
        n = _native(D, hidden, A, B, rows=B)
        n.set_params(_params(D, hidden, A, 12))
        obs, act = _batch(B, D, A, 13)
        _check_step(n, obs, act, tag=" limit", margin=B < R)
        logits, actions = n.act(torch.as_tensor(obs).cuda())
        p = {k: torch.tensor(v, dtype=torch.float64) for k, v in n.get_params("params").items()}
        _close(logits.cpu().numpy(), _forward(p, obs)[0].numpy(), "logits limit")
        assert torch.equal(actions.cpu(), logits.cpu().argmax(dim=1).to(torch.int32))
