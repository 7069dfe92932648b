"""The sensory-perturbation study (--perturb) without a GPU: the NumPy statement of the bias model, the switch of the
training loop on a batched worker, and the C ABI's "off" default and refusals."""
import ctypes as C
import types

import numpy as np
import pytest

from perturb_spec import BIAS_OFF, BiasedArm


def _run(env, rng, episodes=3):
    out = []
    for _ in range(episodes):
        env.reset()
        task = int(rng.randint(env.nb_tasks))
        out.append(env.reset_task_goal(rng.uniform(-1, 1, 3).astype(np.float32), task))
        for _ in range(env.T):
            u = rng.uniform(-1.3, 1.3, 4).astype(np.float32)
            u[:3] = np.clip((env.o[3:6] - env.o[0:3]) * 20, -1, 1)      # (the TRUE object: carrying happens)
            u[3] = -1
            out.append(env.step(u))
    return out


def _flat(x):
    if isinstance(x, dict):
        return [v for k in sorted(x) for v in _flat(x[k])]
    if isinstance(x, (tuple, list)):
        return [v for e in x for v in _flat(e)]
    return [np.atleast_1d(np.asarray(x))]


@pytest.mark.parametrize('nb,dimo', [(4, 40), (8, 52)])
def test_spec_without_bias_is_the_oracle_bit_for_bit(nb, dimo):
    from oracle.env import SyntheticMultiTaskArm
    a = _run(SyntheticMultiTaskArm(nb, dimo, 12, seed=77, env_id=3), np.random.RandomState(1))
    b = _run(BiasedArm(nb, dimo, 12, seed=77, env_id=3), np.random.RandomState(1))
    for x, y in zip(_flat(a), _flat(b)):
        assert x.dtype == y.dtype and x.tobytes() == y.tobytes()


def test_spec_with_bias_reports_an_offset_object_that_moves_on_its_true_coordinates():
    from oracle.env import SyntheticMultiTaskArm
    true_env = SyntheticMultiTaskArm(4, 40, 12, seed=5, env_id=0)
    env = BiasedArm(4, 40, 12, seed=5, env_id=0, bias=True)
    a, b = _run(true_env, np.random.RandomState(2)), _run(env, np.random.RandomState(2))
    assert np.array_equal(env.o, true_env.o)                     # the state is the unbiased env's
    obs = b[-1][0]
    want = (env.o[3:6] + BIAS_OFF).astype(np.float32)
    assert np.array_equal(obs['observation'][3:6], want) and np.array_equal(obs['achieved_goal'][3:6], want)
    keep = np.r_[0:3, 6:40]
    assert np.array_equal(obs['observation'][keep], a[-1][0]['observation'][keep])
    assert np.abs(env.o[3:6] - b[0]['observation'][3:6] + BIAS_OFF).max() > 0      # object 1 was carried
    with pytest.raises(ValueError):
        BiasedArm(1, 8, 4, bias=True).reset()


class _Benv:
    def __init__(self, attached=False):
        self.marked, self.attached = None, attached

    def set_bias(self, idx):
        self.marked = list(idx)
        return self.attached


class _Pol:
    dropped = 0

    def drop_rollout_graphs(self):
        self.dropped += 1


def _worker(B, V, attached=False):
    w = types.SimpleNamespace(benv=_Benv(attached), rollout_batch_size=B, V=V, policy=_Pol(), envs=None)
    w.envs = [w.benv]
    return w


@pytest.mark.parametrize('V', [1, 3])
@pytest.mark.parametrize('B', [2, 4])
def test_perturb_switch_marks_envs_0_and_1_of_every_virtual_rank(B, V):
    from curious_amd.experiment.train import perturb_envs
    a, b = _worker(B, V), _worker(B, V)
    perturb_envs(a, b)
    want = [v * B + i for v in range(V) for i in range(2)]
    assert a.benv.marked == want and b.benv.marked == want
    assert a.policy.dropped == 0 and b.policy.dropped == 0
    # arrays attached only now: the captured rollouts (and the evaluator's slot batch) are dropped
    a, b = _worker(B, V, attached=True), _worker(B, V, attached=True)
    b._eval_env = object()
    perturb_envs(a, b)
    assert a.policy.dropped == 1 and b.policy.dropped == 1 and not hasattr(b, '_eval_env')


def test_perturb_switch_refuses_fewer_than_two_envs_per_rank():
    from curious_amd.experiment.train import perturb_envs
    with pytest.raises(NotImplementedError):
        perturb_envs(_worker(1, 3), _worker(2, 3))


def test_env_cfg_zero_initialised_is_off():
    from curious_amd import _lib, ops
    E = _lib.EnvCfg()
    assert E.bias is None and E.truth is None and list(E.bias_off) == [0.0, 0.0, 0.0]
    assert C.sizeof(_lib.EnvCfg) == 56
    e = ops.make_env_cfg(4, 40, 50, 1)
    assert e.bias is None and e.truth is None
    assert _lib.ABI_VERSION == 11


def test_library_refuses_a_bias_without_truth_or_without_object_1():
    """The checks come before anything touches the device (so they run here)."""
    from curious_amd import _lib
    L = _lib.lib()
    fake = [C.c_void_p(0x10000000 + 0x1000000 * i) for i in range(16)]
    lay = _lib.Layout()
    lay.T, lay.dimo, lay.dimag, lay.dimg, lay.dimu, lay.dimtd = 50, 40, 12, 12, 4, 4
    lay.off_o, lay.off_ag, lay.off_g, lay.off_u, lay.off_td, lay.row_stride = 0, 40, 52, 64, 68, 88

    def reset(E):
        return L.curious_env_reset_count(C.byref(E), C.byref(lay), 0, fake[0], fake[1], fake[2], 8, fake[3], fake[4],
                                         fake[5], fake[6], fake[7], None, None, 0, None)

    def step(E):
        return L.curious_env_step(C.byref(E), C.byref(lay), 0, fake[0], fake[1], fake[2], 4, 0, 8, fake[3], fake[4],
                                  fake[5], fake[6], fake[7], 72, 84, 0.05, None, None)
    E = _lib.EnvCfg()
    E.ntasks, E.dimo, E.T, E.seed = 4, 40, 50, 1
    E.bias = fake[8].value
    for f in (reset, step):
        assert f(E) != 0 and b'needs the true-state array' in L.curious_last_error()
    E.truth = fake[9].value
    E.ntasks, E.dimo = 1, 8
    for f in (reset, step):
        assert f(E) != 0 and b'has none' in L.curious_last_error()
    cfg = _lib.NetCfg()
    cfg.dimo, cfg.dimg, cfg.dimtd, cfg.layers, cfg.dimu, cfg.hidden, cfg.modular = 8, 3, 1, 3, 4, 256, 1
    cfg.max_u = 1.0
    rc = L.curious_policy_rollout(C.byref(cfg), fake[0], 8, 200.0, fake[1], 0.2, 0.3, 5, 1, None, fake[2], 4,
                                  C.byref(E), C.byref(lay), 0, fake[3], fake[4], 0, 50, fake[5], fake[6], fake[7],
                                  fake[8], fake[9], 72, 84, 0.05, None, None)
    assert rc != 0 and b'has none' in L.curious_last_error()
