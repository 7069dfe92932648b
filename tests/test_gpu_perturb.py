"""The sensory-perturbation study (--perturb) on the GPU-resident batched env, against the NumPy statement of the bias
model (tests/perturb_spec.py): the env kernels, every acting route, the evaluator's slots and the training loop."""
import os

import numpy as np
import pytest
import torch

from perturb_spec import BIAS_OFF, BiasedArm
from test_gpu_agent import T, build_pair
from test_gpu_round6 import _rows, _same_state

pytestmark = pytest.mark.gpu


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _replay(rec, tasks, goals, episodes_before, seed, env_ids, biased, nb, dimo, Tn):
    """Each env's recorded actions through the spec (env id, episode counter, task, goal and seed known): the recorded o /
    ag / is_success / change must come out bit for bit."""
    G = 3 * nb
    r = {k: v.cpu().numpy() for k, v in rec.items()}
    for i in range(len(tasks)):
        spec = BiasedArm(nb, dimo, Tn, seed=seed, env_id=int(env_ids[i]), bias=bool(biased[i]))
        spec.episode = int(episodes_before[i])
        spec.reset()
        obs = spec.reset_task_goal(goals[i], int(tasks[i]))
        np.testing.assert_array_equal(r['o'][i, 0], obs['observation'], err_msg='env %d row 0' % i)
        np.testing.assert_array_equal(r['ag'][i, 0], obs['achieved_goal'])
        ag0 = obs['achieved_goal']
        for t in range(Tn):
            obs, _, _, info = spec.step(r['u'][i, t])
            np.testing.assert_array_equal(r['o'][i, t + 1], obs['observation'], err_msg='env %d t %d' % (i, t))
            np.testing.assert_array_equal(r['ag'][i, t + 1], obs['achieved_goal'])
            assert r['info_is_success'][i, t, 0] == np.float32(info['is_success']), (i, t)
            np.testing.assert_array_equal(r['change'][i, t], (np.abs(ag0 - obs['achieved_goal'][:G]) > 1e-3)
                                          .astype(np.float32))


@pytest.mark.parametrize('name', ['MultiTaskFetchArm4-v5', 'MultiTaskFetchArm8-v5'])
def test_env_reset_and_step_with_bias_bit_exact_vs_spec(name):
    """env_reset_kernel / env_step_kernel with the bias on a third of 70 envs against the spec, every env, bit for bit;
    the grippers of biased envs are steered onto the TRUE object 1 so that carrying happens there."""
    from curious_amd import ops
    from curious_amd.layout import RecordLayout
    from oracle.env import ENV_CONFIGS
    nb, dimo, _ = ENV_CONFIGS[name]
    Tn, n, G, seed = 9, 70, 3 * nb, 123456789012
    shapes = dict(o=(Tn + 1, dimo), u=(Tn, 4), g=(Tn, G), ag=(Tn + 1, G), task_descr=(Tn, nb), change=(Tn, G),
                  info_is_success=(Tn, 1))
    layout = RecordLayout(shapes, Tn)
    biased = (np.arange(n) % 3) == 1
    mask = dev(biased.astype(np.int32))
    truth = torch.full([n, 3], -7.0, device='cuda')
    ecfg = ops.make_env_cfg(nb, dimo, Tn, seed, bias=mask, truth=truth)
    rng = np.random.RandomState(0)
    envs = [BiasedArm(nb, dimo, Tn, seed=seed, env_id=5 + i, bias=biased[i]) for i in range(n)]
    o = torch.zeros([n, dimo], device='cuda'); ag = torch.zeros([n, G], device='cuda')
    g = torch.zeros([n, G], device='cuda'); td = torch.zeros([n, nb], device='cuda')
    staging = torch.zeros([n, Tn + 1, layout.row_stride], device='cuda')
    for episode in range(2):
        tasks = rng.randint(nb, size=n).astype(np.int32)
        goals = rng.uniform(-1, 1, (n, 3)).astype(np.float32)
        ops.env_reset(ecfg, layout, 5, dev(np.full(n, episode, np.int32)), dev(tasks), dev(goals), n, o, ag, g, td,
                      staging)
        obs = []
        for i, e in enumerate(envs):
            e.reset()
            obs.append(e.reset_task_goal(goals[i], tasks[i]))
        np.testing.assert_array_equal(o.cpu().numpy(), np.stack([x['observation'] for x in obs]))
        np.testing.assert_array_equal(ag.cpu().numpy(), np.stack([x['achieved_goal'] for x in obs]))
        true0 = np.stack([e.o[3:6].copy() for e in envs])
        np.testing.assert_array_equal(truth.cpu().numpy()[biased], true0[biased])
        ag0 = np.stack([x['achieved_goal'] for x in obs])
        epi1 = dev(np.full(n, episode + 1, np.int32))
        for t in range(Tn):
            u = rng.uniform(-1.3, 1.3, (n, 4)).astype(np.float32)
            true = np.stack([e.o.copy() for e in envs])
            sel = np.arange(n) % 3 != 2
            u[sel, :3] = np.clip((true[sel, 3:6] - true[sel, 0:3]) * 20, -1, 1)
            u[sel, 3] = -1
            ops.env_step(ecfg, layout, 5, epi1, dev(tasks), dev(u), t, n, o, ag, g, td, staging, 0.05)
            res = [e.step(u[i]) for i, e in enumerate(envs)]
            want_o = np.stack([r[0]['observation'] for r in res])
            np.testing.assert_array_equal(o.cpu().numpy(), want_o)
            np.testing.assert_array_equal(ag.cpu().numpy(), want_o[:, :G])
            rec = layout.record_views(staging)
            np.testing.assert_array_equal(rec['o'][:, t + 1].cpu().numpy(), want_o)
            np.testing.assert_array_equal(rec['info_is_success'][:, t, 0].cpu().numpy(),
                                          np.array([r[3]['is_success'] for r in res], np.float32))
            np.testing.assert_array_equal(rec['change'][:, t].cpu().numpy(),
                                          (np.abs(ag0 - want_o[:, :G]) > 1e-3).astype(np.float32))
        true1 = np.stack([e.o[3:6] for e in envs])
        np.testing.assert_array_equal(truth.cpu().numpy()[biased], true1[biased])
        assert (truth.cpu().numpy()[~biased] == -7.0).all()              # (unbiased envs: no truth is written)
        # a biased env's true object moved (carried), and what it reports is the true position + the offset
        assert np.abs(true1[biased] - true0[biased]).max() > 0
        np.testing.assert_array_equal(o.cpu().numpy()[biased, 3:6], (true1[biased] + BIAS_OFF).astype(np.float32))
        assert not np.array_equal(o.cpu().numpy()[biased, 3:6], true1[biased])


@pytest.mark.parametrize('layers', [3, 4])          # 3: the weights-resident rollout kernel; 4: the streaming one
def test_acting_routes_with_bias_equal_launch_per_step_and_spec(layers, route):
    """With the bias on a third of 64 envs: the one-launch rollout (rows_act multi-step / resident) == T launches of the
    fused act-step (tiled: act_step_kernel, rows: one-step rows_act), every env replays through the spec bit for bit,
    and the unbiased envs are what a run without the bias (NULL mask) records."""
    from curious_amd import ops
    from curious_amd.envs import EnvFactory, REWARD_EPS
    nb, dimo, B = 4, 40, 64
    biased = (np.arange(B) % 3) == 1
    outs = {}
    for mode in ('rollout', 'steps'):
        for with_bias in (True, False):
            if mode == 'steps' and not with_bias:
                continue
            agent, _ = build_pair(nb, dimo, rng_mode='device', use_graph=False, layers=layers)
            env = EnvFactory('MultiTaskFetchArm4-v5').make_batched(B)
            env.seed(11)
            if with_bias:
                assert env.set_bias(np.nonzero(biased)[0])
            rs = np.random.RandomState(3)
            ws = torch.empty(ops.workspace_floats(agent.net_cfg, B), dtype=torch.float32, device='cuda')
            u = torch.zeros([B, 4], dtype=torch.float32, device='cuda')
            recs = []
            for ep in range(2):
                tasks, goals = rs.randint(0, nb, B), rs.uniform(-1, 1, (B, 3)).astype(np.float32)
                env.reset_all(tasks, goals)
                args = (agent.net_cfg, agent.theta, B, agent.clip_obs, ws, 0.2, 0.3, 12345)
                tail = (env.o, env.ag, env.g, env.td, env.staging, REWARD_EPS)
                if mode == 'rollout':
                    ops.policy_rollout(*args, 1 + ep * T, u, env._cfg, env.layout, env.env_id0, env.episode, env.tasks,
                                       0, T, *tail, flags=env.flags)
                else:
                    for t in range(T):
                        ops.policy_act_env_step(*args, 1 + ep * T + t, u, env._cfg, env.layout, env.env_id0, env.episode,
                                                env.tasks, t, *tail, flags=env.flags)
                torch.cuda.synchronize()
                recs.append((env.staging.clone(), u.clone(), env.flags.clone(), env.o.clone(), env.ag.clone()))
                if mode == 'steps':
                    _replay(env.layout.record_views(env.staging), tasks, goals, np.full(B, ep), 11,
                            np.arange(B), biased, nb, dimo, T)
            outs[mode, with_bias] = recs
    for a, b in zip(outs['rollout', True], outs['steps', True]):
        for x, y in zip(a, b):
            assert torch.equal(x, y)
    keep = torch.from_numpy(~biased).cuda()
    for a, b in zip(outs['rollout', True], outs['rollout', False]):
        for x, y in zip(a[:2] + a[3:], b[:2] + b[3:]):
            assert torch.equal(x[keep], y[keep])
        assert not torch.equal(a[0][~keep], b[0][~keep])


def test_evaluator_slots_follow_the_bias_of_the_envs_they_wrap():
    """The evaluator's slot batch (several rollouts of the same envs in one launch, wrap = n_envs) reads the bias flag of
    the env a slot wraps: every slot replays through the spec, biased exactly where its env is."""
    from curious_amd.envs import EnvFactory
    from curious_amd.rollout import RolloutWorker
    from curious_amd import logger
    dims = dict(o=40, u=4, g=12, ag=12, task_descr=4, info_is_success=1)
    agent, _ = build_pair(4, 40, rng_mode='device', use_graph=True)
    B = 48
    w = RolloutWorker(EnvFactory('MultiTaskFetchArm4-v5'), agent, dims, logger, T=T, rollout_batch_size=B,
                      exploit=True, compute_Q=True, structure='curious', task_selection='active_competence_progress',
                      queue_length=6, eval=True)
    w.seed(5)
    np.random.seed(8)
    w.generate_eval_rollouts(2)                                       # (slot batch and graphs exist before the switch)
    from curious_amd.experiment.train import perturb_envs
    perturb_envs(w, w)
    w.generate_eval_rollouts(3)
    torch.cuda.synchronize()
    big = w._eval_env
    assert big._wrap == B
    assert big.bias_mask is w.benv.bias_mask
    slots = big.n
    ep_after = big.episode.cpu().numpy()
    env_of = np.arange(slots) % B
    _replay(big.layout.record_views(big.staging), big.tasks_host, big.goals_host, ep_after - 1, 5,
            w.benv.env_id0 + env_of, env_of < 2, 4, 40, T)


def _launch(tmp, sub, n_epochs, resume=None, perturb=False, perturb_epoch=250, **over):
    from curious_amd.experiment import config, train as tr
    config.CACHED_ENVS.clear()
    root = os.path.join(str(tmp), sub, '')
    params = dict(rng_mode='device', use_graph=True, async_store=True, n_cycles=3, n_batches=6, rollout_batch_size=4,
                  n_test_rollouts=2)
    params.update(over)
    tr.launch(env='MultiTaskFetchArm4-v5', trial_id=0, n_epochs=n_epochs, num_cpu=params.pop('num_cpu', 1), seed=7,
              policy_save_interval=2, clip_return=1, normalize_obs=False, structure='curious',
              task_selection='active_competence_progress', goal_selection='random', goal_replay='her',
              task_replay='replay_task_cp_buffer', save_policies=True, override_params=params, save_root=root,
              resume=resume, perturb=perturb, perturb_epoch=perturb_epoch)
    return os.path.join(root, 'MultiTaskFetchArm4-v5', '0')


@pytest.mark.parametrize('num_cpu', [1, 3])
def test_perturbed_training_job_runs_and_equals_the_plain_job_before_the_switch(tmp_path, num_cpu):
    import json
    pert = _launch(tmp_path, 'perturbed', 3, perturb=True, perturb_epoch=1, num_cpu=num_cpu)
    plain = _launch(tmp_path, 'plain', 3, num_cpu=num_cpu)
    a, b = _rows(os.path.join(pert, 'progress.csv')), _rows(os.path.join(plain, 'progress.csv'))
    assert [r['epoch'] for r in a] == ['-1', '0', '1', '2']
    assert a[:2] == b[:2]
    p = json.load(open(os.path.join(pert, 'params.json')))
    assert p['perturb'] is True and p['perturb_epoch'] == 1


def test_perturbed_training_job_resumes_bit_for_bit(tmp_path):
    from curious_amd.checkpoint import STATE_DIR, latest_epoch
    straight = _launch(tmp_path, 'straight', 5, perturb=True, perturb_epoch=2)
    first = _launch(tmp_path, 'resumed', 3, perturb=True, perturb_epoch=2)
    assert latest_epoch(first)['epoch'] == 2
    _launch(tmp_path, 'resumed', 5, resume=first, perturb=True, perturb_epoch=2)
    assert _rows(os.path.join(straight, 'progress.csv')) == _rows(os.path.join(first, 'progress.csv'))
    sa = torch.load(os.path.join(straight, STATE_DIR, 'rank000_epoch000004.pt'), weights_only=False)
    sb = torch.load(os.path.join(first, STATE_DIR, 'rank000_epoch000004.pt'), weights_only=False)
    _same_state(sa, sb)
    with pytest.raises(ValueError, match='configured differently'):
        _launch(tmp_path, 'resumed', 6, resume=first, perturb=True, perturb_epoch=3)
