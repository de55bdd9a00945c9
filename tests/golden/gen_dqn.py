#!/usr/bin/env python3
"""Generate tests/golden/dqn.npz from the REFERENCE's DQN agent (rlcard/agents/dqn_agent.py). Test infrastructure only,
like gen_golden.py (whose reference set-up it reuses): it runs where the reference is present, and nothing in the
product imports it. Data only, plain arrays (allow_pickle=False).

Per game G in (leduc [64, 64], limit [128, 128, 64]) a seeded reference DQNAgent is trained on the CPU against a
RandomAgent for SPECS[G]['episodes'] episodes of env.run(is_training=True) -> reorganize -> feed, so its BatchNorm running
statistics are not the initial ones. Then:

  G_mlp                      the hidden widths
  G_sd_<key>                 every entry of agent.q_estimator.qnet.state_dict() (keys fc_layers.1.*, fc_layers.2.*, ...)
  G_obs u8 [R, obs_dim], G_legal u8 [R, 1] (bitmask, bit a = action a), G_predict f32 [R, num_actions]
                             R = 256 observations of random play (both seats) with the reference's agent.predict rows
                             (-inf where illegal; the values are float32 numbers, stored exactly)

and for leduc the last train() call of the run, its locals as the reference computed them:

  leduc_train_state u8 [B, 36], _action i64 [B], _reward f32 [B], _next_state u8 [B, 36], _done u8 [B],
  _next_legal u8 [B, 1] (bitmask of legal_actions_batch), _q_next f32 [B, 4], _q_next_target f32 [B, 4],
  _best i64 [B], _target f64 [B] (target_batch as numpy made it), leduc_train_gamma f64

The generator asserts that the two estimators differed at that call, that the batch has terminal and non-terminal rows,
and that fewer than 1 % of the predict rows have a top-two legal gap under 1e-4 (tests/test_gpu_dqn.py's greedy check).
"""
import os
import sys

import numpy as np

import gen_golden

OUT = os.path.dirname(os.path.abspath(__file__))
SPECS = {
    'leduc': dict(env_id='leduc-holdem', mlp=[64, 64], episodes=60, seed=42),
    'limit': dict(env_id='limit-holdem', mlp=[128, 128, 64], episodes=60, seed=43),
}
ROWS = 256


def bitmask(ids):
    return np.uint8(sum(1 << int(i) for i in ids))


def train_agent(spec, record):
    import torch
    import rlcard
    from rlcard.agents import DQNAgent, RandomAgent
    from rlcard.utils import set_seed, reorganize
    set_seed(spec['seed'])
    env = rlcard.make(spec['env_id'], config={'seed': spec['seed']})
    agent = DQNAgent(num_actions=env.num_actions, state_shape=env.state_shape[0], mlp_layers=list(spec['mlp']),
                     replay_memory_init_size=40, update_target_estimator_every=10, batch_size=32,
                     device=torch.device('cpu'))
    env.set_agents([agent, RandomAgent(num_actions=env.num_actions)])
    code = DQNAgent.train.__code__

    def prof(frame, event, arg):   # the locals of every DQNAgent.train call as it returns: the last one is kept
        if event == 'return' and frame.f_code is code:
            record.clear()
            record.update({k: v for k, v in frame.f_locals.items() if k != 'self'})

    feeds = 0
    sys.setprofile(prof)
    try:
        for _ in range(spec['episodes']):
            trajectories, payoffs = env.run(is_training=True)
            for ts in reorganize(trajectories, payoffs)[0]:
                agent.feed(ts)
                feeds += 1
    finally:
        sys.setprofile(None)
    print('\n%s: %d feeds, %d train steps' % (spec['env_id'], feeds, agent.train_t))
    return env, agent


def observations(env, agent, seed):
    """ROWS states of uniformly random play (both seats' views) with the agent's predict rows"""
    rng = np.random.RandomState(seed)
    obs, legal, pred = [], [], []
    while len(obs) < ROWS:
        state, _ = env.reset()
        while not env.is_over() and len(obs) < ROWS:
            ids = list(state['legal_actions'].keys())
            obs.append(np.asarray(state['obs']))
            legal.append([bitmask(ids)])
            pred.append(agent.predict(state))
            state, _ = env.step(ids[rng.randint(len(ids))])
    obs = np.stack(obs)
    assert np.array_equal(obs, obs.astype(np.uint8))
    pred = np.stack(pred)
    assert np.array_equal(pred.astype(np.float32).astype(np.float64), pred)
    return obs.astype(np.uint8), np.array(legal, np.uint8), pred.astype(np.float32)


def main():
    gen_golden.setup_reference()
    out = {}
    for game, spec in SPECS.items():
        rec = {}
        env, agent = train_agent(spec, rec)
        out[game + '_mlp'] = np.array(spec['mlp'], np.int32)
        for k, v in agent.q_estimator.qnet.state_dict().items():
            out['%s_sd_%s' % (game, k)] = v.cpu().numpy()
        rm = out[game + '_sd_fc_layers.1.running_mean']
        assert np.abs(rm).max() > 0, 'BatchNorm statistics are still the initial ones'
        obs, legal, pred = observations(env, agent, spec['seed'] + 1)
        out[game + '_obs'], out[game + '_legal'], out[game + '_predict'] = obs, legal, pred
        top = np.sort(np.where(np.isfinite(pred), pred, -np.inf), axis=1)[:, ::-1]
        close = int((np.isfinite(top[:, 1]) & (top[:, 0] - top[:, 1] < 1e-4)).sum())
        assert close <= ROWS // 100, '%d rows with a top-two gap under 1e-4' % close
        print('%s: %d predict rows, |q| <= %.3f, %d rows with a top-two gap under 1e-4'
              % (game, len(pred), np.abs(pred[np.isfinite(pred)]).max(), close))
        if game != 'leduc':
            continue
        B = agent.batch_size
        done = np.asarray(rec['done_batch'])
        assert done.any() and not done.all()
        assert not np.array_equal(rec['q_values_next'], rec['q_values_next_target'])
        out['leduc_train_state'] = np.asarray(rec['state_batch']).astype(np.uint8)
        out['leduc_train_action'] = np.asarray(rec['action_batch'], np.int64)
        out['leduc_train_reward'] = np.asarray(rec['reward_batch'], np.float32)
        assert np.array_equal(out['leduc_train_reward'].astype(np.float64), np.asarray(rec['reward_batch'], np.float64))
        out['leduc_train_next_state'] = np.asarray(rec['next_state_batch']).astype(np.uint8)
        out['leduc_train_done'] = done.astype(np.uint8)
        out['leduc_train_next_legal'] = np.array([[bitmask(l)] for l in rec['legal_actions_batch']], np.uint8)
        out['leduc_train_q_next'] = np.asarray(rec['q_values_next'], np.float32)
        out['leduc_train_q_next_target'] = np.asarray(rec['q_values_next_target'], np.float32)
        out['leduc_train_best'] = np.asarray(rec['best_actions'], np.int64)
        out['leduc_train_target'] = np.asarray(rec['target_batch'])
        out['leduc_train_gamma'] = np.float64(agent.discount_factor)
        assert out['leduc_train_state'].shape == (B, 36) and out['leduc_train_target'].shape == (B,)
        print('leduc train(): batch %d, %d terminal rows, target dtype %s' % (B, int(done.sum()),
                                                                             out['leduc_train_target'].dtype))
    path = os.path.join(OUT, 'dqn.npz')
    np.savez_compressed(path, **out)
    print('dqn.npz: %d arrays, %d bytes' % (len(out), os.path.getsize(path)))


if __name__ == '__main__':
    main()
