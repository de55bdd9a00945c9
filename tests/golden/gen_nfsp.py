#!/usr/bin/env python3
"""Generate tests/golden/nfsp.npz from the REFERENCE's NFSP agent (rlcard/agents/nfsp_agent.py). Test infrastructure
only, like gen_dqn.py (whose set-up it reuses): it runs where the reference is present, and nothing in the product
imports it. Data only, plain arrays (allow_pickle=False).

Per game G in (leduc [64, 64], limit [128, 128, 64]) a seeded reference NFSPAgent is trained on the CPU against a
RandomAgent for SPECS[G]['episodes'] episodes of sample_episode_policy -> env.run(is_training=True) -> reorganize ->
feed, with anticipatory_param 0.5 and batch_size = min_buffer_size_to_learn = 32, so train_sl runs (asserted: train_t >
0, and the BatchNorm running mean has left zero). Then:

  G_mlp                      the hidden widths (the network's mlp_layers without the final num_actions)
  G_sd_<key>                 every entry of agent.policy_network.state_dict() (keys mlp.1.*, mlp.2.*, mlp.4.*, ...)
  G_obs u8 [R, obs_dim], G_legal u8 [R, 1] (bitmask, bit a = action a)
                             R = 256 observations of random play (both seats)
  G_probs f32 [R, A]         agent._act(obs) = np.exp(policy_network(obs)), every action
  G_legal_probs f64 [R, A]   remove_illegal(G_probs[r], legal ids)

and for leduc the last train_sl() call that took a step, its locals as the reference computed them:

  leduc_sl_info_states u8 [B, 36], leduc_sl_action_probs f32 [B, 4] (eval_action_probs), leduc_sl_loss f64 (ce_loss)
  leduc_slpre_<key>          policy_network.state_dict() as that call found it (the loss is a function of these and the
                             batch: the forward runs in train mode, on the batch's own statistics)

The generator asserts that every stored action_probs row is one-hot, and that fewer than 1 % of the observation rows
have a legal action whose logit lies 87 to 104 below the row's maximum: there exp() is denormal in fp32, and a device
expf that flushes denormals may differ from the reference (tests/test_gpu_nfsp.py).
"""
import contextlib
import os
import sys

import numpy as np

import gen_golden
from gen_dqn import ROWS, bitmask

OUT = os.path.dirname(os.path.abspath(__file__))
SPECS = {
    'leduc': dict(env_id='leduc-holdem', mlp=[64, 64], episodes=200, seed=52),
    'limit': dict(env_id='limit-holdem', mlp=[128, 128, 64], episodes=85, seed=53),
}


def train_agent(spec, record):
    import torch
    import rlcard
    from rlcard.agents import NFSPAgent, RandomAgent
    from rlcard.utils import set_seed, reorganize
    set_seed(spec['seed'])
    env = rlcard.make(spec['env_id'], config={'seed': spec['seed']})
    agent = NFSPAgent(num_actions=env.num_actions, state_shape=env.state_shape[0],
                      hidden_layers_sizes=list(spec['mlp']), q_mlp_layers=list(spec['mlp']), anticipatory_param=0.5,
                      batch_size=32, min_buffer_size_to_learn=32, q_replay_memory_init_size=40,
                      q_update_target_estimator_every=10, device=torch.device('cpu'))
    env.set_agents([agent, RandomAgent(num_actions=env.num_actions)])
    code = NFSPAgent.train_sl.__code__
    pre = {}

    def prof(frame, event, arg):   # the state_dict every train_sl call finds, and its locals where it took a step
        if frame.f_code is not code:
            return
        if event == 'call':
            pre.clear()
            pre.update({k: v.clone() for k, v in frame.f_locals['self'].policy_network.state_dict().items()})
        elif event == 'return' and arg is not None:
            record.clear()
            record.update({k: v for k, v in frame.f_locals.items() if k != 'self'})
            record['pre'] = dict(pre)

    feeds = 0
    sys.setprofile(prof)
    try:
        with open(os.devnull, 'w') as null, contextlib.redirect_stdout(null):   # (feed prints every loss)
            for _ in range(spec['episodes']):
                agent.sample_episode_policy()
                trajectories, payoffs = env.run(is_training=True)
                for ts in reorganize(trajectories, payoffs)[0]:
                    agent.feed(ts)
                    feeds += 1
    finally:
        sys.setprofile(None)
    print('%s: %d feeds, %d train_sl steps, reservoir %d' % (spec['env_id'], feeds, agent.train_t,
                                                            len(agent._reservoir_buffer)))
    assert agent.train_t > 0
    return env, agent


def observations(env, agent, seed):
    """ROWS states of uniformly random play (both seats' views) with the agent's probabilities"""
    from rlcard.utils.utils import remove_illegal
    rng = np.random.RandomState(seed)
    obs, legal, probs, lprobs = [], [], [], []
    while len(obs) < ROWS:
        state, _ = env.reset()
        while not env.is_over() and len(obs) < ROWS:
            ids = list(state['legal_actions'].keys())
            obs.append(np.asarray(state['obs']))
            legal.append([bitmask(ids)])
            p = agent._act(state['obs'])
            probs.append(p)
            lprobs.append(remove_illegal(p, ids))
            state, _ = env.step(ids[rng.randint(len(ids))])
    obs = np.stack(obs)
    assert np.array_equal(obs, obs.astype(np.uint8))
    probs = np.stack(probs)
    assert probs.dtype == np.float32
    return obs.astype(np.uint8), np.array(legal, np.uint8), probs, np.stack(lprobs).astype(np.float64)


def main():
    import torch
    gen_golden.setup_reference()
    out = {}
    for game, spec in SPECS.items():
        rec = {}
        env, agent = train_agent(spec, rec)
        out[game + '_mlp'] = np.array(spec['mlp'], np.int32)
        for k, v in agent.policy_network.state_dict().items():
            out['%s_sd_%s' % (game, k)] = v.cpu().numpy()
        assert np.abs(out[game + '_sd_mlp.1.running_mean']).max() > 0, 'BatchNorm statistics are still the initial ones'
        obs, legal, probs, lprobs = observations(env, agent, spec['seed'] + 1)
        out[game + '_obs'], out[game + '_legal'] = obs, legal
        out[game + '_probs'], out[game + '_legal_probs'] = probs, lprobs
        with torch.no_grad():
            logits = agent.policy_network.mlp(torch.from_numpy(obs).float()).numpy().astype(np.float64)
        mask = np.array([[(int(m[0]) >> a) & 1 for a in range(probs.shape[1])] for m in legal], bool)
        below = logits.max(axis=1, keepdims=True) - logits
        band = int((mask & (below >= 87) & (below <= 104)).any(axis=1).sum())
        assert band < ROWS / 100, '%d rows with a legal logit in the denormal band' % band
        print('%s: %d rows, %d in the denormal band, smallest legal probability %.3e'
              % (game, len(obs), band, lprobs[mask].min()))
        if game != 'leduc':
            continue
        states = rec['info_states'].numpy()
        ap = rec['eval_action_probs'].numpy()
        assert np.array_equal(states, states.astype(np.uint8)) and states.shape == (32, 36)
        assert ap.shape == (32, 4) and np.all((ap == 0) | (ap == 1)) and np.all(ap.sum(axis=1) == 1), 'not one-hot'
        out['leduc_sl_info_states'] = states.astype(np.uint8)
        out['leduc_sl_action_probs'] = ap.astype(np.float32)
        out['leduc_sl_loss'] = np.float64(rec['ce_loss'])
        for k, v in rec['pre'].items():
            out['leduc_slpre_' + k] = v.cpu().numpy()
        for t in agent._reservoir_buffer:
            assert np.all((t.action_probs == 0) | (t.action_probs == 1)) and t.action_probs.sum() == 1, 'not one-hot'
        print('leduc train_sl(): batch %d, loss %.6f' % (len(states), rec['ce_loss']))
    path = os.path.join(OUT, 'nfsp.npz')
    np.savez_compressed(path, **out)
    print('nfsp.npz: %d arrays, %d bytes' % (len(out), os.path.getsize(path)))


if __name__ == '__main__':
    main()
