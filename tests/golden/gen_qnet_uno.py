#!/usr/bin/env python3
"""Generate tests/golden/dqn_uno.npz and tests/golden/nfsp_uno.npz from the REFERENCE's DQN and NFSP agents on UNO
(rlcard/agents/dqn_agent.py, nfsp_agent.py; rlcard/envs/uno.py: 240 obs bytes, 61 actions). Test infrastructure only,
like gen_dqn.py and gen_nfsp.py, whose set-up, training loops and recipe (mlp [64, 64], replay_memory_init_size 40,
update_target_estimator_every 10, batch_size 32; NFSP anticipatory_param 0.5, min_buffer_size_to_learn 32) it reuses by
import: it runs where the reference is present, and nothing in the product imports it. Data only, plain arrays
(allow_pickle=False). The arrays are those of dqn.npz / nfsp.npz for Leduc under the game name `uno`:

  dqn_uno.npz   uno_mlp, uno_sd_<key>, uno_obs u8 [256, 240], uno_legal u8 [256, 8] (bit a of the little-endian row =
                action a), uno_predict f32 [256, 61] (-inf where illegal), and the last train() call: uno_train_state,
                _action, _reward, _next_state, _done, _next_legal u8 [B, 8], _q_next, _q_next_target, _best, _target,
                uno_train_gamma
  nfsp_uno.npz  uno_mlp, uno_sd_<key>, uno_obs, uno_legal, uno_probs f32 [256, 61], uno_legal_probs f64 [256, 61], and
                the last train_sl() call that took a step: uno_sl_info_states, uno_sl_action_probs, uno_sl_loss,
                uno_slpre_<key>

What the generator asserts, so that the caps of tests/test_gpu_qnet_wide.py hold for the reference alone: the BatchNorm
statistics have left their initial values; fewer than 1 % of the predict rows have a top-two gap under 1e-4, over the
legal actions and over all 61; the rows contain a single-legal-action row, a row with >= 5 legal ids and a row with
`draw` (id 60) legal; at most 5 % of the NFSP rows are hazard rows (the best legal logit 86 to 106 below the row's
maximum: exp() is denormal in fp32 there, and a device expf that flushes denormals gives the uniform fallback where the
reference renormalises); and at least one row's legal mass underflows entirely (every legal logit >= 106 below the
maximum: the uniform fallback against the reference).
"""
import os

import numpy as np

import gen_dqn
import gen_golden
import gen_nfsp
from gen_dqn import ROWS

OUT = os.path.dirname(os.path.abspath(__file__))
A, D = 61, 240
DQN_SPEC = dict(env_id='uno', mlp=[64, 64], episodes=30, seed=44)
NFSP_SPEC = dict(env_id='uno', mlp=[64, 64], episodes=30, seed=55)   # (seed 54: 17 hazard rows, over the 5 % cap)


def masks(id_lists):
    return np.stack([gen_golden.packbits(ids, A) for ids in id_lists]).astype(np.uint8)


def observations(env, seed):
    """ROWS states of uniformly random play (both seats' views): obs u8 [ROWS, 240], the legal id lists, the states"""
    rng = np.random.RandomState(seed)
    obs, ids_of, states = [], [], []
    while len(obs) < ROWS:
        state, _ = env.reset()
        while not env.is_over() and len(obs) < ROWS:
            ids = list(state['legal_actions'].keys())
            obs.append(np.asarray(state['obs']).reshape(-1))
            ids_of.append(ids)
            states.append(state)
            state, _ = env.step(ids[rng.randint(len(ids))])
    obs = np.stack(obs)
    assert obs.shape == (ROWS, D) and np.array_equal(obs, obs.astype(np.uint8))
    return obs.astype(np.uint8), ids_of, states


def check_rows(ids_of):
    n = np.array([len(i) for i in ids_of])
    assert (n == 1).any() and (n >= 5).any() and any(60 in i for i in ids_of), 'the rows miss a mask case'
    return int((n == 1).sum()), int(n.max())


def dqn(out):
    rec = {}
    env, agent = gen_dqn.train_agent(DQN_SPEC, rec)
    out['uno_mlp'] = np.array(DQN_SPEC['mlp'], np.int32)
    for k, v in agent.q_estimator.qnet.state_dict().items():
        out['uno_sd_' + k] = v.cpu().numpy()
    assert np.abs(out['uno_sd_fc_layers.1.running_mean']).max() > 0, 'BatchNorm statistics are still the initial ones'
    obs, ids_of, states = observations(env, DQN_SPEC['seed'] + 1)
    pred = np.stack([agent.predict(s) for s in states])
    assert pred.shape == (ROWS, A) and np.array_equal(pred.astype(np.float32).astype(np.float64), pred)
    out['uno_obs'], out['uno_legal'], out['uno_predict'] = obs, masks(ids_of), pred.astype(np.float32)
    single, most = check_rows(ids_of)
    every = agent.q_estimator.predict_nograd(obs.astype(np.float32)).astype(np.float64)
    gaps = []
    for what, q in (('legal', pred), ('all-action', every)):
        top = np.sort(np.where(np.isfinite(q), q, -np.inf), axis=1)[:, ::-1]
        two = np.isfinite(top[:, 1])
        close = int((two & (top[:, 0] - top[:, 1] < 1e-4)).sum())
        assert close < ROWS / 100, '%d rows with a %s top-two gap under 1e-4' % (close, what)
        gaps.append((what, close, (top[:, 0] - top[:, 1])[two].min()))
    print('uno dqn: %d rows (%d single-legal, at most %d legal ids), |q| <= %.3f; %s'
          % (ROWS, single, most, np.abs(pred[np.isfinite(pred)]).max(),
             ', '.join('%s gap under 1e-4 on %d rows (smallest %.2e)' % g for g in gaps)))
    B = agent.batch_size
    done = np.asarray(rec['done_batch'])
    assert done.any() and not done.all()
    assert not np.array_equal(rec['q_values_next'], rec['q_values_next_target'])
    out['uno_train_state'] = np.asarray(rec['state_batch']).reshape(B, -1).astype(np.uint8)
    out['uno_train_action'] = np.asarray(rec['action_batch'], np.int64)
    out['uno_train_reward'] = np.asarray(rec['reward_batch'], np.float32)
    assert np.array_equal(out['uno_train_reward'].astype(np.float64), np.asarray(rec['reward_batch'], np.float64))
    out['uno_train_next_state'] = np.asarray(rec['next_state_batch']).reshape(B, -1).astype(np.uint8)
    assert np.array_equal(out['uno_train_state'], np.asarray(rec['state_batch']).reshape(B, -1))
    out['uno_train_done'] = done.astype(np.uint8)
    out['uno_train_next_legal'] = masks(rec['legal_actions_batch'])
    out['uno_train_q_next'] = np.asarray(rec['q_values_next'], np.float32)
    out['uno_train_q_next_target'] = np.asarray(rec['q_values_next_target'], np.float32)
    out['uno_train_best'] = np.asarray(rec['best_actions'], np.int64)
    out['uno_train_target'] = np.asarray(rec['target_batch'])
    out['uno_train_gamma'] = np.float64(agent.discount_factor)
    assert out['uno_train_state'].shape == (B, D) and out['uno_train_next_legal'].shape == (B, 8)
    assert out['uno_train_q_next'].shape == (B, A) and out['uno_train_target'].shape == (B,)
    print('uno train(): batch %d, %d terminal rows' % (B, int(done.sum())))


def nfsp(out):
    import torch
    from rlcard.utils.utils import remove_illegal
    rec = {}
    env, agent = gen_nfsp.train_agent(NFSP_SPEC, rec)
    out['uno_mlp'] = np.array(NFSP_SPEC['mlp'], np.int32)
    for k, v in agent.policy_network.state_dict().items():
        out['uno_sd_' + k] = v.cpu().numpy()
    assert np.abs(out['uno_sd_mlp.1.running_mean']).max() > 0, 'BatchNorm statistics are still the initial ones'
    obs, ids_of, states = observations(env, NFSP_SPEC['seed'] + 1)
    probs = np.stack([agent._act(s['obs']) for s in states])
    assert probs.dtype == np.float32 and probs.shape == (ROWS, A)
    out['uno_obs'], out['uno_legal'] = obs, masks(ids_of)
    out['uno_probs'] = probs
    out['uno_legal_probs'] = np.stack([remove_illegal(p, ids) for p, ids in zip(probs, ids_of)]).astype(np.float64)
    single, most = check_rows(ids_of)
    with torch.no_grad():
        logits = agent.policy_network.mlp(torch.from_numpy(obs).float()).numpy().astype(np.float64)
    mask = np.unpackbits(out['uno_legal'], axis=1, bitorder='little')[:, :A].astype(bool)
    below = (logits.max(axis=1, keepdims=True) - logits)
    best = np.where(mask, below, np.inf).min(axis=1)       # the best legal logit, below the row's maximum
    hazard = int(((best >= 86) & (best <= 106)).sum())
    gone = int((best >= 106).sum())
    assert hazard <= ROWS * 5 // 100, '%d hazard rows' % hazard
    assert gone >= 1, 'no row whose legal mass underflows'
    print('uno nfsp: %d rows (%d single-legal, at most %d legal ids), logits spread %.0f, %d hazard rows, %d rows whose '
          'legal mass underflows' % (ROWS, single, most, below.max(), hazard, gone))
    states_sl = rec['info_states'].numpy().reshape(32, -1)
    ap = rec['eval_action_probs'].numpy()
    assert np.array_equal(states_sl, states_sl.astype(np.uint8)) and states_sl.shape == (32, D)
    assert ap.shape == (32, A) and np.all((ap == 0) | (ap == 1)) and np.all(ap.sum(axis=1) == 1), 'not one-hot'
    out['uno_sl_info_states'] = states_sl.astype(np.uint8)
    out['uno_sl_action_probs'] = ap.astype(np.float32)
    out['uno_sl_loss'] = np.float64(rec['ce_loss'])
    for k, v in rec['pre'].items():
        out['uno_slpre_' + k] = v.cpu().numpy()


def main():
    gen_golden.setup_reference()
    for name, fill in (('dqn_uno.npz', dqn), ('nfsp_uno.npz', nfsp)):
        out = {}
        fill(out)
        path = os.path.join(OUT, name)
        np.savez_compressed(path, **out)
        size = os.path.getsize(path)
        assert size < 400 * 1000, '%s: %d bytes' % (name, size)
        print('%s: %d arrays, %d bytes' % (name, len(out), size))


if __name__ == '__main__':
    main()
