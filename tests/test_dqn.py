"""DQNAgent on the host (rlcard_amd/agents/dqn_agent.py) against the reference's recorded numbers
(tests/golden/dqn.npz, written by tests/golden/gen_dqn.py from rlcard/agents/dqn_agent.py): the network layout and its
forward, the BatchNorm folding the device kernels rely on, and the one-state-at-a-time API. No GPU."""
import os
from collections import OrderedDict

import numpy as np
import pytest

torch = pytest.importorskip('torch')

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'dqn.npz')
ACTIONS = ['call', 'raise', 'fold', 'check']
GAMES = ['leduc', 'limit']


@pytest.fixture(scope='module')
def gold():
    return dict(np.load(GOLDEN, allow_pickle=False))


def state_dict_of(gold, game):
    pre = game + '_sd_'
    return {k[len(pre):]: torch.from_numpy(v) for k, v in gold.items() if k.startswith(pre)}


def estimator_of(gold, game, device='cpu'):
    from rlcard_amd.agents import Estimator
    obs_dim = gold[game + '_obs'].shape[1]
    est = Estimator(num_actions=4, state_shape=[obs_dim], mlp_layers=[int(w) for w in gold[game + '_mlp']],
                    device=torch.device(device))
    est.load_state_dict(state_dict_of(gold, game))
    return est


def legal_ids(mask_row):
    return [a for a in range(8 * len(mask_row)) if (int(mask_row[a // 8]) >> (a % 8)) & 1]


def state_of(gold, game, r):
    ids = legal_ids(gold[game + '_legal'][r])
    return {'obs': gold[game + '_obs'][r].astype(np.float64), 'legal_actions': OrderedDict((a, None) for a in ids),
            'raw_legal_actions': [ACTIONS[a] for a in ids]}


def forward64(wb, x):
    """fp64 forward of a Linear/tanh stack [(W, b)] on rows x."""
    h = np.asarray(x, np.float64)
    for k, (W, b) in enumerate(wb):
        h = h @ np.asarray(W, np.float64).T + np.asarray(b, np.float64)
        if k < len(wb) - 1:
            h = np.tanh(h)
    return h


def unfolded64(est, x):
    """fp64 forward of the eval-mode network as torch defines it: BatchNorm with the running statistics, then the
    Linear/tanh stack."""
    sd = {k: v.detach().cpu().numpy().astype(np.float64) for k, v in est.qnet.state_dict().items()}
    eps = est.qnet.fc_layers[1].eps
    h = (np.asarray(x, np.float64) - sd['fc_layers.1.running_mean']) / np.sqrt(sd['fc_layers.1.running_var'] + eps)
    h = h * sd['fc_layers.1.weight'] + sd['fc_layers.1.bias']
    idx = sorted({int(k.split('.')[1]) for k in sd if k.endswith('.weight')} - {1})
    return forward64([(sd['fc_layers.%d.weight' % i], sd['fc_layers.%d.bias' % i]) for i in idx], h)


@pytest.mark.parametrize('game', GAMES)
def test_reference_state_dict_loads_and_forward_matches_predict(gold, game):
    est = estimator_of(gold, game)
    keys = set(est.qnet.state_dict().keys())
    assert keys == set(state_dict_of(gold, game).keys())
    assert {'fc_layers.1.running_mean', 'fc_layers.2.weight', 'fc_layers.4.bias'} <= keys
    q = est.predict_nograd(gold[game + '_obs'].astype(np.float64))
    want = gold[game + '_predict']
    legal = np.isfinite(want)
    mask = np.array([[(int(m[0]) >> a) & 1 for a in range(4)] for m in gold[game + '_legal']], bool)
    assert np.array_equal(legal, mask)                      # -inf exactly where the action is illegal
    assert np.all(want[~legal] == -np.inf)
    np.testing.assert_allclose(q[legal], want[legal], rtol=1e-5, atol=1e-5)


@pytest.mark.parametrize('game', GAMES)
def test_folded_network_equals_unfolded_in_fp64(gold, game):
    est = estimator_of(gold, game)
    x = gold[game + '_obs']
    a, b = forward64(est.folded_weights(), x), unfolded64(est, x)
    assert np.abs(a - b).max() <= 1e-12
    # the descriptor holds the same weights in fp32, and is cached until the parameters change
    net = est.folded()
    assert net is est.folded()
    assert (net.in_dim, net.num_hidden, net.num_actions) == (x.shape[1], len(gold[game + '_mlp']), 4)
    assert list(net.hidden[:net.num_hidden]) == [int(w) for w in gold[game + '_mlp']]
    for k, (W, bias) in enumerate(est.folded_weights()):
        assert np.array_equal(net.tensors[2 * k].numpy(), W.astype(np.float32))
        assert net.W[k] == net.tensors[2 * k].data_ptr() and net.b[k] == net.tensors[2 * k + 1].data_ptr()
    est.update(x[:8].astype(np.float32), np.zeros(8, np.int64), np.zeros(8, np.float32))
    assert est.folded() is not net
    net2 = est.folded()
    est.load_state_dict(state_dict_of(gold, game))
    assert est.folded() is not net2


def new_agent(gold, **kw):
    from rlcard_amd.agents import DQNAgent
    args = dict(num_actions=4, state_shape=[36], mlp_layers=[64, 64], replay_memory_init_size=8, batch_size=4,
                update_target_estimator_every=3, device=torch.device('cpu'))
    args.update(kw)
    agent = DQNAgent(**args)
    agent.q_estimator.load_state_dict(state_dict_of(gold, 'leduc'))
    return agent


def test_host_api_step_eval_predict(gold):
    agent = new_agent(gold)
    assert agent.use_raw is False
    want = gold['leduc_predict']
    np.random.seed(5)
    for r in range(0, 64):
        st = state_of(gold, 'leduc', r)
        q = agent.predict(st)
        assert q.shape == (4,) and q.dtype == np.float64
        assert np.array_equal(np.isfinite(q), np.isfinite(want[r]))
        np.testing.assert_allclose(q[np.isfinite(q)], want[r][np.isfinite(want[r])], rtol=1e-5, atol=1e-5)
        a, info = agent.eval_step(st)
        assert a == int(np.argmax(want[r])) or np.sort(want[r])[-1] - np.sort(want[r])[-2] < 1e-4
        assert list(info['values'].keys()) == st['raw_legal_actions']
        assert all(np.isfinite(v) for v in info['values'].values())
        assert agent.step(st) in st['legal_actions']
    # epsilon 0 at the end of the schedule: step is the greedy action
    agent.total_t = agent.epsilon_decay_steps
    agent.epsilons[-1] = 0.0
    for r in range(16):
        st = state_of(gold, 'leduc', r)
        assert agent.step(st) == agent.eval_step(st)[0]


def test_host_feed_bookkeeping_and_target_copy(gold):
    agent = new_agent(gold)
    n = len(gold['leduc_obs'])

    def same(a, b):
        return all(torch.equal(x, y) for x, y in zip(a.qnet.state_dict().values(), b.qnet.state_dict().values()))

    assert not same(agent.q_estimator, agent.target_estimator)
    copies = []
    for k in range(20):
        s, s2 = state_of(gold, 'leduc', k % n), state_of(gold, 'leduc', (k + 1) % n)
        before = agent.train_t
        agent.feed([s, int(list(s['legal_actions'])[0]), 0.5 * (k % 3 - 1), s2, k % 4 == 3])
        assert agent.total_t == k + 1
        assert len(agent.memory) == k + 1
        # the reference trains from total_t = replay_memory_init_size on, every train_every transitions
        assert agent.train_t == max(0, k + 1 - 8 + 1)
        if agent.train_t > before and before % 3 == 0:
            assert same(agent.q_estimator, agent.target_estimator)   # copied at train_t 0, 3, 6, ...
            copies.append(before)
        elif agent.train_t > before:
            assert not same(agent.q_estimator, agent.target_estimator)
    assert copies == [0, 3, 6, 9, 12]
    assert np.isfinite(agent.last_loss)
    small = new_agent(gold, replay_memory_size=5)
    for k in range(7):
        small.feed_memory(np.full(36, k), 0, 0.0, np.zeros(36), [0, 1], False)
    assert [int(t[0][0]) for t in small.memory.memory] == [2, 3, 4, 5, 6]      # FIFO
    assert agent.train_steps_for(0, 20) == 13 and agent.train_steps_for(7, 8) == 1 and agent.train_steps_for(0, 7) == 0
    e3 = new_agent(gold, train_every=3)
    assert e3.train_steps_for(0, 20) == len([t for t in range(1, 21) if t - 8 >= 0 and (t - 8) % 3 == 0])
    assert e3.train_steps_for(9, 14) == len([t for t in range(10, 15) if t - 8 >= 0 and (t - 8) % 3 == 0])


def test_checkpoint_round_trip(gold, tmp_path):
    from rlcard_amd.agents import DQNAgent
    agent = new_agent(gold)
    for k in range(12):
        s, s2 = state_of(gold, 'leduc', k), state_of(gold, 'leduc', k + 1)
        agent.feed([s, int(list(s['legal_actions'])[0]), 0.0, s2, False])
    attrs = agent.checkpoint_attributes()
    assert set(attrs) == {'agent_type', 'q_estimator', 'memory', 'total_t', 'train_t', 'replay_memory_init_size',
                          'update_target_estimator_every', 'discount_factor', 'epsilon_start', 'epsilon_end',
                          'epsilon_decay_steps', 'batch_size', 'num_actions', 'train_every', 'device', 'save_path',
                          'save_every'}
    assert attrs['agent_type'] == 'DQNAgent'
    assert set(attrs['q_estimator']) == {'qnet', 'optimizer', 'num_actions', 'learning_rate', 'state_shape',
                                         'mlp_layers', 'device'}
    assert set(attrs['memory']) == {'memory_size', 'batch_size', 'memory'}
    agent.save_checkpoint(str(tmp_path))
    back = DQNAgent.from_checkpoint(torch.load(os.path.join(str(tmp_path), 'checkpoint_dqn.pt'), weights_only=False))
    assert (back.total_t, back.train_t) == (agent.total_t, agent.train_t)
    assert len(back.memory) == len(agent.memory)
    st = state_of(gold, 'leduc', 40)
    assert np.array_equal(back.predict(st), agent.predict(st))
    # a checkpoint dict built from the reference's state_dict alone
    ck = dict(attrs, total_t=7, train_t=2, memory={'memory_size': 50, 'batch_size': 4, 'memory': []},
              q_estimator=dict(attrs['q_estimator'], qnet=state_dict_of(gold, 'leduc'), optimizer=None))
    ref = DQNAgent.from_checkpoint(ck)
    assert (ref.total_t, ref.train_t, ref.memory.memory_size) == (7, 2, 50)
    want = gold['leduc_predict'][40]
    q = ref.predict(st)
    np.testing.assert_allclose(q[np.isfinite(q)], want[np.isfinite(want)], rtol=1e-5, atol=1e-5)


def test_recorded_train_call_is_the_documented_target_line(gold):
    """The recorded train() call: best_actions and target_batch are the masked argmax and the numpy target line
    (float32 product, float64 sum) that DQNAgent.train and cs_dqn_targets restate."""
    g = gold
    done = g['leduc_train_done'].astype(bool)
    qn, qt = g['leduc_train_q_next'], g['leduc_train_q_next_target']
    masked = np.full(qn.shape, -np.inf)
    for k, m in enumerate(g['leduc_train_next_legal']):
        ids = legal_ids(m)
        masked[k, ids] = qn[k, ids]
    best = np.argmax(masked, axis=1)
    assert np.array_equal(best, g['leduc_train_best'])
    target = g['leduc_train_reward'].astype(np.float64) + np.invert(done).astype(np.float32) * \
        float(g['leduc_train_gamma']) * qt[np.arange(len(best)), best]
    assert np.array_equal(target, g['leduc_train_target'])
