"""DQNAgent and NFSPAgent on UNO, on the host, against the reference's recorded numbers (tests/golden/dqn_uno.npz and
nfsp_uno.npz, written by tests/golden/gen_qnet_uno.py from rlcard/agents/dqn_agent.py and nfsp_agent.py on
rlcard/envs/uno.py): 240 obs bytes, 61 actions, legal masks of 8 bytes. The fixtures' shapes, the networks' forwards, the
descriptor the device kernels take, and the one-state-at-a-time API on the recorded states (make('uno') itself opens
the engine's device: tests/test_gpu_uno_agents.py). No GPU."""
import os
from collections import OrderedDict

import numpy as np
import pytest

from test_dqn import legal_ids, state_dict_of
from test_nfsp import mask_of, state_dict_of as policy_state_dict_of

torch = pytest.importorskip('torch')

HERE = os.path.dirname(os.path.abspath(__file__))
GOLDEN_DQN = os.path.join(HERE, 'golden', 'dqn_uno.npz')
GOLDEN_NFSP = os.path.join(HERE, 'golden', 'nfsp_uno.npz')
A, D, LB, ROWS = 61, 240, 8, 256


@pytest.fixture(scope='module')
def gold():
    return dict(np.load(GOLDEN_DQN, allow_pickle=False))


@pytest.fixture(scope='module')
def gold_nfsp():
    return dict(np.load(GOLDEN_NFSP, allow_pickle=False))


def uno_estimator(gold, device='cpu'):
    from rlcard_amd.agents import Estimator
    est = Estimator(num_actions=A, state_shape=[D], mlp_layers=[int(w) for w in gold['uno_mlp']],
                    device=torch.device(device))
    est.load_state_dict(state_dict_of(gold, 'uno'))
    return est


def uno_policy_net(gold_nfsp):
    from rlcard_amd.agents import AveragePolicyNetwork
    net = AveragePolicyNetwork(num_actions=A, state_shape=[D], mlp_layers=[int(w) for w in gold_nfsp['uno_mlp']] + [A])
    net.load_state_dict(policy_state_dict_of(gold_nfsp, 'uno'))
    net.eval()
    return net


def uno_state(g, r):
    ids = legal_ids(g['uno_legal'][r])
    return {'obs': g['uno_obs'][r].astype(np.float64).reshape(4, 4, 15),
            'legal_actions': OrderedDict((a, None) for a in ids), 'raw_legal_actions': ['a%d' % a for a in ids]}


def test_fixtures_have_the_promised_shapes(gold, gold_nfsp):
    for g in (gold, gold_nfsp):
        assert g['uno_obs'].shape == (ROWS, D) and g['uno_obs'].dtype == np.uint8
        assert g['uno_legal'].shape == (ROWS, LB) and g['uno_legal'].dtype == np.uint8
        assert list(g['uno_mlp']) == [64, 64]
        m = mask_of(g['uno_legal'], 64)
        assert not m[:, A:].any() and m.any(axis=1).all()
        n = m.sum(axis=1)
        assert (n == 1).any() and (n >= 5).any() and m[:, 60].any()      # the generator's mask cases
    assert gold['uno_predict'].shape == (ROWS, A) and gold['uno_predict'].dtype == np.float32
    assert gold_nfsp['uno_probs'].shape == (ROWS, A) and gold_nfsp['uno_probs'].dtype == np.float32
    assert gold_nfsp['uno_legal_probs'].shape == (ROWS, A) and gold_nfsp['uno_legal_probs'].dtype == np.float64
    B = len(gold['uno_train_action'])
    assert B == 32
    for k, shape in (('state', (B, D)), ('next_state', (B, D)), ('next_legal', (B, LB)), ('q_next', (B, A)),
                     ('q_next_target', (B, A)), ('best', (B,)), ('target', (B,)), ('reward', (B,)), ('done', (B,))):
        assert gold['uno_train_' + k].shape == shape, k
    assert gold['uno_train_next_legal'].dtype == np.uint8
    assert gold_nfsp['uno_sl_info_states'].shape == (32, D) and gold_nfsp['uno_sl_action_probs'].shape == (32, A)
    assert np.abs(gold['uno_sd_fc_layers.1.running_mean']).max() > 0
    assert np.abs(gold_nfsp['uno_sd_mlp.1.running_mean']).max() > 0


def test_recorded_train_call_is_the_documented_target_line(gold):
    g = gold
    done = g['uno_train_done'].astype(bool)
    qn, qt = g['uno_train_q_next'], g['uno_train_q_next_target']
    masked = np.full(qn.shape, -np.inf)
    for k, m in enumerate(g['uno_train_next_legal']):
        ids = legal_ids(m)
        masked[k, ids] = qn[k, ids]
    best = np.argmax(masked, axis=1)
    assert np.array_equal(best, g['uno_train_best']) and best.max() > 8
    target = g['uno_train_reward'].astype(np.float64) + np.invert(done).astype(np.float32) * \
        float(g['uno_train_gamma']) * qt[np.arange(len(best)), best]
    assert np.array_equal(target, g['uno_train_target'])


def test_dqn_forward_and_host_api_reproduce_the_recorded_rows(gold):
    """tests/test_dqn.py's tolerances for Leduc: rtol = atol = 1e-5 on the legal entries, -inf exactly elsewhere."""
    from rlcard_amd.agents import DQNAgent
    est = uno_estimator(gold)
    want = gold['uno_predict']
    legal = np.isfinite(want)
    assert np.array_equal(legal, mask_of(gold['uno_legal'], A)) and np.all(want[~legal] == -np.inf)
    q = est.predict_nograd(gold['uno_obs'].astype(np.float64))
    np.testing.assert_allclose(q[legal], want[legal], rtol=1e-5, atol=1e-5)
    net = est.folded()
    assert (net.in_dim, net.num_hidden, net.num_actions) == (D, 2, A)
    assert list(net.hidden[:2]) == [64, 64]
    agent = DQNAgent(num_actions=A, state_shape=[4, 4, 15], mlp_layers=[64, 64], device=torch.device('cpu'))
    agent.q_estimator.load_state_dict(state_dict_of(gold, 'uno'))
    np.random.seed(5)
    for r in range(0, ROWS, 4):
        st = uno_state(gold, r)
        p = agent.predict(st)
        assert p.shape == (A,) and np.array_equal(np.isfinite(p), legal[r])
        np.testing.assert_allclose(p[legal[r]], want[r][legal[r]], rtol=1e-5, atol=1e-5)
        a, info = agent.eval_step(st)
        top = np.sort(want[r])
        assert a == int(np.argmax(want[r])) or top[-1] - top[-2] < 1e-4
        assert list(info['values'].keys()) == st['raw_legal_actions']
        assert agent.step(st) in st['legal_actions']


def test_nfsp_forward_and_host_api_reproduce_the_recorded_rows(gold_nfsp):
    """tests/test_nfsp.py's tolerances for Leduc: rtol 1e-5 / atol 1e-7 on np.exp(log_softmax), remove_illegal bit for
    bit on the recorded probabilities, rtol 1e-4 / atol 1e-7 through the agent."""
    from rlcard_amd.agents import NFSPAgent
    from rlcard_amd.utils import remove_illegal
    g = gold_nfsp
    net = uno_policy_net(g)
    agent = NFSPAgent(num_actions=A, state_shape=[4, 4, 15], hidden_layers_sizes=[64, 64], q_mlp_layers=[64, 64],
                      device=torch.device('cpu'))
    agent.policy_network.load_state_dict(policy_state_dict_of(g, 'uno'))
    # a state at a time, as the reference recorded them (NFSPAgent._act): the logits spread over 470, where one ulp of
    # a logit is 3e-5 of its probability, so a batched forward's other summation order alone can pass rtol 1e-5
    p = np.stack([agent._act(g['uno_obs'][r].astype(np.float64).reshape(4, 4, 15)) for r in range(ROWS)])
    np.testing.assert_allclose(p, g['uno_probs'], rtol=1e-5, atol=1e-7)
    want = g['uno_legal_probs']
    m = mask_of(g['uno_legal'], A)
    assert np.all(want[~m] == 0) and np.abs(want.sum(axis=1) - 1).max() < 1e-12
    for r in range(ROWS):
        assert np.array_equal(remove_illegal(g['uno_probs'][r], legal_ids(g['uno_legal'][r])), want[r])
    d = net.folded()
    assert (d.in_dim, d.num_hidden, d.num_actions) == (D, 2, A)
    agent._mode = 'average_policy'
    np.random.seed(3)
    for r in range(0, ROWS, 4):
        st = uno_state(g, r)
        a, info = agent.eval_step(st)
        ids = list(st['legal_actions'])
        assert a in ids and list(info['probs'].keys()) == st['raw_legal_actions']
        np.testing.assert_allclose([info['probs'][k] for k in st['raw_legal_actions']], want[r][ids], rtol=1e-4,
                                   atol=1e-7)
        assert agent.step(st) in ids

