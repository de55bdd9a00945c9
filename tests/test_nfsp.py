"""NFSPAgent on the host (rlcard_amd/agents/nfsp_agent.py) against the reference's recorded numbers
(tests/golden/nfsp.npz, written by tests/golden/gen_nfsp.py from rlcard/agents/nfsp_agent.py): the average-policy
network's layout and forward, the BatchNorm folding the device kernels rely on, the recorded train_sl loss, and the
one-state-at-a-time API. No GPU."""
import os

import numpy as np
import pytest

from test_dqn import legal_ids, state_of as dqn_state_of

torch = pytest.importorskip('torch')

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'nfsp.npz')
GAMES = ['leduc', 'limit']


@pytest.fixture(scope='module')
def gold():
    return dict(np.load(GOLDEN, allow_pickle=False))


def state_dict_of(gold, game, pre='_sd_'):
    pre = game + pre
    return {k[len(pre):]: torch.from_numpy(v) for k, v in gold.items() if k.startswith(pre)}


def network_of(gold, game, device='cpu'):
    from rlcard_amd.agents import AveragePolicyNetwork
    obs_dim = gold[game + '_obs'].shape[1]
    net = AveragePolicyNetwork(num_actions=4, state_shape=[obs_dim],
                               mlp_layers=[int(w) for w in gold[game + '_mlp']] + [4]).to(torch.device(device))
    net.load_state_dict(state_dict_of(gold, game))
    net.eval()
    return net


def state_of(gold, game, r):
    return dqn_state_of(gold, game, r)      # (the same array names: G_obs, G_legal)


def mask_of(legal, A=4):
    return np.unpackbits(np.asarray(legal, np.uint8), axis=1, bitorder='little')[:, :A].astype(bool)


def logits64(wb, x):
    """fp64 forward of a Linear/ReLU stack [(W, b)] on rows x -> the logits."""
    h = np.asarray(x, np.float64)
    for k, (W, b) in enumerate(wb):
        h = h @ np.asarray(W, np.float64).T + np.asarray(b, np.float64)
        if k < len(wb) - 1:
            h = np.maximum(h, 0.0)
    return h


def unfolded_logits64(net, x):
    """fp64 logits of the eval-mode network as torch defines it: BatchNorm with the running statistics, then the
    Linear/ReLU stack."""
    sd = {k: v.detach().cpu().numpy().astype(np.float64) for k, v in net.state_dict().items()}
    h = (np.asarray(x, np.float64) - sd['mlp.1.running_mean']) / np.sqrt(sd['mlp.1.running_var'] + net.mlp[1].eps)
    h = h * sd['mlp.1.weight'] + sd['mlp.1.bias']
    idx = sorted({int(k.split('.')[1]) for k in sd if k.endswith('.weight')} - {1})
    return logits64([(sd['mlp.%d.weight' % i], sd['mlp.%d.bias' % i]) for i in idx], h)


def probs64(logits, mask):
    """The reference chain in fp64: exp(log_softmax) over every action, then remove_illegal (uniform over the legal
    actions where their mass is 0)."""
    z = logits - logits.max(axis=1, keepdims=True)
    p = np.exp(z)
    p = p / p.sum(axis=1, keepdims=True)
    p = np.where(mask, p, 0.0)
    s = p.sum(axis=1, keepdims=True)
    uni = mask / np.maximum(mask.sum(axis=1, keepdims=True), 1)
    with np.errstate(invalid='ignore', divide='ignore'):
        return np.where(s == 0, uni, p / s)


@pytest.mark.parametrize('game', GAMES)
def test_reference_state_dict_loads_and_forward_matches(gold, game):
    from rlcard_amd.utils import remove_illegal
    net = network_of(gold, game)
    keys = set(net.state_dict().keys())
    assert keys == set(state_dict_of(gold, game).keys())
    assert {'mlp.1.running_mean', 'mlp.2.weight', 'mlp.4.bias'} <= keys
    assert np.abs(gold[game + '_sd_mlp.1.running_mean']).max() > 0
    with torch.no_grad():
        logp = net(torch.from_numpy(gold[game + '_obs']).float()).numpy()
    p = np.exp(logp)
    np.testing.assert_allclose(p, gold[game + '_probs'], rtol=1e-5, atol=1e-7)
    np.testing.assert_allclose(p.sum(axis=1), 1.0, atol=1e-5)
    want = gold[game + '_legal_probs']
    m = mask_of(gold[game + '_legal'])
    assert np.all(want[~m] == 0) and np.abs(want.sum(axis=1) - 1).max() < 1e-12
    for r in range(len(p)):
        got = remove_illegal(gold[game + '_probs'][r], legal_ids(gold[game + '_legal'][r]))
        assert np.array_equal(got, want[r])


@pytest.mark.parametrize('game', GAMES)
def test_folded_network_equals_unfolded_in_fp64(gold, game):
    net = network_of(gold, game)
    x = gold[game + '_obs']
    a, b = logits64(net.folded_weights(), x), unfolded_logits64(net, x)
    assert np.abs(a - b).max() <= 1e-11 * max(1.0, np.abs(b).max())
    # the fp64 chain on these logits is the reference's recorded rows, to the fp32 forward's error
    np.testing.assert_allclose(probs64(b, mask_of(gold[game + '_legal'])), gold[game + '_legal_probs'], rtol=2e-4,
                               atol=1e-7)
    # the descriptor holds the same weights in fp32, and is cached until the parameters change
    d = net.folded()
    assert d is net.folded()
    assert (d.in_dim, d.num_hidden, d.num_actions) == (x.shape[1], len(gold[game + '_mlp']), 4)
    assert list(d.hidden[:d.num_hidden]) == [int(w) for w in gold[game + '_mlp']]
    for k, (W, bias) in enumerate(net.folded_weights()):
        assert np.array_equal(d.tensors[2 * k].numpy(), W.astype(np.float32))
        assert d.W[k] == d.tensors[2 * k].data_ptr() and d.b[k] == d.tensors[2 * k + 1].data_ptr()
    with torch.no_grad():
        net.mlp[2].bias.add_(1.0)
    d2 = net.folded()
    assert d2 is not d
    net.load_state_dict(state_dict_of(gold, game))
    assert net.folded() is not d2


def new_agent(gold, **kw):
    from rlcard_amd.agents import NFSPAgent
    args = dict(num_actions=4, state_shape=[36], hidden_layers_sizes=[64, 64], q_mlp_layers=[64, 64], batch_size=32,
                min_buffer_size_to_learn=32, q_replay_memory_init_size=8, q_batch_size=4, anticipatory_param=0.5,
                device=torch.device('cpu'))
    args.update(kw)
    agent = NFSPAgent(**args)
    agent.policy_network.load_state_dict(state_dict_of(gold, 'leduc'))
    return agent


def test_recorded_train_sl_loss(gold):
    """The loss of the recorded batch under the weights the reference's train_sl call found is the recorded loss, and
    train_sl on that batch takes a step and invalidates the descriptor."""
    agent = new_agent(gold)
    agent.policy_network.load_state_dict(state_dict_of(gold, 'leduc', '_slpre_'))
    states = torch.from_numpy(gold['leduc_sl_info_states']).float()
    ap = torch.from_numpy(gold['leduc_sl_action_probs'])
    assert np.all(ap.numpy().sum(axis=1) == 1) and np.all((ap.numpy() == 0) | (ap.numpy() == 1))
    agent.policy_network.train()
    with torch.no_grad():
        loss = float(agent.sl_loss(states, ap))
    agent.policy_network.eval()
    want = float(gold['leduc_sl_loss'])
    # fp32 rounding: the same torch operations, whose sums (64-term dot products, the batch statistics, the mean of
    # 32 rows) may run in another order on another CPU -- 32 ulp of the loss
    assert abs(loss - want) <= 32 * 2.0 ** -24 * max(1.0, abs(want))
    from rlcard_amd.agents.nfsp_agent import Transition
    for s, p in zip(gold['leduc_sl_info_states'], gold['leduc_sl_action_probs']):
        agent._reservoir_buffer.add(Transition(s.astype(np.float64), p.astype(np.float64)))
    d = agent.policy_network.folded()
    before = [p.detach().clone() for p in agent.policy_network.parameters()]
    got = agent.train_sl()       # the whole buffer is the batch, in another order: the same loss up to the sum's order
    assert abs(got - want) <= 1e-5 and agent.train_t == 1 and agent.last_loss == got
    assert any(not torch.equal(a, b) for a, b in zip(before, agent.policy_network.parameters()))
    assert agent.policy_network.folded() is not d and not agent.policy_network.training


def test_host_api_step_eval_feed(gold):
    agent = new_agent(gold)
    assert agent.use_raw is False and agent._mode in ('best_response', 'average_policy')
    want = gold['leduc_legal_probs']
    np.random.seed(3)
    agent._mode = 'average_policy'
    counts = np.zeros(4)
    for r in range(64):
        st = state_of(gold, 'leduc', r)
        a, info = agent.eval_step(st)
        assert a in st['legal_actions'] and list(info['probs'].keys()) == st['raw_legal_actions']
        ids = list(st['legal_actions'])
        np.testing.assert_allclose([info['probs'][k] for k in st['raw_legal_actions']], want[r][ids], rtol=1e-4,
                                   atol=1e-7)
        assert agent.step(st) in st['legal_actions']
        counts[a] += 1
    assert len(agent._reservoir_buffer) == 0            # average_policy steps store nothing
    agent._mode = 'best_response'
    for r in range(40):
        st = state_of(gold, 'leduc', r)
        a = agent.step(st)
        assert a in st['legal_actions']
        t = agent._reservoir_buffer._data[-1]
        assert np.array_equal(t.info_state, st['obs']) and t.action_probs[a] == 1 and t.action_probs.sum() == 1
    assert len(agent._reservoir_buffer) == 40
    agent.evaluate_with = 'best_response'
    a, info = agent.eval_step(state_of(gold, 'leduc', 0))
    assert 'values' in info
    agent.evaluate_with = 'nonsense'
    with pytest.raises(ValueError):
        agent.eval_step(state_of(gold, 'leduc', 0))
    # feed: the inner DQN takes every transition; train_sl runs once the buffer holds min_buffer_size_to_learn
    for k in range(12):
        s, s2 = state_of(gold, 'leduc', k), state_of(gold, 'leduc', k + 1)
        agent.feed([s, int(list(s['legal_actions'])[0]), 0.0, s2, k % 3 == 2])
    assert agent.total_t == 12 == agent._rl_agent.total_t and agent.train_t == 12
    assert agent._rl_agent.train_t == 12 - 8 + 1 and np.isfinite(agent.last_loss)
    small = new_agent(gold, min_buffer_size_to_learn=100)
    for k in range(5):
        s, s2 = state_of(gold, 'leduc', k), state_of(gold, 'leduc', k + 1)
        small.feed([s, int(list(s['legal_actions'])[0]), 0.0, s2, False])
    assert small.total_t == 5 and small.train_t == 0 and small.train_sl() is None
    assert small.sl_steps_for(0, 12) == 12 and new_agent(gold, train_every=5).sl_steps_for(3, 21) == 4


def test_sample_episode_policy_rate(gold):
    agent = new_agent(gold, anticipatory_param=0.25)
    np.random.seed(11)
    n = 0
    for _ in range(4000):
        agent.sample_episode_policy()
        n += agent._mode == 'best_response'
    assert abs(n - 1000) < 5 * np.sqrt(4000 * 0.25 * 0.75)


def test_reservoir_buffer_keeps_its_capacity():
    from rlcard_amd.agents import ReservoirBuffer
    np.random.seed(7)
    buf = ReservoirBuffer(50)
    for k in range(2000):
        buf.add(k)
        assert len(buf) == min(k + 1, 50)
    assert buf._add_calls == 2000 and len(set(buf)) == 50
    assert max(buf) >= 50 and np.mean(list(buf)) > 500       # later elements do replace earlier ones, uniformly
    assert len(buf.sample(20)) == 20
    with pytest.raises(ValueError):
        buf.sample(51)
    back = ReservoirBuffer.from_checkpoint(buf.checkpoint_attributes())
    assert list(back) == list(buf) and back._add_calls == 2000
    buf.clear()
    assert len(buf) == 0 and buf._add_calls == 0


def test_checkpoint_round_trip_restores_the_inner_dqn(gold, tmp_path):
    from rlcard_amd.agents import NFSPAgent
    agent = new_agent(gold)
    agent._mode = 'best_response'
    np.random.seed(2)
    for k in range(36):
        s, s2 = state_of(gold, 'leduc', k), state_of(gold, 'leduc', k + 1)
        agent.feed([s, agent.step(s), 0.0, s2, False])
    assert agent.train_t > 0 and agent._rl_agent.train_t > 0
    attrs = agent.checkpoint_attributes()
    assert set(attrs) == {'agent_type', 'policy_network', 'reservoir_buffer', 'rl_agent', 'policy_network_optimizer',
                          'device', 'anticipatory_param', 'batch_size', 'min_buffer_size_to_learn', 'num_actions',
                          'mode', 'evaluate_with', 'total_t', 'train_t', 'sl_learning_rate', 'train_every'}
    assert attrs['agent_type'] == 'NFSPAgent' and attrs['rl_agent']['agent_type'] == 'DQNAgent'
    assert set(attrs['policy_network']) == {'num_actions', 'state_shape', 'mlp_layers', 'mlp'}
    agent.save_checkpoint(str(tmp_path))
    back = NFSPAgent.from_checkpoint(torch.load(os.path.join(str(tmp_path), 'checkpoint_nfsp.pt'),
                                                weights_only=False))
    assert (back.total_t, back.train_t, back._mode) == (agent.total_t, agent.train_t, 'best_response')
    assert len(back._reservoir_buffer) == len(agent._reservoir_buffer) == 36
    # the inner DQN is the saved one, not a fresh one: counters, memory and Q-values
    assert (back._rl_agent.total_t, back._rl_agent.train_t) == (agent._rl_agent.total_t, agent._rl_agent.train_t)
    assert len(back._rl_agent.memory) == len(agent._rl_agent.memory) == 36
    st = state_of(gold, 'leduc', 50)
    assert np.array_equal(back._rl_agent.predict(st), agent._rl_agent.predict(st))
    assert np.array_equal(back._act(st['obs']), agent._act(st['obs']))
