"""The fused DQN learner's host side (rlcard_amd/agents/dqn_agent.py train_fused; kernel: rlcard_amd/csrc/
cs_dqn_train.hip): the numpy restatement of the kernel's batch sampler -- Floyd's algorithm on Philox draws, as
include/cardsim.h states it at cs_dqn_train -- with its own properties, and the refusals Python makes before any
launch. tests/test_gpu_dqn_train.py holds the kernel to this restatement."""
import numpy as np
import pytest

from test_gpu_nfsp import philox4

torch = pytest.importorskip('torch')

M32 = np.uint64(0xFFFFFFFF)


def floyd_batches(seed, train_ts, size, B):
    """The indices cs_dqn_train draws at the steps train_ts -> int64 [len(train_ts), B]. For i = 0 .. B-1: j = size - B
    + i, r = (x * (j + 1)) >> 64 with x = w[0] | w[1] << 32 of Philox keyed by seed on the counter (train_t, i); the
    i-th index is r, or j where r is already among the earlier ones."""
    assert B <= size < 2 ** 32
    ts = np.asarray(train_ts, np.uint64)
    out = np.zeros((len(ts), B), np.int64)
    for i in range(B):
        w = philox4(seed, ts, i)
        lo, hi = w[0].astype(np.uint64), w[1].astype(np.uint64)
        j = size - B + i
        m = np.uint64(j + 1)
        r = ((hi * m + ((lo * m) >> np.uint64(32))) >> np.uint64(32)).astype(np.int64)   # (x * m) >> 64, m < 2^32
        taken = (out[:, :i] == r[:, None]).any(axis=1)
        out[:, i] = np.where(taken, j, r)
    return out


def test_mulhi_restatement_is_exact():
    rng = np.random.RandomState(3)
    for _ in range(200):
        lo, hi, m = (int(v) for v in rng.randint(0, 2 ** 32, size=3, dtype=np.uint64))
        m = max(m, 1)
        x = lo | (hi << 32)
        got = (np.uint64(hi) * np.uint64(m) + ((np.uint64(lo) * np.uint64(m)) >> np.uint64(32))) >> np.uint64(32)
        assert int(got) == (x * m) >> 64


@pytest.mark.parametrize('size,B', [(7, 3), (64, 64), (100, 32), (5000, 32), (2, 2), (1 << 20, 64)])
def test_samples_are_distinct_and_in_range(size, B):
    got = floyd_batches(11, np.arange(300), size, B)
    assert got.min() >= 0 and got.max() < size
    assert all(len(set(row)) == B for row in got.tolist())
    # other steps, other batches; the same step, the same batch
    assert np.array_equal(got[:5], floyd_batches(11, np.arange(5), size, B))
    if size > B:
        assert len({tuple(row) for row in got.tolist()}) > 1
        assert not np.array_equal(got, floyd_batches(12, np.arange(300), size, B))


def test_a_full_memory_is_drawn_whole():
    for B in (2, 5, 32, 64):
        got = floyd_batches(0, np.arange(50), B, B)
        assert np.array_equal(np.sort(got, axis=1), np.tile(np.arange(B), (50, 1)))


def test_slots_are_drawn_uniformly():
    """20 000 batches of 3 from 7 slots: a slot is in a batch with probability 3/7, so its count is Binomial(20 000,
    3/7) with sigma = sqrt(20 000 * 3/7 * 4/7) = 69.99; every count within 4 sigma of 8571.4 (seed 0, the agent's
    default train_seed). Pairs too: each of the 21 pairs with probability 1/7, sigma 49.49."""
    got = floyd_batches(0, np.arange(20000), 7, 3)
    counts = np.bincount(got.reshape(-1), minlength=7)
    sigma = np.sqrt(20000 * (3 / 7) * (4 / 7))
    print('slot counts', counts, 'sigma %.2f' % sigma)
    assert np.all(np.abs(counts - 20000 * 3 / 7) <= 4 * sigma)
    pair = np.zeros((7, 7), np.int64)
    s = np.sort(got, axis=1)
    for a, b in ((0, 1), (0, 2), (1, 2)):
        np.add.at(pair, (s[:, a], s[:, b]), 1)
    pc = pair[np.triu_indices(7, 1)]
    assert np.all(np.abs(pc - 20000 / 7) <= 4 * np.sqrt(20000 * (1 / 7) * (6 / 7)))


def new_agent(**kw):
    from rlcard_amd.agents import DQNAgent
    torch.manual_seed(1)
    return DQNAgent(num_actions=4, state_shape=[36], mlp_layers=[8], batch_size=4, device=torch.device('cpu'), **kw)


def test_train_fused_needs_attach():
    from rlcard_amd import _abi
    agent = new_agent()
    assert agent.train_seed == 0
    with pytest.raises(_abi.CardsimError, match='attach'):
        agent.train_fused(1)
    with pytest.raises(_abi.CardsimError, match='attach'):
        agent.train_fused(1, debug=True)


@pytest.mark.parametrize('make', [
    lambda ps: torch.optim.SGD(ps, lr=0.1),
    lambda ps: torch.optim.AdamW(ps, lr=0.1),
    lambda ps: torch.optim.Adam(ps, lr=0.1, weight_decay=1e-4),
    lambda ps: torch.optim.Adam(ps, lr=0.1, amsgrad=True),
    lambda ps: torch.optim.Adam(ps, lr=0.1, maximize=True)], ids=['sgd', 'adamw', 'weight_decay', 'amsgrad', 'maximize'])
def test_train_fused_refuses_what_is_not_plain_adam(make):
    """The refusal comes before anything touches the env or the memory (stand-ins here: no GPU on this path)."""
    agent = new_agent()
    agent.vec, agent.device_memory = object(), object()
    agent.q_estimator.optimizer = make(agent.q_estimator.qnet.parameters())
    before = agent.train_t
    with pytest.raises(ValueError, match='Adam'):
        agent.train_fused(1)
    assert agent.train_t == before and len(agent.q_estimator.optimizer.state) == 0


def test_adam_state_is_created_as_torch_creates_it():
    """train_fused's state for a fresh optimizer is what Adam's own first step creates: step a CPU float scalar 0, the
    moments zeros like the parameters -- so optimizer.step() and state_dict() go on from it."""
    agent = new_agent()
    group, states = agent._adam_state()
    params = list(agent.q_estimator.qnet.parameters())
    assert len(states) == len(params) == 6 and group is agent.q_estimator.optimizer.param_groups[0]
    for p, st in zip(params, states):
        assert st['step'].device.type == 'cpu' and st['step'].dtype == torch.float32 and float(st['step']) == 0
        assert st['exp_avg'].shape == p.shape and not st['exp_avg'].any() and not st['exp_avg_sq'].any()
    twin = new_agent()
    x = torch.rand(4, 36)
    for a in (agent, twin):
        a.q_estimator.update(x, torch.zeros(4, dtype=torch.long), torch.ones(4))
    for p, q in zip(params, twin.q_estimator.qnet.parameters()):
        assert torch.equal(p, q)
    assert agent.q_estimator.optimizer.state_dict()['state'][0]['step'] == 1
