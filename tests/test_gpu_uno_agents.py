"""DQN and NFSP on UNO end to end on the device (rlcard_amd/agents on a VecEnv('uno', ...): 240 obs bytes, 61 actions,
8 mask bytes): the replay ring against the numpy restatement of reorganize, the Double-DQN targets against the
reference's recorded train() call (tests/golden/dqn_uno.npz) and numpy, the reservoir against the sequential add, the
collectors against 'random' and 'uno-rule-v1', tournament_vec with a network seat, and the one-state-at-a-time API on
make('uno'). The restatements are tests/test_gpu_dqn.py's and tests/test_gpu_nfsp.py's. Needs a GPU."""
import numpy as np
import pytest

from test_gpu_dqn import RefReplay, assert_same, held, ref_targets, run_targets
from test_gpu_nfsp import RefReservoir, assert_same_reservoir
from test_gpu_nfsp import held as held_reservoir
from test_qnet_uno import A, D, GOLDEN_DQN, LB

torch = pytest.importorskip('torch')
pytestmark = pytest.mark.gpu
N = 65      # a wave of envs and one more


@pytest.fixture(scope='module', autouse=True)
def _need_gpu():
    if not torch.cuda.is_available():
        pytest.fail('GPU tests need a visible GPU (run them on the MI355X box)')


@pytest.fixture(scope='module')
def gold():
    return dict(np.load(GOLDEN_DQN, allow_pickle=False))


def test_replay_matches_reorganize_on_uno():
    from rlcard_amd import VecEnv
    from rlcard_amd.agents import DeviceMemory
    v = VecEnv('uno', N, seed=21)
    v.reset()
    caps = (1 << 15, 500)
    mems = [DeviceMemory(v, cap) for cap in caps]
    ref = RefReplay(2, D, LB)
    tr = v.new_traj_out(96, final_obs=True, select=1)
    carried = []
    for w in range(2):
        v.rollout(96, policy_seed=3, t0=96 * w, out=tr)
        for mem in mems:
            mem.push(tr, (0, 1))
        ref.push({k: x.cpu().numpy() for k, x in tr.items()}, (0, 1))
        carried.append(len(ref.pending))
        for mem, cap in zip(mems, caps):
            assert mem.sizes() == (min(len(ref.out), cap), len(ref.out))
    assert carried[0] > 0                                       # transitions straddle the window edge ...
    want = ref.held(caps[0])
    assert want['done'].any() and not want['done'].all()        # ... and games finished inside the windows
    assert want['next_legal'].shape[1] == LB and (want['next_legal'][:, 7] != 0).any()      # (draw, id 60)
    assert np.all(want['next_legal'][want['done'] == 1] == 0)
    for mem, cap in zip(mems, caps):
        assert_same(held(mem), ref.held(cap), 'capacity %d' % cap)


def test_targets_recorded_uno_batch(gold):
    g = gold
    gamma = float(g['uno_train_gamma'])
    args = (g['uno_train_q_next'], g['uno_train_q_next_target'], g['uno_train_next_legal'], g['uno_train_reward'],
            g['uno_train_done'])
    target, best = run_targets(*args, gamma)
    assert np.array_equal(best, g['uno_train_best'])
    assert np.array_equal(target.view(np.int32), g['uno_train_target'].astype(np.float32).view(np.int32))
    want, wbest = ref_targets(*args, gamma, A)
    assert np.array_equal(wbest, best) and np.array_equal(want.view(np.int32), target.view(np.int32))


def test_targets_random_wide_rows():
    rng = np.random.RandomState(12)
    B = 1000
    m = rng.rand(B, A) < 0.1
    m[::50] = False                                           # no legal action: best 0
    dn = (rng.rand(B) < 0.3).astype(np.uint8)
    m[dn == 1] = False                                        # terminal rows carry an empty mask
    m[7] = True
    nl = np.packbits(np.pad(m, ((0, 0), (0, 8 * LB - A))), axis=1, bitorder='little')
    nl[::7, 7] |= 0xE0                                        # bits 61..63 are no actions
    assert nl.shape == (B, LB)
    qn = np.where(m, rng.randn(B, A), -np.inf).astype(np.float32)
    qn[7] = qn[7, 0]                                          # ties: the first maximum
    qt = (rng.randn(B, A) * 3).astype(np.float32)
    rw = (rng.randint(-8, 9, size=B) * 0.5).astype(np.float32)
    rw[3] = 0.1                # (rewards on non-terminal rows too: the sum and the product round separately)
    for gamma in (0.99, 0.5):
        target, best = run_targets(qn, qt, nl, rw, dn, gamma)
        want, wbest = ref_targets(qn, qt, nl, rw, dn, gamma, A)
        assert np.array_equal(best, wbest) and best.max() > 56 and best[7] == 0
        assert np.all(best[~m.any(axis=1)] == 0)
        assert np.array_equal(target.view(np.int32), want.view(np.int32))


def test_reservoir_matches_sequential_add_on_uno():
    from rlcard_amd import VecEnv
    from rlcard_amd.agents import DeviceReservoir
    v = VecEnv('uno', N, seed=21)
    v.reset()
    g = torch.Generator().manual_seed(6)
    seed = 2 ** 40 + 9
    caps = (1 << 14, 64)
    res = [DeviceReservoir(v, cap, seed) for cap in caps]
    refs = [RefReservoir(cap, seed, 2) for cap in caps]
    for w in range(3):
        tr = v.rollout(16, policy_seed=3, t0=16 * w, final_obs=True)
        mode = (torch.rand((16, N), generator=g) < 0.5).to(torch.uint8).to(v.device)
        wh, mh = {k: x.cpu().numpy() for k, x in tr.items()}, mode.cpu().numpy()
        for r_, ref in zip(res, refs):
            r_.push(tr, mode, (0, 1))
            assert ref.push(wh, mh, (0, 1)) > 64
            assert_same_reservoir(r_, ref, A, 'capacity %d after push %d' % (ref.cap, w))
    assert refs[0].dropped == 0 == refs[0].collisions and refs[1].collisions > 0 and refs[1].dropped > 0
    st, pr = held_reservoir(res[1])
    assert st.shape == (64, D) and pr.shape == (64, A) and (pr.argmax(axis=1) > 8).any()


def new_dqn(v, seed):
    from rlcard_amd.agents import DQNAgent
    torch.manual_seed(seed)
    agent = DQNAgent(num_actions=A, state_shape=[D], mlp_layers=[64, 64], replay_memory_size=4096,
                     replay_memory_init_size=100, batch_size=32, update_target_estimator_every=1000,
                     epsilon_decay_steps=2000, learning_rate=1e-3, device=v.device)
    agent.attach(v)
    agent.generator = torch.Generator(device='cpu').manual_seed(seed)
    return agent


def new_nfsp(v, seed):
    from rlcard_amd.agents import NFSPAgent
    torch.manual_seed(seed)
    agent = NFSPAgent(num_actions=A, state_shape=[D], hidden_layers_sizes=[64, 64], q_mlp_layers=[64, 64],
                      reservoir_buffer_capacity=1024, anticipatory_param=0.5, batch_size=32,
                      min_buffer_size_to_learn=32, q_replay_memory_size=4096, q_replay_memory_init_size=100,
                      q_batch_size=32, q_epsilon_start=0.5, q_epsilon_decay_steps=2000, rl_learning_rate=1e-3,
                      device=v.device)
    agent.attach(v, seed=seed + 100)
    agent.generator = torch.Generator(device='cpu').manual_seed(seed)
    agent._rl_agent.generator = torch.Generator(device='cpu').manual_seed(seed + 1)
    return agent


@pytest.mark.parametrize('opponents', ['random', 'uno-rule-v1'])
def test_dqn_collector_on_uno(opponents):
    from rlcard_amd import VecEnv
    from rlcard_amd.agents import DQNCollector
    runs = []
    for _ in range(2):
        v = VecEnv('uno', N, seed=31)
        agent = new_dqn(v, 1)
        col = DQNCollector(v, agent, seats=(0,), opponents=opponents, steps_per_feed=32, seed=5)
        losses = col.run(train_steps=2)
        assert len(losses) == 2 and np.isfinite(losses).all() and agent.train_t == 2
        got = held(agent.device_memory)
        assert agent.total_t == len(got['action']) > 300
        assert got['state'].shape[1] == D and got['next_legal'].shape[1] == LB and got['action'].max() > 8
        acted = np.unpackbits(got['next_legal'], axis=1, bitorder='little')
        assert not acted[:, A:].any()
        runs.append(got)
    assert_same(runs[0], runs[1], 'two runs')


@pytest.mark.parametrize('opponents', ['random', 'uno-rule-v1'])
def test_nfsp_collector_on_uno(opponents):
    from rlcard_amd import VecEnv
    from rlcard_amd.agents import NFSPCollector
    runs = []
    for _ in range(2):
        v = VecEnv('uno', N, seed=31)
        agent = new_nfsp(v, 1)
        col = NFSPCollector(v, agent, seats=(0,), opponents=opponents, steps_per_feed=32, seed=5)
        rl, sl = col.run(train_steps=2, sl_steps=2)
        assert len(rl) == 2 and len(sl) == 2 and np.isfinite(rl).all() and np.isfinite(sl).all()
        mh = col.mode_rows.cpu().numpy()
        assert 0 < mh.mean() < 1
        st, pr = held_reservoir(agent.device_reservoir)
        assert st.shape[1] == D and pr.shape[1] == A and len(st) > 100
        assert np.all((pr == 0) | (pr == 1)) and np.all(pr.sum(axis=1) == 1)
        runs.append((held(agent._rl_agent.device_memory), st, pr, mh))
    assert_same(runs[0][0], runs[1][0], 'two runs')
    for a, b in zip(runs[0][1:], runs[1][1:]):
        assert np.array_equal(a, b)


@pytest.mark.parametrize('kind', ['dqn', 'nfsp'])
def test_tournament_vec_seats_a_network_against_the_rule_model(kind):
    from rlcard_amd import VecEnv
    from rlcard_amd.utils import tournament_vec
    v = VecEnv('uno', N, seed=77)
    agent = new_dqn(v, 3) if kind == 'dqn' else new_nfsp(v, 3)
    for seating in ([agent, 'uno-rule-v1'], ['uno-rule-v1', agent]):
        res = tournament_vec(v, seating, games_per_env=1, T=64)
        assert len(res) == 2 and np.isfinite(res).all()
        assert res[0] + res[1] == 0 and -1 <= res[0] <= 1


def test_single_env_path_trains_on_uno():
    """run_rl.py --env uno: make -> set_agents -> run(is_training=True) -> reorganize -> feed, against uno-rule-v1
    (host code, but make() opens the engine's device)."""
    import rlcard_amd
    from rlcard_amd import models
    from rlcard_amd.agents import DQNAgent
    from rlcard_amd.utils import reorganize, set_seed
    set_seed(3)
    env = rlcard_amd.make('uno', config={'seed': 3})
    assert env.num_actions == A and int(np.prod(env.state_shape[0])) == D
    agent = DQNAgent(num_actions=env.num_actions, state_shape=env.state_shape[0], mlp_layers=[64, 64],
                     replay_memory_init_size=16, batch_size=8, update_target_estimator_every=5,
                     device=torch.device('cpu'))
    env.set_agents([agent, models.load('uno-rule-v1').agents[1]])
    fed = episodes = 0
    while fed <= 24 and episodes < 12:
        trajectories, payoffs = env.run(is_training=True)
        episodes += 1
        for ts in reorganize(trajectories, payoffs)[0]:
            assert np.asarray(ts[0]['obs']).size == D and max(ts[3]['legal_actions'], default=0) < A
            agent.feed(ts)
            fed += 1
    assert agent.total_t == fed > 24 and agent.train_t == fed - 16 + 1 and np.isfinite(agent.last_loss)
    _, payoffs = env.run(is_training=False)
    assert len(payoffs) == 2 and payoffs[0] + payoffs[1] == 0
