"""DQN on the device (rlcard_amd/csrc/cs_dqn.hip through include/cardsim.h and rlcard_amd/agents/dqn_agent.py): the
fused Q-network policy kernel against fp64 and torch-CPU forwards and against cs_dmc_select's draw, the replay ring
against a numpy restatement of reorganize (rlcard/utils/utils.py:153-179) with the carry between windows, the
Double-DQN targets against the reference's recorded train() call (tests/golden/dqn.npz), and the agent end to end.
Needs a GPU."""
import ctypes as C

import numpy as np
import pytest

from test_dqn import GOLDEN, estimator_of, unfolded64

torch = pytest.importorskip('torch')
pytestmark = pytest.mark.gpu


@pytest.fixture(scope='module', autouse=True)
def _need_gpu():
    if not torch.cuda.is_available():
        pytest.fail('GPU tests need a visible GPU (run them on the MI355X box)')


@pytest.fixture(scope='module')
def gold():
    return dict(np.load(GOLDEN, allow_pickle=False))


def _ptr(t):
    return None if t is None else C.c_void_p(t.data_ptr())


def qnet_values(v, est, obs, legal):
    from rlcard_amd import _abi
    q = torch.empty((obs.shape[0], est.num_actions), dtype=torch.float32, device=v.device)
    _abi.check(_abi.lib().cs_qnet_values(v._h, C.byref(est.folded()), _ptr(obs), _ptr(legal), obs.shape[0], _ptr(q),
                                         v._stream()), 'cs_qnet_values')
    return q


def qnet_actions(v, est, obs, legal, done=None, eps=0.0, seed=0, t=0, row_base=0, q=None):
    from rlcard_amd import _abi
    a = torch.empty(obs.shape[0], dtype=torch.int32, device=v.device)
    _abi.check(_abi.lib().cs_qnet_actions(v._h, C.byref(est.folded()), _ptr(obs), _ptr(legal), _ptr(done),
                                          obs.shape[0], float(eps), seed, t, row_base, _ptr(a), _ptr(q), v._stream()),
               'cs_qnet_actions')
    return a


def random_estimator(num_actions, obs_dim, mlp, seed, device):
    """Seeded random weights, BatchNorm statistics and affine included (so the folding is not the identity)."""
    from rlcard_amd.agents import Estimator
    torch.manual_seed(seed)
    est = Estimator(num_actions=num_actions, state_shape=[obs_dim], mlp_layers=list(mlp), device=torch.device('cpu'))
    g = torch.Generator().manual_seed(seed)
    bn = est.qnet.fc_layers[1]
    with torch.no_grad():
        bn.running_mean.copy_(torch.rand(obs_dim, generator=g) * 2)
        bn.running_var.copy_(torch.rand(obs_dim, generator=g) * 4 + 0.5)
        bn.weight.copy_(torch.rand(obs_dim, generator=g) + 0.5)
        bn.bias.copy_(torch.rand(obs_dim, generator=g) - 0.5)
        for m in est.qnet.fc_layers:
            if isinstance(m, torch.nn.Linear):
                m.bias.copy_(torch.rand(m.bias.shape, generator=g) - 0.5)
    return est


def on_device(est, device):
    from rlcard_amd.agents import Estimator
    d = Estimator(num_actions=est.num_actions, state_shape=est.state_shape, mlp_layers=est.mlp_layers, device=device)
    d.load_state_dict(est.qnet.state_dict())
    return d


# game, config, rows, network: a fixture name or (mlp, seed)
VALUE_CASES = [('leduc-holdem', None, 300, 'leduc'), ('limit-holdem', None, 130, 'limit'),
               ('no-limit-holdem', None, 70, ([20], 1)), ('blackjack', None, 65, ([7, 5, 3, 2], 2))]
_case_cache = {}


def value_case(gold, case):
    """-> (vec, CPU estimator, device estimator, obs u8 [R, D], legal u8 [R, 1]) with rows of a short rollout, and the
    fp64 reference / torch-CPU fp32 forwards of the rows; computed once per case."""
    from rlcard_amd import VecEnv
    game, config, rows, net = case
    key = (game, rows)
    if key in _case_cache:
        return _case_cache[key]
    v = VecEnv(game, 64, seed=5, config=config)
    v.reset()
    tr = v.rollout(8, policy_seed=9)
    obs = tr['obs'].reshape(-1, v.obs_dim)[:rows].contiguous()
    legal = tr['legal'].reshape(-1, v.legal_bytes)[:rows].contiguous()
    assert obs.shape[0] == rows
    if isinstance(net, str):
        cpu = estimator_of(gold, net)
    else:
        cpu = random_estimator(v.num_actions, v.obs_dim, net[0], net[1], 'cpu')
    x = obs.cpu().numpy()
    ref64 = unfolded64(cpu, x)
    q_torch = cpu.predict_nograd(x.astype(np.float32)).astype(np.float64)
    out = dict(v=v, cpu=cpu, dev=on_device(cpu, v.device), obs=obs, legal=legal, ref64=ref64, q_torch=q_torch,
               mask=np.unpackbits(legal.cpu().numpy(), axis=1, bitorder='little')[:, :v.num_actions].astype(bool))
    _case_cache[key] = out
    return out


@pytest.mark.parametrize('case', VALUE_CASES, ids=[c[0] for c in VALUE_CASES])
def test_qnet_values(gold, case):
    """E_kernel <= 8 E_torch over the legal entries (both fp32 sums of at most 128 terms in different orders; the factor
    covers the order, the folded BatchNorm's extra rounding and the device tanhf); illegal entries exactly -inf."""
    c = value_case(gold, case)
    q = qnet_values(c['v'], c['dev'], c['obs'], c['legal']).cpu().numpy()
    m = c['mask']
    assert m.any(axis=1).all() and (not m.all() or case[0] == 'blackjack')   # (hit and stand are always legal)
    assert np.all(q[~m] == -np.inf)
    assert np.isfinite(q[m]).all()
    e_torch = np.abs(c['q_torch'] - c['ref64'])[m].max()
    e_kernel = np.abs(q.astype(np.float64) - c['ref64'])[m].max()
    print('%s: E_torch %.3e E_kernel %.3e ratio %.2f |q| <= %.2f' % (case[0], e_torch, e_kernel, e_kernel / e_torch,
                                                                      np.abs(c['ref64'][m]).max()))
    assert e_kernel <= 8 * e_torch
    # no mask: every action's value, the same numbers
    q_all = qnet_values(c['v'], c['dev'], c['obs'], None).cpu().numpy()
    assert np.isfinite(q_all).all() and np.array_equal(q_all[m], q[m])


@pytest.mark.parametrize('case', VALUE_CASES, ids=[c[0] for c in VALUE_CASES])
def test_qnet_actions(gold, case):
    from rlcard_amd.agents.dmc_agent import select_actions
    c = value_case(gold, case)
    v, est, obs, m = c['v'], c['dev'], c['obs'], c['mask']
    R, A = obs.shape[0], v.num_actions
    # rows with a done byte and rows with an empty mask get -1
    legal = c['legal'].clone()
    done = torch.zeros(R, dtype=torch.uint8, device=v.device)
    legal[3::17] = 0
    done[5::13] = 1
    m = m.copy()
    m[3::17] = False
    dn = done.cpu().numpy().astype(bool)
    q = torch.empty((R, A), dtype=torch.float32, device=v.device)
    greedy = qnet_actions(v, est, obs, legal, done, q=q).cpu().numpy()
    qh = q.cpu().numpy()
    assert np.all(qh[~m] == -np.inf) and np.array_equal(qh[m], qnet_values(v, est, obs, legal).cpu().numpy()[m])
    none = ~m.any(axis=1)
    assert none.any() and dn.any() and (~(none | dn)).sum() > R // 2
    assert np.all(greedy[none | dn] == -1)
    live = ~(none | dn)
    assert np.array_equal(greedy[live], np.argmax(qh, axis=1)[live])          # first maximum of the kernel's own row
    # the fp64 argmax wherever its top-two legal gap is clear of the fp32 error
    e_torch = np.abs(c['q_torch'] - c['ref64'])[c['mask']].max()
    r64 = np.where(m, c['ref64'], -np.inf)
    top = np.sort(r64, axis=1)
    with np.errstate(invalid='ignore'):     # (rows without a legal action: -inf - -inf; they are not live)
        clear = live & ((top[:, -1] - top[:, -2]) > 16 * e_torch)
    assert (live & ~clear).sum() <= R // 100
    assert np.array_equal(greedy[clear], np.argmax(r64, axis=1)[clear])
    # no done pointer: only the empty masks give -1
    g2 = qnet_actions(v, est, obs, legal).cpu().numpy()
    assert np.array_equal(g2 == -1, none) and np.array_equal(g2[live], greedy[live])
    # epsilon draws: cs_dmc_select fed the same values through legal_lists, bit for bit
    counts, offsets, ids = v.legal_lists(legal)
    state_of = torch.repeat_interleave(torch.arange(R, device=v.device), counts.long())
    values = q[state_of, ids.long()].contiguous()
    for eps, seed, t, base in ((0.3, 7, 11, 1000), (1.0, 2 ** 40 + 3, 2 ** 33, 5), (0.0, 1, 2, 3)):
        got = qnet_actions(v, est, obs, legal, None, eps, seed, t, base).cpu().numpy()
        want = select_actions(values, counts, offsets, ids, eps, seed, t, base).cpu().numpy()
        assert np.array_equal(got, want), eps
        if eps == 1.0:
            assert (got[live] != greedy[live]).any()
            assert all(m[r, got[r]] for r in np.nonzero(live)[0])


def test_qnet_refusals(gold):
    from rlcard_amd import VecEnv, _abi
    leduc = VecEnv('leduc-holdem', 64, seed=1)
    dev = on_device(estimator_of(gold, 'leduc'), leduc.device)
    obs = torch.zeros((64, 901), dtype=torch.uint8, device=leduc.device)
    ddz = VecEnv('doudizhu', 2, seed=1)
    with pytest.raises(_abi.CardsimError, match='CS_E_UNSUPPORTED'):
        qnet_values(ddz, dev, obs, None)
    limit_net = on_device(estimator_of(gold, 'limit'), leduc.device)
    with pytest.raises(_abi.CardsimError, match='CS_E_INVALID'):       # in_dim 72 on a 36-byte game
        qnet_values(leduc, limit_net, obs, None)
    net = dev.folded()
    bad = _abi.QNet.from_buffer_copy(net)
    bad.hidden[0] = 129
    q = torch.empty((64, 4), dtype=torch.float32, device=leduc.device)
    assert _abi.lib().cs_qnet_values(leduc._h, C.byref(bad), _ptr(obs), None, 64, _ptr(q), None) == -1
    bad = _abi.QNet.from_buffer_copy(net)
    bad.W[1] = None
    assert _abi.lib().cs_qnet_values(leduc._h, C.byref(bad), _ptr(obs), None, 64, _ptr(q), None) == -1
    with pytest.raises(_abi.CardsimError, match='CS_E_UNSUPPORTED'):
        from rlcard_amd.agents import DeviceMemory
        DeviceMemory(ddz, 16)


# ---- replay ----------------------------------------------------------------------------------------------------------
FIELDS = ('state', 'action', 'reward', 'next_state', 'next_legal', 'done')


class RefReplay:
    """reorganize over consecutive windows, restated: per (env, seat) the transitions [state, action, reward,
    next_state, done] + the next state's legal mask, a row whose next state lies past the window carried to the next
    push; emitted per push as the header documents: completed carried rows in (env, seat) order, then the window's rows
    in (t, env) order."""

    def __init__(self, P, O, LB):
        self.P, self.O, self.LB = P, O, LB
        self.pending = {}
        self.out = []

    def _next(self, w, e, p, t_from):
        """what follows for seat p of env e from row t_from on: its next row, or the game's end"""
        T = w['player'].shape[0]
        for t in range(t_from, T):
            if w['player'][t, e] == p:
                return (w['obs'][t, e], w['legal'][t, e], 0.0, 0)
            if w['done'][t, e]:
                return (w['final_obs'][t, e, p], np.zeros(self.LB, np.uint8), float(w['reward'][t, e, p]), 1)
        return None

    def push(self, w, seats):
        T, n = w['player'].shape
        for e in range(n):
            for p in range(self.P):
                if (e, p) in self.pending:
                    nx = self._next(w, e, p, 0)
                    if nx is not None:
                        s, a = self.pending.pop((e, p))
                        self.out.append((s, a, nx[2], nx[0], nx[1], nx[3]))
        for t in range(T):
            for e in range(n):
                p = int(w['player'][t, e])
                if p >= self.P or p not in seats:
                    continue
                s, a = w['obs'][t, e].copy(), int(w['action'][t, e])
                if w['done'][t, e]:
                    nx = (w['final_obs'][t, e, p], np.zeros(self.LB, np.uint8), float(w['reward'][t, e, p]), 1)
                else:
                    nx = self._next(w, e, p, t + 1)
                if nx is None:
                    assert (e, p) not in self.pending
                    self.pending[(e, p)] = (s, a)
                else:
                    self.out.append((s, a, nx[2], nx[0], nx[1], nx[3]))

    def held(self, cap):
        rows = self.out[-cap:]
        return dict(state=np.array([r[0] for r in rows], np.float32).reshape(-1, self.O),
                    action=np.array([r[1] for r in rows], np.int64),
                    reward=np.array([r[2] for r in rows], np.float32),
                    next_state=np.array([r[3] for r in rows], np.float32).reshape(-1, self.O),
                    next_legal=np.array([r[4] for r in rows], np.uint8).reshape(-1, self.LB),
                    done=np.array([r[5] for r in rows], np.uint8))


def held(mem):
    size = len(mem)
    got = mem.gather(torch.arange(size, device=mem.vec.device))
    return {k: x.cpu().numpy() for k, x in got.items()}


def assert_same(got, want, what):
    for k in FIELDS:
        assert got[k].shape == want[k].shape, (what, k, got[k].shape, want[k].shape)
        assert np.array_equal(got[k], want[k]), (what, k)


# (game, config, envs, steps of each window, capacities: everything held; wraps; a longest-window push overflows it)
EQUAL_WINDOWS = ((16,) * 5, (1 << 16, 1000, 64))
REPLAY_CASES = [('leduc-holdem', None, 300) + EQUAL_WINDOWS, ('no-limit-holdem', None, 100) + EQUAL_WINDOWS,
                ('blackjack', None, 200) + EQUAL_WINDOWS, ('leduc-holdem', {'game_num_players': 3}, 96) + EQUAL_WINDOWS,
                # two waves plus two envs; the push scratch grows (2 -> 8 steps) and is reused at a smaller size
                ('leduc-holdem', None, 130, (2, 8, 2), (1 << 16, 200, 97))]


@pytest.mark.parametrize('all_seats', [False, True], ids=['seat0', 'all'])
@pytest.mark.parametrize('case', REPLAY_CASES, ids=['leduc', 'nolimit', 'blackjack', 'leduc3', 'leduc-grow'])
def test_replay_matches_reorganize_with_carry(case, all_seats):
    from rlcard_amd import VecEnv
    from rlcard_amd.agents import DeviceMemory
    game, config, n, windows, caps = case
    v = VecEnv(game, n, seed=21, config=config)
    v.reset()
    seats = tuple(range(v.num_players)) if all_seats else (0,)
    mems = [DeviceMemory(v, cap) for cap in caps]
    ref = RefReplay(v.num_players, v.obs_dim, v.legal_bytes)
    trajs = {T: v.new_traj_out(T, final_obs=True, select=1) for T in set(windows)}
    carried = t0 = 0
    for w, T in enumerate(windows):
        tr = trajs[T]
        v.rollout(T, policy_seed=3, t0=t0, out=tr)
        t0 += T
        for mem in mems:
            mem.push(tr, seats)
        before = len(ref.out)
        ref.push({k: x.cpu().numpy() for k, x in tr.items()}, seats)
        carried += len(ref.pending)
        if T == max(windows):
            assert len(ref.out) - before > caps[2]       # the push overflows the smallest ring
        for mem, cap in zip(mems, caps):
            assert mem.sizes() == (min(len(ref.out), cap), len(ref.out))
        assert_same(held(mems[2]), ref.held(caps[2]), 'capacity %d after push %d' % (caps[2], w))
    assert carried > 0
    assert len(ref.out) > caps[1]
    for mem, cap in zip(mems, caps):
        assert_same(held(mem), ref.held(cap), 'capacity %d' % cap)
    want = ref.held(1 << 16)
    assert want['done'].any() and not want['done'].all()
    assert np.all(want['next_legal'][want['done'] == 1] == 0) and np.all(want['reward'][want['done'] == 0] == 0)
    # a sample is distinct rows of the memory
    g = torch.Generator(device='cpu').manual_seed(1)
    b = mems[1].sample(32, g)
    all_rows = held(mems[1])
    for k in range(32):
        hits = np.nonzero((all_rows['state'] == b['state'][k].cpu().numpy()).all(axis=1))[0]
        assert len(hits) >= 1
    with pytest.raises(ValueError):
        DeviceMemory(v, 8).sample(1)


def test_replay_straddling_transition_once_and_drop_pending():
    """A transition whose game spans two windows appears exactly once, after the second push; drop_pending removes
    it."""
    from rlcard_amd import VecEnv
    from rlcard_amd.agents import DeviceMemory
    v = VecEnv('leduc-holdem', 300, seed=4)
    v.reset()
    keep, drop = DeviceMemory(v, 1 << 14), DeviceMemory(v, 1 << 14)
    ref_keep, ref_drop = RefReplay(2, 36, 1), RefReplay(2, 36, 1)
    w = []
    for k in range(2):
        tr = v.rollout(16, policy_seed=8, t0=16 * k, final_obs=True)
        w.append({x: y.cpu().numpy() for x, y in tr.items()})
        keep.push(tr, (0, 1))
        drop.push(tr, (0, 1))
        ref_keep.push(w[-1], (0, 1))
        ref_drop.push(w[-1], (0, 1))
        if k == 0:
            first = len(ref_keep.out)
            assert keep.sizes() == (first, first)
            pend = dict(ref_keep.pending)
            assert len(pend) > 20
            drop.drop_pending()
            ref_drop.pending.clear()
    # 16 more steps end every Leduc game in progress: each carried row is completed, and only where it was kept
    assert len(ref_keep.out) - len(ref_drop.out) == len(pend)
    assert keep.sizes()[1] - drop.sizes()[1] == len(pend)
    got = held(keep)
    assert_same(got, ref_keep.held(1 << 14), 'carried')
    # the carried rows come first in the second push, in (env, seat) order, each once
    for j, key in enumerate(sorted(pend)):
        s, a = pend[key]
        assert np.array_equal(got['state'][first + j], s.astype(np.float32)) and got['action'][first + j] == a
    assert_same(held(drop), ref_drop.held(1 << 14), 'dropped')


def test_buffers_may_be_closed_after_their_env():
    """include/cardsim.h: a buffer may be destroyed after its handle. Closing the env first, then its three kinds of
    buffer, raises nothing and leaves the device usable."""
    from rlcard_amd import VecEnv
    from rlcard_amd.agents import DeviceMemory
    from rlcard_amd.agents.dmc_agent import ActorBuffers
    from rlcard_amd.agents.nfsp_agent import DeviceReservoir
    v = VecEnv('leduc-holdem', 64, seed=4)
    bufs = [DeviceMemory(v, 256), DeviceReservoir(v, 256, seed=1), ActorBuffers(v, T=4, slots=3)]
    v.close()
    for b in bufs:
        b.close()
        assert b._h is None
    fresh = VecEnv('leduc-holdem', 64, seed=4)
    fresh.reset()
    out = fresh.step(fresh.policy_actions('random'))
    torch.cuda.synchronize()
    assert out['obs'].shape == (64, fresh.obs_dim) and int(out['obs'].sum()) > 0


# ---- targets ----------------------------------------------------------------------------------------------------------
def ref_targets(qn, qt, next_legal, reward, done, gamma, A):
    """dqn_agent.py:205-218 in numpy: the masked argmax, then float32(1 - done) * gamma * q in float32, plus the
    float64 reward, cast to float32."""
    m = np.unpackbits(next_legal, axis=1, bitorder='little')[:, :A].astype(bool)
    best = np.argmax(np.where(m, qn.astype(np.float64), -np.inf), axis=1)
    prod = np.invert(done.astype(bool)).astype(np.float32) * np.float32(gamma) * qt[np.arange(len(best)), best]
    assert prod.dtype == np.float32
    return (reward.astype(np.float64) + prod).astype(np.float32), best


def run_targets(qn, qt, nl, rw, dn, gamma):
    from rlcard_amd.agents.dqn_agent import dqn_targets
    d = torch.device('cuda')
    t, b = dqn_targets(*(torch.from_numpy(np.ascontiguousarray(x)).to(d) for x in (qn, qt, nl, rw, dn)), gamma)
    return t.cpu().numpy(), b.cpu().numpy()


def test_targets_recorded_batch(gold):
    g = gold
    gamma = float(g['leduc_train_gamma'])
    target, best = run_targets(g['leduc_train_q_next'], g['leduc_train_q_next_target'], g['leduc_train_next_legal'],
                               g['leduc_train_reward'], g['leduc_train_done'], gamma)
    assert np.array_equal(best, g['leduc_train_best'])
    assert np.array_equal(target.view(np.int32), g['leduc_train_target'].astype(np.float32).view(np.int32))
    want, wbest = ref_targets(g['leduc_train_q_next'], g['leduc_train_q_next_target'], g['leduc_train_next_legal'],
                              g['leduc_train_reward'], g['leduc_train_done'], gamma, 4)
    assert np.array_equal(wbest, best) and np.array_equal(want.view(np.int32), target.view(np.int32))


def test_targets_random_rows():
    rng = np.random.RandomState(12)
    B, A = 1000, 5
    nl = rng.randint(0, 32, size=(B, 1)).astype(np.uint8)
    nl[::50] = 0                                             # no legal action: best 0
    dn = (rng.rand(B) < 0.3).astype(np.uint8)
    nl[dn == 1] = 0                                          # terminal rows carry an empty mask
    dn[::50] = 1
    dn[25::50] = 0
    nl[25::50] = 0                                           # (and an empty mask on a non-terminal row)
    m = np.unpackbits(nl, axis=1, bitorder='little')[:, :A].astype(bool)
    qn = np.where(m, rng.randn(B, A), -np.inf).astype(np.float32)
    qn[7] = qn[7, 0] if m[7].all() else qn[7]                # ties: the first maximum
    qt = (rng.randn(B, A) * 3).astype(np.float32)
    rw = (rng.randint(-8, 9, size=B) * 0.5).astype(np.float32)
    rw[dn == 0] = 0
    rw[3] = 0.1                                              # a reward that is no multiple of a power of two
    for gamma in (0.99, 1.0, 0.5):
        target, best = run_targets(qn, qt, nl, rw, dn, gamma)
        want, wbest = ref_targets(qn, qt, nl, rw, dn, gamma, A)
        assert np.array_equal(best, wbest)
        assert np.all(best[~m.any(axis=1)] == 0)
        assert np.array_equal(target.view(np.int32), want.view(np.int32))
        assert np.array_equal(target[dn == 1], rw[dn == 1])


# ---- end to end ------------------------------------------------------------------------------------------------------
def params_of(est):
    return [p.detach().clone() for p in est.qnet.state_dict().values()]


def same_params(a, b):
    return all(torch.equal(x, y) for x, y in zip(a, b))


def new_vec_agent(v, seed):
    from rlcard_amd.agents import DQNAgent
    torch.manual_seed(seed)
    agent = DQNAgent(num_actions=4, state_shape=[36], mlp_layers=[64, 64], replay_memory_size=4096,
                     replay_memory_init_size=100, batch_size=32, update_target_estimator_every=1000,
                     epsilon_decay_steps=2000, learning_rate=1e-3, device=v.device)
    agent.attach(v)
    agent.generator = torch.Generator(device='cpu').manual_seed(seed)
    return agent


def test_collector_feed_train_end_to_end():
    from rlcard_amd import VecEnv
    from rlcard_amd.agents import DQNCollector
    v = VecEnv('leduc-holdem', 256, seed=31)
    agent = new_vec_agent(v, 1)
    col = DQNCollector(v, agent, seats=(0,), opponents='leduc-holdem-rule-v1', steps_per_feed=16, seed=5)
    ref = RefReplay(2, 36, 1)
    start = params_of(agent.q_estimator)
    # round 1: one train step -- the first train() copies the Q-network into the target network (train_t 0)
    tr = col.collect()
    ref.push({k: x.cpu().numpy() for k, x in tr.items()}, (0,))
    assert (tr['player'] == 255).any() and tr['done'].any()
    eps0 = agent.epsilon()
    losses = agent.feed_vec(tr, (0,), train_steps=1)
    assert agent.total_t == len(ref.out) > 100 and len(agent.device_memory) == len(ref.out)
    assert agent.train_t == 1 and len(losses) == 1
    assert agent.epsilon() < eps0 == 1.0
    assert same_params(params_of(agent.q_estimator), params_of(agent.target_estimator))
    assert not same_params(params_of(agent.q_estimator), start)
    # round 2: two more -- no copy before train_t 1000, so the networks part
    losses += col.run(train_steps=2)
    ref.push({k: x.cpu().numpy() for k, x in col.traj.items()}, (0,))
    assert agent.train_t == 3 and agent.total_t == len(ref.out)
    assert not same_params(params_of(agent.q_estimator), params_of(agent.target_estimator))
    # round 3: the reference's number of train() calls for the advance of total_t
    agent.train_every = 400
    t0 = agent.total_t
    losses += col.run()
    ref.push({k: x.cpu().numpy() for k, x in col.traj.items()}, (0,))
    assert agent.total_t == len(ref.out) and len(agent.device_memory) == min(len(ref.out), 4096)
    steps = len([t for t in range(t0 + 1, agent.total_t + 1) if t >= 100 and (t - 100) % 400 == 0])
    assert agent.train_t == 3 + steps and 2 <= steps <= 6
    assert len(losses) == 3 + steps and np.isfinite(losses).all()
    assert_same(held(agent.device_memory), ref.held(4096), 'collector')


def test_collector_replay_is_deterministic():
    from rlcard_amd import VecEnv
    from rlcard_amd.agents import DQNCollector
    runs = []
    for _ in range(2):
        v = VecEnv('leduc-holdem', 256, seed=31)
        agent = new_vec_agent(v, 1)
        col = DQNCollector(v, agent, seats=(0,), opponents='leduc-holdem-rule-v1', steps_per_feed=16, seed=5)
        for _ in range(3):
            assert col.run(train_steps=0) == []
        assert agent.train_t == 0
        runs.append(held(agent.device_memory))
    assert len(runs[0]['action']) > 300
    assert_same(runs[0], runs[1], 'two runs')


class PolicySeat:
    """An engine policy behind the eval_step_vec interface: makes tournament_vec take its stepped form."""

    def __init__(self, vec, policy):
        self.vec, self.policy = vec, policy

    def eval_step_vec(self, state, t=0, seed=0):
        return self.vec.policy_actions(self.policy, 0, t)


class RandomSeat:
    policy_id = 0       # CS_POLICY_RANDOM, the way rlcard_amd.models' agents name their engine policy


def test_tournament_vec_seats_a_network():
    from rlcard_amd import VecEnv
    from rlcard_amd.utils import tournament_vec
    rule = 'leduc-holdem-rule-v1'
    v = VecEnv('leduc-holdem', 256, seed=77)
    agent = new_vec_agent(v, 3)
    res = tournament_vec(v, [agent, rule], 4)
    assert len(res) == 2 and np.isfinite(res).all() and res[0] + res[1] == 0
    v4 = VecEnv('leduc-holdem', 256, seed=77)
    res2 = tournament_vec(v4, [rule, PolicySeat(v4, 'random')], 4)
    assert len(res2) == 2 and np.isfinite(res2).all() and res2[0] + res2[1] == 0
    # with engine policies only the fused path runs, whatever form names the policy: the same numbers as the rollout
    # and payoff_sums by hand
    fused = [tournament_vec(VecEnv('leduc-holdem', 256, seed=77), [rnd, rule], 4, policy_seed=9)
             for rnd in ('random', 0, RandomSeat())]
    v2 = VecEnv('leduc-holdem', 256, seed=77)
    traj, acc, t0 = v2.new_traj_out(64, select=1), v2.new_payoff_sums(), 0
    while int(acc['games_per_env'].min().item()) < 4:
        v2.rollout(64, policy_seed=9, t0=t0, out=traj, policies=['random', rule])
        v2.payoff_sums(traj, acc, 4)
        t0 += 64
    by_hand = list((acc['sums'] / acc['games'].double()).cpu().numpy())
    assert fused[0] == fused[1] == fused[2] == by_hand
    # the stepped form against the fused one where they must agree: rule seats draw nothing and the deals are the
    # envs' own, so each env's first 4 games are the same games
    v3 = VecEnv('leduc-holdem', 256, seed=77)
    stepped = tournament_vec(v3, [PolicySeat(v3, rule), rule], 4)
    both = tournament_vec(VecEnv('leduc-holdem', 256, seed=77), [rule, rule], 4)
    assert stepped == both


def test_single_env_path_trains():
    """run_rl.py's loop: make -> set_agents -> run(is_training=True) -> reorganize -> feed."""
    import rlcard_amd
    from rlcard_amd.agents import DQNAgent, RandomAgent
    from rlcard_amd.utils import reorganize, set_seed
    set_seed(3)
    env = rlcard_amd.make('leduc-holdem', config={'seed': 3})
    agent = DQNAgent(num_actions=env.num_actions, state_shape=env.state_shape[0], mlp_layers=[64, 64],
                     replay_memory_init_size=16, batch_size=8, update_target_estimator_every=5)
    env.set_agents([agent, RandomAgent(num_actions=env.num_actions)])
    start = params_of(agent.q_estimator)
    fed = 0
    for _ in range(24):
        trajectories, payoffs = env.run(is_training=True)
        trans = reorganize(trajectories, payoffs)[0]
        for ts in trans:      # (none where seat 1 moved first and folded)
            assert ts[4] is (ts is trans[-1]) and ts[2] == (payoffs[0] if ts[4] else 0)
            agent.feed(ts)
            fed += 1
    assert agent.total_t == fed == len(agent.memory) and fed > 24
    assert agent.train_t == fed - 16 + 1 and np.isfinite(agent.last_loss)
    assert not same_params(params_of(agent.q_estimator), start)
    _, payoffs = env.run(is_training=False)
    assert len(payoffs) == 2 and payoffs[0] + payoffs[1] == 0
