"""UNO on the HIP engine against the reference's recorded streams (tests/golden/uno.npz, raw_uno.npz) and against
itself: the fused rollout row by row against the step API, the device policies against the host rule agent, state
save / load, Philox mode, refusals and the tournament sums. Shapes: 65 envs (a partial wave) and 257 (more than one
block), T = 160 so that envs finish games (46 steps on average) and restart inside a launch."""
import ctypes as C
import json

import numpy as np
import pytest

import golden_replay as gr
import rawcanon
import rlcard_amd
from rlcard_amd import VecEnv, _abi, models
from rlcard_amd.envs import uno
from rlcard_amd.utils import tournament_vec

torch = pytest.importorskip('torch')
pytestmark = pytest.mark.gpu

T, HALF, SEED, PSEED = 160, 80, 300, 17
KEYS = ('obs', 'legal', 'player', 'action', 'reward', 'done')
WD4 = sum(1 << (15 * c + 14) for c in range(4))
WILD = sum(1 << (15 * c + 13) for c in range(4))


@pytest.fixture(scope='module', autouse=True)
def _need_gpu():
    if not torch.cuda.is_available():
        pytest.fail('GPU tests need a visible GPU (run them on the MI355X box)')


def _np(o):
    return {k: v.cpu().numpy() for k, v in o.items()}


def _rollout(n, policies=None, flags=0, config=None, pseed=PSEED):
    """T steps as two launches of HALF with t0 carried -> numpy trajectory [T, n, ...] with final_obs"""
    v = VecEnv('uno', n, seed=SEED, device=0, config=config)
    if flags:
        v.set_kernel_flags(flags)
    parts = []
    for k in range(T // HALF):
        out = v.new_traj_out(HALF, final_obs=True, select=1)
        parts.append(_np(v.rollout(HALF, policy_seed=pseed, t0=k * HALF, out=out, policies=policies)))
    return {k: np.concatenate([p[k] for p in parts]) for k in parts[0]}


_cache = {}


def random_rollout(n):
    if n not in _cache:
        _cache[n] = _rollout(n)
    return _cache[n]


def legal_u64(rows):
    return rows.astype(np.uint64).dot(np.uint64(1) << (np.uint64(8) * np.arange(8, dtype=np.uint64)))


def walk(roll, n, on_row=None):
    """Steps a second VecEnv with the rollout's own action rows and compares every row. Env e consumes row cursor[e];
    an env whose game ended takes one lazy-reset step that consumes no row. on_row(v, active, cursor, view) is called
    before each step with the envs about to consume a row."""
    v = VecEnv('uno', n, seed=SEED, device=0)
    view = _np(v.reset())
    cursor = np.zeros(n, np.int64)
    pending = np.zeros(n, bool)
    idx = np.arange(n)
    ticks = 0
    while (cursor < T).any():
        act = (cursor < T) & ~pending
        c, e = cursor[act], idx[act]
        for k in ('obs', 'legal', 'player'):
            assert np.array_equal(view[k][e], roll[k][c, e]), (k, ticks)
        if on_row is not None:
            on_row(v, e, c, view)
        actions = np.zeros(n, np.int32)
        actions[e] = roll['action'][c, e]
        view = _np(v.step(torch.from_numpy(actions).cuda()))
        assert np.array_equal(view['reward'][e], roll['reward'][c, e]), ticks
        assert np.array_equal(view['done'][e], roll['done'][c, e]), ticks
        assert not view['done'][~act & (cursor < T)].any()   # a lazy reset deals: never done
        ended = e[view['done'][e] != 0]
        if len(ended):
            for p in range(2):
                fin = v.observe(p)['obs'].cpu().numpy()
                assert np.array_equal(fin[ended], roll['final_obs'][cursor[ended], ended, p]), (p, ticks)
        cursor[act] += 1
        pending = np.zeros(n, bool)
        pending[ended] = True
        ticks += 1
        assert ticks < 3 * T
    return v


# ---- the reference's streams ---------------------------------------------------------------------------------------
def test_single_env_replays_reference_stream():
    d = gr.load('uno')

    class One:
        def __init__(self, ei, seed):
            self.v = VecEnv('uno', 1, seeds=[seed], device=0)

        def reset(self):
            return {k: x[0] for k, x in _np(self.v.reset()).items()}

        def step(self, a):
            return {k: x[0] for k, x in _np(self.v.step([a])).items()}

        def observe(self, p):
            o = _np(self.v.observe(p))
            return o['obs'][0], o['legal'][0]

    assert gr.replay(d, One, 61) == len(d['ev_kind'])


def test_batched_replay_with_lazy_reset():
    """All fixture seeds as one batch; a 'reset' event after a finished game is a step with any action."""
    d = gr.load('uno')
    seeds = [int(s) for s in d['seeds']]
    v = VecEnv('uno', len(seeds), seeds=seeds, device=0)
    per_env = [np.nonzero(d['ev_env'] == i)[0] for i in range(len(seeds))]
    out = _np(v.reset())
    for tick in range(max(len(x) for x in per_env)):
        if tick > 0:
            acts = np.zeros(len(seeds), np.int32)
            for i, ev in enumerate(per_env):
                if tick < len(ev) and d['ev_kind'][ev[tick]] == 1:
                    acts[i] = d['ev_act'][ev[tick]]
            out = _np(v.step(torch.from_numpy(acts).cuda()))
        for i, ev in enumerate(per_env):
            if tick >= len(ev):
                continue
            k = ev[tick]
            assert np.array_equal(out['obs'][i], d['ev_obs'][k]), (i, tick)
            assert np.array_equal(out['legal'][i], d['ev_legal'][k]), (i, tick)
            assert out['player'][i] == d['ev_player'][k] and out['done'][i] == d['ev_done'][k], (i, tick)
            if d['ev_done'][k]:
                assert np.array_equal(out['reward'][i].astype(np.float64), d['ev_payoff'][k]), (i, tick)


def test_raw_side_matches_reference():
    d = gr.load('raw_uno')
    streams = [json.loads(s) for s in d['streams']]
    env, cur = None, -1
    for k in range(len(d['kind'])):
        si, kind, act = int(d['stream'][k]), int(d['kind'][k]), int(d['act'][k])
        if si != cur:
            s = streams[si]
            env = rlcard_amd.make(s['env_id'], dict(s['config'], seed=s['seed']))
            assert env.state_shape == [[4, 4, 15]] * 2 and env.action_shape == [None] * 2 and env.num_actions == 61
            cur = si
        if kind == 0:
            state, player = env.reset()
        elif kind == 1:
            state, player = env.step(act)
        else:
            state, player = env.get_state(act), act
        where = 'event %d (stream %d, kind %d, act %d)' % (k, si, kind, act)
        assert player == int(d['player'][k]) and int(env.is_over()) == int(d['done'][k]), where
        assert state['obs'].shape == (4, 4, 15) and state['obs'].dtype == np.int64 and state['obs'].sum() == 61, where
        assert rawcanon.dumps(rawcanon.state_view(state)) == d['state'][k], where
        assert rawcanon.dumps(env.get_perfect_information()) == d['perfect'][k], where
        if d['payoffs'][k]:
            assert rawcanon.dumps(env.get_payoffs()) == d['payoffs'][k], where


def test_env_run_with_agents_and_illegal_ids():
    from rlcard_amd.agents import RandomAgent
    env = rlcard_amd.make('uno', {'seed': 5})
    env.set_agents([RandomAgent(num_actions=env.num_actions), models.load('uno-rule-v1').agents[1]])
    traj, payoffs = env.run(is_training=False)
    assert payoffs.dtype == np.int64 and sorted(payoffs.tolist()) == [-1, 1]
    assert len(traj) == 2 and all(isinstance(t[-1], dict) for t in traj)
    state, _ = env.reset()
    bad = next(i for i in range(61) if i not in state['legal_actions'])
    env.step(bad)   # an illegal id plays the lowest legal id
    assert env.action_recorder[-1][1] == uno.ACTION_LIST[min(state['legal_actions'])]


# ---- the rollout against the step API ------------------------------------------------------------------------------
@pytest.mark.parametrize('n', [65, 257])
def test_rollout_equals_the_step_api(n):
    roll = random_rollout(n)
    games = roll['done'].sum(axis=0)   # random games last 47 steps on average, the longest recorded 233
    assert (games >= 1).mean() > 0.9 and (games >= 2).mean() > 0.5   # envs finish games and restart inside the launches
    lg = legal_u64(roll['legal'])
    assert ((lg >> roll['action'].astype(np.uint64)) & np.uint64(1)).all()   # every action is legal in its row
    assert (roll['obs'].sum(axis=2) == 61).all() and roll['obs'].max() == 1
    walk(roll, n)


def test_unstaged_fallback_gives_the_same_rollout():
    a, b = random_rollout(65), _rollout(65, flags=2)   # kernel flag bit 1: one global load per draw
    for k in a:
        assert np.array_equal(a[k], b[k]), k


def test_random_policy_actions_are_the_rollouts_pick():
    n = 65
    roll = random_rollout(n)
    v = VecEnv('uno', n, seed=SEED, device=0)
    v.reset()
    alive = np.ones(n, bool)
    for t in range(12):
        a = v.policy_actions('random', policy_seed=PSEED, t=t).cpu().numpy()
        assert np.array_equal(a[alive], roll['action'][t][alive].astype(np.int32)), t
        alive &= roll['done'][t] == 0
        acts = np.where(a < 0, 0, a).astype(np.int32)
        v.step(torch.from_numpy(acts).cuda())
    assert alive.sum() > n // 2


# ---- the rule policy -----------------------------------------------------------------------------------------------
def test_rule_policy_against_the_host_agent():
    n = 65
    roll = _rollout(n, policies=['uno-rule-v1', 'uno-rule-v1'])
    agent = models.load('uno-rule-v1').agents[0]
    seen = {'draw': 0, 'wd4': 0, 'random': 0}

    def on_row(v, e, c, view):
        lg = legal_u64(view['legal'][e])
        act = roll['action'][c, e].astype(np.int64)
        for j, env in enumerate(e):
            m, a = int(lg[j]), int(act[j])
            if (m >> 60) & 1:   # the state the agent reads: the legal list alone decides
                state = {'raw_legal_actions': ['draw'], 'raw_obs': {'hand': []}}
                assert uno.ACTION_LIST[a] == agent.step(state)
                seen['draw'] += 1
            elif m & WD4:
                s = uno.decode_words(v.env_state_words(int(env)))
                hand = s['hands'][s['current']]
                state = {'raw_legal_actions': uno.legal_actions_of(hand, s['target']),
                         'raw_obs': {'hand': [uno.card_str(x) for x in hand]}}
                assert uno.ACTION_LIST[a] == agent.step(state), state
                seen['wd4'] += 1
            else:
                allowed = m & ~WILD or m
                assert (allowed >> a) & 1, (m, a)
                seen['random'] += 1

    walk(roll, n, on_row)
    assert min(seen.values()) > 0, seen


def test_rule_seat_leaves_random_seats_games_alone():
    n = 65
    a = random_rollout(n)
    b = _rollout(n, policies=['random', 'uno-rule-v1'])
    before = np.cumsum(b['player'] == 1, axis=0) == 0          # rows before the env's first rule-seat move
    upto = np.concatenate([np.ones((1, n), bool), before[:-1]])   # ... and the row of that move itself
    assert before.any(axis=0).sum() > n // 4
    assert np.array_equal(a['action'][before], b['action'][before])
    for k in ('obs', 'legal', 'player'):
        assert np.array_equal(a[k][upto], b[k][upto]), k
    c = _rollout(n, policies=['uno-rule-v1', 'uno-rule-v1'], pseed=PSEED)
    d = _rollout(n, policies=['uno-rule-v1', 'uno-rule-v1'], pseed=PSEED)
    for k in c:
        assert np.array_equal(c[k], d[k]), k
    e = _rollout(n, policies=['uno-rule-v1', 'uno-rule-v1'], pseed=PSEED + 1)
    assert not np.array_equal(c['action'], e['action'])   # the rule's random branch follows policy_seed


# ---- state and streams ---------------------------------------------------------------------------------------------
def test_philox_mode_is_deterministic_and_another_stream():
    a = _rollout(65, config={'rng_mode': 'philox'})
    b = _rollout(65, config={'rng_mode': 'philox'})
    for k in a:
        assert np.array_equal(a[k], b[k]), k
    assert a['done'].any() and (a['obs'].sum(axis=2) == 61).all()
    assert not np.array_equal(a['obs'], random_rollout(65)['obs'])


def test_state_save_and_load_in_the_middle_of_a_rollout():
    n = 65
    roll = random_rollout(n)
    v = VecEnv('uno', n, seed=SEED, device=0)
    out = v.new_traj_out(HALF, select=1)
    v.rollout(HALF, policy_seed=PSEED, t0=0, out=out)
    saved = v.save_state()
    x = _np(v.rollout(HALF, policy_seed=PSEED, t0=HALF, out=out))
    v.load_state(saved)
    y = _np(v.rollout(HALF, policy_seed=PSEED, t0=HALF, out=out))
    for k in KEYS:
        assert np.array_equal(x[k], y[k]), k
        assert np.array_equal(x[k], roll[k][HALF:]), k
    words = v.env_state_words(3)
    v.set_env_state_words(3, words)
    assert v.env_state_words(3) == words and len(words) == 56


def test_refusals():
    cfg = _abi.Config(3, -1, 0, 0, 0)
    h = C.c_void_p()
    assert _abi.lib().cs_create(C.byref(h), 5, 8, 0, C.byref(cfg)) == -4
    assert _abi.lib().cs_last_error().startswith(b'uno: game_num_players must be 2')
    with pytest.raises(ValueError):
        rlcard_amd.make('uno', {'game_num_players': 3})
    v = VecEnv('uno', 65, seed=1, device=0)
    with pytest.raises(_abi.CardsimError, match='CS_E_UNSUPPORTED'):
        v.policy_actions(2)
    with pytest.raises(_abi.CardsimError, match='CS_E_UNSUPPORTED'):
        v.rollout(4, out=v.new_traj_out(4, select=1), policies=[2, 'random'])


# ---- tournament ----------------------------------------------------------------------------------------------------
def test_tournament_sums():
    v = VecEnv('uno', 65, seed=SEED, device=0)
    pay = tournament_vec(v, ['uno-rule-v1', 'random'], games_per_env=2, T=64, policy_seed=PSEED)
    assert len(pay) == 2 and pay[0] + pay[1] == 0 and -1 <= pay[0] <= 1
    v = VecEnv('uno', 65, seed=SEED, device=0)
    traj = v.rollout(T, policy_seed=PSEED, out=v.new_traj_out(T, select=1), policies=['uno-rule-v1', 'random'])
    acc = v.payoff_sums(traj, v.new_payoff_sums(), quota=0)
    assert int(acc['games'].item()) == int(traj['done'].sum().item()) > 65
    assert float(acc['sums'].sum().item()) == 0.0
