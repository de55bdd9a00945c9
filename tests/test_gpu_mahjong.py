"""Mahjong on the HIP engine against the reference's recorded streams (tests/golden/mahjong.npz, mahjong_hu.npz,
raw_mahjong.npz) and against itself: the fused rollout row by row against the step API, the judge hook, state save /
load, step_back, Philox mode, constructed states, refusals and the tournament sums. Shapes: 65 envs (a partial wave)
and 257 (more than one block), T = 128: the reference's 300 uniform-random games all ended within 105 steps."""
import ctypes as C
import json

import numpy as np
import pytest

import golden_replay as gr
import rawcanon
import rlcard_amd
from rlcard_amd import VecEnv, _abi
from rlcard_amd.envs import mahjong
from rlcard_amd.utils import tournament_vec
from test_mahjong import raw_view

torch = pytest.importorskip('torch')
pytestmark = pytest.mark.gpu

T, HALF, SEED, PSEED = 128, 64, 500, 23
KEYS = ('obs', 'legal', 'player', 'action', 'reward', 'done')


@pytest.fixture(scope='module', autouse=True)
def _need_gpu():
    if not torch.cuda.is_available():
        pytest.fail('GPU tests need a visible GPU (run them on the MI355X box)')


def _np(o):
    return {k: v.cpu().numpy() for k, v in o.items()}


def _rollout(n, flags=0, config=None, pseed=PSEED):
    """T steps as two launches of HALF with t0 carried -> numpy trajectory [T, n, ...] with final_obs"""
    v = VecEnv('mahjong', n, seed=SEED, device=0, config=config)
    if flags:
        v.set_kernel_flags(flags)
    parts = []
    for k in range(T // HALF):
        out = v.new_traj_out(HALF, final_obs=True, select=1)
        parts.append(_np(v.rollout(HALF, policy_seed=pseed, t0=k * HALF, out=out)))
    return {k: np.concatenate([p[k] for p in parts]) for k in parts[0]}


_cache = {}


def random_rollout(n):
    if n not in _cache:
        _cache[n] = _rollout(n)
    return _cache[n]


def legal_u64(rows):
    return rows.astype(np.uint64).dot(np.uint64(1) << (np.uint64(8) * np.arange(rows.shape[-1], dtype=np.uint64)))


def walk(roll, n):
    """Steps a second VecEnv with the rollout's own action rows and compares every row. Env e consumes row cursor[e];
    an env whose game ended takes one lazy-reset step that consumes no row."""
    v = VecEnv('mahjong', n, seed=SEED, device=0)
    view = _np(v.reset())
    cursor = np.zeros(n, np.int64)
    pending = view['done'] != 0   # (a game won on the deal: the next step deals again)
    assert not pending.any()
    idx = np.arange(n)
    ticks = 0
    while (cursor < T).any():
        act = (cursor < T) & ~pending
        c, e = cursor[act], idx[act]
        for k in ('obs', 'legal', 'player'):
            assert np.array_equal(view[k][e], roll[k][c, e]), (k, ticks)
        actions = np.zeros(n, np.int32)
        actions[e] = roll['action'][c, e]
        view = _np(v.step(torch.from_numpy(actions).cuda()))
        assert np.array_equal(view['reward'][e], roll['reward'][c, e]), ticks
        assert np.array_equal(view['done'][e], roll['done'][c, e]), ticks
        ended = e[view['done'][e] != 0]
        if len(ended):
            for p in range(4):
                fin = v.observe(p)['obs'].cpu().numpy()
                assert np.array_equal(fin[ended], roll['final_obs'][cursor[ended], ended, p]), (p, ticks)
        cursor[act] += 1
        pending = np.zeros(n, bool)
        pending[ended] = True
        ticks += 1
        assert ticks < 3 * T
    return v


class One:
    def __init__(self, ei, seed):
        self.v = VecEnv('mahjong', 1, seeds=[seed], device=0)

    def reset(self):
        return {k: x[0] for k, x in _np(self.v.reset()).items()}

    def step(self, a):
        return {k: x[0] for k, x in _np(self.v.step([a])).items()}

    def observe(self, p):
        o = _np(self.v.observe(p))
        return o['obs'][0], o['legal'][0]


# ---- the reference's streams ---------------------------------------------------------------------------------------
def test_single_env_replays_reference_stream():
    d = gr.load('mahjong')
    assert gr.replay(d, One, 38) == len(d['ev_kind'])


def test_batched_replay_with_lazy_reset():
    """All fixture seeds as one batch; a 'reset' event after a finished game is a step with any action."""
    d = gr.load('mahjong')
    seeds = [int(s) for s in d['seeds']]
    v = VecEnv('mahjong', len(seeds), seeds=seeds, device=0)
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


def test_judge_hook_matches_the_reference():
    h = gr.load('mahjong_hu')
    n = len(h['win'])
    dev = [torch.from_numpy(np.ascontiguousarray(h[k])).cuda() for k in ('hands', 'len', 'piles')]
    win = torch.full((n,), 7, dtype=torch.uint8, device='cuda')
    _abi.check(_abi.lib().cs_debug_mahjong_hu(*[C.c_void_p(x.data_ptr()) for x in dev], n, C.c_void_p(win.data_ptr()),
                                              None), 'cs_debug_mahjong_hu')
    torch.cuda.synchronize()
    bad = np.nonzero(win.cpu().numpy() != h['win'])[0]
    assert len(bad) == 0, (bad[:10], h['hands'][bad[0]], h['len'][bad[0]], h['piles'][bad[0]])
    assert _abi.lib().cs_debug_mahjong_hu(None, None, None, 1, None, None) == -1


def test_raw_side_matches_reference():
    d = gr.load('raw_mahjong')
    streams = [json.loads(s) for s in d['streams']]
    env, cur = None, -1
    for k in range(len(d['kind'])):
        si, kind, act = int(d['stream'][k]), int(d['kind'][k]), int(d['act'][k])
        if si != cur:
            s = streams[si]
            env = rlcard_amd.make(s['env_id'], dict(s['config'], seed=s['seed']))
            assert env.state_shape == [[6, 34, 4]] * 4 and env.action_shape == [None] * 4 and env.num_actions == 38
            cur = si
        if kind == 0:
            state, player = env.reset()
        elif kind == 1:
            state, player = env.step(act)
        else:
            state, player = env.get_state(act), act
        where = 'event %d (stream %d, kind %d, act %d)' % (k, si, kind, act)
        assert player == int(d['player'][k]) and int(env.is_over()) == int(d['done'][k]), where
        assert state['obs'].shape == (6, 34, 4) and state['obs'].dtype == np.int64, where
        assert rawcanon.dumps(raw_view(state)) == d['state'][k], where
        if d['payoffs'][k]:
            assert rawcanon.dumps(env.get_payoffs()) == d['payoffs'][k], where
    card = state['raw_obs']['current_hand'][0]
    assert card.get_str() == '%s-%s' % (card.type, card.trait) and 0 <= card.index_num < 9
    with pytest.raises(NotImplementedError):
        env.get_perfect_information()


def test_env_run_with_agents_and_illegal_ids():
    from rlcard_amd.agents import RandomAgent
    env = rlcard_amd.make('mahjong', {'seed': 5})
    env.set_agents([RandomAgent(num_actions=env.num_actions) for _ in range(4)])
    traj, payoffs = env.run(is_training=False)
    assert payoffs.dtype == np.int64 and sorted(payoffs.tolist()) in ([-1, -1, -1, 1], [0, 0, 0, 0])
    assert len(traj) == 4 and all(isinstance(t[-1], dict) for t in traj)
    state, _ = env.reset()
    env.step(STAND)   # no claim is on offer after the deal: an illegal id plays the lowest legal id
    assert env.action_recorder[-1][1].get_str() == mahjong.ACTION_LIST[min(state['legal_actions'])]


STAND = 37


# ---- the rollout against the step API ------------------------------------------------------------------------------
@pytest.mark.parametrize('n', [65, 257])
def test_rollout_equals_the_step_api(n):
    roll = random_rollout(n)
    lg = legal_u64(roll['legal'])
    assert ((lg >> roll['action'].astype(np.uint64)) & np.uint64(1)).all()   # every action is legal in its row
    obs = roll['obs'].reshape(T, n, 6, 34, 4)
    assert obs.max() == 1 and (np.diff(obs.astype(np.int8), axis=4) <= 0).all()
    assert roll['reward'].shape == (T, n, 4) and roll['final_obs'].shape == (T, n, 4, 816)
    walk(roll, n)


def test_random_games_finish_inside_the_launches():
    games = random_rollout(257)['done'].sum(axis=0)
    assert (games >= 1).mean() >= 0.99


def test_unstaged_fallback_and_serial_refill_give_the_same_rollout():
    a = random_rollout(65)
    for flags in (2, 1):   # bit 1: one global load per draw; bit 0: every block crossing refills in its own lane
        b = _rollout(65, flags=flags)
        for k in a:
            assert np.array_equal(a[k], b[k]), (k, flags)


def test_random_policy_actions_are_the_rollouts_pick():
    n = 65
    roll = random_rollout(n)
    v = VecEnv('mahjong', n, seed=SEED, device=0)
    v.reset()
    alive = np.ones(n, bool)
    for t in range(12):
        a = v.policy_actions('random', policy_seed=PSEED, t=t).cpu().numpy()
        assert np.array_equal(a[alive], roll['action'][t][alive].astype(np.int32)), t
        alive &= roll['done'][t] == 0
        acts = np.where(a < 0, 0, a).astype(np.int32)
        v.step(torch.from_numpy(acts).cuda())
    assert alive.sum() > n // 2


# ---- state and streams ---------------------------------------------------------------------------------------------
def test_philox_mode_is_deterministic_and_another_stream():
    a = _rollout(65, config={'rng_mode': 'philox'})
    b = _rollout(65, config={'rng_mode': 'philox'})
    for k in a:
        assert np.array_equal(a[k], b[k]), k
    assert a['done'].any()
    assert not np.array_equal(a['obs'], random_rollout(65)['obs'])


def test_state_save_and_load_in_the_middle_of_a_rollout():
    n = 65
    roll = random_rollout(n)
    v = VecEnv('mahjong', n, seed=SEED, device=0)
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
    assert v.env_state_words(3) == words and len(words) == 55


def test_step_back_restores_every_level():
    env = rlcard_amd.make('mahjong', {'seed': 9, 'allow_step_back': True})
    state, player = env.reset()
    assert env.step_back() is False
    levels = []
    rng = np.random.RandomState(4)

    def view_of(st):   # (action_record is the env's, which step_back does not rewind -- as in the reference)
        return rawcanon.dumps({k: x for k, x in raw_view(st).items() if k != 'action_record'})

    for _ in range(30):
        if env.is_over():
            break
        levels.append((list(env._state_words()), view_of(state), state['obs'].copy(), player))
        state, player = env.step(int(rng.choice(list(state['legal_actions']))))
    assert len(levels) >= 10
    for words, view, obs, who in reversed(levels):
        state, player = env.step_back()
        assert env._vec.env_state_words(0) == words and player == who
        assert view_of(state) == view and np.array_equal(state['obs'], obs)
    assert env.step_back() is False


def encode_words(deck, table, hands, piles, current, last, before, valid):
    """The packed state words of cs_mahjong.h from ordered tile lists (the inverse of mahjong.decode_words)."""
    b = np.zeros(216, np.uint8)
    b[:len(deck)] = deck
    for i, t in enumerate(table):
        b[135 - i] = t
    for p in range(4):
        b[136 + 16 * p:136 + 16 * p + len(hands[p])] = hands[p]
        b[136 + 16 * p + 14] = len(hands[p])
        b[136 + 16 * p + 15] = len(piles[p])
        for k, (kind, top) in enumerate(piles[p]):
            b[200 + 4 * p + k] = kind << 6 | top
    meta = len(deck) | len(table) << 8 | current << 16 | last << 18 | before << 20 | valid << 22
    return [int(x) for x in b.view('<u4')] + [meta]


def test_constructed_states_one_step_from_a_win():
    v = VecEnv('mahjong', 2, seed=1, device=0)
    v.reset()
    # env 0: player 0 discards winds-south (33), nobody holds a pair of it; player 1 draws bamboo-3 (2) off the deck's
    # end and holds 1 2 3 / 4 5 6 / 7 8 9 of bamboo, three dragons-red and a pair of winds-east: a win by hand
    hand1 = [0, 1, 3, 4, 5, 6, 7, 8, 28, 28, 28, 30, 30]
    hands = [[33] + [9, 11, 13, 15, 17, 18, 20, 22, 24, 26, 27, 29, 31], hand1,
             [10, 12, 14, 16, 19, 21, 23, 25, 27, 29, 31, 32, 32], [9, 11, 13, 15, 17, 18, 20, 22, 24, 26, 10, 12, 14]]
    w0 = encode_words([16, 19, 2], [], hands, [[], [], [], []], 0, 0, 0, 0)
    # env 1: pong of dots-5 (22) is on offer to player 2, who has three piles: the fourth pile wins
    hands = [[0, 2, 4, 6, 8, 10, 12, 14, 16, 27, 28, 29, 30], [1, 3, 5, 7, 9, 11, 13, 15, 17, 19, 21, 23, 25],
             [22, 31, 22, 33], [0, 2, 4, 6, 8, 10, 12, 14, 16, 18, 20, 24, 26]]
    piles = [[], [], [(mahjong.V_PONG, 32), (mahjong.V_GONG, 5), (mahjong.V_CHOW, 9)], []]
    w1 = encode_words([1, 3, 5, 7], [32, 5, 9, 22], hands, piles, 2, 0, 0, mahjong.V_PONG)
    v.set_env_state_words(0, w0)
    v.set_env_state_words(1, w1)
    s1 = mahjong.decode_words(w1)
    assert s1['piles'][2][2] == (2, 9) and mahjong.claim_tiles(2, 9) == [10, 11, 9] and s1['valid_act'] == 1
    seen = _np(v.observe(2))
    assert legal_u64(seen['legal'])[1] == (1 << 34 | 1 << 37) and seen['player'][1] == 2 and not seen['done'].any()
    assert legal_u64(seen['legal'])[0] == sum(1 << t for t in set(w for w in mahjong.decode_words(w0)['hands'][0]))
    out = _np(v.step([33, 34]))
    assert out['done'].tolist() == [1, 1]
    assert out['reward'].tolist() == [[-1, 1, -1, -1], [-1, -1, 1, -1]]
    s0, s1 = (mahjong.decode_words(v.env_state_words(e)) for e in (0, 1))
    assert s0['hands'][1] == hand1 + [2] and s0['table'] == [33] and s0['deck'] == [16, 19] and s0['current'] == 1
    assert s1['hands'][2] == [31, 33] and s1['piles'][2][3] == (1, 22) and s1['table'][-1] == 22   # the table keeps it
    obs = _np(v.observe(2))['obs'].reshape(2, 6, 34, 4)
    assert obs[1, 4, 22].tolist() == [1, 1, 1, 0] and obs[1, 4, 5].tolist() == [1, 1, 1, 1]
    assert obs[1, 4, 9:12, 0].tolist() == [1, 1, 1] and obs[1, 0].sum() == 2 and obs[1, 1].sum() == 4


def test_state_words_that_hold_no_tiles_are_a_finished_game():
    """cs_set_env_state's words are the caller's: a deck, table or hand byte that is no tile, or lists that do not fit,
    load as a finished game (the next step deals), so no id past 33 ever reaches a hand or a legal mask."""
    hands = [[0, 2, 4, 6, 8, 10, 12, 14, 16, 27, 28, 29, 30, 33], [1, 3, 5, 7, 9, 11, 13, 15, 17, 19, 21, 23, 25],
             [18, 20, 22, 24, 26, 31, 32, 0, 2, 4, 6, 8, 10], [1, 3, 5, 7, 9, 11, 13, 15, 17, 19, 21, 23, 25]]
    good = encode_words([1, 3, 5, 7], [32, 5], hands, [[], [], [], []], 0, 0, 0, 0)
    bad = {'deck byte': encode_words([1, 3, 34, 7], [32, 5], hands, [[], [], [], []], 0, 0, 0, 0),
           'table byte': encode_words([1, 3, 5, 7], [32, 200], hands, [[], [], [], []], 0, 0, 0, 0),
           'hand byte': encode_words([1, 3, 5, 7], [32, 5], [[40] + hands[0][1:]] + hands[1:], [[], [], [], []], 0, 0, 0,
                                     0),
           'lists too long': encode_words(list(range(34)) * 4, [32, 5], hands, [[], [], [], []], 0, 0, 0, 0)}
    v = VecEnv('mahjong', 1 + len(bad), seed=3, device=0)
    v.reset()
    v.set_env_state_words(0, good)
    for e, words in enumerate(bad.values()):
        v.set_env_state_words(1 + e, words)
    seen = _np(v.observe(0))
    assert seen['done'].tolist() == [0] + [1] * len(bad), list(bad)
    assert legal_u64(seen['legal'])[0] == sum(1 << t for t in set(hands[0]))
    out = _np(v.step([33] * (1 + len(bad))))   # env 0 discards; the others deal a new game
    assert not out['done'].any() and (out['player'][1:] == 0).all()
    assert (out['obs'].reshape(-1, 6, 34, 4)[1:, 0].sum(axis=(1, 2)) == 14).all()
    assert (legal_u64(out['legal']) < (1 << 38)).all()


def test_refusals():
    cfg = _abi.Config(3, -1, 0, 0, 0)
    h = C.c_void_p()
    assert _abi.lib().cs_create(C.byref(h), 6, 8, 0, C.byref(cfg)) == -4
    assert _abi.lib().cs_last_error().startswith(b'mahjong: game_num_players must be 4')
    with pytest.raises(ValueError):
        rlcard_amd.make('mahjong', {'game_num_players': 3})
    v = VecEnv('mahjong', 65, seed=1, device=0)
    with pytest.raises(_abi.CardsimError, match='CS_E_UNSUPPORTED'):
        v.policy_actions(1)
    with pytest.raises(_abi.CardsimError, match='CS_E_UNSUPPORTED'):
        v.rollout(4, out=v.new_traj_out(4, select=1), policies=[1, 'random', 'random', 'random'])


# ---- tournament ----------------------------------------------------------------------------------------------------
def test_tournament_sums_equal_the_payoff_rows():
    """Windows of HALF steps, as tournament_vec rolls them: the device's sums against the payoff rows summed here."""
    n = 65
    v = VecEnv('mahjong', n, seed=SEED, device=0)
    acc, out = v.new_payoff_sums(), v.new_traj_out(HALF, select=1)
    total, first, games = np.zeros(4), np.zeros(4), 0
    have = np.zeros(n, bool)
    for w in range(8):
        t = _np(v.rollout(HALF, policy_seed=PSEED, t0=w * HALF, out=out, policies=['random'] * 4))
        v.payoff_sums(out, acc, quota=0)
        if w < T // HALF:   # random seats play the plain rollout's games
            assert np.array_equal(t['action'], random_rollout(n)['action'][w * HALF:(w + 1) * HALF])
        done = t['done'] != 0
        total += t['reward'][done].astype(np.float64).sum(axis=0)
        games += int(done.sum())
        for e in np.nonzero(~have & done.any(axis=0))[0]:
            first += t['reward'][int(np.argmax(done[:, e])), e]
            have[e] = True
        if have.all():
            break
    assert have.all() and int(acc['games'].item()) == games >= n
    assert acc['sums'].cpu().numpy().tolist() == total.tolist()   # payoffs are integers: the sums are exact
    v = VecEnv('mahjong', n, seed=SEED, device=0)
    pay = tournament_vec(v, ['random'] * 4, games_per_env=1, T=HALF, policy_seed=PSEED)
    assert len(pay) == 4 and np.array_equal(np.asarray(pay), first / n)
