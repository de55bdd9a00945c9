"""Gin Rummy on the HIP engine against the reference's recorded streams (tests/golden/gin_rummy.npz,
gin_rummy_melds.npz, raw_gin_rummy.npz) and against itself: the fused rollout row by row against the step API, the
two-word legal rows, the judge hook, the novice rule by candidate set, state save / load, Philox mode, constructed
states, refusals and the tournament sums. Shapes: 65 envs (one wave plus one lane) and 257 (more than one 256-thread
block), T = 192 as two chained launches of 96: the reference's longest uniform-random game took 168 steps
(cov_max_uniform), rounded up to a multiple of 32."""
import ctypes as C
import json

import numpy as np
import pytest

import golden_replay as gr
import rawcanon
import rlcard_amd
from rlcard_amd import VecEnv, _abi, models
from rlcard_amd.envs import gin_rummy
from rlcard_amd.models.gin_rummy_rule_models import GinRummyNoviceRuleAgent
from rlcard_amd.utils import tournament_vec
from test_gin_rummy import raw_view

torch = pytest.importorskip('torch')
pytestmark = pytest.mark.gpu

T, HALF, SEED, PSEED = 192, 96, 700, 29
KEYS = ('obs', 'legal', 'player', 'action', 'reward', 'done')
NOVICE = 'gin-rummy-novice-rule'


@pytest.fixture(scope='module', autouse=True)
def _need_gpu():
    if not torch.cuda.is_available():
        pytest.fail('GPU tests need a visible GPU (run them on the MI355X box)')


def _np(o):
    return {k: v.cpu().numpy() for k, v in o.items()}


def _rollout(n, flags=0, config=None, pseed=PSEED, policies=None, game='gin-rummy', steps=T, half=HALF):
    """`steps` steps as launches of `half` with t0 carried -> numpy trajectory [steps, n, ...] with final_obs"""
    v = VecEnv(game, n, seed=SEED, device=0, config=config)
    if flags:
        v.set_kernel_flags(flags)
    parts = []
    for k in range(steps // half):
        out = v.new_traj_out(half, final_obs=True, select=1)
        parts.append(_np(v.rollout(half, policy_seed=pseed, t0=k * half, out=out, policies=policies)))
    return {k: np.concatenate([p[k] for p in parts]) for k in parts[0]}


_cache = {}


def random_rollout(n):
    if n not in _cache:
        _cache[n] = _rollout(n)
    return _cache[n]


def legal_bits(rows):
    """uint8 [..., LB] -> 0/1 [..., 8 LB]"""
    return np.unpackbits(rows, axis=-1, bitorder='little')


def walk(roll, n, game='gin-rummy', steps=T):
    """Steps a second VecEnv with the rollout's own action rows and compares every row. Env e consumes row cursor[e];
    an env whose game ended takes one lazy-reset step that consumes no row."""
    v = VecEnv(game, n, seed=SEED, device=0)
    view = _np(v.reset())
    cursor = np.zeros(n, np.int64)
    pending = view['done'] != 0
    assert not pending.any()
    idx = np.arange(n)
    ticks = 0
    while (cursor < steps).any():
        act = (cursor < steps) & ~pending
        c, e = cursor[act], idx[act]
        for k in ('obs', 'legal', 'player'):
            assert np.array_equal(view[k][e], roll[k][c, e]), (k, ticks)
        actions = np.zeros(n, np.int32)
        actions[e] = roll['action'][c, e]
        view = _np(v.step(torch.from_numpy(actions).cuda()))
        assert np.array_equal(view['reward'][e].view(np.uint32), roll['reward'][c, e].view(np.uint32)), ticks
        assert np.array_equal(view['done'][e], roll['done'][c, e]), ticks
        ended = e[view['done'][e] != 0]
        if len(ended):
            for p in range(v.num_players):
                fin = v.observe(p)['obs'].cpu().numpy()
                assert np.array_equal(fin[ended], roll['final_obs'][cursor[ended], ended, p]), (p, ticks)
        cursor[act] += 1
        pending = np.zeros(n, bool)
        pending[ended] = True
        ticks += 1
        assert ticks < 3 * steps
    return v


class One:
    def __init__(self, ei, seed):
        self.v = VecEnv('gin-rummy', 1, seeds=[seed], device=0)

    def reset(self):
        return {k: x[0] for k, x in _np(self.v.reset()).items()}

    def step(self, a):
        return {k: x[0] for k, x in _np(self.v.step([a])).items()}

    def observe(self, p):
        o = _np(self.v.observe(p))
        return o['obs'][0], o['legal'][0]


# ---- the reference's streams ---------------------------------------------------------------------------------------
def test_single_env_replays_reference_stream():
    """the first seeds of every steering mode through a one-env handle (the whole fixture runs batched, below)"""
    d = gr.load('gin_rummy')
    keep = d['ev_env'] < 12
    part = gr.Fixture({k: (x[keep] if k.startswith('ev_') and len(x) == len(keep) else x) for k, x in d.items()})
    assert gr.replay(part, One, 110) == int(keep.sum())


def test_batched_replay_with_lazy_reset_and_recorded_novice_candidates():
    """All fixture seeds as one batch; a 'reset' event after a finished game is a step with any action. At every event
    the device's novice rule answers an id of the set the reference would choose from."""
    d = gr.load('gin_rummy')
    seeds = [int(s) for s in d['seeds']]
    n = len(seeds)
    v = VecEnv('gin-rummy', n, seeds=seeds, device=0)
    per_env = [np.nonzero(d['ev_env'] == i)[0] for i in range(n)]
    ptr, cand = d['ev_cand_ptr'], d['ev_cand_ids']
    out = _np(v.reset())
    for tick in range(max(len(x) for x in per_env)):
        if tick > 0:
            acts = np.zeros(n, np.int32)
            for i, ev in enumerate(per_env):
                if tick < len(ev) and d['ev_kind'][ev[tick]] == 1:
                    acts[i] = d['ev_act'][ev[tick]]
            out = _np(v.step(torch.from_numpy(acts).cuda()))
        rule = v.policy_actions(NOVICE, policy_seed=tick, t=tick).cpu().numpy()
        for i, ev in enumerate(per_env):
            if tick >= len(ev):
                continue
            k = ev[tick]
            assert np.array_equal(out['obs'][i], d['ev_obs'][k]), (i, tick)
            assert np.array_equal(out['legal'][i], d['ev_legal'][k]), (i, tick)
            assert out['player'][i] == d['ev_player'][k] and out['done'][i] == d['ev_done'][k], (i, tick)
            if d['ev_done'][k]:
                assert np.array_equal(out['reward'][i], d['ev_payoff'][k].astype(np.float32)), (i, tick)
                assert rule[i] == -1
            else:
                assert rule[i] in cand[ptr[k]:ptr[k + 1]], (i, tick, rule[i], cand[ptr[k]:ptr[k + 1]])


def judge_on_device(hands, ln):
    n = len(ln)
    h = torch.from_numpy(np.ascontiguousarray(hands)).cuda()
    l_ = torch.from_numpy(np.ascontiguousarray(ln)).cuda()
    dw = torch.full((n,), -7, dtype=torch.int32, device='cuda')
    card = torch.full((n,), -7, dtype=torch.int32, device='cuda')
    knock = torch.full((n,), -1, dtype=torch.int64, device='cuda')
    gin = torch.full((n,), -1, dtype=torch.int64, device='cuda')
    _abi.check(_abi.lib().cs_debug_gin_melds(*[C.c_void_p(x.data_ptr()) for x in (h, l_)], n,
                                             *[C.c_void_p(x.data_ptr()) for x in (dw, knock, gin, card)], None),
               'cs_debug_gin_melds')
    torch.cuda.synchronize()
    return (dw.cpu().numpy(), knock.cpu().numpy().view(np.uint64), gin.cpu().numpy().view(np.uint64), card.cpu().numpy())


def test_judge_hook_matches_the_reference():
    m = gr.load('gin_rummy_melds')
    dw, knock, gin, card = judge_on_device(m['hands'], m['len'])
    for got, key in ((dw, 'deadwood'), (knock, 'knock'), (gin, 'gin'), (card, 'gin_card')):
        bad = np.nonzero(got != m[key])[0]
        assert len(bad) == 0, (key, bad[:10], m['hands'][bad[0]], got[bad[0]], m[key][bad[0]])
    assert _abi.lib().cs_debug_gin_melds(None, None, 1, None, None, None, None, None) == -1


def test_raw_side_matches_reference():
    d = gr.load('raw_gin_rummy')
    streams = [json.loads(s) for s in d['streams']]
    env, cur = None, -1
    for k in range(len(d['kind'])):
        si, kind, act = int(d['stream'][k]), int(d['kind'][k]), int(d['act'][k])
        if si != cur:
            s = streams[si]
            env = rlcard_amd.make(s['env_id'], dict(s['config'], seed=s['seed']))
            assert env.state_shape == [[5, 52]] * 2 and env.action_shape == [None] * 2 and env.num_actions == 110
            cur = si
        if kind == 0:
            state, player = env.reset()
        elif kind == 1:
            state, player = env.step(act)
        else:
            state, player = env.get_state(act), act
        where = 'event %d (stream %d, kind %d, act %d)' % (k, si, kind, act)
        assert player == int(d['player'][k]) and int(env.is_over()) == int(d['done'][k]), where
        assert state['obs'].shape == (5, 52) and state['obs'].dtype == np.int64, where
        assert rawcanon.dumps(raw_view(state)) == d['state'][k], where
        if d['payoffs'][k]:
            assert rawcanon.dumps(env.get_payoffs()) == d['payoffs'][k], where
        if not env.is_over():   # the host form of the novice rule chooses from the reference's set
            assert sorted(int(a) for a in GinRummyNoviceRuleAgent.candidates(state)) == json.loads(str(d['candidates'][k])), where
    with pytest.raises(NotImplementedError):
        env.get_perfect_information()
    with pytest.raises(NotImplementedError):
        env.step_back()


def test_env_run_with_agents_and_illegal_ids():
    from rlcard_amd.agents import RandomAgent
    env = rlcard_amd.make('gin-rummy', {'seed': 5})
    env.set_agents([RandomAgent(num_actions=env.num_actions), models.load(NOVICE).agents[1]])
    traj, payoffs = env.run(is_training=False)
    assert payoffs.dtype == np.float64 and payoffs.shape == (2,) and -1.0 <= payoffs.min() and payoffs.max() <= 1.0
    assert len(traj) == 2 and all(isinstance(t[-1], dict) and not t[-1]['obs'].any() for t in traj)
    state, _ = env.reset()
    assert env.get_payoffs().tolist() == [0, 0] and env.get_payoffs().dtype == np.int64
    env.step(0)   # `score north` is not legal after the deal: an illegal id plays the lowest legal id
    assert env.action_recorder[-1][1].action_id == min(state['legal_actions'])
    assert str(env.action_recorder[-1][1]) == str(gin_rummy.ACTION_LIST[min(state['legal_actions'])])


# ---- the rollout against the step API ------------------------------------------------------------------------------
@pytest.mark.parametrize('n', [65, 257])
def test_rollout_equals_the_step_api(n):
    roll = random_rollout(n)
    lg = legal_bits(roll['legal'])
    assert roll['legal'].shape == (T, n, 14) and not lg[..., 110:].any()   # bits 110 and 111 are always clear
    assert np.take_along_axis(lg, roll['action'][..., None].astype(np.int64), axis=-1).all()   # every action is legal
    assert (roll['action'] >= 64).any()   # ids of the mask's second word are played
    obs = roll['obs'].reshape(T, n, 5, 52)
    assert obs.max() == 1 and (obs.sum(axis=2) <= 1).all() and set(np.unique(obs[:, :, 0].sum(axis=2))) == {10, 11}
    assert roll['reward'].shape == (T, n, 2) and roll['final_obs'].shape == (T, n, 2, 260) and not roll['final_obs'].any()
    walk(roll, n)


def test_obs_rows_at_every_alignment():
    """260-byte rows are stored 16 bytes at a time from the row's own 16-byte boundary on, with dwords before and after
    it, and byte by byte into a tensor that is not dword aligned: the reset rows at every offset are the aligned ones"""
    n = 65
    want = _np(VecEnv('gin-rummy', n, seed=SEED, device=0).reset())['obs']
    assert want.reshape(n, 5, 52)[:, 0].sum(axis=1).tolist() == [11] * n
    for off in (1, 2, 4, 8, 12, 15):
        v = VecEnv('gin-rummy', n, seed=SEED, device=0)
        out = v.new_step_out()
        base = torch.full((n * 260 + 32,), 7, dtype=torch.uint8, device='cuda')
        out['obs'] = base[off:off + n * 260].view(n, 260)
        v.reset(out=out)
        got = base.cpu().numpy()
        assert np.array_equal(got[off:off + n * 260].reshape(n, 260), want), off
        assert (got[:off] == 7).all() and (got[off + n * 260:] == 7).all(), off   # nothing outside the rows


def test_an_existing_games_rollout_still_equals_the_step_api():
    """Leduc, 257 envs x 64 steps: the skeleton's legal-mask and obs-row paths as the games before Gin Rummy take them"""
    roll = _rollout(257, game='leduc-holdem', steps=64, half=32)
    assert roll['done'].any()
    walk(roll, 257, game='leduc-holdem', steps=64)


def test_random_games_finish_inside_the_launches():
    games = random_rollout(257)['done'].sum(axis=0)
    assert (games >= 1).all()


def test_unstaged_fallback_and_serial_refill_give_the_same_rollout():
    a = random_rollout(65)
    for flags in (2, 1):   # bit 1: one global load per draw; bit 0: every block crossing refills in its own lane
        b = _rollout(65, flags=flags)
        for k in a:
            assert np.array_equal(a[k], b[k]), (k, flags)


def test_random_policy_actions_are_the_rollouts_pick():
    n = 65
    roll = random_rollout(n)
    v = VecEnv('gin-rummy', n, seed=SEED, device=0)
    v.reset()
    alive = np.ones(n, bool)
    for t in range(40):
        a = v.policy_actions('random', policy_seed=PSEED, t=t).cpu().numpy()
        assert np.array_equal(a[alive], roll['action'][t][alive].astype(np.int32)), t
        alive &= roll['done'][t] == 0
        acts = np.where(a < 0, 0, a).astype(np.int32)
        v.step(torch.from_numpy(acts).cuda())
    assert alive.sum() > n // 2
    # ids of the mask's second word: every env one draw from a hand with five knocks among its 16 legal ids
    h1 = MELDED9 + [CL + 0]
    loose, stock, disc = deal_rest(h1, CL + 1, 9)
    for e in range(n):
        v.set_env_state_words(e, encode_words(stock, disc, [h1, loose]))
    v.step([2] * n)
    a = v.policy_actions('random', policy_seed=PSEED, t=7).cpu().numpy()
    one = _np(v.rollout(1, policy_seed=PSEED, t0=7, out=v.new_traj_out(1, select=1)))
    assert np.array_equal(a, one['action'][0].astype(np.int32)) and (a >= 64).any() and (a < 58).any()
    assert set(a[a >= 58].tolist()) <= {58 + c for c in (S + 0, S + 1, S + 2, CL + 0, CL + 1)}


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
    v = VecEnv('gin-rummy', n, seed=SEED, device=0)
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
    assert v.env_state_words(3) == words and len(words) == 29


def encode_words(stock, discard, hands, known=((), ()), current=0, dealer=0, last=gin_rummy.L_DISCARD, picked=0,
                 moves=10):
    """The packed state words of cs_gin_rummy.h from ordered card lists (the inverse of gin_rummy.decode_words); the
    judge's words are left zero, which is right wherever the current player holds 10 cards."""
    b = np.zeros(100, np.uint8)
    b[:len(stock)] = stock
    for i, c in enumerate(discard):
        b[51 - i] = c
    for p in range(2):
        b[52 + 12 * p:52 + 12 * p + len(hands[p])] = hands[p]
        b[76 + 12 * p:76 + 12 * p + len(known[p])] = known[p]
    cnt = (len(stock) | len(discard) << 6 | len(hands[0]) << 12 | len(hands[1]) << 16 | len(known[0]) << 20 |
           len(known[1]) << 24)
    meta = current | dealer << 1 | last << 2 | picked << 6 | moves << 12
    return [int(x) for x in b.view('<u4')] + [cnt, meta, 0, 0]


S, H, D, CL = 0, 13, 26, 39   # suit bases: card id = rank + 13 * suit
MELDED9 = [S + 0, S + 1, S + 2, H + 4, H + 5, H + 6, D + 8, D + 9, D + 10]


def deal_rest(hand0, top, stock_n):
    """hand 1 (ten cards that meld nothing), a stock of stock_n cards ending in `top`, the rest as the discard pile"""
    loose = [c for c in (S + 4, H + 8, D + 1, CL + 5, S + 7, H + 11, D + 4, CL + 9, S + 10, H + 1, D + 6, CL + 12, S + 12)
             if c not in hand0 and c != top][:10]
    assert gin_rummy.best_deadwood(loose) == sum(gin_rummy.card_value(c) for c in loose)
    rest = [c for c in range(52) if c not in hand0 and c not in loose and c != top]
    return loose, rest[:stock_n - 1] + [top], rest[stock_n - 1:]


def test_constructed_states_one_step_from_each_ending():
    melded9 = MELDED9
    v = VecEnv('gin-rummy', 4, seed=1, device=0)
    v.reset()
    # env 0: ten melded cards, the draw is the king of clubs: gin alone is legal, and the king is the card that goes
    h0 = melded9 + [D + 11]
    loose, stock, disc = deal_rest(h0, CL + 12, 9)
    v.set_env_state_words(0, encode_words(stock, disc, [h0, loose]))
    # env 1: nine melded cards and the ace of clubs, the draw is the two of clubs: 3 deadwood, both may knock
    h1 = melded9 + [CL + 0]
    loose1, stock1, disc1 = deal_rest(h1, CL + 1, 9)
    v.set_env_state_words(1, encode_words(stock1, disc1, [h1, loose1]))
    # env 2: two cards of stock left after a discard: dead hand or pick up. env 3: 200 moves: dead hand alone
    loose2, stock2, disc2 = deal_rest(h0, CL + 12, 2)
    v.set_env_state_words(2, encode_words(stock2, disc2, [h0, loose2], current=1))
    v.set_env_state_words(3, encode_words(stock, disc, [h0, loose], moves=200))
    seen = _np(v.observe(0))
    ids = [np.nonzero(r)[0].tolist() for r in legal_bits(seen['legal'])]
    assert ids == [[2, 3], [2, 3], [3, 4], [4]] and seen['player'].tolist() == [0, 0, 1, 0] and not seen['done'].any()
    out = _np(v.step([2, 2, 4, 4]))
    ids = [np.nonzero(r)[0].tolist() for r in legal_bits(out['legal'])]
    assert ids[0] == [5] and ids[2] == [0] and ids[3] == [0] and out['player'].tolist() == [0, 0, 0, 0]
    # (the knock set is the reference's: a cluster of two melds leaves A 2 3 of spades as deadwood of 9 with the clubs)
    knock, can_gin = gin_rummy.going_out_memo(h1 + [CL + 1])
    assert not can_gin and sorted(knock) == [S + 0, S + 1, S + 2, CL + 0, CL + 1]
    assert ids[1] == sorted(6 + c for c in h1 + [CL + 1]) + sorted(58 + c for c in knock)
    out = _np(v.step([5, 58 + CL + 1, 0, 0]))
    assert [np.nonzero(r)[0].tolist() for r in legal_bits(out['legal'])] == [[0], [0], [1], [1]]
    s0, s1 = (gin_rummy.decode_words(v.env_state_words(e)) for e in (0, 1))
    assert s0['hands'][0] == h0 and s0['gone'] == CL + 12 and s0['go_kind'] == gin_rummy.GO_GIN
    assert s1['hands'][0] == h1 and s1['gone'] == CL + 1 and s1['go_kind'] == gin_rummy.GO_KNOCK
    assert out['obs'].reshape(4, 5, 52)[:2].sum(axis=(1, 2)).tolist() == [51, 51]   # the card is nowhere
    out = _np(v.step([0, 0, 1, 1]))
    assert out['done'].tolist() == [0, 0, 1, 1] and out['player'].tolist() == [1, 1, 1, 1]
    dw = lambda cards: np.float32(-gin_rummy.best_deadwood(cards) / 100)   # noqa: E731
    assert out['reward'][2].tolist() == [dw(h0), dw(loose2)] and out['reward'][3].tolist() == [dw(h0), dw(loose)]
    assert dw(h0) == 0 and not np.signbit(out['reward'][3][0])
    out = _np(v.step([1, 1, 0, 0]))   # envs 2 and 3 deal their next game
    assert out['done'].tolist() == [1, 1, 0, 0] and not out['obs'][:2].any() and not out['legal'][:2].any()
    assert out['reward'][0].tolist() == [1.0, dw(loose)] and out['reward'][1].tolist() == [np.float32(0.2), dw(loose1)]
    assert (out['obs'].reshape(4, 5, 52)[2:, 0].sum(axis=1) == 11).all()


def test_state_words_that_hold_no_game_are_a_finished_game():
    """cs_set_env_state's words are the caller's: counts that do not add to 52, a byte that is no card or a card held
    twice load as a finished game (the next step deals), so no list leaves its region."""
    h0 = [S + 0, S + 1, S + 2, H + 4, H + 5, H + 6, D + 8, D + 9, D + 10, D + 11]
    loose, stock, disc = deal_rest(h0, CL + 12, 9)
    good = encode_words(stock, disc, [h0, loose])
    bad = {'counts': encode_words(stock[:-1], disc, [h0, loose]),
           'no card': encode_words([60] + stock[1:], disc, [h0, loose]),
           'twice': encode_words([stock[1]] + stock[1:], disc, [h0, loose]),
           'hand too long': encode_words(stock[:5], disc, [h0 + stock[5:], loose]),
           'known not held': encode_words(stock, disc, [h0, loose], known=([stock[0]], []))}
    v = VecEnv('gin-rummy', 1 + len(bad), seed=3, device=0)
    v.reset()
    v.set_env_state_words(0, good)
    for e, words in enumerate(bad.values()):
        v.set_env_state_words(1 + e, words)
    seen = _np(v.observe(0))
    assert seen['done'].tolist() == [0] + [1] * len(bad), list(bad)
    assert not seen['obs'][1:].any() and not seen['legal'][1:].any()
    out = _np(v.step([2] * (1 + len(bad))))   # env 0 draws; the others deal a new game
    assert not out['done'].any()
    assert (out['obs'].reshape(-1, 5, 52)[:, 0].sum(axis=1) == 11).all() and not legal_bits(out['legal'])[:, 110:].any()


# ---- the novice rule -------------------------------------------------------------------------------------------------
def candidates_of(obs_row, legal_row):
    ids = np.nonzero(legal_bits(legal_row)[:110])[0].tolist()
    return GinRummyNoviceRuleAgent.candidates({'legal_actions': dict.fromkeys(ids), 'obs': obs_row.reshape(5, 52)})


@pytest.mark.parametrize('seats', [(NOVICE, 'random'), (NOVICE, NOVICE)])
def test_rollout_with_the_novice_rule(seats):
    n, steps = 65, 96
    roll = _rollout(n, policies=list(seats), steps=steps, half=steps)
    plain = random_rollout(n)
    rule_seat = np.array([s == NOVICE for s in seats])[roll['player']]
    # a random seat picks what the plain rollout picks while the games are the same: the first row
    assert np.array_equal(roll['obs'][0], plain['obs'][0])
    lg = legal_bits(roll['legal'])
    assert np.take_along_axis(lg, roll['action'][..., None].astype(np.int64), axis=-1).all()
    chosen = {}   # (size of the candidate set, position of the choice in it) -> count
    knocks = 0
    for t in range(steps):
        for e in range(n):
            if not rule_seat[t, e]:
                continue
            a = int(roll['action'][t, e])
            ids = np.nonzero(lg[t, e][:110])[0]
            if (ids >= 58).any():     # every knock-capable state knocks
                assert a >= 58, (t, e, a)
                knocks += 1
            if t < 48 or (ids >= 58).any():
                cand = sorted(candidates_of(roll['obs'][t, e], roll['legal'][t, e]))
                assert a in cand, (t, e, a, cand)
                chosen[(len(cand), cand.index(a))] = chosen.get((len(cand), cand.index(a)), 0) + 1
    assert knocks > 0 and (roll['reward'] == np.float32(0.2)).any()
    # over many rows every candidate of a set is chosen (a uniform pick misses one of k in m rows with chance
    # (1 - 1 / k) ** m: below 1e-5 from 30 rows of two and 40 rows of three on)
    for size, rows in ((2, 30), (3, 40)):
        if sum(chosen.get((size, k), 0) for k in range(size)) >= rows:
            assert all(chosen.get((size, k), 0) > 0 for k in range(size)), chosen
    assert sum(chosen.get((2, k), 0) for k in range(2)) >= 30 and roll['done'].any()


def test_tournament_sums_equal_the_payoff_rows():
    """Windows of HALF steps, as tournament_vec rolls them: the device's sums against the payoff rows summed here."""
    n = 65
    seats = [NOVICE, 'random']
    v = VecEnv('gin-rummy', n, seed=SEED, device=0)
    acc, out = v.new_payoff_sums(), v.new_traj_out(HALF, select=1)
    total, first, games = np.zeros(2), np.zeros(2), 0
    have = np.zeros(n, bool)
    for w in range(8):
        t = _np(v.rollout(HALF, policy_seed=PSEED, t0=w * HALF, out=out, policies=seats))
        v.payoff_sums(out, acc, quota=0)
        done = t['done'] != 0
        for tt, e in zip(*np.nonzero(done)):   # (in the device's order of addition: step, then env)
            total += t['reward'][tt, e].astype(np.float64)
        games += int(done.sum())
        for e in np.nonzero(~have & done.any(axis=0))[0]:
            first += t['reward'][int(np.argmax(done[:, e])), e].astype(np.float64)
            have[e] = True
        if have.all():
            break
    assert have.all() and int(acc['games'].item()) == games >= n
    assert np.allclose(acc['sums'].cpu().numpy(), total, rtol=0, atol=1e-9)   # f32 payoffs summed in f64, any order
    v = VecEnv('gin-rummy', n, seed=SEED, device=0)
    pay = tournament_vec(v, seats, games_per_env=1, T=HALF, policy_seed=PSEED)
    assert len(pay) == 2 and np.allclose(np.asarray(pay), first / n, rtol=0, atol=1e-9)
    assert pay[0] > pay[1]   # the rule knocks; uniform play almost never does


def test_refusals():
    cfg = _abi.Config(3, -1, 0, 0, 0)
    h = C.c_void_p()
    assert _abi.lib().cs_create(C.byref(h), 7, 8, 0, C.byref(cfg)) == -4
    assert _abi.lib().cs_last_error().startswith(b'gin-rummy: game_num_players must be 2')
    with pytest.raises(ValueError):
        rlcard_amd.make('gin-rummy', {'game_num_players': 3})
    with pytest.raises(ValueError):
        VecEnv('gin-rummy', 4, device=0, config={'game_num_players': 4})
    env = rlcard_amd.make('gin-rummy', {'seed': 1, 'allow_step_back': True})
    env.reset()
    with pytest.raises(NotImplementedError):
        env.step_back()
    v = VecEnv('gin-rummy', 65, seed=1, device=0)
    with pytest.raises(_abi.CardsimError, match='CS_E_UNSUPPORTED'):
        v.policy_actions(2)
    with pytest.raises(_abi.CardsimError, match='CS_E_UNSUPPORTED'):
        v.rollout(4, out=v.new_traj_out(4, select=1), policies=[2, 'random'])
    L = _abi.lib()
    out = C.c_void_p()
    assert L.cs_replay_create(v._h, 64, C.byref(out)) == -4 and b'110' in L.cs_last_error()
    assert L.cs_reservoir_create(v._h, 64, 1, C.byref(out)) == -4 and b'110' in L.cs_last_error()
    net = _abi.QNet()
    obs = torch.zeros((4, 260), dtype=torch.uint8, device='cuda')
    q = torch.zeros((4, 110), dtype=torch.float32, device='cuda')
    p = C.c_void_p
    assert L.cs_qnet_values(v._h, C.byref(net), p(obs.data_ptr()), None, 4, p(q.data_ptr()), None) == -4
    assert b'at most 64 actions' in L.cs_last_error()
    assert L.cs_pnet_probs(v._h, C.byref(net), p(obs.data_ptr()), None, 4, p(q.data_ptr()), None) == -4
