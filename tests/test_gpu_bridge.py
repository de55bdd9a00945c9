"""Bridge on the HIP engine against the reference's recorded streams (tests/golden/bridge.npz, raw_bridge.npz) and
against itself: the fused rollout row by row against the step API, the 573-byte obs rows at every alignment, the
unstaged and serial-refill paths, Philox mode, state save / load, constructed states one step from each ending, state
words that hold no game, the random pick, the novice rule, the tournament sums and the refusals. Shapes: 65 envs (one
wave plus one lane) and 257 (four waves plus one lane), T = 96 as two chained launches of 48 (uniform-random games took
56 to 73 steps in the reference)."""
import ctypes as C
import json

import numpy as np
import pytest

import golden_replay as gr
import rawcanon
import rlcard_amd
from rlcard_amd import VecEnv, _abi
from rlcard_amd.envs import bridge
from rlcard_amd.models.bridge_rule_models import BridgeDefenderNoviceRuleAgent
from rlcard_amd.utils import tournament_vec
from test_bridge import perfect_view, raw_view

torch = pytest.importorskip('torch')
pytestmark = pytest.mark.gpu

T, HALF, SEED, PSEED = 96, 48, 700, 29
OBS = 573
KEYS = ('obs', 'legal', 'player', 'action', 'reward', 'done')
PASS, DBL, RDBL, PLAY = 36, 37, 38, 39


@pytest.fixture(scope='module', autouse=True)
def _need_gpu():
    if not torch.cuda.is_available():
        pytest.fail('GPU tests need a visible GPU (run them on the MI355X box)')


def _np(o):
    return {k: v.cpu().numpy() for k, v in o.items()}


def _rollout(n, flags=0, config=None, pseed=PSEED, policies=None, game='bridge', steps=T, half=HALF):
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


def walk(roll, n, game='bridge', steps=T):
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
        self.v = VecEnv('bridge', 1, seeds=[seed], device=0)

    def reset(self):
        return {k: x[0] for k, x in _np(self.v.reset()).items()}

    def step(self, a):
        return {k: x[0] for k, x in _np(self.v.step([a])).items()}

    def observe(self, p):
        o = _np(self.v.observe(p))
        return o['obs'][0], o['legal'][0]


# ---- the reference's streams ---------------------------------------------------------------------------------------
def test_single_env_replays_reference_stream():
    """the first seed of every steering mode but the long one through a one-env handle (every stream runs batched)"""
    d = gr.load('bridge')
    keep = d['ev_env'] < 4
    part = gr.Fixture({k: (x[keep] if k.startswith('ev_') and len(x) == len(keep) else x) for k, x in d.items()})
    assert gr.replay(part, One, 91) == int(keep.sum())


def test_batched_replay_with_lazy_reset():
    """All fixture seeds as one batch, the 319-call auction among them; a 'reset' event after a finished game is a step
    with any action. At the end of every game the four seats' observations are the recorded final ones."""
    d = gr.load('bridge')
    seeds = [int(s) for s in d['seeds']]
    n = len(seeds)
    v = VecEnv('bridge', n, seeds=seeds, device=0)
    per_env = [np.nonzero(d['ev_env'] == i)[0] for i in range(n)]
    fin_rows = {}
    for j, g in enumerate(d['fin_game']):
        fin_rows.setdefault(int(g), []).append(j)
    assert max(len(x) for x in per_env) >= 372
    out = _np(v.reset())
    checked = 0
    for tick in range(max(len(x) for x in per_env)):
        if tick > 0:
            acts = np.zeros(n, np.int32)
            for i, ev in enumerate(per_env):
                if tick < len(ev) and d['ev_kind'][ev[tick]] == 1:
                    acts[i] = d['ev_act'][ev[tick]]
            out = _np(v.step(torch.from_numpy(acts).cuda()))
        fin = None
        for i, ev in enumerate(per_env):
            if tick >= len(ev):
                continue
            k = ev[tick]
            assert np.array_equal(out['obs'][i], d['ev_obs'][k]), (i, tick)
            assert np.array_equal(out['legal'][i], d['ev_legal'][k]), (i, tick)
            assert out['player'][i] == d['ev_player'][k] and out['done'][i] == d['ev_done'][k], (i, tick)
            if d['ev_done'][k]:
                assert np.array_equal(out['reward'][i], d['ev_payoff'][k].astype(np.float32)), (i, tick)
                if fin is None:
                    fin = [v.observe(p)['obs'].cpu().numpy() for p in range(4)]
                for p, j in enumerate(fin_rows[int(d['ev_game'][k])]):
                    assert np.array_equal(fin[p][i], d['fin_obs'][j]), (i, tick, p)
            checked += 1
    assert checked == len(d['ev_env'])


def test_raw_side_matches_reference():
    d = gr.load('raw_bridge')
    streams = [json.loads(s) for s in d['streams']]
    env, cur = None, -1
    for k in range(len(d['kind'])):
        si, kind, act = int(d['stream'][k]), int(d['kind'][k]), int(d['act'][k])
        if si != cur:
            s = streams[si]
            env = rlcard_amd.make(s['env_id'], dict(s['config'], seed=s['seed']))
            assert env.state_shape == [[1, 573]] * 4 and env.action_shape == [None] * 4 and env.num_actions == 91
            assert env.num_players == 4
            cur = si
        if kind == 0:
            state, player = env.reset()
        elif kind == 1:
            state, player = env.step(act)
        else:
            state, player = env.get_state(act), env.get_player_id()
        where = 'event %d (stream %d, kind %d, act %d)' % (k, si, kind, act)
        assert player == int(d['player'][k]) and int(env.is_over()) == int(d['done'][k]), where
        assert state['obs'].shape == (573,) and state['obs'].dtype == np.int64, where
        assert rawcanon.dumps(raw_view(state)) == d['state'][k], where
        assert rawcanon.dumps(env.get_payoffs()) == d['payoffs'][k], where
        assert rawcanon.dumps(perfect_view(env.get_perfect_information())) == d['perfect'][k], where
    with pytest.raises(NotImplementedError):
        env.step_back()


def test_env_run_with_agents_and_illegal_ids():
    from rlcard_amd.agents import RandomAgent
    env = rlcard_amd.make('bridge', {'seed': 5})
    env.set_agents([RandomAgent(num_actions=env.num_actions), BridgeDefenderNoviceRuleAgent()] * 2)
    traj, payoffs = env.run(is_training=False)
    assert payoffs.dtype == np.int64 and payoffs.shape == (4,) and len(traj) == 4
    assert all(isinstance(t[-1], dict) and not t[-1]['obs'][:468].any() for t in traj)
    assert all(a == PASS for a in traj[1][1::2] if a < PLAY) and all(a == PASS for a in traj[3][1::2] if a < PLAY)
    state, _ = env.reset()
    assert env.get_payoffs().tolist() == [0, 0, 0, 0]
    env.step(0)   # no_bid is never legal: an illegal id plays the lowest legal id, the bid of one club
    assert env.action_recorder[-1][1].action_id == 1 == min(state['legal_actions'])
    assert str(env.action_recorder[-1][1]) == '1C' and list(state['legal_actions'])[0] == PASS


# ---- the rollout against the step API ------------------------------------------------------------------------------
@pytest.mark.parametrize('n', [65, 257])
def test_rollout_equals_the_step_api(n):
    roll = random_rollout(n)
    lg = legal_bits(roll['legal'])
    assert roll['legal'].shape == (T, n, 12) and not lg[..., 91:].any() and not lg[..., 0].any()
    assert np.take_along_axis(lg, roll['action'][..., None].astype(np.int64), axis=-1).all()   # every action is legal
    assert (roll['action'] >= 64).any() and (roll['action'] < PASS).any()   # both words of the mask are played
    obs = roll['obs']
    assert obs[..., 481:521].max() > 1 and obs[..., :481].max() == 1 and obs[..., 521:].max() == 1
    assert (obs[..., 476:480].sum(axis=-1) == 1).all()
    assert np.array_equal(np.argmax(obs[..., 476:480], axis=-1), roll['player'])
    assert roll['reward'].shape == (T, n, 4) and roll['final_obs'].shape == (T, n, 4, OBS)
    done = roll['done'] != 0
    assert done.any() and not roll['final_obs'][~done].any() and not roll['final_obs'][done][..., :468].any()
    assert (roll['final_obs'][done][..., 480] == 1).all()
    walk(roll, n)


def test_obs_rows_are_exact_at_every_alignment():
    """573-byte rows start at every byte phase; a lane stores bytes up to its first dword, dwords up to its first 16-byte
    boundary, 16-byte pieces, then dwords and bytes: with the trajectory's obs tensor and final_obs at every offset 0..15
    from a 16-byte boundary every row, the bidding_rep bytes as values, is the row of the aligned run and no byte
    outside the tensor is written. 65 envs: the last wave holds one row."""
    n, steps = 65, T   # (no uniform-random game ends within 48 steps: final_obs needs the 96)
    v = VecEnv('bridge', n, seed=SEED, device=0)
    want = _np(v.rollout(steps, policy_seed=PSEED, out=v.new_traj_out(steps, final_obs=True, select=1)))
    assert want['done'].any() and want['obs'][..., 481:521].max() > 1
    size, fsize = steps * n * OBS, steps * n * 4 * OBS
    for off in range(16):
        v = VecEnv('bridge', n, seed=SEED, device=0)
        out = v.new_traj_out(steps, final_obs=True, select=1)
        base = torch.full((size + 64,), 7, dtype=torch.uint8, device='cuda')
        fbase = torch.zeros((fsize + 64,), dtype=torch.uint8, device='cuda')
        lead = (-base.data_ptr()) % 16 + off
        flead = (-fbase.data_ptr()) % 16 + (off + 5) % 16
        fbase[:flead] = 7
        fbase[flead + fsize:] = 7
        out['obs'] = base[lead:lead + size].view(steps, n, OBS)
        out['final_obs'] = fbase[flead:flead + fsize].view(steps, n, 4, OBS)
        assert out['obs'].data_ptr() % 16 == off
        got = _np(v.rollout(steps, policy_seed=PSEED, out=out))
        for k in want:
            assert np.array_equal(got[k], want[k]), (k, off)
        b, f = base.cpu().numpy(), fbase.cpu().numpy()
        assert (b[:lead] == 7).all() and (b[lead + size:] == 7).all(), off   # nothing outside the rows
        assert (f[:flead] == 7).all() and (f[flead + fsize:] == 7).all(), off


def test_reset_and_step_rows_at_every_alignment():
    n = 65
    want = _np(VecEnv('bridge', n, seed=SEED, device=0).reset())['obs']
    for off in range(16):
        v = VecEnv('bridge', n, seed=SEED, device=0)
        out = v.new_step_out()
        base = torch.full((n * OBS + 64,), 7, dtype=torch.uint8, device='cuda')
        lead = (-base.data_ptr()) % 16 + off
        out['obs'] = base[lead:lead + n * OBS].view(n, OBS)
        v.reset(out=out)
        got = base.cpu().numpy()
        assert np.array_equal(got[lead:lead + n * OBS].reshape(n, OBS), want), off
        assert (got[:lead] == 7).all() and (got[lead + n * OBS:] == 7).all(), off


def test_an_existing_games_rollout_still_equals_the_step_api():
    """Gin Rummy, 257 envs x 64 steps: the skeleton's direct-row path as the game before Bridge takes it"""
    roll = _rollout(257, game='gin-rummy', steps=64, half=32)
    walk(roll, 257, game='gin-rummy', steps=64)


def test_unstaged_fallback_and_serial_refill_give_the_same_rollout():
    a = random_rollout(65)
    for flags in (2, 1):   # bit 1: one global load per draw; bit 0: every block crossing refills in its own lane
        b = _rollout(65, flags=flags)
        for k in a:
            assert np.array_equal(a[k], b[k]), (k, flags)


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
    v = VecEnv('bridge', n, seed=SEED, device=0)
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
    assert v.env_state_words(3) == words and len(words) == 35


# ---- constructed states ------------------------------------------------------------------------------------------------
DECK = [51 - j for j in range(52)]   # seat p is dealt suit p: clubs to seat 0, diamonds, hearts, spades to seat 3
FULL = [0x1FFF << (13 * p) for p in range(4)]


def encode_words(hands, calls, current, dealer=0, last_bid=0, last_bidder=0, cube=0, passes=0, last_call=0, ncards=0,
                 won=(0, 0), declarer=0, leader=0, trick=(), first=0, deck=DECK, ncalls=None):
    """The packed state words of cs_bridge.h (the inverse of bridge.decode_words)."""
    w = [int(x) for x in np.array(deck, np.uint8).view('<u4')]
    for h in hands:
        w += [h & 0xFFFFFFFF, h >> 32]
    cb = np.zeros(40, np.uint8)
    cb[:len(calls)] = calls
    w += [int(x) for x in cb.view('<u4')]
    nc = len(calls) if ncalls is None else ncalls
    meta = current | dealer << 2 | nc << 4 | last_bid << 13 | last_bidder << 19 | cube << 21 | passes << 23 | last_call << 25
    play = ncards | won[0] << 6 | won[1] << 10 | declarer << 14 | leader << 16
    return w + [first, meta, play, sum(c << (8 * i) for i, c in enumerate(trick))]


def last_card_state(bid, won, first):
    """51 cards played, seat 1 led the ace of diamonds to the last trick, hearts and spades followed, seat 0 holds the
    two of clubs: a ruff if clubs are trumps"""
    return encode_words([1, 0, 0, 0], [bid, PASS, PASS, PASS], 0, last_bid=bid, passes=3, ncards=51, won=won, leader=1,
                        trick=(25, 26, 39), first=first)


def test_constructed_states_one_step_from_each_ending():
    v = VecEnv('bridge', 4, seed=1, device=0)
    v.reset()
    # env 0: dealer 1, three passes: the fourth ends the game with zero payoffs and seat 0 stays the current player
    v.set_env_state_words(0, encode_words(FULL, [PASS] * 3, 0, dealer=1, passes=3, last_call=PASS))
    # env 1: one club by seat 0 with six tricks, seat 0 ruffs the last trick: made. env 2: one no-trump, six tricks
    # each, the ace of diamonds wins the last: one down
    v.set_env_state_words(1, last_card_state(1, (6, 6), 1))
    v.set_env_state_words(2, last_card_state(5, (6, 6), 1 << 8))
    # env 3: one club by seat 0 doubled by seat 1, two passes: the third pass makes it the contract, seat 1 leads
    v.set_env_state_words(3, encode_words(FULL, [1, DBL, PASS, PASS], 0, last_bid=1, cube=1, passes=2, last_call=PASS,
                                          first=1))
    seen = _np(v.observe(0))
    ids = [np.nonzero(r)[0].tolist() for r in legal_bits(seen['legal'])]
    assert ids[0] == list(range(1, 36)) + [PASS]
    assert ids[1] == [PLAY] and ids[2] == [PLAY] and ids[3] == list(range(2, 36)) + [PASS, RDBL]
    assert seen['player'].tolist() == [0, 0, 0, 0] and not seen['done'].any()
    assert seen['obs'][1][208 + 52 + 25] == 1 and seen['obs'][1][208:416].sum() == 3 and seen['obs'][1][:208].sum() == 1
    out = _np(v.step([PASS, PLAY, PLAY, PASS]))
    assert out['done'].tolist() == [1, 1, 1, 0] and out['player'].tolist() == [0, 0, 1, 1]
    assert out['reward'].tolist() == [[0, 0, 0, 0], [9, 6, 9, 6], [-1, 7, -1, 7], [0, 0, 0, 0]]
    assert not out['obs'][:3, :468].any() and not out['legal'][:3].any() and (out['obs'][:3, 480] == 1).all()
    assert out['obs'][0][521 + PASS] == 1 and not out['obs'][1][521:560].any()
    assert out['obs'][0][481:521].tolist() == [0] + [PASS] * 4 + [0] * 35
    row = out['obs'][3]   # the doubled contract: seat 1 to lead, sees his own hand and the dummy's (seat 2)
    assert row[:208].reshape(4, 52).sum(axis=1).tolist() == [0, 13, 13, 0] and row[416:468].sum() == 26
    assert row[480] == 1 and row[560 + 1] == 1 and row[568 + 0] == 1 and row[560:573].sum() == 2
    assert row[481:486].tolist() == [1, DBL, PASS, PASS, PASS]
    assert np.nonzero(legal_bits(out['legal'][3]))[0].tolist() == [PLAY + 13 + i for i in range(13)]
    s = bridge.decode_words(v.env_state_words(3))
    assert s['cube'] == 2 and s['declarer'] == 0 and s['bidding_over'] and s['last_bid'] == 1
    out = _np(v.step([0, 0, 0, PLAY + 13]))   # envs 0..2 deal their next game
    assert not out['done'].any() and (out['obs'][:3, :208].sum(axis=1) == 13).all()
    assert not out['obs'][3][560:573].any() and out['obs'][3][208 + 52 + 13] == 1   # the contract left the obs


def test_state_words_that_hold_no_game_are_a_finished_game():
    """cs_set_env_state's words are the caller's: one case per rule of Bridge::load"""
    good = last_card_state(1, (6, 6), 1)
    twice = list(DECK)
    twice[5] = twice[6]
    bad = {'deck': encode_words([1, 0, 0, 0], [1, PASS, PASS, PASS], 0, last_bid=1, passes=3, ncards=51, won=(6, 6),
                                leader=1, trick=(25, 26, 39), first=1, deck=twice),
           'calls counter': encode_words(FULL, [PASS] * 3, 0, passes=1, last_call=PASS, ncalls=400),
           'tricks counter': last_card_state(1, (6, 7), 1),
           'played mask': encode_words([3, 0, 0, 0], [1, PASS, PASS, PASS], 0, last_bid=1, passes=3, ncards=51,
                                       won=(6, 6), leader=1, trick=(25, 26, 39), first=1),
           'trick card': encode_words([1, 0, 0, 0], [1, PASS, PASS, PASS], 0, last_bid=1, passes=3, ncards=51,
                                      won=(6, 6), leader=1, trick=(0, 26, 39), first=1),
           'stored call': encode_words(FULL, [PASS, 39, PASS], 0, passes=1, last_call=PASS),
           'call past the last': encode_words(FULL, [PASS, PASS, PASS, 7], 0, passes=3, last_call=PASS, ncalls=3)}
    # a finished game still shows its calls and its last call: words with the over bit and a last call that is none
    finished = encode_words(FULL, [PASS] * 4, 0, dealer=1, passes=3, last_call=50)
    finished[32] |= 1 << 31
    bad['finished, last call 50'] = finished
    v = VecEnv('bridge', 1 + len(bad), seed=3, device=0)
    v.reset()
    v.set_env_state_words(0, good)
    for e, words in enumerate(bad.values()):
        v.set_env_state_words(1 + e, words)
    seen = _np(v.observe(0))
    assert seen['done'].tolist() == [0] + [1] * len(bad), list(bad)
    assert not seen['legal'][1:].any() and not seen['obs'][1:, :468].any()
    assert not seen['obs'][len(bad), 480:].any()   # (the blank game: no calls, nothing in the contract fields)
    out = _np(v.step([PLAY] * (1 + len(bad))))   # env 0 plays its last card; the others deal a new game
    assert out['done'].tolist() == [1] + [0] * len(bad)
    assert (out['obs'][1:, :208].sum(axis=1) == 13).all() and (out['obs'][1:, 416:468].sum(axis=1) == 39).all()


# ---- policies -------------------------------------------------------------------------------------------------------------
def test_random_policy_actions_are_the_rollouts_pick():
    n = 65
    roll = random_rollout(n)
    v = VecEnv('bridge', n, seed=SEED, device=0)
    v.reset()
    alive = np.ones(n, bool)
    for t in range(40):
        a = v.policy_actions('random', policy_seed=PSEED, t=t).cpu().numpy()
        assert np.array_equal(a[alive], roll['action'][t][alive].astype(np.int32)), t
        alive &= roll['done'][t] == 0
        acts = np.where(a < 0, 0, a).astype(np.int32)
        v.step(torch.from_numpy(acts).cuda())
    assert alive.sum() > n // 2 and (roll['action'][:40] >= 64).any()


def test_rollout_with_the_novice_rule_in_two_seats():
    n = 65
    agent = BridgeDefenderNoviceRuleAgent()
    roll = _rollout(n, policies=['random', agent, 'random', agent])
    plain = random_rollout(n)
    assert np.array_equal(roll['obs'][0], plain['obs'][0])   # the same deals
    lg = legal_bits(roll['legal'])
    assert np.take_along_axis(lg, roll['action'][..., None].astype(np.int64), axis=-1).all()
    rule_seat = (roll['player'] & 1) == 1
    calls = roll['action'] < PLAY
    assert (roll['action'][rule_seat & calls] == PASS).all() and (rule_seat & calls).sum() > n
    assert (roll['action'][~rule_seat & calls] != PASS).any()
    cards = roll['action'][rule_seat & ~calls]
    assert len(set(cards.tolist())) > 26 and roll['done'].any()   # the rule's cards are picked at random
    v = VecEnv('bridge', n, seed=SEED, device=0)
    v.reset()
    a = v.policy_actions(agent, policy_seed=PSEED, t=0).cpu().numpy()
    assert (a == PASS).all()


def test_the_novice_rule_in_all_four_seats_passes_every_game_out():
    n, steps = 257, 48
    roll = _rollout(n, policies=[1, 1, 1, 1], steps=steps, half=steps)
    assert (roll['action'] == PASS).all() and not roll['reward'].any()
    want_done = (np.arange(steps) % 4 == 3)[:, None].repeat(n, axis=1)
    assert np.array_equal(roll['done'] != 0, want_done)
    dealer = np.argmax(roll['obs'][..., 472:476], axis=-1)
    assert np.array_equal(roll['player'], (dealer + (np.arange(steps) % 4)[:, None]) % 4)
    assert len(set(dealer.reshape(-1).tolist())) == 4


def test_tournament_sums_equal_the_payoff_rows():
    """Windows of HALF steps, as tournament_vec rolls them: the device's sums against the payoff rows summed here."""
    n = 65
    agent = BridgeDefenderNoviceRuleAgent()
    seats = ['random', agent, 'random', agent]
    v = VecEnv('bridge', n, seed=SEED, device=0)
    acc, out = v.new_payoff_sums(), v.new_traj_out(HALF, select=1)
    total, first, games = np.zeros(4), np.zeros(4), 0
    have = np.zeros(n, bool)
    for w in range(8):
        t = _np(v.rollout(HALF, policy_seed=PSEED, t0=w * HALF, out=out, policies=seats))
        v.payoff_sums(out, acc, quota=0)
        done = t['done'] != 0
        for tt, e in zip(*np.nonzero(done)):
            total += t['reward'][tt, e].astype(np.float64)
        games += int(done.sum())
        for e in np.nonzero(~have & done.any(axis=0))[0]:
            first += t['reward'][int(np.argmax(done[:, e])), e].astype(np.float64)
            have[e] = True
        if have.all():
            break
    assert have.all() and int(acc['games'].item()) == games >= n
    assert np.array_equal(acc['sums'].cpu().numpy(), total)   # small integers: exact in any order
    v = VecEnv('bridge', n, seed=SEED, device=0)
    pay = tournament_vec(v, seats, games_per_env=1, T=HALF, policy_seed=PSEED)
    assert len(pay) == 4 and np.allclose(np.asarray(pay), first / n, rtol=0, atol=1e-9)
    assert pay[0] == pay[2] and pay[1] == pay[3]


def test_refusals():
    cfg = _abi.Config(2, -1, 0, 0, 0)
    h = C.c_void_p()
    assert _abi.lib().cs_create(C.byref(h), 8, 8, 0, C.byref(cfg)) == -4
    assert _abi.lib().cs_last_error().startswith(b'bridge: game_num_players must be 4')
    with pytest.raises(ValueError):
        rlcard_amd.make('bridge', {'game_num_players': 3})
    with pytest.raises(ValueError):
        VecEnv('bridge', 4, device=0, config={'game_num_players': 2})
    env = rlcard_amd.make('bridge', {'seed': 1, 'allow_step_back': True})
    env.reset()
    with pytest.raises(NotImplementedError):
        env.step_back()
    v = VecEnv('bridge', 65, seed=1, device=0)
    with pytest.raises(_abi.CardsimError, match='CS_E_UNSUPPORTED'):
        v.policy_actions(2)
    with pytest.raises(_abi.CardsimError, match='CS_E_UNSUPPORTED'):
        v.rollout(4, out=v.new_traj_out(4, select=1), policies=[2, 'random', 'random', 'random'])
    L = _abi.lib()
    out = C.c_void_p()
    assert L.cs_replay_create(v._h, 64, C.byref(out)) == -4 and b'bridge 91' in L.cs_last_error()
    assert L.cs_reservoir_create(v._h, 64, 1, C.byref(out)) == -4 and b'bridge 91' in L.cs_last_error()
    net = _abi.QNet()
    obs = torch.zeros((4, OBS), dtype=torch.uint8, device='cuda')
    q = torch.zeros((4, 91), dtype=torch.float32, device='cuda')
    p = C.c_void_p
    assert L.cs_qnet_values(v._h, C.byref(net), p(obs.data_ptr()), None, 4, p(q.data_ptr()), None) == -4
    assert b'at most 64 actions' in L.cs_last_error()
    assert L.cs_pnet_probs(v._h, C.byref(net), p(obs.data_ptr()), None, 4, p(q.data_ptr()), None) == -4
