"""Scout on the HIP engine against the reference's recorded streams (tests/golden/scout.npz, raw_scout.npz) and against
itself: the fused rollout row by row against the step API, the 688-byte obs rows and 26-byte legal rows of a whole wave
and on tensors off their 16-byte boundary, Philox mode, state save / load, constructed states one step from each ending,
state words that hold no game, the random pick over a mask with ids in all four words, the tournament sums and the
refusals. Shapes: 65 envs (one wave plus one lane) and 257 (four waves plus one lane), T = 192 as two chained launches
of 96 (uniform-random games took 4 to 365 steps in the reference, 145 on average)."""
import ctypes as C
import json

import numpy as np
import pytest

import golden_replay as gr
import rawcanon
import rlcard_amd
from rlcard_amd import VecEnv, _abi
from rlcard_amd.envs import scout
from rlcard_amd.utils import tournament_vec
from test_scout import perfect_view, raw_view

torch = pytest.importorskip('torch')
pytestmark = pytest.mark.gpu

T, HALF, SEED, PSEED = 192, 96, 900, 31
OBS, LB, A = 688, 26, 204
KEYS = ('obs', 'legal', 'player', 'action', 'reward', 'done')


@pytest.fixture(scope='module', autouse=True)
def _need_gpu():
    if not torch.cuda.is_available():
        pytest.fail('GPU tests need a visible GPU (run them on the MI355X box)')


def _np(o):
    return {k: v.cpu().numpy() for k, v in o.items()}


def _rollout(n, flags=0, config=None, pseed=PSEED, game='scout', steps=T, half=HALF):
    """`steps` steps as launches of `half` with t0 carried -> numpy trajectory [steps, n, ...] with final_obs"""
    v = VecEnv(game, n, seed=SEED, device=0, config=config)
    if flags:
        v.set_kernel_flags(flags)
    parts = []
    for k in range(steps // half):
        out = v.new_traj_out(half, final_obs=True, select=1)
        parts.append(_np(v.rollout(half, policy_seed=pseed, t0=k * half, out=out)))
    return {k: np.concatenate([p[k] for p in parts]) for k in parts[0]}


_cache = {}


def random_rollout(n):
    if n not in _cache:
        _cache[n] = _rollout(n)
    return _cache[n]


def legal_bits(rows):
    """uint8 [..., LB] -> 0/1 [..., 8 LB]"""
    return np.unpackbits(rows, axis=-1, bitorder='little')


def walk(roll, n, game='scout', steps=T):
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
        self.v = VecEnv('scout', 1, seeds=[seed], device=0)

    def reset(self):
        return {k: x[0] for k, x in _np(self.v.reset()).items()}

    def step(self, a):
        return {k: x[0] for k, x in _np(self.v.step([a])).items()}

    def observe(self, p):
        o = _np(self.v.observe(p))
        return o['obs'][0], o['legal'][0]


# ---- the reference's streams ---------------------------------------------------------------------------------------
def test_single_env_replays_reference_stream():
    """the first seed of the uniform, scout and streak modes through a one-env handle (every stream runs batched)"""
    d = gr.load('scout')
    keep = d['ev_env'] < 3
    part = gr.Fixture({k: (x[keep] if k.startswith('ev_') and len(x) == len(keep) else x) for k, x in d.items()})
    assert gr.replay(part, One, A) == int(keep.sum())


def test_batched_replay_with_lazy_reset():
    """All fixture seeds as one batch; a 'reset' event after a finished game is a step with any action. At the end of
    every game the four seats' observations are the recorded final ones."""
    d = gr.load('scout')
    seeds = [int(s) for s in d['seeds']]
    n = len(seeds)
    v = VecEnv('scout', n, seeds=seeds, device=0)
    per_env = [np.nonzero(d['ev_env'] == i)[0] for i in range(n)]
    fin_rows = {}
    for j, g in enumerate(d['fin_game']):
        fin_rows.setdefault(int(g), []).append(j)
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
    d = gr.load('raw_scout')
    streams = [json.loads(s) for s in d['streams']]
    env, cur = None, -1
    for k in range(len(d['kind'])):
        si, kind, act = int(d['stream'][k]), int(d['kind'][k]), int(d['act'][k])
        if si != cur:
            s = streams[si]
            env = rlcard_amd.make(s['env_id'], dict(s['config'], seed=s['seed']))
            assert env.state_shape == [[688]] * 4 and env.action_shape == [None] * 4 and env.num_actions == 204
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
        assert state['obs'].shape == (688,) and state['obs'].dtype == np.float32, where
        assert rawcanon.dumps(raw_view(state)) == d['state'][k], where
        assert rawcanon.dumps(env.get_payoffs()) == d['payoffs'][k], where
        assert rawcanon.dumps(perfect_view(env.get_perfect_information())) == d['perfect'][k], where
    with pytest.raises(NotImplementedError):
        env.step_back()


def test_env_run_with_agents_and_illegal_ids():
    from rlcard_amd.agents import RandomAgent
    env = rlcard_amd.make('scout', {'seed': 5})
    env.set_agents([RandomAgent(num_actions=env.num_actions) for _ in range(4)])
    traj, payoffs = env.run(is_training=False)
    assert payoffs.dtype == np.int64 and payoffs.shape == (4,) and len(traj) == 4
    assert all(isinstance(t[-1], dict) and t[-1]['obs'].dtype == np.float32 for t in traj)
    last = [t[-1]['raw_obs'] for t in traj]
    assert payoffs.tolist() == [s['points'] - len(s['hand']) for s in last]
    state, player = env.reset()
    assert env.get_payoffs().tolist() == [-12, -11, -11, -11] and state['raw_obs']['must_choose_orientation']
    ids = list(state['legal_actions'])
    assert max(ids) < 136 and state['obs'][676] == 1 and not state['raw_obs']['current_player_forced_scout']
    env.step(203)   # no scout is legal on an empty table: an illegal id plays the lowest legal id
    who, action, context = env.action_recorder[-1]
    assert who == player and action.action_id == min(ids) and context['action_type'] == 'play'
    assert context['cards'] == [str(c) for c in state['raw_obs']['hand'][action.start_idx:action.end_idx]]
    assert not env.get_state(player)['raw_obs']['must_choose_orientation']
    state, player = env.get_state(env.get_player_id()), env.get_player_id()
    scouts = [a for a in state['raw_legal_actions'] if isinstance(a, scout.ScoutAction)]
    assert scouts and state['obs'][683] == np.float32(len(state['raw_obs']['table_set']) / 16) and state['obs'][684] == 0
    nxt, _ = env.step(scouts[-1], raw_action=True)
    who, action, context = env.action_recorder[-1]
    assert action is scouts[-1] and context['action_type'] == 'scout' and context['insertion'] == action.insertion_in_hand
    assert len(nxt['action_record']) == 2 and env.timestep >= 2


# ---- the rollout against the step API ------------------------------------------------------------------------------
@pytest.mark.parametrize('n', [65, 257])
def test_rollout_equals_the_step_api(n):
    roll = random_rollout(n)
    lg = legal_bits(roll['legal'])
    assert roll['legal'].shape == (T, n, LB) and not lg[..., 200:].any()
    assert np.take_along_axis(lg, roll['action'][..., None].astype(np.int64), axis=-1).all()   # every action is legal
    assert {int(x) for x in np.unique(roll['action'] >> 6)} >= {0, 1, 2}   # plays of both words and scouts are played
    obs = roll['obs']
    assert obs[..., :677].max() == 1 and obs[..., 678:682].max() > 1 and obs[..., 686:].max() > 1
    assert (obs[..., 672:677].sum(axis=-1) == 1).all()
    own = np.take_along_axis(obs[..., 678:682], roll['player'][..., None].astype(np.int64), axis=-1)[..., 0]
    assert np.array_equal(own, obs[..., 640:656].sum(axis=-1))   # the row is the current player's
    assert np.array_equal(obs[..., 685] == 1, ~lg[..., :136].any(axis=-1))
    assert roll['reward'].shape == (T, n, 4) and roll['final_obs'].shape == (T, n, 4, OBS)
    done = roll['done'] != 0
    assert done.any() and not roll['final_obs'][~done].any()
    fin = roll['final_obs'][done]
    points = fin[..., 682].astype(np.int64) + 256 * fin[..., 683].astype(np.int64)
    assert np.array_equal(roll['reward'][done], (points - fin[..., 640:656].sum(axis=-1)).astype(np.float32))
    walk(roll, n)


def test_obs_and_legal_rows_of_a_whole_wave_are_exact():
    """every row 0..63 of a wave against a one-env handle of the same seed (its rows are always row 0, so the two sides
    store at different addresses): 26-byte legal rows start at every byte phase within a wave"""
    n, steps = 64, 40
    roll = _rollout(n, steps=steps, half=steps)
    assert {(LB * e) % 16 for e in range(n)} == set(range(0, 16, 2))
    for e in range(n):
        v = VecEnv('scout', 1, seed=SEED + e, device=0)
        out = _np(v.reset())
        for t in range(steps):
            assert np.array_equal(out['obs'][0], roll['obs'][t, e]) and np.array_equal(out['legal'][0], roll['legal'][t, e])
            assert out['player'][0] == roll['player'][t, e]
            out = _np(v.step([int(roll['action'][t, e])]))
            assert out['done'][0] == roll['done'][t, e]
            if out['done'][0]:
                out = _np(v.step([0]))


def test_rows_on_tensors_off_their_16_byte_boundary():
    """an obs tensor that is not 16-byte aligned takes the byte path, final_obs likewise; the rows are those of the
    aligned run and no byte outside the tensors is written (the legal tensor sits between guard bytes as well)"""
    n, steps = 65, 96
    v = VecEnv('scout', n, seed=SEED, device=0)
    want = _np(v.rollout(steps, policy_seed=PSEED, out=v.new_traj_out(steps, final_obs=True, select=1)))
    assert want['done'].any()
    size, fsize, lsize = steps * n * OBS, steps * n * 4 * OBS, steps * n * LB
    for off in (0, 1, 4, 8, 15):
        v = VecEnv('scout', n, seed=SEED, device=0)
        out = v.new_traj_out(steps, final_obs=True, select=1)
        base = torch.full((size + 64,), 7, dtype=torch.uint8, device='cuda')
        fbase = torch.zeros((fsize + 64,), dtype=torch.uint8, device='cuda')
        lbase = torch.full((lsize + 64,), 7, dtype=torch.uint8, device='cuda')
        lead = (-base.data_ptr()) % 16 + off
        flead = (-fbase.data_ptr()) % 16 + (off + 5) % 16
        fbase[:flead] = 7
        fbase[flead + fsize:] = 7
        out['obs'] = base[lead:lead + size].view(steps, n, OBS)
        out['final_obs'] = fbase[flead:flead + fsize].view(steps, n, 4, OBS)
        out['legal'] = lbase[3:3 + lsize].view(steps, n, LB)
        assert out['obs'].data_ptr() % 16 == off
        got = _np(v.rollout(steps, policy_seed=PSEED, out=out))
        for k in want:
            assert np.array_equal(got[k], want[k]), (k, off)
        b, f, l = base.cpu().numpy(), fbase.cpu().numpy(), lbase.cpu().numpy()
        assert (b[:lead] == 7).all() and (b[lead + size:] == 7).all(), off   # nothing outside the rows
        assert (f[:flead] == 7).all() and (f[flead + fsize:] == 7).all(), off
        assert (l[:3] == 7).all() and (l[3 + lsize:] == 7).all(), off


def test_an_existing_games_rollout_still_equals_the_step_api():
    """Bridge, 65 envs x 96 steps: the skeleton's mixed-row path and two-word masks as the game before Scout takes them"""
    roll = _rollout(65, game='bridge', steps=96, half=48)
    walk(roll, 65, game='bridge', steps=96)


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
    v = VecEnv('scout', n, seed=SEED, device=0)
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
    assert v.env_state_words(3) == words and len(words) == 24


# ---- constructed states ------------------------------------------------------------------------------------------------
def card(top, bottom):
    return top | bottom << 4


def encode_words(hands, table, current, owner=4, scouts=0, scores=(0, 0, 0, 0), locked=0, over=False, lengths=None,
                 table_len=None):
    """The packed state words of cs_scout.h (the inverse of scout.decode_words); the forced flag is the engine's"""
    b = np.zeros(80, np.uint8)
    for p, h in enumerate(hands):
        b[16 * p:16 * p + len(h)] = h
    b[64:64 + len(table)] = table
    nh = lengths if lengths is not None else [len(h) for h in hands]
    tl = len(table) if table_len is None else table_len
    meta = tl | owner << 5 | scouts << 8 | current << 10 | locked << 12 | int(over) << 31
    return [int(x) for x in b.view('<u4')] + [sum(k << (8 * p) for p, k in enumerate(nh)), meta,
                                               scores[0] | scores[1] << 16, scores[2] | scores[3] << 16]


# sixteen different cards whose tops are never equal or one apart from their neighbour's: no slice of two
LOOSE16 = [card(t, b) for t, b in ((1, 2), (3, 4), (5, 6), (7, 8), (9, 10), (1, 4), (3, 6), (5, 8), (7, 10), (9, 2), (1, 6),
                                   (3, 8), (5, 10), (7, 2), (9, 4), (1, 8))]
STREAK = encode_words([[card(1, 2)], [card(3, 4)], [card(5, 6)], [card(7, 8), card(1, 3)]], [card(9, 10), card(10, 2)], 3,
                      owner=0, scouts=2)
EMPTY_HAND = encode_words([[card(1, 2)], [], [card(5, 6)], [card(7, 8)]], [card(9, 10)], 0, owner=2)
FULL_HAND = encode_words([[card(10, 3)], LOOSE16, [card(2, 4)], [card(6, 8)]], [], 0)
FORCED = encode_words([[card(1, 2), card(4, 5), card(7, 8)], [card(2, 3)], [card(5, 6)], [card(6, 7)]],
                      [card(9, 10), card(9, 3)], 0, owner=2, scores=(0, 0, 300, 0))


def ids_of(row):
    return np.nonzero(legal_bits(row))[0].tolist()


def test_constructed_states_one_step_from_each_ending():
    v = VecEnv('scout', 4, seed=1, device=0)
    v.reset()
    for e, words in enumerate((STREAK, EMPTY_HAND, FULL_HAND, FORCED)):
        v.set_env_state_words(e, words)
    seen = _np(v.observe(0))
    assert seen['player'].tolist() == [3, 0, 0, 0] and not seen['done'].any()
    front2 = [136, 137, 140, 141]
    assert ids_of(seen['legal'][0]) == [136 + 4 * i + k for i in range(3) for k in range(4)]   # seat 3: scouts only
    assert ids_of(seen['legal'][1]) == front2 and ids_of(seen['legal'][2]) == [0]
    assert ids_of(seen['legal'][3]) == [136 + 4 * i + k for i in range(4) for k in range(4)]
    assert seen['obs'][:, 685].tolist() == [1, 1, 0, 1] and seen['obs'][:, 677].tolist() == [2, 0, 0, 0]
    assert seen['obs'][:, 672:677].argmax(axis=1).tolist() == [0, 2, 4, 2]
    out = _np(v.step([136, 137, 0, 150]))
    assert out['done'].tolist() == [1, 1, 1, 0] and out['player'].tolist() == [0, 1, 1, 1]
    assert out['reward'].tolist() == [[0, -1, -1, -3], [-2, 0, 0, -1], [0, -16, -1, -1], [0, 0, 0, 0]]
    # the streak: three scouts with an owner; the finished game shows the next seat's scouts and forced flag
    assert out['obs'][0][677] == 3 and out['obs'][0][684] == 1 and ids_of(out['legal'][0]) == front2
    assert out['obs'][0][685] == 1 and out['obs'][0][672] == 1 and out['obs'][0][682] == 1   # seat 0 was paid 1
    # the emptied table: no owner, counter 0, nothing legal for the empty hand
    assert out['obs'][1][676] == 1 and out['obs'][1][677] == 0 and not out['legal'][1].any() and out['obs'][1][685] == 1
    s = scout.decode_words(v.env_state_words(1))
    assert [str(c) for c in s['hands'][0]] == ['10/9', '1/2'] and s['scores'] == [0, 0, 1, 0] and s['owner'] is None
    # the full hand: sixteen cards, none beats the ten, and a full hand cannot scout
    assert not out['legal'][2].any() and out['obs'][2][640:656].sum() == 16 and out['obs'][2][686] == 10
    # the forced scout pays the owner from the bank: 300 -> 301, two bytes in seat 2's row
    assert out['obs'][3][685] == 1 and out['obs'][3][677] == 1 and out['obs'][3][684] == 1
    s = scout.decode_words(v.env_state_words(3))
    assert [str(c) for c in s['hands'][0]] == ['1/2', '4/5', '7/8', '9/3'] and s['scores'][2] == 301 and s['locked'][0]
    row = _np(v.observe(2))['obs'][3]
    assert row[682] == 301 & 255 and row[683] == 1 and scout.row_to_obs(row)[682] == np.float32(301 / 16)
    out = _np(v.step([0, 0, 0, 136]))   # envs 0..2 deal their next game
    assert not out['done'].any() and out['obs'][:3, 678:682].tolist() == [[12, 11, 11, 11]] * 3
    assert out['obs'][3][676] == 1 and out['obs'][3][684] == 0   # the second scout emptied the table
    assert scout.decode_words(v.env_state_words(3))['scores'][2] == 302


def test_state_words_that_hold_no_game_are_a_finished_game():
    """cs_set_env_state's words are the caller's: one case per rule of Scout::load"""
    hands = [[card(1, 2), card(4, 5), card(7, 8)], [card(2, 3)], [card(5, 6)], [card(6, 7)]]
    table = [card(9, 10), card(9, 3)]
    bad = {'hand length 17': encode_words(hands, table, 0, owner=2, lengths=[3, 17, 1, 1]),
           'table length 17': encode_words(hands, table, 0, owner=2, table_len=17),
           'top 11': encode_words([[card(11, 2)]] + hands[1:], table, 0, owner=2),
           'top equals bottom': encode_words([[card(4, 4)]] + hands[1:], table, 0, owner=2),
           'a card twice, flipped': encode_words([[card(1, 2), card(3, 2)]] + hands[1:], table, 0, owner=2),
           'a card in hand and on the table': encode_words(hands, [card(9, 10), card(7, 6)], 0, owner=2),
           'a byte past the length': encode_words(hands, table, 0, owner=2, lengths=[2, 1, 1, 1]),
           'an owner with an empty table': encode_words(hands, [], 0, owner=2),
           'a table without an owner': encode_words(hands, table, 0),
           'owner 5': encode_words(hands, table, 0, owner=5),
           'counter 3 in a running game': encode_words(hands, table, 0, owner=2, scouts=3)}
    v = VecEnv('scout', 1 + len(bad), seed=3, device=0)
    v.reset()
    v.set_env_state_words(0, FORCED)
    for e, words in enumerate(bad.values()):
        v.set_env_state_words(1 + e, words)
    seen = _np(v.observe(0))
    assert seen['done'].tolist() == [0] + [1] * len(bad), list(bad)
    assert not seen['legal'][1:].any() and not seen['obs'][1:, :676].any()
    assert (seen['obs'][1:, 676] == 1).all() and (seen['obs'][1:, 685] == 1).all() and not seen['obs'][1:, 677:685].any()
    out = _np(v.step([150] * (1 + len(bad))))   # env 0 scouts; the others deal a new game
    assert not out['done'].any()
    assert out['obs'][1:, 678:682].tolist() == [[12, 11, 11, 11]] * len(bad) and out['obs'][0][677] == 1


# ---- policies -------------------------------------------------------------------------------------------------------------
def test_random_policy_actions_are_the_rollouts_pick():
    n = 65
    roll = random_rollout(n)
    v = VecEnv('scout', n, seed=SEED, device=0)
    v.reset()
    alive = np.ones(n, bool)
    for t in range(40):
        a = v.policy_actions('random', policy_seed=PSEED, t=t).cpu().numpy()
        assert np.array_equal(a[alive], roll['action'][t][alive].astype(np.int32)), t
        alive &= roll['done'][t] == 0
        acts = np.where(a < 0, 0, a).astype(np.int32)
        v.step(torch.from_numpy(acts).cuda())
    assert alive.sum() > n // 2
    # a mask with ids in all four words: fourteen cards against a single one on the table -- singles from id 0 up to
    # 130, scouts 136..193. 257 envs: each draws its own pick
    hand14 = [card(t, b) for t, b in ((3, 1), (5, 2), (7, 3), (9, 4), (2, 6), (4, 7), (6, 8), (8, 9), (10, 1), (3, 5), (5, 7),
                                     (7, 9), (9, 2), (2, 4))]
    wide = encode_words([hand14, [card(1, 4)], [card(1, 6)], [card(1, 8)]], [card(1, 2)], 0, owner=1)
    n = 257
    v = VecEnv('scout', n, seed=SEED, device=0)
    v.reset()
    for e in range(n):
        v.set_env_state_words(e, wide)
    lg = legal_bits(_np(v.observe(0))['legal'])[0]
    assert all(lg[64 * w:64 * w + 64].any() for w in range(4)) and lg.sum() == 14 + 2 * 15
    a = v.policy_actions('random', policy_seed=PSEED, t=7).cpu().numpy()
    r = _np(v.rollout(1, policy_seed=PSEED, t0=7, out=v.new_traj_out(1, select=1)))
    assert np.array_equal(a, r['action'][0].astype(np.int32)) and lg[a].all()
    assert {int(x) for x in a >> 6} == {0, 1, 2, 3}


def test_tournament_sums_equal_the_payoff_rows():
    """Windows of HALF steps, as tournament_vec rolls them: the device's sums against the payoff rows summed here."""
    n = 65
    seats = ['random'] * 4
    v = VecEnv('scout', n, seed=SEED, device=0)
    acc, out = v.new_payoff_sums(), v.new_traj_out(HALF, select=1)
    total, first, games = np.zeros(4), np.zeros(4), 0
    have = np.zeros(n, bool)
    for w in range(12):
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
    v = VecEnv('scout', n, seed=SEED, device=0)
    pay = tournament_vec(v, seats, games_per_env=1, T=HALF, policy_seed=PSEED)
    assert len(pay) == 4 and np.allclose(np.asarray(pay), first / n, rtol=0, atol=1e-9)


def test_refusals():
    cfg = _abi.Config(2, -1, 0, 0, 0)
    h = C.c_void_p()
    assert _abi.lib().cs_create(C.byref(h), 10, 8, 0, C.byref(cfg)) == -4
    assert _abi.lib().cs_last_error().startswith(b'scout: game_num_players must be 4')
    for bad in ({'game_num_players': 3}, {'hand_size': 12}, {'rank_count': 8}, {'allow_step_back': True}):
        with pytest.raises(ValueError):
            rlcard_amd.make('scout', bad)
    with pytest.raises(ValueError):
        VecEnv('scout', 4, device=0, config={'game_num_players': 2})
    v = VecEnv('scout', 65, seed=1, device=0)
    for policy in (1, 2):
        with pytest.raises(_abi.CardsimError, match='CS_E_UNSUPPORTED'):
            v.policy_actions(policy)
    with pytest.raises(_abi.CardsimError, match='CS_E_UNSUPPORTED'):
        v.rollout(4, out=v.new_traj_out(4, select=1), policies=[1, 'random', 'random', 'random'])
    L = _abi.lib()
    out = C.c_void_p()
    assert L.cs_replay_create(v._h, 64, C.byref(out)) == -4 and b'at most 16 bytes' in L.cs_last_error()
    assert L.cs_reservoir_create(v._h, 64, 1, C.byref(out)) == -4 and b'scout 204' in L.cs_last_error()
    net = _abi.QNet()
    obs = torch.zeros((4, OBS), dtype=torch.uint8, device='cuda')
    q = torch.zeros((4, A), dtype=torch.float32, device='cuda')
    p = C.c_void_p
    assert L.cs_qnet_values(v._h, C.byref(net), p(obs.data_ptr()), None, 4, p(q.data_ptr()), None) == -4
    assert b'at most 64 actions' in L.cs_last_error()
    assert L.cs_pnet_probs(v._h, C.byref(net), p(obs.data_ptr()), None, 4, p(q.data_ptr()), None) == -4
