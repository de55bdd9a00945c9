"""CPU-side checks of Scout: the registries and the game's static shape, the 204 action names, the fixtures' own coverage
and internal consistency (tests/golden/gen_scout.py wrote them from the reference), the row-to-float32 mapping of
rlcard_amd/envs/scout.py against the reference's recorded floats, and the rules of the kernels
(rlcard_amd/csrc/cs_scout_rules.h) compiled for the host into a stand-alone program (tools/scout_rules_main.cpp) under
ASan and UBSan: its answers on every (hand, table) -> legal-id set and every strength comparison the reference computed
in the recorded games, and on 120 000 seeded random hands and tables against a direct restatement written here.

raw_view() and perfect_view() are the canon of the raw fixture (raw_scout.npz): the state dict's keys in their order,
obs by dtype and shape (its values are pinned by scout.npz), every raw_obs field with cards as (top, bottom, rank, text)
and actions as (text, id, fields), the legal_actions keys in their order, and of action_record its length and last
entry; get_perfect_information's keys in their order with the same card form and the legal actions by id."""
import json
import os
import random
import subprocess

import numpy as np
import pytest

import golden_replay as gr
import rawcanon
import rlcard_amd
from rlcard_amd import _abi
from rlcard_amd.envs import scout

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEED = {'end_streak': 3, 'end_empty_hand': 3, 'end_full_hand': 3, 'hand16': 3, 'forced_pays': 3, 'scout_empties': 3,
        'back_ins0': 3, 'back_insN': 3, 'flip_ins0': 3, 'flip_insN': 3, 'play_len4': 3, 'group_beats_run': 3,
        'play_on_empty': 3, 'short_game': 3, 'long_game': 3, 'illegal_id': 20}
LARGEST_FIXTURE = 615488   # tests/golden/gin_rummy.npz, the largest fixture before these


def card_view(c):
    return (int(c.top), int(c.bottom), int(c.rank), str(c))


def action_view(a):
    if hasattr(a, 'start_idx'):
        return (str(a), int(a.action_id), 'play', int(a.start_idx), int(a.end_idx))
    return (str(a), int(a.action_id), 'scout', bool(a.from_front), int(a.insertion_in_hand), bool(a.flip))


def record_view(entry):
    player, action, context = entry
    return (int(player), action_view(action), {k: (bool(v) if isinstance(v, (bool, np.bool_)) else v)
                                               for k, v in context.items()})


def raw_view(state):
    """The canonical view of a Scout Env state dict (the reference's or rlcard_amd's)."""
    ro = state['raw_obs']
    assert state['raw_legal_actions'] is ro['legal_actions']   # (one list under both keys)
    rec = state['action_record']
    return {'keys': list(state.keys()), 'obs': (state['obs'].dtype.name, list(state['obs'].shape)),
            'raw_keys': list(ro.keys()), 'hand': [card_view(c) for c in ro['hand']], 'points': ro['points'],
            'table_set': [card_view(c) for c in ro['table_set']], 'table_owner': ro['table_owner'],
            'consecutive_scouts': ro['consecutive_scouts'], 'legal_actions': [action_view(a) for a in ro['legal_actions']],
            'num_players': ro['num_players'], 'current_player': ro['current_player'], 'num_cards': ro['num_cards'],
            'must_choose_orientation': ro['must_choose_orientation'], 'orientation_flipped': ro['orientation_flipped'],
            'table_front_top': ro['table_front_top'], 'table_back_top': ro['table_back_top'],
            'current_player_forced_scout': ro['current_player_forced_scout'],
            'legal_keys': [int(a) for a in state['legal_actions'].keys()],
            'action_record': (len(rec), record_view(rec[-1]) if rec else None)}


def perfect_view(info):
    """The canonical view of get_perfect_information (the reference's objects or rlcard_amd's)."""
    return {'keys': list(info.keys()), 'num_players': info['num_players'],
            'hand_cards': [[card_view(c) for c in h] for h in info['hand_cards']],
            'table_set': [card_view(c) for c in info['table_set']], 'table_owner': info['table_owner'],
            'current_player': info['current_player'], 'legal_actions': [int(a.action_id) for a in info['legal_actions']],
            'consecutive_scouts': info['consecutive_scouts']}


def test_scout_is_registered():
    from rlcard_amd.envs import _entry_points
    assert _entry_points['scout'] == ('rlcard_amd.envs.scout', 'ScoutEnv')
    assert _abi.game_id('scout') == 10 and 'scout' not in _abi.GAME_IDS   # (GAME_IDS: the games in oracle/)
    info, _ = _abi.game_info('scout')
    assert tuple(getattr(info, f) for f, _t in _abi.GameInfo._fields_) == (688, 204, 4, 26, 1, 24, 204, 9984, 24, 0, 64)
    with pytest.raises(_abi.CardsimError, match='scout: game_num_players must be 4'):
        _abi.game_info('scout', 3)


def test_make_needs_a_device_and_refuses_other_configs():
    import torch
    for cfg in ({'hand_size': 12}, {'rank_count': 9}, {'allow_step_back': True}, {'game_num_players': 3}):
        with pytest.raises(ValueError):
            rlcard_amd.make('scout', cfg)
    if not torch.cuda.is_available():   # no CPU fallback: the engine says so, as for every other game
        with pytest.raises(_abi.CardsimError):
            rlcard_amd.make('scout', {'seed': 1})
        with pytest.raises(_abi.CardsimError):
            rlcard_amd.make('bridge', {'seed': 1})


def test_action_table_is_the_references():
    names = [str(s) for s in gr.load('raw_scout')['action_names']]
    assert len(names) == 204 == len(scout.ACTIONS) == len(scout.ACTION_LIST) and names == scout.ACTION_LIST
    assert [str(a) for a in scout.ACTIONS] == names and [a.action_id for a in scout.ACTIONS] == list(range(204))
    assert names[0] == 'play-0-1' and names[15] == 'play-0-16' and names[16] == 'play-1-2' and names[135] == 'play-15-16'
    assert names[136:140] == ['scout-front-0-normal', 'scout-front-0-flip', 'scout-back-0-normal', 'scout-back-0-flip']
    assert names[203] == 'scout-back-16-flip'
    a = scout.ScoutEvent.from_action_id(137)
    assert (a.from_front, a.insertion_in_hand, a.flip) == (True, 0, True) and a == scout.ScoutAction(True, 0, True)
    p = scout.ScoutEvent.from_action_id(17)
    assert (p.start_idx, p.end_idx) == (1, 3) and repr(p) == 'play-1-3'
    with pytest.raises(Exception):
        scout.ScoutEvent.from_action_id(204)
    c = scout.ScoutCard(3, 7)
    assert (c.rank, str(c), str(c.flip()), c.flip().rank) == (3, '3/7', '7/3', 7)


def test_fixture_coverage_and_sizes():
    d = gr.load('scout')
    for k, v in NEED.items():
        assert int(d['cov_' + k]) >= v, k
    for ei in range(len(d['seeds'])):   # several consecutive games per seed
        assert len(set(d['ev_game'][d['ev_env'] == ei])) == 3
    assert d['ev_obs'].shape[1] == 688 and d['ev_legal'].shape[1] == 26 and d['ev_obs'].dtype == np.uint8
    assert len(d['fin_game']) == 4 * len(set(d['ev_game']))
    per_game = np.bincount(d['ev_game'])
    assert per_game.max() >= 301 and per_game.min() <= 9   # reset + steps
    lg = np.unpackbits(d['ev_legal'], axis=1, bitorder='little')
    assert not lg[:, 204:].any() and not lg[:, 200:204].any()   # (insertion point 16 needs a 16-card hand, which cannot scout)
    assert lg.sum(axis=1).max() >= 60
    assert str(d['python_version']).startswith('3.')
    assert len(d['rule_legal']) >= 1000 and len(d['rule_cmp']) >= 1000
    for name in ('scout', 'raw_scout'):
        assert os.path.getsize(os.path.join(gr.GOLDEN, name + '.npz')) <= LARGEST_FIXTURE
    r = gr.load('raw_scout')
    assert len(r['state']) == len(r['perfect']) == len(r['payoffs']) == len(r['kind']) > 100


def test_every_obs_row_is_consistent_with_its_stream():
    """the rows' own structure: one-hot card planes under the occupancy bytes, counts that agree with them, the owner
    flag, the current seat's legal mask against the forced flag"""
    d = gr.load('scout')
    obs = d['ev_obs']
    planes = obs[:, :640].reshape(-1, 4, 16, 10)
    occ = obs[:, 640:672].reshape(-1, 2, 16)
    assert obs[:, :677].max() == 1 and obs[:, 685].max() == 1
    assert np.array_equal(planes.sum(axis=3)[:, 0], occ[:, 0]) and np.array_equal(planes.sum(axis=3)[:, 1], occ[:, 0])
    assert np.array_equal(planes.sum(axis=3)[:, 2], occ[:, 1]) and np.array_equal(planes.sum(axis=3)[:, 3], occ[:, 1])
    assert not (planes[:, 0] & planes[:, 1]).any() and not (planes[:, 2] & planes[:, 3]).any()   # top != bottom
    assert (np.diff(occ.astype(np.int8), axis=2) <= 0).all()   # filled from position 0
    assert (obs[:, 672:677].sum(axis=1) == 1).all()
    assert np.array_equal(obs[:, 684], occ[:, 1].sum(axis=1)) and np.array_equal(obs[:, 676] == 1, obs[:, 684] == 0)
    player = d['ev_player']
    own = obs[np.arange(len(obs)), 678 + player]
    assert np.array_equal(own, occ[:, 0].sum(axis=1))
    assert obs[:, 677].max() == 3 and obs[:, 678:682].max() == 16 and obs[:, 686:].max() <= 10
    front = np.argmax(planes[:, 2, 0], axis=1) + 1
    assert np.array_equal(obs[:, 686], np.where(obs[:, 684] > 0, front, 0))
    lg = np.unpackbits(d['ev_legal'], axis=1, bitorder='little')
    assert np.array_equal(obs[:, 685] == 1, ~lg[:, :136].any(axis=1))
    assert np.array_equal(lg[:, 136:].any(axis=1), (obs[:, 684] > 0) & (own < 16))
    for j, g in enumerate(d['fin_game']):   # a seat's final row shows its own hand count
        row = d['fin_obs'][j]
        assert row[640:656].sum() == row[678 + j % 4]


def test_row_to_float32_reproduces_the_references_floats():
    d = gr.load('scout')
    assert set(d['frac_den'].tolist()) == {3, 10, 16}
    for den, num, bits in zip(d['frac_den'], d['frac_num'], d['frac_bits']):
        row = np.zeros(688, np.uint8)
        at = {3: 677, 10: 686, 16: 678}[int(den)]
        if den == 16 and num > 16:
            at = 682
        if at == 682:
            row[682], row[683] = int(num) & 255, int(num) >> 8
        else:
            row[at] = num
        got = scout.row_to_obs(row)
        assert got.dtype == np.float32 and got.view(np.uint32)[at] == bits, (den, num)
        assert np.float32(np.float64(num) / np.float64(den)).view(np.uint32) == bits
    for den, top in ((3, 3), (10, 10), (16, 16)):
        have = set(d['frac_num'][d['frac_den'] == den].tolist())
        assert set(range(top + 1)) <= have, (den, have)
    rows = d['ev_obs'][d['ref_rows_idx']]
    want = d['ref_rows_f32']
    assert want.dtype == np.float32 and len(rows) >= 30
    for row, ref in zip(rows, want):
        assert np.array_equal(scout.row_to_obs(row).view(np.uint32), ref.view(np.uint32))
        assert np.array_equal(scout.obs_to_row(ref), row)
    row = np.zeros(688, np.uint8)   # a score past one byte: 300 / 16 in entry 682, the table length in 683
    row[682], row[683], row[684] = 300 & 255, 300 >> 8, 5
    got = scout.row_to_obs(row)
    assert got[682] == np.float32(18.75) and got[683] == np.float32(5 / 16) and got[684] == 0


def test_raw_fixture_is_canonical_json():
    d = gr.load('raw_scout')
    for k in range(0, len(d['kind']), 23):
        s = json.loads(str(d['state'][k]))
        assert s['__dict__'][0][0] == 'keys'
        assert s['__dict__'][0][1] == ['obs', 'legal_actions', 'raw_obs', 'raw_legal_actions', 'action_record']
        assert s['__dict__'][2][1] == ['hand', 'points', 'table_set', 'table_owner', 'consecutive_scouts', 'legal_actions',
                                       'num_players', 'current_player', 'num_cards', 'must_choose_orientation',
                                       'orientation_flipped', 'table_front_top', 'table_back_top',
                                       'current_player_forced_scout']
        p = json.loads(str(d['perfect'][k]))
        assert p['__dict__'][0][1] == ['num_players', 'hand_cards', 'table_set', 'table_owner', 'current_player',
                                       'legal_actions', 'consecutive_scouts']
    assert set(np.unique(d['kind'])) <= {0, 1, 3}
    texts = ' '.join(str(s) for s in d['state'][:400])
    assert '"action_type","play"' in texts and '"action_type","scout"' in texts and '"direction","back"' in texts


# ---- the rules, compiled for the host under sanitizers ------------------------------------------------------------------
@pytest.fixture(scope='module')
def rules_exe(tmp_path_factory):
    exe = tmp_path_factory.mktemp('scout') / 'scout_rules_main'
    subprocess.run(['g++', '-std=c++17', '-O1', '-Wall', '-Werror', '-Wno-unknown-pragmas', '-fsanitize=address,undefined',
                    '-fno-sanitize-recover=all', os.path.join(ROOT, 'tools', 'scout_rules_main.cpp'), '-o', str(exe)],
                   check=True, capture_output=True)
    return str(exe)


def run_rules(exe, lines):
    p = subprocess.run([exe], input=('\n'.join(lines) + '\n').encode(), capture_output=True, timeout=300)
    assert p.returncode == 0, (p.returncode, p.stderr[-2000:])
    return p.stdout.decode().split('\n')[:len(lines)]


def lists_line(cmd, a, b):
    return '%s %d %s %d %s' % (cmd, len(a), ' '.join(map(str, a)), len(b), ' '.join(map(str, b)))


def mask_of(answer):
    w = answer.split()
    return sum(int(x, 16) << (64 * i) for i, x in enumerate(w[:4])), int(w[4])


def test_host_compiled_rules_match_every_recorded_answer(rules_exe):
    d = gr.load('scout')
    legal, cmp_ = d['rule_legal'], d['rule_cmp']
    lines = [lists_line('L', r[:r[16]].tolist(), r[17:17 + r[33]].tolist()) for r in legal]
    lines += [lists_line('S', r[:r[16]].tolist(), r[17:17 + r[33]].tolist()) for r in cmp_]
    got = iter(run_rules(rules_exe, lines))
    for r in legal:
        mask, forced = mask_of(next(got))
        assert mask == int.from_bytes(bytes(r[34:60].tolist()), 'little') and forced == int(r[60]), r
    for r in cmp_:
        assert [int(x) for x in next(got).split()] == [int(x) for x in r[34:39]], r
    assert (cmp_[:, 34] == 1).any() and (cmp_[:, 34] == 0).any() and set(cmp_[:, 35].tolist()) == {0, 1, 2}


# a direct restatement of the rules (round.get_legal_actions as the issue describes it), slice by slice
def direct_kind_rank(r):
    if len(r) == 1:
        return (0, r[0])
    if all(x == r[0] for x in r):
        return (2, r[0])
    steps = {b - a for a, b in zip(r, r[1:])}
    if steps == {1} or steps == {-1}:
        return (1, max(r[0], r[-1]))
    return (0, max(r))


def direct_valid(r):
    return len(r) < 2 or direct_kind_rank(r)[0] in (1, 2)


def direct_stronger(r, t):
    if not t:
        return True
    if len(r) != len(t):
        return len(r) > len(t)
    return direct_kind_rank(r) > direct_kind_rank(t)


def direct_legal(hand, table):
    ids = []
    for s in range(len(hand)):
        for e in range(s + 1, len(hand) + 1):
            if direct_valid(hand[s:e]) and direct_stronger(hand[s:e], table):
                ids.append(scout.ACTION_SPACE['play-%d-%d' % (s, e)])
    forced = not ids
    if table and len(hand) < 16:
        for i in range(len(hand) + 1):
            for k in range(4 if len(table) > 1 else 2):
                ids.append(136 + 4 * i + k)
    return sum(1 << i for i in ids), int(forced)


def random_list(rng):
    """0..16 ranks: uniform, or stitched from groups and runs so that long valid slices and equal lengths occur"""
    n = rng.randint(0, 16)
    if rng.random() < 0.4:
        return [rng.randint(1, 10) for _ in range(n)]
    out = []
    while len(out) < n:
        k, r, step = rng.randint(1, 5), rng.randint(1, 10), rng.choice((0, 1, -1))
        for _ in range(k):
            if 1 <= r <= 10:
                out.append(r)
            r += step
    return out[:n]


def test_host_compiled_rules_against_a_direct_restatement(rules_exe):
    rng = random.Random(20261021)
    cases = [(random_list(rng), random_list(rng)) for _ in range(120000)]
    cases += [([], []), ([5], []), ([], [5]), (list(range(1, 11)) + [10] * 6, [3] * 16), ([7] * 16, [7] * 15)]
    lines = [lists_line('L', h, t) for h, t in cases] + [lists_line('S', h, t) for h, t in cases[:20000]]
    lines += ['V %d %s' % (len(h), ' '.join(map(str, h))) for h, _ in cases[:20000]]
    got = iter(run_rules(rules_exe, lines))
    seen_words = set()
    for h, t in cases:
        mask, forced = mask_of(next(got))
        assert (mask, forced) == direct_legal(h, t), (h, t)
        seen_words |= {i for i in range(4) if (mask >> (64 * i)) & (2 ** 64 - 1)}
    assert seen_words == {0, 1, 2, 3}
    for h, t in cases[:20000]:
        a, b = (direct_kind_rank(h) if h else (0, 0)), (direct_kind_rank(t) if t else (0, 0))
        assert [int(x) for x in next(got).split()] == [int(direct_stronger(h, t)), a[0], a[1], b[0], b[1]], (h, t)
    for h, _ in cases[:20000]:
        assert int(next(got)) == int(direct_valid(h)), h
