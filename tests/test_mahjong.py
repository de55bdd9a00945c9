"""CPU-side checks of Mahjong: the registries and the game's static shape, the action table, a C99 consumer of
CS_GAME_MAHJONG, the fixtures' own coverage and internal consistency (tests/golden/gen_mahjong.py wrote them from the
reference), and the win judge of the kernels (rlcard_amd/csrc/cs_mahjong_hu.h) compiled for the host into a small
stand-alone program and run over every row of tests/golden/mahjong_hu.npz.

raw_view() is the canon of the raw fixture (raw_mahjong.npz): the reference's state dicts hold tile objects, which
tests/rawcanon.py has no form for, so every tile becomes its get_str() string first; everything else is rawcanon's."""
import os
import subprocess

import numpy as np

import golden_replay as gr
import rawcanon
from rlcard_amd import _abi
from rlcard_amd.envs import mahjong

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEED = {'win_hand': 3, 'win_piles': 3, 'exhausted': 2, 'winner_seat1': 1, 'winner_seat2': 1, 'winner_seat3': 1,
        'pong': 10, 'gong': 3, 'chow': 3, 'wrap_chow': 1, 'stand_then_chow': 1, 'stand_chain_draw': 1, 'illegal_id': 20}


def _s(x):
    return x if isinstance(x, str) else x.get_str()


def raw_view(state):
    """The canonical view of a Mahjong Env state dict (the reference's or rlcard_amd's): tiles as strings."""
    raw = state['raw_obs']
    view = {'valid_act': [_s(x) for x in raw['valid_act']], 'table': [_s(c) for c in raw['table']],
            'player': raw['player'], 'current_hand': [_s(c) for c in raw['current_hand']],
            'players_pile': {p: [[_s(c) for c in pile] for pile in piles] for p, piles in raw['players_pile'].items()},
            'action_cards': [_s(c) for c in raw['action_cards']]}
    assert list(raw.keys()) == list(view.keys())
    return {'raw_obs': view, 'raw_legal_actions': [_s(c) for c in state['raw_legal_actions']],
            'legal_keys': list(state['legal_actions'].keys()),
            'action_record': [(p, _s(a)) for p, a in state['action_record']]}


def test_mahjong_is_registered():
    from rlcard_amd.envs import _entry_points
    assert _entry_points['mahjong'] == ('rlcard_amd.envs.mahjong', 'MahjongEnv')
    assert _abi.game_id('mahjong') == 6 and 'mahjong' not in _abi.GAME_IDS   # (GAME_IDS: the games in oracle/)
    info, _ = _abi.game_info('mahjong')
    assert tuple(getattr(info, f) for f, _t in _abi.GameInfo._fields_) == (816, 38, 4, 5, 1, 55, 38, 9984, 55, 0, 64)
    assert 'cs_debug_mahjong_hu' in _abi.SYMBOLS


def test_action_table_is_the_references():
    names = [str(s) for s in gr.load('mahjong')['action_names']]
    assert mahjong.ACTION_LIST == names and len(names) == 38
    assert names[0] == 'bamboo-1' and names[26] == 'dots-9' and names[27] == 'dragons-green'
    assert names[33] == 'winds-south' and names[34:] == ['pong', 'chow', 'gong', 'stand']
    assert [c.get_str() for c in mahjong.CARDS] == names[:34]
    assert [mahjong.CARDS[t].index_num for t in (0, 8, 9, 26, 27, 29, 30, 33)] == [0, 8, 0, 8, 0, 2, 0, 3]


C_SOURCE = r'''
#include <stdio.h>
#include "cardsim.h"
int main(void)
{
    cs_game_info info;
    cs_config cfg = {0};
    int r = cs_game_info_get(CS_GAME_MAHJONG, &cfg, &info);
    printf("%d %d %d %d %d %d\n", r, info.obs_dim, info.num_actions, info.num_players, info.legal_bytes,
           info.action_bytes);
    cfg.num_players = 3;
    r = cs_game_info_get(CS_GAME_MAHJONG, &cfg, &info);
    printf("%d %s\n", r, cs_last_error());
    return CS_GAME_MAHJONG == 6 && cs_abi_version() == 3 ? 0 : 1;
}
'''


def test_c99_consumer_of_the_mahjong_game_id(tmp_path):
    src = tmp_path / 'mahjong_game.c'
    src.write_text(C_SOURCE)
    exe = tmp_path / 'mahjong_game'
    libdir = os.path.dirname(_abi.LIB_PATH)
    rocm_lib = '/opt/rocm/lib'
    subprocess.run(['gcc', '-std=c99', '-Wall', '-Werror', '-I', os.path.join(ROOT, 'include'), str(src), '-o', str(exe),
                    '-L', libdir, '-lcardsim', '-Wl,-rpath,' + libdir, '-Wl,-rpath,' + rocm_lib,
                    '-Wl,-rpath-link,' + rocm_lib], check=True, capture_output=True)
    p = subprocess.run([str(exe)], capture_output=True, timeout=60)
    lines = p.stdout.decode().splitlines()
    assert p.returncode == 0 and lines[0].split() == ['0', '816', '38', '4', '5', '1'], (p.stdout, p.stderr)
    assert lines[1].startswith('-4 mahjong: game_num_players must be 4'), lines


def test_fixture_coverage_and_sizes():
    d = gr.load('mahjong')
    for k, v in NEED.items():
        assert int(d['cov_' + k]) >= v, k
    for ei in range(len(d['seeds'])):   # several consecutive games per seed
        assert len(set(d['ev_game'][d['ev_env'] == ei])) >= 3
    assert len(d['fin_game']) == 4 * len(set(d['ev_game']))   # the final observations of all four seats
    # the payoff rows: +1 / -1 / -1 / -1 or all zero, every seat winning somewhere
    pay = d['ev_payoff'][d['ev_done'] != 0]
    assert {tuple(sorted(r)) for r in pay.tolist()} == {(-1.0, -1.0, -1.0, 1.0), (0.0, 0.0, 0.0, 0.0)}
    assert set(np.argmax(pay[pay.max(axis=1) > 0], axis=1)) == {0, 1, 2, 3}
    h = gr.load('mahjong_hu')
    assert h['pat_sets'].shape == (3 ** 9,) and len(h['win']) >= 2000 and int(h['win'].sum()) >= 200
    assert set(np.unique(h['piles'])) == {0, 1, 2, 3, 4} and {11, 14} <= set(np.unique(h['len']))
    if bool(h['order_matters']):   # two permutations of one hand with different answers
        lo, hi = (int(x) for x in h['order_pair'])
        assert sorted(h['hands'][lo][:h['len'][lo]]) == sorted(h['hands'][hi][:h['len'][hi]])
        assert h['piles'][lo] == h['piles'][hi] and h['win'][lo] != h['win'][hi]
    for name in ('mahjong', 'mahjong_hu', 'raw_mahjong'):
        assert os.path.getsize(os.path.join(gr.GOLDEN, name + '.npz')) <= 500 * 1000


def test_every_obs_row_is_consistent_with_its_stream():
    """Per row: every tile's four columns are filled from column 0; a reset row is 14 hand tiles and nothing else; the
    hand plane holds as many tiles as the hand it shows -- each seat's hand size is followed through the stream: 13
    after the deal (14 for seat 0), -1 per discard, -2 per pong, -3 per gong, one less than the chow's pile per chow,
    +1 for the seat that draws when no claim is offered -- in the step rows and in the final rows of all four seats
    (a claim on offer shows the claimer's hand to everyone); without a claim on offer the hand plane's tiles are the
    legal ids; the table plane holds the discards so far less the chows, the pile planes 3 per pong, 4 per gong and 2
    or 3 per chow."""
    d = gr.load('mahjong')
    obs = np.concatenate([d['ev_obs'], d['fin_obs']]).reshape(-1, 6, 34, 4)
    assert obs.max() == 1 and (np.diff(obs.astype(np.int8), axis=3) <= 0).all()
    ev = d['ev_obs'].reshape(-1, 6, 34, 4)
    fin = d['fin_obs'].reshape(-1, 6, 34, 4)
    fin_rows = {}
    for j, g in enumerate(d['fin_game']):
        fin_rows.setdefault(int(g), []).append(j)
    legal = np.unpackbits(d['ev_legal'], axis=1, bitorder='little')[:, :38]
    assert d['ev_legal'].shape[1] == 5
    played = pongs = gongs = chows = finals = 0
    size = [0, 0, 0, 0]
    for k in range(len(ev)):
        cur, offered = int(d['ev_player'][k]), bool(legal[k, 37])
        if d['ev_kind'][k] == 0:
            assert ev[k, 0].sum() == 14 and ev[k, 1:].sum() == 0 and cur == 0 and not offered
            played = pongs = gongs = chows = 0
            size = [14, 13, 13, 13]
        else:
            a, actor = int(d['ev_act'][k]), int(d['ev_player'][k - 1])
            if not legal[k - 1, a]:
                a = int(np.argmax(legal[k - 1]))   # an illegal id plays the lowest legal id
            played += a < 34
            pongs += a == 34
            chows += a == 35
            gongs += a == 36
            if a < 34:
                size[actor] -= 1
            elif a == 34:
                size[actor] -= 2
            elif a == 36:
                size[actor] -= 3
            elif a == 35:   # the pile's tiles but the table's: two hand tiles, one for the wrap-around chow
                grown = int(ev[k, 2 + actor].sum()) - int(ev[k - 1, 2 + actor].sum())
                assert grown in (2, 3), k
                size[actor] -= grown - 1
            if (a < 34 or a == 37) and not offered:
                size[cur] += 1   # nobody claims (any more): the next seat draws
        assert ev[k, 0].sum() == size[cur], (k, size)   # hand plane = hand size (the observer is the current player)
        assert ev[k, 1].sum() == played - chows, k
        piles = int(ev[k, 2:].sum()) - 3 * pongs - 4 * gongs
        assert 2 * chows <= piles <= 3 * chows, k
        if offered:
            assert legal[k].sum() == 2 and legal[k, 34:37].sum() == 1, k
        else:
            assert np.array_equal(ev[k, 0, :, 0], legal[k, :34]) and not legal[k, 34:].any(), k
        if d['ev_done'][k]:   # the final rows of the four seats: their own hands, the claimer's while a claim is offered
            rows = fin_rows[int(d['ev_game'][k])]
            assert len(rows) == 4
            for p, j in enumerate(rows):
                assert fin[j, 0].sum() == size[cur if offered else p], (k, p)
                assert np.array_equal(fin[j, 1:], ev[k, 1:]), (k, p)   # table and piles are everyone's
            finals += 1
    assert finals == len(fin_rows) and min(size) >= 1 and d['ev_obs'].shape[1] == 816


def test_raw_fixture_is_canonical_json():
    import json
    d = gr.load('raw_mahjong')
    n = len(d['kind'])
    assert n > 100 and len(d['state']) == n == len(d['payoffs'])
    for k in range(0, n, 29):
        s = json.loads(str(d['state'][k]))
        assert s['__dict__'][0][0] == 'raw_obs'
    assert set(np.unique(d['kind'])) <= {0, 1, 3}
    view = raw_view({'raw_obs': {'valid_act': ['play'], 'table': [], 'player': 0, 'current_hand': [mahjong.CARDS[3]],
                                 'players_pile': {0: [], 1: [], 2: [], 3: []}, 'action_cards': [mahjong.CARDS[3]]},
                     'raw_legal_actions': [mahjong.CARDS[3]], 'legal_actions': {3: None},
                     'action_record': [(0, mahjong.CARDS[5]), (1, 'stand')]})
    assert '"bamboo-4"' in rawcanon.dumps(view) and view['action_record'] == [(0, 'bamboo-6'), (1, 'stand')]


HOST_JUDGE = r'''
// reads "n" then n rows "len piles t0 .. t13" -> one judge_hu answer per row; then "m" patterns of nine counts -> cal_set
#include <cstdio>
#include "cs_mahjong_hu.h"
int main()
{
    long n = 0, m = 0;
    if (scanf("%ld", &n) != 1) return 2;
    for (long i = 0; i < n; i++) {
        int len, piles, t;
        uint32_t h[4] = {0, 0, 0, 0};
        if (scanf("%d %d", &len, &piles) != 2) return 2;
        for (int k = 0; k < 14; k++) {
            if (scanf("%d", &t) != 1) return 2;
            h[k >> 2] |= (uint32_t)t << (8 * (k & 3));
        }
        printf("%d\n", (int)cs::mj::judge_hu(h, len, piles));
    }
    if (scanf("%ld", &m) != 1) return 2;
    for (long i = 0; i < m; i++) {
        cs::mj::Counts c{{0, 0, 0, 0}};
        int v;
        for (int k = 0; k < 9; k++) {
            if (scanf("%d", &v) != 1) return 2;
            c.s[1] |= (uint64_t)v << (4 * k);
        }
        uint64_t used = 0;
        const int sets = cs::mj::cal_set(c, used);
        printf("%d %llu\n", sets, (unsigned long long)(used >> 9));
    }
    return 0;
}
'''


def test_host_compiled_judge_matches_every_recorded_row(tmp_path):
    h = gr.load('mahjong_hu')
    src = tmp_path / 'judge_main.cpp'
    src.write_text(HOST_JUDGE)
    exe = tmp_path / 'judge_main'
    subprocess.run(['g++', '-std=c++17', '-O1', '-Wall', '-Werror', '-fsanitize=address,undefined',
                    '-fno-sanitize-recover=all', '-I', os.path.join(ROOT, 'rlcard_amd', 'csrc'), str(src), '-o',
                    str(exe)], check=True, capture_output=True)
    n = len(h['win'])
    lines = [str(n)]
    for i in range(n):
        lines.append('%d %d %s' % (h['len'][i], h['piles'][i], ' '.join(str(int(t)) for t in h['hands'][i])))
    lines.append(str(3 ** 9))
    for code in range(3 ** 9):
        lines.append(' '.join(str((code // 3 ** v) % 3) for v in range(9)))
    p = subprocess.run([str(exe)], input='\n'.join(lines).encode(), capture_output=True, timeout=120)
    assert p.returncode == 0, p.stderr[-2000:]
    out = p.stdout.decode().split('\n')
    got = np.array([int(x) for x in out[:n]], np.uint8)
    bad = np.nonzero(got != h['win'])[0]
    assert len(bad) == 0, (bad[:10], h['hands'][bad[0]], h['len'][bad[0]], h['piles'][bad[0]])
    pats = np.array([[int(x) for x in line.split()] for line in out[n:n + 3 ** 9]], np.int64)
    assert np.array_equal(pats[:, 0], h['pat_sets']) and np.array_equal(pats[:, 1], h['pat_used'])
