"""CPU-side checks of UNO: the generated action table, the registries, the host rule agent against the reference's
recorded decisions (tests/golden/uno_rule.npz), a C99 consumer of CS_GAME_UNO, and the fixtures' own coverage
(tests/golden/gen_uno.py wrote them from the reference)."""
import json
import os
import subprocess

import numpy as np

import golden_replay as gr
import rlcard_amd
from rlcard_amd import _abi, models
from rlcard_amd.envs import uno

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_action_table_is_the_references():
    names = [str(s) for s in gr.load('uno')['action_names']]
    assert uno.ACTION_LIST == names and len(names) == 61
    assert [uno.ACTION_SPACE[a] for a in names] == list(range(61))
    assert names[0] == 'r-0' and names[59] == 'y-wild_draw_4' and names[60] == 'draw'


def test_uno_is_registered():
    from rlcard_amd.envs import _entry_points
    assert _entry_points['uno'] == ('rlcard_amd.envs.uno', 'UnoEnv')
    assert _abi.game_id('uno') == 5 and 'uno' not in _abi.GAME_IDS   # (GAME_IDS: the games with an oracle restatement)
    info, _ = _abi.game_info('uno')
    assert tuple(getattr(info, f) for f, _t in _abi.GameInfo._fields_) == (240, 61, 2, 8, 1, 56, 61, 9984, 56, 0, 64)
    model = models.load('uno-rule-v1')
    assert len(model.agents) == 2 and model.agents[0].use_raw and model.agents[0].policy_id == 1
    assert models.policy_id_of('uno-rule-v1') == 1
    assert rlcard_amd.models.uno_rule_models.UNORuleModelV1 is type(model)


def test_host_rule_agent_matches_reference_decisions():
    z = gr.load('uno_rule')
    agent = models.load('uno-rule-v1').agents[0]
    per_branch = {0: 0, 1: 0, 2: 0}
    np.random.seed(3)
    for s, b, a, allowed in zip(z['state'], z['branch'], z['action'], z['allowed']):
        state = json.loads(str(s))
        got = agent.step(state)
        assert got in json.loads(str(allowed)), (state, got)
        if b != 2:   # draw, and the wild_draw_4 colour choice: deterministic
            assert got == str(a), (state, got, a)
        assert agent.eval_step(state)[1] == []
        per_branch[int(b)] += 1
    assert min(per_branch.values()) >= 50, per_branch
    assert int(z['cov_ties']) >= 1   # colour-count ties (the first colour in hand order wins)
    assert int(z['cov_all_wild']) >= 1   # the search found all-wild hands (the wild filter is skipped there)


C_SOURCE = r'''
#include <stdio.h>
#include "cardsim.h"
int main(void)
{
    cs_game_info info;
    cs_config cfg = {0};
    int r = cs_game_info_get(CS_GAME_UNO, &cfg, &info);
    printf("%d %d %d %d %d %d\n", r, info.obs_dim, info.num_actions, info.num_players, info.legal_bytes,
           info.action_bytes);
    cfg.num_players = 3;
    r = cs_game_info_get(CS_GAME_UNO, &cfg, &info);
    printf("%d %s\n", r, cs_last_error());
    return CS_GAME_UNO == 5 && cs_abi_version() == 3 ? 0 : 1;
}
'''


def test_c99_consumer_of_the_uno_game_id(tmp_path):
    src = tmp_path / 'uno_game.c'
    src.write_text(C_SOURCE)
    exe = tmp_path / 'uno_game'
    libdir = os.path.dirname(_abi.LIB_PATH)
    rocm_lib = '/opt/rocm/lib'
    subprocess.run(['gcc', '-std=c99', '-Wall', '-Werror', '-I', os.path.join(ROOT, 'include'), str(src), '-o', str(exe),
                    '-L', libdir, '-lcardsim', '-Wl,-rpath,' + libdir, '-Wl,-rpath,' + rocm_lib,
                    '-Wl,-rpath-link,' + rocm_lib], check=True, capture_output=True)
    p = subprocess.run([str(exe)], capture_output=True, timeout=60)
    lines = p.stdout.decode().splitlines()
    assert p.returncode == 0 and lines[0].split() == ['0', '240', '61', '2', '8', '1'], (p.stdout, p.stderr)
    assert lines[1].startswith('-4 uno: game_num_players must be 2'), lines


def test_fixture_coverage():
    d = gr.load('uno')
    need = {'rep_draw': 3, 'rep_draw2': 1, 'top_wd4_reshuffle': 2, 'top_skip': 1, 'top_reverse': 1, 'top_draw_2': 1,
            'top_wild': 1, 'wild_target_recoloured': 1, 'two_copies': 1, 'long_game': 1,
            'wild_in_hand_recoloured': 1}
    for k, v in need.items():
        assert int(d['cov_' + k]) >= v, k
    assert int(d['cov_max_steps']) > 150
    assert int(d['cov_wd4_replace']) >= 0   # a replace_deck through wild_draw_4: recorded whether the search found one
    # illegal ids in the stream: events whose action is not in the legal mask of the event before it
    assert int(d['cov_illegal_id']) >= 20
    # several consecutive games per seed
    for ei in range(len(d['seeds'])):
        assert len(set(d['ev_game'][d['ev_env'] == ei])) >= 3
    for name in ('uno', 'raw_uno', 'uno_rule'):
        assert os.path.getsize(os.path.join(gr.GOLDEN, name + '.npz')) <= 500 * 1000


def test_every_obs_row_has_61_ones():
    d = gr.load('uno')
    assert d['ev_obs'].shape[1] == 240 and d['ev_obs'].max() == 1
    assert (d['ev_obs'].sum(axis=1) == 61).all() and (d['fin_obs'].sum(axis=1) == 61).all()
    assert d['ev_legal'].shape[1] == 8
    # plane 2 (two copies of a card) and a recoloured wild target are really in the observed rows
    assert d['ev_obs'][:, 120:180].any()


def test_raw_fixture_is_canonical_json():
    d = gr.load('raw_uno')
    n = len(d['kind'])
    assert n > 200 and len(d['state']) == n == len(d['perfect']) == len(d['payoffs'])
    for k in range(0, n, 37):
        s = json.loads(str(d['state'][k]))
        json.loads(str(d['perfect'][k]))
        assert s['__dict__'][0][0] == 'raw_obs'
    assert set(np.unique(d['kind'])) <= {0, 1, 3}


def test_step_back_and_player_count_are_refused_before_the_engine():
    import pytest
    with pytest.raises(ValueError, match='UNO'):
        rlcard_amd.make('uno', {'allow_step_back': True})
    with pytest.raises(ValueError, match='game_num_players must be 2'):
        rlcard_amd.VecEnv('uno', 4, config={'game_num_players': 3})
