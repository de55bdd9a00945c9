"""CPU-side checks of the C ABI boundary: the in-tree library loads and exports every symbol include/cardsim.h
declares; calls fail loudly (no CPU fallback) without a GPU."""
import ctypes as C
import os
import re

import pytest

from rlcard_amd import _abi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def header_symbols():
    src = open(os.path.join(ROOT, 'include', 'cardsim.h')).read()
    return sorted(set(re.findall(r'\b(cs_[a-z0-9_]+)\s*\(', src)))


def test_library_exports_every_declared_symbol():
    L = _abi.lib()
    declared = header_symbols()
    assert set(declared) == set(_abi.SYMBOLS)
    for s in declared:
        assert hasattr(L, s), s


def test_game_info_shapes():
    shapes = {'leduc-holdem': (36, 4, 2, 1, 1), 'limit-holdem': (72, 4, 2, 1, 1), 'blackjack': (2, 2, 1, 1, 1),
              'doudizhu': (901, 27472, 3, 3434, 2), 'no-limit-holdem': (54, 5, 2, 1, 1)}
    epw = {'leduc-holdem': 64, 'limit-holdem': 32, 'blackjack': 64, 'doudizhu': 2, 'no-limit-holdem': 32}
    for game, (o, a, p, lb, ab) in shapes.items():
        info, _ = _abi.game_info(game)
        assert (info.obs_dim, info.num_actions, info.num_players, info.legal_bytes, info.action_bytes) == \
            (o, a, p, lb, ab)
        assert info.envs_per_wave == epw[game], game   # cs_traj_probe's write pattern
    for game, n in (('limit-holdem', 5), ('no-limit-holdem', 12), ('leduc-holdem', 4)):
        assert _abi.game_info(game, n)[0].envs_per_wave == 64
    assert _abi.game_info('blackjack', 6, 8)[0].envs_per_wave == 64
    assert _abi.ABI_VERSION == 2 and _abi.lib().cs_abi_version() == 3   # 3: + cs_state_bytes / _save / _load


def test_doudizhu_action_table_is_compiled_in():
    """The .incbin'd table is the one tools/gen_ddz_table.py derives from the reference capture."""
    import importlib.util
    spec = importlib.util.spec_from_file_location('gen_ddz_table', os.path.join(ROOT, 'tools', 'gen_ddz_table.py'))
    g = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(g)
    blob = g.build(os.path.join(ROOT, 'tests', 'golden', 'ddz_actions.npz'))
    assert open(os.path.join(ROOT, 'rlcard_amd', 'csrc', 'ddz_actions.bin'), 'rb').read() == blob
    assert blob in open(_abi.LIB_PATH, 'rb').read()


def test_create_fails_loudly_without_gpu():
    import torch
    if torch.cuda.is_available():
        pytest.skip('GPU present')
    h = C.c_void_p()
    cfg = _abi.Config(0, -1)
    rc = _abi.lib().cs_create(C.byref(h), 1, 64, 0, C.byref(cfg))
    assert rc == -2 and b'GPU' in _abi.lib().cs_last_error()
    with pytest.raises(_abi.CardsimError):
        _abi.check(rc, 'cs_create')


def test_invalid_arguments_are_rejected():
    info = _abi.GameInfo()
    assert _abi.lib().cs_game_info_get(9, None, C.byref(info)) == -4
    assert _abi.lib().cs_create(None, 1, 64, 0, None) == -1


def test_nplayer_game_info():
    """game_num_players 3..22 (Leduc 3..5; 2P + 5 <= 52 dealt cards): same obs / action shapes, one packed word per
    player plus shared words, no deal queue (cs_holdem_n.h); counts past the engine's range are refused."""
    for game, words_extra, top in (('leduc-holdem', 1, 5), ('limit-holdem', 3, 22), ('no-limit-holdem', 3, 22)):
        two, _ = _abi.game_info(game, 2)
        for n in range(3, top + 1):
            info, _ = _abi.game_info(game, n)
            assert (info.obs_dim, info.num_actions, info.legal_bytes) == (two.obs_dim, two.num_actions, two.legal_bytes)
            assert info.num_players == n and info.state_words == n + words_extra
        with pytest.raises(_abi.CardsimError):
            _abi.game_info(game, top + 1)
    info, _ = _abi.game_info('no-limit-holdem', 6, chips_for_each=50, dealer_id=5)
    assert info.num_players == 6


# cs_game_info of every supported (game, game_num_players, game_num_decks; 0 / -1: default), recorded from the library
# as it stood before the launch table (cs_engine.h GameOps) replaced the per-entry-point dispatch. Columns: obs_dim,
# num_actions, num_players, legal_bytes, action_bytes, state_words, action_feature_dim, rng_period, game_words,
# deal_queue_depth, envs_per_wave.
GAME_INFO = {
    ('blackjack', 0, -1): (2, 2, 1, 1, 1, 32, 2, 9984, 32, 0, 64),
    ('leduc-holdem', 0, -1): (36, 4, 2, 1, 1, 2, 4, 9984, 2, 0, 64),
    ('limit-holdem', 0, -1): (72, 4, 2, 1, 1, 21, 4, 9984, 4, 8, 32),
    ('doudizhu', 0, -1): (901, 27472, 3, 3434, 2, 36, 54, 1248, 36, 0, 2),
    ('no-limit-holdem', 0, -1): (54, 5, 2, 1, 1, 21, 5, 9984, 4, 8, 32),
    ('leduc-holdem', 3, -1): (36, 4, 3, 1, 1, 4, 4, 9984, 4, 0, 64),
    ('leduc-holdem', 4, -1): (36, 4, 4, 1, 1, 5, 4, 9984, 5, 0, 64),
    ('leduc-holdem', 5, -1): (36, 4, 5, 1, 1, 6, 4, 9984, 6, 0, 64),
    ('limit-holdem', 3, -1): (72, 4, 3, 1, 1, 6, 4, 9984, 6, 0, 64),
    ('limit-holdem', 4, -1): (72, 4, 4, 1, 1, 7, 4, 9984, 7, 0, 64),
    ('limit-holdem', 5, -1): (72, 4, 5, 1, 1, 8, 4, 9984, 8, 0, 64),
    ('limit-holdem', 6, -1): (72, 4, 6, 1, 1, 9, 4, 9984, 9, 0, 64),
    ('limit-holdem', 7, -1): (72, 4, 7, 1, 1, 10, 4, 9984, 10, 0, 64),
    ('limit-holdem', 8, -1): (72, 4, 8, 1, 1, 11, 4, 9984, 11, 0, 64),
    ('limit-holdem', 9, -1): (72, 4, 9, 1, 1, 12, 4, 9984, 12, 0, 64),
    ('limit-holdem', 10, -1): (72, 4, 10, 1, 1, 13, 4, 9984, 13, 0, 64),
    ('limit-holdem', 11, -1): (72, 4, 11, 1, 1, 14, 4, 9984, 14, 0, 64),
    ('limit-holdem', 12, -1): (72, 4, 12, 1, 1, 15, 4, 9984, 15, 0, 64),
    ('limit-holdem', 13, -1): (72, 4, 13, 1, 1, 16, 4, 9984, 16, 0, 64),
    ('limit-holdem', 14, -1): (72, 4, 14, 1, 1, 17, 4, 9984, 17, 0, 64),
    ('limit-holdem', 15, -1): (72, 4, 15, 1, 1, 18, 4, 9984, 18, 0, 64),
    ('limit-holdem', 16, -1): (72, 4, 16, 1, 1, 19, 4, 9984, 19, 0, 64),
    ('limit-holdem', 17, -1): (72, 4, 17, 1, 1, 20, 4, 9984, 20, 0, 64),
    ('limit-holdem', 18, -1): (72, 4, 18, 1, 1, 21, 4, 9984, 21, 0, 64),
    ('limit-holdem', 19, -1): (72, 4, 19, 1, 1, 22, 4, 9984, 22, 0, 64),
    ('limit-holdem', 20, -1): (72, 4, 20, 1, 1, 23, 4, 9984, 23, 0, 64),
    ('limit-holdem', 21, -1): (72, 4, 21, 1, 1, 24, 4, 9984, 24, 0, 64),
    ('limit-holdem', 22, -1): (72, 4, 22, 1, 1, 25, 4, 9984, 25, 0, 64),
    ('no-limit-holdem', 3, -1): (54, 5, 3, 1, 1, 6, 5, 9984, 6, 0, 64),
    ('no-limit-holdem', 4, -1): (54, 5, 4, 1, 1, 7, 5, 9984, 7, 0, 64),
    ('no-limit-holdem', 5, -1): (54, 5, 5, 1, 1, 8, 5, 9984, 8, 0, 64),
    ('no-limit-holdem', 6, -1): (54, 5, 6, 1, 1, 9, 5, 9984, 9, 0, 64),
    ('no-limit-holdem', 7, -1): (54, 5, 7, 1, 1, 10, 5, 9984, 10, 0, 64),
    ('no-limit-holdem', 8, -1): (54, 5, 8, 1, 1, 11, 5, 9984, 11, 0, 64),
    ('no-limit-holdem', 9, -1): (54, 5, 9, 1, 1, 12, 5, 9984, 12, 0, 64),
    ('no-limit-holdem', 10, -1): (54, 5, 10, 1, 1, 13, 5, 9984, 13, 0, 64),
    ('no-limit-holdem', 11, -1): (54, 5, 11, 1, 1, 14, 5, 9984, 14, 0, 64),
    ('no-limit-holdem', 12, -1): (54, 5, 12, 1, 1, 15, 5, 9984, 15, 0, 64),
    ('no-limit-holdem', 13, -1): (54, 5, 13, 1, 1, 16, 5, 9984, 16, 0, 64),
    ('no-limit-holdem', 14, -1): (54, 5, 14, 1, 1, 17, 5, 9984, 17, 0, 64),
    ('no-limit-holdem', 15, -1): (54, 5, 15, 1, 1, 18, 5, 9984, 18, 0, 64),
    ('no-limit-holdem', 16, -1): (54, 5, 16, 1, 1, 19, 5, 9984, 19, 0, 64),
    ('no-limit-holdem', 17, -1): (54, 5, 17, 1, 1, 20, 5, 9984, 20, 0, 64),
    ('no-limit-holdem', 18, -1): (54, 5, 18, 1, 1, 21, 5, 9984, 21, 0, 64),
    ('no-limit-holdem', 19, -1): (54, 5, 19, 1, 1, 22, 5, 9984, 22, 0, 64),
    ('no-limit-holdem', 20, -1): (54, 5, 20, 1, 1, 23, 5, 9984, 23, 0, 64),
    ('no-limit-holdem', 21, -1): (54, 5, 21, 1, 1, 24, 5, 9984, 24, 0, 64),
    ('no-limit-holdem', 22, -1): (54, 5, 22, 1, 1, 25, 5, 9984, 25, 0, 64),
    ('blackjack', 1, -1): (2, 2, 1, 1, 1, 32, 2, 9984, 32, 0, 64),
    ('blackjack', 1, 0): (2, 2, 1, 1, 1, 32, 2, 9984, 32, 0, 64),
    ('blackjack', 1, 1): (2, 2, 1, 1, 1, 32, 2, 9984, 32, 0, 64),
    ('blackjack', 1, 2): (2, 2, 1, 1, 1, 168, 2, 624, 168, 0, 64),
    ('blackjack', 1, 8): (2, 2, 1, 1, 1, 168, 2, 624, 168, 0, 64),
    ('blackjack', 2, -1): (2, 2, 2, 1, 1, 32, 2, 9984, 32, 0, 64),
    ('blackjack', 2, 0): (2, 2, 2, 1, 1, 32, 2, 9984, 32, 0, 64),
    ('blackjack', 2, 1): (2, 2, 2, 1, 1, 32, 2, 9984, 32, 0, 64),
    ('blackjack', 2, 2): (2, 2, 2, 1, 1, 168, 2, 624, 168, 0, 64),
    ('blackjack', 2, 8): (2, 2, 2, 1, 1, 168, 2, 624, 168, 0, 64),
    ('blackjack', 3, -1): (2, 2, 3, 1, 1, 32, 2, 9984, 32, 0, 64),
    ('blackjack', 3, 0): (2, 2, 3, 1, 1, 32, 2, 9984, 32, 0, 64),
    ('blackjack', 3, 1): (2, 2, 3, 1, 1, 32, 2, 9984, 32, 0, 64),
    ('blackjack', 3, 2): (2, 2, 3, 1, 1, 168, 2, 624, 168, 0, 64),
    ('blackjack', 3, 8): (2, 2, 3, 1, 1, 168, 2, 624, 168, 0, 64),
    ('blackjack', 4, -1): (2, 2, 4, 1, 1, 32, 2, 9984, 32, 0, 64),
    ('blackjack', 4, 0): (2, 2, 4, 1, 1, 32, 2, 9984, 32, 0, 64),
    ('blackjack', 4, 1): (2, 2, 4, 1, 1, 32, 2, 9984, 32, 0, 64),
    ('blackjack', 4, 2): (2, 2, 4, 1, 1, 168, 2, 624, 168, 0, 64),
    ('blackjack', 4, 8): (2, 2, 4, 1, 1, 168, 2, 624, 168, 0, 64),
    ('blackjack', 5, -1): (2, 2, 5, 1, 1, 168, 2, 624, 168, 0, 64),
    ('blackjack', 5, 0): (2, 2, 5, 1, 1, 168, 2, 624, 168, 0, 64),
    ('blackjack', 5, 1): (2, 2, 5, 1, 1, 168, 2, 624, 168, 0, 64),
    ('blackjack', 5, 2): (2, 2, 5, 1, 1, 168, 2, 624, 168, 0, 64),
    ('blackjack', 5, 8): (2, 2, 5, 1, 1, 168, 2, 624, 168, 0, 64),
    ('blackjack', 6, -1): (2, 2, 6, 1, 1, 168, 2, 624, 168, 0, 64),
    ('blackjack', 6, 0): (2, 2, 6, 1, 1, 168, 2, 624, 168, 0, 64),
    ('blackjack', 6, 1): (2, 2, 6, 1, 1, 168, 2, 624, 168, 0, 64),
    ('blackjack', 6, 2): (2, 2, 6, 1, 1, 168, 2, 624, 168, 0, 64),
    ('blackjack', 6, 8): (2, 2, 6, 1, 1, 168, 2, 624, 168, 0, 64),
    ('blackjack', 7, -1): (2, 2, 7, 1, 1, 168, 2, 624, 168, 0, 64),
    ('blackjack', 7, 0): (2, 2, 7, 1, 1, 168, 2, 624, 168, 0, 64),
    ('blackjack', 7, 1): (2, 2, 7, 1, 1, 168, 2, 624, 168, 0, 64),
    ('blackjack', 7, 2): (2, 2, 7, 1, 1, 168, 2, 624, 168, 0, 64),
    ('blackjack', 7, 8): (2, 2, 7, 1, 1, 168, 2, 624, 168, 0, 64),
}
NOLIMIT_6_CHIPS50_DEALER5 = (54, 5, 6, 1, 1, 9, 5, 9984, 9, 0, 64)
# (game id, num_players, num_decks, chips_for_each, dealer_plus1, rng_mode) the engine refuses
REFUSED = {'leduc 6 players': (1, 6, -1, 0, 0, 0), 'limit 23 players': (2, 23, -1, 0, 0, 0),
           'blackjack 8 players': (0, 8, -1, 0, 0, 0), 'blackjack 9 decks': (0, 1, 9, 0, 0, 0),
           'blackjack shoe with philox': (0, 1, 2, 0, 0, 1), 'no-limit 256 chips': (4, 2, -1, 256, 0, 0),
           'doudizhu 2 players': (3, 2, -1, 0, 0, 0), 'game id 9': (9, 0, -1, 0, 0, 0)}


def test_game_info_of_every_config_and_refusals():
    """Every cs_game_info field of every supported config equals the recorded table: the launch table entry that
    cs_game_info_get and cs_create share reports what the separate game_info chain did. Unsupported configs are
    refused with CS_E_UNSUPPORTED, the same text, and an all-zero cs_game_info."""
    fields = [f for f, _ in _abi.GameInfo._fields_]
    assert len(fields) == 11

    def row(info):
        return tuple(getattr(info, f) for f in fields)

    covered = [(g, 0, -1) for g in _abi.GAME_IDS] + [('leduc-holdem', n, -1) for n in range(3, 6)] + \
        [(g, n, -1) for g in ('limit-holdem', 'no-limit-holdem') for n in range(3, 23)] + \
        [('blackjack', n, d) for n in range(1, 8) for d in (-1, 0, 1, 2, 8)]
    assert sorted(GAME_INFO) == sorted(covered)
    for (game, players, decks), exp in GAME_INFO.items():
        assert row(_abi.game_info(game, players, decks)[0]) == exp, (game, players, decks)
    info, _ = _abi.game_info('no-limit-holdem', 6, chips_for_each=50, dealer_id=5)
    assert row(info) == NOLIMIT_6_CHIPS50_DEALER5
    for what, (game, players, decks, chips, dealer_plus1, mode) in REFUSED.items():
        cfg = _abi.Config(players, decks, chips, dealer_plus1, mode)
        info = _abi.GameInfo()
        assert _abi.lib().cs_game_info_get(game, C.byref(cfg), C.byref(info)) == -4, what
        assert _abi.lib().cs_last_error() == b'unsupported game or game config', what
        assert row(info) == (0,) * 11, what


@pytest.mark.gpu
@pytest.mark.parametrize('game', [1, 2, 4])   # Leduc, Limit, No-limit (the last two keep a deal queue)
def test_c_driver_parity_and_deal_queue_decode(game):
    """tools/abi_driver (C, no Python): a rollout through the ABI against the oracle, then every checked env's stream
    position from cs_get_rng_ctl minus its queued deals' draws, decoded from cs_get_env_state with nothing but the
    layout include/cardsim.h documents (game_words, deal_queue_depth, header bit fields), against the oracle."""
    import subprocess
    import sys
    drv = os.path.join(ROOT, 'tools', 'abi_driver')
    assert os.path.exists(drv), 'build() compiles tools/abi_driver'
    n, T = 4096, 64
    keys = subprocess.run([sys.executable, os.path.join(ROOT, 'tools', 'keys.py'), '42', str(n)], cwd=ROOT,
                          capture_output=True, check=True).stdout
    p = subprocess.run([drv, str(game), str(n), str(T), '1024'], input=keys, capture_output=True, cwd=ROOT,
                       timeout=120)
    out = p.stdout.decode()
    assert p.returncode == 0, out + p.stderr.decode()
    assert 'parity: 0 mismatching' in out and 'stream positions: 0 mismatching' in out, out
    if game in (2, 4):
        assert 'deal queue depth 8' in out
        assert ' 0 of 1024 envs hold queued deals' not in out   # the decode was exercised
