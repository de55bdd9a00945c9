"""cs_seed on every RNG layout: the byte ring (Leduc), DouDizhu's two word blocks, the Blackjack shoe's word column.

What no other test covers: cs_seed with first_env > 0, keys of length 1, and DouDizhu's seeding with kernel flag bit 0
(both blocks twisted in-lane). Handles hold N = 130 envs -- two full waves plus two lanes -- and are seeded through
cs_seed directly with synthetic keys, key_len = 1 + (i & 1). The expected MT19937 words come from the oracle's
or_mt_fill (tests/test_oracle.py pins the oracle's generator to numpy's known answers); the tempering is restated here,
since the engine stores untempered state words.

Layouts (rlcard_amd/csrc): ring = wbuf[624] u32 + 16 slots of 624 tempered low bytes, env e seeded with kb = 1 + e % 15
blocks, ctl = (kb - 1) << 19 (cs_ring.h); DouDizhu = two 624-word blocks, ctl 0 (cs_doudizhu.hip); shoe = the 624 words
of init_by_array awaiting their first twist (cs_blackjack_shoe.hip)."""
import ctypes as C
import functools

import numpy as np
import pytest

from rlcard_amd import _abi

torch = pytest.importorskip('torch')

N = 130
SPLIT = 65
SAMPLE = (0, 1, 14, 15, 63, 64, 65, 129)
MT_N = 624
RING_GEN = 15

GAMES = {'leduc': ('leduc-holdem', {}), 'doudizhu': ('doudizhu', {}), 'shoe': ('blackjack', {'game_num_decks': 2})}
# the finished game DouDizhu's seeding leaves (cs_doudizhu.h state words): all zero but the five trace words 12..16
# (no action yet), greater_player NONE = 3 in word 18 and current player 0 | winner 0 << 8 in word 19
DDZ_SEEDED = [0] * 12 + [0xFFFFFFFF] * 5 + [0, 3, 0] + [0] * 16


def _keys(salt):
    """[N][2] u32 keys, key_len 1 + (i & 1); the second word of a length-1 key is junk the engine must ignore"""
    i = np.arange(N, dtype=np.uint64)
    k0 = (i * np.uint64(2654435761) + np.uint64(salt)) & np.uint64(0xFFFFFFFF)
    k1 = (i * np.uint64(40503) + np.uint64(salt * 7 + 1)) & np.uint64(0xFFFFFFFF)
    keys = np.ascontiguousarray(np.stack([k0, k1], axis=1).astype(np.uint32))
    lens = np.ascontiguousarray((1 + (np.arange(N) & 1)).astype(np.int32))
    return keys, lens


def _temper(y):
    y = y.astype(np.uint32).copy()
    y ^= y >> np.uint32(11)
    y ^= (y << np.uint32(7)) & np.uint32(0x9D2C5680)
    y ^= (y << np.uint32(15)) & np.uint32(0xEFC60000)
    y ^= y >> np.uint32(18)
    return y


def _seed(v, keys, lens, first=0):
    with torch.cuda.device(v.device):
        _abi.check(_abi.lib().cs_seed(v._h, keys.ctypes.data_as(C.c_void_p), lens.ctypes.data_as(C.c_void_p), first,
                                      len(lens), v._stream()), 'cs_seed')


def _read(v):
    """{env: (ctl, state words, RNG words)} of the sampled envs"""
    L = _abi.lib()
    nw = C.c_int32()
    _abi.check(L.cs_env_rng_words(v._h, C.byref(nw)), 'cs_env_rng_words')
    buf = torch.zeros(nw.value, dtype=torch.int32, device=v.device)
    out = {}
    for e in SAMPLE:
        _abi.check(L.cs_copy_env_rng(v._h, e, C.c_void_p(buf.data_ptr()), v._stream()), 'cs_copy_env_rng')
        torch.cuda.synchronize()
        words = buf.cpu().numpy().view(np.uint32)[1:].copy()   # word 0 is the ctl word again
        ctl = C.c_uint32()
        _abi.check(L.cs_get_rng_ctl(v._h, e, C.byref(ctl)), 'cs_get_rng_ctl')
        out[e] = (ctl.value, v.env_state_words(e), words)
    return out


def _vec(game, mode):
    from rlcard_amd import VecEnv
    env_id, cfg = GAMES[game]
    return VecEnv(env_id, N, seed=5, device=0, config=dict(cfg, rng_mode=mode))


@functools.lru_cache(maxsize=None)
def _seeded(game, mode):
    """(A, B, B after a reseed with kernel flag bit 0): A takes the keys K in one call; B is seeded with other keys
    first, then with K[65:] at first_env 65, then with K[:65] at first_env 0"""
    assert torch.cuda.is_available(), 'needs the GPU'
    keys, lens = _keys(11)
    a = _vec(game, mode)
    _seed(a, keys, lens)
    ra = _read(a)
    a.close()
    b = _vec(game, mode)
    _seed(b, *_keys(12))
    _seed(b, keys[SPLIT:], lens[SPLIT:], SPLIT)
    _seed(b, keys[:SPLIT], lens[:SPLIT], 0)
    rb = _read(b)
    rf = None
    if game == 'doudizhu' and mode == 'mt19937':
        _seed(b, *_keys(12))
        b.set_kernel_flags(1)
        _seed(b, keys, lens)
        rf = _read(b)
    b.close()
    return ra, rb, rf


@functools.lru_cache(maxsize=None)
def _outputs(env, n):
    """the first n tempered MT19937 outputs of env `env`'s key (the oracle's generator)"""
    import oracle_lib
    keys, lens = _keys(11)
    out = np.zeros(n, np.uint32)
    oracle_lib.lib().or_mt_fill(oracle_lib.P(np.ascontiguousarray(keys[env])), int(lens[env]), oracle_lib.P(out), n)
    return out


def _ring_defined(e, words, mode):
    """the words of a ring env that seeding defines: wbuf (Philox: counter and key, words 0..2) and slots < kb"""
    kb = 1 + e % RING_GEN
    head = words[:MT_N] if mode == 'mt19937' else words[:3]
    return np.concatenate([head, words[MT_N:MT_N + kb * MT_N // 4]])


@pytest.mark.gpu
def test_leduc_ring_seeding_matches_mt19937(oracle):
    ra, _, _ = _seeded('leduc', 'mt19937')
    for e in SAMPLE:
        ctl, _, words = ra[e]
        kb = 1 + e % RING_GEN
        out = _outputs(e, MT_N * kb)
        assert ctl == (kb - 1) << 19, 'env %d ctl %#x' % (e, ctl)
        assert np.array_equal(_temper(words[:MT_N]), out[MT_N * (kb - 1):]), 'env %d: wbuf is not block %d' % (e, kb - 1)
        ring = words[MT_N:].view(np.uint8)
        assert np.array_equal(ring[:MT_N * kb], (out & 255).astype(np.uint8)), 'env %d: ring slots < %d' % (e, kb)


@pytest.mark.gpu
def test_doudizhu_seeding_matches_mt19937(oracle):
    ra, _, rf = _seeded('doudizhu', 'mt19937')
    for e in SAMPLE:
        ctl, st, words = ra[e]
        assert ctl == 0, 'env %d ctl %#x' % (e, ctl)
        assert len(words) == 2 * MT_N
        assert np.array_equal(_temper(words), _outputs(e, 2 * MT_N)), 'env %d: the two blocks' % e
        assert st == DDZ_SEEDED, 'env %d state words' % e
        # kernel flag bit 0 (the second block twisted in-lane): the same words
        fctl, fst, fwords = rf[e]
        assert fctl == 0 and fst == DDZ_SEEDED and np.array_equal(fwords, words), 'env %d with flag bit 0' % e


@pytest.mark.gpu
@pytest.mark.parametrize('game,mode', [('leduc', 'mt19937'), ('leduc', 'philox'), ('doudizhu', 'mt19937'),
                                       ('doudizhu', 'philox'), ('shoe', 'mt19937')])
def test_split_seeding_equals_one_call(game, mode):
    ra, rb, _ = _seeded(game, mode)
    for e in SAMPLE:
        (actl, ast, aw), (bctl, bst, bw) = ra[e], rb[e]
        assert actl == bctl, '%s %s env %d ctl %#x vs %#x' % (game, mode, e, actl, bctl)
        assert ast == bst, '%s %s env %d state words' % (game, mode, e)
        if game == 'leduc':
            aw, bw = _ring_defined(e, aw, mode), _ring_defined(e, bw, mode)
        elif game == 'doudizhu' and mode == 'philox':
            aw, bw = aw[:3], bw[:3]           # the key and the draw count
        else:
            assert len(aw) == (2 * MT_N if game == 'doudizhu' else MT_N)   # every word is defined
        assert np.array_equal(aw, bw), '%s %s env %d RNG words' % (game, mode, e)
