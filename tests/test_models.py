"""CPU-side checks of the rule models (rlcard_amd.models) and of what the engine needs for them: the registry, every
agent against the reference's recorded decisions (tests/golden/rule_models.npz, written by gen_rule_models.py), the
three new C-ABI symbols from a C file that includes only include/cardsim.h, and the gfx950 resource numbers of the
rollout kernels read from the code object's metadata."""
import os
import re
import subprocess

import numpy as np
import pytest

import golden_replay
from rlcard_amd import _abi, models

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ACTIONS = ['call', 'raise', 'fold', 'check']
LEDUC_CARDS = ['SJ', 'HJ', 'SQ', 'HQ', 'SK', 'HK']
RULES = {'leduc': ['leduc-holdem-rule-v1', 'leduc-holdem-rule-v2'], 'limit': ['limit-holdem-rule-v1']}


@pytest.fixture(scope='module')
def fx():
    return golden_replay.load('rule_models')


def limit_card(c):
    return 'SHDC'[c // 13] + 'A23456789TJQK'[c % 13]


def raw_state(game, d, k):
    """The raw state a rule agent reads, rebuilt from decision k of the fixture: hand, public cards, legal names."""
    legal = [ACTIONS[i] for i in range(4) if (int(d[game + '_dec_legal'][k]) >> i) & 1]
    hand = [int(c) for c in d[game + '_dec_hand'][k] if c >= 0]
    pub = [int(c) for c in d[game + '_dec_public'][k] if c >= 0]
    if game == 'leduc':
        raw = {'hand': LEDUC_CARDS[hand[0]], 'public_card': LEDUC_CARDS[pub[0]] if pub else None}
    else:
        raw = {'hand': [limit_card(c) for c in hand], 'public_cards': [limit_card(c) for c in pub]}
    raw['legal_actions'] = legal
    return {'raw_obs': raw, 'raw_legal_actions': legal}


def test_registry_loads_the_three_rule_models():
    for name in ('leduc-holdem-rule-v1', 'leduc-holdem-rule-v2', 'limit-holdem-rule-v1'):
        m = models.load(name)
        assert isinstance(m, models.Model)
        assert len(m.agents) == 2
        for a in m.agents:
            assert a.use_raw is True and a.policy_id == models.POLICY_IDS[name]
    assert [models.policy_id_of(x) for x in ('random', 0, 2, models.load('leduc-holdem-rule-v2').agents[0])] == \
        [0, 0, 2, 2]
    with pytest.raises(ValueError):
        models.load('no-such-model')
    with pytest.raises(ValueError):
        models.register('leduc-holdem-rule-v1', 'rlcard_amd.models.leducholdem_rule_models:LeducHoldemRuleModelV1')


@pytest.mark.parametrize('game', ['leduc', 'limit'])
def test_agents_reproduce_the_reference_decisions(fx, game):
    """Every 'would play' record of fixture (a): step and eval_step of each rule agent on the rebuilt raw state."""
    assert list(fx[game + '_rules']) == RULES[game]
    would = fx[game + '_dec_would']
    n = len(would)
    assert n > 1000
    counts = np.zeros((len(RULES[game]), 4), np.int64)
    for r, name in enumerate(RULES[game]):
        agent = models.load(name).agents[0]
        for k in range(n):
            s = raw_state(game, fx, k)
            got = agent.step(s)
            assert got == ACTIONS[would[k, r]], (name, k, s, got)
            assert agent.eval_step(s) == (got, [])
            counts[r, would[k, r]] += 1
    assert np.array_equal(counts, fx[game + '_a_counts'])   # the coverage the generator states in the file


def test_fixture_covers_every_answer_and_fallback(fx):
    """What the generator asserted with the reference alone, read back from the counts it stored."""
    assert (fx['leduc_a_counts'][0, [0, 1]] > 0).all() and (fx['leduc_a_counts'][1, [0, 1, 2]] > 0).all()
    assert (fx['limit_a_counts'][0] > 0).all()
    assert ((fx['leduc_a_fallbacks'].sum(axis=0) + fx['limit_a_fallbacks'].sum(axis=0)) > 0).all()


C_SOURCE = r'''
#include "cardsim.h"
#include <stdio.h>
int main(void)
{
    /* the three entry points by their declared types, and the policy ids */
    int (*a)(cs_handle*, int32_t, uint64_t, uint64_t, uint64_t, const int32_t*, const cs_traj_out*, void*) =
        cs_rollout_policy;
    int (*b)(cs_handle*, int32_t, uint64_t, uint64_t, uint64_t, int32_t*, void*) = cs_policy_actions;
    int (*c)(cs_handle*, int32_t, const cs_traj_out*, int32_t, int32_t*, double*, int64_t*, void*) = cs_payoff_sums;
    int32_t seats[2] = {CS_POLICY_RULE_V1, CS_POLICY_RULE_V2};
    /* null handles are refused before any device is touched */
    int r = a(0, 1, 0, 0, 0, seats, 0, 0) | b(0, CS_POLICY_RANDOM, 0, 0, 0, 0, 0) | c(0, 1, 0, 0, 0, 0, 0, 0);
    printf("%d %d\n", r, cs_abi_version());
    return r == CS_E_INVALID ? 0 : 1;
}
'''


def test_c_file_with_only_the_header_links_the_new_symbols(tmp_path):
    src = tmp_path / 'policy_syms.c'
    src.write_text(C_SOURCE)
    exe = tmp_path / 'policy_syms'
    libdir = os.path.dirname(_abi.LIB_PATH)
    rocm_lib = '/opt/rocm/lib'
    subprocess.run(['gcc', '-std=c99', '-Wall', '-Werror', '-I', os.path.join(ROOT, 'include'), str(src), '-o', str(exe),
                    '-L', libdir, '-lcardsim', '-Wl,-rpath,' + libdir, '-Wl,-rpath,' + rocm_lib,
                    '-Wl,-rpath-link,' + rocm_lib], check=True, capture_output=True)
    p = subprocess.run([str(exe)], capture_output=True, timeout=60)
    assert p.returncode == 0 and p.stdout.split() == [b'-1', b'3'], (p.stdout, p.stderr)


# VGPRs, SGPRs, LDS bytes, scratch bytes of the random rollouts, from the code object of the commit before the policy
# kernels were added: the policy path must leave them as they were
PARENT_ROLLOUT = {
    'Leduc': (69, 106, 26688, 0),
    'Limit': (104, 106, 35392, 0),
    'Nolimit': (114, 106, 33088, 0),
}
MIN_WAVES = {'Leduc': 6, 'Limit': 4}   # G::MIN_WAVES, the launch bound the policy kernel shares with its game


def kernel_resources(co):
    """kernel name -> (vgprs, sgprs, lds bytes, scratch bytes) from the AMDGPU metadata note of a code object."""
    notes = subprocess.run(['/opt/rocm/llvm/bin/llvm-readelf', '--notes', co], check=True, capture_output=True,
                           text=True).stdout
    out = {}
    for block in notes.split('- .agpr_count')[1:]:
        def field(name):
            return int(re.search(r'\.%s:\s+(\d+)' % name, block).group(1))
        name = re.search(r'\.name:\s+(_Z\w+)', block)   # (kernel arguments may carry plain names of their own)
        if name is None:
            continue
        out[name.group(1)] = (field('vgpr_count'), field('sgpr_count'), field('group_segment_fixed_size'),
                     field('private_segment_fixed_size'), field('vgpr_spill_count'), field('sgpr_spill_count'))
    return out


@pytest.mark.slow
def test_gfx950_rollout_kernels_resources(tmp_path):
    """Cross-compiles the unit that instantiates the heads-up games for gfx950 and reads each rollout kernel's numbers
    from the code object's metadata: the policy instantiations use no scratch and fit the wave count of their game's
    launch bound (512 VGPRs per SIMD lane, allocated in blocks of 8), and k_rollout<Leduc / Limit / Nolimit> have
    the registers, LDS and scratch of the parent commit."""
    co = str(tmp_path / 'cs_kernels.co')
    csrc = os.path.join(ROOT, 'rlcard_amd', 'csrc')
    subprocess.run(['/opt/rocm/bin/hipcc', '-O3', '-std=c++17', '--offload-arch=gfx950', '--cuda-device-only',
                    '--no-gpu-bundle-output', '-DCS_DDZ_TABLE_FILE="unused"', '-c', '-o', co,
                    os.path.join(csrc, 'cs_kernels.hip')], check=True, capture_output=True)
    res = kernel_resources(co)

    def find(game, policy):   # k_rollout<game, policy> (Itanium mangling: Lb0 / Lb1 for the bool)
        hits = [v for k, v in res.items() if re.fullmatch(r'_ZN2cs9k_rolloutINS_\d+%sELb%dEEEvNS_11RolloutArgsE'
                                                          % (game, policy), k)]
        assert len(hits) == 1, (game, policy, sorted(res))
        return hits[0]

    for game, parent in PARENT_ROLLOUT.items():
        print(game, 'k_rollout', find(game, 0))
        assert find(game, 0)[:4] == parent, game
    for game, waves in MIN_WAVES.items():
        vgprs, sgprs, lds, scratch, vspill, sspill = find(game, 1)
        print(game, 'k_rollout (policy)', vgprs, sgprs, lds, scratch)
        assert scratch == 0 and vspill == 0, game
        assert (vgprs + 7) // 8 * 8 * waves <= 512, game
