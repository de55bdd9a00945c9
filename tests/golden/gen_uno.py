"""Writes the UNO fixtures from the reference implementation (rlcard/games/uno, rlcard/envs/uno.py,
rlcard/models/uno_rule_models.py), imported through gen_golden.py's copy-and-stub setup. Runs only where the
reference is installed; the tests read what it wrote.

  uno.npz       event streams in the layout tests/golden_replay.py replays (obs rows flattened to 240 bytes, legal masks
                as 8 packed bytes, final observations of both players), several consecutive games per seed, actions
                from this script's own seeded RNG. Some events carry an illegal id in ev_act: there the reference was
                fed the lowest legal id, which is what the engine's ABI plays for an illegal id, so the recorded outcome
                is the reference's for that action. The seeds are found by a search over the reference so that the
                stream holds the rare paths (cov_* arrays: replace_deck through `draw` and through draw_2, top-card
                wild_draw_4 reshuffles, every kind of top card, a recoloured wild as target and in a hand, duplicate
                cards, a game of more than 150 steps). action_names is the reference's id -> name list.
  raw_uno.npz   the canonical-JSON stream tests/rawcanon.py defines, every call through rlcard.make('uno').
  uno_rule.npz  UNORuleAgentV1.step on recorded raw states: the action of the two deterministic branches, the set of
                actions the random branch may take.

The generator asserts that the reference never reached the two cases this engine's ABI defines for itself (an illegal
id, an empty deck after replace_deck): both would raise or draw from the global np.random in the reference."""
import json
import os
import random
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import gen_golden as gg   # noqa: E402

OUT = gg.OUT
GAMES_PER_SEED = 3
ILLEGAL_P = 0.06
NEED = {'rep_draw': 3, 'rep_draw2': 1, 'top_wd4_reshuffle': 2, 'top_skip': 1, 'top_reverse': 1, 'top_draw_2': 1,
        'top_wild': 1, 'wild_target_recoloured': 1, 'two_copies': 1, 'long_game': 1, 'wild_in_hand_recoloured': 1,
        'illegal_id': 20}
NEED_RAW = {k: 1 for k in NEED if k not in ('long_game', 'illegal_id', 'rep_draw2', 'top_wd4_reshuffle')}

COV = {}
CTX = []


def bump(k, n=1):
    COV[k] = COV.get(k, 0) + n


def instrument():
    """Counters on the reference's rare paths (wrappers only: behaviour unchanged)."""
    from rlcard.games.uno.round import UnoRound
    from rlcard.games.uno.dealer import UnoDealer
    rep, draw, non = UnoRound.replace_deck, UnoRound._perform_draw_action, UnoRound._preform_non_number_action
    flip, shuf = UnoDealer.flip_top_card, UnoDealer.shuffle

    def replace_deck(self):
        bump({'draw': 'rep_draw', 'draw_2': 'rep_draw2', 'wild_draw_4': 'rep_wd4'}[CTX[-1]])
        rep(self)
        assert self.dealer.deck, 'replace_deck left an empty deck: the ABI-defined case was reached'

    def perform_draw(self, players):
        CTX.append('draw')
        try:
            draw(self, players)
        finally:
            CTX.pop()

    def non_number(self, players, card):
        CTX.append(card.trait)
        try:
            non(self, players, card)
        finally:
            CTX.pop()

    def flip_top_card(self):
        CTX.append('flip')
        try:
            top = flip(self)
        finally:
            CTX.pop()
        bump('top_' + top.trait if not top.trait.isdigit() else 'top_number')
        return top

    def shuffle(self):
        if CTX and CTX[-1] == 'flip':
            bump('top_wd4_reshuffle')
        shuf(self)

    UnoRound.replace_deck, UnoRound._perform_draw_action = replace_deck, perform_draw
    UnoRound._preform_non_number_action = non_number
    UnoDealer.flip_top_card, UnoDealer.shuffle = flip_top_card, shuffle


def observe_cov(env):
    g = env.game
    t = g.round.target
    if t.type == 'wild' and t.color != t.str[0]:
        bump('wild_target_recoloured')
    for p in g.players:
        if any(c.type == 'wild' and c.color != c.str[0] for c in p.hand):
            bump('wild_in_hand_recoloured')
        strs = [c.str for c in p.hand if c.type != 'wild']
        if len(strs) != len(set(strs)):
            bump('two_copies')


def play(seed, games, illegal_p, on_reset=None, on_step=None, on_final=None):
    """`games` consecutive games of rlcard.make('uno') under `seed`; actions from a RNG seeded by the seed alone, so the
    search and the recording play the same games. -> coverage counters of this run."""
    import rlcard
    COV.clear()
    env = rlcard.make('uno', config={'seed': int(seed)})
    rng = random.Random(7919 * int(seed) + 13)
    for g in range(games):
        state, player = env.reset()
        observe_cov(env)
        if on_reset:
            on_reset(env, g, state, player)
        n = 0
        while not env.is_over():
            ids = sorted(state['legal_actions'].keys())
            a = fed = rng.choice(ids)
            if illegal_p > 0 and rng.random() < illegal_p:
                bad = [i for i in range(61) if i not in ids]
                a, fed = rng.choice(bad), ids[0]   # the engine gets `a`, the reference the lowest legal id
                bump('illegal_id')
            assert fed in ids   # the reference never decodes an illegal id (it would draw from the global np.random)
            state, player = env.step(fed)
            n += 1
            observe_cov(env)
            if on_step:
                on_step(env, g, a, fed, state, player)
        if n > 150:
            bump('long_game')
        bump('max_steps', max(0, n - COV.get('max_steps', 0)))
        if on_final:
            on_final(env, g)
    return dict(COV)


def search(need, illegal_p, limit=6000):
    """Seeds, in ascending order, each taken if it adds to a count still below its minimum."""
    have = {k: 0 for k in need}
    seeds = []
    for seed in range(limit):
        c = play(seed, GAMES_PER_SEED, illegal_p)
        if any(have[k] < need[k] and c.get(k, 0) > 0 for k in need):
            seeds.append(seed)
            for k in need:
                have[k] += c.get(k, 0)
        if all(have[k] >= need[k] for k in need):
            return seeds
    sys.exit('seed search exhausted: %s' % have)


def find_wd4_replace(limit_games=20000):
    for seed in range(100000, 100000 + limit_games // GAMES_PER_SEED):
        if play(seed, GAMES_PER_SEED, ILLEGAL_P).get('rep_wd4', 0):
            return seed
    return None


def flat(state):
    return dict(state, obs=np.asarray(state['obs']).reshape(-1))


def gen_events():
    from rlcard.games.uno.utils import ACTION_LIST
    seeds = search(NEED, ILLEGAL_P)
    wd4 = find_wd4_replace()
    if wd4 is not None:
        seeds.append(wd4)
    st = gg.Stream(240, 61, 2)
    total = {}
    counter = [0]
    for ei, seed in enumerate(seeds):
        base = counter[0]

        def on_reset(env, g, state, player):
            st.add(ei, base + g, 0, -1, flat(state), player, env.is_over(), None)

        def on_step(env, g, a, fed, state, player):
            done = env.is_over()
            st.add(ei, base + g, 1, a, flat(state), player, done, env.get_payoffs() if done else None)

        def on_final(env, g):
            st.add_final(base + g, [flat(env.get_state(p)) for p in range(2)])

        c = play(seed, GAMES_PER_SEED, ILLEGAL_P, on_reset, on_step, on_final)
        counter[0] += GAMES_PER_SEED
        for k, v in c.items():
            total[k] = max(total.get(k, 0), v) if k == 'max_steps' else total.get(k, 0) + v
    for k, v in NEED.items():
        assert total.get(k, 0) >= v, (k, total)
    assert all(int(np.sum(o)) == 61 for o in st.obs)
    cov = {'cov_' + k: np.array(total.get(k, 0), dtype=np.int64) for k in list(NEED) + ['rep_wd4', 'max_steps']}
    cov['cov_wd4_replace'] = cov.pop('cov_rep_wd4')
    st.save(os.path.join(OUT, 'uno.npz'), seeds, action_names=np.array(ACTION_LIST), **cov)
    print('uno.npz: %d seeds, %d events, coverage %s' % (len(seeds), len(st.obs), total))


def gen_raw():
    seeds = search(NEED_RAW, 0.0)
    rec = gg.RawStream()
    meta = []
    for si, seed in enumerate(seeds):
        def on_reset(env, g, state, player):
            rec.add(si, 0, -1, state, player, env)

        def on_step(env, g, a, fed, state, player):
            rec.add(si, 1, a, state, player, env, env.get_payoffs() if env.is_over() else None)

        def on_final(env, g):
            for p in range(2):
                rec.add(si, 3, p, env.get_state(p), p, env)

        play(seed, 2, 0.0, on_reset, on_step, on_final)
        meta.append({'env_id': 'uno', 'config': {}, 'seed': seed, 'games': 2, 'step_back': False})
    rec.save(os.path.join(OUT, 'raw_uno.npz'), meta)
    print('raw_uno.npz: %d streams, %d events' % (len(seeds), len(rec.state)))


def gen_rule():
    """States met by two UNORuleAgentV1 seats (so wild_draw_4 decisions occur), by branch: 0 draw, 1 wild_draw_4,
    2 random. Stored: the raw state as JSON, the action taken (branches 0, 1), the actions the rule may take."""
    import rlcard
    from rlcard.models.uno_rule_models import UNORuleAgentV1
    agent = UNORuleAgentV1()
    rows = {0: [], 1: [], 2: []}
    ties = all_wild = 0
    seed = 0
    while seed < 3000 and (min(len(r) for r in rows.values()) < 50 or ties < 5 or (all_wild == 0 and seed < 1500)):
        env = rlcard.make('uno', config={'seed': seed})
        np.random.seed(seed)
        state, player = env.reset()
        while not env.is_over():
            legal, hand = state['raw_legal_actions'], state['raw_obs']['hand']
            action = agent.step(state)
            view = json.dumps({'raw_obs': {'hand': hand}, 'raw_legal_actions': legal})
            if 'draw' in legal:
                b, allowed = 0, ['draw']
            elif any(a.split('-')[1] == 'wild_draw_4' for a in legal):
                b, allowed = 1, [action]
                nums = agent.count_colors(agent.filter_wild(hand))
                tie = sorted(nums.values())[-2:].count(max(nums.values())) == 2
                aw = all(c[2:6] == 'wild' for c in hand)
                ties += tie
                all_wild += aw
                if tie or aw:   # the rare ones always go in, ahead of the cap
                    rows[1].insert(0, (view, b, action, json.dumps(allowed)))
                    b = None
            else:
                b, allowed = 2, sorted(set(agent.filter_wild(legal)))
            assert action in allowed
            if b is not None and len(rows[b]) < 120:
                rows[b].append((view, b, action, json.dumps(allowed)))
            state, player = env.step(action, True)
        seed += 1
    allr = [r for b in (0, 1, 2) for r in rows[b][:160]]
    assert all(len(rows[b]) >= 50 for b in rows)
    np.savez_compressed(os.path.join(OUT, 'uno_rule.npz'), state=np.array([r[0] for r in allr]),
                        branch=np.array([r[1] for r in allr], dtype=np.int32), action=np.array([r[2] for r in allr]),
                        allowed=np.array([r[3] for r in allr]), cov_ties=np.array(ties, dtype=np.int64),
                        cov_all_wild=np.array(all_wild, dtype=np.int64))
    print('uno_rule.npz: %s states per branch, %d colour ties, %d all-wild hands' % (
        {b: len(rows[b]) for b in rows}, ties, all_wild))


def main():
    gg.setup_reference()
    instrument()
    which = sys.argv[1:] or ['events', 'raw', 'rule']
    if 'events' in which:
        gen_events()
    if 'raw' in which:
        gen_raw()
    if 'rule' in which:
        gen_rule()


if __name__ == '__main__':
    main()
