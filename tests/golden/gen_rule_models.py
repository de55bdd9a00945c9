#!/usr/bin/env python3
"""Generate tests/golden/rule_models.npz from the REFERENCE's rule models (rlcard/models/: leduc-holdem-rule-v1,
leduc-holdem-rule-v2, limit-holdem-rule-v1). Test infrastructure only, like gen_golden.py (whose reference set-up it
reuses): it runs where the reference is present, and nothing in the product imports it. Data only, plain arrays.

Two parts per game G in (leduc, limit); action ids are the envs' (0 call, 1 raise, 2 fold, 3 check), cards are the
engine's ids (Leduc: index into SJ HJ SQ HQ SK HK; Limit: card2index, suit * 13 + rank with S H D C x A 2 .. K):

(a) decisions -- SEEDS_A seeds x 8 consecutive games on one env per seed, every action picked uniformly among the legal
    ids by random.Random(1000003 * (i + 1) + seed) as gen_golden.drive seeds it. At every decision:
      G_dec_env, G_dec_game, G_dec_player, G_dec_action (the action taken), G_dec_hand [D, 2] (-1 padded),
      G_dec_public [D, 5] (-1 padded), G_dec_legal (bitmask of the legal ids), G_dec_would [D, R] (what rule r of
      G_rules would play on that state), G_a_seeds.
    G_a_counts [R, 4]: how often rule r answered each action id; G_a_fallbacks [R, 3]: how often its answer came from
    the raise->call, check->fold, call->raise fallback. The generator asserts that every action a rule can return and
    (over both games) each of the three fallbacks occurs.
(b) games -- for every pairing of G_pairs (rule of seat 0, rule of seat 1) and each of SEEDS_B seeds, an env seeded
    once whose run() is called 8 times with the reference's agents:
      G_game_pair, G_game_env (seed index), G_game_payoffs [M, 2], G_game_ptr [M + 1] into G_act_player / G_act_id
      (the action record of each game), G_b_seeds.
"""
import os
import random

import numpy as np

import gen_golden

OUT = os.path.dirname(os.path.abspath(__file__))
ACTIONS = ['call', 'raise', 'fold', 'check']
LEDUC_CARDS = ['SJ', 'HJ', 'SQ', 'HQ', 'SK', 'HK']
GAMES_PER_ENV = 8
FALLBACK_FROM = ['raise', 'check', 'call']   # -> call, fold, raise

SPECS = {
    'leduc': dict(env_id='leduc-holdem', rules=['leduc-holdem-rule-v1', 'leduc-holdem-rule-v2'],
                  pairs=[(0, 0), (1, 1), (0, 1), (1, 0)],
                  # what each rule can answer at all: v1 finds raise legal unless the round's two raises are spent, and
                  # then a bet is open and call is legal, so it never checks or folds; v2 never checks
                  reachable=[{'raise', 'call'}, {'raise', 'call', 'fold'}]),
    'limit': dict(env_id='limit-holdem', rules=['limit-holdem-rule-v1'], pairs=[(0, 0)],
                  reachable=[{'raise', 'call', 'fold', 'check'}]),
}


def card_id(game, s):
    if game == 'leduc':
        return LEDUC_CARDS.index(s)
    return 'SHDC'.index(s[0]) * 13 + 'A23456789TJQK'.index(s[1])


def wanted_action(agent, rule, state):
    """The action the reference rule aims at before its fallback: its answer on the same state with every action
    legal (Leduc v1 has no fallback of that kind: its answer is its aim)."""
    if rule == 'leduc-holdem-rule-v1':
        return None
    return agent.step(dict(state, raw_legal_actions=list(ACTIONS)))


def gen_decisions(game, spec, seeds, out):
    import rlcard
    import rlcard.models as models
    agents = [models.load(r).agents[0] for r in spec['rules']]
    R = len(agents)
    cols = {k: [] for k in ('env', 'game', 'player', 'action', 'legal')}
    hands, publics, would = [], [], []
    counts = np.zeros((R, 4), np.int64)
    fallbacks = np.zeros((R, 3), np.int64)
    for ei, seed in enumerate(seeds):
        env = rlcard.make(spec['env_id'], config={'seed': int(seed)})
        rng = random.Random(1000003 * (ei + 1) + int(seed))
        for g in range(GAMES_PER_ENV):
            state, player = env.reset()
            while not env.is_over():
                legal = sorted(state['legal_actions'].keys())
                raw = state['raw_obs']
                if game == 'leduc':
                    hand = [raw['hand']]
                    public = [raw['public_card']] if raw['public_card'] else []
                else:
                    hand, public = list(raw['hand']), list(raw['public_cards'])
                a = rng.choice(legal)
                w = []
                for r, agent in enumerate(agents):
                    name = agent.step(state)
                    assert agent.eval_step(state)[0] == name
                    w.append(ACTIONS.index(name))
                    counts[r, w[-1]] += 1
                    aim = wanted_action(agent, spec['rules'][r], state)
                    if aim is not None and aim != name:
                        fallbacks[r, FALLBACK_FROM.index(aim)] += 1
                cols['env'].append(ei)
                cols['game'].append(g)
                cols['player'].append(player)
                cols['action'].append(a)
                cols['legal'].append(sum(1 << i for i in legal))
                hands.append([card_id(game, c) for c in hand] + [-1] * (2 - len(hand)))
                publics.append([card_id(game, c) for c in public] + [-1] * (5 - len(public)))
                would.append(w)
                state, player = env.step(a)
    for r in range(R):
        seen = {ACTIONS[i] for i in range(4) if counts[r, i]}
        assert seen == spec['reachable'][r], (spec['rules'][r], seen)
    for k, v in cols.items():
        out['%s_dec_%s' % (game, k)] = np.array(v, np.int32)
    out[game + '_dec_hand'] = np.array(hands, np.int8)
    out[game + '_dec_public'] = np.array(publics, np.int8)
    out[game + '_dec_would'] = np.array(would, np.int8)
    out[game + '_a_seeds'] = np.array(seeds, np.int64)
    out[game + '_a_counts'] = counts
    out[game + '_a_fallbacks'] = fallbacks
    out[game + '_rules'] = np.array(spec['rules'])
    print('%s (a): %d decisions; answers per rule (call raise fold check) %s; fallbacks (raise->call check->fold '
          'call->raise) %s' % (game, len(would), counts.tolist(), fallbacks.tolist()))
    return fallbacks


def gen_games(game, spec, seeds, out):
    import rlcard
    import rlcard.models as models
    pair_col, env_col, pay, ptr, act_p, act_a = [], [], [], [0], [], []
    loaded = [models.load(r).agents for r in spec['rules']]
    for pi, (r0, r1) in enumerate(spec['pairs']):
        for ei, seed in enumerate(seeds):
            env = rlcard.make(spec['env_id'], config={'seed': int(seed)})
            env.set_agents([loaded[r0][0], loaded[r1][1]])
            for g in range(GAMES_PER_ENV):
                _, payoffs = env.run(is_training=False)
                pair_col.append(pi)
                env_col.append(ei)
                pay.append(np.asarray(payoffs, np.float64))
                for p, a in env.action_recorder:
                    act_p.append(int(p))
                    act_a.append(ACTIONS.index(a))
                ptr.append(len(act_a))
    out[game + '_game_pair'] = np.array(pair_col, np.int32)
    out[game + '_game_env'] = np.array(env_col, np.int32)
    out[game + '_game_payoffs'] = np.stack(pay)
    out[game + '_game_ptr'] = np.array(ptr, np.int64)
    out[game + '_act_player'] = np.array(act_p, np.int8)
    out[game + '_act_id'] = np.array(act_a, np.int8)
    out[game + '_pairs'] = np.array(spec['pairs'], np.int32)
    out[game + '_b_seeds'] = np.array(seeds, np.int64)
    print('%s (b): %d games, %d actions' % (game, len(pay), len(act_a)))


def main():
    gen_golden.setup_reference()
    out = {}
    seeds_a = list(range(100, 164))          # 64 seeds: enough for every reachable answer and fallback (asserted)
    seeds_b = list(range(7, 7 + 32))
    total = np.zeros(3, np.int64)
    for game, spec in SPECS.items():
        total += gen_decisions(game, spec, seeds_a, out).sum(axis=0)
        gen_games(game, spec, seeds_b, out)
    assert (total > 0).all(), 'a fallback never occurred: %s' % total.tolist()
    np.savez_compressed(os.path.join(OUT, 'rule_models.npz'), **out)
    print('rule_models.npz: fallbacks over both games %s' % total.tolist())


if __name__ == '__main__':
    main()
