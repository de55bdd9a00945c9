"""Writes the Gin Rummy fixtures from the reference implementation (rlcard/games/gin_rummy, rlcard/envs/gin_rummy.py,
rlcard/models/gin_rummy_rule_models.py), imported through gen_golden.py's copy-and-stub setup. Runs only where the
reference is installed; the tests read what it wrote.

  gin_rummy.npz        event streams in the layout tests/golden_replay.py replays (obs rows flattened to 260 bytes, legal
                       masks as 14 packed bytes, final observations of both seats), three consecutive games per seed.
                       Uniform random play seldom knocks and almost never gins, so the play is steered by the seed
                       (MODES): uniform; gin and knock whenever legal, else the novice rule's discard; never knock, so
                       that the hand plays on to a gin; always draw (the stock runs dead); always pick up (200 moves).
                       Seeds 0..BASE-1 are always taken; a search over further seeds adds those that raise a cov_*
                       counter still below its minimum (NEED). Some events carry an illegal id in ev_act: there the
                       reference was fed the lowest legal id, which is what the engine's ABI plays for an illegal id.
                       Per event ev_cand_ids / ev_cand_ptr: the ids the novice rule would choose from. cov_max_uniform
                       is the longest uniform-random game in steps; python_version is sys.version (the order of a
                       Python set is CPython's).
  gin_rummy_melds.npz  the judge alone on ordered hands of 10 and 11 cards, half from the streams, half built meld-rich
                       (overlapping runs and sets, four of a kind, runs of 6..11): the best deadwood count, and for 11
                       cards judge.get_going_out_cards' knock and gin sets as card masks and gin_cards[0].
  raw_gin_rummy.npz    the raw side of rlcard.make('gin-rummy') as canonical JSON (tests/test_gin_rummy.py raw_view
                       defines the canon), with the novice rule's candidate ids per decision and action_names, the
                       text of the reference's 110 ActionEvents.

`baseline` prints the reference's env.run rate with random agents on one core (profiles/ref_cpu_baseline.json)."""
import json
import os
import random
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import gen_golden as gg   # noqa: E402

OUT = gg.OUT
GAMES_PER_SEED = 3
BASE = 102
ILLEGAL_P = 0.02
MODES = ['uniform', 'go_out', 'gin_hunt', 'always_draw', 'always_pick', 'uniform']
NEED = {'gin_one_deadwood': 3, 'gin_no_deadwood': 1, 'gin_many_cards': 2, 'knock': 20, 'dead_stock': 5, 'dead_moves': 5,
        'pick_up_barred': 50, 'four_of_a_kind': 3, 'run_of_five': 5, 'dealer0': 20, 'dealer1': 20, 'illegal_id': 20}
NEED_RAW = {'gin_one_deadwood': 1, 'knock': 2, 'dead_stock': 1, 'pick_up_barred': 5, 'knock_many_cards': 2}

COV = {}


def bump(k, n=1):
    COV[k] = COV.get(k, 0) + n


def cid(card):
    from rlcard.games.gin_rummy.utils import utils
    return utils.get_card_id(card)


def novice_candidates(state):
    """the list GinRummyNoviceRuleAgent.step hands to np.random.choice: the agent itself is run with that call caught"""
    from rlcard.models.gin_rummy_rule_models import GinRummyNoviceRuleAgent as Agent
    seen = []

    def catch(actions, *args, **kwargs):
        seen.append([int(a) for a in actions])
        return actions[0]

    real = np.random.choice
    np.random.choice = catch
    try:
        Agent.step(state)
    finally:
        np.random.choice = real
    return seen[0]


def pick(rng, env, state, mode):
    ids = list(state['legal_actions'].keys())
    if mode == 'uniform' or len(ids) == 1:
        return rng.choice(ids)
    if ids[0] in (2, 4) and 3 in ids:   # draw (or dead hand) / pick up
        if mode == 'always_draw':
            return ids[0]
        if mode == 'always_pick':
            return 3
        return rng.choice(ids) if rng.random() < 0.7 else 3
    knocks = [a for a in ids if a >= 58]
    discards = [a for a in ids if 6 <= a < 58]
    if mode == 'go_out' and knocks:
        return rng.choice(knocks)
    if mode in ('go_out', 'gin_hunt'):
        cand = [a for a in novice_candidates(dict(state, legal_actions={a: None for a in discards})) if a < 58]
        return rng.choice(cand)
    return rng.choice(discards)


def play(seed, games, illegal_p, on_reset=None, on_step=None, on_final=None):
    """`games` consecutive games of rlcard.make('gin-rummy') under `seed`; actions from a RNG seeded by the seed alone,
    so the search and the recording play the same games. -> coverage counters of this run."""
    import rlcard
    from rlcard.games.gin_rummy import judge
    from rlcard.games.gin_rummy.utils import melding
    COV.clear()
    env = rlcard.make('gin-rummy', config={'seed': int(seed)})
    rng = random.Random(7919 * int(seed) + 13)
    mode = MODES[int(seed) % len(MODES)]
    for g in range(games):
        state, player = env.reset()
        bump('dealer%d' % env.game.round.dealer_id)
        if on_reset:
            on_reset(env, g, state, player)
        n = 0
        while not env.is_over():
            ids = list(state['legal_actions'].keys())
            a = fed = pick(rng, env, state, mode)
            if illegal_p > 0 and rng.random() < illegal_p:
                bad = [i for i in range(110) if i not in ids]
                a, fed = rng.choice(bad), min(ids)   # the engine gets `a`, the reference the lowest legal id
                bump('illegal_id')
            hand = list(env.game.round.players[env.game.round.current_player_id].hand)
            if len(hand) == 11:
                for m in melding.get_all_set_melds(hand):
                    if len(m) == 4:
                        bump('four_of_a_kind')
                        break
                for m in melding.get_all_run_melds(hand):
                    if len(m) >= 5:
                        bump('run_of_five')
                        break
            if fed == 5:
                _, gin_cards = judge.get_going_out_cards(hand, 10)
                none_left = False
                for cl in melding.get_meld_clusters(hand):
                    if sum(len(m) for m in cl) == 11:
                        none_left = True
                bump('gin_no_deadwood' if none_left else 'gin_one_deadwood')
                if len(gin_cards) > 1:
                    bump('gin_many_cards')
            elif fed >= 58:
                bump('knock')
                if sum(1 for i in ids if i >= 58) > 1:
                    bump('knock_many_cards')
            elif fed == 4:
                bump('dead_moves' if len(env.game.round.move_sheet) >= 200 else 'dead_stock')
            state, player = env.step(fed)
            if fed == 3 and len(state['legal_actions']) > 1:
                picked = cid(env.game.round.move_sheet[-1].card)
                assert 6 + picked not in state['legal_actions']
                bump('pick_up_barred')
            n += 1
            if on_step:
                on_step(env, g, a, fed, state, player)
        if mode == 'uniform':
            bump('max_uniform', max(0, n - COV.get('max_uniform', 0)))
        if on_final:
            on_final(env, g)
    return dict(COV)


def _cov_of(args):
    seed, games, illegal_p = args
    return seed, play(seed, games, illegal_p)


def search(need, illegal_p, games, base, limit=6000):
    """Seeds 0..base-1, then further seeds in ascending order, each taken if it adds to a count still below its minimum."""
    from multiprocessing import Pool
    have = {k: 0 for k in need}
    seeds = []
    with Pool(min(8, os.cpu_count() or 1)) as pool:
        for seed, c in pool.imap(_cov_of, ((s, games, illegal_p) for s in range(limit)), chunksize=4):
            if seed < base or any(have[k] < need[k] and c.get(k, 0) > 0 for k in need if k != 'illegal_id'):
                seeds.append(seed)
                for k in need:
                    have[k] += c.get(k, 0)
            if seed >= base - 1 and all(have[k] >= need[k] for k in need):
                pool.terminate()
                return seeds
    sys.exit('seed search exhausted: %s' % have)


def flat(state):
    return dict(state, obs=np.asarray(state['obs']).reshape(-1))


def gen_events():
    seeds = search(NEED, ILLEGAL_P, GAMES_PER_SEED, BASE)
    st = gg.Stream(260, 110, 2)
    total = {}
    counter = [0]
    cand_ids, cand_ptr = [], [0]
    hands = []   # the current player's ordered hand at every decision, for gin_rummy_melds.npz

    def note(env, state):
        c = sorted(novice_candidates(state)) if not env.is_over() else []
        cand_ids.extend(c)
        cand_ptr.append(len(cand_ids))
        if not env.is_over():
            h = [cid(x) for x in env.game.round.players[env.game.round.current_player_id].hand]
            if len(h) in (10, 11):
                hands.append(h)

    for ei, seed in enumerate(seeds):
        base = counter[0]

        def on_reset(env, g, state, player):
            st.add(ei, base + g, 0, -1, flat(state), player, env.is_over(), None)
            note(env, state)

        def on_step(env, g, a, fed, state, player):
            done = env.is_over()
            st.add(ei, base + g, 1, a, flat(state), player, done, env.get_payoffs() if done else None)
            note(env, state)

        def on_final(env, g):
            st.add_final(base + g, [flat(env.get_state(p)) for p in range(2)])

        c = play(seed, GAMES_PER_SEED, ILLEGAL_P, on_reset, on_step, on_final)
        counter[0] += GAMES_PER_SEED
        for k, v in c.items():
            total[k] = max(total.get(k, 0), v) if k == 'max_uniform' else total.get(k, 0) + v
    for k, v in NEED.items():
        assert total.get(k, 0) >= v, (k, total)
    assert counter[0] >= 300
    cov = {'cov_' + k: np.array(total.get(k, 0), dtype=np.int64) for k in list(NEED) + ['max_uniform', 'knock_many_cards']}
    path = os.path.join(OUT, 'gin_rummy.npz')
    st.save(path, seeds, ev_cand_ids=np.array(cand_ids, np.int16), ev_cand_ptr=np.array(cand_ptr, np.int64),
            python_version=np.array(sys.version), **cov)
    print('gin_rummy.npz: %d seeds, %d games, %d events, %d bytes, coverage %s' % (
        len(seeds), counter[0], len(st.obs), os.path.getsize(path), total))
    print('longest uniform-random game: %d steps' % total.get('max_uniform', 0))
    return hands


# ---- the judge ---------------------------------------------------------------------------------------------------
def judge_row(hand):
    """(best deadwood, knock mask, gin mask, gin card) of an ordered hand of card ids, by the reference's functions"""
    from rlcard.games.gin_rummy import judge
    from rlcard.games.gin_rummy.utils import melding, utils
    cards = [utils.get_card(c) for c in hand]
    total = sum(utils.get_deadwood_value(c) for c in cards)
    best = total
    for cl in melding.get_meld_clusters(hand=cards):
        melded = [c for m in cl for c in m]
        best = min(best, sum(utils.get_deadwood_value(c) for c in cards if c not in melded))
    if len(cards) == 10:
        bc = melding.get_best_meld_clusters(hand=cards)
        assert best == utils.get_deadwood_count(hand=cards, meld_cluster=bc[0] if bc else [])
        return best, 0, 0, -1
    knock, gin = judge.get_going_out_cards(cards, 10)
    km = sum(1 << cid(c) for c in knock)
    gm = sum(1 << cid(c) for c in gin)
    return best, km, gm, (cid(gin[0]) if gin else -1)


def built_hand(rng, n):
    """a meld-rich hand of n cards: runs of 3..11, sets of 3 and 4 that cross them, topped up at random"""
    cards = []

    def add(cs):
        for c in cs:
            if c not in cards and len(cards) < n:
                cards.append(c)

    kind = rng.randrange(6)
    if kind == 0:     # one long run, 6..11
        s, ln = rng.randrange(4), rng.randint(6, 11)
        a = rng.randint(0, 13 - ln)
        add([13 * s + a + k for k in range(ln)])
    elif kind == 1:   # four of a kind crossing runs
        r = rng.randint(1, 11)
        add([13 * s + r for s in range(4)])
        for s in rng.sample(range(4), 2):
            add([13 * s + r + d for d in (-1, 1)] + ([13 * s + r + 2] if r + 2 < 13 else []))
    elif kind == 2:   # three runs over the same ranks: runs and sets overlap
        a = rng.randint(0, 9)
        for s in rng.sample(range(4), 3):
            add([13 * s + a + k for k in range(rng.randint(3, 4))])
    elif kind == 3:   # two fours of a kind and a set of three
        rs = rng.sample(range(13), 3)
        add([13 * s + rs[0] for s in range(4)])
        add([13 * s + rs[1] for s in range(4)])
        add([13 * s + rs[2] for s in range(3)])
    elif kind == 4:   # two runs and a set
        for _ in range(2):
            s, ln = rng.randrange(4), rng.randint(3, 5)
            a = rng.randint(0, 13 - ln)
            add([13 * s + a + k for k in range(ln)])
        r = rng.randrange(13)
        add([13 * s + r for s in rng.sample(range(4), 3)])
    else:             # low cards: small deadwood, knocks with several candidates
        add(rng.sample([13 * s + r for s in range(4) for r in range(5)], min(n, 9)))
    rest = [c for c in range(52) if c not in cards]
    rng.shuffle(rest)
    add(rest)
    rng.shuffle(cards)
    return cards


def gen_melds(stream_hands):
    rng = random.Random(20261020)
    rows = []
    seen = set()
    rng.shuffle(stream_hands)
    for want in (10, 11):
        k = 0
        for h in stream_hands:
            if len(h) == want and tuple(h) not in seen and k < 1100:
                seen.add(tuple(h))
                rows.append(h)
                k += 1
        for _ in range(1100):
            rows.append(built_hand(rng, want))
    n = len(rows)
    hands = np.zeros((n, 11), np.uint8)
    ln = np.zeros(n, np.uint8)
    dw = np.zeros(n, np.int32)
    knock = np.zeros(n, np.uint64)
    gin = np.zeros(n, np.uint64)
    card = np.zeros(n, np.int32)
    for i, h in enumerate(rows):
        hands[i, :len(h)] = h
        ln[i] = len(h)
        dw[i], km, gm, card[i] = judge_row(h)
        knock[i], gin[i] = km, gm
    g11 = ln == 11
    stats = {'rows': n, 'len10': int((ln == 10).sum()), 'len11': int(g11.sum()), 'gin': int((gin != 0).sum()),
             'gin_many': int(sum(bin(int(x)).count('1') > 1 for x in gin)), 'knock': int((knock != 0).sum()),
             'dead0_11': int(((dw == 0) & g11).sum())}
    assert n >= 4000 and stats['gin'] >= 100 and stats['gin_many'] >= 20 and stats['dead0_11'] >= 10, stats
    path = os.path.join(OUT, 'gin_rummy_melds.npz')
    np.savez_compressed(path, hands=hands, len=ln, deadwood=dw, knock=knock, gin=gin, gin_card=card,
                        python_version=np.array(sys.version))
    print('gin_rummy_melds.npz: %s, %d bytes' % (stats, os.path.getsize(path)))


# ---- the raw side --------------------------------------------------------------------------------------------------
def gen_raw():
    import rawcanon
    sys.path.insert(0, os.path.dirname(os.path.dirname(OUT)))   # the repository root: test_gin_rummy imports rlcard_amd
    import test_gin_rummy
    seeds = search(NEED_RAW, 0.0, 2, 0)
    cols = {k: [] for k in ('stream', 'kind', 'act', 'player', 'done')}
    states, payoffs, cands, meta = [], [], [], []

    def add(si, kind, act, state, player, env, pay=None):
        for k, v in zip(cols, (si, kind, act, player, int(env.is_over()))):
            cols[k].append(int(v))
        states.append(rawcanon.dumps(test_gin_rummy.raw_view(state)))
        payoffs.append('' if pay is None else rawcanon.dumps(pay))
        cands.append(json.dumps(sorted(int(x) for x in novice_candidates(state)) if not env.is_over() else []))

    for si, seed in enumerate(seeds):
        def on_reset(env, g, state, player):
            add(si, 0, -1, state, player, env, env.get_payoffs())

        def on_step(env, g, a, fed, state, player):
            add(si, 1, a, state, player, env, env.get_payoffs())

        def on_final(env, g):
            for p in range(2):
                add(si, 3, p, env.get_state(p), p, env)

        play(seed, 2, 0.0, on_reset, on_step, on_final)
        meta.append({'env_id': 'gin-rummy', 'config': {}, 'seed': seed, 'games': 2, 'step_back': False})
    d = {k: np.array(v, dtype=np.int32) for k, v in cols.items()}
    from rlcard.games.gin_rummy.utils.action_event import ActionEvent
    d.update(state=np.array(states), payoffs=np.array(payoffs), candidates=np.array(cands),
             action_names=np.array([str(ActionEvent.decode_action(i)) for i in range(110)]),
             streams=np.array([json.dumps(s, sort_keys=True) for s in meta]), python_version=np.array(sys.version))
    path = os.path.join(OUT, 'raw_gin_rummy.npz')
    np.savez_compressed(path, **d)
    print('raw_gin_rummy.npz: %d streams, %d events, %d bytes' % (len(seeds), len(states), os.path.getsize(path)))


def baseline(seconds=10.0):
    """env.run(is_training=False) with a RandomAgent per seat, one process: env-steps/s (Env.timestep)"""
    import rlcard
    from rlcard.agents import RandomAgent
    env = rlcard.make('gin-rummy', config={'seed': 42})
    env.set_agents([RandomAgent(num_actions=env.num_actions) for _ in range(env.num_players)])
    np.random.seed(42)
    t0 = time.perf_counter()
    steps = games = 0
    while time.perf_counter() - t0 < seconds:
        before = env.timestep
        env.run(is_training=False)
        steps += env.timestep - before
        games += 1
    dt = time.perf_counter() - t0
    print(json.dumps({'value': steps / dt, 'unit': 'env-steps/s', 'processes': 1, 'env_steps': steps, 'games': games,
                      'seconds': dt}))


def main():
    gg.setup_reference()
    which = sys.argv[1:] or ['events', 'raw']
    if 'events' in which:
        gen_melds(gen_events())
    if 'raw' in which:
        gen_raw()
    if 'baseline' in which:
        baseline()


if __name__ == '__main__':
    main()
