"""Writes the Bridge fixtures from the reference implementation (rlcard/games/bridge, rlcard/envs/bridge.py), imported
through gen_golden.py's copy-and-stub setup. Runs only where the reference is installed; the tests read what it wrote.

  bridge.npz      event streams in the layout tests/golden_replay.py replays (obs rows of 573 bytes, legal masks as 12
                  packed bytes, final observations of all four seats), three consecutive games per seed. Uniform random
                  play bids up fast (about ten calls, high contracts that go down), so the play is steered by the seed
                  (MODES): uniform; everybody passes; one low bid and three passes; low bids with doubles and redoubles
                  taken whenever legal; an auction kept alive past the 40-call cap of bidding_rep; once, the longest
                  auction there is (three passes, then 35 times bid P P X P P XX P P: 319 calls). Cards are always played
                  uniformly. Seeds 0..BASE-1 are always taken; a search over further seeds adds those that raise a cov_*
                  counter still below its minimum (NEED). Some events carry an illegal id in ev_act: there the reference
                  was fed the lowest legal id, which is what the engine's ABI plays for an illegal id.
                  rule_calls / rule_cards / rule_tricks / rule_pay: every call legality, card legality, trick winner and
                  payoff the reference computed in these games, as inputs and answer of rlcard_amd/csrc/cs_bridge_rules.h.
  raw_bridge.npz  the raw side of rlcard.make('bridge') as canonical JSON (tests/test_bridge.py raw_view and
                  perfect_view define the canon) with action_names, the text of the reference's 91 ActionEvents
                  (index 0, no_bid, has none: '').

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
BASE = 36
ILLEGAL_P = 0.02
MODES = ['uniform', 'pass_out', 'one_bid', 'low', 'long', 'low']
FULL_SEED = 4   # a 'long' seed: its first game runs the 319-call auction
NEED = {'pass_out': 3, 'four_calls': 3, 'doubled': 5, 'redoubled': 5, 'bid_over_double': 5, 'declarer_not_last_bidder': 5,
        'board1': 3, 'board2': 3, 'board3': 3, 'board4': 3, 'nt': 3, 'suit_C': 3, 'suit_D': 3, 'suit_H': 3, 'suit_S': 3,
        'ruff': 10, 'overruff': 3, 'discard_loses': 10, 'made': 5, 'down': 5, 'cap_dealer0': 1, 'cap_dealer1': 1,
        'cap_dealer2': 1, 'cap_dealer3': 1, 'full_auction': 1, 'illegal_id': 20}
NEED_RAW = {'pass_out': 1, 'doubled': 1, 'dummy_seat': 1}
PASS, DBL, RDBL, PLAY = 36, 37, 38, 39

COV = {}
RULES = {'calls': [], 'cards': [], 'tricks': [], 'pay': []}


def bump(k, n=1):
    COV[k] = COV.get(k, 0) + n


def pick(rng, env, ids, mode, g, target):
    """the action of a steering mode; `target`: the number of calls a 'long' auction is kept alive for"""
    rnd = env.game.round
    if ids[0] >= PLAY or mode == 'uniform':
        return rng.choice(ids)
    calls = len(rnd.move_sheet) - 1
    bids = [a for a in ids if a < PASS]
    if mode == 'pass_out':
        return PASS
    if mode == 'one_bid':
        return PASS if rnd.contract_bid_move or not bids or rng.random() < 0.3 else rng.choice(bids[:10])
    if mode == 'low':
        for a in (RDBL, DBL):
            if a in ids and rng.random() < 0.8:
                return a
        if bids and rng.random() < (0.5 if rnd.contract_bid_move else 0.8):
            return rng.choice(bids[:4])
        return PASS
    # 'long': never the pass that ends the auction before `target` calls
    if calls >= target:
        return PASS
    if target == 319 and calls < 3:
        return PASS
    trailing = 0
    for m in reversed(rnd.move_sheet[1:]):
        if m.action.action_id != PASS:
            break
        trailing += 1
    if trailing < 2:
        return PASS
    for a in (RDBL, DBL):   # (after two passes: bid P P X P P XX P P is the longest round of calls a bid allows)
        if a in ids:
            return a
    if not bids:
        return PASS
    return bids[0] if target == 319 else rng.choice(bids[:3])


def rule_facts(env, ids):
    """inputs and answer of the rules header at this decision (before the step)"""
    from rlcard.games.bridge.utils.move import MakeBidMove
    rnd = env.game.round
    cur = rnd.current_player_id
    cb = rnd.contract_bid_move
    if not rnd.is_bidding_over():
        cube = {1: 0, 2: 1, 4: 2}[rnd.doubling_cube]
        RULES['calls'].append([cb.action.action_id if cb else 0, cb.player.player_id if cb else 0, cube, cur,
                               sum(1 << a for a in ids)])
    elif not rnd.is_over():
        tm = rnd.get_trick_moves()
        led = tm[0].card.card_id if tm and len(tm) < 4 else -1
        hand = sum(1 << c.card_id for c in rnd.players[cur].hand)
        RULES['cards'].append([hand, led, sum(1 << (a - PLAY) for a in ids)])
    assert cb is None or isinstance(cb, MakeBidMove)


def after_step(env, fed, before_cube, before_won):
    rnd = env.game.round
    cb = rnd.contract_bid_move
    if fed < PASS and before_cube > 1:
        bump('bid_over_double')
    if fed < PLAY and rnd.is_bidding_over():
        calls = len(rnd.move_sheet) - 1
        dealer = rnd.dealer_id
        if calls > 40 - dealer:
            bump('cap_dealer%d' % dealer)
        if calls == 319:
            bump('full_auction')
        if cb is None:
            bump('pass_out')
        else:
            if calls == 4:
                bump('four_calls')
            if rnd.doubling_cube == 2:
                bump('doubled')
            if rnd.doubling_cube == 4:
                bump('redoubled')
            if rnd.get_declarer().player_id != cb.player.player_id:
                bump('declarer_not_last_bidder')
            bump('nt' if not cb.action.bid_suit else 'suit_' + cb.action.bid_suit)
    if fed >= PLAY and rnd.play_card_count % 4 == 0:
        tm = rnd.get_trick_moves()
        cards = [m.card.card_id for m in tm]
        trump = cb.action.bid_suit
        strain = 4 if not trump else 'CDHS'.index(trump)
        winner = [m.player.player_id for m in tm].index(rnd.current_player_id)
        assert sum(rnd.won_trick_counts) == sum(before_won) + 1
        RULES['tricks'].append(cards + [strain, winner])
        led = cards[0] // 13
        trumps = [i for i, c in enumerate(cards) if c // 13 == strain]
        if strain != 4 and led != strain and trumps:
            bump('ruff')
            if len(trumps) > 1 and winner != trumps[0]:
                bump('overruff')
        if any(c // 13 != led and c // 13 != strain for c in cards[1:]):
            bump('discard_loses')
    if env.is_over():
        pay = [int(x) for x in env.get_payoffs()]
        RULES['pay'].append([cb.action.action_id if cb else 0, cb.player.player_id if cb else 0] +
                            list(rnd.won_trick_counts) + pay)
        if cb:
            bump('made' if pay[cb.player.player_id] > 0 else 'down')


def play(seed, games, illegal_p, on_reset=None, on_step=None, on_final=None, keep_rules=False):
    """`games` consecutive games of rlcard.make('bridge') under `seed`; actions from a RNG seeded by the seed alone, so
    the search and the recording play the same games. -> coverage counters of this run."""
    import rlcard
    COV.clear()
    if not keep_rules:
        for v in RULES.values():
            del v[:]
    env = rlcard.make('bridge', config={'seed': int(seed)})
    rng = random.Random(7919 * int(seed) + 13)
    mode = MODES[int(seed) % len(MODES)]
    for g in range(games):
        state, player = env.reset()
        rnd = env.game.round
        bump('board%d' % rnd.board_id)
        target = 319 if (int(seed) == FULL_SEED and g == 0) else rng.randint(41, 60)
        if on_reset:
            on_reset(env, g, state, player)
        while not env.is_over():
            ids = list(state['legal_actions'].keys())
            assert ids == state['raw_legal_actions']
            rule_facts(env, ids)
            a = fed = pick(rng, env, ids, mode, g, target)
            # (no illegal id inside the 319-call auction: the lowest legal id there is a bid, which would shorten it)
            if illegal_p > 0 and rng.random() < illegal_p and not (target == 319 and ids[0] < PLAY):
                bad = [i for i in range(91) if i not in ids]
                a, fed = rng.choice(bad), min(ids)   # the engine gets `a`, the reference the lowest legal id
                bump('illegal_id')
            cube, won = env.game.round.doubling_cube, list(env.game.round.won_trick_counts)
            state, player = env.step(fed)
            after_step(env, fed, cube, won)
            rnd = env.game.round
            if not env.is_over() and rnd.is_bidding_over() and rnd.get_dummy().player_id == player:
                bump('dummy_seat')
            if on_step:
                on_step(env, g, a, fed, state, player)
        if on_final:
            on_final(env, g)
    return dict(COV)


def _cov_of(args):
    seed, games, illegal_p = args
    return seed, play(seed, games, illegal_p)


def search(need, illegal_p, games, base, limit=3000):
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


def gen_events():
    seeds = search(NEED, ILLEGAL_P, GAMES_PER_SEED, BASE)
    st = gg.Stream(573, 91, 4)
    total = {}
    counter = [0]
    rules = {k: [] for k in RULES}
    for ei, seed in enumerate(seeds):
        base = counter[0]

        def on_reset(env, g, state, player):
            st.add(ei, base + g, 0, -1, state, player, env.is_over(), None)

        def on_step(env, g, a, fed, state, player):
            done = env.is_over()
            st.add(ei, base + g, 1, a, state, player, done, env.get_payoffs() if done else None)

        def on_final(env, g):
            st.add_final(base + g, [env.get_state(p) for p in range(4)])

        c = play(seed, GAMES_PER_SEED, ILLEGAL_P, on_reset, on_step, on_final)
        counter[0] += GAMES_PER_SEED
        for k, v in c.items():
            total[k] = total.get(k, 0) + v
        for k in RULES:
            rules[k].extend(RULES[k])
    for k, v in NEED.items():
        assert total.get(k, 0) >= v, (k, total)
    cov = {'cov_' + k: np.array(total.get(k, 0), dtype=np.int64) for k in list(NEED) + ['dummy_seat']}
    uniq = {k: np.unique(np.array(v, dtype=np.int64), axis=0) for k, v in rules.items()}
    path = os.path.join(OUT, 'bridge.npz')
    st.save(path, seeds, python_version=np.array(sys.version), rule_calls=uniq['calls'], rule_cards=uniq['cards'],
            rule_tricks=uniq['tricks'], rule_pay=uniq['pay'], **cov)
    print('bridge.npz: %d seeds, %d games, %d events, %d bytes, coverage %s' % (
        len(seeds), counter[0], len(st.obs), os.path.getsize(path), total))
    print('rules: %s' % {k: len(v) for k, v in uniq.items()})


# ---- the raw side --------------------------------------------------------------------------------------------------
def gen_raw():
    import rawcanon
    sys.path.insert(0, os.path.dirname(os.path.dirname(OUT)))   # the repository root: test_bridge imports rlcard_amd
    import test_bridge
    seeds = search(NEED_RAW, 0.0, 2, 0)
    cols = {k: [] for k in ('stream', 'kind', 'act', 'player', 'done')}
    states, payoffs, perfect, meta = [], [], [], []
    total = {}

    def add(si, kind, act, state, player, env):
        for k, v in zip(cols, (si, kind, act, player, int(env.is_over()))):
            cols[k].append(int(v))
        states.append(rawcanon.dumps(test_bridge.raw_view(state)))
        payoffs.append(rawcanon.dumps(env.get_payoffs()))
        perfect.append(rawcanon.dumps(test_bridge.perfect_view(env.get_perfect_information())))

    for si, seed in enumerate(seeds):
        def on_reset(env, g, state, player):
            add(si, 0, -1, state, player, env)

        def on_step(env, g, a, fed, state, player):
            add(si, 1, a, state, player, env)

        def on_final(env, g):
            for p in range(4):
                add(si, 3, p, env.get_state(p), env.game.round.current_player_id, env)

        for k, v in play(seed, 2, 0.0, on_reset, on_step, on_final).items():
            total[k] = total.get(k, 0) + v
        meta.append({'env_id': 'bridge', 'config': {}, 'seed': seed, 'games': 2, 'step_back': False})
    d = {k: np.array(v, dtype=np.int32) for k, v in cols.items()}
    from rlcard.games.bridge.utils.action_event import ActionEvent
    d.update(state=np.array(states), payoffs=np.array(payoffs), perfect=np.array(perfect),
             action_names=np.array([''] + [str(ActionEvent.from_action_id(i)) for i in range(1, 91)]),
             streams=np.array([json.dumps(s, sort_keys=True) for s in meta]), python_version=np.array(sys.version))
    d.update({'cov_' + k: np.array(v, dtype=np.int64) for k, v in total.items()})
    for k, v in NEED_RAW.items():
        assert total.get(k, 0) >= v, (k, total)
    path = os.path.join(OUT, 'raw_bridge.npz')
    np.savez_compressed(path, **d)
    print('raw_bridge.npz: %d streams, %d events, %d bytes' % (len(seeds), len(states), os.path.getsize(path)))


def baseline(seconds=10.0):
    """env.run(is_training=False) with a RandomAgent per seat, one process: env-steps/s (Env.timestep)"""
    import rlcard
    from rlcard.agents import RandomAgent
    env = rlcard.make('bridge', config={'seed': 42})
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
        gen_events()
    if 'raw' in which:
        gen_raw()
    if 'baseline' in which:
        baseline()


if __name__ == '__main__':
    main()
