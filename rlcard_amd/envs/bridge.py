"""Bridge env (rlcard/envs/bridge.py, games/bridge/) over the HIP engine (rlcard_amd/csrc/cs_bridge.h).

Every raw field is decoded from the env's packed state words: the shuffled deck (one card id per byte; seat p's hand, in
list order, is deck[51 - 13 p - i] for i = 0..12 without the cards it has played), the four hand masks, the first 40
calls, the first bidder per side and strain, and the two words of counters. obs and raw_obs are the same 573-value int64
array and always show the current player, whoever asks.

The order of the legal actions is the reference's (judger.get_legal_actions): pass, the bids above the last one in
ascending order, dbl or rdbl; during the play the cards in hand order (those of the led suit if the hand has any).

Four players, DefaultBridgePayoffDelegate and DefaultBridgeStateExtractor only. The reference's Bridge game has no
step_back; step_back here raises NotImplementedError. get_perfect_information returns the reference's keys (its
'contact' spelling included) as plain data: the tray as (board, dealer, vul), a move as (player, action id), cards as
card ids. get_payoffs is computed on the host from the state, as the reference computes it from its round."""
from collections import OrderedDict

import numpy as np

from .env import Env

SUITS = ['C', 'D', 'H', 'S']
RANKS = ['2', '3', '4', '5', '6', '7', '8', '9', 'T', 'J', 'Q', 'K', 'A']
NO_BID, FIRST_BID, LAST_BID, PASS, DBL, RDBL, PLAY = 0, 1, 35, 36, 37, 38, 39
NUM_ACTIONS = 91
CALLS_KEPT = 40


def card_text(c):
    return RANKS[c % 13] + SUITS[c // 13]


def bid_amount(a):
    return 1 + (a - FIRST_BID) // 5


def bid_strain(a):
    return (a - FIRST_BID) % 5


class ActionEvent(object):
    """games/bridge/utils/action_event.py: an action is its id; a bid carries amount and suit, a play its card id"""

    def __init__(self, action_id):
        self.action_id = int(action_id)
        if not FIRST_BID <= self.action_id < NUM_ACTIONS:
            raise Exception('ActionEvent from_action_id: invalid action_id=%d' % self.action_id)
        self.card_id = self.action_id - PLAY if self.action_id >= PLAY else None

    @staticmethod
    def from_action_id(action_id):
        return ActionEvent(action_id)

    def __eq__(self, other):
        return isinstance(other, ActionEvent) and self.action_id == other.action_id

    def __hash__(self):
        return hash(self.action_id)

    def __str__(self):
        a = self.action_id
        if a <= LAST_BID:
            return '%d%s' % (bid_amount(a), (SUITS + ['NT'])[bid_strain(a)])
        if a < PLAY:
            return ('pass', 'dbl', 'rdbl')[a - PASS]
        return card_text(self.card_id)

    __repr__ = __str__


# (id 0, no_bid, is no action: the reference's from_action_id raises there, and so does ActionEvent(0))
ACTION_LIST = [None] + [ActionEvent(i) for i in range(1, NUM_ACTIONS)]


def decode_words(w):
    """The packed state words of one env (cs_bridge.h) -> the hands in list order and the round's fields."""
    deck = [int(x) for x in np.array(w[:13], dtype='<u4').view(np.uint8)]
    masks = [int(w[13 + 2 * p]) | int(w[14 + 2 * p]) << 32 for p in range(4)]
    calls = [int(x) for x in np.array(w[21:31], dtype='<u4').view(np.uint8)]
    first, meta, play, trick = int(w[31]), int(w[32]), int(w[33]), int(w[34])
    ncalls, ncards = (meta >> 4) & 511, play & 63
    k = ncards & 3
    shown = 0 if ncards == 0 else (4 if k == 0 else k)
    passes = (meta >> 23) & 3
    return {'hands': [[c for c in (deck[51 - 13 * p - i] for i in range(13)) if c < 52 and (masks[p] >> c) & 1]
                      for p in range(4)],
            'calls': calls[:min(ncalls, CALLS_KEPT)], 'first': first, 'current': meta & 3, 'dealer': (meta >> 2) & 3,
            'ncalls': ncalls, 'last_bid': (meta >> 13) & 63, 'last_bidder': (meta >> 19) & 3,
            'cube': (1, 2, 4, 4)[(meta >> 21) & 3], 'passes': passes, 'last_call': (meta >> 25) & 63,
            'over': bool(meta >> 31), 'bidding_over': ncalls >= 4 and passes >= 3, 'ncards': ncards,
            'won': [(play >> 6) & 15, (play >> 10) & 15], 'declarer': (play >> 14) & 3, 'leader': (play >> 16) & 3,
            'trick': [(trick >> (8 * i)) & 255 for i in range(shown)]}


def legal_ids_of(s):
    """Judger.get_legal_actions of the current player as ids, in the reference's order"""
    if s['over']:
        return []
    cur = s['current']
    if not s['bidding_over']:
        ids = [PASS] + list(range(s['last_bid'] + 1, LAST_BID + 1))
        if s['last_bid']:
            theirs = (s['last_bidder'] ^ cur) & 1
            if theirs and s['cube'] == 1:
                ids.append(DBL)
            if not theirs and s['cube'] == 2:
                ids.append(RDBL)
        return ids
    hand = s['hands'][cur]
    if 0 < len(s['trick']) < 4:
        suit = [c for c in hand if c // 13 == s['trick'][0] // 13]
        if suit:
            hand = suit
    return [PLAY + c for c in hand]


def payoffs_of(s):
    """DefaultBridgePayoffDelegate.get_payoffs on the round as it stands"""
    if not s['last_bid']:
        return np.array([0, 0, 0, 0])
    side = s['last_bidder'] & 1
    need = bid_amount(s['last_bid']) + 6
    won = s['won'][side]
    decl = need + 2 if need <= won else won - need
    return np.array([decl if p & 1 == side else s['won'][side ^ 1] for p in range(4)])


class BridgeEnv(Env):
    name = 'bridge'
    default_game_config = {'game_num_players': 4}
    configurable = True   # a 'game_num_players' other than 4 is refused, not ignored
    actions = ACTION_LIST

    def __init__(self, config):
        super().__init__(config)
        self.state_shape = [[1, 573] for _ in range(self.num_players)]
        self.action_shape = [None for _ in range(self.num_players)]

    def _lists(self):
        return decode_words(self._state_words())

    def step_back(self):
        raise NotImplementedError   # (the reference's BridgeGame has no step_back)

    def _extract_state(self, out, player_id, via='get_state'):
        ids = legal_ids_of(self._lists())
        obs = out['obs'].astype(np.int64)
        # (the reference's state dict has these four keys in this order and no 'action_record')
        return {'obs': obs, 'legal_actions': OrderedDict((i, None) for i in ids), 'raw_legal_actions': list(ids),
                'raw_obs': obs}

    def _decode_action(self, action_id):
        """A legal id is played as it is; any other id plays the lowest legal id (the reference raises there; defined by
        the engine's ABI, include/cardsim.h). With nothing legal the id is decoded as it is: id 0 raises."""
        ids = legal_ids_of(self._lists())
        if ids and action_id not in ids:
            action_id = min(ids)
        return ActionEvent.from_action_id(action_id)

    def _action_id(self, raw):
        if isinstance(raw, ActionEvent):
            return raw.action_id
        return int(raw)

    def _raw_action(self, action_id):
        return ACTION_LIST[action_id]

    def get_payoffs(self):
        return payoffs_of(self._lists())

    def get_perfect_information(self):
        """round.get_perfect_information as plain data"""
        s = self._lists()
        dealer = s['dealer']
        vul = [[0, 0, 0, 0], [1, 0, 1, 0], [0, 1, 0, 1], [1, 1, 1, 1]][dealer]   # Tray.vul of board dealer + 1
        last_call = None
        if (not s['bidding_over'] or s['ncards'] == 0) and s['ncalls'] > 0:
            last_call = ((dealer + s['ncalls'] - 1) % 4, s['last_call'])
        trick = [None, None, None, None]
        for i, c in enumerate(s['trick']):
            trick[(s['leader'] + i) % 4] = c
        phase = 'game over' if s['over'] else ('play card' if s['bidding_over'] else 'make bid')
        state = {}
        state['move_count'] = 1 + s['ncalls'] + s['ncards']
        state['tray'] = (dealer + 1, dealer, vul)
        state['current_player_id'] = s['current']
        state['round_phase'] = phase
        state['last_call_move'] = last_call
        state['doubling_cube'] = s['cube']
        state['contact'] = (s['last_bidder'], s['last_bid']) if s['bidding_over'] and s['last_bid'] else None
        state['hands'] = s['hands']
        state['trick_moves'] = trick
        return state
