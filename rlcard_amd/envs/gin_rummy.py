"""Gin Rummy env (rlcard/envs/gin_rummy.py, games/gin_rummy/) over the HIP engine (rlcard_amd/csrc/cs_gin_rummy.h).

Every raw field is decoded from the env's packed state words: the ordered stock pile, discard pile, hands and
known_cards, one byte per card (card id = rank + 13 * suit), the counts word and the meta word. obs and raw_obs are the
same [5][52] array and always show the current player, whoever asks; once the game is over they are all zero and the
legal set is empty, as in the reference.

The order of the legal actions is the reference's (judge.get_legal_actions): the discards in hand order, then the knocks
in the order of a CPython set of cards filled cluster by cluster from the player's memoised melds (player.py: sets by
rank id, then runs by suit). Card.__hash__ is rank + 100 * suit and CPython hashes a small int to itself, so a real set
of those ints iterates in the same order. The memo lists the four three-card subsets of four of a kind in hand order
when the four were dealt together and in S H D C order when the fourth card arrived later; the env follows which case
holds (_dealt4).

Two players and the reference's default Settings only. step_back raises NotImplementedError, as the reference's
GinRummyGame.step_back does; get_perfect_information raises NotImplementedError, as the reference's base Env does.
get_payoffs is computed on the host from the final state in float64, like the reference (the engine's reward rows are
the nearest f32)."""
from collections import OrderedDict

import numpy as np

from .env import Env

RANKS = ['A', '2', '3', '4', '5', '6', '7', '8', '9', 'T', 'J', 'Q', 'K']
SUITS = ['S', 'H', 'D', 'C']
SCORE_N, SCORE_S, DRAW, PICK, DEAD, GIN, DISCARD, KNOCK = 0, 1, 2, 3, 4, 5, 6, 58
L_NONE, L_DRAW, L_PICK, L_DISCARD, L_DEAD, L_GIN, L_KNOCK, L_SCORE_N, L_SCORE_S = range(9)
GO_DEAD, GO_KNOCK, GO_GIN = 1, 2, 3
MAX_MOVES, DEAD_STOCK = 200, 2
NAMES = ['score N', 'score S', 'draw_card', 'pick_up_discard', 'declare_dead_hand', 'gin']


def card_text(c):
    return RANKS[c % 13] + SUITS[c // 13]


def card_hash(c):
    return c % 13 + 100 * (c // 13)


def card_value(c):
    return min(c % 13 + 1, 10)


class ActionEvent(object):
    """games/gin_rummy/utils/action_event.py: an action is its id; discards and knocks carry their card id"""

    def __init__(self, action_id):
        self.action_id = int(action_id)
        self.card_id = (self.action_id - DISCARD) % 52 if self.action_id >= DISCARD else None

    def __eq__(self, other):
        return isinstance(other, ActionEvent) and self.action_id == other.action_id

    def __hash__(self):
        return hash(self.action_id)

    def __str__(self):
        a = self.action_id
        if a < DISCARD:
            return NAMES[a]
        return '%s %s' % ('discard' if a < KNOCK else 'knock', card_text(self.card_id))

    __repr__ = __str__


ACTION_LIST = [ActionEvent(i) for i in range(110)]


def decode_words(w):
    """The packed state words of one env (cs_gin_rummy.h) -> the ordered card lists and the round's fields."""
    b = np.array(w[:25], dtype='<u4').view(np.uint8)
    cnt, meta = int(w[25]), int(w[26])
    ns, nd = cnt & 63, (cnt >> 6) & 63
    nh = [(cnt >> 12) & 15, (cnt >> 16) & 15]
    nk = [(cnt >> 20) & 15, (cnt >> 24) & 15]
    return {'stock': [int(x) for x in b[:ns]], 'discard': [int(b[51 - i]) for i in range(nd)],
            'hands': [[int(b[52 + 12 * p + i]) for i in range(nh[p])] for p in range(2)],
            'known': [[int(b[76 + 12 * p + i]) for i in range(nk[p])] for p in range(2)],
            'current': meta & 1, 'dealer': (meta >> 1) & 1, 'last': (meta >> 2) & 15, 'picked': (meta >> 6) & 63,
            'moves': (meta >> 12) & 255, 'go_kind': (meta >> 20) & 3, 'go_player': (meta >> 22) & 1,
            'over': bool((meta >> 23) & 1), 'gone': (meta >> 24) & 63 if (meta >> 30) & 1 else None}


# ---- melds on the host (the raw side's orders and the float64 payoffs; the engine's judge is cs_gin_melds.h) ---------
def run_melds(hand):
    """melding.get_all_run_melds as card-id tuples: by suit, every maximal run's slices [i, j), i then j ascending"""
    out = []
    have = set(hand)
    for s in range(4):
        r = 0
        while r < 13:
            if 13 * s + r not in have:
                r += 1
                continue
            e = r
            while e < 13 and 13 * s + e in have:
                e += 1
            n = e - r
            for i in range(n - 2):
                for j in range(i + 3, n + 1):
                    out.append(tuple(13 * s + r + k for k in range(i, j)))
            r = e
    return out


def set_melds_memo(hand, dealt4=()):
    """player.py's meld_kinds_by_rank_id flattened: by rank id; four of a kind gives the whole set and its four
    three-card subsets, leaving out each card in hand order (dealt together) or in S H D C order (grown)"""
    out = []
    for r in range(13):
        cards = [c for c in hand if c % 13 == r]
        if len(cards) == 3:
            out.append(tuple(cards))
        elif len(cards) == 4:
            if r not in dealt4:
                cards = [13 * s + r for s in range(4)]
            out.append(tuple(cards))
            out.extend(tuple(c for c in cards if c != x) for x in cards)
    return out


def clusters(melds):
    """get_meld_clusters: every meld, disjoint pair i < j and disjoint triple i < j < k, in that nesting"""
    sets = [frozenset(m) for m in melds]
    for i in range(len(melds)):
        yield (i,)
        for j in range(i + 1, len(melds)):
            if sets[j] & sets[i]:
                continue
            yield (i, j)
            for k in range(j + 1, len(melds)):
                if sets[k] & sets[i] or sets[k] & sets[j]:
                    continue
                yield (i, j, k)


def best_deadwood(hand):
    melds = run_melds(hand) + set_melds_memo(hand)
    total = sum(card_value(c) for c in hand)
    best = total
    for cl in clusters(melds):
        best = min(best, total - sum(card_value(c) for i in cl for c in melds[i]))
    return best


def going_out_memo(hand, dealt4=()):
    """judge._get_going_out_cards over the player's memoised clusters -> (knock card ids in the reference's list order,
    whether the gin set is non-empty)"""
    melds = set_melds_memo(hand, dealt4) + run_melds(hand)
    knock, gin = set(), False
    for cl in clusters(melds):
        melded = set(c for i in cl for c in melds[i])
        dead = [c for c in hand if c not in melded]
        if len(dead) <= 1:
            gin = True
            continue
        values = [card_value(c) for c in dead]
        count = sum(values)
        if count <= 10 + max(values):
            for c in dead:
                if count - card_value(c) <= 10:
                    knock.add(card_hash(c))
    return [h % 100 + 13 * (h // 100) for h in knock], gin


def legal_ids_of(s, dealt4=()):
    """Judge.get_legal_actions of the current player as ids, in the reference's order"""
    if s['over']:
        return []
    la = s['last']
    if la in (L_NONE, L_DRAW, L_PICK):
        hand = s['hands'][s['current']]
        knock, gin = going_out_memo(hand, dealt4) if len(hand) == 11 else ([], False)
        if gin:
            return [GIN]
        cards = [c for c in hand if not (la == L_PICK and c == s['picked'])]
        return [DISCARD + c for c in cards] + [KNOCK + c for c in knock]
    if la == L_DISCARD:
        if s['moves'] >= MAX_MOVES:
            return [DEAD]
        return [DRAW, PICK] if len(s['stock']) > DEAD_STOCK else [DEAD, PICK]
    if la == L_SCORE_N:
        return [SCORE_S]
    if la == L_SCORE_S:
        return []
    return [SCORE_N]


class GinRummyEnv(Env):
    name = 'gin-rummy'
    default_game_config = {'game_num_players': 2}
    configurable = True   # a 'game_num_players' other than 2 is refused, not ignored
    actions = ACTION_LIST

    def __init__(self, config):
        super().__init__(config)
        self.state_shape = [[5, 52] for _ in range(self.num_players)]
        self.action_shape = [None for _ in range(self.num_players)]
        self._dealt4 = [set(), set()]

    def _lists(self):
        return decode_words(self._state_words())

    # which ranks a seat holds as four of a kind dealt together (see the module docstring)
    def _after_deal(self):
        s = self._lists()
        self._dealt4 = [set(r for r in range(13) if sum(1 for c in h if c % 13 == r) == 4) for h in s['hands']]

    def _after_step(self, player, decoded, before):
        s = self._lists()
        for p in range(2):
            self._dealt4[p] = set(r for r in self._dealt4[p] if sum(1 for c in s['hands'][p] if c % 13 == r) == 4)

    def step_back(self):
        raise NotImplementedError   # games/gin_rummy/game.py step_back

    def _extract_state(self, out, player_id, via='get_state'):
        s = self._lists()
        ids = legal_ids_of(s, self._dealt4[s['current']])
        obs = out['obs'].astype(np.int64).reshape(5, 52)
        # (the reference's state dict has these four keys and no 'action_record')
        return {'obs': obs, 'legal_actions': OrderedDict((i, None) for i in ids), 'raw_legal_actions': list(ids),
                'raw_obs': obs}

    def _decode_action(self, action_id):
        """A legal id is played as it is; any other id plays the lowest legal id (the reference raises or corrupts its
        lists there; defined by the engine's ABI, include/cardsim.h)."""
        s = self._lists()
        ids = legal_ids_of(s, self._dealt4[s['current']])
        if ids and action_id not in ids:
            action_id = min(ids)
        return ACTION_LIST[action_id]

    def _action_id(self, raw):
        if isinstance(raw, ActionEvent):
            return raw.action_id
        return int(raw)

    def _raw_action(self, action_id):
        return ACTION_LIST[action_id]

    def get_payoffs(self):
        """envs/gin_rummy.py get_payoffs: [0, 0] until `score south` has been played, then get_payoff_gin_rummy_v1 of
        both seats in float64"""
        s = self._lists()
        if not (s['over'] and s['last'] == L_SCORE_S):
            return np.array([0, 0])
        pay = []
        for p in range(2):
            if s['go_player'] == p and s['go_kind'] == GO_KNOCK:
                pay.append(0.2)
            elif s['go_player'] == p and s['go_kind'] == GO_GIN:
                pay.append(1)
            else:
                pay.append(-best_deadwood(s['hands'][p]) / 100)
        return np.array(pay)
