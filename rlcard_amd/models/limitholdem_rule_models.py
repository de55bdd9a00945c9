"""Limit Hold'em rule agent with the behaviour of rlcard/models/limitholdem_rule_models.py: it reads the raw state
(hand and public_cards as index strings, suit then rank: 'SA', 'HT') and answers an action name. The same rule runs on
the device as Limit::rule_action (rlcard_amd/csrc/cs_limit.h), selected by policy_id."""
from .model import Model
from .leducholdem_rule_models import legal_or_fallback

HIGH_KICKERS = 'KQJT'
HIGH_BOARD = 'AKQJT'
LOW_BOARD = '2345'


class LimitholdemRuleAgentV1(object):
    """Three kinds of hand, decided from the two hole ranks in order:
      a pair            raises before the flop, later only when the board holds its rank;
      an ace            with a K/Q/J/T kicker raises before the flop, later when the board holds any of A K Q J T; with a
                        smaller kicker it needs the two hole cards suited, later also that suit on the board;
      anything else     raises before the flop when both hole cards are K/Q/J/T; later it calls -- unless every board
                        card is a 2..5, where it checks on the flop and folds on the turn and river.
    Otherwise it folds. The last case restates the reference's max(public_cards_ranks) in ['5', '4', '3', '2']: a
    maximum of rank characters, in which every digit sorts below every letter, so it holds exactly when all board
    cards are 2..5. An action that is not legal becomes call (from raise), fold (from check) or raise (from call)."""
    policy_id = 1   # CS_POLICY_RULE_V1

    def __init__(self):
        self.use_raw = True

    @staticmethod
    def step(state):
        legal = state['raw_legal_actions']
        raw = state['raw_obs']
        hand, board = raw['hand'], raw['public_cards']
        r0, r1 = hand[0][1], hand[1][1]
        suited = hand[0][0] == hand[1][0]
        pair = r0 == r1
        ace = 'A' in (r0, r1)
        high_kicker = r0 in HIGH_KICKERS or r1 in HIGH_KICKERS
        board_ranks = [c[1] for c in board]
        board_suits = [c[0] for c in board]
        action = 'fold'
        if len(board) == 0:
            if pair or (ace and (high_kicker or suited)) or (not ace and r0 in HIGH_KICKERS and r1 in HIGH_KICKERS):
                action = 'raise'
        elif len(board) in (3, 4, 5):
            if pair:
                if r0 in board_ranks:
                    action = 'raise'
            elif ace:
                if high_kicker:
                    if any(r in HIGH_BOARD for r in board_ranks):
                        action = 'raise'
                elif suited and hand[0][0] in board_suits:
                    action = 'raise'
            elif all(r in LOW_BOARD for r in board_ranks):
                action = 'check' if len(board) == 3 else 'fold'
            else:
                action = 'call'
        return legal_or_fallback(action, legal)

    def eval_step(self, state):
        return self.step(state), []


class LimitholdemRuleModelV1(Model):
    num_players = 2   # the default limit-holdem table; the rule reads only the acting seat's own view

    def __init__(self):
        agent = LimitholdemRuleAgentV1()
        self.rule_agents = [agent for _ in range(self.num_players)]

    @property
    def agents(self):
        return self.rule_agents

    @property
    def use_raw(self):
        return True
