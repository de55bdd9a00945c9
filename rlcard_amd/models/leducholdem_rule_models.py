"""Leduc Hold'em rule agents with the behaviour of rlcard/models/leducholdem_rule_models.py: they read the raw state
(state['raw_obs'], state['raw_legal_actions']) and answer an action name. The same rules run on the device as
Leduc::rule_action (rlcard_amd/csrc/cs_leduc.h), selected by policy_id."""
from .model import Model

# what a rule plays when the action it wants is not legal (fold is always legal)
FALLBACK = {'raise': 'call', 'check': 'fold', 'call': 'raise'}


def legal_or_fallback(action, legal_actions):
    return action if action in legal_actions else FALLBACK.get(action, action)


class LeducHoldemRuleAgentV1(object):
    """Plays the most aggressive legal action: raise, else call, else check, else fold."""
    policy_id = 1   # CS_POLICY_RULE_V1

    def __init__(self):
        self.use_raw = True

    @staticmethod
    def step(state):
        legal = state['raw_legal_actions']
        for action in ('raise', 'call', 'check'):
            if action in legal:
                return action
        return 'fold'

    def eval_step(self, state):
        return self.step(state), []


class LeducHoldemRuleAgentV2(object):
    """With the public card out: raise when its rank matches the hand's (call where raise is illegal), fold otherwise.
    Before the public card the reference compares hand[0] with 'K' and 'Q'; a Leduc hand is an index string such as
    'SK', so hand[0] is the suit, neither branch is ever taken, and the agent always folds there. That is kept."""
    policy_id = 2   # CS_POLICY_RULE_V2

    def __init__(self):
        self.use_raw = True

    @staticmethod
    def step(state):
        legal = state['raw_legal_actions']
        raw = state['raw_obs']
        hand, public = raw['hand'], raw['public_card']
        if public:
            action = 'raise' if public[1] == hand[1] else 'fold'
        else:
            action = {'K': 'raise', 'Q': 'check'}.get(hand[0], 'fold')   # hand[0] is 'S' or 'H': always fold
        return legal_or_fallback(action, legal)

    def eval_step(self, state):
        return self.step(state), []


class _LeducRuleModel(Model):
    agent_class = None
    num_players = 2   # the default leduc-holdem table; the rules read only the acting seat's own view

    def __init__(self):
        agent = self.agent_class()
        self.rule_agents = [agent for _ in range(self.num_players)]

    @property
    def agents(self):
        return self.rule_agents


class LeducHoldemRuleModelV1(_LeducRuleModel):
    agent_class = LeducHoldemRuleAgentV1


class LeducHoldemRuleModelV2(_LeducRuleModel):
    agent_class = LeducHoldemRuleAgentV2
