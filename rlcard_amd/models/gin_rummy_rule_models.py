"""Gin Rummy novice rule agent with the behaviour of rlcard/models/gin_rummy_rule_models.py: it reads
state['legal_actions'] and the hand plane state['obs'][0] and answers an action id. The same rule runs on the device as
GinRummy::rule_action (rlcard_amd/csrc/cs_gin_rummy.h), selected by policy_id; there every pick takes the rollout's
policy word instead of the global np.random."""
from collections import OrderedDict

import numpy as np

from .model import Model
from ..envs.gin_rummy import GIN, DISCARD, KNOCK, best_deadwood


class GinRummyNoviceRuleAgent(object):
    """Gins if it can, else knocks if it can, else discards a card that leaves the least best deadwood in the other ten,
    else plays a random legal action."""
    policy_id = 1   # CS_POLICY_RULE_V1

    def __init__(self):
        self.use_raw = False

    @staticmethod
    def candidates(state):
        """the ids the rule chooses from, in the reference's list order"""
        legal = list(state['legal_actions'].keys()) if isinstance(state['legal_actions'], (dict, OrderedDict)) \
            else list(state['legal_actions'])
        gins = [a for a in legal if a == GIN]
        knocks = [a for a in legal if a >= KNOCK]
        discards = [a for a in legal if DISCARD <= a < KNOCK]
        if gins:
            return gins
        if knocks:
            return knocks
        if discards:
            hand = [int(c) for c in np.flatnonzero(np.asarray(state['obs'])[0])]
            best, final = [], 999
            for a in discards:
                dw = best_deadwood([c for c in hand if c != a - DISCARD])
                if dw < final:
                    final, best = dw, [a]
                elif dw == final:
                    best.append(a)
            if best:
                return best
        return legal

    @staticmethod
    def step(state):
        return np.random.choice(GinRummyNoviceRuleAgent.candidates(state))

    def eval_step(self, state):
        return self.step(state), []


class GinRummyNoviceRuleModel(Model):
    num_players = 2

    def __init__(self):
        agent = GinRummyNoviceRuleAgent()
        self.rule_agents = [agent for _ in range(self.num_players)]

    @property
    def agents(self):
        return self.rule_agents
