"""UNO rule agent with the behaviour of rlcard/models/uno_rule_models.py: it reads the raw state (state['raw_obs'],
state['raw_legal_actions']) and answers an action name. The same rule runs on the device as Uno::rule_action
(rlcard_amd/csrc/cs_uno.h), selected by policy_id; there the random branch takes the rollout's policy word instead of
the global np.random, uniformly over the distinct legal ids."""
import numpy as np

from .model import Model


class UNORuleAgentV1(object):
    """Draws when it must; with a wild_draw_4 legal plays it in the colour most frequent in the hand; otherwise a random
    legal action, keeping the plain wild cards as long as anything else is legal."""
    policy_id = 1   # CS_POLICY_RULE_V1

    def __init__(self):
        self.use_raw = True

    def step(self, state):
        legal_actions = state['raw_legal_actions']
        hand = state['raw_obs']['hand']
        if 'draw' in legal_actions:
            return 'draw'
        for action in legal_actions:
            if action.split('-')[1] == 'wild_draw_4':
                color_nums = self.count_colors(self.filter_wild(hand))
                return max(color_nums, key=color_nums.get) + '-wild_draw_4'
        return np.random.choice(self.filter_wild(legal_actions))

    def eval_step(self, state):
        return self.step(state), []

    @staticmethod
    def filter_wild(hand):
        """The cards (or actions) that are not wild or wild_draw_4; all of them if nothing else is there."""
        filtered = [card for card in hand if card[2:6] != 'wild']
        return filtered if filtered else hand

    @staticmethod
    def count_colors(hand):
        """colour letter -> cards of that colour, keys in order of first appearance (max() keeps the first maximum)"""
        color_nums = {}
        for card in hand:
            color_nums[card[0]] = color_nums.get(card[0], 0) + 1
        return color_nums


class UNORuleModelV1(Model):
    num_players = 2

    def __init__(self):
        agent = UNORuleAgentV1()
        self.rule_agents = [agent for _ in range(self.num_players)]

    @property
    def agents(self):
        return self.rule_agents

    @property
    def use_raw(self):
        return True
