"""Bridge rule agent with the behaviour of rlcard/models/bridge_rule_models.py: it reads state['raw_legal_actions'] and
answers an action id. The same rule runs on the device as Bridge::rule_action (rlcard_amd/csrc/cs_bridge.h), selected
by policy_id; there the random pick takes the rollout's policy word instead of the global np.random. The reference
registers no model id for this agent, and neither does rlcard_amd.models: hand the agent itself to
VecEnv.rollout(policies=...), VecEnv.policy_actions or tournament_vec."""
import numpy as np

from ..envs.bridge import PASS


class BridgeDefenderNoviceRuleAgent(object):
    """Passes whenever pass is legal (the whole auction), otherwise plays a uniformly random legal card."""
    policy_id = 1   # CS_POLICY_RULE_V1

    def __init__(self):
        self.use_raw = False

    @staticmethod
    def step(state):
        legal = state['raw_legal_actions']
        if PASS in legal:
            return PASS
        return np.random.choice(legal)

    def eval_step(self, state):
        return self.step(state), []
