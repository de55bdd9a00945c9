"""Model registry (rlcard/models/registration.py): register(model_id, entry_point) / load(model_id). The entry point
('module:Class') is imported when the model is first loaded."""
import importlib

# names VecEnv.rollout(policies=...) accepts -> the engine's policy id (include/cardsim.h CS_POLICY_*)
POLICY_IDS = {'random': 0, 'leduc-holdem-rule-v1': 1, 'leduc-holdem-rule-v2': 2, 'limit-holdem-rule-v1': 1,
              'uno-rule-v1': 1, 'gin-rummy-novice-rule': 1}


def policy_id_of(policy):
    """A policy given as a registered name, an engine id, or an agent carrying policy_id -> the engine id."""
    if isinstance(policy, str):
        if policy not in POLICY_IDS:
            raise ValueError('Cannot find policy: {}'.format(policy))
        return POLICY_IDS[policy]
    if hasattr(policy, 'policy_id'):
        return int(policy.policy_id)
    return int(policy)


class ModelSpec(object):
    def __init__(self, model_id, entry_point):
        self.model_id = model_id
        self.entry_point = entry_point

    def load(self):
        mod_name, class_name = self.entry_point.split(':')
        return getattr(importlib.import_module(mod_name), class_name)()


class ModelRegistry(object):
    def __init__(self):
        self.model_specs = {}

    def register(self, model_id, entry_point):
        if model_id in self.model_specs:
            raise ValueError('Cannot re-register model_id: {}'.format(model_id))
        self.model_specs[model_id] = ModelSpec(model_id, entry_point)

    def load(self, model_id):
        if model_id not in self.model_specs:
            raise ValueError('Cannot find model_id: {}'.format(model_id))
        return self.model_specs[model_id].load()


model_registry = ModelRegistry()


def register(model_id, entry_point):
    return model_registry.register(model_id, entry_point)


def load(model_id):
    return model_registry.load(model_id)
