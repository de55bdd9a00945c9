"""Rule-based opponents with the surface of rlcard/models/: register / load(name) -> a Model whose .agents holds one
agent per seat. Every agent here also carries policy_id, the id the engine's fused rollout plays for that rule on the
device (include/cardsim.h CS_POLICY_*; VecEnv.rollout(policies=...), VecEnv.policy_actions, utils.tournament_vec)."""
from .registration import register, load, POLICY_IDS, policy_id_of  # noqa: F401
from .model import Model  # noqa: F401

register(model_id='leduc-holdem-rule-v1', entry_point='rlcard_amd.models.leducholdem_rule_models:LeducHoldemRuleModelV1')
register(model_id='leduc-holdem-rule-v2', entry_point='rlcard_amd.models.leducholdem_rule_models:LeducHoldemRuleModelV2')
register(model_id='limit-holdem-rule-v1', entry_point='rlcard_amd.models.limitholdem_rule_models:LimitholdemRuleModelV1')
register(model_id='uno-rule-v1', entry_point='rlcard_amd.models.uno_rule_models:UNORuleModelV1')
register(model_id='gin-rummy-novice-rule',
         entry_point='rlcard_amd.models.gin_rummy_rule_models:GinRummyNoviceRuleModel')
