from .random_agent import RandomAgent  # noqa: F401
from .cfr_agent import CFRAgent  # noqa: F401
from .dmc_agent import DMCAgent, DMCModel, DMCNet, ActorBuffers, DMCActor  # noqa: F401
from .dqn_agent import DQNAgent, Estimator, EstimatorNetwork, Memory, DeviceMemory, DQNCollector  # noqa: F401
from .nfsp_agent import (NFSPAgent, AveragePolicyNetwork, ReservoirBuffer, DeviceReservoir,  # noqa: F401
                         NFSPCollector)
