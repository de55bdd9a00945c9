"""The base class of a loadable model (rlcard/models/model.py)."""


class Model(object):
    def __init__(self):
        pass

    @property
    def agents(self):
        """One agent per seat of the game, each with step(state), eval_step(state) and use_raw."""
        raise NotImplementedError
