"""NFSP (Neural Fictitious Self-Play, https://arxiv.org/abs/1603.01121): a DQN best response plus an average-policy
network trained by supervised learning on the best response's own actions, held in a reservoir buffer.

* AveragePolicyNetwork / ReservoirBuffer / NFSPAgent -- the API and the torch module layout of
  rlcard/agents/nfsp_agent.py (`mlp` = Flatten, BatchNorm1d, Linear/ReLU ..., Linear with a log-softmax forward, so a
  reference state_dict loads unchanged), used one state at a time through rlcard_amd.make(...).run().
* The vectorised path, for every env of a VecEnv at once (include/cardsim.h, rlcard_amd/csrc/cs_dqn.hip, cs_nfsp.hip):
    AveragePolicyNetwork.folded()   the network as the kernels take it: a cs_qnet descriptor read as Linear/ReLU
    NFSPAgent.step_vec              cs_nfsp_actions: each env in its own mode, the Q-network's epsilon-greedy action or
                                    an action sampled from the average policy, each network on its own rows
    NFSPAgent.eval_step_vec / predict_probs_vec   the average policy alone (cs_nfsp_actions without modes, cs_pnet_probs)
    DeviceReservoir                 cs_reservoir: the reservoir buffer in HBM, filled from rollout-layout trajectories
    NFSPAgent.feed_vec / train_sl   the inner DQNAgent.feed_vec, the reservoir push, and the cross-entropy step in torch
    NFSPCollector                   DQNCollector's acting loop with the mode of every step recorded
"""
import ctypes as C
import os
import random
from collections import namedtuple

import numpy as np
import torch
from torch import nn

from .. import _abi
from ..utils import remove_illegal
from .._abi import ptr as _ptr
from .dqn_agent import DQNAgent, DQNCollector, DeviceBuffer, descriptor, fold_batchnorm, seat_mask

Transition = namedtuple('Transition', 'info_state action_probs')


class AveragePolicyNetwork(nn.Module):
    """Flatten -> BatchNorm1d -> Linear (-> ReLU, except after the last) per entry of mlp_layers, whose last entry is
    num_actions. forward gives the log-probabilities."""

    def __init__(self, num_actions=2, state_shape=None, mlp_layers=None):
        super().__init__()
        self.num_actions = num_actions
        self.state_shape = state_shape
        self.mlp_layers = mlp_layers
        dims = [int(np.prod(state_shape))] + [int(w) for w in mlp_layers]
        mlp = [nn.Flatten(), nn.BatchNorm1d(dims[0])]
        for k, (i, o) in enumerate(zip(dims[:-1], dims[1:])):
            mlp.append(nn.Linear(i, o))
            if k != len(dims) - 2:
                mlp.append(nn.ReLU())
        self.mlp = nn.Sequential(*mlp)
        self._folded = None

    def forward(self, s):
        return torch.log_softmax(self.mlp(s), dim=-1)

    def load_state_dict(self, *args, **kw):
        r = super().load_state_dict(*args, **kw)
        self._folded = None
        return r

    # -- the network as the kernels take it --------------------------------------------------------------------------
    def folded_weights(self):
        """[(W, b)] per Linear as float64 numpy, the eval-mode BatchNorm folded into the first (dqn_agent.fold_batchnorm)."""
        return fold_batchnorm(self.mlp[1], [m for m in self.mlp if isinstance(m, nn.Linear)])

    def _version(self):
        sd = self.state_dict()
        return tuple(t._version for t in sd.values()) + (str(next(iter(sd.values())).device),)

    def folded(self):
        """The cs_qnet descriptor (_abi.QNet) of this network, which cs_pnet_probs and cs_nfsp_actions read as
        Linear/ReLU: folded_weights() as float32 tensors on the network's device (the first bias folded around those
        float32 weights, fold_batchnorm's weights32). Cached; train_sl(),
        load_state_dict() and any in-place change of the parameters invalidate it."""
        ver = self._version()
        if self._folded is not None and self._folded[0] == ver:
            return self._folded[1]
        net = descriptor(fold_batchnorm(self.mlp[1], [m for m in self.mlp if isinstance(m, nn.Linear)], weights32=True),
                         self.mlp[1].weight.device)
        self._folded = (ver, net)
        return net

    # -- checkpoints ---------------------------------------------------------------------------------------------------
    def checkpoint_attributes(self):
        return {'num_actions': self.num_actions, 'state_shape': self.state_shape, 'mlp_layers': self.mlp_layers,
                'mlp': self.mlp.state_dict()}

    @classmethod
    def from_checkpoint(cls, checkpoint):
        net = cls(num_actions=checkpoint['num_actions'], state_shape=checkpoint['state_shape'],
                  mlp_layers=checkpoint['mlp_layers'])
        net.mlp.load_state_dict(checkpoint['mlp'])
        return net


class ReservoirBuffer:
    """Reservoir sampling over a stream (https://en.wikipedia.org/wiki/Reservoir_sampling): the host list. Element k
    of the stream is appended while the list is short of its capacity; afterwards it replaces element
    np.random.randint(0, k + 1) if that index is inside the list."""

    def __init__(self, reservoir_buffer_capacity):
        self._reservoir_buffer_capacity = reservoir_buffer_capacity
        self._data = []
        self._add_calls = 0

    def add(self, element):
        if len(self._data) < self._reservoir_buffer_capacity:
            self._data.append(element)
        else:
            idx = np.random.randint(0, self._add_calls + 1)
            if idx < self._reservoir_buffer_capacity:
                self._data[idx] = element
        self._add_calls += 1

    def sample(self, num_samples):
        if len(self._data) < num_samples:
            raise ValueError('{} elements could not be sampled from size {}'.format(num_samples, len(self._data)))
        return random.sample(self._data, num_samples)

    def clear(self):
        self._data = []
        self._add_calls = 0

    def checkpoint_attributes(self):
        return {'data': self._data, 'add_calls': self._add_calls,
                'reservoir_buffer_capacity': self._reservoir_buffer_capacity}

    @classmethod
    def from_checkpoint(cls, checkpoint):
        buf = cls(checkpoint['reservoir_buffer_capacity'])
        buf._data = checkpoint['data']
        buf._add_calls = checkpoint['add_calls']
        return buf

    def __len__(self):
        return len(self._data)

    def __iter__(self):
        return iter(self._data)


class DeviceReservoir(DeviceBuffer):
    """The reservoir buffer of a VecEnv's envs in HBM (include/cardsim.h cs_reservoir): push() offers a rollout-layout
    trajectory's best-response rows with ReservoirBuffer.add's semantics, the replacement draws Philox keyed by `seed`
    on the element's stream index; index k is slot k, as in ReservoirBuffer's list. sizes(): (elements held, elements
    ever offered: ReservoirBuffer._add_calls)."""
    KIND, TOO_MANY = 'reservoir', '%d elements could not be sampled from size %d'

    def __init__(self, vec, capacity, seed=0):
        self.vec, self.capacity, self.seed = vec, int(capacity), int(seed) & (2 ** 64 - 1)
        self.create('cs_reservoir_create', vec._h, self.capacity, self.seed, device=vec.device)

    def push(self, traj, mode_rows, seats):
        """Offer the rows of a trajectory ([T][N] rows) that the seats `seats` played with mode_rows[t][e] != 0 (uint8
        [T][N], the best-response steps)."""
        T = traj['player'].shape[0]
        if tuple(mode_rows.shape) != tuple(traj['player'].shape) or mode_rows.dtype != torch.uint8:
            raise ValueError('mode_rows must be uint8 %s' % (tuple(traj['player'].shape),))
        self._call('push', int(T), C.byref(_abi.traj(traj)), _ptr(mode_rows.contiguous()), seat_mask(seats),
                   self.vec._stream())

    @property
    def add_calls(self):
        return self.sizes()[1]

    def gather(self, idx):
        """Slots idx (int64, each in [0, len(self))) -> dict of device tensors: state float32 [B, obs_dim],
        action_probs float32 [B, num_actions] (one-hot)."""
        v, d = self.vec, self.vec.device
        idx, B = self._indices(idx)
        out = dict(state=torch.empty((B, v.obs_dim), dtype=torch.float32, device=d),
                   action_probs=torch.empty((B, v.num_actions), dtype=torch.float32, device=d))
        if B:
            self._call('gather', _ptr(idx), B, _ptr(out['state']), _ptr(out['action_probs']), v._stream())
        return out

    def clear(self):
        self._call('clear', self.vec._stream())


class NFSPAgent:
    """rlcard's NFSPAgent (constructor arguments and methods), plus attach() and the *_vec methods for a VecEnv. As in
    the reference, the supervised step minimises the cross-entropy against the stored action probabilities, which are
    one-hot rows of the best response's actions."""

    def __init__(self, num_actions=4, state_shape=None, hidden_layers_sizes=None, reservoir_buffer_capacity=20000,
                 anticipatory_param=0.1, batch_size=256, train_every=1, rl_learning_rate=0.1, sl_learning_rate=0.005,
                 min_buffer_size_to_learn=100, q_replay_memory_size=20000, q_replay_memory_init_size=100,
                 q_update_target_estimator_every=1000, q_discount_factor=0.99, q_epsilon_start=0.06, q_epsilon_end=0,
                 q_epsilon_decay_steps=int(1e6), q_batch_size=32, q_train_every=1, q_mlp_layers=None,
                 evaluate_with='average_policy', device=None, save_path=None, save_every=float('inf')):
        self.use_raw = False
        self._num_actions = num_actions
        self._state_shape = state_shape
        self._layer_sizes = list(hidden_layers_sizes) + [num_actions]
        self._batch_size = batch_size
        self._train_every = train_every
        self._sl_learning_rate = sl_learning_rate
        self._anticipatory_param = anticipatory_param
        self._min_buffer_size_to_learn = min_buffer_size_to_learn
        self._reservoir_buffer = ReservoirBuffer(reservoir_buffer_capacity)
        self.evaluate_with = evaluate_with
        if device is None:
            device = torch.device('cuda:0' if torch.cuda.is_available() else 'cpu')
        self.device = device
        self.total_t = 0    # transitions fed
        self.train_t = 0    # train_sl() steps taken
        self._rl_agent = DQNAgent(q_replay_memory_size, q_replay_memory_init_size, q_update_target_estimator_every,
                                  q_discount_factor, q_epsilon_start, q_epsilon_end, q_epsilon_decay_steps,
                                  q_batch_size, num_actions, state_shape, q_train_every, q_mlp_layers,
                                  rl_learning_rate, device)
        self.policy_network = AveragePolicyNetwork(num_actions, state_shape, self._layer_sizes).to(self.device)
        self.policy_network.eval()
        for p in self.policy_network.parameters():
            if p.dim() > 1:
                nn.init.xavier_uniform_(p.data)
        self.policy_network_optimizer = torch.optim.Adam(self.policy_network.parameters(), lr=sl_learning_rate)
        self.sample_episode_policy()
        self.vec = None
        self.device_reservoir = None
        self.mode = None           # uint8 [N][num_players] after attach(): 1 best_response, 0 average_policy
        self.generator = None      # torch.Generator of DeviceReservoir.sample (None: torch's global one)
        self.mode_generator = None   # torch.Generator of sample_episode_policy_vec calls without a seed
        self._scratch = None
        self._seeded = None        # the generator sample_episode_policy_vec re-seeds per call
        self.last_loss = None
        self.save_path = save_path
        self.save_every = save_every

    # -- one state at a time (the reference's API) ---------------------------------------------------------------------
    def feed(self, ts):
        """Feed one transition to the inner DQN agent; once the reservoir holds min_buffer_size_to_learn elements,
        train the average policy every train_every transitions."""
        self._rl_agent.feed(ts)
        self.total_t += 1
        if self.total_t > 0 and len(self._reservoir_buffer) >= self._min_buffer_size_to_learn and \
                self.total_t % self._train_every == 0:
            self.train_sl()

    def step(self, state):
        """The action for training. best_response: the inner DQN's epsilon-greedy action, stored with the state as a
        one-hot row; average_policy: a draw from the average policy over the legal actions."""
        obs = state['obs']
        legal = list(state['legal_actions'].keys())
        if self._mode == 'best_response':
            action = self._rl_agent.step(state)
            one_hot = np.zeros(self._num_actions)
            one_hot[action] = 1
            self._add_transition(obs, one_hot)
        else:
            probs = remove_illegal(self._act(obs), legal)
            action = np.random.choice(len(probs), p=probs)
        return action

    def eval_step(self, state):
        """evaluate_with 'average_policy': a draw from the average policy, info['probs'] per raw legal action;
        'best_response': the inner DQN's eval_step."""
        if self.evaluate_with == 'best_response':
            return self._rl_agent.eval_step(state)
        if self.evaluate_with != 'average_policy':
            raise ValueError("'evaluate_with' should be either 'average_policy' or 'best_response'.")
        legal = list(state['legal_actions'].keys())
        probs = remove_illegal(self._act(state['obs']), legal)
        action = np.random.choice(len(probs), p=probs)
        info = {'probs': {state['raw_legal_actions'][i]: float(probs[legal[i]]) for i in range(len(legal))}}
        return action, info

    def sample_episode_policy(self):
        """Draw the episode's mode: best_response with probability anticipatory_param."""
        self._mode = 'best_response' if np.random.rand() < self._anticipatory_param else 'average_policy'

    def _act(self, info_state):
        """The average policy's probabilities of one observation (every action, illegal ones included)."""
        x = torch.from_numpy(np.expand_dims(info_state, axis=0)).float().to(self.device)
        with torch.no_grad():
            logp = self.policy_network(x).cpu().numpy()
        return np.exp(logp)[0]

    def _add_transition(self, state, probs):
        self._reservoir_buffer.add(Transition(info_state=state, action_probs=probs))

    def sl_loss(self, info_states, action_probs):
        """The cross-entropy of a batch in train mode (batch statistics in the BatchNorm), inside the graph."""
        logp = self.policy_network(info_states)
        return -(action_probs * logp).sum(dim=-1).mean()

    def train_sl(self):
        """One Adam step of the average policy on a sampled batch -> the loss, or None while the buffer holds fewer
        than batch_size or min_buffer_size_to_learn elements. With a device reservoir attached the batch is sampled
        and stacked on the device."""
        res = self.device_reservoir
        held = len(res) if res is not None else len(self._reservoir_buffer)
        if held < self._batch_size or held < self._min_buffer_size_to_learn:
            return None
        if res is not None:
            b = res.sample(self._batch_size, self.generator)
            info_states, action_probs = b['state'], b['action_probs']
        else:
            transitions = self._reservoir_buffer.sample(self._batch_size)
            info_states = torch.from_numpy(np.array([t.info_state for t in transitions])).float().to(self.device)
            action_probs = torch.from_numpy(np.array([t.action_probs for t in transitions])).float().to(self.device)
        self.policy_network_optimizer.zero_grad()
        self.policy_network.train()
        loss = self.sl_loss(info_states, action_probs)
        loss.backward()
        self.policy_network_optimizer.step()
        self.policy_network.eval()
        self.policy_network._folded = None
        self.last_loss = loss = loss.item()
        self.train_t += 1
        if self.save_path and self.train_t % self.save_every == 0:
            self.save_checkpoint(self.save_path)
        return loss

    def set_device(self, device):
        self.device = device
        self._rl_agent.set_device(device)
        self.policy_network.to(device)
        self.policy_network._folded = None

    # -- every env of a VecEnv at once ---------------------------------------------------------------------------------
    @property
    def device_memory(self):
        return self._rl_agent.device_memory

    def attach(self, vec, replay_memory_size=None, reservoir_buffer_capacity=None, seed=0):
        """Use `vec`'s device: the inner DQN attaches (its replay memory becomes a DeviceMemory), the average policy
        moves there, the reservoir becomes a DeviceReservoir (default capacity: the host buffer's; `seed` keys its
        replacement draws) and every (env, seat) gets a mode byte, all average_policy until
        sample_episode_policy_vec draws them."""
        self.vec = vec
        self._rl_agent.attach(vec, replay_memory_size)
        self.set_device(vec.device)
        for st in self.policy_network_optimizer.state.values():
            for k, x in st.items():
                if torch.is_tensor(x):
                    st[k] = x.to(vec.device)
        cap = int(reservoir_buffer_capacity if reservoir_buffer_capacity is not None
                  else self._reservoir_buffer._reservoir_buffer_capacity)
        self.device_reservoir = DeviceReservoir(vec, cap, seed)
        self.mode = torch.zeros((vec.num_envs, vec.num_players), dtype=torch.uint8, device=vec.device)
        self._scratch = None
        return self.device_reservoir

    def _need_vec(self):
        if self.vec is None:
            raise _abi.CardsimError('NFSPAgent.attach(vec) comes before the *_vec methods')
        return self.vec

    def sample_episode_policy_vec(self, where=None, t=0, seed=None):
        """sample_episode_policy for every seat of the envs in `where` (bool [N]; None: every env): best_response with
        probability anticipatory_param. The draw comes from a torch.Generator on the device: one seeded with (seed, t)
        for this call, or, without a seed, the agent's mode_generator (None: torch's global one)."""
        v = self._need_vec()
        g = self.mode_generator
        if seed is not None:
            if self._seeded is None or self._seeded.device != torch.device(v.device):
                self._seeded = torch.Generator(device=v.device)
            g = self._seeded
            g.manual_seed((int(seed) * 0x9E3779B97F4A7C15 + int(t) * 0xD1B54A32D192ED03 + 1) & (2 ** 63 - 1))
        new = (torch.rand(self.mode.shape, generator=g, device=v.device) < self._anticipatory_param).to(torch.uint8)
        self.mode = new if where is None else torch.where(where.bool().unsqueeze(-1), new, self.mode)
        return self.mode

    def mode_rows(self, state):
        """uint8 [N]: the mode of each env's acting seat."""
        p = state['player'].long().clamp_max(self.vec.num_players - 1).unsqueeze(-1)
        return self.mode.gather(1, p).squeeze(-1).contiguous()

    def _nfsp_actions(self, state, mode_rows, eps, t, seed, probs=None):
        v = self._need_vec()
        obs, legal, done = state['obs'], state['legal'], state.get('done')
        rows = obs.shape[0]
        out = torch.empty(rows, dtype=torch.int32, device=v.device)
        qnet = None
        if mode_rows is not None:
            qnet = C.byref(self._rl_agent.q_estimator.folded())
            if self._scratch is None or self._scratch[0] != rows:
                need = _abi.call('cs_nfsp_scratch_bytes', rows)
                self._scratch = (rows, torch.empty(need, dtype=torch.uint8, device=v.device))
        scratch = self._scratch[1] if mode_rows is not None else None
        _abi.call('cs_nfsp_actions', v._h, qnet, C.byref(self.policy_network.folded()), _ptr(obs), _ptr(legal),
                  _ptr(done), _ptr(mode_rows), rows, float(eps), int(seed) & (2 ** 64 - 1), int(t), v.env_base,
                  _ptr(out), _ptr(probs), _ptr(scratch), v._stream(), device=v.device)
        return out

    def step_vec(self, state, t, seed=0, mode_rows=None):
        """NFSPAgent.step for every env of a step output `state` (obs, legal, player, done), each in the mode of its
        acting seat (or mode_rows uint8 [N]): int32 [N] actions, -1 where the env's game is over. Storing the
        best-response steps is feed_vec's part. The draws are keyed by (seed, env, t)."""
        if mode_rows is None:
            mode_rows = self.mode_rows(state)
        return self._nfsp_actions(state, mode_rows, self._rl_agent.epsilon(), t, seed)

    def eval_step_vec(self, state, t=0, seed=0):
        """NFSPAgent.eval_step for every env: an action sampled from the average policy (keyed by (seed, env, t)), or
        the greedy Q action with evaluate_with='best_response'."""
        if self.evaluate_with == 'best_response':
            return self._rl_agent.eval_step_vec(state, t, seed)
        if self.evaluate_with != 'average_policy':
            raise ValueError("'evaluate_with' should be either 'average_policy' or 'best_response'.")
        return self._nfsp_actions(state, None, 0.0, t, seed)

    def predict_probs_vec(self, obs, legal=None):
        """The average policy for rows of observations (cs_pnet_probs): float32 [rows, num_actions], 0 where
        illegal."""
        v = self._need_vec()
        probs = torch.empty((obs.shape[0], self._num_actions), dtype=torch.float32, device=v.device)
        _abi.call('cs_pnet_probs', v._h, C.byref(self.policy_network.folded()), _ptr(obs), _ptr(legal), obs.shape[0],
                  _ptr(probs), v._stream(), device=v.device)
        return probs

    def sl_steps_for(self, t0, t1):
        """train_sl() calls the reference's feed makes while total_t goes from t0 to t1 with the buffer past
        min_buffer_size_to_learn: the multiples of train_every in (t0, t1]."""
        e = self._train_every
        return max(0, t1 // e - t0 // e)

    def feed_vec(self, traj, mode_rows, seats, train_steps=None, sl_steps=None, fused=False):
        """The inner DQNAgent.feed_vec (push, train), then the trajectory's best-response rows of `seats` into the
        reservoir; total_t advances by the transitions the replay memory took, and train_sl runs as often as feed
        would have run it over that advance, with the reservoir as the push left it (or exactly sl_steps times)
        -> (the DQN losses, the average-policy losses). fused: the inner agent's steps run on the device
        (DQNAgent.train_fused); train_sl stays torch."""
        rl = self._rl_agent
        t_rl = rl.total_t
        rl_losses = rl.feed_vec(traj, seats, train_steps, fused)
        self.device_reservoir.push(traj, mode_rows, seats)
        t0 = self.total_t
        self.total_t += rl.total_t - t_rl
        if sl_steps is None:
            enough = len(self.device_reservoir) >= self._min_buffer_size_to_learn
            sl_steps = self.sl_steps_for(t0, self.total_t) if enough else 0
        sl_losses = [self.train_sl() for _ in range(int(sl_steps))]
        return rl_losses, [x for x in sl_losses if x is not None]

    # -- checkpoints ---------------------------------------------------------------------------------------------------
    def checkpoint_attributes(self):
        return {
            'agent_type': 'NFSPAgent',
            'policy_network': self.policy_network.checkpoint_attributes(),
            'reservoir_buffer': self._reservoir_buffer.checkpoint_attributes(),
            'rl_agent': self._rl_agent.checkpoint_attributes(),
            'policy_network_optimizer': self.policy_network_optimizer.state_dict(),
            'device': self.device,
            'anticipatory_param': self._anticipatory_param,
            'batch_size': self._batch_size,
            'min_buffer_size_to_learn': self._min_buffer_size_to_learn,
            'num_actions': self._num_actions,
            'mode': self._mode,
            'evaluate_with': self.evaluate_with,
            'total_t': self.total_t,
            'train_t': self.train_t,
            'sl_learning_rate': self._sl_learning_rate,
            'train_every': self._train_every,
        }

    @classmethod
    def from_checkpoint(cls, checkpoint):
        """Restore an agent from checkpoint_attributes(). The reference calls self._rl_agent.from_checkpoint(...) and
        throws its result away, which leaves a freshly initialised inner DQN; here the result is assigned, so the
        inner DQN comes back with its Q-network, memory and counters (total_t, train_t)."""
        pn = checkpoint['policy_network']
        agent = cls(anticipatory_param=checkpoint['anticipatory_param'], batch_size=checkpoint['batch_size'],
                    min_buffer_size_to_learn=checkpoint['min_buffer_size_to_learn'],
                    num_actions=checkpoint['num_actions'], sl_learning_rate=checkpoint['sl_learning_rate'],
                    train_every=checkpoint['train_every'], evaluate_with=checkpoint['evaluate_with'],
                    device=checkpoint['device'], q_mlp_layers=checkpoint['rl_agent']['q_estimator']['mlp_layers'],
                    state_shape=checkpoint['rl_agent']['q_estimator']['state_shape'],
                    hidden_layers_sizes=list(pn['mlp_layers'])[:-1],
                    reservoir_buffer_capacity=checkpoint['reservoir_buffer']['reservoir_buffer_capacity'])
        agent.policy_network = AveragePolicyNetwork.from_checkpoint(pn).to(agent.device)
        agent.policy_network.eval()
        agent._reservoir_buffer = ReservoirBuffer.from_checkpoint(checkpoint['reservoir_buffer'])
        agent._mode = checkpoint['mode']
        agent.total_t = checkpoint['total_t']
        agent.train_t = checkpoint['train_t']
        agent.policy_network_optimizer = torch.optim.Adam(agent.policy_network.parameters(),
                                                          lr=agent._sl_learning_rate)
        agent.policy_network_optimizer.load_state_dict(checkpoint['policy_network_optimizer'])
        agent._rl_agent = DQNAgent.from_checkpoint(checkpoint['rl_agent'])
        agent._rl_agent.set_device(agent.device)
        return agent

    def save_checkpoint(self, path, filename='checkpoint_nfsp.pt'):
        torch.save(self.checkpoint_attributes(), os.path.join(path, filename))


class NFSPCollector(DQNCollector):
    """DQNCollector's acting loop for an NFSPAgent: the mode of every step's acting seat is recorded next to the
    trajectory (mode_rows uint8 [T][N], what feed_vec takes), and the modes of an env's seats are drawn again where a
    game has just ended, because that env's next step starts a new game. The agent may hold every seat: self-play with
    one pair of networks, a mode per (env, seat)."""

    def __init__(self, vec, agent, seats=(0,), opponents='random', steps_per_feed=64, seed=0):
        super().__init__(vec, agent, seats, opponents, steps_per_feed, seed)
        self.mode_rows = torch.zeros((self.steps, vec.num_envs), dtype=torch.uint8, device=vec.device)
        agent.sample_episode_policy_vec(None, -1, self.seed)

    def _agent_actions(self, k, state):
        m = self.agent.mode_rows(state)
        self.mode_rows[k].copy_(m)
        return self.agent.step_vec(state, self.t, self.seed, mode_rows=m)

    def _stepped(self, state):
        self.agent.sample_episode_policy_vec(state['done'], self.t, self.seed)

    def run(self, train_steps=None, sl_steps=None, fused=False):
        """collect() + agent.feed_vec -> (the DQN losses, the average-policy losses)."""
        return self.agent.feed_vec(self.collect(), self.mode_rows, self.seats, train_steps, sl_steps, fused)
