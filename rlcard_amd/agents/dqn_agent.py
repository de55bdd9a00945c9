"""DQN (Double DQN with a target network and a replay memory), the agent of the reference's examples/run_rl.py.

* EstimatorNetwork / Estimator / Memory / DQNAgent -- the API and the torch module layout of
  rlcard/agents/dqn_agent.py (`fc_layers` = Flatten, BatchNorm1d, Linear/Tanh ..., Linear, so a reference state_dict
  loads unchanged), used one state at a time through rlcard_amd.make(...).run() and utils.reorganize.
* The vectorised path, for every env of a VecEnv at once (include/cardsim.h, rlcard_amd/csrc/cs_dqn.hip):
    Estimator.folded()   the network as the kernels take it: eval-mode BatchNorm folded into the first Linear
    DQNAgent.step_vec / eval_step_vec   cs_qnet_actions: Q-values, legal mask, argmax and the epsilon draw in one kernel
    DeviceMemory         cs_replay: the replay FIFO in HBM, filled from rollout-layout trajectories (reorganize on the
                         device, with the transitions that straddle two windows carried, not dropped)
    DQNAgent.feed_vec / train   targets from cs_dqn_targets; forward / backward / Adam stay torch
    DQNAgent.train_fused cs_dqn_train: whole train steps on the device, many per launch (feed_vec(..., fused=True))
    DQNCollector         the acting loop (the DMCActor pattern): the agent's seats by step_vec, the others by an engine
                         policy, recorded into a trajectory with final observations
"""
import ctypes as C
import os
import random
from copy import deepcopy

import numpy as np
import torch
from torch import nn

from .. import _abi
from .._abi import ptr as _ptr


def descriptor(wb, device):
    """[(W, b)] per Linear (float64 numpy, BatchNorm folded) -> the cs_qnet descriptor (_abi.QNet): float32 tensors on
    `device`, kept alive by the descriptor's `tensors`."""
    if not 1 <= len(wb) - 1 <= 4:
        raise ValueError('the Q-network kernels take 1..4 hidden layers, got %d' % (len(wb) - 1))
    net = _abi.QNet()
    net.in_dim = wb[0][0].shape[1]
    net.num_hidden = len(wb) - 1
    net.num_actions = wb[-1][0].shape[0]
    net.tensors = []
    for k, (W, b) in enumerate(wb):
        if k < net.num_hidden:
            net.hidden[k] = W.shape[0]
        Wt = torch.from_numpy(np.ascontiguousarray(W, dtype=np.float32)).to(device)
        bt = torch.from_numpy(np.ascontiguousarray(b, dtype=np.float32)).to(device)
        net.tensors += [Wt, bt]
        net.W[k], net.b[k] = Wt.data_ptr(), bt.data_ptr()
    return net


def fold_batchnorm(bn, linears, weights32=False):
    """[(W, b)] per Linear as float64 numpy, the eval-mode BatchNorm1d `bn` folded into the first: with s = gamma /
    sqrt(running_var + eps) and c = beta - running_mean * s, BatchNorm is x * s + c, so W0' = W0 * s (per input
    column) and b0' = b0 + W0 . c. weights32 (the device descriptors): the running mean's share of b0' is taken with W0'
    as float32 will hold it, b0' = b0 + W0 . beta - fl32(W0') . running_mean, so that the kernel's sum is fl32(W0') .
    (x - running_mean) + ...: a weight's rounding then counts by how far its feature is from its mean, not by the
    feature (a trained UNO net has scales s of up to 316 on features that hardly ever leave their mean)."""
    f64 = lambda t: t.detach().cpu().numpy().astype(np.float64)   # noqa: E731
    s = f64(bn.weight) / np.sqrt(f64(bn.running_var) + bn.eps)
    c = f64(bn.bias) - f64(bn.running_mean) * s
    out = [(f64(m.weight), f64(m.bias)) for m in linears]
    W0, b0 = out[0]
    Wf = W0 * s[None, :]
    if weights32:
        out[0] = (Wf, b0 + W0 @ f64(bn.bias) - Wf.astype(np.float32).astype(np.float64) @ f64(bn.running_mean))
    else:
        out[0] = (Wf, b0 + W0 @ c)
    return out


class EstimatorNetwork(nn.Module):
    """Flatten -> BatchNorm1d -> (Linear -> Tanh) per entry of mlp_layers -> Linear to num_actions."""

    def __init__(self, num_actions=2, state_shape=None, mlp_layers=None):
        super().__init__()
        self.num_actions = num_actions
        self.state_shape = state_shape
        self.mlp_layers = mlp_layers
        dims = [int(np.prod(state_shape))] + [int(w) for w in mlp_layers]
        fc = [nn.Flatten(), nn.BatchNorm1d(dims[0])]
        for i, o in zip(dims[:-1], dims[1:]):
            fc += [nn.Linear(i, o, bias=True), nn.Tanh()]
        fc.append(nn.Linear(dims[-1], num_actions, bias=True))
        self.fc_layers = nn.Sequential(*fc)

    def forward(self, s):
        return self.fc_layers(s)


class Estimator:
    """The Q-network with its Adam optimizer and MSE loss. Arrays in and out are numpy (torch tensors on the
    estimator's device are taken as they are)."""

    def __init__(self, num_actions=2, learning_rate=0.001, state_shape=None, mlp_layers=None, device=None):
        self.num_actions = num_actions
        self.learning_rate = learning_rate
        self.state_shape = state_shape
        self.mlp_layers = mlp_layers
        self.device = device
        self.qnet = EstimatorNetwork(num_actions, state_shape, mlp_layers).to(device)
        self.qnet.eval()
        for p in self.qnet.parameters():
            if p.dim() > 1:
                nn.init.xavier_uniform_(p.data)
        self.mse_loss = nn.MSELoss(reduction='mean')
        self.optimizer = torch.optim.Adam(self.qnet.parameters(), lr=self.learning_rate)
        self._folded = None

    def _tensor(self, x, dtype):
        if not torch.is_tensor(x):
            x = torch.from_numpy(np.asarray(x))
        return x.to(device=self.device, dtype=dtype)

    def predict_nograd(self, s):
        """Q-values [batch, num_actions] of states s, outside the graph (numpy in -> numpy out)."""
        with torch.no_grad():
            q = self.qnet(self._tensor(s, torch.float32))
        return q if torch.is_tensor(s) else q.cpu().numpy()

    def update(self, s, a, y):
        """One Adam step on the MSE between Q(s)[a] and the targets y -> the batch loss."""
        self.optimizer.zero_grad()
        self.qnet.train()
        q = self.qnet(self._tensor(s, torch.float32))
        Q = torch.gather(q, dim=-1, index=self._tensor(a, torch.long).unsqueeze(-1)).squeeze(-1)
        loss = self.mse_loss(Q, self._tensor(y, torch.float32))
        loss.backward()
        self.optimizer.step()
        self.qnet.eval()
        self._folded = None
        return loss.item()

    def load_state_dict(self, state_dict):
        r = self.qnet.load_state_dict(state_dict)
        self._folded = None
        return r

    # -- the network as the kernels take it --------------------------------------------------------------------------
    def folded_weights(self):
        """[(W, b)] per Linear as float64 numpy, the eval-mode BatchNorm folded into the first: with s = gamma /
        sqrt(running_var + eps) and c = beta - running_mean * s, BatchNorm is x * s + c, so W0' = W0 * s (per input
        column) and b0' = b0 + W0 . c."""
        return fold_batchnorm(self.qnet.fc_layers[1], [m for m in self.qnet.fc_layers if isinstance(m, nn.Linear)])

    def _version(self):
        return tuple(t._version for t in self.qnet.state_dict().values()) + (str(self.device),)

    def folded(self):
        """The cs_qnet descriptor (_abi.QNet) of this network: folded_weights() as float32 tensors on the estimator's
        device (kept alive by the descriptor's `tensors`), the first bias folded around those float32 weights
        (fold_batchnorm's weights32). Cached; update(), load_state_dict() and any in-place change of the parameters
        invalidate it."""
        ver = self._version()
        if self._folded is not None and self._folded[0] == ver:
            return self._folded[1]
        net = descriptor(fold_batchnorm(self.qnet.fc_layers[1],
                                        [m for m in self.qnet.fc_layers if isinstance(m, nn.Linear)], weights32=True),
                         self.device)
        self._folded = (ver, net)
        return net

    # -- checkpoints ---------------------------------------------------------------------------------------------------
    def checkpoint_attributes(self):
        return {'qnet': self.qnet.state_dict(), 'optimizer': self.optimizer.state_dict(),
                'num_actions': self.num_actions, 'learning_rate': self.learning_rate,
                'state_shape': self.state_shape, 'mlp_layers': self.mlp_layers, 'device': self.device}

    @classmethod
    def from_checkpoint(cls, checkpoint):
        est = cls(num_actions=checkpoint['num_actions'], learning_rate=checkpoint['learning_rate'],
                  state_shape=checkpoint['state_shape'], mlp_layers=checkpoint['mlp_layers'],
                  device=checkpoint['device'])
        est.load_state_dict(checkpoint['qnet'])
        if checkpoint.get('optimizer') is not None:
            est.optimizer.load_state_dict(checkpoint['optimizer'])
        return est


class Memory:
    """The host replay memory: a FIFO list of (state, action, reward, next_state, done, legal_actions)."""

    def __init__(self, memory_size, batch_size):
        self.memory_size = memory_size
        self.batch_size = batch_size
        self.memory = []

    def __len__(self):
        return len(self.memory)

    def save(self, state, action, reward, next_state, legal_actions, done):
        if len(self.memory) == self.memory_size:
            self.memory.pop(0)
        self.memory.append((state, action, reward, next_state, done, legal_actions))

    def sample(self):
        """batch_size distinct transitions (random.sample) -> state, action, reward, next_state, done arrays and the
        tuple of the next states' legal-action lists."""
        cols = tuple(zip(*random.sample(self.memory, self.batch_size)))
        return tuple(np.array(c) for c in cols[:-1]) + (cols[-1],)

    def checkpoint_attributes(self):
        return {'memory_size': self.memory_size, 'batch_size': self.batch_size, 'memory': self.memory}

    @classmethod
    def from_checkpoint(cls, checkpoint):
        m = cls(checkpoint['memory_size'], checkpoint['batch_size'])
        m.memory = checkpoint['memory']
        return m


def seat_mask(seats):
    m = 0
    for p in seats:
        m |= 1 << int(p)
    return m


class DeviceBuffer(_abi.Handle):
    """What the buffers of a VecEnv's envs in HBM share (DeviceMemory, nfsp_agent.DeviceReservoir): the two counters
    of cs_<KIND>_size, the index tensor of gather() and sampling without replacement."""
    KIND = None          # 'replay' / 'reservoir'
    TOO_MANY = None      # sample()'s ValueError text for (asked, held)

    def _call(self, what, *args):
        """cs_<KIND>_<what>(buffer, *args) with the env's device current"""
        return _abi.call('cs_%s_%s' % (self.KIND, what), self._h, *args, device=self.vec.device)

    def sizes(self):
        """(elements held, elements ever appended or offered); synchronises."""
        size, total = C.c_int64(), C.c_int64()
        self._call('size', C.byref(size), C.byref(total))
        return size.value, total.value

    def __len__(self):
        return self.sizes()[0]

    def _indices(self, idx):
        """gather's idx as a flat int64 tensor on the env's device, and its length"""
        idx = torch.as_tensor(idx, device=self.vec.device).to(torch.int64).contiguous().reshape(-1)
        return idx, int(idx.numel())

    def sample(self, count, generator=None):
        """count distinct elements, uniformly (what random.sample gives the host buffers' sample), drawn from a
        torch.Generator (None: torch's global one)."""
        size = len(self)
        if count > size:
            raise ValueError(self.TOO_MANY % (count, size))
        dev = generator.device if generator is not None else 'cpu'
        return self.gather(torch.randperm(size, generator=generator, device=dev)[:count])


class DeviceMemory(DeviceBuffer):
    """The replay memory of a VecEnv's envs in HBM (include/cardsim.h cs_replay): push() turns a rollout-layout
    trajectory into transitions on the device, in the FIFO order the header documents; index k is the k-th oldest
    transition held, as in Memory's list."""
    KIND, TOO_MANY = 'replay', 'sample larger than the memory: %d > %d'

    def __init__(self, vec, capacity):
        self.vec, self.capacity = vec, int(capacity)
        self.create('cs_replay_create', vec._h, self.capacity, device=vec.device)

    def push(self, traj, seats):
        """Append the transitions of the seats `seats` of a trajectory ([T][N] rows with final_obs: VecEnv.rollout(...,
        final_obs=True) or DQNCollector's)."""
        T = traj['player'].shape[0]
        s = _abi.traj(traj, 'obs', 'legal', 'player', 'action', 'reward', 'done', 'final_obs')
        self._call('push', int(T), C.byref(s), seat_mask(seats), self.vec._stream())

    def drop_pending(self):
        """Forget the transitions waiting for their next state (after vec.reset() or a re-seed: their games are
        gone)."""
        self._call('drop_pending', self.vec._stream())

    @property
    def total(self):
        return self.sizes()[1]

    def gather(self, idx):
        """Transitions idx (int64, each in [0, len(self))) -> dict of device tensors: state / next_state float32
        [B, obs_dim], action int64 [B], reward float32 [B], next_legal uint8 [B, legal_bytes], done uint8 [B]."""
        v, d = self.vec, self.vec.device
        idx, B = self._indices(idx)
        out = dict(state=torch.empty((B, v.obs_dim), dtype=torch.float32, device=d),
                   action=torch.empty(B, dtype=torch.int64, device=d),
                   reward=torch.empty(B, dtype=torch.float32, device=d),
                   next_state=torch.empty((B, v.obs_dim), dtype=torch.float32, device=d),
                   next_legal=torch.empty((B, v.legal_bytes), dtype=torch.uint8, device=d),
                   done=torch.empty(B, dtype=torch.uint8, device=d))
        if B:
            b = _abi.ReplayBatch(*(_ptr(out[k]) for k in ('state', 'action', 'reward', 'next_state', 'next_legal',
                                                          'done')))
            self._call('gather', _ptr(idx), B, C.byref(b), v._stream())
        return out


def dqn_targets(q_next, q_next_target, next_legal, reward, done, gamma):
    """Double-DQN targets on the device (cs_dqn_targets) -> (target float32 [B], best int32 [B])."""
    d = q_next.device
    B, A = q_next.shape
    target = torch.empty(B, dtype=torch.float32, device=d)
    best = torch.empty(B, dtype=torch.int32, device=d)
    if B:
        _abi.call('cs_dqn_targets', _ptr(q_next.contiguous()), _ptr(q_next_target.contiguous()),
                  _ptr(next_legal.contiguous()), _ptr(reward.contiguous()), _ptr(done.contiguous()), B, A, float(gamma),
                  _ptr(target), _ptr(best), _abi.stream(d), device=d)
    return target, best


FUSED_MAX_STEPS = 4096   # train steps of one cs_dqn_train launch


class DQNAgent:
    """rlcard's DQNAgent (constructor arguments and methods), plus attach() and the *_vec methods for a VecEnv."""

    def __init__(self, replay_memory_size=20000, replay_memory_init_size=100, update_target_estimator_every=1000,
                 discount_factor=0.99, epsilon_start=1.0, epsilon_end=0.1, epsilon_decay_steps=20000, batch_size=32,
                 num_actions=2, state_shape=None, train_every=1, mlp_layers=None, learning_rate=0.00005, device=None,
                 save_path=None, save_every=float('inf')):
        self.use_raw = False
        self.replay_memory_init_size = replay_memory_init_size
        self.update_target_estimator_every = update_target_estimator_every
        self.discount_factor = discount_factor
        self.epsilon_decay_steps = epsilon_decay_steps
        self.batch_size = batch_size
        self.num_actions = num_actions
        self.train_every = train_every
        if device is None:
            device = torch.device('cuda:0' if torch.cuda.is_available() else 'cpu')
        self.device = device
        self.total_t = 0    # transitions fed
        self.train_t = 0    # train() calls
        self.epsilons = np.linspace(epsilon_start, epsilon_end, epsilon_decay_steps)
        kw = dict(num_actions=num_actions, learning_rate=learning_rate, state_shape=state_shape,
                  mlp_layers=mlp_layers, device=self.device)
        self.q_estimator = Estimator(**kw)
        self.target_estimator = Estimator(**kw)
        self.memory = Memory(replay_memory_size, batch_size)
        self.device_memory = None
        self.vec = None
        self.generator = None    # torch.Generator of DeviceMemory.sample (None: torch's global one)
        self.last_loss = None
        self.train_seed = 0      # key of train_fused's sampler (the draws are keyed by (train_seed, train_t))
        self.save_path = save_path
        self.save_every = save_every

    # -- one state at a time (the reference's API) ---------------------------------------------------------------------
    def feed(self, ts):
        """Store one transition [state, action, reward, next_state, done]; past the first replay_memory_init_size
        transitions, train every train_every of them."""
        state, action, reward, next_state, done = tuple(ts)
        self.feed_memory(state['obs'], action, reward, next_state['obs'], list(next_state['legal_actions'].keys()),
                         done)
        self.total_t += 1
        tmp = self.total_t - self.replay_memory_init_size
        if tmp >= 0 and tmp % self.train_every == 0:
            self.train()

    def epsilon(self):
        return float(self.epsilons[min(self.total_t, self.epsilon_decay_steps - 1)])

    def step(self, state):
        """Epsilon-greedy action for training: eps / len(legal) on every legal action, the rest on the best one."""
        q = self.predict(state)
        eps = self.epsilon()
        legal = list(state['legal_actions'].keys())
        probs = np.full(len(legal), eps / len(legal), dtype=float)
        probs[legal.index(int(np.argmax(q)))] += 1.0 - eps
        return legal[np.random.choice(len(probs), p=probs)]

    def eval_step(self, state):
        q = self.predict(state)
        legal = list(state['legal_actions'].keys())
        info = {'values': {state['raw_legal_actions'][i]: float(q[legal[i]]) for i in range(len(legal))}}
        return np.argmax(q), info

    def predict(self, state):
        """Q-values of one state as float64 [num_actions], -inf where the action is illegal."""
        q = self.q_estimator.predict_nograd(np.expand_dims(state['obs'], 0))[0]
        masked = np.full(self.num_actions, -np.inf, dtype=float)
        legal = list(state['legal_actions'].keys())
        masked[legal] = q[legal]
        return masked

    def train(self):
        """One Double-DQN step on a sampled batch -> the loss. With a device memory attached the batch is sampled and
        the targets are computed on the device."""
        if self.device_memory is not None:
            b = self.device_memory.sample(self.batch_size, self.generator)
            q_next = self.q_estimator.predict_nograd(b['next_state'])
            q_next_target = self.target_estimator.predict_nograd(b['next_state'])
            target, _ = dqn_targets(q_next, q_next_target, b['next_legal'], b['reward'], b['done'],
                                    self.discount_factor)
            loss = self.q_estimator.update(b['state'], b['action'], target)
        else:
            state, action, reward, next_state, done, legal = self.memory.sample()
            B = len(action)
            q_next = self.q_estimator.predict_nograd(next_state)
            masked = np.full((B, self.num_actions), -np.inf, dtype=float)
            for k in range(B):
                masked[k, list(legal[k])] = q_next[k, list(legal[k])]
            best = np.argmax(masked, axis=1)
            q_next_target = self.target_estimator.predict_nograd(next_state)
            target = reward + np.invert(done).astype(np.float32) * self.discount_factor * \
                q_next_target[np.arange(B), best]
            loss = self.q_estimator.update(np.array(state), action, target)
        self.last_loss = loss
        if self.train_t % self.update_target_estimator_every == 0:
            self.target_estimator = deepcopy(self.q_estimator)
        self.train_t += 1
        if self.save_path and self.train_t % self.save_every == 0:
            self.save_checkpoint(self.save_path)
        return loss

    def feed_memory(self, state, action, reward, next_state, legal_actions, done):
        self.memory.save(state, action, reward, next_state, legal_actions, done)

    def set_device(self, device):
        self.device = device
        for est in (self.q_estimator, self.target_estimator):
            est.device = device
            est.qnet.to(device)
            est._folded = None

    # -- every env of a VecEnv at once ---------------------------------------------------------------------------------
    def attach(self, vec, replay_memory_size=None):
        """Use `vec`'s device: the estimators move there and the replay memory becomes a DeviceMemory of
        replay_memory_size transitions (default: the host memory's size)."""
        self.vec = vec
        self.set_device(vec.device)
        # (Adam's state follows its parameters; a fresh optimizer is only needed when it already held CPU state)
        for est in (self.q_estimator, self.target_estimator):
            for st in est.optimizer.state.values():
                for k, x in st.items():
                    if torch.is_tensor(x):
                        st[k] = x.to(vec.device)
        cap = int(replay_memory_size if replay_memory_size is not None else self.memory.memory_size)
        self.device_memory = DeviceMemory(vec, cap)
        return self.device_memory

    def _actions_vec(self, state, eps, t, seed, q=None):
        v = self.vec
        if v is None:
            raise _abi.CardsimError('DQNAgent.attach(vec) comes before the *_vec methods')
        net = self.q_estimator.folded()
        obs, legal, done = state['obs'], state['legal'], state.get('done')
        rows = obs.shape[0]
        out = torch.empty(rows, dtype=torch.int32, device=v.device)
        _abi.call('cs_qnet_actions', v._h, C.byref(net), _ptr(obs), _ptr(legal), _ptr(done), rows, float(eps),
                  int(seed) & (2 ** 64 - 1), int(t), v.env_base, _ptr(out), _ptr(q), v._stream(), device=v.device)
        return out

    def step_vec(self, state, t, seed=0):
        """DQNAgent.step for every env of a step output `state` (obs, legal, done): int32 [N] actions, -1 where the
        env's game is over. Epsilon comes from the schedule at total_t; the draw is keyed by (seed, env, t)."""
        return self._actions_vec(state, self.epsilon(), t, seed)

    def eval_step_vec(self, state, t=0, seed=0):
        """DQNAgent.eval_step for every env: the greedy action (t and seed are unused: nothing is drawn)."""
        return self._actions_vec(state, 0.0, t, seed)

    def predict_vec(self, obs, legal=None):
        """DQNAgent.predict for rows of observations (cs_qnet_values): float32 [rows, num_actions], -inf where
        illegal."""
        v = self.vec
        net = self.q_estimator.folded()
        q = torch.empty((obs.shape[0], self.num_actions), dtype=torch.float32, device=v.device)
        _abi.call('cs_qnet_values', v._h, C.byref(net), _ptr(obs), _ptr(legal), obs.shape[0], _ptr(q), v._stream(),
                  device=v.device)
        return q

    def train_steps_for(self, t0, t1):
        """train() calls the reference's feed makes while total_t goes from t0 to t1."""
        first = max(t0 + 1, self.replay_memory_init_size)
        if first > t1:
            return 0
        e = self.train_every
        first += (-(first - self.replay_memory_init_size)) % e
        return 0 if first > t1 else (t1 - first) // e + 1

    def feed_vec(self, traj, seats, train_steps=None, fused=False):
        """Push the seats' transitions of a trajectory into the device memory, advance total_t by the number
        appended, and train as often as feed would have over that advance (or exactly train_steps times) -> the
        losses. fused: the steps run on the device (train_fused, in launches of at most FUSED_MAX_STEPS), and the
        losses come back as one float32 device tensor."""
        mem = self.device_memory
        before = mem.total
        mem.push(traj, seats)
        fresh = mem.total - before
        t0 = self.total_t
        self.total_t += fresh
        n = self.train_steps_for(t0, self.total_t) if train_steps is None else int(train_steps)
        if not fused:
            return [self.train() for _ in range(n)]
        losses = [self.train_fused(min(FUSED_MAX_STEPS, n - k)) for k in range(0, n, FUSED_MAX_STEPS)]
        return torch.cat(losses) if losses else torch.empty(0, dtype=torch.float32, device=self.device)

    # -- the learner on the device -------------------------------------------------------------------------------------
    def _adam_state(self):
        """The Q-network's optimizer as cs_dqn_train takes it: (the param group, the state dict per parameter in
        parameters() order), the state created as Adam's first step would create it where there is none yet."""
        opt = self.q_estimator.optimizer
        if type(opt) is not torch.optim.Adam or len(opt.param_groups) != 1:
            raise ValueError('train_fused takes torch.optim.Adam with one parameter group, got %s' % type(opt).__name__)
        g = opt.param_groups[0]
        for flag in ('weight_decay', 'amsgrad', 'maximize', 'capturable', 'fused'):
            if g.get(flag):
                raise ValueError('train_fused takes plain Adam: %s=%r is not supported' % (flag, g[flag]))
        states = []
        for p in self.q_estimator.qnet.parameters():
            st = opt.state[p]
            if len(st) == 0:
                st['step'] = torch.zeros((), dtype=torch.float32, device='cpu')
                st['exp_avg'] = torch.zeros_like(p, memory_format=torch.preserve_format)
                st['exp_avg_sq'] = torch.zeros_like(p, memory_format=torch.preserve_format)
            states.append(st)
        return g, states

    @staticmethod
    def _dqn_net(est, keep):
        """cs_dqn_net of an Estimator's network (the tensors are torch's own; `keep` holds them past the call)"""
        fc = est.qnet.fc_layers
        bn, linears = fc[1], [m for m in fc if isinstance(m, nn.Linear)]
        if not 1 <= len(linears) - 1 <= 4:
            raise ValueError('the train kernel takes 1..4 hidden layers, got %d' % (len(linears) - 1))
        if bn.momentum is None or not bn.affine or not bn.track_running_stats:
            raise ValueError('train_fused takes an affine BatchNorm1d with running statistics and a momentum')
        net = _abi.DqnNet()
        net.in_dim, net.num_hidden, net.num_actions = bn.num_features, len(linears) - 1, linears[-1].out_features
        tensors = [bn.weight, bn.bias, bn.running_mean, bn.running_var, bn.num_batches_tracked]
        net.bn_weight, net.bn_bias, net.bn_mean, net.bn_var, net.bn_tracked = (t.data_ptr() for t in tensors)
        net.bn_eps, net.bn_momentum = bn.eps, bn.momentum
        for k, m in enumerate(linears):
            if k < net.num_hidden:
                net.hidden[k] = m.out_features
            net.W[k], net.b[k] = m.weight.data_ptr(), m.bias.data_ptr()
            tensors += [m.weight, m.bias]
        for t in tensors:
            if not t.is_cuda or t.device != bn.weight.device or not t.is_contiguous() or \
                    t.dtype != (torch.int64 if t is bn.num_batches_tracked else torch.float32):
                raise ValueError('train_fused takes contiguous float32 parameters on the env\'s device')
        keep += tensors
        return net

    def train_fused(self, steps, idx=None, debug=False):
        """`steps` train() calls in one kernel launch (cs_dqn_train: sampling, targets, forward, backward and Adam of
        every step on the device, in place on the networks' and the optimizer's tensors) -> the losses, a float32
        device tensor [steps]; nothing waits for the device. The batches are drawn by the kernel's own sampler, keyed by
        (train_seed, train_t), not by `generator`; idx (int64 [steps, batch_size]) gives them instead. debug: also the
        indices used (int64 [steps, B]), the targets (float32 [steps, B]) and the last step's gradients (float32, flat,
        in qnet.parameters() order)."""
        if self.device_memory is None or self.vec is None:
            raise _abi.CardsimError('DQNAgent.attach(vec) comes before train_fused')
        steps, B = int(steps), int(self.batch_size)
        group, states = self._adam_state()
        keep = []
        qnet = self._dqn_net(self.q_estimator, keep)
        tnet = self._dqn_net(self.target_estimator, keep)
        d = keep[0].device
        ad = _abi.DqnAdam()
        names = [('bn_weight', None), ('bn_bias', None)] + [(w, k) for k in range(qnet.num_hidden + 1)
                                                            for w in ('W', 'b')]
        for (name, k), st in zip(names, states):
            m, v = st['exp_avg'], st['exp_avg_sq']
            if m.device != d or not m.is_contiguous() or not v.is_contiguous():
                raise ValueError('train_fused: Adam\'s state is not on the env\'s device')
            if k is None:
                setattr(ad, name + '_m', m.data_ptr())
                setattr(ad, name + '_v', v.data_ptr())
            else:
                getattr(ad, name + '_m')[k] = m.data_ptr()
                getattr(ad, name + '_v')[k] = v.data_ptr()
        ad.lr, ad.eps = float(group['lr']), float(group['eps'])
        ad.beta1, ad.beta2 = (float(x) for x in group['betas'])
        ad.step0 = int(float(states[0]['step']))
        args = _abi.DqnTrainArgs()
        args.K, args.B, args.gamma = steps, B, float(self.discount_factor)
        args.seed, args.train_t0 = int(self.train_seed) & (2 ** 64 - 1), int(self.train_t)
        every = self.update_target_estimator_every
        args.target_every = int(every) if every and every != float('inf') else 0
        loss = torch.empty(max(steps, 0), dtype=torch.float32, device=d)
        out = None
        if idx is not None:
            idx = torch.as_tensor(idx, device=d).to(torch.int64).contiguous()
            if tuple(idx.shape) != (steps, B):
                raise ValueError('train_fused: idx must be [steps, batch_size]')
            args.idx = idx.data_ptr()
        if debug:
            n_par = sum(p.numel() for p in self.q_estimator.qnet.parameters())
            out = (torch.empty((max(steps, 0), B), dtype=torch.int64, device=d),
                   torch.empty((max(steps, 0), B), dtype=torch.float32, device=d),
                   torch.empty(n_par, dtype=torch.float32, device=d))
            args.idx_out, args.target_out, args.grads = (t.data_ptr() for t in out)
        args.loss = loss.data_ptr()
        _abi.call('cs_dqn_train', self.device_memory._h, C.byref(qnet), C.byref(tnet), C.byref(ad), C.byref(args),
                  self.vec._stream(), device=d)
        # the kernel wrote behind torch's version counters: the host-side counters and caches follow by hand
        for st in states:
            st['step'] += steps
        before = self.train_t
        self.train_t += steps
        self.q_estimator._folded = None
        self.target_estimator._folded = None
        self.last_loss = loss[-1]
        if self.save_path and self.train_t // self.save_every != before // self.save_every:
            self.save_checkpoint(self.save_path)
        return (loss,) + out if debug else loss

    # -- checkpoints ---------------------------------------------------------------------------------------------------
    def checkpoint_attributes(self):
        return {
            'agent_type': 'DQNAgent',
            'q_estimator': self.q_estimator.checkpoint_attributes(),
            'memory': self.memory.checkpoint_attributes(),
            'total_t': self.total_t,
            'train_t': self.train_t,
            'replay_memory_init_size': self.replay_memory_init_size,
            'update_target_estimator_every': self.update_target_estimator_every,
            'discount_factor': self.discount_factor,
            'epsilon_start': self.epsilons.min(),
            'epsilon_end': self.epsilons.max(),
            'epsilon_decay_steps': self.epsilon_decay_steps,
            'batch_size': self.batch_size,
            'num_actions': self.num_actions,
            'train_every': self.train_every,
            'device': self.device,
            'save_path': self.save_path,
            'save_every': self.save_every,
        }

    @classmethod
    def from_checkpoint(cls, checkpoint):
        q = checkpoint['q_estimator']
        agent = cls(replay_memory_size=checkpoint['memory']['memory_size'],
                    replay_memory_init_size=checkpoint['replay_memory_init_size'],
                    update_target_estimator_every=checkpoint['update_target_estimator_every'],
                    discount_factor=checkpoint['discount_factor'], epsilon_start=checkpoint['epsilon_start'],
                    epsilon_end=checkpoint['epsilon_end'], epsilon_decay_steps=checkpoint['epsilon_decay_steps'],
                    batch_size=checkpoint['batch_size'], num_actions=checkpoint['num_actions'],
                    state_shape=q['state_shape'], train_every=checkpoint['train_every'], mlp_layers=q['mlp_layers'],
                    learning_rate=q['learning_rate'], device=checkpoint['device'], save_path=checkpoint['save_path'],
                    save_every=checkpoint['save_every'])
        agent.total_t = checkpoint['total_t']
        agent.train_t = checkpoint['train_t']
        agent.q_estimator = Estimator.from_checkpoint(q)
        agent.target_estimator = deepcopy(agent.q_estimator)
        agent.memory = Memory.from_checkpoint(checkpoint['memory'])
        return agent

    def save_checkpoint(self, path, filename='checkpoint_dqn.pt'):
        torch.save(self.checkpoint_attributes(), os.path.join(path, filename))


class DQNCollector:
    """The acting loop of a DQNAgent on a VecEnv (the DMCActor pattern): each step, the envs whose acting seat is one
    of `seats` take the agent's step_vec action, the others `opponents`' (an engine policy name or id, or one per
    seat); collect() records steps_per_feed steps into a trajectory with final observations, run() also feeds it. A
    step on a finished game starts the next one (lazy auto-reset) and is not a transition (player 255). The opponents
    are VecEnv.policy_actions': games without engine policies (include/cardsim.h CS_POLICY_*) raise, unless the agent
    holds every seat."""

    def __init__(self, vec, agent, seats=(0,), opponents='random', steps_per_feed=64, seed=0):
        self.vec, self.agent, self.seats = vec, agent, tuple(int(p) for p in seats)
        if agent.vec is not vec:
            agent.attach(vec)
        P = vec.num_players
        self.opponents = list(opponents) if isinstance(opponents, (list, tuple)) else [opponents] * P
        self.steps, self.seed, self.t = int(steps_per_feed), int(seed), 0
        lut = torch.zeros(256, dtype=torch.bool)
        lut[list(self.seats)] = True
        self.mine = lut.to(vec.device)
        self.traj = vec.new_traj_out(self.steps, final_obs=True, select=1)
        self.state = vec.reset()
        agent.device_memory.drop_pending()
        self._obs = vec.new_step_out()

    def _opponent_actions(self, state):
        v = self.vec
        acts = None
        for pol in sorted(set(self.opponents[p] for p in range(v.num_players) if p not in self.seats), key=str):
            a = v.policy_actions(pol, self.seed, self.t)
            if acts is None:
                acts = a
            else:
                who = torch.tensor([self.opponents[p] == pol for p in range(v.num_players)], device=v.device)
                acts = torch.where(who[state['player'].long().clamp_max(v.num_players - 1)], a, acts)
        return acts

    def collect(self):
        """steps_per_feed env steps -> the trajectory ([T][N] rows with final_obs; reused by the next call)."""
        v, tr, st = self.vec, self.traj, self.state
        for k in range(self.steps):
            acts = self._agent_actions(k, st)
            opp = self._opponent_actions(st)
            if opp is not None:
                acts = torch.where(self.mine[st['player'].long()], acts, opp)
            over = st['done'].bool()
            tr['obs'][k].copy_(st['obs'])
            tr['legal'][k].copy_(st['legal'])
            tr['player'][k].copy_(torch.where(over, torch.full_like(st['player'], 255), st['player']))
            tr['action'][k].copy_(acts.clamp_min(0).to(tr['action'].dtype))
            st = v.step(acts)
            tr['reward'][k].copy_(st['reward'])
            tr['done'][k].copy_(st['done'])
            ended = st['done'].bool().unsqueeze(-1)
            for p in range(v.num_players):   # every seat's view of the finished games (Env.run's final states)
                tr['final_obs'][k, :, p].copy_(torch.where(ended, v.observe(p, self._obs)['obs'], 0))
            self._stepped(st)
            self.t += 1
        self.state = st
        return tr

    def _agent_actions(self, k, state):
        """the agent's actions for step k of the window"""
        return self.agent.step_vec(state, self.t, self.seed)

    def _stepped(self, state):
        """after every env step, with the state it led to (NFSPCollector resamples the finished games' modes)"""

    def run(self, train_steps=None, fused=False):
        """collect() + agent.feed_vec -> the losses of the train steps (fused: on the device, as a tensor)."""
        return self.agent.feed_vec(self.collect(), self.seats, train_steps, fused)
