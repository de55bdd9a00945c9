"""The fused DQN learner (rlcard_amd/csrc/cs_dqn_train.hip through cs_dqn_train and DQNAgent.train_fused): whole train
steps on the device against fp64 torch on the CPU on the same batch. Needs a GPU.

The bound used throughout is the project's (test_gpu_dqn.py, test_gpu_nfsp.py): with E_torch the error of fp32 torch on
the CPU against the fp64 reference, E_kernel <= 8 E_torch + 4 ulp of the tensor's largest reference magnitude, per
tensor."""
import numpy as np
import pytest

from test_dqn_train import floyd_batches

torch = pytest.importorskip('torch')
pytestmark = pytest.mark.gpu

GAMMA = 0.99
# name: (game, envs of the rollout that fills the memory, mlp_layers, batch size)
CASES = {'leduc': ('leduc-holdem', 256, [64, 64], 32),       # the default
         'odd': ('leduc-holdem', 65, [7, 5, 3, 2], 5),       # odd everything, four hidden layers, padded rows
         'b2': ('leduc-holdem', 65, [128], 2),               # the smallest batch, one wide layer
         'b64': ('leduc-holdem', 256, [64, 64], 64),         # the largest batch
         'uno': ('uno', 256, [128, 128], 32),                # byte obs of 240, 61 actions, 8 mask bytes
         'mahjong': ('mahjong', 65, [64], 32),               # 816 obs bytes: one column per thread, no output groups
         'widest': ('mahjong', 65, [128, 128, 128, 128], 64),   # the most LDS a game there is needs: 156 416 B
         # obs rows that are no whole dwords: the byte-wise gather and the first layer's scalar k loop
         'nolimit': ('no-limit-holdem', 256, [64, 64], 32),  # 54 obs bytes, 5 actions: 18 output groups, 972 threads
         'blackjack': ('blackjack', 256, [128], 32),         # 2 raw obs bytes up to about 30, 2 actions, one seat
         'limit': ('limit-holdem', 256, [20], 5)}            # 72 obs bytes in 14 uneven output groups, 8 padded rows
ALL = list(CASES)


@pytest.fixture(scope='module', autouse=True)
def _need_gpu():
    if not torch.cuda.is_available():
        pytest.fail('GPU tests need a visible GPU (run them on the MI355X box)')


_worlds = {}


def world(name):
    """The case's env and a 16-step random rollout with final observations, made once."""
    from rlcard_amd import VecEnv
    if name not in _worlds:
        game, n, mlp, B = CASES[name]
        v = VecEnv(game, n, seed=13)
        v.reset()
        traj = v.rollout(16, policy_seed=5, final_obs=True)
        _worlds[name] = dict(v=v, traj=traj, mlp=mlp, B=B, seats=tuple(range(v.num_players)))
    return _worlds[name]


def randomize(est, seed, bn_bias=True):
    """Seeded BatchNorm statistics and affine and Linear biases (test_gpu_dqn.random_estimator's), on the CPU."""
    g = torch.Generator().manual_seed(seed)
    bn = est.qnet.fc_layers[1]
    D = bn.num_features
    with torch.no_grad():
        bn.running_mean.copy_(torch.rand(D, generator=g) * 0.5)
        bn.running_var.copy_(torch.rand(D, generator=g) * 0.5 + 0.1)
        bn.weight.copy_(torch.rand(D, generator=g) + 0.5)
        bias = torch.rand(D, generator=g) - 0.5
        if bn_bias:
            bn.bias.copy_(bias)
        for m in est.qnet.fc_layers:
            if isinstance(m, torch.nn.Linear):
                m.bias.copy_(torch.rand(m.bias.shape, generator=g) - 0.5)


def new_agent(name, lr=1e-3, every=1000, adam='seeded', cap=8192, seed=7, bn_bias=True, push=True):
    """A seeded agent on the case's env with the case's rollout in its memory; two calls give identical agents.
    adam='seeded': non-trivial moments and step 2; 'fresh': no optimizer state yet."""
    from rlcard_amd.agents import DQNAgent
    w = world(name)
    v = w['v']
    torch.manual_seed(seed)
    agent = DQNAgent(num_actions=v.num_actions, state_shape=[v.obs_dim], mlp_layers=list(w['mlp']),
                     batch_size=w['B'], replay_memory_size=cap, update_target_estimator_every=every,
                     discount_factor=GAMMA, learning_rate=lr, device=torch.device('cpu'))
    randomize(agent.q_estimator, seed + 1, bn_bias)
    randomize(agent.target_estimator, seed + 2)
    agent.attach(v, cap)
    if push:
        agent.device_memory.push(w['traj'], w['seats'])
    if adam == 'seeded':
        g = torch.Generator().manual_seed(seed + 3)
        for st in agent._adam_state()[1]:
            st['exp_avg'].copy_(torch.randn(st['exp_avg'].shape, generator=g) * 1e-3)
            st['exp_avg_sq'].copy_(torch.rand(st['exp_avg_sq'].shape, generator=g) * 1e-5)
            st['step'].fill_(2)
    return agent


def state_of(est):
    return {k: t.detach().cpu().clone() for k, t in est.qnet.state_dict().items()}


def adam_of(agent):
    """[(exp_avg, exp_avg_sq)] on the CPU, in parameters() order"""
    opt = agent.q_estimator.optimizer
    return [(opt.state[p]['exp_avg'].cpu().clone(), opt.state[p]['exp_avg_sq'].cpu().clone())
            for p in agent.q_estimator.qnet.parameters()]


def everything(agent):
    """every tensor a train step may change, as a flat list of CPU tensors"""
    out = list(state_of(agent.q_estimator).values()) + list(state_of(agent.target_estimator).values())
    for m, v in adam_of(agent):
        out += [m, v]
    return out


def same(a, b):
    return len(a) == len(b) and all(torch.equal(x, y) for x, y in zip(a, b))


def twin(agent, state, dtype):
    """the EstimatorNetwork of `state` on the CPU in dtype"""
    from rlcard_amd.agents import EstimatorNetwork
    e = agent.q_estimator
    net = EstimatorNetwork(e.num_actions, e.state_shape, e.mlp_layers).to(dtype)
    net.load_state_dict(state)
    return net


def batch_of(agent, idx):
    b = agent.device_memory.gather(idx)
    return {k: x.cpu() for k, x in b.items()}


def ref_targets(agent, q_state, t_state, b, dtype):
    """train()'s target line on the CPU in dtype -> (y, q_next masked to -inf, best)"""
    A = agent.num_actions
    qn_net, qt_net = twin(agent, q_state, dtype).eval(), twin(agent, t_state, dtype).eval()
    with torch.no_grad():
        qn, qt = qn_net(b['next_state'].to(dtype)), qt_net(b['next_state'].to(dtype))
    m = torch.from_numpy(np.unpackbits(b['next_legal'].numpy(), axis=1, bitorder='little')[:, :A].astype(bool))
    masked = torch.where(m, qn, torch.full_like(qn, -np.inf))
    best = torch.where(m.any(dim=1), masked.argmax(dim=1), torch.zeros(len(m), dtype=torch.long))
    live = (1 - b['done'].to(dtype)) * torch.tensor(GAMMA, dtype=dtype)
    y = b['reward'].to(dtype) + live * qt[torch.arange(len(best)), best]
    return y, masked, best, m


def ulp4(ref):
    return 4 * float(np.spacing(np.float32(np.abs(np.asarray(ref, np.float64)).max())))


def check_bound(got, ref64, ref32, what):
    got, ref64, ref32 = (np.asarray(x, np.float64) for x in (got, ref64, ref32))
    e_t, e_k = np.abs(ref32 - ref64).max(), np.abs(got - ref64).max()
    tol = 8 * e_t + ulp4(ref64)
    print('%s: E_torch %.3e E_kernel %.3e bound %.3e max|ref| %.3e' % (what, e_t, e_k, tol, np.abs(ref64).max()))
    assert np.isfinite(got).all(), what
    assert e_k <= tol, what


# ---- 1. sampler ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('name', ['leduc', 'odd', 'b2', 'b64'])
def test_sampler_is_the_restatement(name):
    agent = new_agent(name)
    size, B = len(agent.device_memory), agent.batch_size
    assert size > 200
    agent.train_seed, agent.train_t = 2 ** 40 + 3, 77
    _, idx, _, _ = agent.train_fused(6, debug=True)
    want = floyd_batches(2 ** 40 + 3, np.arange(77, 83), size, B)
    assert np.array_equal(idx.cpu().numpy(), want)
    assert agent.train_t == 83
    _, idx2, _, _ = agent.train_fused(1, debug=True)         # the next launch goes on at train_t 83
    assert np.array_equal(idx2.cpu().numpy(), floyd_batches(2 ** 40 + 3, [83], size, B))
    given = torch.from_numpy(want[::-1].copy())              # given indices are used as they are
    _, idx3, _, _ = agent.train_fused(6, idx=given, debug=True)
    assert np.array_equal(idx3.cpu().numpy(), want[::-1])


def test_sampler_draws_a_full_memory_whole():
    agent = new_agent('leduc', cap=32)
    assert len(agent.device_memory) == 32
    _, idx, _, _ = agent.train_fused(3, debug=True)
    assert np.array_equal(np.sort(idx.cpu().numpy(), axis=1), np.tile(np.arange(32), (3, 1)))
    assert np.array_equal(idx.cpu().numpy(), floyd_batches(0, np.arange(3), 32, 32))


# ---- 2. targets ------------------------------------------------------------------------------------------------------
def check_targets(agent, name, both_done=False):
    """target_out of a launch's first step (the networks as they were before it) against the fp64 eval forwards and
    the target line. Every row of the seeded cases is clear: the fp64 top-two gap of q_next over the legal actions
    exceeds 16 E_torch (rows with fewer than two legal actions have nothing to confuse). -> the two steps' indices"""
    agent.train_t = 5
    q_state, t_state = state_of(agent.q_estimator), state_of(agent.target_estimator)
    _, idx, y, _ = agent.train_fused(2, debug=True)
    b = batch_of(agent, idx[0])
    y64, masked64, best64, m = ref_targets(agent, q_state, t_state, b, torch.float64)
    y32, masked32, best32, _ = ref_targets(agent, q_state, t_state, b, torch.float32)
    e_q = float((masked32.double() - masked64)[m].abs().max()) if m.any() else 0.0
    top = torch.sort(masked64, dim=1).values
    clear = (m.sum(dim=1) < 2) | ((top[:, -1] - top[:, -2]) > 16 * e_q)
    print('%s: E_torch(q_next) %.3e, unclear rows %d of %d' % (name, e_q, int((~clear).sum()), len(clear)))
    assert clear.all()
    assert torch.equal(best32, best64)
    got = y[0].cpu()
    check_bound(got.numpy(), y64.numpy(), y32.numpy(), name + ' targets')
    dn = b['done'].bool()
    assert torch.equal(got[dn], b['reward'][dn])                       # a terminal row: exactly the reward
    if both_done:                                                      # (terminal and non-terminal rows)
        assert dn.any() and not dn.all()
    return idx.cpu().numpy()


@pytest.mark.parametrize('name', ALL)
def test_targets(name):
    check_targets(new_agent(name), name, both_done=name in ('leduc', 'b64'))


# ---- 3. gradients ----------------------------------------------------------------------------------------------------
def ref_update(agent, q_state, b, y, dtype):
    """Estimator.update's forward and backward on the CPU in dtype with y as the constant target -> (loss, grads in
    parameters() order, the network after the forward)"""
    net = twin(agent, q_state, dtype).train()
    q = net(b['state'].to(dtype))
    Q = q.gather(1, b['action'].unsqueeze(1)).squeeze(1)
    loss = torch.nn.functional.mse_loss(Q, y.to(dtype))
    loss.backward()
    return loss.detach(), [p.grad for p in net.parameters()], net


def check_gradients(agent, name, zero_bias):
    """K = 1: the gradients, the loss and BatchNorm's running statistics against fp64 autograd of the train-mode
    EstimatorNetwork on the same batch, with the kernel's own target_out as the constant target (so that an argmax
    near-tie cannot leak in).
    Columns of the batch that are constant: train-mode BatchNorm maps them to its bias beta_k, so dL/dW_0[o][k] =
    beta_k * db_0[o] -- exactly zero where beta_k is zero, which is how a fresh network starts; the 'leduc' case keeps
    BatchNorm's bias at zero and asserts the exact zeros, the other cases have a random bias and those columns fall
    under the bound like every other."""
    agent.train_t = 5
    q_state = state_of(agent.q_estimator)
    tracked = int(q_state['fc_layers.1.num_batches_tracked'])
    loss, idx, y, grads = agent.train_fused(1, debug=True)
    b = batch_of(agent, idx[0])
    yk = y[0].cpu()
    l64, g64, n64 = ref_update(agent, q_state, b, yk, torch.float64)
    l32, g32, n32 = ref_update(agent, q_state, b, yk, torch.float32)
    flat = grads.cpu()
    names = [k for k, _ in n64.named_parameters()]
    at = 0
    for k, a64, a32 in zip(names, g64, g32):
        got = flat[at:at + a64.numel()].reshape(a64.shape)
        at += a64.numel()
        check_bound(got.numpy(), a64.numpy(), a32.numpy(), '%s grad %s' % (name, k))
        if k == 'fc_layers.2.weight':
            const = (b['state'] == b['state'][0]).all(dim=0)
            if zero_bias:
                assert const.any() and not const.all()
                assert not got[:, const].any() and not a64[:, const].any()
                assert got[:, ~const].abs().max() > 0
    assert at == flat.numel()
    check_bound(loss.cpu().numpy(), l64.numpy().reshape(1), l32.numpy().reshape(1), name + ' loss')
    after = state_of(agent.q_estimator)
    for k in ('running_mean', 'running_var'):
        check_bound(after['fc_layers.1.' + k].numpy(), getattr(n64.fc_layers[1], k).numpy(),
                    getattr(n32.fc_layers[1], k).numpy(), '%s %s' % (name, k))
    assert int(after['fc_layers.1.num_batches_tracked']) == tracked + 1 == int(n64.fc_layers[1].num_batches_tracked)
    assert after['fc_layers.1.num_batches_tracked'].dtype == torch.int64


@pytest.mark.parametrize('name', ALL)
def test_gradients(name):
    zero_bias = name == 'leduc'
    check_gradients(new_agent(name, bn_bias=not zero_bias), name, zero_bias)


# ---- 3b. a wrapped ring, given indices out of range --------------------------------------------------------------------
@pytest.mark.parametrize('cap', [97, 1000])
def test_wrapped_ring(cap):
    """A capacity under the 'leduc' rollout's 3 850 transitions: the ring has wrapped and its oldest transition is not
    in slot 0, so slot = (total - size + pick) % cap is no identity and no permutation of one batch (the cap = 32 tests
    above cannot tell a wrong slot). The sampler draws from cap; the targets and the gradients are test_targets' and
    test_gradients' against gather() on the same ring, which test_gpu_dqn.py's 'leduc-grow' case holds to RefReplay
    wrapped. The last 97 transitions of a 16-step window are all terminal (a row whose game goes on waits for the next
    push), so that ring checks slots, states, actions and rewards; 1000 has rows of both kinds, as 'leduc' asserts."""
    agent = new_agent('leduc', cap=cap)
    size, total = agent.device_memory.sizes()
    print('wrapped ring: size %d total %d, oldest in slot %d' % (size, total, total % cap))
    assert total > cap and size == cap and total % cap != 0
    agent.train_seed = 2 ** 40 + 3
    idx = check_targets(agent, 'leduc cap %d' % cap, both_done=cap == 1000)
    assert np.array_equal(idx, floyd_batches(2 ** 40 + 3, [5, 6], cap, 32))
    check_gradients(new_agent('leduc', cap=cap, bn_bias=False), 'leduc cap %d' % cap, True)


def test_given_indices_are_clamped():
    """idx entries outside [0, size) are the caller's error and are clamped: idx_out shows 0 and size - 1, and the
    step is the one a twin agent makes on the clamped indices, bit for bit."""
    first, second = new_agent('leduc'), new_agent('leduc')
    size, B = len(first.device_memory), first.batch_size
    good = floyd_batches(11, [0, 1], size, B)
    bad = good.copy()
    bad[0, 3], bad[1, B - 1] = -5, size + 3
    good[0, 3], good[1, B - 1] = 0, size - 1
    _, idx_out, _, _ = first.train_fused(2, idx=torch.from_numpy(bad), debug=True)
    assert np.array_equal(idx_out.cpu().numpy(), good)
    second.train_fused(2, idx=torch.from_numpy(good))
    assert same(everything(first), everything(second))
    assert not same(everything(first)[:4], everything(new_agent('leduc'))[:4])


# ---- 4. Adam ---------------------------------------------------------------------------------------------------------
def check_adam(agent, ts, lr):
    """Consecutive K = 1 calls at Adam's steps ts, each checked from the kernel's own fp32 gradient g and the m0, v0,
    p0 read before the call, with u = 2^-24:
      m1 = m0 + (1 - beta1)(g - m0): three roundings and the constant's        -> |m1 - m64| <= 5 u max(|m0|, |g|)
      v1 = beta2 v0 + (1 - beta2) g^2: four roundings and the constants'       -> |v1 - v64| <= 6 u max(v0, g^2)
      p1 = p0 - Delta, Delta = step * m1 / (sqrt(v1) * rbc2 + eps) from fp64 bias corrections: the kernel rounds the
      two constants step and rbc2 = 1 / sqrt(1 - beta2^t), sqrt, the denominator's FMA, the product and the quotient:
      six roundings in Delta and one in the subtraction, doubled                -> |p1 - (p0 - Delta64)| <= 2 u |p1| +
      8 u |Delta64|, Delta64 formed in fp64 from the kernel's m1, v1."""
    b1, b2, eps, u = 0.9, 0.999, 1e-8, 2.0 ** -24
    agent.train_t = 5
    for t in ts:
        agent._adam_state()
        p0 = [p.detach().cpu().double() for p in agent.q_estimator.qnet.parameters()]
        mv0 = adam_of(agent)
        _, _, _, grads = agent.train_fused(1, debug=True)
        flat, at = grads.cpu().double(), 0
        p1 = [p.detach().cpu().double() for p in agent.q_estimator.qnet.parameters()]
        for k, ((m0, v0), (m1, v1)) in enumerate(zip(mv0, adam_of(agent))):
            g = flat[at:at + m0.numel()].reshape(m0.shape)
            at += m0.numel()
            m0, v0, m1, v1 = m0.double(), v0.double(), m1.double(), v1.double()
            m64 = m0 + (1 - b1) * (g - m0)
            v64 = b2 * v0 + (1 - b2) * g * g
            assert ((m1 - m64).abs() <= 5 * u * torch.maximum(m0.abs(), g.abs())).all(), (t, k)
            assert ((v1 - v64).abs() <= 6 * u * torch.maximum(v0, g * g)).all(), (t, k)
            delta = (lr / (1 - b1 ** t)) * m1 / (v1.sqrt() / np.sqrt(1 - b2 ** t) + eps)
            assert ((p1[k] - (p0[k] - delta)).abs() <= 2 * u * p1[k].abs() + 8 * u * delta.abs()).all(), (t, k)
            assert g.abs().max() > 0 and delta.abs().max() > 0
        steps = {int(s['step']) for s in agent.q_estimator.optimizer.state_dict()['state'].values()}
        assert steps == {t}


@pytest.mark.parametrize('name', ['leduc', 'odd', 'uno', 'nolimit', 'blackjack', 'limit'])
def test_adam_exactly(name):
    """from a fresh optimizer: t = 1, 2, 3"""
    check_adam(new_agent(name, lr=1e-3, adam='fresh'), (1, 2, 3), 1e-3)


def test_adam_far_from_step_one():
    """Seeded moments and step 999 999, so the kernel's t is 10^6 and its fp64 bias corrections come out of 20
    squarings in pow_u64 (beta2^t underflows to 0, beta1^t long before it): the same bounds."""
    agent = new_agent('leduc', lr=1e-3, adam='seeded')
    for st in agent._adam_state()[1]:
        st['step'].fill_(999999)
    check_adam(agent, (10 ** 6,), 1e-3)


# ---- 5. chunking and determinism -------------------------------------------------------------------------------------
@pytest.mark.parametrize('name', ['leduc', 'odd', 'uno', 'mahjong', 'nolimit', 'blackjack', 'limit'])
def test_chunking_and_determinism(name):
    """8 steps in one launch, in 8 launches, and as 3 + 5 leave bit-identical parameters, buffers, Adam state, target
    network and losses (target copies at train_t 3 and 6 included); so do two fresh runs."""
    runs = []
    for chunks in ((8,), (1,) * 8, (3, 5), (8,)):
        agent = new_agent(name, every=3)
        agent.train_t = 1
        losses = torch.cat([agent.train_fused(k) for k in chunks]).cpu()
        assert agent.train_t == 9 and torch.isfinite(losses).all()
        runs.append(everything(agent) + [losses])
    for r in runs[1:]:
        assert same(runs[0], r)
    assert not same(runs[0][:4], everything(new_agent(name, every=3))[:4])


# ---- 6. target copy --------------------------------------------------------------------------------------------------
def test_target_copy():
    first, second = new_agent('leduc', every=3), new_agent('leduc', every=3)
    assert first.train_t == 0
    before = state_of(first.target_estimator)
    first.train_fused(4)                                     # copies after the updates of train_t 0 and 3
    q1, t1 = state_of(first.q_estimator), state_of(first.target_estimator)
    assert same(list(q1.values()), list(t1.values()))
    assert not same(list(t1.values()), list(before.values()))
    assert int(t1['fc_layers.1.num_batches_tracked']) == 4
    second.train_fused(5)                                    # one more update after the copy at train_t 3
    q2, t2 = state_of(second.q_estimator), state_of(second.target_estimator)
    assert same(list(t2.values()), list(q1.values()))
    assert not same(list(t2.values()), list(q2.values()))
    never = new_agent('leduc', every=0)
    tn = state_of(never.target_estimator)
    never.train_fused(4)
    assert same(list(state_of(never.target_estimator).values()), list(tn.values()))


# ---- 7. learning -----------------------------------------------------------------------------------------------------
def test_learning():
    """A memory of exactly B transitions (every step trains on all of them), lr 1e-2, no target copies, 300 steps: the
    last loss is under a tenth of the first. The torch train() path under the same setup comes first, so that the
    condition is known to hold for the reference alone."""
    ref = new_agent('leduc', lr=1e-2, every=10 ** 9, adam='fresh', cap=32)
    ref.train_t = 1                                          # (train()'s first call would copy at train_t 0)
    ref.generator = torch.Generator(device='cpu').manual_seed(1)
    assert len(ref.device_memory) == 32
    ref_losses = [ref.train() for _ in range(300)]
    print('torch: first %.4f last %.4f' % (ref_losses[0], ref_losses[-1]))
    assert ref_losses[-1] < 0.1 * ref_losses[0]
    agent = new_agent('leduc', lr=1e-2, every=0, adam='fresh', cap=32)
    losses = agent.train_fused(300).cpu().numpy()
    print('fused: first %.4f last %.4f' % (losses[0], losses[-1]))
    assert np.isfinite(losses).all() and losses[-1] < 0.1 * losses[0]
    assert float(agent.last_loss) == losses[-1] and agent.last_loss.is_cuda


# ---- 8. interplay ----------------------------------------------------------------------------------------------------
def test_interplay_with_the_torch_paths():
    from rlcard_amd.agents import DQNAgent, Estimator
    agent = new_agent('leduc', adam='fresh')
    agent.generator = torch.Generator(device='cpu').manual_seed(3)
    d0 = agent.q_estimator.folded()
    agent.train_fused(2)
    d1 = agent.q_estimator.folded()
    assert d1 is not d0
    fresh = Estimator(num_actions=4, state_shape=[36], mlp_layers=[64, 64], device=agent.device)
    fresh.load_state_dict(agent.q_estimator.qnet.state_dict())
    want = fresh.folded()
    assert same([t.cpu() for t in d1.tensors], [t.cpu() for t in want.tensors])
    assert not same([t.cpu() for t in d1.tensors], [t.cpu() for t in d0.tensors])
    assert np.isfinite(agent.train())                        # the torch step goes on from the kernel's state
    assert agent.train_t == 3
    steps = [float(s['step']) for s in agent.q_estimator.optimizer.state_dict()['state'].values()]
    assert steps == [3.0] * 8
    back = DQNAgent.from_checkpoint(agent.checkpoint_attributes())
    assert back.train_t == 3
    assert same(list(state_of(back.q_estimator).values()), list(state_of(agent.q_estimator).values()))
    o1, o2 = back.q_estimator.optimizer.state_dict(), agent.q_estimator.optimizer.state_dict()
    for k in o2['state']:
        assert torch.equal(o1['state'][k]['exp_avg'].cpu(), o2['state'][k]['exp_avg'].cpu())
        assert float(o1['state'][k]['step']) == 3.0


def test_collectors_feed_the_fused_learner():
    from rlcard_amd import VecEnv
    from rlcard_amd.agents import DQNAgent, DQNCollector, NFSPCollector
    from test_gpu_nfsp import new_vec_agent
    v = VecEnv('leduc-holdem', 256, seed=31)
    torch.manual_seed(1)
    agent = DQNAgent(num_actions=4, state_shape=[36], mlp_layers=[64, 64], replay_memory_size=4096,
                     replay_memory_init_size=100, batch_size=32, update_target_estimator_every=1000,
                     epsilon_decay_steps=2000, learning_rate=1e-3, device=v.device)
    col = DQNCollector(v, agent, seats=(0,), opponents='leduc-holdem-rule-v1', steps_per_feed=16, seed=5)
    start = list(state_of(agent.q_estimator).values())
    losses = col.run(train_steps=4, fused=True)
    assert agent.train_t == 4 and losses.shape == (4,) and losses.is_cuda and torch.isfinite(losses).all()
    assert not same(start, list(state_of(agent.q_estimator).values()))
    assert col.run(train_steps=0, fused=True).shape == (0,) and agent.train_t == 4
    # without train_steps: the reference's count for the advance of total_t
    agent.train_every = 100
    t0 = agent.total_t
    losses = col.run(fused=True)
    steps = len([t for t in range(t0 + 1, agent.total_t + 1) if t >= 100 and (t - 100) % 100 == 0])
    assert steps >= 1 and agent.train_t == 4 + steps and losses.shape == (steps,)
    assert col.run(train_steps=1) and agent.train_t == 5 + steps      # the default path is the torch one, a list
    # NFSP passes it to its inner agent; train_sl stays torch
    v2 = VecEnv('leduc-holdem', 256, seed=32)
    nfsp = new_vec_agent(v2, 2)
    ncol = NFSPCollector(v2, nfsp, seats=(0, 1), steps_per_feed=16, seed=5)
    rl, sl = ncol.run(train_steps=4, sl_steps=0, fused=True)
    assert nfsp._rl_agent.train_t == 4 and rl.shape == (4,) and torch.isfinite(rl).all() and sl == []


# ---- 9. refusals -----------------------------------------------------------------------------------------------------
def test_refusals():
    from rlcard_amd import VecEnv, _abi
    from rlcard_amd.agents import DeviceMemory
    agent = new_agent('leduc')
    before = everything(agent)
    for B, K in ((1, 1), (65, 1), (32, 0), (32, 4097)):
        agent.batch_size = B
        with pytest.raises(_abi.CardsimError, match='CS_E_INVALID'):
            agent.train_fused(K)
    agent.batch_size = 32
    assert agent.train_t == 0 and same(before, everything(agent))
    empty = new_agent('leduc', push=False)
    with pytest.raises(_abi.CardsimError, match='CS_E_STATE'):
        empty.train_fused(1)
    assert empty.train_t == 0
    ddz = VecEnv('doudizhu', 2, seed=1)
    with pytest.raises(_abi.CardsimError, match='CS_E_UNSUPPORTED'):
        DeviceMemory(ddz, 16)
