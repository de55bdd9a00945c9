"""NFSP on the device (rlcard_amd/csrc/cs_dqn.hip and cs_nfsp.hip through include/cardsim.h and
rlcard_amd/agents/nfsp_agent.py): the average-policy head of the network kernel against an fp64 restatement of the
reference chain (np.exp(log_softmax), remove_illegal) and a torch-CPU fp32 one, its sampled action against a numpy
restatement of the draw, the per-mode row lists against cs_qnet_actions and the all-average call, the reservoir
against a sequential numpy ReservoirBuffer.add with the same Philox draws, and the agent end to end. Needs a GPU."""
import ctypes as C

import numpy as np
import pytest

import test_dqn
from test_gpu_dqn import VALUE_CASES, value_case
from test_nfsp import GOLDEN, network_of, probs64, unfolded_logits64

torch = pytest.importorskip('torch')
pytestmark = pytest.mark.gpu

ULP = 2.0 ** -24      # one ulp of 1.0 in fp32


@pytest.fixture(scope='module', autouse=True)
def _need_gpu():
    if not torch.cuda.is_available():
        pytest.fail('GPU tests need a visible GPU (run them on the MI355X box)')


@pytest.fixture(scope='module')
def gold():
    return dict(np.load(GOLDEN, allow_pickle=False))


@pytest.fixture(scope='module')
def gold_dqn():
    return dict(np.load(test_dqn.GOLDEN, allow_pickle=False))


def _ptr(t):
    return None if t is None else C.c_void_p(t.data_ptr())


def pnet_probs(v, net, obs, legal):
    from rlcard_amd import _abi
    p = torch.empty((obs.shape[0], net.num_actions), dtype=torch.float32, device=v.device)
    _abi.check(_abi.lib().cs_pnet_probs(v._h, C.byref(net.folded()), _ptr(obs), _ptr(legal), obs.shape[0], _ptr(p),
                                        v._stream()), 'cs_pnet_probs')
    return p


def nfsp_actions(v, est, net, obs, legal, done=None, mode=None, eps=0.0, seed=0, t=0, row_base=0, probs=None):
    from rlcard_amd import _abi
    L = _abi.lib()
    rows = obs.shape[0]
    a = torch.full((rows,), -7, dtype=torch.int32, device=v.device)
    scratch = None
    if mode is not None:
        need = L.cs_nfsp_scratch_bytes(rows)
        assert need > 0
        scratch = torch.empty(need, dtype=torch.uint8, device=v.device)
    q = None if est is None else C.byref(est.folded())
    _abi.check(L.cs_nfsp_actions(v._h, q, C.byref(net.folded()), _ptr(obs), _ptr(legal), _ptr(done), _ptr(mode), rows,
                                 float(eps), seed, t, row_base, _ptr(a), _ptr(probs), _ptr(scratch), v._stream()),
               'cs_nfsp_actions')
    return a


def random_policy_net(num_actions, obs_dim, mlp, seed):
    """Seeded random weights, BatchNorm statistics and affine included (so the folding is not the identity)."""
    from rlcard_amd.agents import AveragePolicyNetwork
    torch.manual_seed(seed)
    net = AveragePolicyNetwork(num_actions=num_actions, state_shape=[obs_dim], mlp_layers=list(mlp) + [num_actions])
    g = torch.Generator().manual_seed(seed)
    bn = net.mlp[1]
    with torch.no_grad():
        bn.running_mean.copy_(torch.rand(obs_dim, generator=g) * 2)
        bn.running_var.copy_(torch.rand(obs_dim, generator=g) * 4 + 0.5)
        bn.weight.copy_(torch.rand(obs_dim, generator=g) + 0.5)
        bn.bias.copy_(torch.rand(obs_dim, generator=g) - 0.5)
        for m in net.mlp:
            if isinstance(m, torch.nn.Linear):
                torch.nn.init.xavier_uniform_(m.weight)
                m.bias.copy_(torch.rand(m.bias.shape, generator=g) - 0.5)
    net.eval()
    return net


def on_device(net, device):
    from rlcard_amd.agents import AveragePolicyNetwork
    d = AveragePolicyNetwork(num_actions=net.num_actions, state_shape=net.state_shape, mlp_layers=net.mlp_layers)
    d.load_state_dict(net.state_dict())
    d.eval()
    return d.to(device)


# ---- Philox4x32-10, restated ------------------------------------------------------------------------------------------
M32 = np.uint64(0xFFFFFFFF)


def philox4(seed, ctr, blk):
    """Words r[0..3] (uint32 arrays) of Philox4x32-10 with the key `seed` on the counter (ctr, blk): ctr a uint64
    array, blk an int; the engine's philox4(seed, env, blk)."""
    ctr = np.asarray(ctr, np.uint64)
    c0, c1 = ctr & M32, ctr >> np.uint64(32)
    c2 = np.full(ctr.shape, blk & 0xFFFFFFFF, np.uint64)
    c3 = np.full(ctr.shape, (blk >> 32) & 0xFFFFFFFF, np.uint64)
    k0, k1 = seed & 0xFFFFFFFF, (seed >> 32) & 0xFFFFFFFF
    for _ in range(10):
        p0, p1 = np.uint64(0xD2511F53) * c0, np.uint64(0xCD9E8D57) * c2
        n0 = (p1 >> np.uint64(32)) ^ c1 ^ np.uint64(k0)
        n2 = (p0 >> np.uint64(32)) ^ c3 ^ np.uint64(k1)
        c0, c1, c2, c3 = n0, p1 & M32, n2, p0 & M32
        k0, k1 = (k0 + 0x9E3779B9) & 0xFFFFFFFF, (k1 + 0xBB67AE85) & 0xFFFFFFFF
    return [x.astype(np.uint32) for x in (c0, c1, c2, c3)]


def test_philox_restatement_is_the_oracles(oracle):
    L = oracle.lib()
    L.or_philox4.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p]
    for seed, ctr, blk in ((0, 0, 0), (2 ** 64 - 1, 2 ** 64 - 1, 2 ** 64 - 1), (0x299f31d0a4093822, 0x85a308d3243f6a88,
                                                                              0x0370734413198a2e), (7, 2 ** 40 + 5, 11)):
        c = (C.c_uint32 * 4)(ctr & 0xFFFFFFFF, ctr >> 32, blk & 0xFFFFFFFF, blk >> 32)
        k = (C.c_uint32 * 2)(seed & 0xFFFFFFFF, seed >> 32)
        o = (C.c_uint32 * 4)()
        L.or_philox4(c, k, o)
        assert [int(x[0]) for x in philox4(seed, np.array([ctr], np.uint64), blk)] == list(o)


# ---- probabilities ------------------------------------------------------------------------------------------------------
_pcache = {}


def prob_case(gold, gold_dqn, case):
    """test_gpu_dqn's rows of the case (value_case) with an average-policy network: the fixture's for Leduc and Limit,
    seeded random weights otherwise; the fp64 reference and the torch-CPU fp32 chain of the rows, computed once."""
    from rlcard_amd.utils import remove_illegal
    game, _, rows, spec = case
    if game in _pcache:
        return _pcache[game]
    c = value_case(gold_dqn, case)
    v, x, m = c['v'], c['obs'].cpu().numpy(), c['mask']
    cpu = network_of(gold, spec) if isinstance(spec, str) else random_policy_net(v.num_actions, v.obs_dim, spec[0],
                                                                                 spec[1])
    ref64 = probs64(unfolded_logits64(cpu, x), m)
    with torch.no_grad():
        p32 = np.exp(cpu(torch.from_numpy(x).float()).numpy())      # NFSPAgent._act
    assert p32.dtype == np.float32
    p_torch = np.stack([remove_illegal(p32[r], np.nonzero(m[r])[0]) for r in range(rows)])
    out = dict(c, cpu=cpu, net=on_device(cpu, v.device), ref64=ref64, p_torch=p_torch)
    _pcache[game] = out
    return out


@pytest.mark.parametrize('case', VALUE_CASES, ids=[c[0] for c in VALUE_CASES])
def test_pnet_probs(gold, gold_dqn, case):
    """E_kernel <= 8 E_torch + 4 ulp(1): the factor is the project's bound for this accumulation order against
    torch's; the additive term covers the head's device expf and its two fp32 divisions on values of at most 1, which
    the reference does in fp64. Illegal entries exactly 0, rows sum to 1."""
    c = prob_case(gold, gold_dqn, case)
    m = c['mask']
    p = pnet_probs(c['v'], c['net'], c['obs'], c['legal']).cpu().numpy()
    assert m.any(axis=1).all()
    assert np.all(p[~m] == 0) and np.all(p[m] >= 0)
    assert np.abs(p.astype(np.float64).sum(axis=1) - 1).max() <= 8 * ULP
    e_torch = np.abs(c['p_torch'] - c['ref64']).max()
    e_kernel = np.abs(p.astype(np.float64) - c['ref64']).max()
    print('%s: E_torch %.3e E_kernel %.3e ratio %.2f (bound %.3e)' % (case[0], e_torch, e_kernel,
                                                                      e_kernel / e_torch, 8 * e_torch + 4 * ULP))
    assert e_kernel <= 8 * e_torch + 4 * ULP
    # no mask: the softmax over every action
    p_all = pnet_probs(c['v'], c['net'], c['obs'], None).cpu().numpy()
    every = probs64(unfolded_logits64(c['cpu'], c['obs'].cpu().numpy()), np.ones_like(m))
    assert np.abs(p_all.astype(np.float64) - every).max() <= 8 * e_torch + 4 * ULP


def test_underflow_falls_back_to_uniform():
    """A net whose logits are (0, 200, 0, 0) whatever the observation: with action 1 illegal the legal mass is
    exp(-200) = 0 in fp32, and the row is exactly 1 / count on the legal actions; with action 1 legal it is that
    action."""
    from rlcard_amd import VecEnv
    from rlcard_amd.agents.dqn_agent import descriptor

    class Net:
        num_actions = 4

        def __init__(self, device):
            wb = [(np.zeros((8, 36)), np.zeros(8)), (np.zeros((4, 8)), np.array([0.0, 200.0, 0.0, 0.0]))]
            self._d = descriptor(wb, device)

        def folded(self):
            return self._d

    v = VecEnv('leduc-holdem', 64, seed=1)
    masks = [0b1101, 0b0101, 0b0100, 0b1001, 0b1111, 0b0010, 0b0110]
    R = 70
    legal = torch.tensor([masks[r % len(masks)] for r in range(R)], dtype=torch.uint8, device=v.device).reshape(R, 1)
    obs = torch.ones((R, 36), dtype=torch.uint8, device=v.device)
    p = pnet_probs(v, Net(v.device), obs, legal).cpu().numpy()
    for r in range(R):
        mk = masks[r % len(masks)]
        ids = [a for a in range(4) if (mk >> a) & 1]
        want = np.zeros(4, np.float32)
        if 1 in ids:
            want[1] = 1
        else:
            want[ids] = np.float32(1) / np.float32(len(ids))
        assert np.array_equal(p[r], want), (r, mk, p[r])


# ---- sampling -----------------------------------------------------------------------------------------------------------
def sample_ref(probs, mask, done, seed, t, row_base):
    """The draw restated: u = (r[2] >> 8) * 2^-24 of philox4(seed, row_base + row, t), the first legal action in id
    order whose running fp32 sum passes u, else the last legal one; -1 for done rows and empty masks."""
    R, A = probs.shape
    ctr = (np.uint64(row_base) + np.arange(R, dtype=np.uint64))
    u = (philox4(seed, ctr, t)[2] >> np.uint32(8)).astype(np.float32) * np.float32(ULP)
    c = np.zeros(R, np.float32)
    pick = np.full(R, -1, np.int32)
    last = np.full(R, -1, np.int32)
    for a in range(A):
        c = np.where(mask[:, a], (c + probs[:, a]).astype(np.float32), c)
        last = np.where(mask[:, a], a, last)
        pick = np.where(mask[:, a] & (pick < 0) & (u < c), a, pick)
    pick = np.where(pick < 0, last, pick)
    return np.where(done, -1, pick).astype(np.int32)


@pytest.mark.parametrize('case', VALUE_CASES[:2], ids=[c[0] for c in VALUE_CASES[:2]])
def test_sampled_actions_match_the_restated_draw(gold, gold_dqn, case):
    c = prob_case(gold, gold_dqn, case)
    v, net, obs = c['v'], c['net'], c['obs']
    R, A = obs.shape[0], v.num_actions
    legal = c['legal'].clone()
    done = torch.zeros(R, dtype=torch.uint8, device=v.device)
    legal[3::17] = 0
    done[5::13] = 1
    m = c['mask'].copy()
    m[3::17] = False
    dn = done.cpu().numpy().astype(bool)
    seen = set()
    for seed, t, base in ((7, 11, 1000), (2 ** 40 + 3, 2 ** 33 + 1, 2 ** 35 + 5), (1, 2, 3)):
        probs = torch.full((R, A), -1.0, dtype=torch.float32, device=v.device)
        got = nfsp_actions(v, None, net, obs, legal, done, None, 0.0, seed, t, base, probs).cpu().numpy()
        ph = probs.cpu().numpy()
        live = m.any(axis=1)
        assert np.array_equal(ph[live], pnet_probs(v, net, obs, legal).cpu().numpy()[live])
        want = sample_ref(ph, m, dn, seed, t, base)
        assert np.array_equal(got, want), (seed, t, base)
        assert np.all(got[~live | dn] == -1) and np.all(got[live & ~dn] >= 0)
        assert all(m[r, got[r]] for r in np.nonzero(live & ~dn)[0])
        seen.add(got.tobytes())
    assert len(seen) == 3                               # the draws depend on the key
    # no done pointer: only the empty masks give -1
    g2 = nfsp_actions(v, None, net, obs, legal, None, None, 0.0, 7, 11, 1000).cpu().numpy()
    assert np.array_equal(g2 == -1, ~m.any(axis=1))


def test_sampled_action_frequencies(gold, gold_dqn):
    """65 536 copies of one observation, row_base 0: each legal action's count within 5 sigma of N p."""
    c = prob_case(gold, gold_dqn, VALUE_CASES[0])
    v, net = c['v'], c['net']
    p_rows = pnet_probs(v, net, c['obs'], c['legal']).cpu().numpy()
    # a row with every action it has well inside (0, 1)
    r = int(np.argmax(np.where(c['mask'], p_rows, 1.0).min(axis=1) * (c['mask'].sum(axis=1) >= 2)))
    p = p_rows[r].astype(np.float64)
    assert c['mask'][r].sum() >= 2 and p[c['mask'][r]].min() > 1e-3
    N = 65536
    obs = c['obs'][r:r + 1].expand(N, -1).contiguous()
    legal = c['legal'][r:r + 1].expand(N, -1).contiguous()
    got = nfsp_actions(v, None, net, obs, legal, None, None, 0.0, 5, 9, 0).cpu().numpy()
    counts = np.bincount(got, minlength=v.num_actions)
    print('p', p, 'counts', counts)
    assert counts.sum() == N and np.all(counts[~c['mask'][r]] == 0)
    for a in np.nonzero(c['mask'][r])[0]:
        assert abs(counts[a] - N * p[a]) <= 5 * np.sqrt(N * p[a] * (1 - p[a])), a


# ---- modes --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('case', VALUE_CASES[:2], ids=[c[0] for c in VALUE_CASES[:2]])
def test_each_network_runs_on_its_own_rows(gold, gold_dqn, case):
    from test_gpu_dqn import qnet_actions
    c = prob_case(gold, gold_dqn, case)
    v, est, net = c['v'], c['dev'], c['net']
    R, A = c['obs'].shape[0], v.num_actions
    legal = c['legal'].clone()
    done = torch.zeros(R, dtype=torch.uint8, device=v.device)
    legal[3::17] = 0
    done[5::13] = 1
    rng = np.random.RandomState(4)
    modes = {'rate 0.1': (rng.rand(R) < 0.1).astype(np.uint8), 'all 0': np.zeros(R, np.uint8),
             'all 1': np.ones(R, np.uint8)}
    assert 0 < modes['rate 0.1'].sum() < R // 4
    eps, seed, t, base = 0.3, 2 ** 40 + 3, 2 ** 33, 77
    SENT = -3.0
    differ = False
    for rows in (R, 65, 1):
        o, lg, dn = c['obs'][:rows].contiguous(), legal[:rows].contiguous(), done[:rows].contiguous()
        br = qnet_actions(v, est, o, lg, dn, eps, seed, t, base).cpu().numpy()
        p_avg = torch.full((rows, A), SENT, dtype=torch.float32, device=v.device)
        avg = nfsp_actions(v, None, net, o, lg, dn, None, eps, seed, t, base, p_avg).cpu().numpy()
        p_avg = p_avg.cpu().numpy()
        assert np.all(p_avg != SENT)
        differ = differ or bool((br != avg).any())
        for name, mode in modes.items():
            mh = mode[:rows].astype(bool)
            md = torch.from_numpy(mode[:rows].copy()).to(v.device)
            probs = torch.full((rows, A), SENT, dtype=torch.float32, device=v.device)
            got = nfsp_actions(v, est, net, o, lg, dn, md, eps, seed, t, base, probs).cpu().numpy()
            ph = probs.cpu().numpy()
            assert np.array_equal(got[mh], br[mh]), (name, rows)           # cs_qnet_actions, bit for bit
            assert np.array_equal(got[~mh], avg[~mh]), (name, rows)        # the mode = NULL call
            assert np.all(ph[mh] == SENT), (name, rows)
            assert np.array_equal(ph[~mh], p_avg[~mh]), (name, rows)
            # probs NULL: the same actions
            g2 = nfsp_actions(v, est, net, o, lg, dn, md, eps, seed, t, base).cpu().numpy()
            assert np.array_equal(g2, got)
    assert differ


def test_refusals(gold, gold_dqn):
    from rlcard_amd import VecEnv, _abi
    from rlcard_amd.agents import DeviceReservoir
    leduc = VecEnv('leduc-holdem', 64, seed=1)
    net = on_device(network_of(gold, 'leduc'), leduc.device)
    obs = torch.zeros((64, 901), dtype=torch.uint8, device=leduc.device)
    ddz = VecEnv('doudizhu', 2, seed=1)
    with pytest.raises(_abi.CardsimError, match='CS_E_UNSUPPORTED'):
        pnet_probs(ddz, net, obs, None)
    limit_net = on_device(network_of(gold, 'limit'), leduc.device)
    with pytest.raises(_abi.CardsimError, match='CS_E_INVALID'):       # in_dim 72 on a 36-byte game
        pnet_probs(leduc, limit_net, obs, None)
    d = net.folded()
    p = torch.empty((64, 4), dtype=torch.float32, device=leduc.device)
    bad = _abi.QNet.from_buffer_copy(d)
    bad.hidden[0] = 129
    assert _abi.lib().cs_pnet_probs(leduc._h, C.byref(bad), _ptr(obs), None, 64, _ptr(p), None) == -1
    bad = _abi.QNet.from_buffer_copy(d)
    bad.W[1] = None
    assert _abi.lib().cs_pnet_probs(leduc._h, C.byref(bad), _ptr(obs), None, 64, _ptr(p), None) == -1
    bad = _abi.QNet.from_buffer_copy(d)
    bad.num_hidden = 5
    assert _abi.lib().cs_pnet_probs(leduc._h, C.byref(bad), _ptr(obs), None, 64, _ptr(p), None) == -1
    assert _abi.lib().cs_pnet_probs(leduc._h, C.byref(d), _ptr(obs), None, 64, None, None) == -1
    with pytest.raises(_abi.CardsimError, match='CS_E_UNSUPPORTED'):
        DeviceReservoir(ddz, 16)


# ---- reservoir ----------------------------------------------------------------------------------------------------------
class RefReservoir:
    """ReservoirBuffer.add, sequential, with np.random.randint(0, k + 1) restated as the engine's draw: x = r[0] |
    r[1] << 32 of philox4(seed, k, 0), j = (x * (k + 1)) >> 64."""

    def __init__(self, cap, seed, P):
        self.cap, self.seed, self.P = cap, seed, P
        self.data = []
        self.calls = 0
        self.dropped = 0       # candidates whose draw fell outside the buffer
        self.collisions = 0    # candidates that replaced one of the same push

    def candidates(self, w, mode, seats):
        T, n = w['player'].shape
        return [(t, e) for t in range(T) for e in range(n)
                if w['player'][t, e] < self.P and int(w['player'][t, e]) in seats and mode[t, e]]

    def push(self, w, mode, seats):
        cand = self.candidates(w, mode, seats)
        ks = self.calls + np.arange(len(cand), dtype=np.uint64)
        r = philox4(self.seed, ks, 0)
        hit = set()
        for i, (t, e) in enumerate(cand):
            k = self.calls
            item = (w['obs'][t, e].copy(), int(w['action'][t, e]))
            if len(self.data) < self.cap:
                slot = len(self.data)
                self.data.append(item)
            else:
                x = int(r[0][i]) | (int(r[1][i]) << 32)
                slot = (x * (k + 1)) >> 64
                assert 0 <= slot <= k
                if slot < self.cap:
                    self.data[slot] = item
                else:
                    self.dropped += 1
                    slot = None
            if slot is not None:
                self.collisions += slot in hit
                hit.add(slot)
            self.calls += 1
        return len(cand)


def held(res):
    size = len(res)
    got = res.gather(torch.arange(size, device=res.vec.device))
    return got['state'].cpu().numpy(), got['action_probs'].cpu().numpy()


def assert_same_reservoir(res, ref, A, what):
    st, pr = held(res)
    assert res.sizes() == (len(ref.data), ref.calls), what
    assert st.shape == (len(ref.data), len(ref.data[0][0])) and pr.shape == (len(ref.data), A), what
    assert np.array_equal(st, np.array([d[0] for d in ref.data], np.float32)), what
    assert np.all((pr == 0) | (pr == 1)) and np.all(pr.sum(axis=1) == 1), what
    assert np.array_equal(pr.argmax(axis=1), np.array([d[1] for d in ref.data])), what


# (game, config, envs, steps of each window, a capacity smaller than the longest window's push, and a number of
# candidates every push exceeds)
RESERVOIR_CASES = [('leduc-holdem', None, 300, (16,) * 5, 64, 100),
                   ('leduc-holdem', {'game_num_players': 3}, 96, (16,) * 5, 64, 100),
                   # two waves plus two envs; the push scratch grows (2 -> 8 steps) and is reused at a smaller size. A
                   # 2-step window has 260 rows, a quarter of them seat 0's in best-response mode: 30 is far below that
                   ('leduc-holdem', None, 130, (2, 8, 2), 97, 30)]


@pytest.mark.parametrize('all_seats', [False, True], ids=['seat0', 'all'])
@pytest.mark.parametrize('case', RESERVOIR_CASES, ids=['leduc', 'leduc3', 'leduc-grow'])
def test_reservoir_matches_sequential_add(case, all_seats):
    from rlcard_amd import VecEnv
    from rlcard_amd.agents import DeviceReservoir
    game, config, n, steps, small, least = case
    v = VecEnv(game, n, seed=21, config=config)
    v.reset()
    P, A = v.num_players, v.num_actions
    seats = tuple(range(P)) if all_seats else (0,)
    g = torch.Generator().manual_seed(6)
    windows = []
    t0 = 0
    for T in steps:
        tr = v.rollout(T, policy_seed=3, t0=t0, final_obs=True)
        t0 += T
        tr = {k: x.clone() for k, x in tr.items()}
        mode = (torch.rand((T, n), generator=g) < 0.5).to(torch.uint8).to(v.device)
        windows.append((tr, mode, {k: x.cpu().numpy() for k, x in tr.items()}, mode.cpu().numpy()))
    counts = [len(RefReservoir(1, 0, P).candidates(wh, mh, seats)) for _, _, wh, mh in windows]
    assert min(counts) > least and max(counts) > small
    mid = counts[0] + counts[1] + counts[2] // 2         # fills in the middle of the third push
    caps = (1 << 16, mid, small)
    seed = 2 ** 40 + 9
    res = [DeviceReservoir(v, cap, seed) for cap in caps]
    refs = [RefReservoir(cap, seed, P) for cap in caps]
    for w, (tr, mode, wh, mh) in enumerate(windows):
        for r_, ref in zip(res, refs):
            r_.push(tr, mode, seats)
            assert ref.push(wh, mh, seats) == counts[w]
            assert_same_reservoir(r_, ref, A, 'capacity %d after push %d' % (ref.cap, w))
    assert refs[0].calls == sum(counts) < (1 << 16) and refs[0].dropped == 0 == refs[0].collisions   # pure append
    assert len(refs[1].data) == mid and refs[1].dropped > 0
    assert refs[2].collisions > 0 and refs[2].dropped > 0
    # slots: index k is slot k, outside [0, size) clamped
    st, pr = held(res[1])
    got = res[1].gather(torch.tensor([0, mid - 1, mid + 5, -3], device=v.device))
    assert np.array_equal(got['state'].cpu().numpy(), st[[0, mid - 1, mid - 1, 0]])
    assert np.array_equal(got['action_probs'].cpu().numpy(), pr[[0, mid - 1, mid - 1, 0]])
    b = res[1].sample(32, torch.Generator(device='cpu').manual_seed(1))
    assert b['state'].shape == (32, v.obs_dim) and b['action_probs'].shape == (32, A)
    assert np.all(b['action_probs'].cpu().numpy().sum(axis=1) == 1)
    with pytest.raises(ValueError):
        res[1].sample(mid + 1)
    # clear empties it, and the stream starts again
    res[2].clear()
    assert res[2].sizes() == (0, 0)
    fresh = RefReservoir(small, seed, P)
    tr, mode, wh, mh = windows[0]
    res[2].push(tr, mode, seats)
    fresh.push(wh, mh, seats)
    assert_same_reservoir(res[2], fresh, A, 'after clear')


# ---- end to end ---------------------------------------------------------------------------------------------------------
def new_vec_agent(v, seed, **kw):
    from rlcard_amd.agents import NFSPAgent
    torch.manual_seed(seed)
    args = dict(num_actions=4, state_shape=[36], hidden_layers_sizes=[64, 64], q_mlp_layers=[64, 64],
                reservoir_buffer_capacity=1024, anticipatory_param=0.5, batch_size=32, min_buffer_size_to_learn=32,
                q_replay_memory_size=4096, q_replay_memory_init_size=100, q_batch_size=32, q_epsilon_start=0.5,
                q_epsilon_decay_steps=2000, rl_learning_rate=1e-3, device=v.device)
    args.update(kw)
    agent = NFSPAgent(**args)
    agent.attach(v, seed=seed + 100)
    agent.generator = torch.Generator(device='cpu').manual_seed(seed)
    agent._rl_agent.generator = torch.Generator(device='cpu').manual_seed(seed + 1)
    return agent


def policy_params(agent):
    return [p.detach().clone() for p in agent.policy_network.state_dict().values()]


@pytest.mark.parametrize('seats,opponents', [((0, 1), 'random'), ((0,), 'leduc-holdem-rule-v1')],
                         ids=['self-play', 'rule-opponent'])
def test_collector_feed_train_end_to_end(seats, opponents):
    from rlcard_amd import VecEnv
    from rlcard_amd.agents import NFSPCollector
    v = VecEnv('leduc-holdem', 256, seed=31)
    agent = new_vec_agent(v, 1)
    col = NFSPCollector(v, agent, seats=seats, opponents=opponents, steps_per_feed=16, seed=5)
    ref = RefReservoir(1024, 101, 2)
    start = policy_params(agent)
    d0 = agent.policy_network.folded()
    for rnd in range(3):
        tr = col.collect()
        mh = col.mode_rows.cpu().numpy()
        wh = {k: x.cpu().numpy() for k, x in tr.items()}
        assert 0 < mh.mean() < 1 and (wh['player'] == 255).any() and wh['done'].any()
        t0, rl0 = agent.total_t, agent._rl_agent.total_t
        rl_losses, sl_losses = agent.feed_vec(tr, col.mode_rows, seats, train_steps=1, sl_steps=2)
        ref.push(wh, mh, seats)
        assert_same_reservoir(agent.device_reservoir, ref, 4, 'round %d' % rnd)
        assert agent.total_t - t0 == agent._rl_agent.total_t - rl0 > 100
        assert len(rl_losses) == 1 and len(sl_losses) == 2 and np.isfinite(sl_losses).all()
    assert ref.calls > 1024 and ref.dropped > 0          # the reservoir went past its capacity
    assert agent.train_t == 6 and agent._rl_agent.train_t == 3
    assert any(not torch.equal(a, b) for a, b in zip(start, policy_params(agent)))
    assert agent.policy_network.folded() is not d0
    # modes: the envs whose game ended were drawn again, the others kept theirs; the reference's train_sl cadence
    assert agent.mode.shape == (256, 2) and 0 < agent.mode.float().mean().item() < 1
    agent._train_every = 200
    t0 = agent.total_t
    _, sl = col.run(train_steps=0)
    steps = len([t for t in range(t0 + 1, agent.total_t + 1) if t % 200 == 0])
    assert len(sl) == steps >= 1 and agent.train_t == 6 + steps


def test_collector_reservoir_is_deterministic():
    from rlcard_amd import VecEnv
    from rlcard_amd.agents import NFSPCollector
    runs = []
    for _ in range(2):
        v = VecEnv('leduc-holdem', 256, seed=31)
        agent = new_vec_agent(v, 1)
        col = NFSPCollector(v, agent, seats=(0, 1), steps_per_feed=16, seed=5)
        for _ in range(3):
            assert col.run(train_steps=0, sl_steps=0) == ([], [])
        assert agent.train_t == 0
        runs.append(held(agent.device_reservoir) + (col.mode_rows.cpu().numpy(),))
    assert len(runs[0][0]) > 300
    for a, b in zip(runs[0], runs[1]):
        assert np.array_equal(a, b)


def test_tournament_vec_seats_an_nfsp_agent():
    from rlcard_amd import VecEnv
    from rlcard_amd.utils import tournament_vec
    v = VecEnv('leduc-holdem', 256, seed=77)
    agent = new_vec_agent(v, 3)
    res = tournament_vec(v, [agent, 'leduc-holdem-rule-v1'], 4)
    assert len(res) == 2 and np.isfinite(res).all() and res[0] + res[1] == 0
    agent.evaluate_with = 'best_response'
    res = tournament_vec(v, [agent, 'leduc-holdem-rule-v1'], 4)
    assert len(res) == 2 and np.isfinite(res).all() and res[0] + res[1] == 0
    # predict_probs_vec: the rows cs_pnet_probs gives
    st = v.reset()
    p = agent.predict_probs_vec(st['obs'], st['legal']).cpu().numpy()
    assert p.shape == (256, 4) and np.abs(p.astype(np.float64).sum(axis=1) - 1).max() <= 8 * ULP
