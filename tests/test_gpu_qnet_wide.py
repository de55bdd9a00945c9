"""The network kernel's wide instantiations (rlcard_amd/csrc/cs_dqn.hip: games of 9..64 actions, the obs rows kept as
bytes) on UNO -- 240 obs bytes, 61 actions, 8 mask bytes -- through cs_qnet_values, cs_qnet_actions, cs_pnet_probs and
cs_nfsp_actions: the reference's trained networks on its recorded rows (tests/golden/dqn_uno.npz, nfsp_uno.npz) and
seeded random ones against fp64 and torch-CPU forwards, the 64-bit mask's edges on a bias-only net, the epsilon draw
against cs_dmc_select's, the average-policy head against the fp64 chain and the restated draw, and the row lists.
The bounds are tests/test_gpu_dqn.py's and tests/test_gpu_nfsp.py's. Needs a GPU."""
import ctypes as C

import numpy as np
import pytest

from test_dqn import unfolded64
from test_gpu_dqn import on_device, qnet_actions, qnet_values, random_estimator
from test_gpu_nfsp import ULP, nfsp_actions, pnet_probs, sample_ref
from test_gpu_nfsp import on_device as policy_on_device
from test_nfsp import mask_of, probs64, unfolded_logits64
from test_qnet_uno import A, D, GOLDEN_DQN, GOLDEN_NFSP, LB, ROWS, uno_estimator, uno_policy_net

torch = pytest.importorskip('torch')
pytestmark = pytest.mark.gpu


@pytest.fixture(scope='module', autouse=True)
def _need_gpu():
    if not torch.cuda.is_available():
        pytest.fail('GPU tests need a visible GPU (run them on the MI355X box)')


@pytest.fixture(scope='module')
def gold():
    return dict(np.load(GOLDEN_DQN, allow_pickle=False))


@pytest.fixture(scope='module')
def gold_nfsp():
    return dict(np.load(GOLDEN_NFSP, allow_pickle=False))


@pytest.fixture(scope='module')
def vec():
    from rlcard_amd import VecEnv
    v = VecEnv('uno', 65, seed=5)
    assert (v.obs_dim, v.num_actions, v.legal_bytes) == (D, A, LB)
    return v


def _ptr(t):
    return None if t is None else C.c_void_p(t.data_ptr())


def dev(v, x):
    return torch.from_numpy(np.ascontiguousarray(x)).to(v.device)


# ---- values -----------------------------------------------------------------------------------------------------------
# the fixture's network on its 256 rows; seeded random ones on the first 65 (a partial block) and the first 130 (two
# blocks and two rows) of them: two waves and the widest layout; an output tile of K = 20, no multiple of the 16-unit
# stage; four layers, whose output tile lands in the other buffer than with two; one 128-unit layer
NETS = [('fixture', None, (ROWS,)), ('128-128-64', ([128, 128, 64], 1), (65, 130)), ('20', ([20], 2), (65, 130)),
        ('7-5-3-2', ([7, 5, 3, 2], 3), (65, 130)), ('128', ([128], 4), (65, 130))]
_cache = {}


def value_case(gold, v, name):
    """-> the CPU and device estimators, the case's rows, and their fp64 / torch-CPU fp32 forwards (computed once)"""
    if name in _cache:
        return _cache[name]
    _, spec, sizes = [n for n in NETS if n[0] == name][0]
    R = max(sizes)
    x, lg = gold['uno_obs'][:R], gold['uno_legal'][:R]
    cpu = uno_estimator(gold) if spec is None else random_estimator(A, D, spec[0], spec[1], 'cpu')
    out = dict(cpu=cpu, dev=on_device(cpu, v.device), obs=dev(v, x), legal=dev(v, lg), mask=mask_of(lg, A),
               ref64=unfolded64(cpu, x), q_torch=cpu.predict_nograd(x.astype(np.float32)).astype(np.float64))
    _cache[name] = out
    return out


@pytest.mark.parametrize('name', [n[0] for n in NETS])
def test_wide_values(gold, vec, name):
    """E_kernel <= 8 E_torch over the legal entries (tests/test_gpu_dqn.py's bound: both sides are fp32 sums in
    different orders, so it scales with the 240-term first layer by itself); illegal entries exactly -inf; without a
    mask the same numbers.
    Measured on the MI355X (profiles/EXPERIMENTS.md W-1): see the table there."""
    c = value_case(gold, vec, name)
    for R in [n for n in NETS if n[0] == name][0][2]:
        obs, legal, m = c['obs'][:R].contiguous(), c['legal'][:R].contiguous(), c['mask'][:R]
        q = qnet_values(vec, c['dev'], obs, legal).cpu().numpy()
        assert q.shape == (R, A) and m.any(axis=1).all() and not m.all(axis=1).any()
        assert np.all(q[~m] == -np.inf) and np.isfinite(q[m]).all()
        e_torch = np.abs(c['q_torch'][:R] - c['ref64'][:R])[m].max()
        e_kernel = np.abs(q.astype(np.float64) - c['ref64'][:R])[m].max()
        print('uno %s, %d rows: E_torch %.3e E_kernel %.3e ratio %.2f |q| <= %.2f'
              % (name, R, e_torch, e_kernel, e_kernel / e_torch, np.abs(c['ref64'][:R][m]).max()))
        assert e_kernel <= 8 * e_torch
        q_all = qnet_values(vec, c['dev'], obs, None).cpu().numpy()
        assert np.isfinite(q_all).all() and np.array_equal(q_all[m], q[m])
        e_all = np.abs(q_all.astype(np.float64) - c['ref64'][:R]).max()
        e_torch_all = np.abs(c['q_torch'][:R] - c['ref64'][:R]).max()
        assert e_all <= 8 * e_torch_all
        if name == 'fixture':     # the reference's own agent.predict rows
            want = gold['uno_predict']
            assert np.array_equal(np.isfinite(want), m)
            e_rec = np.abs(q[m].astype(np.float64) - want[m].astype(np.float64)).max()
            print('uno fixture: |kernel - recorded predict| <= %.3e (%.2f E_torch)' % (e_rec, e_rec / e_torch))
            assert e_rec <= 8 * e_torch


# ---- mask edges -------------------------------------------------------------------------------------------------------
class BiasNet:
    """A net whose outputs are `out_bias` whatever the observation: zero weights (tanh(0) = relu(0) = 0)."""
    num_actions = A

    def __init__(self, device, out_bias):
        from rlcard_amd.agents.dqn_agent import descriptor
        self._d = descriptor([(np.zeros((8, D)), np.zeros(8)), (np.zeros((A, 8)), np.asarray(out_bias, np.float64))],
                             device)

    def folded(self):
        return self._d


def bits(ids, n=LB):
    m = np.zeros(8 * n, np.uint8)
    m[list(ids)] = 1
    return np.packbits(m, bitorder='little')


# only id 0, only id 60, a byte's edge, the two mask words' edge, all 61, none, all 64 bits (61..63 are ignored)
EDGE_MASKS = [[0], [60], [7, 8], [31, 32], range(A), [], range(64)]


def test_wide_mask_edges(vec):
    v = vec
    R = 70                                                      # a block and a partial one
    ids_of = [[a for a in EDGE_MASKS[r % len(EDGE_MASKS)] if a < A] for r in range(R)]
    legal = dev(v, np.stack([bits(EDGE_MASKS[r % len(EDGE_MASKS)]) for r in range(R)]))
    obs = torch.ones((R, D), dtype=torch.uint8, device=v.device)
    rng = np.random.RandomState(3)
    flat = np.full(A, 0.5, np.float32)
    peaks = (rng.rand(A) - 2).astype(np.float32)                # distinct values below the two equal maxima
    peaks[[33, 60]] = 1.25
    for bias, pick in ((flat, min), (peaks, lambda ids: 33 if 33 in ids else (60 if 60 in ids else
                                                                                 max(ids, key=lambda a: peaks[a])))):
        net = BiasNet(v.device, bias)
        q = torch.empty((R, A), dtype=torch.float32, device=v.device)
        got = qnet_actions(v, net, obs, legal, q=q).cpu().numpy()
        qh = q.cpu().numpy()
        for r in range(R):
            want = np.full(A, -np.inf, np.float32)
            want[ids_of[r]] = bias[ids_of[r]]
            assert np.array_equal(qh[r], want), (r, ids_of[r])                   # the biases exactly
            assert got[r] == (pick(ids_of[r]) if ids_of[r] else -1), (r, ids_of[r], got[r])
        assert np.array_equal(qnet_values(v, net, obs, legal).cpu().numpy(), qh)
        assert np.array_equal(qnet_values(v, net, obs, None).cpu().numpy(), np.tile(bias, (R, 1)))
        # epsilon 1: a uniform legal id, whatever the mask's upper bits say
        drawn = qnet_actions(v, net, obs, legal, None, 1.0, 9, 4, 100).cpu().numpy()
        for r in range(R):
            assert (drawn[r] in ids_of[r]) if ids_of[r] else drawn[r] == -1
        full = [r for r in range(R) if len(ids_of[r]) == A]
        assert len(set(drawn[full])) > 5 and max(drawn[full]) < A


# ---- actions ----------------------------------------------------------------------------------------------------------
def test_wide_actions(gold, vec):
    """tests/test_gpu_dqn.py test_qnet_actions on the fixture's UNO rows."""
    from rlcard_amd.agents.dmc_agent import select_actions
    v = vec
    c = value_case(gold, v, 'fixture')
    est, obs = c['dev'], c['obs']
    R = obs.shape[0]
    legal = c['legal'].clone()
    done = torch.zeros(R, dtype=torch.uint8, device=v.device)
    legal[3::17] = 0
    done[5::13] = 1
    m = c['mask'].copy()
    m[3::17] = False
    dn = done.cpu().numpy().astype(bool)
    q = torch.empty((R, A), dtype=torch.float32, device=v.device)
    greedy = qnet_actions(v, est, obs, legal, done, q=q).cpu().numpy()
    qh = q.cpu().numpy()
    assert np.all(qh[~m] == -np.inf) and np.array_equal(qh[m], qnet_values(v, est, obs, legal).cpu().numpy()[m])
    none = ~m.any(axis=1)
    assert none.any() and dn.any() and (~(none | dn)).sum() > R // 2
    assert np.all(greedy[none | dn] == -1)
    live = ~(none | dn)
    assert np.array_equal(greedy[live], np.argmax(qh, axis=1)[live])          # first maximum of the kernel's own row
    e_torch = np.abs(c['q_torch'] - c['ref64'])[c['mask']].max()
    r64 = np.where(m, c['ref64'], -np.inf)
    top = np.sort(r64, axis=1)
    with np.errstate(invalid='ignore'):
        clear = live & ((top[:, -1] - top[:, -2]) > 16 * e_torch)
    assert (live & ~clear).sum() <= live.sum() // 100
    assert np.array_equal(greedy[clear], np.argmax(r64, axis=1)[clear])
    assert (greedy[clear] > 8).any()
    g2 = qnet_actions(v, est, obs, legal).cpu().numpy()
    assert np.array_equal(g2 == -1, none) and np.array_equal(g2[live], greedy[live])
    # epsilon draws: cs_dmc_select fed the same values through legal_lists, bit for bit
    counts, offsets, ids = v.legal_lists(legal)
    state_of = torch.repeat_interleave(torch.arange(R, device=v.device), counts.long())
    values = q[state_of, ids.long()].contiguous()
    multi = live & (m.sum(axis=1) > 1)
    for eps, seed, t, base in ((0.3, 7, 11, 1000), (1.0, 2 ** 40 + 3, 2 ** 33, 5), (0.0, 1, 2, 3)):
        got = qnet_actions(v, est, obs, legal, None, eps, seed, t, base).cpu().numpy()
        want = select_actions(values, counts, offsets, ids, eps, seed, t, base).cpu().numpy()
        assert np.array_equal(got, want), eps
        if eps == 1.0:
            assert (got[multi] != greedy[multi]).any()
            assert all(m[r, got[r]] for r in np.nonzero(~none)[0])


# ---- average policy ---------------------------------------------------------------------------------------------------
_pcache = {}


def policy_case(gold_nfsp, v):
    """The fixture's average-policy network on its 256 rows. The reference for a row is the fp64 chain, or, where the
    row's legal mass underflows entirely in fp32 (every legal logit >= 106 below the maximum), the uniform row the
    reference's fp32 chain falls back to. Hazard rows -- the best legal logit 86 to 106 below the maximum, by these
    fp64 logits: exp() is denormal in fp32 there, and a device expf that flushes denormals gives the fallback where
    the reference renormalises -- are left out of the comparisons with the fp64 chain."""
    from rlcard_amd.utils import remove_illegal
    if _pcache:
        return _pcache
    g = gold_nfsp
    cpu = uno_policy_net(g)
    x, lg = g['uno_obs'], g['uno_legal']
    m = mask_of(lg, A)
    logits = unfolded_logits64(cpu, x)
    best = np.where(m, logits.max(axis=1, keepdims=True) - logits, np.inf).min(axis=1)
    hazard, gone = (best >= 86) & (best <= 106), best > 106
    uni = m / m.sum(axis=1, keepdims=True)
    ref64 = np.where(gone[:, None], uni, probs64(logits, m))
    with torch.no_grad():
        p32 = np.exp(cpu(torch.from_numpy(x).float()).numpy())
    p_torch = np.stack([remove_illegal(p32[r], np.nonzero(m[r])[0]) for r in range(ROWS)])
    _pcache.update(cpu=cpu, net=policy_on_device(cpu, v.device), obs=dev(v, x), legal=dev(v, lg), mask=m,
                   logits=logits, ref64=ref64, p_torch=p_torch, hazard=hazard, gone=gone)
    return _pcache


def test_wide_probs(gold_nfsp, vec):
    """E_kernel <= 8 E_torch + 4 ulp(1) on the rows that are no hazard rows (tests/test_gpu_nfsp.py's bound); illegal
    entries exactly 0; row sums within (A + 4) 2^-24 of 1 (a sequential fp32 sum of <= A terms carries (A - 1) u, the
    two divisions u each; the narrow test's 8 ulp is this at A = 4); fully underflowed rows exactly 1 / count.
    Measured on the MI355X: E_torch 7.212e-07, E_kernel 5.757e-06, ratio 7.98 (bound 6.008e-06); with the first bias
    folded from the float64 weights instead of the float32 ones the descriptor holds it was 6.194e-06, ratio 8.59
    (profiles/EXPERIMENTS.md W-1)."""
    c = policy_case(gold_nfsp, vec)
    m, keep = c['mask'], ~c['hazard']
    assert c['hazard'].sum() <= ROWS * 5 // 100 and c['gone'].any()
    p = pnet_probs(vec, c['net'], c['obs'], c['legal']).cpu().numpy()
    assert np.all(p[~m] == 0) and np.all(p[m] >= 0)
    worst = np.abs(p.astype(np.float64).sum(axis=1) - 1).max()
    assert worst <= (A + 4) * ULP
    e_torch = np.abs(c['p_torch'] - c['ref64'])[keep].max()
    e_kernel = np.abs(p.astype(np.float64) - c['ref64'])[keep].max()
    print('uno fixture policy: %d hazard rows, %d underflowed; E_torch %.3e E_kernel %.3e ratio %.2f (bound %.3e), '
          'row sums within %.1f ulp' % (c['hazard'].sum(), c['gone'].sum(), e_torch, e_kernel,
                                        e_kernel / max(e_torch, 1e-300), 8 * e_torch + 4 * ULP, worst / ULP))
    for r in np.nonzero(c['gone'])[0]:
        want = np.where(m[r], np.float32(1) / np.float32(m[r].sum()), np.float32(0))
        assert np.array_equal(p[r], want), r
    assert np.array_equal(p[c['gone']], gold_nfsp['uno_legal_probs'][c['gone']].astype(np.float32))
    # no mask: the softmax over every action
    p_all = pnet_probs(vec, c['net'], c['obs'], None).cpu().numpy()
    every = probs64(c['logits'], np.ones_like(m))
    with torch.no_grad():
        t_all = np.exp(c['cpu'](torch.from_numpy(gold_nfsp['uno_obs']).float()).numpy()).astype(np.float64)
    e_torch_all = np.abs(t_all - every).max()
    e_kernel_all = np.abs(p_all.astype(np.float64) - every).max()
    print('uno fixture policy, no mask: E_torch %.3e E_kernel %.3e' % (e_torch_all, e_kernel_all))
    assert e_kernel_all <= 8 * e_torch_all + 4 * ULP
    assert e_kernel <= 8 * e_torch + 4 * ULP


def test_wide_underflow_falls_back_to_uniform(vec):
    """Logit 200 on id 40, 0 elsewhere: with id 40 illegal the legal mass is exp(-200) = 0 in fp32 and the row is
    exactly 1 / count on the legal ids, at 1, 2 and 60 of them; with all 61 legal the row is that action."""
    v = vec
    bias = np.zeros(A)
    bias[40] = 200.0
    net = BiasNet(v.device, bias)
    sets = [[60], [0, 33], [a for a in range(A) if a != 40], list(range(A)), [39, 41], [40, 60]]
    R = 66
    legal = dev(v, np.stack([bits(sets[r % len(sets)]) for r in range(R)]))
    obs = torch.ones((R, D), dtype=torch.uint8, device=v.device)
    p = pnet_probs(v, net, obs, legal).cpu().numpy()
    for r in range(R):
        ids = sets[r % len(sets)]
        want = np.zeros(A, np.float32)
        if 40 in ids:
            want[40] = 1
        else:
            want[ids] = np.float32(1) / np.float32(len(ids))
        assert np.array_equal(p[r], want), (r, ids, p[r])


def test_wide_sampled_actions(gold_nfsp, vec):
    c = policy_case(gold_nfsp, vec)
    v, net, obs = vec, c['net'], c['obs']
    legal = c['legal'].clone()
    done = torch.zeros(ROWS, dtype=torch.uint8, device=v.device)
    legal[3::17] = 0
    done[5::13] = 1
    m = c['mask'].copy()
    m[3::17] = False
    dn = done.cpu().numpy().astype(bool)
    live = m.any(axis=1)
    seen = set()
    for seed, t, base in ((7, 11, 1000), (2 ** 40 + 3, 2 ** 33 + 1, 2 ** 35 + 5), (1, 2, 3)):
        probs = torch.full((ROWS, A), -1.0, dtype=torch.float32, device=v.device)
        got = nfsp_actions(v, None, net, obs, legal, done, None, 0.0, seed, t, base, probs).cpu().numpy()
        ph = probs.cpu().numpy()
        assert np.array_equal(ph[live], pnet_probs(v, net, obs, legal).cpu().numpy()[live])
        assert np.array_equal(got, sample_ref(ph, m, dn, seed, t, base)), (seed, t, base)
        assert np.all(got[~live | dn] == -1) and all(m[r, got[r]] for r in np.nonzero(live & ~dn)[0])
        seen.add(got.tobytes())
    assert len(seen) == 3                               # the draws depend on the key


# ---- row lists --------------------------------------------------------------------------------------------------------
def test_wide_row_lists(gold, gold_nfsp, vec):
    v = vec
    R = 130
    cq, cp = value_case(gold, v, 'fixture'), policy_case(gold_nfsp, v)
    est, net = cq['dev'], cp['net']
    obs = cq['obs'][:R].contiguous()
    legal = cq['legal'][:R].clone()
    done = torch.zeros(R, dtype=torch.uint8, device=v.device)
    legal[3::17] = 0
    done[5::13] = 1
    rng = np.random.RandomState(4)
    modes = {'mixed': (rng.rand(R) < 0.4).astype(np.uint8), 'all 0': np.zeros(R, np.uint8), 'all 1': np.ones(R, np.uint8)}
    assert 20 < modes['mixed'].sum() < R - 20
    eps, seed, t, base = 0.3, 2 ** 40 + 3, 2 ** 33, 77
    SENT = -3.0
    br = qnet_actions(v, est, obs, legal, done, eps, seed, t, base).cpu().numpy()
    p_avg = torch.full((R, A), SENT, dtype=torch.float32, device=v.device)
    avg = nfsp_actions(v, None, net, obs, legal, done, None, eps, seed, t, base, p_avg).cpu().numpy()
    p_avg = p_avg.cpu().numpy()
    assert np.all(p_avg != SENT) and (br != avg).any()
    for name, mode in modes.items():
        mh = mode.astype(bool)
        probs = torch.full((R, A), SENT, dtype=torch.float32, device=v.device)
        got = nfsp_actions(v, est, net, obs, legal, done, dev(v, mode), eps, seed, t, base, probs).cpu().numpy()
        ph = probs.cpu().numpy()
        assert np.array_equal(got[mh], br[mh]), name               # cs_qnet_actions, bit for bit
        assert np.array_equal(got[~mh], avg[~mh]), name            # the all-average call
        assert np.all(ph[mh] == SENT) and np.array_equal(ph[~mh], p_avg[~mh]), name


# ---- refusals ---------------------------------------------------------------------------------------------------------
def test_wide_refusals(gold, gold_nfsp, vec):
    from rlcard_amd import VecEnv, _abi
    from rlcard_amd.agents import DeviceMemory, DeviceReservoir
    v = vec
    est = value_case(gold, v, 'fixture')['dev']
    net = policy_case(gold_nfsp, v)['net']
    ddz = VecEnv('doudizhu', 2, seed=1)
    obs = torch.zeros((64, 901), dtype=torch.uint8, device=v.device)
    for call in (lambda: qnet_values(ddz, est, obs, None), lambda: pnet_probs(ddz, net, obs, None),
                 lambda: DeviceMemory(ddz, 16), lambda: DeviceReservoir(ddz, 16)):
        with pytest.raises(_abi.CardsimError, match='CS_E_UNSUPPORTED'):
            call()
    leduc = VecEnv('leduc-holdem', 64, seed=1)
    with pytest.raises(_abi.CardsimError, match='CS_E_INVALID'):       # in_dim 240 on a 36-byte game
        qnet_values(leduc, est, obs, None)
    q = torch.empty((64, A), dtype=torch.float32, device=v.device)
    bad = _abi.QNet.from_buffer_copy(est.folded())
    bad.hidden[0] = 129
    assert _abi.lib().cs_qnet_values(v._h, C.byref(bad), _ptr(obs), None, 64, _ptr(q), None) == -1
    # the largest descriptor the struct allows runs
    big = on_device(random_estimator(A, D, [128, 128, 128, 128], 6, 'cpu'), v.device)
    rows = value_case(gold, v, 'fixture')
    got = qnet_values(v, big, rows['obs'][:65].contiguous(), rows['legal'][:65].contiguous()).cpu().numpy()
    assert np.isfinite(got[rows['mask'][:65]]).all() and np.all(got[~rows['mask'][:65]] == -np.inf)
