"""The agent kernels on Mahjong -- 816 obs bytes, 38 actions, 5 mask bytes, 4 seats -- where the wide instantiations
of the network kernel (rlcard_amd/csrc/cs_dqn.hip) take paths UNO's 240 / 61 / 8 / 2 cannot reach: an obs row of 204
dwords, longer than the block, so the staging's (row, unit) walk advances by its wrap alone; more than 64 KiB of
dynamic LDS for every net; mask rows of 5 bytes, not dword-aligned, with bits 38 and 39 no actions; a [row][38] head
image. And the replay ring, the reservoir and a collector with four seats, a seat's next row typically four rows on.
The rows are a device rollout's (pinned to the reference by tests/golden/mahjong.npz); the restatements and the bounds
are tests/test_gpu_dqn.py's, tests/test_gpu_nfsp.py's and tests/test_gpu_qnet_wide.py's. Needs a GPU."""
import numpy as np
import pytest

from test_dqn import unfolded64
from test_gpu_dqn import RefReplay, assert_same, held, on_device, qnet_actions, qnet_values, random_estimator
from test_gpu_nfsp import ULP, RefReservoir, assert_same_reservoir, nfsp_actions, pnet_probs, random_policy_net
from test_gpu_nfsp import held as held_reservoir
from test_gpu_nfsp import on_device as policy_on_device
from test_gpu_nfsp import philox4, sample_ref
from test_nfsp import mask_of, probs64, unfolded_logits64

torch = pytest.importorskip('torch')
pytestmark = pytest.mark.gpu
N = 65      # a wave of envs and one more
D, A, LB, P = 816, 38, 5, 4


@pytest.fixture(scope='module', autouse=True)
def _need_gpu():
    if not torch.cuda.is_available():
        pytest.fail('GPU tests need a visible GPU (run them on the MI355X box)')


@pytest.fixture(scope='module')
def rows():
    """The first 130 rows of a 128-step random rollout: 65 are a partial block, 130 two blocks and two rows."""
    from rlcard_amd import VecEnv
    v = VecEnv('mahjong', N, seed=5)
    assert (v.obs_dim, v.num_actions, v.legal_bytes, v.num_players) == (D, A, LB, P)
    v.reset()
    tr = v.rollout(128, policy_seed=9, final_obs=True)
    obs = tr['obs'].reshape(-1, D)[:130].contiguous()
    legal = tr['legal'].reshape(-1, LB)[:130].contiguous()
    x, lg = obs.cpu().numpy(), legal.cpu().numpy()
    return dict(v=v, obs=obs, legal=legal, x=x, mask=mask_of(lg, A))


def dev(v, x):
    return torch.from_numpy(np.ascontiguousarray(x)).to(v.device)


# ---- values -----------------------------------------------------------------------------------------------------------
# one wave and the least LDS a Mahjong net takes (79 616 B); two waves; an output tile of K = 20, no multiple of the
# 16-unit stage; four layers, whose output tile lands in the other buffer than with one; one 128-unit layer
NETS = {'64': ([64], 1), '128-128-64': ([128, 128, 64], 2), '20': ([20], 3), '7-5-3-2': ([7, 5, 3, 2], 4),
        '128': ([128], 5)}
_cache = {}


def value_case(rows, name):
    """-> the CPU and device estimators and the fp64 / torch-CPU fp32 forwards of the 130 rows (computed once)"""
    if name not in _cache:
        cpu = random_estimator(A, D, NETS[name][0], NETS[name][1], 'cpu')
        _cache[name] = dict(cpu=cpu, dev=on_device(cpu, rows['v'].device), ref64=unfolded64(cpu, rows['x']),
                            q_torch=cpu.predict_nograd(rows['x'].astype(np.float32)).astype(np.float64))
    return _cache[name]


@pytest.mark.parametrize('name', list(NETS))
def test_mahjong_values(rows, name):
    """tests/test_gpu_qnet_wide.py test_wide_values' checks: E_kernel <= 8 E_torch over the legal entries, illegal
    entries exactly -inf, without a mask the same numbers. Measured on the MI355X: profiles/EXPERIMENTS.md W-2."""
    v, c = rows['v'], value_case(rows, name)
    for R in (65, 130):
        obs, legal, m = rows['obs'][:R].contiguous(), rows['legal'][:R].contiguous(), rows['mask'][:R]
        q = qnet_values(v, c['dev'], obs, legal).cpu().numpy()
        assert q.shape == (R, A) and m.any(axis=1).all() and not m.all(axis=1).any()
        assert np.all(q[~m] == -np.inf) and np.isfinite(q[m]).all()
        e_torch = np.abs(c['q_torch'][:R] - c['ref64'][:R])[m].max()
        e_kernel = np.abs(q.astype(np.float64) - c['ref64'][:R])[m].max()
        print('mahjong %s, %d rows: E_torch %.3e E_kernel %.3e ratio %.2f |q| <= %.2f'
              % (name, R, e_torch, e_kernel, e_kernel / e_torch, np.abs(c['ref64'][:R][m]).max()))
        assert e_kernel <= 8 * e_torch
        q_all = qnet_values(v, c['dev'], obs, None).cpu().numpy()
        assert np.isfinite(q_all).all() and np.array_equal(q_all[m], q[m])
        e_all = np.abs(q_all.astype(np.float64) - c['ref64'][:R]).max()
        e_torch_all = np.abs(c['q_torch'][:R] - c['ref64'][:R]).max()
        assert e_all <= 8 * e_torch_all


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


def bits(ids):
    m = np.zeros(8 * LB, np.uint8)
    m[list(ids)] = 1
    return np.packbits(m, bitorder='little')


# only id 0, only id 37, a byte's edge, the dword's edge inside the 5-byte row, all 38, none, all 40 bits (38 and 39 are
# ignored)
EDGE_MASKS = [[0], [37], [7, 8], [31, 32], range(A), [], range(40)]


def test_mahjong_mask_edges(rows):
    """Consecutive rows carry different masks, so a row stride other than 5 bytes shows."""
    v = rows['v']
    R = 70                                                      # a block and a partial one
    ids_of = [[a for a in EDGE_MASKS[r % len(EDGE_MASKS)] if a < A] for r in range(R)]
    legal = dev(v, np.stack([bits(EDGE_MASKS[r % len(EDGE_MASKS)]) for r in range(R)]))
    assert legal.shape == (R, LB)
    obs = torch.ones((R, D), dtype=torch.uint8, device=v.device)
    rng = np.random.RandomState(3)
    flat = np.full(A, 0.5, np.float32)
    peaks = (rng.rand(A) - 2).astype(np.float32)                # distinct values below the two equal maxima
    peaks[[33, 37]] = 1.25
    for bias, pick, key in ((flat, min, (9, 4, 100)),
                            (peaks, lambda ids: 33 if 33 in ids else (37 if 37 in ids else
                                                                      max(ids, key=lambda a: peaks[a])),
                             (2 ** 40 + 3, 2 ** 33, 5))):
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
        # epsilon 1: the draw restated (include/cardsim.h cs_qnet_actions) -- the ((r[1] * count) >> 32)-th legal id of
        # Philox on (row_base + row, t), count the legal ids below A whatever the mask's upper bits say. On some of the
        # rows with all 40 bits set a count of 40 picks another id, so a mask that keeps bits 38 and 39 shows
        seed, t, base = key
        r1 = philox4(seed, np.uint64(base) + np.arange(R, dtype=np.uint64), t)[1].astype(np.uint64)
        kth = lambda r, count: int((int(r1[r]) * count) >> 32)
        want = np.array([ids_of[r][kth(r, len(ids_of[r]))] if ids_of[r] else -1 for r in range(R)], np.int32)
        over = [r for r in range(R) if len(EDGE_MASKS[r % len(EDGE_MASKS)]) == 40]
        assert sum(kth(r, 40) >= A or kth(r, 40) != kth(r, A) for r in over) >= 3
        drawn = qnet_actions(v, net, obs, legal, None, 1.0, seed, t, base).cpu().numpy()
        assert np.array_equal(drawn, want), key
        full = [r for r in range(R) if len(ids_of[r]) == A]
        assert len(set(drawn[full])) > 5 and max(drawn[full]) < A
    # the softmax head counts the legal ids too: logit 200 on id 5, illegal, under all 40 bits but that one -- the legal
    # mass underflows and the row is exactly 1 / 37 on the 37 legal ids (tests/test_gpu_qnet_wide.py's fallback test)
    bias = np.zeros(A)
    bias[5] = 200.0
    sets = [[a for a in range(40) if a != 5], [0, 37], list(range(40)), [4, 6, 38, 39]]
    lg = dev(v, np.stack([bits(sets[r % len(sets)]) for r in range(R)]))
    p = pnet_probs(v, BiasNet(v.device, bias), obs, lg).cpu().numpy()
    for r in range(R):
        ids = [a for a in sets[r % len(sets)] if a < A]
        want = np.zeros(A, np.float32)
        if 5 in ids:
            want[5] = 1
        else:
            want[ids] = np.float32(1) / np.float32(len(ids))
        assert np.array_equal(p[r], want), (r, ids, p[r])


# ---- actions ----------------------------------------------------------------------------------------------------------
def test_mahjong_actions(rows):
    """tests/test_gpu_dqn.py test_qnet_actions on the 130 rows with the two-wave net."""
    from rlcard_amd.agents.dmc_agent import select_actions
    v, c = rows['v'], value_case(rows, '128-128-64')
    est, obs = c['dev'], rows['obs']
    R = obs.shape[0]
    legal = rows['legal'].clone()
    done = torch.zeros(R, dtype=torch.uint8, device=v.device)
    legal[3::17] = 0
    done[5::13] = 1
    m = rows['mask'].copy()
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
    # the fp64 argmax wherever its top-two legal gap is clear of the fp32 error
    e_torch = np.abs(c['q_torch'] - c['ref64'])[rows['mask']].max()
    r64 = np.where(m, c['ref64'], -np.inf)
    top = np.sort(r64, axis=1)
    with np.errstate(invalid='ignore'):     # (rows without a legal action: -inf - -inf; they are not live)
        clear = live & ((top[:, -1] - top[:, -2]) > 16 * e_torch)
    assert (live & ~clear).sum() <= R // 100
    assert np.array_equal(greedy[clear], np.argmax(r64, axis=1)[clear])
    # no done pointer: only the empty masks give -1
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
PNETS = {'64': ([64], 1), '128-128': ([128, 128], 2)}
_pcache = {}


def policy_case(rows, name):
    """A seeded random average-policy network with the fp64 chain and the torch-CPU fp32 chain of the 130 rows. No row
    is near fp32's underflow (tests/test_gpu_qnet_wide.py policy_case's hazard rows): the best legal logit lies within
    86 of the maximum."""
    from rlcard_amd.utils import remove_illegal
    if name not in _pcache:
        cpu = random_policy_net(A, D, PNETS[name][0], PNETS[name][1])
        x, m = rows['x'], rows['mask']
        logits = unfolded_logits64(cpu, x)
        assert np.where(m, logits.max(axis=1, keepdims=True) - logits, np.inf).min(axis=1).max() < 86
        with torch.no_grad():
            p32 = np.exp(cpu(torch.from_numpy(x).float()).numpy())      # NFSPAgent._act
        assert p32.dtype == np.float32
        p_torch = np.stack([remove_illegal(p32[r], np.nonzero(m[r])[0]) for r in range(len(x))])
        _pcache[name] = dict(cpu=cpu, net=policy_on_device(cpu, rows['v'].device), logits=logits,
                             ref64=probs64(logits, m), p_torch=p_torch)
    return _pcache[name]


@pytest.mark.parametrize('name', list(PNETS))
def test_mahjong_probs(rows, name):
    """tests/test_gpu_nfsp.py test_pnet_probs' bound, E_kernel <= 8 E_torch + 4 ulp(1); illegal entries exactly 0; row
    sums within (A + 4) 2^-24 of 1 (tests/test_gpu_qnet_wide.py test_wide_probs). Measured: EXPERIMENTS.md W-2."""
    v, c = rows['v'], policy_case(rows, name)
    for R in (65, 130):
        obs, legal, m = rows['obs'][:R].contiguous(), rows['legal'][:R].contiguous(), rows['mask'][:R]
        p = pnet_probs(v, c['net'], obs, legal).cpu().numpy()
        assert m.any(axis=1).all()
        assert np.all(p[~m] == 0) and np.all(p[m] >= 0)
        assert np.abs(p.astype(np.float64).sum(axis=1) - 1).max() <= (A + 4) * ULP
        e_torch = np.abs(c['p_torch'][:R] - c['ref64'][:R]).max()
        e_kernel = np.abs(p.astype(np.float64) - c['ref64'][:R]).max()
        print('mahjong policy %s, %d rows: E_torch %.3e E_kernel %.3e ratio %.2f (bound %.3e)'
              % (name, R, e_torch, e_kernel, e_kernel / e_torch, 8 * e_torch + 4 * ULP))
        assert e_kernel <= 8 * e_torch + 4 * ULP
        # no mask: the softmax over every action
        p_all = pnet_probs(v, c['net'], obs, None).cpu().numpy()
        every = probs64(c['logits'][:R], np.ones_like(m))
        assert np.abs(p_all.astype(np.float64) - every).max() <= 8 * e_torch + 4 * ULP


@pytest.mark.parametrize('name', list(PNETS))
def test_mahjong_sampled_actions(rows, name):
    """tests/test_gpu_nfsp.py test_sampled_actions_match_the_restated_draw."""
    v, c = rows['v'], policy_case(rows, name)
    net, obs = c['net'], rows['obs']
    R = obs.shape[0]
    legal = rows['legal'].clone()
    done = torch.zeros(R, dtype=torch.uint8, device=v.device)
    legal[3::17] = 0
    done[5::13] = 1
    m = rows['mask'].copy()
    m[3::17] = False
    dn = done.cpu().numpy().astype(bool)
    live = m.any(axis=1)
    seen = set()
    for seed, t, base in ((7, 11, 1000), (2 ** 40 + 3, 2 ** 33 + 1, 2 ** 35 + 5), (1, 2, 3)):
        probs = torch.full((R, A), -1.0, dtype=torch.float32, device=v.device)
        got = nfsp_actions(v, None, net, obs, legal, done, None, 0.0, seed, t, base, probs).cpu().numpy()
        ph = probs.cpu().numpy()
        assert np.array_equal(ph[live], pnet_probs(v, net, obs, legal).cpu().numpy()[live])
        assert np.array_equal(got, sample_ref(ph, m, dn, seed, t, base)), (seed, t, base)
        assert np.all(got[~live | dn] == -1) and all(m[r, got[r]] for r in np.nonzero(live & ~dn)[0])
        seen.add(got.tobytes())
    assert len(seen) == 3                               # the draws depend on the key
    # no done pointer: only the empty masks give -1
    g2 = nfsp_actions(v, None, net, obs, legal, None, None, 0.0, 7, 11, 1000).cpu().numpy()
    assert np.array_equal(g2 == -1, ~live)


# ---- row lists --------------------------------------------------------------------------------------------------------
def test_mahjong_row_lists(rows):
    """tests/test_gpu_nfsp.py test_each_network_runs_on_its_own_rows on the 130 rows: each network's rows are those of
    that network run alone, bit for bit. In the last mode neither list's length (65, 65) is a multiple of 64."""
    v = rows['v']
    R = 130
    est, net = value_case(rows, '64')['dev'], policy_case(rows, '128-128')['net']
    obs = rows['obs']
    legal = rows['legal'].clone()
    done = torch.zeros(R, dtype=torch.uint8, device=v.device)
    legal[3::17] = 0
    done[5::13] = 1
    rng = np.random.RandomState(4)
    modes = {'mixed': (rng.rand(R) < 0.4).astype(np.uint8), 'all 0': np.zeros(R, np.uint8),
             'all 1': np.ones(R, np.uint8), '65 + 65': np.repeat(np.array([1, 0], np.uint8), 65)}
    assert 20 < modes['mixed'].sum() < R - 20 and modes['mixed'].sum() % 64 and (R - modes['mixed'].sum()) % 64
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
        # probs NULL: the same actions
        g2 = nfsp_actions(v, est, net, obs, legal, done, dev(v, mode), eps, seed, t, base).cpu().numpy()
        assert np.array_equal(g2, got), name


# ---- replay -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('seats', [(0, 1, 2, 3), (0, 2)], ids=['all', 'seats02'])
def test_mahjong_replay_matches_reorganize(seats):
    """tests/test_gpu_dqn.py test_replay_matches_reorganize_with_carry with four seats: everything held, a ring that
    wraps, and one that every push overflows."""
    from rlcard_amd import VecEnv
    from rlcard_amd.agents import DeviceMemory
    v = VecEnv('mahjong', N, seed=21)
    v.reset()
    caps = (1 << 16, 1000, 97)
    mems = [DeviceMemory(v, cap) for cap in caps]
    ref = RefReplay(P, D, LB)
    tr = v.new_traj_out(64, final_obs=True, select=1)
    carried = []
    for w in range(2):
        v.rollout(64, policy_seed=3, t0=64 * w, out=tr)
        for mem in mems:
            mem.push(tr, seats)
        before = len(ref.out)
        ref.push({k: x.cpu().numpy() for k, x in tr.items()}, seats)
        carried.append(len(ref.pending))
        assert len(ref.out) - before > caps[1]                  # the push overflows the two smaller rings
        for mem, cap in zip(mems, caps):
            assert mem.sizes() == (min(len(ref.out), cap), len(ref.out))
    assert carried[0] > 0                                       # transitions straddle the window edge ...
    want = ref.held(caps[0])
    assert len(ref.out) < caps[0]
    assert want['done'].any() and not want['done'].all()        # ... and games finished inside the windows
    assert np.all(want['next_legal'][want['done'] == 1] == 0) and np.all(want['reward'][want['done'] == 0] == 0)
    assert want['next_legal'].shape[1] == LB and (want['next_legal'][:, 4] != 0).any()      # (ids 32..37)
    assert not np.unpackbits(want['next_legal'], axis=1, bitorder='little')[:, A:].any()
    for mem, cap in zip(mems, caps):
        assert_same(held(mem), ref.held(cap), 'capacity %d' % cap)


# ---- reservoir --------------------------------------------------------------------------------------------------------
def test_mahjong_reservoir_matches_sequential_add():
    """tests/test_gpu_uno_agents.py test_reservoir_matches_sequential_add_on_uno with four seats."""
    from rlcard_amd import VecEnv
    from rlcard_amd.agents import DeviceReservoir
    v = VecEnv('mahjong', N, seed=21)
    v.reset()
    g = torch.Generator().manual_seed(6)
    seed = 2 ** 40 + 9
    seats = (0, 1, 2, 3)
    caps = (1 << 14, 64)
    res = [DeviceReservoir(v, cap, seed) for cap in caps]
    refs = [RefReservoir(cap, seed, P) for cap in caps]
    for w in range(3):
        tr = v.rollout(16, policy_seed=3, t0=16 * w, final_obs=True)
        mode = (torch.rand((16, N), generator=g) < 0.5).to(torch.uint8).to(v.device)
        wh, mh = {k: x.cpu().numpy() for k, x in tr.items()}, mode.cpu().numpy()
        for r_, ref in zip(res, refs):
            r_.push(tr, mode, seats)
            assert ref.push(wh, mh, seats) > 64
            assert_same_reservoir(r_, ref, A, 'capacity %d after push %d' % (ref.cap, w))
    assert refs[0].dropped == 0 == refs[0].collisions and refs[1].collisions > 0 and refs[1].dropped > 0
    st, pr = held_reservoir(res[1])
    assert st.shape == (64, D) and pr.shape == (64, A)


# ---- collector --------------------------------------------------------------------------------------------------------
def test_mahjong_dqn_collector_with_the_fused_learner():
    """The epsilon policy kernel and the learner together on this game: two runs leave the same memory."""
    from rlcard_amd import VecEnv
    from rlcard_amd.agents import DQNAgent, DQNCollector
    runs = []
    for _ in range(2):
        v = VecEnv('mahjong', N, seed=31)
        torch.manual_seed(1)
        agent = DQNAgent(num_actions=A, state_shape=[D], mlp_layers=[64, 64], replay_memory_size=4096,
                         replay_memory_init_size=100, batch_size=32, update_target_estimator_every=1000,
                         epsilon_decay_steps=2000, learning_rate=1e-3, device=v.device)
        agent.attach(v)
        col = DQNCollector(v, agent, seats=(0,), opponents='random', steps_per_feed=32, seed=5)
        losses = col.run(train_steps=2, fused=True)
        assert losses.shape == (2,) and losses.is_cuda and torch.isfinite(losses).all() and agent.train_t == 2
        got = held(agent.device_memory)
        assert agent.total_t == len(got['action']) > 300
        assert got['state'].shape[1] == D and got['next_legal'].shape[1] == LB
        assert not np.unpackbits(got['next_legal'], axis=1, bitorder='little')[:, A:].any()
        runs.append((got, losses.cpu()))
    assert_same(runs[0][0], runs[1][0], 'two runs')
    assert torch.equal(runs[0][1], runs[1][1])
