// cs_abi.cpp -- the extern "C" boundary (include/cardsim.h): handle lifetime, argument validation, error codes,
// stream plumbing. No exceptions cross it; HIP errors become CS_E_DEVICE with the runtime's message.
#include <hip/hip_runtime.h>
#include <stdio.h>
#include <string.h>
#include <new>
#include <string>
#include "cs_engine.h"
#include "cs_doudizhu.h"
#include "cs_dqn.h"

namespace cs {
namespace ddz {
std::string table_create(void** dev, Tab* tab);
}
}  // namespace cs

struct cs_handle {
    cs::Buffers b;
    const cs::GameOps* ops;   // the game type's launchers, cs_game_info and buffer layouts (cs::find_game at cs_create)
    int32_t device;
    bool seeded;
    void* table_dev;     // doudizhu: device action table (one allocation)
    cs::ddz::Tab tab;    // doudizhu: views into it, passed to the kernels by value
    cs::DevBuf scan;     // cs_legal_lists: prefix-scan scratch, grown on demand
    cs::DevBuf cfr;      // cs_cfr_train with n > 1: the ordered reduction's records and sort buffers
};

// What the buffers created on a handle (cs_dmc, cs_replay, cs_reservoir) share. A buffer may outlive its handle only
// to be destroyed: destroy uses `device`, never `h`.
struct cs_sub {
    cs_handle* h;
    int32_t device;      // h->device, copied at create
    cs::DevBuf mem;      // one allocation carved into the buffer's parts
    cs::DevBuf scratch;  // per-call scratch sized by the call's window, grown on demand
    cs::DevBuf scan;     // prefix-scan scratch, grown on demand
};

namespace {
thread_local std::string g_err;

int fail(int code, const char* msg)
{
    g_err = msg;
    return code;
}

int fail_hip(hipError_t e, const char* where)
{
    g_err = std::string(where) + ": " + hipGetErrorString(e);
    return CS_E_DEVICE;
}

int done(hipError_t e, const char* where) { return e == hipSuccess ? CS_OK : fail_hip(e, where); }

int set_device(const cs_handle* h) { return done(hipSetDevice(h->device), "hipSetDevice"); }

// cs_reset / cs_step / cs_observe under a step record: the call publishes the next sequence number, and a launch that
// failed published nothing
template <class Launch>
int recorded(cs_handle* h, const char* name, Launch launch)
{
    if (h->b.rec.seq) h->b.rec.seqv++;
    const hipError_t e = launch();
    if (e != hipSuccess && h->b.rec.seq) h->b.rec.seqv--;
    return done(e, name);
}

// A buffer of handle h: its one allocation of `total` bytes, zeroed from byte `zero_from` on
template <class S>
int sub_create(cs_handle* h, size_t total, size_t zero_from, const char* name, S** out)
{
    S* s = new (std::nothrow) S();
    if (!s) return fail(CS_E_INVALID, "out of host memory");
    s->h = h;
    s->device = h->device;
    hipError_t e = s->mem.reserve(total);
    if (e == hipSuccess) e = hipMemset((uint8_t*)s->mem.p + zero_from, 0, total - zero_from);
    if (e != hipSuccess) {
        s->mem.release();
        delete s;
        return fail_hip(e, name);
    }
    *out = s;
    return CS_OK;
}

template <class S>
void sub_destroy(S* s)
{
    if (!s) return;
    (void)hipSetDevice(s->device);
    s->mem.release();
    s->scratch.release();
    s->scan.release();
    delete s;
}

// the device buffers that hold the envs' state (cs_state_*): pointer and bytes of each, in a fixed order
int state_parts(const cs_handle* h, void* ptr[5], size_t bytes[5])
{
    const size_t n = (size_t)h->b.n;
    ptr[0] = h->b.mt;    bytes[0] = n * (size_t)h->ops->mt_words * sizeof(uint32_t);
    ptr[1] = h->b.ctl;   bytes[1] = n * sizeof(uint32_t);
    ptr[2] = h->b.state; bytes[2] = n * (size_t)h->ops->info.state_words * sizeof(uint32_t);
    ptr[3] = h->b.sctl;  bytes[3] = h->b.sctl ? n * sizeof(uint32_t) : 0;
    ptr[4] = h->b.sbuf;  bytes[4] = h->b.sbuf ? (n + 63) / 64 * 64 * (size_t)h->ops->stage_bytes : 0;
    return 5;
}
size_t part_span(size_t bytes) { return (bytes + 255) / 256 * 256; }   // each part 256-B aligned in the buffer
}  // namespace

extern "C" {

const char* cs_last_error(void) { return g_err.c_str(); }
const char* cs_version(void) { return "rlcard_amd cardsim 0.2 (gfx950)"; }
int32_t cs_abi_version(void) { return CS_ABI_VERSION; }

int cs_game_info_get(int32_t game, const cs_config* cfg, cs_game_info* info)
{
    if (!info) return fail(CS_E_INVALID, "info is null");
    memset(info, 0, sizeof(*info));
    const cs::GameOps* ops = cs::find_game(game, cfg);
    if (!ops && game == CS_GAME_UNO)
        return fail(CS_E_UNSUPPORTED, "uno: game_num_players must be 2 (the reference's payoffs are defined for two)");
    if (!ops && game == CS_GAME_MAHJONG)
        return fail(CS_E_UNSUPPORTED, "mahjong: game_num_players must be 4 (the reference's game is four-handed)");
    if (!ops && game == CS_GAME_GIN_RUMMY)
        return fail(CS_E_UNSUPPORTED, "gin-rummy: game_num_players must be 2 (the reference's game is two-handed)");
    if (!ops && game == CS_GAME_BRIDGE)
        return fail(CS_E_UNSUPPORTED, "bridge: game_num_players must be 4 (the reference's game is four-handed)");
    if (!ops && game == CS_GAME_SCOUT)
        return fail(CS_E_UNSUPPORTED, "scout: game_num_players must be 4 (the reference's env builds a four-player game)");
    if (!ops) return fail(CS_E_UNSUPPORTED, "unsupported game or game config");
    *info = ops->info;
    return CS_OK;
}

int cs_create(cs_handle** out, int32_t game, int64_t num_envs, int32_t device, const cs_config* cfg)
{
    if (!out) return fail(CS_E_INVALID, "out is null");
    *out = nullptr;
    if (num_envs <= 0) return fail(CS_E_INVALID, "num_envs must be positive");
    if (cfg && cfg->rng_mode != CS_RNG_MT19937 && cfg->rng_mode != CS_RNG_PHILOX)
        return fail(CS_E_INVALID, "rng_mode must be CS_RNG_MT19937 or CS_RNG_PHILOX");
    const cs::GameOps* ops = cs::find_game(game, cfg);
    if (!ops && game == CS_GAME_UNO)
        return fail(CS_E_UNSUPPORTED, "uno: game_num_players must be 2 (the reference's payoffs are defined for two)");
    if (!ops && game == CS_GAME_MAHJONG)
        return fail(CS_E_UNSUPPORTED, "mahjong: game_num_players must be 4 (the reference's game is four-handed)");
    if (!ops && game == CS_GAME_GIN_RUMMY)
        return fail(CS_E_UNSUPPORTED, "gin-rummy: game_num_players must be 2 (the reference's game is two-handed)");
    if (!ops && game == CS_GAME_BRIDGE)
        return fail(CS_E_UNSUPPORTED, "bridge: game_num_players must be 4 (the reference's game is four-handed)");
    if (!ops && game == CS_GAME_SCOUT)
        return fail(CS_E_UNSUPPORTED, "scout: game_num_players must be 4 (the reference's env builds a four-player game)");
    if (!ops) return fail(CS_E_UNSUPPORTED, "unsupported game or game config");
    const cs_game_info& info = ops->info;
    int ndev = 0;
    hipError_t e = hipGetDeviceCount(&ndev);
    if (e != hipSuccess || ndev == 0) return fail(CS_E_DEVICE, "no HIP device available (the engine needs a GPU)");
    if (device < 0 || device >= ndev) return fail(CS_E_INVALID, "device index out of range");
    cs_handle* h = new (std::nothrow) cs_handle();
    if (!h) return fail(CS_E_INVALID, "out of host memory");
    h->device = device;
    h->ops = ops;
    h->seeded = false;
    h->b.game = game;
    h->b.n = num_envs;
    h->b.num_players = info.num_players;
    h->b.obs_dim = info.obs_dim;
    h->b.num_actions = info.num_actions;
    h->b.action_bytes = info.action_bytes;
    h->b.num_decks = cfg ? cfg->num_decks : 1;
    h->b.chips_for_each = (cfg && cfg->chips_for_each > 0) ? cfg->chips_for_each : 100;
    h->b.dealer_id = cfg ? cfg->dealer_plus1 - 1 : -1;
    h->b.rng_mode = cfg ? cfg->rng_mode : CS_RNG_MT19937;
    h->b.rec = cs::StepRecord{nullptr, nullptr, 0u, 0};
    h->b.kernel_flags = 0;
    h->b.table = nullptr;
    if (int r = set_device(h)) { delete h; return r; }
    const size_t n = (size_t)num_envs;
    if ((e = hipMalloc((void**)&h->b.mt, n * (size_t)ops->mt_words * sizeof(uint32_t))) != hipSuccess ||
        (e = hipMalloc((void**)&h->b.ctl, n * sizeof(uint32_t))) != hipSuccess ||
        (e = hipMalloc((void**)&h->b.state, n * (size_t)info.state_words * sizeof(uint32_t))) != hipSuccess) {
        cs_destroy(h);
        return fail_hip(e, "hipMalloc (env state)");
    }
    if (game == CS_GAME_DOUDIZHU) {
        const std::string err = cs::ddz::table_create(&h->table_dev, &h->tab);
        if (!err.empty()) {
            cs_destroy(h);
            return fail(CS_E_DEVICE, err.c_str());
        }
        h->b.table = &h->tab;
    }
    if (ops->stage_bytes > 0) {   // rollout staging rows, whole waves (the copy moves 16-B chunks of full rows)
        const size_t rows = (n + 63) / 64 * 64;
        if ((e = hipMalloc((void**)&h->b.sctl, n * sizeof(uint32_t))) != hipSuccess ||
            (e = hipMalloc((void**)&h->b.sbuf, rows * (size_t)ops->stage_bytes)) != hipSuccess) {
            cs_destroy(h);
            return fail_hip(e, "hipMalloc (rollout staging)");
        }
    }
    *out = h;
    return CS_OK;
}

void cs_destroy(cs_handle* h)
{
    if (!h) return;
    (void)hipSetDevice(h->device);
    if (h->b.mt) (void)hipFree(h->b.mt);
    if (h->b.ctl) (void)hipFree(h->b.ctl);
    if (h->b.state) (void)hipFree(h->b.state);
    if (h->b.sctl) (void)hipFree(h->b.sctl);
    if (h->b.sbuf) (void)hipFree(h->b.sbuf);
    if (h->table_dev) (void)hipFree(h->table_dev);
    h->scan.release();
    h->cfr.release();
    delete h;
}

int cs_seed(cs_handle* h, const uint32_t* keys, const int32_t* key_len, int64_t first_env, int64_t n, void* stream)
{
    if (!h || !keys || !key_len) return fail(CS_E_INVALID, "null argument");
    if (first_env < 0 || n <= 0 || first_env + n > h->b.n) return fail(CS_E_INVALID, "env range out of bounds");
    for (int64_t i = 0; i < n; i++)
        if (key_len[i] < 1 || key_len[i] > 2) return fail(CS_E_INVALID, "key_len must be 1 or 2");
    int r = set_device(h);
    if (r != CS_OK) return r;
    hipStream_t s = (hipStream_t)stream;
    // seeding is rare: stage the (pageable) host keys synchronously, launch, wait, free
    uint32_t* dk = nullptr;
    int32_t* dl = nullptr;
    hipError_t e = hipStreamSynchronize(s);
    if (e != hipSuccess) return fail_hip(e, "cs_seed (pending work on the stream)");
    if ((e = hipMalloc((void**)&dk, (size_t)n * 2 * sizeof(uint32_t))) != hipSuccess)
        return fail_hip(e, "hipMalloc (keys)");
    if ((e = hipMalloc((void**)&dl, (size_t)n * sizeof(int32_t))) != hipSuccess) {
        (void)hipFree(dk);
        return fail_hip(e, "hipMalloc (key_len)");
    }
    e = hipMemcpy(dk, keys, (size_t)n * 2 * sizeof(uint32_t), hipMemcpyHostToDevice);
    if (e == hipSuccess) e = hipMemcpy(dl, key_len, (size_t)n * sizeof(int32_t), hipMemcpyHostToDevice);
    if (e == hipSuccess) e = h->ops->seed(h->b, dk, dl, first_env, n, s);
    if (e == hipSuccess) e = hipStreamSynchronize(s);
    (void)hipFree(dk);
    (void)hipFree(dl);
    if (e != hipSuccess) return fail_hip(e, "cs_seed");
    h->seeded = true;
    return CS_OK;
}

int cs_reset(cs_handle* h, const cs_step_out* out, void* stream)
{
    if (!h || !out) return fail(CS_E_INVALID, "null argument");
    if (!h->seeded) return fail(CS_E_STATE, "cs_reset before cs_seed");
    int r = set_device(h);
    if (r != CS_OK) return r;
    return recorded(h, "cs_reset", [&] { return h->ops->reset(h->b, *out, (hipStream_t)stream); });
}

int cs_step(cs_handle* h, const int32_t* actions, const cs_step_out* out, void* stream)
{
    if (!h || !out || !actions) return fail(CS_E_INVALID, "null argument");
    if (!h->seeded) return fail(CS_E_STATE, "cs_step before cs_seed");
    int r = set_device(h);
    if (r != CS_OK) return r;
    return recorded(h, "cs_step", [&] { return h->ops->step(h->b, actions, *out, (hipStream_t)stream); });
}

int cs_observe(cs_handle* h, int32_t player, const cs_step_out* out, void* stream)
{
    if (!h || !out) return fail(CS_E_INVALID, "null argument");
    if (player < 0 || player >= h->ops->info.num_players) return fail(CS_E_INVALID, "player out of range");
    int r = set_device(h);
    if (r != CS_OK) return r;
    return recorded(h, "cs_observe", [&] { return h->ops->observe(h->b, player, *out, (hipStream_t)stream); });
}

int cs_set_step_record(cs_handle* h, int64_t env, uint32_t* words, uint32_t* seq)
{
    if (!h) return fail(CS_E_INVALID, "null argument");
    if (seq && (!words || env < 0 || env >= h->b.n)) return fail(CS_E_INVALID, "words / env out of range");
    if (words && ((uintptr_t)words & 15u)) return fail(CS_E_INVALID, "words must be 16-byte aligned");
    h->b.rec = cs::StepRecord{seq ? words : nullptr, seq, 0u, seq ? env : 0};
    return CS_OK;
}

int cs_cfr_train(cs_handle* h, int32_t iterations, int64_t iteration0, double* policy, double* average_policy,
                 double* regrets, uint32_t* flags, void* stream)
{
    if (!h || !policy || !average_policy || !regrets || !flags) return fail(CS_E_INVALID, "null argument");
    if (h->b.game != CS_GAME_LEDUC) return fail(CS_E_UNSUPPORTED, "cs_cfr_train supports leduc-holdem only");
    if (h->b.num_players != 2) return fail(CS_E_UNSUPPORTED, "cs_cfr_train: 2-player leduc-holdem only");
    if (iterations < 0 || iteration0 < 0) return fail(CS_E_INVALID, "negative iteration count");
    if (!h->seeded) return fail(CS_E_STATE, "cs_cfr_train before cs_seed");
    int r = set_device(h);
    if (r != CS_OK) return r;
    const cs::CfrTables t{policy, average_policy, regrets, flags};
    return done(cs::launch_cfr(h->b, iterations, iteration0, t, h->cfr, (hipStream_t)stream), "cs_cfr_train");
}

int cs_rollout(cs_handle* h, int32_t T, uint64_t policy_seed, uint64_t t0, uint64_t env_base, const cs_traj_out* out,
               void* stream)
{
    if (!h || !out) return fail(CS_E_INVALID, "null argument");
    if (!out->obs || !out->legal || !out->player || !out->action || !out->reward || !out->done)
        return fail(CS_E_INVALID, "cs_rollout needs every trajectory buffer");
    if (T <= 0) return fail(CS_E_INVALID, "T must be positive");
    if (!h->seeded) return fail(CS_E_STATE, "cs_rollout before cs_seed");
    int r = set_device(h);
    if (r != CS_OK) return r;
    return done(h->ops->rollout(h->b, T, policy_seed, t0, env_base, *out, (hipStream_t)stream), "cs_rollout");
}

int cs_rollout_policy(cs_handle* h, int32_t T, uint64_t policy_seed, uint64_t t0, uint64_t env_base,
                      const int32_t* seat_policy, const cs_traj_out* out, void* stream)
{
    if (!h || !out || !seat_policy) return fail(CS_E_INVALID, "null argument");
    if (!out->obs || !out->legal || !out->player || !out->action || !out->reward || !out->done)
        return fail(CS_E_INVALID, "cs_rollout_policy needs every trajectory buffer");
    if (T <= 0) return fail(CS_E_INVALID, "T must be positive");
    const int32_t P = h->ops->info.num_players;
    bool rules = false;
    for (int32_t p = 0; p < P; p++) {
        if (seat_policy[p] < CS_POLICY_RANDOM || seat_policy[p] > CS_POLICY_RULE_V2)
            return fail(CS_E_INVALID, "unknown policy id");
        rules |= seat_policy[p] != CS_POLICY_RANDOM;
    }
    if (!h->seeded) return fail(CS_E_STATE, "cs_rollout_policy before cs_seed");
    int r = set_device(h);
    if (r != CS_OK) return r;
    hipError_t e;
    if (!rules && !h->ops->rollout_policy) {   // every seat random on a game without policy kernels: cs_rollout
        e = h->ops->rollout(h->b, T, policy_seed, t0, env_base, *out, (hipStream_t)stream);
    } else {
        uint32_t seats = 0;
        for (int32_t p = 0; p < P; p++) {
            if (!h->ops->rollout_policy || seat_policy[p] > h->ops->max_policy)
                return fail(CS_E_UNSUPPORTED, "rule policies: 2-player leduc-holdem (v1, v2), limit-holdem (v1), uno (v1), gin-rummy (v1) and bridge (v1) only");
            seats |= (uint32_t)seat_policy[p] << (8 * p);   // (P <= 4 wherever rollout_policy is set: one byte per seat)
        }
        e = h->ops->rollout_policy(h->b, T, policy_seed, t0, env_base, seats, *out, (hipStream_t)stream);
    }
    return done(e, "cs_rollout_policy");
}

int cs_policy_actions(cs_handle* h, int32_t policy, uint64_t policy_seed, uint64_t t, uint64_t env_base,
                      int32_t* actions, void* stream)
{
    if (!h || !actions) return fail(CS_E_INVALID, "null argument");
    if (policy < CS_POLICY_RANDOM || policy > CS_POLICY_RULE_V2) return fail(CS_E_INVALID, "unknown policy id");
    if (!h->ops->policy_actions || policy > h->ops->max_policy)
        return fail(CS_E_UNSUPPORTED, "rule policies: 2-player leduc-holdem (v1, v2), limit-holdem (v1), uno (v1), gin-rummy (v1) and bridge (v1) only");
    if (!h->seeded) return fail(CS_E_STATE, "cs_policy_actions before cs_seed");
    int r = set_device(h);
    if (r != CS_OK) return r;
    return done(h->ops->policy_actions(h->b, policy, policy_seed, t, env_base, actions, (hipStream_t)stream),
                                       "cs_policy_actions");
}

int cs_payoff_sums(cs_handle* h, int32_t T, const cs_traj_out* traj, int32_t quota, int32_t* games_per_env,
                   double* sums, int64_t* games, void* stream)
{
    if (!h || !traj || !games_per_env || !sums || !games) return fail(CS_E_INVALID, "null argument");
    if (!traj->reward || !traj->done) return fail(CS_E_INVALID, "traj needs reward and done");
    if (T <= 0) return fail(CS_E_INVALID, "T must be positive");
    int r = set_device(h);
    if (r != CS_OK) return r;
    return done(cs::launch_payoff_sums(h->b, T, *traj, quota, games_per_env, sums, games, (hipStream_t)stream),
                                       "cs_payoff_sums");
}

// ---- DMC ----------------------------------------------------------------------------------------------------------
struct cs_dmc : cs_sub {   // mem: the ring and the counters; scratch: i64 [rows], the ring row of each trajectory row
    cs::DmcRing r;
};

int cs_dmc_create(cs_handle* h, int32_t T, int32_t slots, cs_dmc** out)
{
    if (!h || !out) return fail(CS_E_INVALID, "null argument");
    *out = nullptr;
    if (T <= 0 || slots < 2) return fail(CS_E_INVALID, "cs_dmc_create: T > 0 and slots >= 2");
    int r = set_device(h);
    if (r != CS_OK) return r;
    const int64_t streams = h->b.n * h->ops->info.num_players, rows = streams * slots * (int64_t)T;
    const int64_t O = h->ops->info.obs_dim, F = h->ops->info.action_feature_dim;
    cs::Carve c;
    const size_t o_st = c.take<int8_t>(rows * O), o_act = c.take<int8_t>(rows * F), o_tgt = c.take<float>(rows),
                 o_ret = c.take<float>(rows), o_dne = c.take<uint8_t>(rows), o_ctr = c.take<int64_t>(streams),
                 o_gs = c.take<int64_t>(streams), o_em = c.take<int64_t>(streams),
                 o_cnt = c.take<int32_t>(streams + 1), o_off = c.take<int64_t>(streams + 1),
                 o_flag = c.take<uint32_t>(1);
    // counters, counts (incl. the trailing 0) and the flag start at zero; the ring rows are written before read
    cs_dmc* d = nullptr;
    if ((r = sub_create(h, c.bytes(), o_ctr, "cs_dmc_create", &d)) != CS_OK) return r;
    uint8_t* m = (uint8_t*)d->mem.p;
    d->r = cs::DmcRing{T, slots, (int32_t)F, (int8_t*)(m + o_st), (int8_t*)(m + o_act), (float*)(m + o_tgt),
                       (float*)(m + o_ret), m + o_dne, (int64_t*)(m + o_ctr), (int64_t*)(m + o_gs),
                       (int64_t*)(m + o_em), (int32_t*)(m + o_cnt), (int64_t*)(m + o_off), (uint32_t*)(m + o_flag)};
    *out = d;
    return CS_OK;
}

void cs_dmc_destroy(cs_dmc* d) { sub_destroy(d); }

int cs_dmc_fill(cs_dmc* d, int32_t T_roll, const cs_traj_out* traj, int64_t* ready, int64_t cap, int64_t* nready,
                void* stream)
{
    if (!d || !traj || !nready || (cap > 0 && !ready)) return fail(CS_E_INVALID, "null argument");
    if (!traj->player || !traj->done || !traj->reward) return fail(CS_E_INVALID, "traj needs player, reward and done");
    if (T_roll <= 0) return fail(CS_E_INVALID, "T_roll must be positive");
    int r = set_device(d->h);
    if (r != CS_OK) return r;
    const int64_t rows = (int64_t)T_roll * d->h->b.n;
    hipError_t e = d->scratch.reserve((size_t)rows * sizeof(int64_t));
    if (e == hipSuccess)
        e = cs::launch_dmc_fill(d->h->b, d->r, T_roll, *traj, ready, cap, nready, (int64_t*)d->scratch.p, d->scan,
                                (hipStream_t)stream);
    return done(e, "cs_dmc_fill");
}

int cs_dmc_gather(cs_dmc* d, int32_t player, const int64_t* chunks, int64_t count, const cs_dmc_batch* out,
                  void* stream)
{
    if (!d || !out || (count > 0 && !chunks)) return fail(CS_E_INVALID, "null argument");
    if (player < 0 || player >= d->h->ops->info.num_players) return fail(CS_E_INVALID, "player out of range");
    if (count < 0 || count > 0x7FFFFFFF) return fail(CS_E_INVALID, "count out of range");
    if (count == 0) return CS_OK;
    int r = set_device(d->h);
    if (r != CS_OK) return r;
    const int32_t od = d->h->ops->info.obs_dim;
    const int32_t sd = d->h->b.game == CS_GAME_DOUDIZHU && player == 0 ? cs::ddz::OBS_LANDLORD : od;
    return done(cs::launch_dmc_gather(d->r, sd, od, chunks, count, *out, (hipStream_t)stream), "cs_dmc_gather");
}

int cs_dmc_status(cs_dmc* d, uint32_t* host_flags)
{
    if (!d || !host_flags) return fail(CS_E_INVALID, "null argument");
    int r = set_device(d->h);
    if (r != CS_OK) return r;
    return done(hipMemcpy(host_flags, d->r.flag, sizeof(uint32_t), hipMemcpyDeviceToHost), "cs_dmc_status");
}

int cs_dmc_layer1(cs_handle* h, const float* X, const int32_t* state_of, const int32_t* ids, int64_t E, int32_t H,
                  const float* W_act, const float* b1, float* h1, void* stream)
{
    if (!h || !X || !state_of || !ids || !W_act || !b1 || !h1) return fail(CS_E_INVALID, "null argument");
    if (E < 0 || E > 0x7FFFFFFF || H <= 0 || H % 4) return fail(CS_E_INVALID, "E / H out of range");
    if (E == 0) return CS_OK;
    int r = set_device(h);
    if (r != CS_OK) return r;
    return done(cs::launch_dmc_layer1(X, state_of, ids, E, H, W_act, b1, h->ops->info.action_feature_dim, h->b, h1,
                                      (hipStream_t)stream), "cs_dmc_layer1");
}

int cs_dmc_select(const float* values, const int32_t* counts, const int64_t* offsets, const int32_t* ids, int64_t S,
                  float eps, uint64_t seed, uint64_t t, uint64_t state_base, int32_t* actions, void* stream)
{
    if (!values || !counts || !offsets || !ids || !actions) return fail(CS_E_INVALID, "null argument");
    if (S <= 0) return fail(CS_E_INVALID, "S must be positive");
    return done(cs::launch_dmc_select(values, counts, offsets, ids, S, eps, seed, t, state_base, actions,
                                      (hipStream_t)stream), "cs_dmc_select");
}

// ---- DQN ----------------------------------------------------------------------------------------------------------
static int qnet_check(const cs_handle* h, const cs_qnet* net, const void* obs, int64_t rows)
{
    if (!h || !net || !obs) return fail(CS_E_INVALID, "null argument");
    const cs_game_info& info = h->ops->info;
    if (info.num_actions > 64)
        return fail(CS_E_UNSUPPORTED, "the Q-network kernel takes games of at most 64 actions (gin-rummy has 110, bridge 91, scout 204)");
    if (net->in_dim != info.obs_dim || net->num_actions != info.num_actions)
        return fail(CS_E_INVALID, "cs_qnet: in_dim / num_actions are not the handle's game's");
    if (net->num_hidden < 1 || net->num_hidden > CS_QNET_MAX_HIDDEN)
        return fail(CS_E_INVALID, "cs_qnet: num_hidden must be 1..4");
    for (int l = 0; l <= net->num_hidden; l++) {
        if (l < net->num_hidden && (net->hidden[l] < 1 || net->hidden[l] > CS_QNET_MAX_WIDTH))
            return fail(CS_E_INVALID, "cs_qnet: hidden widths must be 1..128");
        if (!net->W[l] || !net->b[l]) return fail(CS_E_INVALID, "cs_qnet: null weights");
    }
    // (every descriptor the checks above pass needs 100 352 B at most on the games there are -- qnet_lds_bytes of
    // Mahjong with two 128-unit layers: the 816 x 72 obs bytes make the first buffer 230 units, the second holds 128,
    // (230 + 128) x 256 B, plus two weight tiles of 4 352 B; this guards a future game's obs)
    if (cs::qnet_lds_bytes(*net) > 160 * 1024)
        return fail(CS_E_UNSUPPORTED, "cs_qnet: the net needs more than the 160 KiB of LDS a block can have");
    if (rows < 0 || rows > 0x7FFFFFFF) return fail(CS_E_INVALID, "rows out of range");
    return CS_OK;
}

int cs_qnet_values(cs_handle* h, const cs_qnet* net, const void* obs, const void* legal, int64_t rows, float* q,
                   void* stream)
{
    int r = qnet_check(h, net, obs, rows);
    if (r != CS_OK) return r;
    if (!q) return fail(CS_E_INVALID, "null argument");
    if (rows == 0) return CS_OK;
    if ((r = set_device(h)) != CS_OK) return r;
    return done(cs::launch_qnet(*net, (const uint8_t*)obs, (const uint8_t*)legal, nullptr, rows, 0.f, 0, 0, 0, nullptr,
                                q, (hipStream_t)stream), "cs_qnet_values");
}

int cs_qnet_actions(cs_handle* h, const cs_qnet* net, const void* obs, const void* legal, const void* done,
                    int64_t rows, float eps, uint64_t seed, uint64_t t, uint64_t row_base, int32_t* actions, float* q,
                    void* stream)
{
    int r = qnet_check(h, net, obs, rows);
    if (r != CS_OK) return r;
    if (!actions) return fail(CS_E_INVALID, "null argument");
    if (rows == 0) return CS_OK;
    if ((r = set_device(h)) != CS_OK) return r;
    return ::done(cs::launch_qnet(*net, (const uint8_t*)obs, (const uint8_t*)legal, (const uint8_t*)done, rows, eps,
                                  seed, t, row_base, actions, q, (hipStream_t)stream), "cs_qnet_actions");
}

struct cs_replay : cs_sub {   // mem: the ring, the pending store and the counter; scratch: i32 [2][entries], code and
    cs::ReplayRing r;         // pos of a push
    int64_t seen_total = 0;   // cs_dqn_train: the ring's total as last read (it only grows)
};

int cs_replay_create(cs_handle* h, int64_t capacity, cs_replay** out)
{
    if (!h || !out) return fail(CS_E_INVALID, "null argument");
    *out = nullptr;
    if (capacity <= 0) return fail(CS_E_INVALID, "capacity must be positive");
    const cs_game_info& info = h->ops->info;
    if (info.legal_bytes > 16) return fail(CS_E_UNSUPPORTED, "cs_replay: legal masks of at most 16 bytes");
    if (info.num_actions > 64)   // (the replay feeds the Q-network kernel, which takes at most 64 actions)
        return fail(CS_E_UNSUPPORTED, "cs_replay: games of at most 64 actions (gin-rummy has 110, bridge 91, scout 204)");
    int r = set_device(h);
    if (r != CS_OK) return r;
    const int64_t O = info.obs_dim, LB = info.legal_bytes, NP = h->b.n * info.num_players, cap = capacity;
    cs::Carve c;
    const size_t o_st = c.take<uint8_t>(cap * O), o_nst = c.take<uint8_t>(cap * O), o_nlg = c.take<uint8_t>(cap * LB),
                 o_act = c.take<int32_t>(cap), o_rew = c.take<float>(cap), o_dne = c.take<uint8_t>(cap),
                 o_pst = c.take<uint8_t>(NP * O), o_pact = c.take<int32_t>(NP), o_np = c.take<int32_t>(NP),
                 o_pv = c.take<uint8_t>(NP), o_tot = c.take<int64_t>(1);
    // no pending rows, nothing appended; the slots are written before they are read
    cs_replay* p = nullptr;
    if ((r = sub_create(h, c.bytes(), o_pv, "cs_replay_create", &p)) != CS_OK) return r;
    uint8_t* m = (uint8_t*)p->mem.p;
    p->r = cs::ReplayRing{cap, (int32_t)O, (int32_t)LB, info.num_players, info.action_bytes, m + o_st, m + o_nst,
                          m + o_nlg, (int32_t*)(m + o_act), (float*)(m + o_rew), m + o_dne, (int64_t*)(m + o_tot),
                          m + o_pv, m + o_pst, (int32_t*)(m + o_pact), (int32_t*)(m + o_np)};
    *out = p;
    return CS_OK;
}

void cs_replay_destroy(cs_replay* r) { sub_destroy(r); }

int cs_replay_push(cs_replay* r, int32_t T, const cs_traj_out* traj, uint32_t seat_mask, void* stream)
{
    if (!r || !traj) return fail(CS_E_INVALID, "null argument");
    if (!traj->obs || !traj->legal || !traj->player || !traj->action || !traj->reward || !traj->done ||
        !traj->final_obs)
        return fail(CS_E_INVALID, "cs_replay_push needs every trajectory buffer, final_obs included");
    if (T <= 0) return fail(CS_E_INVALID, "T must be positive");
    const int64_t entries = r->h->b.n * r->r.P + (int64_t)T * r->h->b.n + 1;
    if (entries > 0x7FFFFFFF) return fail(CS_E_INVALID, "cs_replay_push: window too large (T * n must stay below 2^31)");
    int rc = set_device(r->h);
    if (rc != CS_OK) return rc;
    hipError_t e = r->scratch.reserve((size_t)entries * 2 * sizeof(int32_t));
    if (e != hipSuccess) return done(e, "cs_replay_push");
    // code, and pos in the second half of what is allocated (the largest push so far)
    int32_t *code = (int32_t*)r->scratch.p, *pos = code + r->scratch.bytes / (2 * sizeof(int32_t));
    e = cs::launch_replay_push(r->h->b, r->r, T, *traj, seat_mask, code, pos, r->scan, (hipStream_t)stream);
    return done(e, "cs_replay_push");
}

int cs_replay_drop_pending(cs_replay* r, void* stream)
{
    if (!r) return fail(CS_E_INVALID, "null argument");
    int rc = set_device(r->h);
    if (rc != CS_OK) return rc;
    return done(hipMemsetAsync(r->r.pvalid, 0, (size_t)(r->h->b.n * r->r.P), (hipStream_t)stream),
                               "cs_replay_drop_pending");
}

int cs_replay_size(cs_replay* r, int64_t* size, int64_t* total)
{
    if (!r || (!size && !total)) return fail(CS_E_INVALID, "null argument");
    int rc = set_device(r->h);
    if (rc != CS_OK) return rc;
    int64_t t = 0;
    hipError_t e = hipDeviceSynchronize();
    if (e == hipSuccess) e = hipMemcpy(&t, r->r.total, sizeof(int64_t), hipMemcpyDeviceToHost);
    if (e != hipSuccess) return fail_hip(e, "cs_replay_size");
    if (total) *total = t;
    if (size) *size = t < r->r.cap ? t : r->r.cap;
    return CS_OK;
}

int cs_replay_gather(cs_replay* r, const int64_t* idx, int64_t B, const cs_replay_batch* out, void* stream)
{
    if (!r || !out) return fail(CS_E_INVALID, "null argument");
    if (B <= 0) return CS_OK;
    if (!idx) return fail(CS_E_INVALID, "null argument");
    if (B > 0x7FFFFFFF / 32) return fail(CS_E_INVALID, "B out of range");
    int rc = set_device(r->h);
    if (rc != CS_OK) return rc;
    return done(cs::launch_replay_gather(r->r, idx, B, *out, (hipStream_t)stream), "cs_replay_gather");
}

int cs_dqn_targets(const float* q_next, const float* q_next_target, const void* next_legal, const float* reward,
                   const void* done, int64_t B, int32_t num_actions, float gamma, float* target, int32_t* best,
                   void* stream)
{
    if (!q_next || !next_legal || (!target && !best)) return fail(CS_E_INVALID, "null argument");
    if (target && (!q_next_target || !reward || !done)) return fail(CS_E_INVALID, "null argument");
    if (num_actions <= 0) return fail(CS_E_INVALID, "num_actions must be positive");
    if (B < 0 || B > 0x7FFFFFFF) return fail(CS_E_INVALID, "B out of range");
    if (B == 0) return CS_OK;
    return ::done(cs::launch_dqn_targets(q_next, q_next_target, (const uint8_t*)next_legal, reward, (const uint8_t*)done,
                                         B, num_actions, gamma, target, best, (hipStream_t)stream), "cs_dqn_targets");
}

static int dqn_net_check(const cs_replay* r, const cs_dqn_net* n)
{
    const cs_game_info& info = r->h->ops->info;
    if (n->in_dim != info.obs_dim || n->num_actions != info.num_actions)
        return fail(CS_E_INVALID, "cs_dqn_net: in_dim / num_actions are not the ring's game's");
    if (n->num_hidden < 1 || n->num_hidden > CS_QNET_MAX_HIDDEN)
        return fail(CS_E_INVALID, "cs_dqn_net: num_hidden must be 1..4");
    for (int l = 0; l <= n->num_hidden; l++) {
        if (l < n->num_hidden && (n->hidden[l] < 1 || n->hidden[l] > CS_QNET_MAX_WIDTH))
            return fail(CS_E_INVALID, "cs_dqn_net: hidden widths must be 1..128");
        if (!n->W[l] || !n->b[l]) return fail(CS_E_INVALID, "cs_dqn_net: null weights");
    }
    if (!n->bn_weight || !n->bn_bias || !n->bn_mean || !n->bn_var || !n->bn_tracked)
        return fail(CS_E_INVALID, "cs_dqn_net: null BatchNorm tensors");
    if (!(n->bn_eps > 0.f) || !(n->bn_momentum >= 0.f && n->bn_momentum <= 1.f))
        return fail(CS_E_INVALID, "cs_dqn_net: BatchNorm eps must be positive and momentum in [0, 1]");
    return CS_OK;
}

int cs_dqn_train(cs_replay* r, const cs_dqn_net* qnet, const cs_dqn_net* target, const cs_dqn_adam* opt,
                 const cs_dqn_train_args* args, void* stream)
{
    if (!r || !qnet || !target || !opt || !args) return fail(CS_E_INVALID, "null argument");
    if (args->B < 2 || args->B > 64) return fail(CS_E_INVALID, "cs_dqn_train: B must be 2..64");
    if (args->K < 1 || args->K > 4096) return fail(CS_E_INVALID, "cs_dqn_train: K must be 1..4096");
    if (!args->loss) return fail(CS_E_INVALID, "cs_dqn_train: null loss buffer");
    if (args->target_every < 0) return fail(CS_E_INVALID, "cs_dqn_train: target_every must not be negative");
    int rc = dqn_net_check(r, qnet);
    if (rc != CS_OK) return rc;
    if ((rc = dqn_net_check(r, target)) != CS_OK) return rc;
    if (target->num_hidden != qnet->num_hidden) return fail(CS_E_INVALID, "cs_dqn_train: the networks' shapes differ");
    for (int l = 0; l < qnet->num_hidden; l++)
        if (target->hidden[l] != qnet->hidden[l])
            return fail(CS_E_INVALID, "cs_dqn_train: the networks' shapes differ");
    if (!opt->bn_weight_m || !opt->bn_weight_v || !opt->bn_bias_m || !opt->bn_bias_v)
        return fail(CS_E_INVALID, "cs_dqn_adam: null state");
    for (int l = 0; l <= qnet->num_hidden; l++)
        if (!opt->W_m[l] || !opt->W_v[l] || !opt->b_m[l] || !opt->b_v[l])
            return fail(CS_E_INVALID, "cs_dqn_adam: null state");
    if (!(opt->lr >= 0.0) || !(opt->beta1 >= 0.0 && opt->beta1 < 1.0) || !(opt->beta2 >= 0.0 && opt->beta2 < 1.0) ||
        !(opt->eps >= 0.0) || opt->step0 < 0)
        return fail(CS_E_INVALID, "cs_dqn_adam: lr, eps >= 0, betas in [0, 1) and step0 >= 0");
    if (cs::dqn_train_lds_bytes(*qnet, args->B) > 160 * 1024)
        return fail(CS_E_UNSUPPORTED, "cs_dqn_train: the step needs more than the 160 KiB of LDS a workgroup can have");
    if ((rc = set_device(r->h)) != CS_OK) return rc;
    if (!args->idx && r->seen_total < args->B) {   // (once the ring is known to hold B transitions it always does)
        int64_t t = 0;
        hipError_t e = hipDeviceSynchronize();
        if (e == hipSuccess) e = hipMemcpy(&t, r->r.total, sizeof(int64_t), hipMemcpyDeviceToHost);
        if (e != hipSuccess) return fail_hip(e, "cs_dqn_train");
        r->seen_total = t;
        if (t < args->B) return fail(CS_E_STATE, "cs_dqn_train: the memory holds fewer than B transitions");
    }
    return done(cs::launch_dqn_train(r->r, *qnet, *target, *opt, *args, (hipStream_t)stream), "cs_dqn_train");
}

// ---- NFSP ---------------------------------------------------------------------------------------------------------
int cs_pnet_probs(cs_handle* h, const cs_qnet* net, const void* obs, const void* legal, int64_t rows, float* probs,
                  void* stream)
{
    int r = qnet_check(h, net, obs, rows);
    if (r != CS_OK) return r;
    if (!probs) return fail(CS_E_INVALID, "null argument");
    if (rows == 0) return CS_OK;
    if ((r = set_device(h)) != CS_OK) return r;
    return done(cs::launch_pnet(*net, (const uint8_t*)obs, (const uint8_t*)legal, nullptr, rows, 0, 0, 0, nullptr,
                                probs, (hipStream_t)stream), "cs_pnet_probs");
}

int64_t cs_nfsp_scratch_bytes(int64_t rows)
{
    if (rows < 0 || rows > 0x7FFFFFFF) return fail(CS_E_INVALID, "rows out of range");
    size_t bytes = 0;
    hipError_t e = cs::nfsp_scratch_bytes(rows > 0 ? rows : 1, &bytes);
    return e == hipSuccess ? (int64_t)bytes : fail_hip(e, "cs_nfsp_scratch_bytes");
}

int cs_nfsp_actions(cs_handle* h, const cs_qnet* qnet, const cs_qnet* pnet, const void* obs, const void* legal,
                    const void* done, const void* mode, int64_t rows, float eps, uint64_t seed, uint64_t t,
                    uint64_t row_base, int32_t* actions, float* probs, void* scratch, void* stream)
{
    int r = qnet_check(h, pnet, obs, rows);
    if (r != CS_OK) return r;
    if (mode && (r = qnet_check(h, qnet, obs, rows)) != CS_OK) return r;
    if (!actions || (mode && !scratch)) return fail(CS_E_INVALID, "null argument");
    if (rows == 0) return CS_OK;
    if ((r = set_device(h)) != CS_OK) return r;
    hipError_t e;
    if (!mode)
        e = cs::launch_pnet(*pnet, (const uint8_t*)obs, (const uint8_t*)legal, (const uint8_t*)done, rows, seed, t,
                            row_base, actions, probs, (hipStream_t)stream);
    else
        e = cs::launch_nfsp_actions(*qnet, *pnet, (const uint8_t*)obs, (const uint8_t*)legal, (const uint8_t*)done,
                                    (const uint8_t*)mode, rows, eps, seed, t, row_base, actions, probs, scratch,
                                    (hipStream_t)stream);
    return ::done(e, "cs_nfsp_actions");
}

struct cs_reservoir : cs_sub {   // mem: the slots, the occupant words and the counter; scratch: i32 [entries], the scan
    cs::Reservoir r;             // output of a push
    size_t tail;                 // bytes from the occupant words to the end of mem (what clear zeroes)
};

int cs_reservoir_create(cs_handle* h, int64_t capacity, uint64_t seed, cs_reservoir** out)
{
    if (!h || !out) return fail(CS_E_INVALID, "null argument");
    *out = nullptr;
    if (capacity <= 0) return fail(CS_E_INVALID, "capacity must be positive");
    const cs_game_info& info = h->ops->info;
    if (info.num_actions > 64)
        return fail(CS_E_UNSUPPORTED, "cs_reservoir: games of at most 64 actions (gin-rummy has 110, bridge 91, scout 204)");
    int rc = set_device(h);
    if (rc != CS_OK) return rc;
    const int64_t O = info.obs_dim, cap = capacity;
    cs::Carve c;
    const size_t o_st = c.take<uint8_t>(cap * O), o_act = c.take<int32_t>(cap),
                 o_occ = c.take<unsigned long long>(cap), o_calls = c.take<int64_t>(1);
    cs_reservoir* p = nullptr;
    if ((rc = sub_create(h, c.bytes(), 0, "cs_reservoir_create", &p)) != CS_OK) return rc;
    uint8_t* m = (uint8_t*)p->mem.p;
    p->r = cs::Reservoir{cap, (int32_t)O, info.num_players, info.num_actions, info.action_bytes, seed, m + o_st,
                         (int32_t*)(m + o_act), (unsigned long long*)(m + o_occ), (int64_t*)(m + o_calls)};
    p->tail = c.bytes() - o_occ;
    *out = p;
    return CS_OK;
}

void cs_reservoir_destroy(cs_reservoir* r) { sub_destroy(r); }

int cs_reservoir_push(cs_reservoir* r, int32_t T, const cs_traj_out* traj, const void* mode, uint32_t seat_mask,
                      void* stream)
{
    if (!r || !traj || !mode) return fail(CS_E_INVALID, "null argument");
    if (!traj->obs || !traj->player || !traj->action)
        return fail(CS_E_INVALID, "cs_reservoir_push needs the trajectory's obs, player and action");
    if (T <= 0) return fail(CS_E_INVALID, "T must be positive");
    const int64_t entries = (int64_t)T * r->h->b.n + 1;
    if (entries > 0x7FFFFFFF)
        return fail(CS_E_INVALID, "cs_reservoir_push: window too large (T * n must stay below 2^31)");
    int rc = set_device(r->h);
    if (rc != CS_OK) return rc;
    hipError_t e = r->scratch.reserve((size_t)entries * sizeof(int32_t));
    if (e == hipSuccess)
        e = cs::launch_reservoir_push(r->r, T, r->h->b.n, (const uint8_t*)traj->obs, (const uint8_t*)traj->player,
                                      traj->action, (const uint8_t*)mode, seat_mask, (int32_t*)r->scratch.p, r->scan,
                                      (hipStream_t)stream);
    return done(e, "cs_reservoir_push");
}

int cs_reservoir_size(cs_reservoir* r, int64_t* size, int64_t* add_calls)
{
    if (!r || (!size && !add_calls)) return fail(CS_E_INVALID, "null argument");
    int rc = set_device(r->h);
    if (rc != CS_OK) return rc;
    int64_t t = 0;
    hipError_t e = hipDeviceSynchronize();
    if (e == hipSuccess) e = hipMemcpy(&t, r->r.add_calls, sizeof(int64_t), hipMemcpyDeviceToHost);
    if (e != hipSuccess) return fail_hip(e, "cs_reservoir_size");
    if (add_calls) *add_calls = t;
    if (size) *size = t < r->r.cap ? t : r->r.cap;
    return CS_OK;
}

int cs_reservoir_gather(cs_reservoir* r, const int64_t* idx, int64_t B, float* state, float* probs, void* stream)
{
    if (!r) return fail(CS_E_INVALID, "null argument");
    if (B <= 0) return CS_OK;
    if (!idx) return fail(CS_E_INVALID, "null argument");
    if (B > 0x7FFFFFFF / 32) return fail(CS_E_INVALID, "B out of range");
    int rc = set_device(r->h);
    if (rc != CS_OK) return rc;
    return done(cs::launch_reservoir_gather(r->r, idx, B, state, probs, (hipStream_t)stream), "cs_reservoir_gather");
}

int cs_reservoir_clear(cs_reservoir* r, void* stream)
{
    if (!r) return fail(CS_E_INVALID, "null argument");
    int rc = set_device(r->h);
    if (rc != CS_OK) return rc;
    return done(hipMemsetAsync(r->r.occ, 0, r->tail, (hipStream_t)stream), "cs_reservoir_clear");
}

int cs_traj_probe(cs_handle* h, int32_t T, const cs_traj_out* out, void* stream)
{
    if (!h || !out) return fail(CS_E_INVALID, "null argument");
    if (T <= 0) return fail(CS_E_INVALID, "T must be positive");
    for (const void* p : {out->obs, out->legal, out->player, out->action, out->reward, out->done})
        if (((uintptr_t)p & 15u) != 0) return fail(CS_E_INVALID, "trajectory tensors must be 16-byte aligned");
    int r = set_device(h);
    if (r != CS_OK) return r;
    const cs_game_info& info = h->ops->info;   // envs_per_wave: the game's rollout kernel's (G::EPW)
    return done(cs::launch_traj_probe(h->b, T, *out, info.obs_dim, info.legal_bytes, info.action_bytes,
                                      info.envs_per_wave, (hipStream_t)stream), "cs_traj_probe");
}

int cs_state_bytes(const cs_handle* h, int64_t* bytes)
{
    if (!h || !bytes) return fail(CS_E_INVALID, "null argument");
    void* ptr[5];
    size_t nb[5];
    size_t total = 0;
    for (int i = 0, k = state_parts(h, ptr, nb); i < k; i++) total += part_span(nb[i]);
    *bytes = (int64_t)total;
    return CS_OK;
}

static int state_copy(cs_handle* h, void* buf, bool save, void* stream)
{
    if (!h || !buf) return fail(CS_E_INVALID, "null argument");
    if (((uintptr_t)buf & 15u) != 0) return fail(CS_E_INVALID, "state buffer must be 16-byte aligned");
    int r = set_device(h);
    if (r != CS_OK) return r;
    void* ptr[5];
    size_t nb[5];
    size_t off = 0;
    for (int i = 0, k = state_parts(h, ptr, nb); i < k; i++) {
        if (nb[i]) {
            char* b = (char*)buf + off;
            hipError_t e = save ? hipMemcpyAsync(b, ptr[i], nb[i], hipMemcpyDeviceToDevice, (hipStream_t)stream)
                                : hipMemcpyAsync(ptr[i], b, nb[i], hipMemcpyDeviceToDevice, (hipStream_t)stream);
            if (e != hipSuccess) return fail_hip(e, save ? "cs_state_save" : "cs_state_load");
        }
        off += part_span(nb[i]);
    }
    return CS_OK;
}

int cs_state_save(cs_handle* h, void* buf, void* stream) { return state_copy(h, buf, true, stream); }
int cs_state_load(cs_handle* h, const void* buf, void* stream) { return state_copy(h, (void*)buf, false, stream); }

int cs_transitions(cs_handle* h, int32_t T, const cs_traj_out* traj, const cs_trans_out* out, void* stream)
{
    if (!h || !traj || !out) return fail(CS_E_INVALID, "null argument");
    if (!traj->player || !traj->reward || !traj->done) return fail(CS_E_INVALID, "traj needs player, reward and done");
    if (T <= 0) return fail(CS_E_INVALID, "T must be positive");
    int r = set_device(h);
    if (r != CS_OK) return r;
    return done(cs::launch_transitions(h->b, T, *traj, *out, (hipStream_t)stream), "cs_transitions");
}

int cs_legal_lists(cs_handle* h, const void* legal, int64_t rows, int32_t* counts, int64_t* offsets, int32_t* ids,
                   void* stream)
{
    if (!h || !legal || !counts || !offsets) return fail(CS_E_INVALID, "null argument");
    if (rows <= 0 || rows > ((int64_t)1 << 31) - 1) return fail(CS_E_INVALID, "rows out of range");
    int r = set_device(h);
    if (r != CS_OK) return r;
    return done(cs::launch_legal_lists(h->b, h->ops->info.legal_bytes, (const uint8_t*)legal, rows, counts, offsets,
                                       ids, h->scan, (hipStream_t)stream), "cs_legal_lists");
}

int cs_action_features(cs_handle* h, const int32_t* ids, int64_t count, void* features, void* stream)
{
    if (!h || !ids || !features) return fail(CS_E_INVALID, "null argument");
    if (count <= 0) return fail(CS_E_INVALID, "count must be positive");
    int r = set_device(h);
    if (r != CS_OK) return r;
    hipStream_t s = (hipStream_t)stream;
    return done(h->b.game == CS_GAME_DOUDIZHU ? cs::ddz::launch_features(h->b, ids, count, (uint8_t*)features,
                                                                         s) : cs::launch_onehot(ids, count,
                                                                         h->ops->info.num_actions, (uint8_t*)features,
                                                                         s), "cs_action_features");
}

// cs_get_env_state (to_host) / cs_set_env_state: env's packed state words between the device and host_words
static int env_state_copy(cs_handle* h, int64_t env, uint32_t* host_words, int32_t nwords, bool to_host)
{
    if (!h || !host_words) return fail(CS_E_INVALID, "null argument");
    if (env < 0 || env >= h->b.n || nwords < h->ops->info.state_words) return fail(CS_E_INVALID, "bad env or nwords");
    int r = set_device(h);
    if (r != CS_OK) return r;
    hipError_t e = hipDeviceSynchronize();
    const int sw = h->ops->info.state_words;
    auto copy = [&](uint32_t* dev, uint32_t* host, int words) {
        return to_host ? hipMemcpy(host, dev, sizeof(uint32_t) * words, hipMemcpyDeviceToHost)
                       : hipMemcpy(dev, host, sizeof(uint32_t) * words, hipMemcpyHostToDevice);
    };
    if (h->ops->env_major) {
        if (e == hipSuccess) e = copy(h->b.state + (size_t)env * sw, host_words, sw);
    } else {
        for (int w = 0; w < sw && e == hipSuccess; w++)
            e = copy(h->b.state + (size_t)w * h->b.n + env, host_words + w, 1);
    }
    return done(e, to_host ? "cs_get_env_state" : "cs_set_env_state");
}

int cs_get_env_state(cs_handle* h, int64_t env, uint32_t* host_words, int32_t nwords)
{
    return env_state_copy(h, env, host_words, nwords, true);
}

int cs_copy_env_state(cs_handle* h, int64_t env, uint32_t* dst, void* stream)
{
    if (!h || !dst) return fail(CS_E_INVALID, "null argument");
    if (env < 0 || env >= h->b.n) return fail(CS_E_INVALID, "bad env");
    if (h->ops->info.state_words > 64) return fail(CS_E_UNSUPPORTED, "state too large for cs_copy_env_state");
    int r = set_device(h);
    if (r != CS_OK) return r;
    return done(cs::launch_copy_state(h->b, env, h->ops->info.state_words, h->ops->env_major ? 1 : 0, dst,
                                      (hipStream_t)stream), "cs_copy_env_state");
}

int cs_set_env_state(cs_handle* h, int64_t env, const uint32_t* host_words, int32_t nwords)
{
    return env_state_copy(h, env, const_cast<uint32_t*>(host_words), nwords, false);
}

int cs_env_rng_words(cs_handle* h, int32_t* words)
{
    if (!h || !words) return fail(CS_E_INVALID, "null argument");
    *words = 1 + h->ops->mt_words;
    return CS_OK;
}

static int rng_copy(cs_handle* h, int64_t env, uint32_t* buf, int32_t load, void* stream, const char* what)
{
    if (!h || !buf) return fail(CS_E_INVALID, "null argument");
    if (env < 0 || env >= h->b.n) return fail(CS_E_INVALID, "bad env");
    int r = set_device(h);
    if (r != CS_OK) return r;
    const uint32_t clear = h->b.sbuf ? (1u << 17) : 0u;   // restored streams restage from the ring
    hipError_t e = cs::launch_rng_copy(h->b, env, h->ops->mt_words, h->ops->mt_columns ? 1 : 0, clear, buf, load,
                                       (hipStream_t)stream);
    return done(e, what);
}

int cs_copy_env_rng(cs_handle* h, int64_t env, uint32_t* dst, void* stream)
{
    return rng_copy(h, env, dst, 0, stream, "cs_copy_env_rng");
}

int cs_load_env_rng(cs_handle* h, int64_t env, const uint32_t* src, void* stream)
{
    return rng_copy(h, env, const_cast<uint32_t*>(src), 1, stream, "cs_load_env_rng");
}

int cs_get_rng_ctl(cs_handle* h, int64_t env, uint32_t* host_ctl)
{
    if (!h || !host_ctl) return fail(CS_E_INVALID, "null argument");
    if (env < 0 || env >= h->b.n) return fail(CS_E_INVALID, "bad env");
    int r = set_device(h);
    if (r != CS_OK) return r;
    hipError_t e = hipDeviceSynchronize();
    if (e == hipSuccess) e = hipMemcpy(host_ctl, h->b.ctl + env, sizeof(uint32_t), hipMemcpyDeviceToHost);
    return done(e, "cs_get_rng_ctl");
}

int cs_debug_holdem_rank7(const int8_t* cards, int64_t n, uint32_t* values, void* stream)
{
    if (!cards || !values) return fail(CS_E_INVALID, "null argument");
    if (n <= 0 || n > ((int64_t)1 << 31)) return fail(CS_E_INVALID, "n out of range");
    return done(cs::launch_debug_rank7(cards, n, values, (hipStream_t)stream), "cs_debug_holdem_rank7");
}

int cs_debug_mahjong_hu(const uint8_t* hands, const uint8_t* len, const uint8_t* piles, int64_t n, uint8_t* win,
                        void* stream)
{
    if (!hands || !len || !piles || !win) return fail(CS_E_INVALID, "null argument");
    if (n <= 0 || n > ((int64_t)1 << 31)) return fail(CS_E_INVALID, "n out of range");
    return done(cs::launch_debug_mahjong_hu(hands, len, piles, n, win, (hipStream_t)stream), "cs_debug_mahjong_hu");
}

int cs_debug_gin_melds(const uint8_t* hands, const uint8_t* len, int64_t n, int32_t* deadwood, uint64_t* knock,
                       uint64_t* gin, int32_t* gin_card, void* stream)
{
    if (!hands || !len || !deadwood || !knock || !gin || !gin_card) return fail(CS_E_INVALID, "null argument");
    if (n <= 0 || n > ((int64_t)1 << 31)) return fail(CS_E_INVALID, "n out of range");
    return done(cs::launch_debug_gin_melds(hands, len, n, deadwood, knock, gin, gin_card, (hipStream_t)stream),
                "cs_debug_gin_melds");
}

int cs_debug_ddz_legal(cs_handle* h, const uint8_t* counts, const int32_t* prev, int64_t n, uint8_t* legal,
                       void* stream)
{
    if (!h || !counts || !prev || !legal) return fail(CS_E_INVALID, "null argument");
    if (h->b.game != CS_GAME_DOUDIZHU) return fail(CS_E_UNSUPPORTED, "cs_debug_ddz_legal needs a doudizhu handle");
    if (n <= 0 || n > ((int64_t)1 << 31)) return fail(CS_E_INVALID, "n out of range");
    int r = set_device(h);
    if (r != CS_OK) return r;
    return done(cs::ddz::launch_debug_legal(h->b, counts, prev, n, legal, (hipStream_t)stream), "cs_debug_ddz_legal");
}

int cs_debug_set_serial_refill(cs_handle* h, int32_t enable)
{
    if (!h) return fail(CS_E_INVALID, "null argument");
    h->b.kernel_flags = (h->b.kernel_flags & ~1) | (enable ? 1 : 0);
    return CS_OK;
}

int cs_debug_set_kernel_flags(cs_handle* h, int32_t flags)
{
    if (!h) return fail(CS_E_INVALID, "null argument");
    if (flags < 0 || flags > 7) return fail(CS_E_INVALID, "unknown kernel flag bits");
    h->b.kernel_flags = flags;
    return CS_OK;
}

}  // extern "C"
