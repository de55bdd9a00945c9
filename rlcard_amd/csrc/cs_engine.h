// cs_engine.h -- internal interface between the C ABI (cs_abi.cpp) and the kernels: the device buffers of a handle, the
// per-game-type launch table (GameOps, find_game) and the launchers of the game-independent kernels.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "../../include/cardsim.h"
#include "cs_devbuf.h"

namespace cs {

// Byte-ring slots of the lane-per-env games' MT19937 streams (cs_ring.h): 16 = 15 blocks twisted per refill from one
// read and one write of the block words (8: seven, 4: three)
constexpr int RING_SLOTS_HOST = 16;
constexpr int RING_ENV_WORDS_HOST = 624 + RING_SLOTS_HOST * 624 / 4;   // u32 per env: block words + the ring bytes

// cs_set_step_record: the single-step kernels also write env `env`'s packed state words to `words`, then -- after a
// system-scope fence that orders every output store of that env's wave -- `seqv` to *seq (both typically in mapped
// host memory), so a single-env host can spin on *seq instead of synchronising the stream
struct StepRecord {
    uint32_t* words;
    uint32_t* seq;
    uint32_t seqv;
    int64_t env;
};

struct Buffers {
    int32_t game;
    int64_t n;
    uint32_t* mt;     // the envs' RNG words: [n][GameOps::mt_words], or [mt_words][n] where GameOps::mt_columns
    uint32_t* ctl;    // [n]
    uint32_t* state;  // [state_words][n] (lane-per-env games) or [n][state_words] (doudizhu, wave per env)
    uint32_t* sctl;   // [n] rollout MT staging: staged stream position | staged count << 16
    uint8_t* sbuf;    // [n][stage bytes] rollout MT staging rows persisted between launches
    const void* table;  // game-specific read-only table (doudizhu action table), or null
    int32_t num_players, num_decks;
    int32_t chips_for_each, dealer_id;   // no-limit hold'em (cs_config; dealer_id -1 = drawn)
    int32_t kernel_flags;   // cs_debug_set_kernel_flags bits 0..2 (bit 0 alone: cs_debug_set_serial_refill)
    int32_t rng_mode;       // cs_config.rng_mode
    StepRecord rec;         // seq == nullptr: off
    int32_t obs_dim, num_actions, action_bytes;   // cs_game_info of the handle
};

// DMC actor-buffer ring of a handle (cs_dmc.hip): per (env, player) stream, `slots` chunks of T rows
struct DmcRing {
    int32_t T, slots, F;          // rows per chunk, chunks per stream, action feature bytes
    int8_t* st;                   // [streams][slots][T][obs_dim]
    int8_t* act;                  // [streams][slots][T][F]
    float* tgt;                   // [streams][slots][T]
    float* ret;
    uint8_t* dne;
    int64_t* ctr;                 // [streams] rows appended
    int64_t* gstart;              // [streams] first row of the game in progress
    int64_t* emitted;             // [streams] chunks handed out
    int32_t* counts;              // [streams + 1] chunks ready in the last fill (last entry 0)
    int64_t* offsets;             // [streams + 1]
    uint32_t* flag;               // bit 0: rows dropped (ring full)
};

// One concrete game type -- a Game class of the skeleton (cs_skeleton.h ops_of<G>), the Blackjack shoe or DouDizhu: its
// five launchers and the facts the ABI layer needs about it. cs_create looks it up once (find_game) and the handle
// keeps the pointer: the allocation and every launch follow the same descriptor.
struct GameOps {
    hipError_t (*seed)(const Buffers& b, const uint32_t* keys_dev, const int32_t* klen_dev, int64_t first,
                       int64_t count, hipStream_t s);
    hipError_t (*reset)(const Buffers& b, const cs_step_out& o, hipStream_t s);
    hipError_t (*step)(const Buffers& b, const int32_t* actions, const cs_step_out& o, hipStream_t s);
    hipError_t (*observe)(const Buffers& b, int32_t player, const cs_step_out& o, hipStream_t s);
    hipError_t (*rollout)(const Buffers& b, int32_t T, uint64_t seed, uint64_t t0, uint64_t env_base,
                          const cs_traj_out& o, hipStream_t s);
    cs_game_info info;      // what cs_game_info_get reports
    int32_t stage_bytes;    // rollout MT staging row per env (Buffers::sbuf), 0: none
    int32_t mt_words;       // u32 per env in Buffers::mt
    bool mt_columns;        // word k of env e at mt[k * n + e] (the shoe) instead of mt[e * mt_words + k]
    bool env_major;         // state is [n][state_words] (DouDizhu) instead of [state_words][n]
    // Rule policies (include/cardsim.h CS_POLICY_*), null where the type has none (every positional initialiser above
    // leaves them so): the rollout with seat p playing byte p of `seats`, and one policy's action per env
    hipError_t (*rollout_policy)(const Buffers& b, int32_t T, uint64_t seed, uint64_t t0, uint64_t env_base,
                                 uint32_t seats, const cs_traj_out& o, hipStream_t s);
    hipError_t (*policy_actions)(const Buffers& b, int32_t policy, uint64_t seed, uint64_t t, uint64_t env_base,
                                 int32_t* actions, hipStream_t s);
    int32_t max_policy;     // largest CS_POLICY_* id the two launchers take
};

// The type that serves `cfg` (null: the game's defaults), or null where the engine has none (cs_kernels.hip). The
// other units each export one function, the finder of the types they instantiate (null for any other):
const GameOps* find_game(int32_t game, const cs_config* cfg);
const GameOps* find_holdem_n(int32_t game, int32_t num_players);     // cs_holdem_n.hip: 3..6 (Leduc 3..5) + the next 3
const GameOps* find_holdem_n10(int32_t game, int32_t num_players);   // cs_holdem_n10.hip: Limit / No-limit 7..10
const GameOps* find_holdem_n16(int32_t game, int32_t num_players);   // cs_holdem_n16.hip: 11..16
const GameOps* find_holdem_n22(int32_t game, int32_t num_players);   // cs_holdem_n22.hip: 17..22
// cs_blackjack_shoe.hip: Blackjack up to 7 players and 8 decks (word-stream RNG, materialised shoe; MT19937 only)
const GameOps* find_blackjack_shoe(int32_t num_players, int32_t num_decks, int32_t rng_mode);

// cs_dmc.hip
hipError_t launch_dmc_fill(const Buffers& b, const DmcRing& d, int32_t T, const cs_traj_out& tr, int64_t* ready,
                           int64_t cap, int64_t* nready, int64_t* dst, DevBuf& scan, hipStream_t s);
hipError_t launch_dmc_gather(const DmcRing& d, int32_t state_dim, int32_t obs_dim, const int64_t* chunks,
                             int64_t count, const cs_dmc_batch& o, hipStream_t s);
hipError_t launch_dmc_layer1(const float* X, const int32_t* state_of, const int32_t* ids, int64_t E, int32_t H,
                             const float* Wa, const float* b1, int32_t F, const Buffers& b, float* h1, hipStream_t s);
hipError_t launch_dmc_select(const float* values, const int32_t* counts, const int64_t* offsets, const int32_t* ids,
                             int64_t S, float eps, uint64_t seed, uint64_t t, uint64_t base, int32_t* actions,
                             hipStream_t s);

// cs_cfr.hip: chance-sampling CFR tables on Leduc (device pointers, [CFR_NI][4] fp64 + [CFR_NI] u32 flags)
constexpr int CFR_NI = 2700;
struct CfrTables {
    double* policy;
    double* avg;
    double* regrets;
    uint32_t* flags;
};
// scratch (batched mode, n > 1): the deals' table contributions, reduced in a fixed order (cs_cfr.hip); handle-owned
hipError_t launch_cfr(const Buffers& b, int32_t iterations, int64_t iteration0, const CfrTables& t, DevBuf& scratch,
                      hipStream_t s);

// cs_traj.hip
hipError_t launch_traj_probe(const Buffers& b, int32_t T, const cs_traj_out& tr, int32_t obs_dim, int32_t legal_bytes,
                             int32_t action_bytes, int32_t epw, hipStream_t s);
hipError_t launch_transitions(const Buffers& b, int32_t T, const cs_traj_out& tr, const cs_trans_out& o,
                              hipStream_t s);
hipError_t launch_payoff_sums(const Buffers& b, int32_t T, const cs_traj_out& tr, int32_t quota, int32_t* games_per_env,
                              double* sums, int64_t* games, hipStream_t s);
hipError_t launch_legal_lists(const Buffers& b, int32_t lb, const uint8_t* legal, int64_t rows, int32_t* counts,
                              int64_t* offsets, int32_t* ids, DevBuf& scan, hipStream_t s);
hipError_t launch_onehot(const int32_t* ids, int64_t count, int32_t na, uint8_t* out, hipStream_t s);
hipError_t launch_copy_state(const Buffers& b, int64_t env, int32_t sw, int32_t env_major, uint32_t* dst,
                             hipStream_t s);
hipError_t launch_rng_copy(const Buffers& b, int64_t env, int32_t mtw, int32_t column, uint32_t clear_mask,
                           uint32_t* buf, int32_t load, hipStream_t s);   // cs_traj.hip
hipError_t launch_debug_rank7(const int8_t* cards, int64_t n, uint32_t* values, hipStream_t s);   // cs_kernels.hip
hipError_t launch_debug_mahjong_hu(const uint8_t* hands, const uint8_t* len, const uint8_t* piles, int64_t n,
                                   uint8_t* win, hipStream_t s);   // cs_kernels.hip

hipError_t launch_debug_gin_melds(const uint8_t* hands, const uint8_t* len, int64_t n, int32_t* deadwood,
                                  uint64_t* knock, uint64_t* gin, int32_t* gin_card, hipStream_t s);   // cs_kernels.hip

namespace ddz {   // cs_doudizhu.hip
hipError_t launch_seed(const Buffers& b, const uint32_t* keys_dev, const int32_t* klen_dev, int64_t first,
                       int64_t count, hipStream_t s);
hipError_t launch_reset(const Buffers& b, const cs_step_out& o, hipStream_t s);
hipError_t launch_step(const Buffers& b, const int32_t* actions, const cs_step_out& o, hipStream_t s);
hipError_t launch_observe(const Buffers& b, int32_t player, const cs_step_out& o, hipStream_t s);
hipError_t launch_rollout(const Buffers& b, int32_t T, uint64_t seed, uint64_t t0, uint64_t env_base,
                          const cs_traj_out& o, hipStream_t s);
hipError_t launch_features(const Buffers& b, const int32_t* ids, int64_t count, uint8_t* out, hipStream_t s);
hipError_t launch_debug_legal(const Buffers& b, const uint8_t* counts, const int32_t* prev, int64_t n,
                              uint8_t* legal, hipStream_t s);
}  // namespace ddz

}  // namespace cs
