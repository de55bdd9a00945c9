// cs_kernels.hip -- lockstep env kernels for gfx950 (one lane = one env, one wave = 64 consecutive envs).
//
// The kernel skeleton (cs_skeleton.h) instantiated for the heads-up hold'em games and Blackjack; 3..22-player hold'em
// is instantiated in cs_holdem_n*.hip, the Blackjack shoe in cs_blackjack_shoe.hip. find_game maps a game id and
// cs_config to the launch table entry (cs_engine.h GameOps) of its type; this is the one place that decides it, and
// cs_abi.cpp asks once per handle.
#include "cs_skeleton.h"
#include "cs_leduc.h"
#include "cs_limit.h"
#include "cs_blackjack.h"
#include "cs_doudizhu.h"
#include "cs_nolimit.h"
#include "cs_uno.h"
#include "cs_mahjong.h"
#include "cs_gin_rummy.h"
#include "cs_bridge.h"
#include "cs_scout.h"

namespace cs {

// DouDizhu: its own kernels (cs_doudizhu.hip: a wave per env, env-major state, two 624-word MT blocks per env)
static const GameOps* ddz_ops()
{
    static const GameOps ops = [] {
        cs_game_info info{};
        info.obs_dim = ddz::OBS;
        info.num_actions = ddz::NA;
        info.num_players = ddz::P;
        info.legal_bytes = ddz::LB;
        info.action_bytes = 2;
        info.state_words = ddz::WORDS;
        info.action_feature_dim = 54;
        info.rng_period = 2 * 624;
        info.game_words = ddz::WORDS;
        info.envs_per_wave = 2;   // k_rollout2: one env per half-wave
        return GameOps{ddz::launch_seed, ddz::launch_reset, ddz::launch_step, ddz::launch_observe,
                       ddz::launch_rollout, info, 0, 2 * 624, false, true};
    }();
    return &ops;
}

const GameOps* find_game(int32_t game, const cs_config* cfg)
{
    const int32_t np = cfg ? cfg->num_players : 0;   // <= 0: the game's default
    switch (game) {
    case CS_GAME_LEDUC:
    case CS_GAME_LIMIT:
        if (np > 2) return find_holdem_n(game, np);
        if (np != 0 && np != 2) return nullptr;
        return game == CS_GAME_LEDUC ? ops_of<Leduc>() : ops_of<Limit>();
    case CS_GAME_BLACKJACK: {
        const int32_t p = np > 0 ? np : 1, nd = (cfg && cfg->num_decks >= 0) ? cfg->num_decks : 1;
        // the byte-ring kernel (cs_blackjack.h) covers one deck and at most 4 players; the rest (which only a cfg
        // asks for) are shoes
        if (p > 4 || nd > 1) return find_blackjack_shoe(p, nd, cfg->rng_mode);
        switch (p) {
        case 1: return ops_of<Blackjack<1>>();
        case 2: return ops_of<Blackjack<2>>();
        case 3: return ops_of<Blackjack<3>>();
        default: return ops_of<Blackjack<4>>();
        }
    }
    case CS_GAME_NOLIMIT: {
        const int32_t p = np > 0 ? np : 2;
        if (cfg && (cfg->chips_for_each < 0 || cfg->chips_for_each > 255 || cfg->dealer_plus1 < 0 ||
                    cfg->dealer_plus1 > p))
            return nullptr;
        if (p > 2) return find_holdem_n(game, p);
        return p == 2 ? ops_of<Nolimit>() : nullptr;
    }
    case CS_GAME_UNO: return (np == 0 || np == Uno::P) ? ops_of<Uno>() : nullptr;   // (cs_create names the refusal)
    case CS_GAME_MAHJONG: return (np == 0 || np == Mahjong::P) ? ops_of<Mahjong>() : nullptr;   // (as UNO)
    case CS_GAME_GIN_RUMMY: return (np == 0 || np == GinRummy::P) ? ops_of<GinRummy>() : nullptr;   // (as UNO)
    case CS_GAME_BRIDGE: return (np == 0 || np == Bridge::P) ? ops_of<Bridge>() : nullptr;   // (as UNO)
    case CS_GAME_SCOUT: return (np == 0 || np == Scout::P) ? ops_of<Scout>() : nullptr;   // (as UNO)
    case CS_GAME_DOUDIZHU: return (np == 0 || np == ddz::P) ? ddz_ops() : nullptr;
    default: return nullptr;
    }
}

// Test hook (cs_debug_holdem_rank7): the showdown evaluator of the hold'em kernels (tally_card + holdem_rank7, the
// functions holdem_showdown and Limit's game end call) on arbitrary 7-card hands, one thread per hand
__global__ __launch_bounds__(BLOCK) void k_debug_rank7(const int8_t* __restrict__ cards, int64_t n, uint32_t* values)
{
    const int64_t i = (int64_t)blockIdx.x * BLOCK + threadIdx.x;
    if (i >= n) return;
    uint64_t cnt = 0, sm = 0;
#pragma unroll
    for (int k = 0; k < 7; k++) tally_card((int)cards[i * 7 + k], cnt, sm);
    values[i] = holdem_rank7(cnt, sm);
}

hipError_t launch_debug_rank7(const int8_t* cards, int64_t n, uint32_t* values, hipStream_t s)
{
    hipLaunchKernelGGL(k_debug_rank7, dim3((unsigned)((n + BLOCK - 1) / BLOCK)), dim3(BLOCK), 0, s, cards, n, values);
    return hipGetLastError();
}

// Test hook (cs_debug_mahjong_hu): the win judge of the Mahjong kernels (cs_mahjong_hu.h judge_hu) on arbitrary ordered
// hands, one thread per hand
__global__ __launch_bounds__(BLOCK) void k_debug_mahjong_hu(const uint8_t* __restrict__ hands,
                                                            const uint8_t* __restrict__ len,
                                                            const uint8_t* __restrict__ piles, int64_t n, uint8_t* win)
{
    const int64_t i = (int64_t)blockIdx.x * BLOCK + threadIdx.x;
    if (i >= n) return;
    uint32_t h[4] = {0u, 0u, 0u, 0u};
#pragma unroll
    for (int k = 0; k < mj::HAND_MAX; k++) h[k >> 2] |= (uint32_t)hands[i * mj::HAND_MAX + k] << (8 * (k & 3));
    win[i] = (uint8_t)mj::judge_hu(h, (int)len[i], (int)piles[i]);
}

hipError_t launch_debug_mahjong_hu(const uint8_t* hands, const uint8_t* len, const uint8_t* piles, int64_t n,
                                   uint8_t* win, hipStream_t s)
{
    hipLaunchKernelGGL(k_debug_mahjong_hu, dim3((unsigned)((n + BLOCK - 1) / BLOCK)), dim3(BLOCK), 0, s, hands, len,
                       piles, n, win);
    return hipGetLastError();
}

// Test hook (cs_debug_gin_melds): the meld judge of the Gin Rummy kernels (cs_gin_melds.h) on arbitrary ordered hands,
// one thread per hand
__global__ __launch_bounds__(BLOCK) void k_debug_gin_melds(const uint8_t* __restrict__ hands,
                                                           const uint8_t* __restrict__ len, int64_t n,
                                                           int32_t* deadwood, uint64_t* knock, uint64_t* gin_o,
                                                           int32_t* gin_card)
{
    const int64_t i = (int64_t)blockIdx.x * BLOCK + threadIdx.x;
    if (i >= n) return;
    uint32_t h[gin::HAND_WORDS] = {0u, 0u, 0u};
#pragma unroll
    for (int k = 0; k < gin::HAND_MAX; k++) h[k >> 2] |= (uint32_t)hands[i * gin::HAND_MAX + k] << (8 * (k & 3));
    const int ln = len[i] <= gin::HAND_MAX ? (int)len[i] : gin::HAND_MAX;
    deadwood[i] = gin::best_deadwood(h, ln);
    uint64_t kn = 0, g = 0;
    int card = -1;
    if (ln == gin::HAND_MAX) {
        gin::going_out<true>(h, ln, &kn, &g);
        card = gin::gin_card(h, ln);
    }
    knock[i] = kn;
    gin_o[i] = g;
    gin_card[i] = card;
}

hipError_t launch_debug_gin_melds(const uint8_t* hands, const uint8_t* len, int64_t n, int32_t* deadwood,
                                  uint64_t* knock, uint64_t* gin_o, int32_t* gin_card, hipStream_t s)
{
    hipLaunchKernelGGL(k_debug_gin_melds, dim3((unsigned)((n + BLOCK - 1) / BLOCK)), dim3(BLOCK), 0, s, hands, len, n,
                       deadwood, knock, gin_o, gin_card);
    return hipGetLastError();
}

}  // namespace cs
