/*
 * cardsim.h -- C ABI of the MI355X-native batched card-game engine (rlcard_amd).
 *
 * The reference (pmcgannon22/rlcard) has no FFI: its env path is pure Python. This ABI is the
 * boundary a binding (ctypes here: rlcard_amd/_abi.py; cgo/JNI/N-API stubs in INTEGRATION.md) calls to replace,
 * for a whole batch of envs at once, the reference calls listed per entry point. POD types only, 64-bit sizes,
 * no exceptions across the boundary: every call returns CS_OK (0) or a negative CS_E_* code, and
 * cs_last_error() returns a thread-local message for the last failure on the calling thread.
 *
 * Ownership: env state and the per-env MT19937 streams live in device memory owned by the handle. Every output
 * buffer is caller-owned DEVICE memory (e.g. torch tensors' data_ptr()) with the documented shape/dtype, C-contiguous.
 * All work is enqueued asynchronously on the caller's hipStream_t (`stream`, NULL = default stream); a handle is not
 * thread-safe: drive it from one stream/thread. One handle per GPU.
 */
#ifndef RLCARD_AMD_CARDSIM_H
#define RLCARD_AMD_CARDSIM_H
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

enum {
    CS_OK = 0,
    CS_E_INVALID = -1,   /* bad argument (null pointer, size, config) */
    CS_E_DEVICE = -2,    /* HIP runtime error (no device, launch failure, out of memory) */
    CS_E_STATE = -3,     /* call out of order (e.g. reset before seed) */
    CS_E_UNSUPPORTED = -4
};

/* game ids; names as registered by rlcard/envs/__init__.py:6-54 (CS_GAME_UNO: 'uno', two players; CS_GAME_MAHJONG:
 * 'mahjong', four players; CS_GAME_GIN_RUMMY: 'gin-rummy', two players, the reference's default Settings;
 * CS_GAME_BRIDGE: 'bridge', four players, the reference's default payoff delegate and state extractor;
 * CS_GAME_SCOUT: 'scout', four players, hands of up to 16 cards of ranks 1..10. Id 9 stays unassigned: it is the id
 * the ABI's own tests have always used for "no such game", and cs_game_info_get / cs_create keep refusing it) */
enum { CS_GAME_BLACKJACK = 0, CS_GAME_LEDUC = 1, CS_GAME_LIMIT = 2, CS_GAME_DOUDIZHU = 3, CS_GAME_NOLIMIT = 4,
       CS_GAME_UNO = 5, CS_GAME_MAHJONG = 6, CS_GAME_GIN_RUMMY = 7, CS_GAME_BRIDGE = 8, CS_GAME_SCOUT = 10 };

typedef struct cs_handle cs_handle;

/* Game configuration: the 'game_*' keys Env.__init__ forwards to Game.configure (rlcard/envs/env.py:33-39). */
typedef struct {
    int32_t num_players; /* blackjack 'game_num_players' (default 1); leduc/limit/no-limit 2; doudizhu 3 (0 = default);
                            uno 2 only: any other count is CS_E_UNSUPPORTED (the reference's payoffs[1 - winner]);
                            mahjong 4 only: any other count is CS_E_UNSUPPORTED; gin-rummy 2 only, bridge 4 only and scout 4 only,
                            likewise */
    int32_t num_decks;   /* blackjack 'game_num_decks' (default 1, 0 = infinite); ignored elsewhere (-1 = default) */
    int32_t chips_for_each; /* no-limit 'chips_for_each' (nolimitholdem/game.py:45-56): stack, 1..255 (0 = 100) */
    int32_t dealer_plus1;   /* no-limit 'dealer_id' + 1: 0 = None (drawn by the first game, then kept), 1..N fixed */
    int32_t rng_mode;       /* CS_RNG_MT19937 (0): every env draws numpy's RandomState stream of its seed, bit-exact
                               with the reference; CS_RNG_PHILOX (1): a counter-based Philox4x32-10 byte stream keyed
                               by the same seed key -- same games and rules, NOT the reference's deals; no MT19937
                               state traffic (every game; doudizhu draws the same byte stream) */
    int32_t reserved[3];
} cs_config;

enum { CS_RNG_MT19937 = 0, CS_RNG_PHILOX = 1 };

/* Static shape of a game (rlcard Env.num_players / num_actions / state_shape). */
typedef struct {
    int32_t obs_dim;      /* bytes per obs row: leduc 36, limit 72, no-limit 54, blackjack 2, doudizhu 901 (landlord 790),
                             uno 240 ([4][4][15] row-major, every row holds exactly 61 ones), mahjong 816 ([6][34][4]
                             row-major: hand, table, the four players' piles; a tile's row is 1 in columns < its count),
                             gin-rummy 260 ([5][52] row-major, always the CURRENT player's: hand, top discard, the other
                             discards, the opponent's known cards, stock + the opponent's cards not known; all zero once
                             the game is over), bridge 573 (always the CURRENT player's: hands [4][52], trick pile [4][52]
                             by seat, hidden cards [52], vul [4], dealer [4], current player [4], bidding over [1],
                             bidding_rep [40] at bytes 481..520 -- the action ids 1..38 of the first 40 - dealer calls
                             from index dealer on, RAW values, every other byte is 0/1 --, last call [39] by id, bid
                             amount [8], trump [5]; card id = 13 * suit + rank, suits C D H S, ranks 2..A), scout 688 (the asking
                             seat's: hand by top and by bottom, table set by top and by bottom [4][16][10], hand and
                             table occupancy [2][16], owner one-hot [5] with its last byte, 676, for no owner, then RAW
                             integers where the reference has fractions: consecutive scouts 677 (x / 3), the four hand
                             counts 678..681 (x / 16), the seat's points 682, 683 low byte first (x / 16), table length
                             684 (x / 16), forced scout 685 (0/1), the tops of the table's front and back card 686, 687
                             (x / 10); the reference's order is points, table length, orientation flag (always 0), and
                             rlcard_amd/envs/scout.py maps a row to its float32 vector) */
    int32_t num_actions;  /* leduc/limit 4, no-limit 5, blackjack 2, doudizhu 27472, uno 61 (8 legal bytes),
                             mahjong 38 (5 legal bytes: tiles 0..33, pong 34, chow 35, gong 36, stand 37),
                             gin-rummy 110 (14 legal bytes, bits 110 and 111 always 0: score north 0, score south 1,
                             draw 2, pick up 3, dead hand 4, gin 5, discard card c 6 + c, knock card c 58 + c, card id =
                             rank + 13 * suit with ranks A 2 .. K and suits S H D C),
                             bridge 91 (12 legal bytes, bits 91..95 always 0: no_bid 0 is never legal, bids 1..35 = 1 + 5 *
                             (amount - 1) + strain with strains C D H S NT, pass 36, dbl 37, rdbl 38, play card c 39 + c),
                             scout 204 (26 legal bytes, bits 204..207 always 0: play-s-e, the hand slice [s, e), 16 s -
                             s (s - 1) / 2 + e - s - 1 for 0 <= s < e <= 16; scout at insertion point i 136 + 4 i + k, k = 0
                             front, 1 front flipped, 2 back, 3 back flipped) */
    int32_t num_players;
    int32_t legal_bytes;  /* ceil(num_actions / 8): legal-action bitmask bytes per row */
    int32_t action_bytes; /* dtype width of rollout action rows: 1 (uint8) or 2 (int16, doudizhu) */
    int32_t state_words;  /* packed u32 words of game state per env */
    int32_t action_feature_dim; /* bytes per cs_action_features row: doudizhu 54, otherwise num_actions (one-hot) */
    int32_t rng_period;   /* draws after which the stream position of cs_get_rng_ctl wraps: doudizhu 1 248 (two word
                             blocks), the others the byte ring's 9 984 (16 slots of 624) */
    int32_t game_words;   /* packed game words at the start of the state_words (cs_get_env_state); = state_words for
                             every game without a deal queue */
    int32_t deal_queue_depth; /* DQ: deals the rollout may draw ahead (heads-up Limit / No-limit hold'em: 8 in this
                             build; 0 = no queue). state_words = game_words + 1 + 2 * DQ when DQ > 0; layout at
                             cs_get_env_state */
    int32_t envs_per_wave; /* envs one 64-lane wave of cs_rollout plays (doudizhu 2, heads-up Limit / No-limit 32,
                             otherwise 64): the write pattern cs_traj_probe reproduces */
} cs_game_info;
/* cs_game_info grows at its end between ABI versions (2: game_words, deal_queue_depth, envs_per_wave; 3 adds the
 * cs_state_* functions); a consumer built against this header checks cs_abi_version() >= CS_ABI_VERSION before
 * calling cs_game_info_get, which writes sizeof(cs_game_info) bytes of this version. Functions added without a
 * layout change keep the version (cs_rollout_policy, cs_policy_actions, cs_payoff_sums; cs_qnet_values,
 * cs_qnet_actions, the cs_replay_* functions, cs_dqn_targets, cs_dqn_train; cs_pnet_probs, cs_nfsp_scratch_bytes, cs_nfsp_actions,
 * the cs_reservoir_* functions): a consumer that may meet an older library looks the symbol up. */
#define CS_ABI_VERSION 3

/* Outputs of reset/step/observe, all device pointers, one row per env:
 *   obs    uint8  [n][obs_dim]     the current player's observation (values 0/1; blackjack: the two scores;
 *                                  no-limit: 52 card bits, then my chips and the largest chips in the pot)
 *   legal  uint8  [n][legal_bytes] legal-action bitmask, bit a of byte a/8 (LSB first) = action id a
 *   player uint8  [n]              current player id (Env.get_player_id)
 *   reward float  [n][num_players] payoffs of the transition (non-zero only where done; Env.get_payoffs). f32 of the
 *                                  reference's float64 payoffs, and exact for every payoff a game can reach: Leduc
 *                                  (judger.py:50-56) splits total / #winners among at most 2 winners (2 cards per
 *                                  rank; 3..5 players included), so its payoffs are multiples of 0.25; hold'em pays
 *                                  whole chips (/ 2 big blinds in Limit), Blackjack +-1 / 0, DouDizhu 0 / 1
 *                                  (tests/test_reward_precision.py enumerates them)
 *   done   uint8  [n]              1 if the game is over after this call (Env.is_over)
 * Any pointer may be NULL to skip that output. */
typedef struct {
    void* obs;
    void* legal;
    void* player;
    void* reward;
    void* done;
} cs_step_out;

/* Rollout trajectory, all device pointers, rows [T][n]:
 *   obs [T][n][obs_dim] u8, legal [T][n][legal_bytes] u8, player [T][n] u8 (the acting player's pre-step view),
 *   action [T][n] (uint8 or int16 per cs_game_info.action_bytes), reward [T][n][num_players] f32, done [T][n] u8,
 *   final_obs [T][n][num_players][obs_dim] u8 OPTIONAL (NULL = skip): where done[t][e] = 1, every player's observation
 *   of the finished game (the final states Env.run appends, envs/env.py:161-164); other rows are not written. */
typedef struct {
    void* obs;
    void* legal;
    void* player;
    void* action;
    void* reward;
    void* done;
    void* final_obs;
} cs_traj_out;

/* Transitions of a rollout trajectory, all device pointers [T][n] (any may be NULL to skip it):
 *   next_t i32   row of the acting player's next observation in the same game (obs[next_t][e]); -1 = the game ended
 *                first (next state = final_obs[end_t][e][player]); -2 = the game continues past the window
 *   end_t  i32   row where the row's game ends, -1 = past the window
 *   reward f32   the acting player's payoff on its last transition of the game, else 0
 *   done   u8    1 on that last transition
 *   ret    f32   the acting player's payoff of the game (DMC target), NaN if the game ends past the window */
typedef struct {
    void* next_t;
    void* end_t;
    void* reward;
    void* done;
    void* ret;
} cs_trans_out;

/* Shape of a game under a config. Replaces reading Env.num_players / num_actions / state_shape. */
int cs_game_info_get(int32_t game, const cs_config* cfg, cs_game_info* info);

/* Create n envs of `game` on HIP device `device`. Replaces rlcard.make(env_id, config) (envs/registration.py:77-89)
 * for n independent envs; allocates state (state_words*4 B/env) + the MT19937 streams in HBM: lane games' byte ring
 * 12 480 B/env (624 block words + 16 x 624 ring bytes), doudizhu 4 992 B/env, Blackjack shoes 2 496 B/env. */
int cs_create(cs_handle** out, int32_t game, int64_t num_envs, int32_t device, const cs_config* cfg);
void cs_destroy(cs_handle* h);

/* Seed envs [first_env, first_env + n) from init_by_array keys computed on the host from each env's seed
 * (rlcard/utils/seeding.py:33-113): keys [n][2] u32 (HOST memory), key_len [n] (1 or 2). Replaces Env.seed(seed)
 * (envs/env.py:228-231). Marks those envs as finished (the next reset/step starts a game). */
int cs_seed(cs_handle* h, const uint32_t* keys, const int32_t* key_len, int64_t first_env, int64_t n, void* stream);

/* Start a new game in every env. Replaces Env.reset() (envs/env.py:52-63) -> Game.init_game + _extract_state. */
int cs_reset(cs_handle* h, const cs_step_out* out, void* stream);

/* One Env.step (envs/env.py:65-86) per env with actions [n] int32 (DEVICE memory). Illegal ids follow the
 * reference's _decode_action (envs/leducholdem.py:81-96, limitholdem.py:81-96); where the reference is undefined the
 * ABI defines the step -- UNO: an illegal id plays the lowest legal id (the reference draws a legal id from the global
 * np.random), and a deal or draw that finds fewer cards than it needs even after replace_deck takes the cards that are
 * there (the reference raises IndexError); Mahjong: an illegal id plays the lowest legal id (the reference raises),
 * a game already won on the deal is done = 1 at the reset row with zero rewards, and a finished game's legal mask may
 * be zero; Gin Rummy: an illegal id plays the lowest legal id (the reference raises or corrupts its lists), the game
 * ends (done = 1, payoffs) at the step that plays `score south`, and its state has no undo (the reference's step_back
 * raises NotImplementedError); Bridge: an illegal id plays the lowest legal id (the reference raises), four opening
 * passes end the game with zero payoffs and the last passer as the current player, a game takes up to 371 steps, and
 * state words that hold no game (cs_set_env_state) load as a finished game; Scout: an illegal id plays the lowest legal
 * id (the reference raises), a game has no length bound, a finished game's legal mask and forced-scout flag are those of
 * the seat the turn passed to (as the reference shows them), a score saturates at 65 535, and state words that hold no
 * game load as a finished game. Envs whose game was already over
 * start a new game instead (lazy auto-reset: action ignored, done = 0, reward = 0), so an RL loop never calls
 * reset() per env. */
int cs_step(cs_handle* h, const int32_t* actions, const cs_step_out* out, void* stream);

/* Observation of `player` in every env without changing state. Replaces Env.get_state(player_id)
 * (envs/env.py:188-197), e.g. the final states Env.run appends for every player (env.py:161-164). */
int cs_observe(cs_handle* h, int32_t player, const cs_step_out* out, void* stream);

/* T fused lockstep steps with an in-kernel uniform-random policy over the legal actions (the random-agent
 * benchmark policy of examples/run_random.py, agents/random_agent.py:17-47, with the global np.random replaced by
 * Philox4x32-10 keyed by (policy_seed) on counter (env_base + env, t0 + t)). A finished game restarts immediately.
 * Replaces T iterations of the Env.run loop (envs/env.py:120-169) for every env. */
int cs_rollout(cs_handle* h, int32_t T, uint64_t policy_seed, uint64_t t0, uint64_t env_base, const cs_traj_out* out,
               void* stream);

/* Policies the engine can play on the device, per seat of cs_rollout_policy or for the acting player of
 * cs_policy_actions. The rule policies restate the reference's rule models (rlcard/models/leducholdem_rule_models.py,
 * limitholdem_rule_models.py; the Python forms are rlcard_amd.models) on the packed game state:
 *   CS_POLICY_RANDOM   uniform over the legal actions, the policy of cs_rollout (same Philox counter, same pick)
 *   CS_POLICY_RULE_V1  Leduc: leduc-holdem-rule-v1 (raise, else call, else check, else fold);
 *                      Limit: limit-holdem-rule-v1 (hole-card classes against the board's ranks and suits)
 *                      UNO: uno-rule-v1 (rlcard/models/uno_rule_models.py): `draw` if legal; else, with a wild_draw_4
 *                      legal, the wild_draw_4 of the colour most frequent in the hand (wild cards left out unless the
 *                      hand is all wild, ties to the colour met first in hand order); else uniform over the legal ids
 *                      without the *-wild ids (kept if nothing else is legal) -- the reference draws that pick from the
 *                      global np.random, the engine from the step's policy word with CS_POLICY_RANDOM's formula, so a
 *                      rule seat's games are a function of policy_seed
 *                      Gin Rummy: gin-rummy-novice-rule (rlcard/models/gin_rummy_rule_models.py): gin if legal; else a
 *                      uniform pick among the knock ids; else among the discards after which the other 10 cards have
 *                      the least best deadwood; else among the legal ids -- every pick from the step's policy word
 *                      Bridge: BridgeDefenderNoviceRuleAgent (rlcard/models/bridge_rule_models.py): pass whenever it is
 *                      legal, else a uniform pick among the legal ids from the step's policy word
 *   CS_POLICY_RULE_V2  Leduc only: leduc-holdem-rule-v2 (raise on a rank match with the public card, else fold)
 * A hold'em rule that aims at an illegal action plays call for raise, fold for check and raise for call, as the reference
 * does. Rule policies exist for default 2-player Leduc, heads-up Limit hold'em, UNO, Gin Rummy and Bridge; with any other game or
 * player count a rule id returns CS_E_UNSUPPORTED (so does CS_POLICY_RULE_V2 on Limit, UNO, Gin Rummy and Bridge, and every rule id on
 * Mahjong and Scout, for which the reference has no rule model; cs_policy_actions(CS_POLICY_RANDOM) works there). */
enum { CS_POLICY_RANDOM = 0, CS_POLICY_RULE_V1 = 1, CS_POLICY_RULE_V2 = 2 };

/* cs_rollout with seat p playing seat_policy[p] (HOST array of num_players CS_POLICY_* ids): the way to play a fixed
 * baseline -- Env.run with models.load(name).agents (rlcard/utils/utils.py tournament) -- in the fused rollout. A
 * random seat picks exactly what cs_rollout picks at the same (policy_seed, env_base + env, t0 + t) and legal set, so
 * an all-random seat_policy gives cs_rollout's trajectory and end state byte for byte; a rule seat reads the env's game
 * state and draws nothing. Same outputs as cs_rollout. */
int cs_rollout_policy(cs_handle* h, int32_t T, uint64_t policy_seed, uint64_t t0, uint64_t env_base,
                      const int32_t* seat_policy, const cs_traj_out* out, void* stream);

/* The action `policy` takes for the current player of every env, without changing any state: actions int32 [n]
 * (DEVICE), -1 where the env's game is over (cs_step ignores that env's action and starts its next game). A random
 * pick is the one cs_rollout_policy makes at step counter t. Lets a learner stepping with cs_step take its opponents'
 * moves on the device (agent.eval_step of a rule agent for every env at once). */
int cs_policy_actions(cs_handle* h, int32_t policy, uint64_t policy_seed, uint64_t t, uint64_t env_base,
                      int32_t* actions, void* stream);

/* Tournament sums of a rollout trajectory of this handle (rlcard/utils/utils.py:200-225 tournament, for every env at
 * once): the payoff rows of the games that end inside `traj` (needs reward and done, [T][n] rows) are added to sums
 * (double [num_players], DEVICE) and counted in *games (int64, DEVICE), env e contributing a game only while
 * games_per_env[e] (int32 [n], DEVICE) is below `quota`, and counting it there. All three accumulate across calls (zero
 * them first), so over consecutive windows every env contributes exactly its first `quota` games: which games count
 * does not depend on where the windows end, and short games are not favoured. quota <= 0: no limit. The sums are exact
 * and independent of the order of addition wherever the payoffs are multiples of a power of two (every game here: see
 * cs_step_out reward). */
int cs_payoff_sums(cs_handle* h, int32_t T, const cs_traj_out* traj, int32_t quota, int32_t* games_per_env,
                   double* sums, int64_t* games, void* stream);

/* Placement probe of a trajectory allocation: zeros written into every non-NULL tensor of `out` ([T][n] rows, the
 * cs_rollout layout) in the rollout's write order, without game logic or state change. Where a trajectory lands in HBM
 * sets how fast it takes the rollout's writes (the same kernel runs 14 % slower in some allocations, and
 * this probe's time separates them exactly), so a caller can time it on a few candidate allocations and keep the
 * fastest (rlcard_amd.VecEnv.new_traj_out(select=k)). No reference counterpart (an allocation policy of this engine). */
int cs_traj_probe(cs_handle* h, int32_t T, const cs_traj_out* out, void* stream);

/* The whole engine state of a handle's envs -- MT streams, control words, game state, the rollout's staged stream rows
 * -- as one device buffer of cs_state_bytes bytes: cs_state_save copies it out, cs_state_load back in (async on
 * `stream`, device-to-device). A save / rollout / load sequence leaves the envs exactly as they were: how
 * rlcard_amd.VecEnv.new_traj_out times a real rollout on each candidate trajectory allocation without moving the
 * envs. The analogue of the reference's whole-game snapshot for step_back (rlcard/envs/env.py:88-106, the game's
 * deepcopy history), for every env at once. Since ABI version 3. */
int cs_state_bytes(const cs_handle* h, int64_t* bytes);
int cs_state_save(cs_handle* h, void* buf, void* stream);
int cs_state_load(cs_handle* h, const void* buf, void* stream);

/* rlcard's reorganize (utils/utils.py:153-179: per player [state, action, reward, next_state, done]) and the DMC
 * return target (agents/dmc_agent/utils.py:97-163) of a cs_rollout trajectory of this handle, on the device. `traj`
 * needs player, reward and done. Games still running at the end of the window come out as next_t = -2. */
int cs_transitions(cs_handle* h, int32_t T, const cs_traj_out* traj, const cs_trans_out* out, void* stream);

/* Legal-action id lists of `rows` legal bitmask rows of this game (wavefront compaction; the keys of
 * state['legal_actions']): counts i32 [rows], offsets i64 [rows + 1] (exclusive prefix sum, offsets[rows] = total),
 * ids i32 [total] ascending per row. ids may be NULL: size it from offsets[rows], then call again with it. */
int cs_legal_lists(cs_handle* h, const void* legal, int64_t rows, int32_t* counts, int64_t* offsets, int32_t* ids,
                   void* stream);

/* Action features of `count` action ids (Env.get_action_feature: doudizhu _cards2array of the combo, 54 B,
 * envs/doudizhu.py:136-142; other games one-hot of num_actions, envs/env.py:211-220): u8 [count][action_feature_dim]. */
int cs_action_features(cs_handle* h, const int32_t* ids, int64_t count, void* features, void* stream);

/* Chance-sampling CFR on Leduc Hold'em (rlcard/agents/cfr_agent.py:30-123) over this handle's envs: `iterations` x
 * CFRAgent.train(). Per iteration, for each player, every env deals a new game from its own stream (Env.reset) and
 * the whole betting tree under that deal is traversed with the reference's step / step_back recursion (traverse_tree),
 * accumulating regrets and the average policy; then regret matching updates the policy (update_policy). Tables are
 * caller-owned DEVICE buffers indexed by the Leduc observation the reference keys its dicts with
 * (((hand * 4 + public + 1) * 15 + my chips) * 15 + others' chips, 2700 rows): policy / average_policy / regrets
 * double [2700][4] (policy initialised to 0.25 = the reference's row for an unseen key), flags uint32 [2700] (bit 0:
 * key in policy, bit 1: key in regrets and average_policy), zero-initialised. iteration0 = the agent's iteration
 * count before this call. A 1-env handle is the reference agent, bit-exact (same fp64 operation order); with more
 * envs, each deals its own game per player per iteration and the tables add the deals' terms in one fixed order
 * (records sorted by infoset, then a sequential sum per segment: bit-exact with the oracle and run to run,
 * cs_cfr.hip). Leduc only. */
int cs_cfr_train(cs_handle* h, int32_t iterations, int64_t iteration0, double* policy, double* average_policy,
                 double* regrets, uint32_t* flags, void* stream);

/* ---- DMC learner side (rlcard/agents/dmc_agent/) ----------------------------------------------------------------
 * Actor buffers (utils.py:97-163 act): every (env, player) of a handle keeps its stream of transitions -- state = the
 * obs the player acted on (int8 [obs_dim]), action = Env.get_action_feature of its action (int8 [action_feature_dim]),
 * target = the player's payoff of that game on each of its rows, done / episode_return set on its last row of the
 * game -- and a T-row chunk is handed out once more than T rows of finished games are queued (`while size[p] > T`).
 * The streams live in a ring of `slots` chunks per (env, player) in HBM. Chunk ids handed out by cs_dmc_fill must be
 * gathered (cs_dmc_gather) before the next cs_dmc_fill reuses their slots; rows that would overwrite a chunk still
 * held are dropped and flagged (cs_dmc_status). Needs slots * T >= T + the rows one fill adds per (env, player) +
 * the longest game's rows.
 * Lifetime of the buffers created on a handle (cs_dmc, cs_replay, cs_reservoir): a buffer may be destroyed after its
 * handle; every other call on it needs the handle alive. */
typedef struct cs_dmc cs_dmc;

/* get_batch (utils.py:33-46) output, DEVICE pointers, [T][B] rows (any may be NULL):
 *   state int8 [T][B][state_dim(player)] (doudizhu landlord 790, peasants 901), action int8 [T][B][feature_dim],
 *   target float [T][B], done uint8 [T][B], episode_return float [T][B] */
typedef struct {
    void* state;
    void* action;
    void* target;
    void* done;
    void* episode_return;
} cs_dmc_batch;

int cs_dmc_create(cs_handle* h, int32_t T, int32_t slots, cs_dmc** out);
void cs_dmc_destroy(cs_dmc* d);
/* Append the rows of a trajectory of this handle (cs_rollout layout [T_roll][n]; needs obs, player, action, reward,
 * done; player >= num_players marks a row that is not a transition) to the streams, in time order. The chunks that
 * become ready are listed in ready (int64 [cap], DEVICE) as ids, in (env, player, chunk) order; *nready (int64,
 * DEVICE) = their number (entries past cap are not written). Replaces the per-actor act loop for every env at once. */
int cs_dmc_fill(cs_dmc* d, int32_t T_roll, const cs_traj_out* traj, int64_t* ready, int64_t cap, int64_t* nready,
                void* stream);
/* get_batch: `count` chunk ids (DEVICE int64, all of player `player`) stacked along dim 1 into `out`. */
int cs_dmc_gather(cs_dmc* d, int32_t player, const int64_t* chunks, int64_t count, const cs_dmc_batch* out,
                  void* stream);
/* Synchronous, sticky flags: bit 0 = rows were dropped because a stream's ring was full (slots too few, or chunks not
 * gathered) -- those streams are broken (no chunk holding a dropped row is ever listed, later rows of the stream are
 * dropped too); bit 1 = a fill had more ready chunks than `cap` (the rest are listed by the next fill). */
int cs_dmc_status(cs_dmc* d, uint32_t* host_flags);

/* DMCNet scoring of legal actions (model.py:21-43 forward, 91-110 predict), first layer fused: for entry i (state
 * state_of[i], action ids[i]) h1[i] = relu(X[state_of[i]] + b1 + W_act . feature(ids[i])), X = W_obs . obs precomputed
 * per state ([S][H] float), W_act float [feature_dim][H] (the first Linear's action columns, transposed), b1 [H],
 * h1 float [E][H]; H a multiple of 4. Features as cs_action_features. All DEVICE memory. */
int cs_dmc_layer1(cs_handle* h, const float* X, const int32_t* state_of, const int32_t* ids, int64_t E, int32_t H,
                  const float* W_act, const float* b1, float* h1, void* stream);
/* Per state s (legal entries [offsets[s], offsets[s] + counts[s]) of values / ids, cs_legal_lists layout): the id with
 * the largest value (np.argmax: first maximum), or with probability eps a uniform legal id (DMCAgent.step; Philox
 * keyed by seed on (state_base + s, t) in place of np.random). actions int32 [S], -1 where a state has no entry. */
int cs_dmc_select(const float* values, const int32_t* counts, const int64_t* offsets, const int32_t* ids, int64_t S,
                  float eps, uint64_t seed, uint64_t t, uint64_t state_base, int32_t* actions, void* stream);

/* ---- DQN agent (rlcard/agents/dqn_agent.py) ---------------------------------------------------------------------
 * Q-network of the agent as the kernels take it: a plain Linear/tanh stack, x -> tanh(W[0] x + b[0]) -> ... ->
 * W[num_hidden] x + b[num_hidden]. The caller folds the eval-mode BatchNorm1d that precedes the first Linear in
 * EstimatorNetwork into W[0] / b[0] (rlcard_amd.agents.Estimator.folded()). All pointers DEVICE memory, fp32. */
enum { CS_QNET_MAX_HIDDEN = 4, CS_QNET_MAX_WIDTH = 128 };
typedef struct {
    int32_t in_dim;        /* = cs_game_info.obs_dim */
    int32_t num_hidden;    /* 1..4 tanh layers */
    int32_t hidden[4];     /* widths, each 1..128 */
    int32_t num_actions;   /* = cs_game_info.num_actions, <= 64 */
    int32_t reserved;
    const float* W[5];     /* W[k] [out_k][in_k] row-major (torch Linear.weight), W[num_hidden] = output layer */
    const float* b[5];
} cs_qnet;

/* DQNAgent.predict for `rows` observation rows: obs u8 [rows][obs_dim], legal u8 [rows][legal_bytes] or NULL (every
 * action legal) -> q f32 [rows][num_actions], -inf where the action is illegal. The mask is the row's legal_bytes
 * bytes read as one little-endian word (UNO: 8 bytes, 61 bits); bits from num_actions up are ignored. Refusals (both
 * functions): a game with more than 64 actions CS_E_UNSUPPORTED (DouDizhu); in_dim / num_actions not the handle's
 * game's, widths or layer counts out of range, null weights CS_E_INVALID. Every descriptor within those ranges runs on
 * every game of at most 64 actions there is (a block of 64 rows needs 100 352 B of LDS at most, on Mahjong: a game of
 * more than 8 actions or 128 obs bytes keeps its obs rows as bytes); a net that needed more than the 160 KiB a block
 * can have -- only a game with some 1 700 obs bytes could -- would be CS_E_UNSUPPORTED. */
int cs_qnet_values(cs_handle* h, const cs_qnet* net, const void* obs, const void* legal, int64_t rows, float* q,
                   void* stream);
/* DQNAgent.step / eval_step for `rows` rows: actions i32 [rows] = the first maximum of the row's Q-values among its
 * legal actions, or with probability eps a uniform legal action -- cs_dmc_select's draw: Philox keyed by seed on
 * (row_base + row, t), u = (r[0] >> 8) * 2^-24 < eps picks the ((r[1] * count) >> 32)-th legal action -- which has the
 * distribution of DQNAgent.step's eps / len + (1 - eps) on the best action. A row whose done byte is set (done u8
 * [rows], may be NULL) or whose legal mask is empty gets -1, cs_policy_actions' convention (cs_step ignores that
 * action). q (may be NULL) takes cs_qnet_values' rows. */
int cs_qnet_actions(cs_handle* h, const cs_qnet* net, const void* obs, const void* legal, const void* done,
                    int64_t rows, float eps, uint64_t seed, uint64_t t, uint64_t row_base, int32_t* actions, float* q,
                    void* stream);

/* Replay memory of a handle's envs on the device (dqn_agent.py Memory: a FIFO of `capacity` transitions [state,
 * action, reward, next_state, done] plus the next state's legal mask). Each slot holds state and next_state u8
 * [obs_dim], next_legal u8 [legal_bytes], action i32, reward f32, done u8. Games with a legal mask longer than 16
 * bytes (DouDizhu) are CS_E_UNSUPPORTED. */
typedef struct cs_replay cs_replay;
/* cs_replay_gather outputs, DEVICE pointers (any may be NULL): state / next_state f32 [B][obs_dim] (the u8 -> f32
 * conversion is fused), action i64 [B], reward f32 [B], next_legal u8 [B][legal_bytes], done u8 [B] */
typedef struct { void *state, *action, *reward, *next_state, *next_legal, *done; } cs_replay_batch;
int  cs_replay_create(cs_handle* h, int64_t capacity, cs_replay** out);
void cs_replay_destroy(cs_replay* r);
/* reorganize (rlcard/utils/utils.py:153-179) of a trajectory window of this handle (cs_rollout layout [T][n], every
 * tensor including final_obs) for the seats in seat_mask (bit p = seat p). Row (t, e) with acting seat p: state =
 * obs[t][e], next_state = obs[next_t][e] with its legal row, or, where the game ended first, final_obs[end_t][e][p],
 * next_legal = 0, done = 1, reward = the seat's payoff. Rows with player >= num_players are not transitions. A row
 * whose seat neither acts again nor sees its game end inside the window is kept pending (at most one per (env, seat))
 * and completed by a later push -- by that seat's next row or by the game's end there, whatever that push's seat_mask.
 * Order, the FIFO's: a push appends first the pending transitions it completes, in (env, seat) order, then its own
 * completed rows in (t, env) order; positions come from a prefix sum. Of a push that yields more than `capacity`
 * transitions only the last `capacity` are written. */
int  cs_replay_push(cs_replay* r, int32_t T, const cs_traj_out* traj, uint32_t seat_mask, void* stream);
/* Forget the pending rows (after a reset or re-seed of the envs: their games are gone). */
int  cs_replay_drop_pending(cs_replay* r, void* stream);
/* total = transitions ever appended, size = min(total, capacity). HOST out, synchronous. */
int  cs_replay_size(cs_replay* r, int64_t* size, int64_t* total);
/* Memory.sample's stacking: idx i64 [B] (DEVICE), idx[k] in [0, size) = the k-th OLDEST transition held (the
 * reference's list index). An index outside that range is the caller's error (the kernel clamps it). B <= 0: no-op. */
int  cs_replay_gather(cs_replay* r, const int64_t* idx, int64_t B, const cs_replay_batch* out, void* stream);

/* Double-DQN targets (dqn_agent.py:205-218), all DEVICE: q_next / q_next_target f32 [B][num_actions], next_legal u8
 * [B][ceil(num_actions / 8)], reward f32 [B], done u8 [B] -> best i32 [B] = the first maximum of q_next[b] over the
 * legal actions (0 if none is legal: np.argmax of an all -inf row), target f32 [B] = reward[b] + (done[b] ? 0 : gamma)
 * * q_next_target[b][best[b]], the product and the sum each rounded to fp32 (no FMA contraction): the reference's
 * numpy line bit for bit. target or best may be NULL. */
int cs_dqn_targets(const float* q_next, const float* q_next_target, const void* next_legal, const float* reward,
                   const void* done, int64_t B, int32_t num_actions, float gamma, float* target, int32_t* best,
                   void* stream);

/* The DQN learner on the device: K dependent train steps (dqn_agent.py train() and Estimator.update) in one launch of
 * one workgroup, each step sampling its batch from the replay ring, computing the Double-DQN targets, the train-mode
 * forward, the backward and the Adam step, in place on the caller's tensors. All pointers DEVICE memory.
 * The network UNFOLDED (EstimatorNetwork's state_dict): BatchNorm1d over the in_dim inputs, then cs_qnet's stack. */
typedef struct {
    int32_t in_dim;        /* = cs_game_info.obs_dim */
    int32_t num_hidden;    /* 1..4 */
    int32_t hidden[4];     /* widths, each 1..128 */
    int32_t num_actions;   /* = cs_game_info.num_actions, <= 64 */
    int32_t reserved;
    float* bn_weight;      /* [in_dim] BatchNorm1d.weight, .bias, .running_mean, .running_var */
    float* bn_bias;
    float* bn_mean;
    float* bn_var;
    int64_t* bn_tracked;   /* [1] num_batches_tracked */
    float bn_eps, bn_momentum;
    float* W[5];           /* W[k] [out_k][in_k] row-major, W[num_hidden] = output layer */
    float* b[5];
} cs_dqn_net;
/* torch.optim.Adam's state of the Q-network's parameters (exp_avg m, exp_avg_sq v of each tensor) and its
 * hyperparameters; step0 = the steps taken so far (state['step']); the launch's step k is Adam step step0 + k + 1. */
typedef struct {
    float *bn_weight_m, *bn_weight_v, *bn_bias_m, *bn_bias_v;
    float* W_m[5];
    float* W_v[5];
    float* b_m[5];
    float* b_v[5];
    double lr, beta1, beta2, eps;
    int64_t step0;
} cs_dqn_adam;
typedef struct {
    int32_t K;             /* train steps of the launch, 1..4096 */
    int32_t B;             /* batch size, 2..64 */
    float gamma;           /* discount factor */
    int32_t reserved;
    uint64_t seed;         /* key of the sampler */
    uint64_t train_t0;     /* train_t of step 0 (the sampler's counter and the target-copy schedule) */
    int64_t target_every;  /* > 0: after the update of a step with train_t % target_every == 0 the Q-network's
                              state_dict is copied into the target network's; 0: never */
    const int64_t* idx;    /* i64 [K][B] or NULL: the batches' indices (cs_replay_gather's meaning, clamped alike) */
    float* loss;           /* f32 [K] the steps' losses */
    int64_t* idx_out;      /* i64 [K][B] or NULL: the indices used */
    float* target_out;     /* f32 [K][B] or NULL: the targets y */
    float* grads;          /* f32 or NULL: the gradients of the launch's last step, flat, in the order bn_weight, bn_bias,
                              W[0], b[0], W[1], b[1], ... (EstimatorNetwork.parameters()) */
} cs_dqn_train_args;
/* Step k (train_t = train_t0 + k) of the launch, restating train():
 *   indices  idx[k], or B distinct slots drawn uniformly from the size = min(total, capacity) transitions held, by
 *            Floyd's algorithm: for i = 0 .. B-1, j = size - B + i, r = (x * (j + 1)) >> 64 with x = w[0] | w[1] << 32
 *            of Philox keyed by seed on the counter (train_t, i); the i-th index is r, or j where r is already taken.
 *   targets  eval-mode forwards (BatchNorm on its running statistics) of next_state through qnet and target, then
 *            cs_dqn_targets' line.
 *   update   train-mode forward of state (BatchNorm on the batch's mean and biased variance; running_mean / running_var
 *            move by bn_momentum, the latter towards the unbiased variance; num_batches_tracked += 1), loss = mean
 *            (Q[b][action_b] - y_b)^2, backward through the step's old weights, Adam on every parameter: m += (1 -
 *            beta1)(g - m), v = beta2 v + (1 - beta2) g^2, p -= (lr / (1 - beta1^t)) m / (sqrt(v) / sqrt(1 - beta2^t) +
 *            eps), the two bias corrections formed in fp64.
 * Everything is fp32 with fixed summation orders: the result is a function of the arguments alone, bit for bit, and
 * K steps in one launch leave what K launches of one step leave. Nothing is read back: the call returns once the
 * launch is queued, except that the form without idx reads the ring's total once (synchronously) while the ring is not
 * yet known to hold B transitions.
 * Refusals: null or out-of-range descriptors (cs_qnet's ranges; target's dims must be qnet's; in_dim / num_actions the
 * ring's game's), B outside 2..64, K outside 1..4096 CS_E_INVALID; a net whose step needs more than the 160 KiB of
 * LDS a workgroup can have CS_E_UNSUPPORTED (no game of at most 64 actions there is: 816 obs bytes, B = 64 and four
 * layers of 128 fit); fewer than B transitions held, in the form without idx, CS_E_STATE. */
int cs_dqn_train(cs_replay* r, const cs_dqn_net* qnet, const cs_dqn_net* target, const cs_dqn_adam* opt,
                 const cs_dqn_train_args* args, void* stream);

/* ---- NFSP agent (rlcard/agents/nfsp_agent.py) -------------------------------------------------------------------
 * The average-policy network is a cs_qnet descriptor read as Linear/ReLU (AveragePolicyNetwork with its BatchNorm
 * folded: rlcard_amd.agents.AveragePolicyNetwork.folded()). Its head restates NFSPAgent._act and remove_illegal in
 * fp32: p[a] = expf(l[a] - max) / sum over every action, illegal entries zeroed, the legal ones divided by their sum,
 * or 1 / count each where that sum is exactly 0. Refusals are cs_qnet_values'.
 *
 * probs f32 [rows][num_actions] for `rows` observation rows (obs, legal as in cs_qnet_values), 0 where illegal. */
int cs_pnet_probs(cs_handle* h, const cs_qnet* net, const void* obs, const void* legal, int64_t rows, float* probs,
                  void* stream);
/* NFSPAgent.step for `rows` rows, each in its own mode (mode u8 [rows], DEVICE): a row with mode != 0 (best_response)
 * gets exactly cs_qnet_actions' action of that row under (eps, seed, t, row_base) from qnet; a row with mode 0
 * (average_policy) gets an action sampled from pnet's probabilities: with r = Philox keyed by seed on (row_base + row,
 * t) -- the epsilon draw's call -- u = (r[2] >> 8) * 2^-24, the first legal action a in id order with u < c_a, c the
 * running fp32 sum of the row's probabilities (the last legal action if rounding leaves u >= c). Done rows and rows
 * with an empty mask get -1. mode NULL: every row average policy (qnet may be NULL then). probs (may be NULL) f32
 * [rows][num_actions] takes the average-policy rows' probabilities; the other rows are left untouched. The rows are
 * compacted by mode into one index list per network on the device (no host synchronisation) in `scratch`: DEVICE
 * memory of cs_nfsp_scratch_bytes(rows) bytes (a negative CS_E_* code on failure), 256-byte aligned, the caller's
 * (unused when mode is NULL). */
int64_t cs_nfsp_scratch_bytes(int64_t rows);
int cs_nfsp_actions(cs_handle* h, const cs_qnet* qnet, const cs_qnet* pnet, const void* obs, const void* legal,
                    const void* done, const void* mode, int64_t rows, float eps, uint64_t seed, uint64_t t,
                    uint64_t row_base, int32_t* actions, float* probs, void* scratch, void* stream);

/* Reservoir buffer of a handle's envs on the device (nfsp_agent.py ReservoirBuffer of (info_state, action_probs)).
 * Only best-response steps are stored and their action_probs are one-hot, so a slot holds state u8 [obs_dim] and the
 * action id. Games with more than 64 actions (DouDizhu, Gin Rummy, Bridge, Scout) are CS_E_UNSUPPORTED. */
typedef struct cs_reservoir cs_reservoir;
int  cs_reservoir_create(cs_handle* h, int64_t capacity, uint64_t seed, cs_reservoir** out);
void cs_reservoir_destroy(cs_reservoir* r);
/* Offer the rows of a trajectory window (cs_rollout layout [T][n]; obs, player and action are read) to the buffer:
 * the candidates are the rows with player < num_players, that seat in seat_mask and mode[t][e] != 0 (mode u8 [T][n],
 * DEVICE), in (t, env) order. Candidate number pos of the push has stream index k = add_calls + pos and is added as
 * ReservoirBuffer.add adds its k-th element: to slot k while k < capacity; afterwards to slot j = (x * (k + 1)) >> 64,
 * x = r[0] | r[1] << 32 of Philox keyed by seed on (k, 0), if j < capacity, and dropped otherwise. The buffer after the
 * push is the sequential algorithm's (of several candidates on one slot the last one stays). add_calls advances by
 * the number of candidates. */
int  cs_reservoir_push(cs_reservoir* r, int32_t T, const cs_traj_out* traj, const void* mode, uint32_t seat_mask,
                       void* stream);
/* add_calls = candidates ever offered, size = min(add_calls, capacity). HOST out, synchronous. */
int  cs_reservoir_size(cs_reservoir* r, int64_t* size, int64_t* add_calls);
/* idx i64 [B] (DEVICE), slot indices in [0, size) (outside: the caller's error, clamped) -> state f32 [B][obs_dim],
 * probs f32 [B][num_actions] one-hot (either may be NULL). B <= 0: no-op. */
int  cs_reservoir_gather(cs_reservoir* r, const int64_t* idx, int64_t B, float* state, float* probs, void* stream);
/* ReservoirBuffer.clear: empty, add_calls 0. */
int  cs_reservoir_clear(cs_reservoir* r, void* stream);

/* Copy the packed state words of env `env` (state_words u32, HOST buffer) -- the raw fields behind
 * Env.get_state()['raw_obs'] / get_perfect_information for single-env compatibility and debugging. Synchronous.
 * Heads-up Limit and No-limit hold'em (cs_game_info.deal_queue_depth = DQ > 0): words [0, game_words) are the game,
 * then the env's deal queue -- deals the rollout drew ahead from the env's stream, oldest first, that the next games
 * will use -- as one header word H and DQ entries of two words (entry k at words game_words + 1 + 2k, +2 + 2k). With
 * CB = log2(DQ) + 1 and XB = 2 CB - 1 (DQ 8: CB 4, XB 7; DQ 4: CB 3, XB 5):
 *   H bits [0, CB)        number of queued deals (0..DQ)
 *   H bits [CB, 2CB - 1)  slot of the oldest queued deal; queued deal i (i < count) is in slot (head + i) % DQ
 *   H bit XB, XB + 1      No-limit only: the dealer seat has been drawn / the drawn dealer seat
 *   H bits XB + 2 + 2k, XB + 3 + 2k   bits 8..7 of slot k's draw count
 *   e0 (first word of a slot) bits 25..31  bits 6..0 of the slot's draw count: MT19937 words the deal consumed
 *                                          (saturating at 511), so the env's position in its own game stream is the
 *                                          cs_get_rng_ctl position minus the queued deals' draw counts
 * Other bits of the entries are the engine's packed deal (holes, board, blind seat) -- opaque to a consumer. */
int cs_get_env_state(cs_handle* h, int64_t env, uint32_t* host_words, int32_t nwords);

/* Asynchronous cs_get_env_state: the state words of env `env` copied on `stream` into dst (u32 [state_words],
 * DEVICE memory), so a single-env host can bring them back with its step outputs in one transfer (rlcard_amd.make's
 * Env: one packed device-to-host copy per Env.step, envs/env.py:65-86). */
int cs_copy_env_state(cs_handle* h, int64_t env, uint32_t* dst, void* stream);

/* Single-env completion without a stream synchronisation (rlcard_amd.make's Env: one launch and a spin per Env.step):
 * when seq is not NULL, every later cs_reset / cs_step / cs_observe also writes env `env`'s packed state words to
 * `words` (state_words u32, 16-byte aligned) and then -- after a system-scope fence ordering all of that env's output
 * stores -- the call's sequence number to *seq: 1 for the first call after cs_set_step_record, then 2, 3, ... Both
 * are device-visible pointers, typically mapped pinned host memory the host polls. seq NULL turns it off. Only that
 * env's outputs are covered; meant for single-env handles. */
int cs_set_step_record(cs_handle* h, int64_t env, uint32_t* words, uint32_t* seq);

/* Overwrite the packed state words of env `env` from a HOST buffer taken by cs_get_env_state: Env.step_back
 * (envs/env.py:88-108) restores the game from its history. The env's RNG stream is left where it is, as the
 * reference's history does not hold np_random for most games (Blackjack's does: cs_load_env_rng). Synchronous. */
int cs_set_env_state(cs_handle* h, int64_t env, const uint32_t* host_words, int32_t nwords);

/* An env's whole RNG stream (numpy RandomState: position word + MT19937 block words / byte ring) as *words u32, for
 * the state a deep copy of the reference's RandomState holds. cs_copy_env_rng copies env `env`'s stream into dst,
 * cs_load_env_rng writes it back from src (both DEVICE memory, asynchronous on `stream`). Blackjack's Game.step
 * deep-copies the dealer -- its np_random included -- before every step and Game.step_back restores that copy
 * (rlcard/games/blackjack/game.py:66-70, 125-135), so the reference's redraws after a step back replay the undone
 * cards: rlcard_amd.make's Blackjack Env snapshots the stream with its history and loads it on step_back. */
int cs_env_rng_words(cs_handle* h, int32_t* words);
int cs_copy_env_rng(cs_handle* h, int64_t env, uint32_t* dst, void* stream);
int cs_load_env_rng(cs_handle* h, int64_t env, const uint32_t* src, void* stream);

/* Stream position (u32 draws consumed) bookkeeping word of env `env` (HOST out). Synchronous; for parity tests.
 * The position is ctl & 0x3FFF (DouDizhu: ctl & 0x7FF), the draws consumed modulo cs_game_info.rng_period; the other
 * bits are the engine's. Hold'em envs with a deal queue: the position includes the draws of the queued deals (their
 * counts are decoded as cs_get_env_state documents; tools/abi_driver.c). */
int cs_get_rng_ctl(cs_handle* h, int64_t env, uint32_t* host_ctl);

/* Evaluator test hook: the value the hold'em kernels' showdown evaluator gives `n` 7-card hands (Hand.evaluateHand +
 * the tie-break of compare_hands, limitholdem/utils.py:3-614): cards int8 [n][7] card2index ids (suit * 13 + rank,
 * S H D C x A 2 .. K; DEVICE), values uint32 [n] (DEVICE): category << 20 | five 4-bit tie-break ranks -- larger
 * wins, equal splits. No handle: the evaluator is stateless. */
int cs_debug_holdem_rank7(const int8_t* cards, int64_t n, uint32_t* values, void* stream);

/* Mahjong win-judge test hook: the judge_hu of the Mahjong kernels (rlcard/games/mahjong/judger.py judge_hu / cal_set)
 * on `n` ordered hands: hands u8 [n][14] (tile = action id 0..33, in hand order -- the order decides which pairs the
 * judge tries), len u8 [n] (tiles used of each row, <= 14), piles u8 [n] (the player's pile count) -> win u8 [n]
 * (0 / 1). All DEVICE memory; stateless (no handle). */
int cs_debug_mahjong_hu(const uint8_t* hands, const uint8_t* len, const uint8_t* piles, int64_t n, uint8_t* win,
                        void* stream);

/* Gin Rummy meld-judge test hook: the judge of the Gin Rummy kernels (rlcard_amd/csrc/cs_gin_melds.h; the reference's
 * utils/melding.py, judge._get_going_out_cards, round.gin) on `n` ordered hands: hands u8 [n][11] (card id = rank +
 * 13 * suit, in hand order), len u8 [n] (cards used of each row, <= 11) -> deadwood i32 [n] (the best deadwood count of
 * the row's cards), and for rows of 11 cards knock u64 [n] and gin u64 [n] (the knock and gin sets as card masks) and
 * gin_card i32 [n] (gin_cards[0], -1 with an empty gin set); rows of another length get 0, 0, -1. All DEVICE memory;
 * stateless (no handle). */
int cs_debug_gin_melds(const uint8_t* hands, const uint8_t* len, int64_t n, int32_t* deadwood, uint64_t* knock,
                       uint64_t* gin, int32_t* gin_card, void* stream);

/* DouDizhu legal-set test hook: the legal-action bitmask the step / rollout kernels build, for `n` (hand, previous
 * play) cases: counts u8 [n][15] (cards per rank 3 .. A, 2, black joker, red joker), prev i32 [n] (the largest play
 * on the table, made by another player; < 0 = leading) -> legal u8 [n][3434] (bit = id, pass included when
 * following). All DEVICE memory. Replaces Judger.playable_cards_from_hand (doudizhu/judger.py:124-258) /
 * get_gt_cards (doudizhu/utils.py:225-262). Needs a doudizhu handle (its action table). */
int cs_debug_ddz_legal(cs_handle* h, const uint8_t* counts, const int32_t* prev, int64_t n, uint8_t* legal,
                       void* stream);

/* Testing hook: when enabled, the wave-cooperative MT refill is skipped, so every block crossing takes the in-lane
 * serial twist; results must be identical. */
int cs_debug_set_serial_refill(cs_handle* h, int32_t enable);

/* Tuning hook: kernel variant bits (bit 0 = serial MT refill; DouDizhu rollouts: every legal set through the group
 * pass, no following fast path; bit 1 = DouDizhu rollouts: the whole legal image zeroed at every step; bit 2 = dword
 * instead of 16-B obs stores). Results are identical for every value. */
int cs_debug_set_kernel_flags(cs_handle* h, int32_t flags);

const char* cs_last_error(void);
const char* cs_version(void);
int32_t cs_abi_version(void);   /* CS_ABI_VERSION of the library */

#ifdef __cplusplus
}
#endif
#endif
