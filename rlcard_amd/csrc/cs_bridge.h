// cs_bridge.h -- Bridge (4 players, the reference's default payoff delegate and state extractor) as a lane-per-env
// lockstep state machine.
//
// Behaviour (reference file):
//   rlcard/games/bridge/utils/action_event.py   the 91 action ids (cs_bridge_rules.h)
//   rlcard/games/bridge/utils/bridge_card.py    card id = 13 * suit + rank, suits C D H S, ranks 2..A
//   rlcard/games/bridge/utils/tray.py           board b: dealer (b - 1) % 4, vul none / N-S / E-W / all for b = 1..4
//   rlcard/games/bridge/game.py     init_game: np_random.choice([1, 2, 3, 4]) is the board, then BridgeRound
//   rlcard/games/bridge/dealer.py   the 52 cards in id order, np_random.shuffle, 13 stock_pile.pop()s per player: player
//                                   p's hand, in list order, is deck[51 - 13 p - i], i = 0..12
//   rlcard/games/bridge/round.py    make_call (a bid sets the cube back to 1), is_bidding_over (at least four calls, the
//                                   last three passes), is_over (passed out, or every hand empty), get_declarer (the first
//                                   player of the contract side to have bid the contract's strain), the left defender
//                                   leads, play_card (cs_bridge_rules.h trick_winner), get_trick_moves (after the fourth
//                                   card the whole trick until the next card is played). Four opening passes end the game
//                                   and leave the last passer as the current player.
//   rlcard/games/bridge/judger.py   get_legal_actions (cs_bridge_rules.h)
//   rlcard/envs/bridge.py           DefaultBridgeStateExtractor: 573 values, always the CURRENT player's whoever asks:
//                                   hands [4][52] (the player's own; once bidding is over also the dummy's, or the
//                                   declarer's if the player is the dummy), trick pile [4][52] by seat, hidden cards [52],
//                                   vul [4], dealer [4], current player [4], is_bidding_rep [1] (1 when bidding is OVER),
//                                   bidding_rep [40] (the action ids of the first 40 - dealer calls from index dealer on:
//                                   raw values, not 0/1), last_bid_rep [39] (by the last move's id; zero after the deal
//                                   and after a played card), bid_amount_rep [8] and trump_suit_rep [5] (only between the
//                                   end of the auction and the opening lead). Once the game is over the hands, trick,
//                                   hidden and contract fields are zero, the rest stay.
//                                   DefaultBridgePayoffDelegate (cs_bridge_rules.h payoffs)
// Hand order is observable on the raw side (raw_legal_actions lists the cards in hand order), so the state keeps the
// 52 shuffled bytes; a hand is the cards of its deal still in its mask. The auction can run to 319 calls (three passes,
// then 35 times bid P P X P P XX P P), a game to 371 steps; the state keeps the first 40 calls (all bidding_rep can
// show), the first bidder per side and strain (the declarer), and counters.
// Packed state, 35 u32 words per env (word-major [35][N]) = the lane's LDS scratch, byte b in byte b % 4 of word b / 4:
//   words  0..12   the shuffled deck, one card id per byte
//   words 13..20   the four hands as card masks: seat p in words 13 + 2 p (cards 0..31) and 14 + 2 p (cards 32..51)
//   words 21..30   the first 40 calls, one action id (1..38) per byte, zero past the last
//   word  31       the first bidder per side s and strain k, two bits at 2 (5 s + k): bit 0 some bid, bit 1 seat >> 1
//   word  32       current player | dealer << 2 | number of calls << 4 (9 bits) | last bid id << 13 (6 bits, 0 none) |
//                  last bidder << 19 | cube code << 21 (0, 1 dbl, 2 rdbl) | trailing passes << 23 (at most 3) | the last
//                  move's call id << 25 (6 bits; 0 after the deal and after a played card) | over << 31
//   word  33       cards played (6 bits) | tricks of side 0 << 6 | of side 1 << 10 (4 bits each) | declarer << 14 |
//                  leader of the trick shown << 16
//   word  34       the trick shown, one card per byte in play order
// The k-th call is seat (dealer + k) % 4's, so no call needs its player stored.
// Defined by this ABI where the reference raises: an illegal action id plays the lowest legal id. Words written through
// cs_set_env_state that hold no game (load) are a finished game.
#pragma once
#include "cs_device.h"
#include "cs_bridge_rules.h"
#include "../../include/cardsim.h"

namespace cs {

struct Bridge : GameDefaults {
    static constexpr int OBS = 573, A = 91, P = 4, LB = 12, WORDS = 35, ACTION_BYTES = 1;
    static constexpr int NBITS = 18;            // obs bitmap words (573 bits)
    static constexpr int RAW_SPAN_AT = 481, RAW_SPAN_LEN = 40;   // bidding_rep: raw bytes among the 0/1 bytes
    static constexpr int NB = NBITS + RAW_SPAN_LEN / 4;           // observe(): the bitmap, then the span's bytes
    static constexpr bool RAW_OBS = false;
    static constexpr int SCRATCH_WORDS = WORDS;   // the whole state lives in the lane's LDS scratch
    static constexpr int STAGE_W = 64, STAGE_PAD = 4, STAGE_R = 16, STAGE_RF = 32;
    static constexpr int RESTAGE_B = 4;
    static constexpr bool OBS_DIRECT = true;   // 573 B: per-lane stores from the row's own byte and 16-byte phase
    // LDS per block: state 35 x 1 KB = 35 840 B + stage rows 4 x (64 x 68 + 16) = 17 472 B = 53 312 B (+ 20 B): three
    // blocks per CU (160 KB = 163 840 B >= 3 x 53 760 with the allocation rounded up), three waves per SIMD. The
    // registers bind first: the row writer's rollout takes 187 VGPRs (9 SGPRs spilled to lanes), two waves per SIMD;
    // held to 168 for three it spills VGPRs to scratch and measured slower (4.5 against 4.2 ms, profiles/EXPERIMENTS.md
    // B-1), so the budget asked for is two
    static constexpr int MIN_WAVES = CS_PROF_BRIDGE_WAVES > 0 ? CS_PROF_BRIDGE_WAVES : 2;   // (cs_prof.h: an A/B knob)
    static constexpr int EPW = 64;
    static constexpr int MAX_POLICY = CS_POLICY_RULE_V1;
    static constexpr int NCARDS = 52, W_HAND = 13, W_CALLS = 21, W_FIRST = 31, W_META = 32, W_PLAY = 33, W_TRICK = 34;
    static constexpr int CALLS_KEPT = 40, MAX_CALLS = 319;

    uint32_t* s;   // lane scratch: state word i at s[i * WAVE]

    __device__ __forceinline__ uint32_t& L(int i) const { return s[i * WAVE]; }
    static_assert(WAVE * 4 == 256, "state byte address");
    __device__ __forceinline__ uint8_t& B(int b) const { return ((uint8_t*)s)[b + 252 * (b >> 2)]; }

    __device__ __forceinline__ uint32_t meta() const { return L(W_META); }
    __device__ __forceinline__ uint32_t play() const { return L(W_PLAY); }
    __device__ __forceinline__ int current() const { return meta() & 3; }
    __device__ __forceinline__ int dealer() const { return (meta() >> 2) & 3; }
    __device__ __forceinline__ int ncalls() const { return (meta() >> 4) & 511; }
    __device__ __forceinline__ int last_bid() const { return (meta() >> 13) & 63; }
    __device__ __forceinline__ int last_bidder() const { return (meta() >> 19) & 3; }
    __device__ __forceinline__ int cube() const { return (meta() >> 21) & 3; }
    __device__ __forceinline__ int passes() const { return (meta() >> 23) & 3; }
    __device__ __forceinline__ int last_call() const { return (meta() >> 25) & 63; }
    __device__ __forceinline__ bool is_over() const { return meta() >> 31; }
    __device__ __forceinline__ int ncards() const { return play() & 63; }
    __device__ __forceinline__ int won(int side) const { return (play() >> (6 + 4 * side)) & 15; }
    __device__ __forceinline__ int declarer() const { return (play() >> 14) & 3; }
    __device__ __forceinline__ int leader() const { return (play() >> 16) & 3; }
    __device__ __forceinline__ bool bidding_over() const { return ncalls() >= 4 && passes() >= 3; }
    __device__ __forceinline__ void set_meta(int shift, uint32_t mask, int v) const
    {
        L(W_META) = (meta() & ~(mask << shift)) | ((uint32_t)v & mask) << shift;
    }
    __device__ __forceinline__ void set_play(int shift, uint32_t mask, int v) const
    {
        L(W_PLAY) = (play() & ~(mask << shift)) | ((uint32_t)v & mask) << shift;
    }
    __device__ __forceinline__ uint64_t hand(int p) const
    {
        return (uint64_t)L(W_HAND + 2 * p) | (uint64_t)L(W_HAND + 2 * p + 1) << 32;
    }
    __device__ __forceinline__ void set_hand(int p, uint64_t h) const
    {
        L(W_HAND + 2 * p) = (uint32_t)h;
        L(W_HAND + 2 * p + 1) = (uint32_t)(h >> 32);
    }
    // cards of the trick shown: none before the opening lead, all four after a trick's last card
    __device__ __forceinline__ int trick_shown() const
    {
        const int n = ncards(), k = n & 3;
        return n == 0 ? 0 : (k == 0 ? 4 : k);
    }
    __device__ __forceinline__ int trick_card(int i) const { return (L(W_TRICK) >> (8 * (i & 3))) & 255; }

    __device__ __forceinline__ void bind(uint32_t* lane_scratch, const GameParams&) { s = lane_scratch; }
    __device__ __forceinline__ void blank()
    {
#pragma unroll 1
        for (int w = 0; w < WORDS; w++) L(w) = 0u;
        L(W_META) = 1u << 31;
    }
    // the 13 cards dealt to seat p; bit 63: a byte that is no card, or one met twice in `seen`
    __device__ __forceinline__ uint64_t dealt(int p, uint64_t& seen) const
    {
        uint64_t m = 0;
#pragma unroll 1
        for (int i = 0; i < 13; i++) {
            const int c = B(NCARDS - 1 - 13 * p - i);
            const uint64_t bit = 1ull << (c & 63);
            if (c >= NCARDS || (seen & bit)) m |= 1ull << 63;
            else m |= bit;
            seen |= bit;
        }
        return m;
    }
    __device__ __forceinline__ void load(const uint32_t* st, int64_t n, int64_t env)
    {
#pragma unroll 1
        for (int w = 0; w < WORDS; w++) L(w) = st[(int64_t)w * n + env];
        // words written by cs_set_env_state are the caller's: the deck holds each of the 52 cards once, every hand is
        // what is left of its deal, the counters agree with the hands, the trick's cards have been played, the stored
        // calls are calls; anything else is a finished game. Of a finished game observe() still shows the dealer, the
        // current player, the last call and the stored calls, so those are checked for it too (else: the blank one).
        const int nc = ncalls(), n_played = ncards(), k = n_played & 3, shown = trick_shown();
        if (is_over()) {
            bool fine = nc <= MAX_CALLS && last_call() <= bridge::RDBL;
#pragma unroll 1
            for (int i = 0; i < CALLS_KEPT; i++) {
                const int c = B(4 * W_CALLS + i);
                fine = fine && (i < nc ? (c >= bridge::FIRST_BID && c <= bridge::RDBL) : c == 0);
            }
            if (!fine) blank();
            return;
        }
        bool ok = nc <= MAX_CALLS && last_bid() <= bridge::LAST_BID && cube() <= bridge::CUBE_RDBL &&
                  last_call() <= bridge::RDBL && n_played < NCARDS && !(play() >> 18) &&
                  won(0) + won(1) == (n_played >> 2) && !(L(W_FIRST) >> 20);
        const bool bo = bidding_over();
        ok = ok && (bo ? last_bid() > 0 : n_played == 0);          // (a passed-out or played-out game is over)
        ok = ok && ((nc > 0 && n_played == 0) == (last_call() > 0));
        uint64_t seen = 0, left = 0;
        if (ok) {
            const int lead = leader();
#pragma unroll 1
            for (int p = 0; p < P; p++) {
                const uint64_t d = dealt(p, seen), h = hand(p);
                const int in_trick = ((p - lead) & 3) < k ? 1 : 0;   // seats that have played to the trick under way
                ok = ok && !(d >> 63) && !(h & ~d) && __popcll(h) == 13 - (n_played >> 2) - in_trick;
                left |= h;
            }
            const uint64_t played = bridge::CARDS52 & ~left;
#pragma unroll 1
            for (int i = 0; i < shown; i++) {
                const int c = trick_card(i);
                ok = ok && c < NCARDS && ((played >> (c & 63)) & 1ull);
            }
#pragma unroll 1
            for (int i = 0; i < CALLS_KEPT; i++) {
                const int c = B(4 * W_CALLS + i);
                ok = ok && (i < nc ? (c >= bridge::FIRST_BID && c <= bridge::RDBL) : c == 0);
            }
        }
        if (!ok) blank();
    }
    __device__ __forceinline__ void store(uint32_t* st, int64_t n, int64_t env) const
    {
#pragma unroll 1
        for (int w = 0; w < WORDS; w++) st[(int64_t)w * n + env] = L(w);
    }

    // ---- Game.init_game ---------------------------------------------------------------------------------------------
    template <class Rng>
    __device__ __forceinline__ void reset(Rng& rng)
    {
        const int dl = (int)rng.interval(3u);   // np_random.choice([1, 2, 3, 4]) - 1: the dealer
#pragma unroll 1
        for (int w = 0; w < NCARDS / 4; w++) {   // BridgeCard.get_deck(): card id i at index i
            const uint32_t b = 4u * (uint32_t)w;
            L(w) = b | (b + 1u) << 8 | (b + 2u) << 16 | (b + 3u) << 24;
        }
#pragma unroll 1
        for (int w = NCARDS / 4; w < WORDS; w++) L(w) = 0u;
        // np_random.shuffle: Fisher-Yates i = 51 .. 1, j = random_interval(i), swap
        rng.draw_intervals((uint32_t)NCARDS - 1u, [&](uint32_t k, uint32_t j) {
            const uint32_t i = (uint32_t)NCARDS - 1u - k;
            uint8_t& pi = B((int)i);
            uint8_t& pj = B((int)j);
            const uint8_t ci = pi, cj = pj;
            pi = cj;
            pj = ci;
        });
#pragma unroll 1
        for (int p = 0; p < P; p++) {
            uint64_t seen = 0;
            set_hand(p, dealt(p, seen) & bridge::CARDS52);
        }
        L(W_META) = (uint32_t)dl | (uint32_t)dl << 2;
    }

    // ---- Judger.get_legal_actions as an id mask ---------------------------------------------------------------------
    __device__ __forceinline__ Legal128 legal() const
    {
        Legal128 m{0ull, 0ull};
        if (is_over()) return m;
        if (!bidding_over()) {
            m.lo = bridge::legal_calls(last_bid(), last_bidder(), cube(), current());
        } else {
            const int k = ncards() & 3;
            const uint64_t c = bridge::legal_cards(hand(current()), k > 0 ? trick_card(0) : -1);
            m.lo = c << bridge::PLAY;
            m.hi = c >> (64 - bridge::PLAY);
        }
        return m;
    }

    // ---- envs/bridge.py DefaultBridgeStateExtractor.extract_state: the current player's, whoever asks ----------------
    template <int POS>
    __device__ static __forceinline__ void put(uint32_t (&bits)[NB], uint64_t v)
    {
        constexpr int W = POS / 32, S = POS % 32;
        bits[W] |= (uint32_t)(v << S);
        if constexpr (W + 1 < NBITS) bits[W + 1] |= (uint32_t)(S ? v >> (32 - S) : v >> 32);
        if constexpr (S != 0 && W + 2 < NBITS) bits[W + 2] |= (uint32_t)(v >> (64 - S));
    }
    __device__ __forceinline__ void observe(int, uint32_t (&bits)[NB]) const
    {
#pragma unroll
        for (int w = 0; w < NB; w++) bits[w] = 0u;
        const int cur = current(), dl = dealer();
        const bool over = is_over(), bo = bidding_over();
        if (!over) {
            const int dc = declarer(), shown = trick_shown(), lead = leader();
            // the other hand the player sees: the dummy's, or the declarer's from the dummy's seat
            const int dummy = (dc + 2) & 3, other = dummy != cur ? dummy : dc;
            uint64_t hidden;
            if (bo) {
                if (((cur ^ dc) & 1) == 0) hidden = hand((cur + 1) & 3) | hand((cur + 3) & 3);
                else hidden = hand(dc) | hand((cur + 2) & 3);
            } else {
                hidden = hand((cur + 1) & 3) | hand((cur + 2) & 3) | hand((cur + 3) & 3);
            }
            uint64_t hv[P], tv[P];
#pragma unroll
            for (int p = 0; p < P; p++) {
                hv[p] = (p == cur || (bo && p == other)) ? hand(p) : 0ull;
                const int i = (p - lead) & 3;   // seat p's place in the trick shown
                tv[p] = i < shown ? 1ull << (trick_card(i) & 63) : 0ull;
            }
            put<0>(bits, hv[0]);
            put<52>(bits, hv[1]);
            put<104>(bits, hv[2]);
            put<156>(bits, hv[3]);
            put<208>(bits, tv[0]);
            put<260>(bits, tv[1]);
            put<312>(bits, tv[2]);
            put<364>(bits, tv[3]);
            put<416>(bits, hidden);
            if (bo && ncards() == 0) {   // the contract shows until the opening lead
                const int lb = last_bid() > 0 ? last_bid() : 1;
                put<560>(bits, 1ull << bridge::bid_amount(lb));
                put<568>(bits, 1ull << bridge::bid_strain(lb));
            }
        }
        const uint32_t vul = dl == 0 ? 0u : (dl == 1 ? 5u : (dl == 2 ? 10u : 15u));   // Tray.vul of board dl + 1
        put<468>(bits, (uint64_t)(vul | 16u << dl | 256u << cur | (bo ? 4096u : 0u)));
        const int lc = last_call();
        if (lc > 0) put<521>(bits, 1ull << lc);
        // bidding_rep: the first 40 - dealer calls from byte `dealer` of the span on
        uint32_t prev = 0u;
#pragma unroll
        for (int j = 0; j < RAW_SPAN_LEN / 4; j++) {
            const uint32_t w = L(W_CALLS + j);
            bits[NBITS + j] = (uint32_t)(((uint64_t)w << 32 | prev) >> (32 - 8 * dl));
            prev = w;
        }
    }

    template <class Rng>
    __device__ __forceinline__ void step(int a, Rng&)
    {
        const Legal128 lg = legal();
        if (legal_empty(lg)) return;
        if (a < 0 || a >= A || !legal_has(lg, a)) a = legal_lowest(lg);   // this ABI's fallback: lowest legal id
        const int cur = current();
        if (a < bridge::PLAY) {   // round.make_call
            const int nc = ncalls();
            if (nc < CALLS_KEPT) B(4 * W_CALLS + nc) = (uint8_t)a;
            set_meta(4, 511u, nc < 511 ? nc + 1 : nc);
            if (a == bridge::PASS) {
                const int ps = passes();
                set_meta(23, 3u, ps < 3 ? ps + 1 : ps);
            } else {
                set_meta(23, 3u, 0);
                if (a == bridge::DBL) {
                    set_meta(21, 3u, bridge::CUBE_DBL);
                } else if (a == bridge::RDBL) {
                    set_meta(21, 3u, bridge::CUBE_RDBL);
                } else {
                    set_meta(21, 3u, bridge::CUBE_1);
                    set_meta(13, 63u, a);
                    set_meta(19, 3u, cur);
                    const int slot = 2 * (5 * (cur & 1) + bridge::bid_strain(a));
                    if (!((L(W_FIRST) >> slot) & 1u)) L(W_FIRST) |= (1u | (uint32_t)(cur >> 1) << 1) << slot;
                }
            }
            set_meta(25, 63u, a);
            if (bidding_over()) {
                const int lb = last_bid();
                if (lb == 0) {
                    L(W_META) |= 1u << 31;   // passed out: the last passer stays the current player
                } else {
                    const int side = last_bidder() & 1;
                    const uint32_t e = L(W_FIRST) >> (2 * (5 * side + bridge::bid_strain(lb)));
                    const int dc = (e & 1u) ? side + 2 * (int)((e >> 1) & 1u) : last_bidder();
                    set_play(14, 3u, dc);
                    set_meta(0, 3u, (dc + 1) & 3);   // the left defender leads
                }
            } else {
                set_meta(0, 3u, (cur + 1) & 3);
            }
        } else {   // round.play_card
            const int c = a - bridge::PLAY, n = ncards(), k = n & 3;
            set_hand(cur, hand(cur) & ~(1ull << c));
            if (k == 0) {
                set_play(16, 3u, cur);
                L(W_TRICK) = 0u;
            }
            L(W_TRICK) |= (uint32_t)c << (8 * k);
            set_play(0, 63u, n + 1);
            set_meta(25, 63u, 0);
            if (k == 3) {
                const uint32_t t = L(W_TRICK);
                const int w = bridge::trick_winner(t & 255, (t >> 8) & 255, (t >> 16) & 255, t >> 24,
                                                   bridge::bid_strain(last_bid() > 0 ? last_bid() : 1));
                const int seat = (leader() + w) & 3;
                const int side = seat & 1, tw = won(side);
                set_play(6 + 4 * side, 15u, tw < 13 ? tw + 1 : tw);
                set_meta(0, 3u, seat);
            } else {
                set_meta(0, 3u, (cur + 1) & 3);
            }
            if (n + 1 >= NCARDS) L(W_META) |= 1u << 31;
        }
    }

    __device__ __forceinline__ void payoffs(float (&r)[P]) const
    {
        int v[P];
        bridge::payoffs(last_bid(), last_bidder(), won(0), won(1), v);
#pragma unroll
        for (int p = 0; p < P; p++) r[p] = (float)v[p];
    }

    // ---- BridgeDefenderNoviceRuleAgent (models/bridge_rule_models.py): pass whenever it is legal, otherwise a uniform
    // pick among the legal ids from the step's policy word, by the random policy's formula
    __device__ __forceinline__ int rule_action(uint32_t, int, const Legal128& lg, uint32_t r) const
    {
        if ((lg.lo >> bridge::PASS) & 1ull) return bridge::PASS;
        return pick_legal128(lg, r);
    }
};

}  // namespace cs
