// cs_gin_rummy.h -- Gin Rummy (2 players, the reference's default Settings) as a lane-per-env lockstep state machine.
//
// Behaviour (reference file):
//   rlcard/games/gin_rummy/utils/action_event.py   the 110 action ids: score north 0, score south 1, draw 2, pick up
//                                   the discard 3, declare dead hand 4, gin 5, discard card c = 6 + c, knock card c =
//                                   58 + c (card id = rank + 13 * suit, utils.py:36-39)
//   rlcard/games/gin_rummy/game.py  init_game: np_random.choice([0, 1]) is the dealer, then GinRummyRound (dealer.py: the
//                                   52 cards in id order, np_random.shuffle, stock_pile.pop() per card), 11 cards to the
//                                   non-dealer, 10 to the dealer; the non-dealer moves first
//   rlcard/games/gin_rummy/round.py draw_card, pick_up_discard (the card joins known_cards), declare_dead_hand, discard,
//                                   knock, gin (cs_gin_melds.h gin_card), score_player_0 / 1; every move lengthens
//                                   move_sheet, which starts with the deal move
//   rlcard/games/gin_rummy/judge.py get_legal_actions by the last action (cs_gin_melds.h going_out)
//   rlcard/games/gin_rummy/utils/scorers.py   get_payoff_gin_rummy_v1: 0.2 to the knocker, 1 to the ginner, otherwise
//                                   -best deadwood / 100
//   rlcard/envs/gin_rummy.py        obs [5][52] 0/1 of the CURRENT player whoever asks: hand, top discard, the other
//                                   discards, the opponent's known cards, stock + the opponent's cards not known; all
//                                   zero once the game is over
//   rlcard/models/gin_rummy_rule_models.py   gin-rummy-novice-rule = CS_POLICY_RULE_V1 (rule_action below)
// Order is observable on the raw side (the piles, the hands and known_cards are lists) and in the gin card, so the
// state keeps ordered lists, one byte per card.
// Packed state, 29 u32 words per env (word-major [29][N]) = the lane's LDS scratch, byte b in byte b % 4 of word b / 4:
//   bytes   0..51   the stock pile up from byte 0 (stock[i] at byte i, pop() takes byte ns - 1) and the discard pile down
//                   from byte 51 (discard_pile[i] at byte 51 - i); ns + nd <= 52
//   bytes  52..75   the hands, 12 bytes per player: hand[i] at 52 + 12 p + i (i < 11)
//   bytes  76..99   known_cards, 12 bytes per player: known_cards[i] at 76 + 12 p + i (i < 11)
//   word 25         ns | nd << 6 | len(hand 0) << 12 | len(hand 1) << 16 | len(known 0) << 20 | len(known 1) << 24
//   word 26         current_player | dealer << 1 | last action kind << 2 (0 none, 1 draw, 2 pick up, 3 discard, 4 dead
//                   hand, 5 gin, 6 knock, 7 score north, 8 score south) | picked-up card << 6 | len(move_sheet) << 12 |
//                   going-out kind << 20 (0 none, 1 dead hand, 2 knock, 3 gin) | going-out player << 22 | over << 23 |
//                   the card that left the game << 24 | one has << 30 (round.knock and round.gin take the card out of
//                   the hand and put it nowhere)
//   words 27, 28    what the judge said of the current player's 11 cards: the knock set as a 52-bit card mask, bit 63 =
//                   the gin set is not empty. Written by the step that makes the hand 11 cards (the deal, a draw, a pick
//                   up) and cleared by every other: legal() reads it, no step judges twice.
// The two piles, the two hands and the card that left always hold the 52 cards between them, so no list can outgrow its
// region.
// Defined by this ABI where the reference raises: an illegal action id plays the lowest legal id.
#pragma once
#include "cs_device.h"
#include "cs_gin_melds.h"
#include "../../include/cardsim.h"

namespace cs {

struct GinRummy : GameDefaults {
    static constexpr int OBS = 260, A = 110, P = 2, LB = 14, WORDS = 29, ACTION_BYTES = 1;
    static constexpr int NB = 9;               // obs bitmap words (260 bits)
    static constexpr bool RAW_OBS = false;
    static constexpr int SCRATCH_WORDS = WORDS;   // the whole state lives in the lane's LDS scratch
    static constexpr int STAGE_W = 64, STAGE_PAD = 4, STAGE_R = 16, STAGE_RF = 32;
    static constexpr int RESTAGE_B = 4;
    static constexpr bool OBS_DIRECT = true;   // 260 = 16 x 16 + 4: per-lane 16-byte stores and a dword head / tail
    // LDS per block: state 29 KB + stage rows 17 KB = 46 KB: three blocks per CU (160 KB), three waves per SIMD
    static constexpr int MIN_WAVES = 3;
    static constexpr int EPW = 64;
    static constexpr int MAX_POLICY = CS_POLICY_RULE_V1;
    static constexpr int NCARDS = 52, HANDS = 52, KNOWN = 76, W_CNT = 25, W_META = 26, W_KNOCK = 27;
    static constexpr int SCORE_N = 0, SCORE_S = 1, DRAW = 2, PICK = 3, DEAD = 4, GIN = 5, DISCARD = 6, KNOCK = 58;
    static constexpr int L_NONE = 0, L_DRAW = 1, L_PICK = 2, L_DISCARD = 3, L_DEAD = 4, L_GIN = 5, L_KNOCK = 6,
                         L_SCORE_N = 7, L_SCORE_S = 8;
    static constexpr int GO_DEAD = 1, GO_KNOCK = 2, GO_GIN = 3;
    static constexpr int MAX_MOVES = 200, DEAD_STOCK = 2;   // Settings: max_move_count, stockpile_dead_card_count

    uint32_t* s;   // lane scratch: state word i at s[i * WAVE]

    __device__ __forceinline__ uint32_t& L(int i) const { return s[i * WAVE]; }
    static_assert(WAVE * 4 == 256, "state byte address");
    __device__ __forceinline__ uint8_t& B(int b) const { return ((uint8_t*)s)[b + 252 * (b >> 2)]; }

    __device__ __forceinline__ int ns() const { return L(W_CNT) & 63; }
    __device__ __forceinline__ int nd() const { return (L(W_CNT) >> 6) & 63; }
    __device__ __forceinline__ int nh(int p) const { return (L(W_CNT) >> (12 + 4 * p)) & 15; }
    __device__ __forceinline__ int nk(int p) const { return (L(W_CNT) >> (20 + 4 * p)) & 15; }
    __device__ __forceinline__ void add_cnt(int shift, int d) const { L(W_CNT) += (uint32_t)d << shift; }
    __device__ __forceinline__ uint32_t meta() const { return L(W_META); }
    __device__ __forceinline__ int current() const { return meta() & 1; }
    __device__ __forceinline__ int last() const { return (meta() >> 2) & 15; }
    __device__ __forceinline__ int picked() const { return (meta() >> 6) & 63; }
    __device__ __forceinline__ int moves() const { return (meta() >> 12) & 255; }
    __device__ __forceinline__ int go_kind() const { return (meta() >> 20) & 3; }
    __device__ __forceinline__ int go_player() const { return (meta() >> 22) & 1; }
    __device__ __forceinline__ bool is_over() const { return (meta() >> 23) & 1; }
    __device__ __forceinline__ uint64_t gone_mask() const { return (uint64_t)((meta() >> 30) & 1u) << ((meta() >> 24) & 63u); }
    __device__ __forceinline__ void set_field(int shift, uint32_t mask, int v) const
    {
        L(W_META) = (meta() & ~(mask << shift)) | ((uint32_t)v & mask) << shift;
    }
    __device__ __forceinline__ uint8_t& hand(int p, int i) const { return B(HANDS + 12 * p + i); }
    __device__ __forceinline__ uint8_t& known(int p, int i) const { return B(KNOWN + 12 * p + i); }

    __device__ __forceinline__ void bind(uint32_t* lane_scratch, const GameParams&) { s = lane_scratch; }
    __device__ __forceinline__ void blank()
    {
#pragma unroll 1
        for (int w = 0; w < WORDS; w++) L(w) = 0u;
        L(W_META) = 1u << 23;
    }
    // the cards of a list of n bytes from byte b0 on, step d; bit 63: a byte that is no card, or one met twice
    __device__ __forceinline__ uint64_t list_mask(int b0, int d, int n) const
    {
        uint64_t m = 0;
#pragma unroll 1
        for (int i = 0; i < n; i++) {
            const int c = B(b0 + d * i);
            const uint64_t bit = 1ull << (c & 63);
            if (c >= NCARDS || (m & bit)) m |= 1ull << 63;
            else m |= bit;
        }
        return m;
    }
    __device__ __forceinline__ uint64_t hand_mask(int p) const { return list_mask(HANDS + 12 * p, 1, nh(p)); }
    __device__ __forceinline__ uint64_t known_mask(int p) const { return list_mask(KNOWN + 12 * p, 1, nk(p)); }
    __device__ __forceinline__ void load(const uint32_t* st, int64_t n, int64_t env)
    {
#pragma unroll 1
        for (int w = 0; w < WORDS; w++) L(w) = st[(int64_t)w * n + env];
        if (is_over()) return;   // (nothing of a finished game is read)
        // words written by cs_set_env_state are the caller's: the four card lists hold each of the 52 cards once (that
        // is what keeps every list inside its region), known_cards are hand cards; anything else is a finished game
        const uint64_t gone = gone_mask();
        bool ok = !(meta() >> 31) && !(gone >> NCARDS) && ns() + nd() + nh(0) + nh(1) + (gone ? 1 : 0) == NCARDS && nh(0) <= gin::HAND_MAX && nh(1) <= gin::HAND_MAX &&
                  nk(0) <= nh(0) && nk(1) <= nh(1) && last() <= L_SCORE_S && picked() < NCARDS;
        if (ok) {
            const uint64_t a = list_mask(0, 1, ns()), b = list_mask(NCARDS - 1, -1, nd());
            const uint64_t h0 = hand_mask(0), h1 = hand_mask(1), k0 = known_mask(0), k1 = known_mask(1);
            ok = !((a | b | h0 | h1 | k0 | k1) >> 63) && (a | b | h0 | h1 | gone) == gin::CARDS52 && !(k0 & ~h0) && !(k1 & ~h1);
        }
        if (!ok) blank();
    }
    __device__ __forceinline__ void store(uint32_t* st, int64_t n, int64_t env) const
    {
#pragma unroll 1
        for (int w = 0; w < WORDS; w++) st[(int64_t)w * n + env] = L(w);
    }

    // ---- the lists (every access bounded by the list's own counter) -----------------------------------------------
    __device__ __forceinline__ void hand_push(int p, int c) const
    {
        hand(p, nh(p)) = (uint8_t)c;
        add_cnt(12 + 4 * p, 1);
    }
    // stock_pile.pop() into the hand (nothing where the stock or the hand's 11 bytes have run out)
    __device__ __forceinline__ int draw(int p) const
    {
        const int k = ns();
        if (k == 0 || nh(p) >= gin::HAND_MAX) return -1;
        const int c = B(k - 1);
        add_cnt(0, -1);
        hand_push(p, c);
        return c;
    }
    // hand.remove(card) / known_cards.remove(card): the later cards keep their order
    __device__ __forceinline__ void remove_card(int p, int c) const
    {
        int n = nh(p), o = 0;
        for (int i = 0; i < n; i++) {
            const int x = hand(p, i);
            if (x != c) hand(p, o++) = (uint8_t)x;
        }
        add_cnt(12 + 4 * p, o - n);
        n = nk(p);
        o = 0;
        for (int i = 0; i < n; i++) {
            const int x = known(p, i);
            if (x != c) known(p, o++) = (uint8_t)x;
        }
        add_cnt(20 + 4 * p, o - n);
    }
    __device__ __forceinline__ void hand_words(int p, uint32_t (&hw)[gin::HAND_WORDS]) const
    {
        const int w = (HANDS + 12 * p) >> 2;
        hw[0] = L(w);
        hw[1] = L(w + 1);
        hw[2] = L(w + 2);
    }
    // the judge on seat p's 11 cards, its answer into the state (see the header)
    __device__ __forceinline__ void judge(int p) const
    {
        uint32_t hw[gin::HAND_WORDS];
        hand_words(p, hw);
        uint64_t knock, g;
        gin::going_out<false>(hw, nh(p), &knock, &g);
        const uint64_t v = knock | (g ? 1ull << 63 : 0ull);
        L(W_KNOCK) = (uint32_t)v;
        L(W_KNOCK + 1) = (uint32_t)(v >> 32);
    }
    __device__ __forceinline__ void forget() const
    {
        L(W_KNOCK) = 0u;
        L(W_KNOCK + 1) = 0u;
    }

    // ---- Game.init_game ---------------------------------------------------------------------------------------------
    template <class Rng>
    __device__ __forceinline__ void reset(Rng& rng)
    {
        const int dealer = (int)rng.interval(1u);   // np_random.choice([0, 1])
#pragma unroll 1
        for (int w = 0; w < NCARDS / 4; w++) {   // utils.get_deck(): card id i at index i
            const uint32_t b = 4u * (uint32_t)w;
            L(w) = b | (b + 1u) << 8 | (b + 2u) << 16 | (b + 3u) << 24;
        }
#pragma unroll 1
        for (int w = NCARDS / 4; w < WORDS; w++) L(w) = 0u;
        L(W_CNT) = NCARDS;
        // np_random.shuffle: Fisher-Yates i = 51 .. 1, j = random_interval(i), swap
        rng.draw_intervals((uint32_t)NCARDS - 1u, [&](uint32_t k, uint32_t j) {
            const uint32_t i = (uint32_t)NCARDS - 1u - k;
            uint8_t& pi = B((int)i);
            uint8_t& pj = B((int)j);
            const uint8_t ci = pi, cj = pj;
            pi = cj;
            pj = ci;
        });
        const int first = dealer ^ 1;
        for (int k = 0; k < 11; k++) draw(first);
        for (int k = 0; k < 10; k++) draw(dealer);
        L(W_META) = (uint32_t)first | (uint32_t)dealer << 1 | 1u << 12;   // move_sheet = [the deal]
        judge(first);
    }

    // ---- Judge.get_legal_actions as an id mask ---------------------------------------------------------------------
    __device__ __forceinline__ Legal128 legal() const
    {
        Legal128 m{0ull, 0ull};
        if (is_over()) return m;
        const int la = last();
        if (la == L_NONE || la == L_DRAW || la == L_PICK) {
            const uint64_t v = (uint64_t)L(W_KNOCK) | (uint64_t)L(W_KNOCK + 1) << 32;
            if (v >> 63) {
                m.lo = 1ull << GIN;
                return m;
            }
            const uint64_t h = hand_mask(current()) & gin::CARDS52;
            uint64_t d = h;
            if (la == L_PICK) d &= ~(1ull << picked());   // is_allowed_to_discard_picked_up_card = False
            const uint64_t k = v & h;
            m.lo = d << DISCARD | k << KNOCK;
            m.hi = k >> (64 - KNOCK);
        } else if (la == L_DISCARD) {
            if (moves() >= MAX_MOVES) m.lo = 1ull << DEAD;
            else if (ns() > DEAD_STOCK) m.lo = 1ull << DRAW | 1ull << PICK;
            else m.lo = 1ull << DEAD | 1ull << PICK;
        } else if (la == L_SCORE_N) {
            m.lo = 1ull << SCORE_S;
        } else if (la != L_SCORE_S) {   // dead hand, gin, knock
            m.lo = 1ull << SCORE_N;
        }
        return m;
    }

    // ---- envs/gin_rummy.py _extract_state: five planes of 52, the current player's whoever asks ---------------------
    template <int POS>
    __device__ static __forceinline__ void put(uint32_t (&bits)[NB], uint64_t v)
    {
        constexpr int W = POS / 32, S = POS % 32;
        bits[W] |= (uint32_t)(v << S);
        if constexpr (W + 1 < NB) bits[W + 1] |= (uint32_t)(S ? v >> (32 - S) : v >> 32);
        if constexpr (S != 0 && W + 2 < NB) bits[W + 2] |= (uint32_t)(v >> (64 - S));
    }
    __device__ __forceinline__ void observe(int, uint32_t (&bits)[NB]) const
    {
#pragma unroll
        for (int w = 0; w < NB; w++) bits[w] = 0u;
        if (is_over()) return;
        const int cur = current(), n = nd();
        const uint64_t h = hand_mask(cur) & gin::CARDS52, k = known_mask(cur ^ 1) & gin::CARDS52;
        const uint64_t top = n > 0 ? 1ull << (B(NCARDS - n) & 63) : 0ull;
        const uint64_t dead = list_mask(NCARDS - 1, -1, n > 0 ? n - 1 : 0) & gin::CARDS52;
        // stock + the opponent's cards not known = every card that is in none of the four planes above and has not left
        const uint64_t unknown = gin::CARDS52 & ~(h | top | dead | k | gone_mask());
        put<0>(bits, h);
        put<52>(bits, top);
        put<104>(bits, dead);
        put<156>(bits, k);
        put<208>(bits, unknown);
    }

    template <class Rng>
    __device__ __forceinline__ void step(int a, Rng&)
    {
        const Legal128 lg = legal();
        if (legal_empty(lg)) return;
        if (a < 0 || a >= A || !legal_has(lg, a)) a = legal_lowest(lg);   // this ABI's fallback: lowest legal id
        const int cur = current();
        int la, next = cur;
        forget();
        if (a == DRAW) {
            draw(cur);
            la = L_DRAW;
            judge(cur);
        } else if (a == PICK) {
            const int n = nd();
            int c = 0;
            if (n > 0 && nh(cur) < gin::HAND_MAX && nk(cur) < gin::HAND_MAX) {
                c = B(NCARDS - n);
                add_cnt(6, -1);
                hand_push(cur, c);
                known(cur, nk(cur)) = (uint8_t)c;
                add_cnt(20 + 4 * cur, 1);
            }
            set_field(6, 63u, c);
            la = L_PICK;
            judge(cur);
        } else if (a == DEAD) {
            set_field(20, 7u, GO_DEAD | cur << 2);
            la = L_DEAD;
            next = 0;
        } else if (a == GIN) {
            uint32_t hw[gin::HAND_WORDS];
            hand_words(cur, hw);
            const int c = gin::gin_card(hw, nh(cur));
            if (c >= 0) {
                remove_card(cur, c);
                set_field(24, 127u, c | 64);
            }
            set_field(20, 7u, GO_GIN | cur << 2);
            la = L_GIN;
            next = 0;
        } else if (a >= KNOCK) {
            remove_card(cur, a - KNOCK);
            set_field(24, 127u, (a - KNOCK) | 64);
            set_field(20, 7u, GO_KNOCK | cur << 2);
            la = L_KNOCK;
            next = 0;
        } else if (a >= DISCARD) {
            const int c = a - DISCARD;
            remove_card(cur, c);
            if (ns() + nd() < NCARDS) {
                B(NCARDS - 1 - nd()) = (uint8_t)c;
                add_cnt(6, 1);
            }
            la = L_DISCARD;
            next = cur ^ 1;
        } else if (a == SCORE_N) {
            la = L_SCORE_N;
            next = 1;
        } else {
            la = L_SCORE_S;
            set_field(23, 1u, 1);
        }
        set_field(2, 15u, la);
        set_field(0, 1u, next);
        const int mv = moves();
        set_field(12, 255u, mv < 255 ? mv + 1 : mv);
    }

    __device__ __forceinline__ void payoffs(float (&r)[P]) const
    {
        const int kind = go_kind(), who = go_player();
#pragma unroll 1
        for (int p = 0; p < P; p++) {
            if (who == p && kind == GO_KNOCK) {
                r[p] = 0.2f;
            } else if (who == p && kind == GO_GIN) {
                r[p] = 1.f;
            } else {
                uint32_t hw[gin::HAND_WORDS];
                hand_words(p, hw);
                r[p] = gin::deadwood_payoff(gin::best_deadwood(hw, nh(p)));
            }
        }
    }

    // ---- gin-rummy-novice-rule (models/gin_rummy_rule_models.py GinRummyNoviceRuleAgent.step) ----------------------
    // gin if legal; else one of the knocks; else one of the discards after which the other 10 cards have the least best
    // deadwood; else any legal id. The reference draws each pick from the global np.random; here it is the step's policy
    // word r with the random policy's formula. A hand's melds without card c are its melds that do not hold c, so the
    // meld list is built once for all the discards.
    __device__ __forceinline__ int rule_action(uint32_t, int player, const Legal128& lg, uint32_t r) const
    {
        if ((lg.lo >> GIN) & 1ull) return GIN;
        const uint64_t knocks = (lg.lo >> KNOCK | lg.hi << (64 - KNOCK)) & gin::CARDS52;
        if (knocks) return KNOCK + pick_legal64(knocks, r);
        const uint64_t discards = (lg.lo >> DISCARD) & gin::CARDS52;
        if (discards) {
            uint32_t hw[gin::HAND_WORDS];
            hand_words(player, hw);
            gin::Melds ms;
            gin::build(hw, nh(player), ms);
            const int total = gin::mask_value(hand_mask(player) & gin::CARDS52);
            int best = 999;
            uint64_t cand = 0;
            for (uint64_t d = discards; d; d &= d - 1) {
                const int c = gin::ctz52(d);
                const int dw = total - gin::card_value(c) - gin::best_melded(ms, 1ull << c);
                if (dw < best) {
                    best = dw;
                    cand = 0;
                }
                if (dw == best) cand |= 1ull << c;
            }
            return DISCARD + pick_legal64(cand, r);
        }
        return pick_legal128(lg, r);
    }
};

}  // namespace cs
