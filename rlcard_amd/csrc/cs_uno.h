// cs_uno.h -- UNO (2 players) as a lane-per-env lockstep state machine.
//
// Behaviour (reference file):
//   rlcard/games/uno/utils.py    init_deck: per colour r, g, b, y the numbers 0..9 (1..9 twice), skip / reverse /
//                                draw_2 twice, one wild, one wild_draw_4 (108 cards); the 61 action ids are
//                                colour * 15 + trait (traits 0..9, skip 10, reverse 11, draw_2 12, wild 13,
//                                wild_draw_4 14) and draw = 60; encode_hand / encode_target
//   rlcard/games/uno/dealer.py   np_random.shuffle of the deck list, deal_cards = deck.pop() per card, flip_top_card
//                                (a wild_draw_4 goes back and the whole deck is reshuffled, in a loop)
//   rlcard/games/uno/game.py     init_game: 7 cards to each player, top card flipped and performed; payoffs +1 / -1
//   rlcard/games/uno/round.py    flip_top_card (a wild top is coloured by choice(colours)), perform_top_card,
//                                proceed_round, get_legal_actions, replace_deck, _perform_draw_action,
//                                _preform_non_number_action
//   rlcard/envs/uno.py           obs [4][4][15] 0/1 (three hand planes, one target plane), legal ids
//   rlcard/models/uno_rule_models.py   uno-rule-v1 = CS_POLICY_RULE_V1 (rule_action below)
// Order is observable (hand order gives the order of the legal list and which duplicate is played; the played pile's
// order feeds replace_deck), so the state keeps ordered lists. A card is one byte: bits 0..5 its identity = the action
// id that plays it with its ORIGINAL colour (colour * 15 + trait), bits 6..7 its LIVE colour. The two differ only for
// the 8 wild cards: card.color is rewritten when a wild is played, drawn by the `draw` action or flipped as the top
// card, and survives replace_deck and being dealt again, while card.str -- what state['target'] and so obs plane 3
// show -- keeps the original colour. Matching uses the live colour.
// Every card changes colour only at the moment it becomes the target, so the target is kept by value.
// With two players (x + direction) % 2 is the other player whatever the direction, and nothing observable shows the
// direction, so it is not kept: reverse passes the turn, skip and the draw cards keep it.
// Packed state, 56 u32 words per env (word-major [56][N]) = the lane's LDS scratch, byte b in byte b % 4 of word b / 4:
//   bytes   0..107  the draw pile up from byte 0 (deck[i] at byte i, deck.pop() takes byte nd - 1) and the played
//                   pile down from byte 107 (played_cards[i] at byte 107 - i); nd + np <= 108
//   bytes 108..215  player 0's hand up from byte 108 (hand[i] at 108 + i), player 1's down from byte 215 (215 - i)
//   word 54         nd | np << 8 | len(hand 0) << 16 | len(hand 1) << 24
//   word 55         target card | current_player << 8 | over << 9 | winner << 10
// The four lists always hold the 108 cards between them, so no list can outgrow its region.
// Defined by this ABI where the reference is undefined: an illegal action id plays the lowest legal id (the reference
// draws from the global np.random); a deal or a draw that finds fewer cards than it needs even after replace_deck
// takes the cards that are there (a draw that finds none only passes the turn; the reference raises IndexError).
#pragma once
#include "cs_device.h"
#include "../../include/cardsim.h"

namespace cs {

struct Uno : GameDefaults {
    static constexpr int OBS = 240, A = 61, P = 2, LB = 8, WORDS = 56, ACTION_BYTES = 1;
    static constexpr int NB = 8;               // obs bitmap words
    static constexpr bool RAW_OBS = false;
    static constexpr int SCRATCH_WORDS = WORDS;   // the whole state lives in the lane's LDS scratch
    static constexpr int STAGE_W = 64, STAGE_PAD = 4, STAGE_R = 16, STAGE_RF = 32;
    static constexpr int RESTAGE_B = 4;
    static constexpr bool OBS_DIRECT = true;   // no 60 KB obs image per block: two blocks per CU instead of one
    static constexpr int MIN_WAVES = 2;   // the LDS (state 56 KB + stage rows 17 KB per block) allows two blocks per CU
    static constexpr int EPW = 64;
    static constexpr int MAX_POLICY = CS_POLICY_RULE_V1;
    static constexpr int NCARDS = 108, HAND0 = 108, HAND1 = 215, W_CNT = 54, W_META = 55, DRAW = 60;
    static constexpr uint64_t WILD_IDS = 1ull << 13 | 1ull << 28 | 1ull << 43 | 1ull << 58;   // the four *-wild ids
    static constexpr uint64_t WD4_IDS = WILD_IDS << 1;                                        // *-wild_draw_4

    uint32_t* s;   // lane scratch: state word i at s[i * WAVE]

    __device__ __forceinline__ uint32_t& L(int i) const { return s[i * WAVE]; }
    // byte b of the state: (b >> 2) * 256 + (b & 3) = b + 252 * (b >> 2)
    static_assert(WAVE * 4 == 256, "state byte address");
    __device__ __forceinline__ uint8_t& B(int b) const { return ((uint8_t*)s)[b + 252 * (b >> 2)]; }

    __device__ __forceinline__ int nd() const { return L(W_CNT) & 255; }
    __device__ __forceinline__ int np() const { return (L(W_CNT) >> 8) & 255; }
    __device__ __forceinline__ int nh(int p) const { return (L(W_CNT) >> (16 + 8 * p)) & 255; }
    __device__ __forceinline__ void add_cnt(int field, int d) const { L(W_CNT) += (uint32_t)d << (8 * field); }
    __device__ __forceinline__ int target() const { return L(W_META) & 255; }
    __device__ __forceinline__ void set_target(int c) const { L(W_META) = (L(W_META) & ~255u) | (uint32_t)c; }
    __device__ __forceinline__ int current() const { return (L(W_META) >> 8) & 1; }
    __device__ __forceinline__ bool is_over() const { return (L(W_META) >> 9) & 1; }
    __device__ __forceinline__ void pass_turn() const { L(W_META) ^= 1u << 8; }

    __device__ static __forceinline__ int trait_of(int c) { return (c & 63) % 15; }
    __device__ static __forceinline__ int live_of(int c) { return c >> 6; }
    __device__ __forceinline__ uint8_t& hand(int p, int i) const { return B(p ? HAND1 - i : HAND0 + i); }

    __device__ __forceinline__ void bind(uint32_t* lane_scratch, const GameParams&) { s = lane_scratch; }
    __device__ __forceinline__ void blank()
    {
#pragma unroll 1
        for (int w = 0; w < WORDS; w++) L(w) = 0u;
        L(W_META) = 1u << 9;
    }
    __device__ __forceinline__ void load(const uint32_t* st, int64_t n, int64_t env)
    {
#pragma unroll 4
        for (int w = 0; w < WORDS; w++) L(w) = st[(int64_t)w * n + env];
        // words written by cs_set_env_state are the caller's: the four lists hold the 108 cards between them (that is
        // what keeps every list inside its region); anything else is a finished game
        if (nd() + np() + nh(0) + nh(1) != NCARDS) blank();
    }
    __device__ __forceinline__ void store(uint32_t* st, int64_t n, int64_t env) const
    {
#pragma unroll 4
        for (int w = 0; w < WORDS; w++) st[(int64_t)w * n + env] = L(w);
    }

    // ---- the lists ------------------------------------------------------------------------------------------------
    __device__ __forceinline__ int deck_pop() const
    {
        const int k = nd() - 1;
        add_cnt(0, -1);
        return B(k);
    }
    __device__ __forceinline__ void played_push(int c) const
    {
        B(NCARDS - 1 - np()) = (uint8_t)c;
        add_cnt(1, 1);
    }
    __device__ __forceinline__ void hand_push(int p, int c) const
    {
        hand(p, nh(p)) = (uint8_t)c;
        add_cnt(2 + p, 1);
    }
    // Dealer.deal_cards: deck.pop() per card (what is there, where the deck runs out)
    __device__ __forceinline__ void deal(int p, int k) const
    {
        for (; k > 0 && nd() > 0; k--) hand_push(p, deck_pop());
    }
    // np_random.shuffle of deck[0..n): Fisher-Yates i = n - 1 .. 1, j = random_interval(i), swap
    template <class Rng>
    __device__ __forceinline__ void shuffle(Rng& rng, int n) const
    {
        if (n < 2) return;
        const uint32_t hi = (uint32_t)n - 1u;
        rng.draw_intervals(hi, [&](uint32_t k, uint32_t j) {
            const uint32_t i = hi - k;
            uint8_t& pi = B((int)i);
            uint8_t& pj = B((int)j);
            const uint8_t ci = pi, cj = pj;
            pi = cj;
            pj = ci;
        });
    }
    // Round.replace_deck: deck.extend(played_cards), shuffle, played_cards = []. The played pile (down from byte 107)
    // is reversed in place, then moved down behind the deck (ascending, destination <= source).
    template <class Rng>
    __device__ __forceinline__ void replace_deck(Rng& rng) const
    {
        const int d = nd(), p = np(), lo = NCARDS - p;
        for (int i = 0; i < p / 2; i++) {
            uint8_t& x = B(lo + i);
            uint8_t& y = B(NCARDS - 1 - i);
            const uint8_t cx = x, cy = y;
            x = cy;
            y = cx;
        }
        if (d != lo)
            for (int i = 0; i < p; i++) B(d + i) = B(lo + i);
        L(W_CNT) = (L(W_CNT) & 0xFFFF0000u) | (uint32_t)(d + p);
        shuffle(rng, d + p);
    }

    // ---- Game.init_game ---------------------------------------------------------------------------------------------
    template <class Rng>
    __device__ __forceinline__ void reset(Rng& rng)
    {
        // init_deck's order: 27 cards per colour, k = 0..24 the traits (k + 1) / 2, then wild and wild_draw_4
#pragma unroll 1
        for (int w = 0; w < NCARDS / 4; w++) {
            uint32_t v = 0;
#pragma unroll
            for (int q = 0; q < 4; q++) {
                const int i = 4 * w + q, col = i / 27, k = i - 27 * col;
                const int trait = k <= 24 ? (k + 1) >> 1 : k - 12;
                v |= (uint32_t)((col * 15 + trait) | (col << 6)) << (8 * q);
            }
            L(w) = v;
        }
        L(W_CNT) = NCARDS;
        L(W_META) = 0;
        shuffle(rng, NCARDS);
        deal(0, 7);
        deal(1, 7);
        int top = deck_pop();
        while (trait_of(top) == 14) {   // Dealer.flip_top_card: a wild_draw_4 goes back, the deck is reshuffled
            B(nd()) = (uint8_t)top;
            add_cnt(0, 1);
            shuffle(rng, nd());
            top = deck_pop();
        }
        const int tt = trait_of(top);
        if (tt == 13) top = (top & 63) | (int)rng.interval(3u) << 6;   // choice(colours)
        set_target(top);
        played_push(top);
        // perform_top_card: skip and reverse give player 1 the first turn, draw_2 deals two cards to player 0
        if (tt == 10 || tt == 11) pass_turn();
        else if (tt == 12) deal(0, 2);
    }

    // ---- Round.get_legal_actions of `player`'s hand as an id mask --------------------------------------------------
    __device__ __forceinline__ uint64_t legal_of(int player) const
    {
        const int t = target(), tl = live_of(t), ttr = trait_of(t);
        const int n = nh(player);
        uint64_t m = 0;
        bool wild = false, wd4 = false;
        for (int i = 0; i < n; i++) {
            const int c = hand(player, i), tr = trait_of(c);
            if (tr >= 13) {
                wild |= tr == 13;
                wd4 |= tr == 14;
            } else if (live_of(c) == tl || (ttr < 13 && tr == ttr)) {
                m |= 1ull << (c & 63);
            }
        }
        if (wild) m |= WILD_IDS;
        if (m == 0 && wd4) m = WD4_IDS;
        if (m == 0) m = 1ull << DRAW;
        return m;
    }
    __device__ __forceinline__ uint64_t legal() const { return legal_of(current()); }

    // ---- envs/uno.py _extract_state: planes 0..2 the hand (no copy / one / two; the wild columns for all four
    // colours at once, in plane 1), plane 3 the target by its original colour. Bit plane * 60 + colour * 15 + trait.
    __device__ __forceinline__ void observe(int player, uint32_t (&bits)[NB]) const
    {
        const int n = nh(player);
        uint64_t once = 0, twice = 0;
        for (int i = 0; i < n; i++) {
            const int c = hand(player, i), tr = trait_of(c);
            const uint64_t bit = tr >= 13 ? (tr == 13 ? WILD_IDS : WD4_IDS) : 1ull << (c & 63);
            twice |= tr >= 13 ? 0ull : once & bit;
            once |= bit;
        }
        constexpr uint64_t M60 = (1ull << 60) - 1;
        const uint64_t p0 = ~once & M60, p1 = once & ~twice, p2 = twice, p3 = 1ull << (target() & 63);
        // 240 bits: p0 at 0, p1 at 60, p2 at 120, p3 at 180
        const uint64_t q0 = p0 | p1 << 60, q1 = p1 >> 4 | p2 << 56, q2 = p2 >> 8 | p3 << 52, q3 = p3 >> 12;
        bits[0] = (uint32_t)q0; bits[1] = (uint32_t)(q0 >> 32);
        bits[2] = (uint32_t)q1; bits[3] = (uint32_t)(q1 >> 32);
        bits[4] = (uint32_t)q2; bits[5] = (uint32_t)(q2 >> 32);
        bits[6] = (uint32_t)q3; bits[7] = (uint32_t)(q3 >> 32);
    }

    // ---- Round._preform_non_number_action for the current player's card (two players: see the header) -----------
    template <class Rng>
    __device__ __forceinline__ void perform(int card, Rng& rng) const
    {
        const int tr = trait_of(card), cur = current();
        if (tr == 11) {
            pass_turn();   // reverse
        } else if (tr == 12 || tr == 14) {
            const int k = tr == 12 ? 2 : 4;
            if (nd() < k) replace_deck(rng);
            deal(cur ^ 1, k);
        }   // skip, draw_2, wild_draw_4: the turn comes back; wild: handled by the caller
        if (tr == 13) pass_turn();
        set_target(card);
    }

    template <class Rng>
    __device__ __forceinline__ void step(int a, Rng& rng)
    {
        const int cur = current();
        const uint64_t lg = legal_of(cur);
        if (a < 0 || a >= A || !((lg >> a) & 1ull)) a = __builtin_ctzll(lg);   // this ABI's fallback: lowest legal id
        if (a == DRAW) {   // Round._perform_draw_action
            if (nd() == 0) replace_deck(rng);
            if (nd() == 0) {   // nothing to draw even so: the turn passes
                pass_turn();
                return;
            }
            int card = deck_pop();
            const int tr = trait_of(card);
            if (tr >= 13) {
                card = (card & 63) | (int)rng.interval(3u) << 6;
                set_target(card);
                played_push(card);
                pass_turn();
            } else if (live_of(card) == live_of(target())) {
                played_push(card);
                if (tr < 10) {
                    set_target(card);
                    pass_turn();
                } else {
                    perform(card, rng);
                }
            } else {
                hand_push(cur, card);
                pass_turn();
            }
            return;
        }
        // Round.proceed_round: the first hand card of the action's trait (wild cards: recoloured) or colour and trait
        const int col = a / 15, tr = a - 15 * col, n = nh(cur);
        const bool wild = tr >= 13;
        const int want = a | col << 6;
        int k = 0;
        for (; k < n; k++) {
            const int c = hand(cur, k);
            if (wild ? trait_of(c) == tr : c == want) break;
        }
        if (k == n) return;   // (a legal id always has its card)
        const int card = wild ? ((hand(cur, k) & 63) | col << 6) : want;
        for (int i = k; i + 1 < n; i++) hand(cur, i) = hand(cur, i + 1);
        add_cnt(2 + cur, -1);
        if (n == 1) L(W_META) |= 1u << 9 | (uint32_t)cur << 10;   // is_over, winner: before the card is performed
        played_push(card);
        if (tr < 10) {
            pass_turn();
            set_target(card);
        } else {
            perform(card, rng);
        }
    }

    __device__ __forceinline__ void payoffs(float (&r)[P]) const
    {
        const int w = (L(W_META) >> 10) & 1;
        r[0] = w == 0 ? 1.f : -1.f;
        r[1] = w == 1 ? 1.f : -1.f;
    }

    // ---- uno-rule-v1 (models/uno_rule_models.py UNORuleAgentV1.step) ---------------------------------------------
    // draw if legal; with a wild_draw_4 legal, the wild_draw_4 of the colour most frequent in the hand (wild cards
    // left out unless the hand is all wild, then by their live colours; ties to the colour met first in hand order);
    // otherwise uniform over the legal ids without the *-wild ids (kept if nothing else is legal). The reference draws
    // that last pick from the global np.random; here it is the step's policy word r with the random policy's formula.
    __device__ __forceinline__ int rule_action(uint32_t, int player, uint64_t lg, uint32_t r) const
    {
        if ((lg >> DRAW) & 1ull) return DRAW;
        if (lg & WD4_IDS) {
            const int n = nh(player);
            uint32_t cnt = 0, cntw = 0;   // cards per live colour, 8 bits each: without / with the wild cards
            int plain = 0;
            for (int i = 0; i < n; i++) {
                const int c = hand(player, i);
                const bool w = trait_of(c) >= 13;
                cntw += 1u << (8 * live_of(c));
                cnt += w ? 0u : 1u << (8 * live_of(c));
                plain += w ? 0 : 1;
            }
            if (plain == 0) cnt = cntw;
            int best = 0, bestc = 0;
            for (int i = 0; i < n; i++) {   // max over a dict built in hand order: the first colour with the largest count
                const int c = hand(player, i);
                if (plain != 0 && trait_of(c) >= 13) continue;
                const int k = (cnt >> (8 * live_of(c))) & 255;
                if (k > best) {
                    best = k;
                    bestc = live_of(c);
                }
            }
            return bestc * 15 + 14;
        }
        const uint64_t plain = lg & ~WILD_IDS;
        return pick_legal64(plain ? plain : lg, r);
    }
};

}  // namespace cs
