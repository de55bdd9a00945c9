// cs_mahjong.h -- Mahjong (4 players) as a lane-per-env lockstep state machine.
//
// Behaviour (reference file):
//   rlcard/games/mahjong/utils.py   card_encoding_dict: the 38 action ids -- bamboo 1..9 = 0..8, characters 9..17,
//                                   dots 18..26, dragons green / red / white 27..29, winds east / west / north / south
//                                   30..33, pong 34, chow 35, gong 36, stand 37; init_deck: dots, bamboo, characters,
//                                   dragons, winds, that list of 34 four times over; encode_cards
//   rlcard/games/mahjong/card.py    a tile is (type, trait, index_num); the four copies of a tile are ONE object, so
//                                   `card in hand` / hand.index(card) compare tiles by value: a tile is its id here
//   rlcard/games/mahjong/dealer.py  np_random.shuffle of the deck list (the game's only draw), deal_cards = deck.pop()
//   rlcard/games/mahjong/game.py    init_game: 13 tiles to players 0..3, one more to player 0; is_over = judge_game
//   rlcard/games/mahjong/round.py   proceed_round (play / pong / gong / chow / stand), get_state
//   rlcard/games/mahjong/player.py  play_card, pong, gong (the table keeps its tile), chow (pops the table)
//   rlcard/games/mahjong/judger.py  judge_pong_gong (after a discard, players 0..3, first hit), judge_chow (inside
//                                   `stand`, offered to last_player + 1 only), judge_game, judge_hu (cs_mahjong_hu.h)
//   rlcard/envs/mahjong.py          obs [6][34][4] 0/1: hand, table, the four players' piles; column k of a tile's row
//                                   is set while k < its count; payoffs +1 / -1 / -1 / -1, all 0 without a winner
// Quirks kept: pong and gong leave the table's tile where it is and pile 3 / 4 copies of it; chow is judged only when a
// claim is refused, for the player after the one who acted last, with the shapes [i + 1, i + 2] at index 0 and
// [i - 2, i - 1] otherwise -- at index 1 hand_list[-1] is the suit's 9, and the pile is the suit's 1 plus the table
// tile; a claimer discards without drawing; after refused claims the draw goes to (player_before_act + 1) % 4; while
// a claim is offered every observer's hand plane is the current player's; judge_game's winner is the highest winning
// id; an empty deck ends the game.
// The order of a hand is observable (judge_hu's pair order, the raw side), so hands are ordered lists.
// Packed state, 55 u32 words per env (word-major [55][N]) = the lane's LDS scratch, byte b in byte b % 4 of word b / 4:
//   bytes   0..135  the deck up from byte 0 (deck[i] at byte i, deck.pop() takes byte nd - 1) and the table down from
//                   byte 135 (table[i] at byte 135 - i); nd + nt <= 136
//   bytes 136..199  the hands, 16 bytes per player: hand[i] at 136 + 16 p + i (i < 14), byte 14 len(hand), byte 15
//                   len(pile)
//   bytes 200..215  the piles, 4 bytes per player: pile k of player p at 200 + 4 p + k = kind << 6 | the table tile it
//                   claimed (kind 1 pong: 3 copies, 3 gong: 4 copies, 2 chow: [t - 2, t - 1, t], [t + 1, t + 2, t] at
//                   index 0, [t - 1, t] at index 1)
//   word 54         nd | nt << 8 | current_player << 16 | last_player << 18 | player_before_act << 20 |
//                   valid_act << 22 (0 none, 1 pong, 2 chow, 3 gong) | judge_hu of seats 0..3 << 24 | over << 28
// The judge's answers are kept in the meta word: a step re-judges only the seats whose hand or pile it changed, and
// is_over() reads a bit. last_cards is not kept: it is the table's last tile under valid_act's shape.
// Defined by this ABI where the reference raises or misbehaves: an illegal action id plays the lowest legal id; a game
// already won on the deal is done = 1 at the reset row; an empty legal set is a zero mask.
#pragma once
#include "cs_device.h"
#include "cs_mahjong_hu.h"
#include "../../include/cardsim.h"

namespace cs {

struct Mahjong : GameDefaults {
    static constexpr int OBS = 816, A = 38, P = 4, LB = 5, WORDS = 55, ACTION_BYTES = 1;
    static constexpr int NB = 26;              // obs bitmap words (816 bits)
    static constexpr bool RAW_OBS = false;
    static constexpr int SCRATCH_WORDS = WORDS;   // the whole state lives in the lane's LDS scratch
    static constexpr int STAGE_W = 64, STAGE_PAD = 4, STAGE_R = 16, STAGE_RF = 32;
    static constexpr int RESTAGE_B = 4;
    static constexpr bool OBS_DIRECT = true;   // 816 = 51 x 16: the rows leave as per-lane 16-byte stores
    // LDS per block: state 55 KB + stage rows 17 KB = 72 KB: two blocks per CU (160 KB), as UNO; a third does not fit
    static constexpr int MIN_WAVES = 2;
    static constexpr int EPW = 64;
    static constexpr bool RANDOM_ACTIONS = true;   // cs_policy_actions(CS_POLICY_RANDOM); the reference has no rule model
    static constexpr int NTILES = 136, HANDS = 136, PILES = 200, W_META = 54;
    static constexpr int PONG = 34, CHOW = 35, GONG = 36, STAND = 37;
    static constexpr int V_PONG = 1, V_CHOW = 2, V_GONG = 3;

    uint32_t* s;   // lane scratch: state word i at s[i * WAVE]

    __device__ __forceinline__ uint32_t& L(int i) const { return s[i * WAVE]; }
    static_assert(WAVE * 4 == 256, "state byte address");
    __device__ __forceinline__ uint8_t& B(int b) const { return ((uint8_t*)s)[b + 252 * (b >> 2)]; }

    __device__ __forceinline__ uint32_t meta() const { return L(W_META); }
    __device__ __forceinline__ int nd() const { return meta() & 255; }
    __device__ __forceinline__ int nt() const { return (meta() >> 8) & 255; }
    __device__ __forceinline__ int current() const { return (meta() >> 16) & 3; }
    __device__ __forceinline__ int last_player() const { return (meta() >> 18) & 3; }
    __device__ __forceinline__ int before_act() const { return (meta() >> 20) & 3; }
    __device__ __forceinline__ int valid_act() const { return (meta() >> 22) & 3; }
    __device__ __forceinline__ int wins() const { return (meta() >> 24) & 15; }
    __device__ __forceinline__ bool is_over() const { return (meta() >> 28) & 1; }
    __device__ __forceinline__ void set_field(int shift, uint32_t mask, int v) const
    {
        L(W_META) = (meta() & ~(mask << shift)) | ((uint32_t)v & mask) << shift;
    }
    __device__ __forceinline__ uint8_t& hand(int p, int i) const { return B(HANDS + 16 * p + i); }
    __device__ __forceinline__ uint8_t& nh(int p) const { return B(HANDS + 16 * p + 14); }
    __device__ __forceinline__ uint8_t& npile(int p) const { return B(HANDS + 16 * p + 15); }
    __device__ __forceinline__ uint8_t& pile(int p, int k) const { return B(PILES + 4 * p + k); }
    __device__ __forceinline__ int table_top() const { return nt() > 0 ? B(NTILES - nt()) : 0; }

    __device__ __forceinline__ void bind(uint32_t* lane_scratch, const GameParams&) { s = lane_scratch; }
    __device__ __forceinline__ void blank()
    {
#pragma unroll 1
        for (int w = 0; w < WORDS; w++) L(w) = 0u;
        L(W_META) = 1u << 28;
    }
    __device__ __forceinline__ void load(const uint32_t* st, int64_t n, int64_t env)
    {
#pragma unroll 5
        for (int w = 0; w < WORDS; w++) L(w) = st[(int64_t)w * n + env];
        // words written by cs_set_env_state are the caller's: every list must fit its region and hold tiles; anything
        // else is a finished game
        bool ok = nd() + nt() <= NTILES;
        for (int p = 0; p < P; p++) ok = ok && nh(p) <= mj::HAND_MAX && npile(p) <= 4;
        if (ok) {
            for (int p = 0; p < P; p++) {
                for (int i = 0; i < nh(p); i++) ok = ok && hand(p, i) < mj::TILES;
                for (int k = 0; k < npile(p); k++) ok = ok && (pile(p, k) & 63) < mj::TILES && (pile(p, k) >> 6) != 0;
            }
            const int d = nd(), t0 = NTILES - nt();   // the deck's bytes [0, d) and the table's [t0, 136)
#pragma unroll 1
            for (int w = 0; w < NTILES / 4; w++) {
                const uint32_t v = L(w);
#pragma unroll
                for (int q = 0; q < 4; q++) {
                    const int b = 4 * w + q;
                    ok = ok && (!(b < d || b >= t0) || ((v >> (8 * q)) & 255u) < (uint32_t)mj::TILES);
                }
            }
        }
        if (!ok) blank();
    }
    __device__ __forceinline__ void store(uint32_t* st, int64_t n, int64_t env) const
    {
#pragma unroll 5
        for (int w = 0; w < WORDS; w++) st[(int64_t)w * n + env] = L(w);
    }

    // ---- the lists ------------------------------------------------------------------------------------------------
    // Dealer.deal_cards(player, 1): deck.pop() (nothing where the deck or the hand's 14 bytes have run out)
    __device__ __forceinline__ void draw(int p) const
    {
        const int k = nd(), n = nh(p);
        if (k == 0 || n >= mj::HAND_MAX) return;
        hand(p, n) = B(k - 1);
        nh(p) = (uint8_t)(n + 1);
        L(W_META) -= 1u;
    }
    // hand.pop(hand.index(tile)) up to `copies` times: the first occurrences go, the rest keep their order
    __device__ __forceinline__ void hand_remove(int p, int tile, int copies) const
    {
        const int n = nh(p);
        int o = 0;
        for (int i = 0; i < n; i++) {
            const int c = hand(p, i);
            if (c == tile && copies > 0) {
                copies--;
            } else {
                hand(p, o) = (uint8_t)c;
                o++;
            }
        }
        nh(p) = (uint8_t)o;
    }
    __device__ __forceinline__ int hand_count(int p, int tile) const
    {
        const int n = nh(p);
        int k = 0;
        for (int i = 0; i < n; i++) k += hand(p, i) == tile;
        return k;
    }
    __device__ __forceinline__ void pile_push(int p, int kind, int tile) const
    {
        const int k = npile(p);
        if (k >= 4) return;
        pile(p, k) = (uint8_t)(kind << 6 | tile);
        npile(p) = (uint8_t)(k + 1);
    }
    // the judge on seat p, its answer into the meta word
    __device__ __forceinline__ void judge(int p) const
    {
        const int w = (HANDS + 16 * p) >> 2;
        const uint32_t h[4] = {L(w), L(w + 1), L(w + 2), L(w + 3)};
        const bool win = mj::judge_hu(h, nh(p), npile(p));
        set_field(24 + p, 1u, win);
    }
    // judge_game after a step: a winner or an empty deck ends the game
    __device__ __forceinline__ void settle() const { set_field(28, 1u, wins() != 0 || nd() == 0); }

    // np_random.shuffle of deck[0..n): Fisher-Yates i = n - 1 .. 1, j = random_interval(i), swap
    template <class Rng>
    __device__ __forceinline__ void shuffle(Rng& rng, int n) const
    {
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

    // ---- Game.init_game ---------------------------------------------------------------------------------------------
    template <class Rng>
    __device__ __forceinline__ void reset(Rng& rng)
    {
        // init_deck's order: dots, bamboo, characters, dragons, winds, four times
#pragma unroll 1
        for (int w = 0; w < NTILES / 4; w++) {
            uint32_t v = 0;
#pragma unroll
            for (int q = 0; q < 4; q++) {
                const int j = (4 * w + q) % 34;
                v |= (uint32_t)(j < 9 ? j + 18 : j < 27 ? j - 9 : j) << (8 * q);
            }
            L(w) = v;
        }
#pragma unroll 1
        for (int w = NTILES / 4; w < WORDS; w++) L(w) = 0u;
        L(W_META) = NTILES;
        shuffle(rng, NTILES);
        for (int p = 0; p < P; p++)
            for (int k = 0; k < 13; k++) draw(p);
        draw(0);
#pragma unroll 1
        for (int p = 0; p < P; p++) judge(p);
        settle();
    }

    // ---- Game.get_legal_actions of the current player as an id mask -------------------------------------------------
    __device__ __forceinline__ uint64_t legal() const
    {
        const int v = valid_act();
        if (v) return 1ull << STAND | 1ull << (v == V_PONG ? PONG : v == V_CHOW ? CHOW : GONG);
        const int p = current(), n = nh(p);
        uint64_t m = 0;
        for (int i = 0; i < n; i++) m |= 1ull << hand(p, i);
        return m;
    }

    // ---- envs/mahjong.py _extract_state: six planes of 34 x 4, a tile's row filled from column 0 up to its count ------
    struct Plane {   // 4 bits per tile: tiles 0..15, 16..31, 32..33
        uint64_t a, b;
        uint32_t c;
        __device__ __forceinline__ void add(int t)
        {
            const int sh = 4 * (t & 15), k = t >> 4;
            const uint64_t m = 15ull << sh;
            uint64_t w = k == 0 ? a : k == 1 ? b : (uint64_t)c;
            w |= (((w & m) << 1) & m) | 1ull << sh;   // plane[index][:num] = 1
            a = k == 0 ? w : a;
            b = k == 1 ? w : b;
            c = k == 2 ? (uint32_t)w : c;
        }
    };
    template <int POS>
    __device__ static __forceinline__ void put(uint32_t (&bits)[NB], uint64_t v)
    {
        constexpr int W = POS / 32, S = POS % 32;
        bits[W] |= (uint32_t)(v << S);
        if constexpr (W + 1 < NB) bits[W + 1] |= (uint32_t)(v >> (32 - S));
        if constexpr (S != 0 && W + 2 < NB) bits[W + 2] |= (uint32_t)(v >> (64 - S));
    }
    template <int K>
    __device__ static __forceinline__ void put_plane(uint32_t (&bits)[NB], const Plane& pl)
    {
        put<136 * K>(bits, pl.a);
        put<136 * K + 64>(bits, pl.b);
        put<136 * K + 128>(bits, (uint64_t)(pl.c & 255u));
    }
    __device__ __forceinline__ Plane pile_plane(int p) const
    {
        Plane pl{0, 0, 0};
        const int n = npile(p);
        for (int k = 0; k < n; k++) {
            const int d = pile(p, k), kind = d >> 6, t = d & 63, idx = t % 9;
            if (kind == V_CHOW) {
                if (idx == 0) {
                    pl.add(t + 1);
                    pl.add(t + 2);
                } else {
                    if (idx > 1) pl.add(t - 2);
                    pl.add(t - 1);
                }
                pl.add(t);
            } else {
                const int copies = kind == V_GONG ? 4 : 3;
                for (int q = 0; q < copies; q++) pl.add(t);
            }
        }
        return pl;
    }
    __device__ __forceinline__ void observe(int player, uint32_t (&bits)[NB]) const
    {
#pragma unroll
        for (int w = 0; w < NB; w++) bits[w] = 0u;
        {
            const int p = valid_act() ? current() : player, n = nh(p);   // Round.get_state: a claim shows the claimer's
            Plane pl{0, 0, 0};
            for (int i = 0; i < n; i++) pl.add(hand(p, i));
            put_plane<0>(bits, pl);
        }
        {
            Plane pl{0, 0, 0};
            const int n = nt();
#pragma unroll 1
            for (int i = 0; i < n; i++) pl.add(B(NTILES - 1 - i));
            put_plane<1>(bits, pl);
        }
        put_plane<2>(bits, pile_plane(0));
        put_plane<3>(bits, pile_plane(1));
        put_plane<4>(bits, pile_plane(2));
        put_plane<5>(bits, pile_plane(3));
    }

    // Judger.judge_chow's test on `claimer`'s hand for table tile `top` (a suit tile)
    __device__ __forceinline__ bool chow_ok(int claimer, int top) const
    {
        const int base = top / 9 * 9, idx = top - base, n = nh(claimer);
        uint32_t have = 0;   // the suit's values in the hand
        for (int i = 0; i < n; i++) {
            const int c = hand(claimer, i) - base;
            if (c >= 0 && c < 9) have |= 1u << c;
        }
        const uint32_t need = idx == 0 ? 6u : idx == 1 ? 0x101u : 3u << (idx - 2);   // hand_list[-1] is the 9
        return (have & need) == need;
    }

    template <class Rng>
    __device__ __forceinline__ void step(int a, Rng&)
    {
        const int cur = current();
        const uint64_t lg = legal();
        if (lg == 0) return;
        if (a < 0 || a >= A || !((lg >> a) & 1ull)) a = __builtin_ctzll(lg);   // this ABI's fallback: lowest legal id
        const int top = table_top();
        int changed = 0;   // seats whose hand or pile this step changes
        if (a == STAND) {
            // Judger.judge_chow: the player after last_player, suits only
            const int claimer = last_player() + 1;
            const bool offer = claimer < P && top < 27 && nt() > 0 && chow_ok(claimer, top);
            set_field(18, 3u, cur);
            if (offer) {
                set_field(22, 3u, V_CHOW);
                set_field(16, 3u, claimer);
            } else {
                const int next = (before_act() + 1) & 3;
                set_field(16, 3u, next);
                set_field(22, 3u, 0);
                draw(next);
                changed = 1 << next;
            }
        } else if (a == PONG || a == GONG) {   // Player.pong / gong: the table keeps the tile
            hand_remove(cur, top, a == PONG ? 3 : 4);
            pile_push(cur, a == PONG ? V_PONG : V_GONG, top);
            set_field(18, 3u, cur);
            set_field(22, 3u, 0);
            changed = 1 << cur;
        } else if (a == CHOW) {   // Player.chow: table.pop(), one copy of each hand tile of the shape
            const int idx = top % 9;
            if (nt() > 0) L(W_META) -= 1u << 8;
            if (idx == 0) {
                hand_remove(cur, top + 1, 1);
                hand_remove(cur, top + 2, 1);
            } else {
                if (idx > 1) hand_remove(cur, top - 2, 1);
                hand_remove(cur, top - 1, 1);
            }
            pile_push(cur, V_CHOW, top);
            set_field(18, 3u, cur);
            set_field(22, 3u, 0);
            changed = 1 << cur;
        } else {   // Player.play_card, then Judger.judge_pong_gong over players 0..3
            hand_remove(cur, a, 1);
            if (nd() + nt() < NTILES) {
                B(NTILES - 1 - nt()) = (uint8_t)a;
                L(W_META) += 1u << 8;
            }
            set_field(20, 3u, cur);
            set_field(18, 3u, cur);
            changed = 1 << cur;
            int claimer = -1, what = 0;
            for (int p = P - 1; p >= 0; p--) {
                if (p == cur) continue;
                const int k = hand_count(p, a);
                if (k == 2 || k == 3) {
                    claimer = p;
                    what = k == 3 ? V_GONG : V_PONG;
                }
            }
            if (claimer >= 0) {
                set_field(22, 3u, what);
                set_field(16, 3u, claimer);
            } else {
                const int next = (cur + 1) & 3;
                set_field(16, 3u, next);
                draw(next);
                changed |= 1 << next;
            }
        }
#pragma unroll 1
        for (int p = 0; p < P; p++)
            if ((changed >> p) & 1) judge(p);
        settle();
    }

    // Env.get_payoffs: judge_game's winner is the last winning player of its loop
    __device__ __forceinline__ void payoffs(float (&r)[P]) const
    {
        const int w = wins();
        const int winner = w ? 31 - __builtin_clz((unsigned)w) : -1;
#pragma unroll
        for (int p = 0; p < P; p++) r[p] = w == 0 ? 0.f : (p == winner ? 1.f : -1.f);
    }
};

}  // namespace cs
