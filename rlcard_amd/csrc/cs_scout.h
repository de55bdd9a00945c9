// cs_scout.h -- Scout (4 players, hands of up to 16 ordered two-sided cards) as a lane-per-env lockstep state machine.
//
// Behaviour (reference file):
//   rlcard/games/scout/utils/utils.py   init_deck: the 45 cards (top, bottom), 1 <= top < bottom <= 10, top-major; the 204
//                                       action ids, slice validity and strength (cs_scout_rules.h)
//   rlcard/games/scout/dealer.py        ScoutDealer.__init__: np_random.shuffle(deck); deal_cards: deck.pop()
//   rlcard/games/scout/round.py         ScoutRound.__init__: a second np_random.shuffle, then one card at a time round
//                                       robin from seat 0 until the deck is empty (deal k, k = 0..44, is deck[44 - k] and
//                                       goes to the end of seat k % 4's hand: 12, 11, 11, 11 cards), then
//                                       np_random.randint(4) is the first player. proceed_round: the player's first move
//                                       locks his orientation unflipped. A play takes hand[s:e] as the new table set, the
//                                       old one vanishes and pays its length to the player, who becomes the owner; the
//                                       scout counter restarts. A scout pops the table's front or back card, flips it if
//                                       asked and inserts it into the hand; a forced scout (the player had no slice to
//                                       play) pays 1 to the owner; the counter goes up; an emptied table clears owner and
//                                       counter; counter 3 with an owner ends the game. Then the turn passes on, and a next
//                                       seat without a legal action ends the game too. get_legal_actions also sets
//                                       current_player_forced_scout, for a finished game as well: the legal actions and
//                                       the flag of a finished game are those of the seat the turn passed to.
//   rlcard/games/scout/judger.py        payoffs: score - len(hand) per seat
//   rlcard/envs/scout.py                the 688 observation values (below)
// The observation row, 688 bytes. Bytes 0..675 are the reference's values (all 0 or 1): four 16 x 10 one-hot planes (the
// asking seat's hand by top and by bottom, the table set by top and by bottom: byte 160 k + 10 i + v - 1), the hand's and
// the table's 16 occupancy bytes (640.., 656..), the owner one-hot (672..676, the last for no owner). The reference's
// eleven scalars follow as integers where it has fractions, in this row's own order (RAW_SPAN: bytes 676..687):
//   676 no owner (0 / 1) | 677 consecutive scouts (x / 3) | 678..681 the four hand counts (x / 16) | 682, 683 the asking
//   seat's points, low byte first (x / 16) | 684 table length (x / 16) | 685 forced scout (0 / 1) | 686, 687 the top of
//   the table's front and back card (x / 10)
// The reference has points in entry 682, the table length in 683 and its orientation flag in 684, which is always 0 (the
// env never calls set_orientation): the row spends that byte on the points' high byte. envs/scout.py maps a row to the
// reference's float32 vector. A score has no proven bound below 256 (a forced scout pays from a bank), so it is kept in
// 16 bits and saturates there.
// Packed state, 24 u32 words per env (word-major [24][N]), byte b in byte b % 4 of word b / 4:
//   words  0..15   the four hands, 16 card bytes each in hand order (top | bottom << 4), zero past the hand's length
//   words 16..19   the table set likewise
//   word  20       the four hand lengths, one byte each
//   word  21       table length (5 bits) | owner << 5 (3 bits, 4 none) | consecutive scouts << 8 (2 bits) | current
//                  player << 10 | orientation locked << 12 (one bit per seat) | forced scout << 16 | over << 31
//   words 22, 23   the scores, 16 bits each: seats 0 and 1, seats 2 and 3
// The lane's LDS scratch holds seven words more: the legal mask of the state (204 bits), rebuilt by whatever changes the
// state (reset, step, load), so legal() is seven LDS loads.
// Defined by this ABI where the reference raises: an illegal action id plays the lowest legal id. Words written through
// cs_set_env_state that hold no game (load) are a finished game.
#pragma once
#include "cs_device.h"
#include "cs_scout_rules.h"
#include "../../include/cardsim.h"

namespace cs {

struct Scout : GameDefaults {
    static constexpr int OBS = 688, A = 204, P = 4, LB = 26, WORDS = 24, ACTION_BYTES = 1;
    static constexpr int NBITS = 22;            // obs bitmap words (688 bits)
    static constexpr int RAW_SPAN_AT = 676, RAW_SPAN_LEN = 12;   // the scalars: raw bytes after the 0/1 bytes
    static constexpr int NB = NBITS + RAW_SPAN_LEN / 4;
    static constexpr bool RAW_OBS = false;
    static constexpr int MASK_WORDS = 7;                        // 204 bits
    static constexpr int SCRATCH_WORDS = WORDS + MASK_WORDS;    // the state and its legal mask live in the lane's LDS
    static constexpr int STAGE_W = 64, STAGE_PAD = 4, STAGE_R = 16, STAGE_RF = 32;
    static constexpr int RESTAGE_B = 4;
    static constexpr bool OBS_DIRECT = true;   // 688 B = 43 16-byte pieces per row, stored by the row's own lane
    // LDS per block: scratch 31 x 1 KB = 31 744 B + stage rows 17 472 B = 49 216 B (+ 20 B): three blocks per CU
    static constexpr int MIN_WAVES = CS_PROF_SCOUT_WAVES > 0 ? CS_PROF_SCOUT_WAVES : 2;   // (cs_prof.h: an A/B knob)
    static constexpr int EPW = 64;
    static constexpr bool RANDOM_ACTIONS = true;   // cs_policy_actions(CS_POLICY_RANDOM); the reference has no rule model
    static constexpr int HAND = 16, W_TABLE = 16, W_NH = 20, W_META = 21, W_SCORE = 22, W_MASK = WORDS;
    static constexpr int NO_OWNER = 4;
    static constexpr int STREAK = P - 1;   // consecutive scouts that end the game (num_players - 1 in the reference)
    static_assert(STREAK <= 3, "the scout counter is two bits");

    uint32_t* s;   // lane scratch: state word i at s[i * WAVE]

    __device__ __forceinline__ uint32_t& L(int i) const { return s[i * WAVE]; }
    static_assert(WAVE * 4 == 256, "state byte address");
    __device__ __forceinline__ uint8_t& B(int b) const { return ((uint8_t*)s)[b + 252 * (b >> 2)]; }
    __device__ __forceinline__ uint8_t& hand(int p, int i) const { return B(HAND * p + i); }
    __device__ __forceinline__ uint8_t& table(int i) const { return B(4 * W_TABLE + i); }

    __device__ __forceinline__ uint32_t meta() const { return L(W_META); }
    __device__ __forceinline__ int nh(int p) const { return (L(W_NH) >> (8 * p)) & 255; }
    __device__ __forceinline__ int tlen() const { return meta() & 31; }
    __device__ __forceinline__ int owner() const { return (meta() >> 5) & 7; }
    __device__ __forceinline__ int scouts() const { return (meta() >> 8) & 3; }
    __device__ __forceinline__ int current() const { return (meta() >> 10) & 3; }
    __device__ __forceinline__ int locked() const { return (meta() >> 12) & 15; }
    __device__ __forceinline__ bool forced() const { return (meta() >> 16) & 1; }
    __device__ __forceinline__ bool is_over() const { return meta() >> 31; }
    __device__ __forceinline__ int score(int p) const { return (L(W_SCORE + (p >> 1)) >> (16 * (p & 1))) & 0xFFFF; }
    __device__ __forceinline__ void set_meta(int shift, uint32_t mask, int v) const
    {
        L(W_META) = (meta() & ~(mask << shift)) | ((uint32_t)v & mask) << shift;
    }
    __device__ __forceinline__ void add_score(int p, int d) const   // (saturating: a score never wraps)
    {
        const int v = score(p) + d;
        const uint32_t nv = v > 0xFFFF ? 0xFFFFu : (uint32_t)v;
        uint32_t& w = L(W_SCORE + (p >> 1));
        w = (w & ~(0xFFFFu << (16 * (p & 1)))) | nv << (16 * (p & 1));
    }

    __device__ __forceinline__ void bind(uint32_t* lane_scratch, const GameParams&) { s = lane_scratch; }
    __device__ __forceinline__ void blank()
    {
#pragma unroll 1
        for (int w = 0; w < SCRATCH_WORDS; w++) L(w) = 0u;   // (no hand, no table: nothing is legal)
        L(W_META) = 1u << 31 | (uint32_t)NO_OWNER << 5 | 1u << 16;
    }

    // ---- get_legal_actions of the current player into the scratch's mask words, and the forced flag --------------------
    __device__ __forceinline__ void build_mask(uint64_t (&m)[4], bool& fs) const
    {
        const int cur = current(), n = nh(cur), tl = tlen();
        uint8_t r[HAND], t[HAND];
#pragma unroll
        for (int q = 0; q < HAND / 4; q++) {
            const uint32_t hw = L(4 * cur + q), tw = L(W_TABLE + q);
#pragma unroll
            for (int i = 0; i < 4; i++) {
                r[4 * q + i] = (uint8_t)((hw >> (8 * i)) & 15u);
                t[4 * q + i] = (uint8_t)((tw >> (8 * i)) & 15u);
            }
        }
        const int ts = scout::strength16(t, tl);
        scout::legal_mask(r, n, tl, ts, m, &fs, CS_PROF_SCOUT_MASK == 2);
    }
    __device__ __forceinline__ void refresh() const
    {
        uint64_t m[4];
        bool fs;
        build_mask(m, fs);
        L(W_MASK + 0) = (uint32_t)m[0];
        L(W_MASK + 1) = (uint32_t)(m[0] >> 32);
        L(W_MASK + 2) = (uint32_t)m[1];
        L(W_MASK + 3) = (uint32_t)(m[1] >> 32);
        L(W_MASK + 4) = (uint32_t)m[2];
        L(W_MASK + 5) = (uint32_t)(m[2] >> 32);
        L(W_MASK + 6) = (uint32_t)m[3];
        set_meta(16, 1u, fs);
    }
    __device__ __forceinline__ Legal256 legal() const
    {
        Legal256 m;
#if CS_PROF_SCOUT_MASK == 1
        bool fs;
        build_mask(m.w, fs);
#else
        m.w[0] = (uint64_t)L(W_MASK + 0) | (uint64_t)L(W_MASK + 1) << 32;
        m.w[1] = (uint64_t)L(W_MASK + 2) | (uint64_t)L(W_MASK + 3) << 32;
        m.w[2] = (uint64_t)L(W_MASK + 4) | (uint64_t)L(W_MASK + 5) << 32;
        m.w[3] = (uint64_t)L(W_MASK + 6);
#endif
        return m;
    }

    // the `len` cards of a list from byte `at`: each a card, none met before in `seen` (by card, whatever its
    // orientation), zero bytes past the length
    __device__ __forceinline__ bool cards_ok(int at, int len, uint64_t& seen) const
    {
        bool ok = true;
#pragma unroll 1
        for (int i = 0; i < HAND; i++) {
            const int c = B(at + i);
            if (i < len) {
                const bool card = scout::is_card(c);
                const uint64_t bit = 1ull << (card ? scout::card_index(c) : 63);
                ok = ok && card && !(seen & bit);
                seen |= bit;
            } else {
                ok = ok && c == 0;
            }
        }
        return ok;
    }
    __device__ __forceinline__ void load(const uint32_t* st, int64_t n, int64_t env)
    {
#pragma unroll 1
        for (int w = 0; w < WORDS; w++) L(w) = st[(int64_t)w * n + env];
        // words written by cs_set_env_state are the caller's: lengths of at most 16, an owner exactly when the table
        // holds a card, a scout counter below 3 while the game runs, every card byte a card and no card twice in either
        // orientation; anything else is a finished game. A finished game is still observed, so it is checked alike.
        const int tl = tlen(), ow = owner();
        bool ok = tl <= HAND && ow <= NO_OWNER && (ow < NO_OWNER) == (tl > 0) && (is_over() || scouts() < STREAK) &&
                  !((meta() >> 17) & 0x3FFFu);
        uint64_t seen = 0;
#pragma unroll 1
        for (int p = 0; p < P; p++) {
            const int k = nh(p);
            ok = ok && k <= HAND;
            ok = ok && cards_ok(HAND * p, k <= HAND ? k : 0, seen);
        }
        ok = ok && cards_ok(4 * W_TABLE, tl <= HAND ? tl : 0, seen);
        if (!ok) {
            blank();
            return;
        }
        refresh();   // (the mask and the forced flag are the state's own: never taken from the words)
        if (legal_empty(legal())) L(W_META) |= 1u << 31;   // (a game whose player has no action is over)
    }
    __device__ __forceinline__ void store(uint32_t* st, int64_t n, int64_t env) const
    {
#pragma unroll 1
        for (int w = 0; w < WORDS; w++) st[(int64_t)w * n + env] = L(w);
    }

    // ---- Game.init_game ---------------------------------------------------------------------------------------------
    template <class Rng>
    __device__ __forceinline__ void shuffle45(Rng& rng, int at) const
    {
        // np_random.shuffle: Fisher-Yates i = 44 .. 1, j = random_interval(i), swap
        rng.draw_intervals((uint32_t)scout::NCARDS - 1u, [&](uint32_t k, uint32_t j) {
            const uint32_t i = (uint32_t)scout::NCARDS - 1u - k;
            uint8_t& pi = B(at + (int)i);
            uint8_t& pj = B(at + (int)j);
            const uint8_t ci = pi, cj = pj;
            pi = cj;
            pj = ci;
        });
    }
    template <class Rng>
    __device__ __forceinline__ void reset(Rng& rng)
    {
        // the deck is built and shuffled in bytes 48..92 (seat 3's hand, the table and the counters, all written below)
        constexpr int DECK = 48;
        int k = 0;
#pragma unroll 1
        for (int top = 1; top <= 10; top++) {
#pragma unroll 1
            for (int bottom = top + 1; bottom <= 10; bottom++) B(DECK + k++) = (uint8_t)(top | bottom << 4);
        }
        shuffle45(rng, DECK);   // ScoutDealer.__init__
        shuffle45(rng, DECK);   // ScoutRound.__init__
        const int first = (int)rng.interval(3u);   // np_random.randint(4)
        // deal k is deck[44 - k], to seat k % 4: seat p's card i is deck[44 - 4 i - p]
#pragma unroll 1
        for (int p = 0; p < 3; p++) {
#pragma unroll 1
            for (int i = 0; i < HAND; i++) hand(p, i) = 4 * i + p < scout::NCARDS ? B(DECK + 44 - 4 * i - p) : (uint8_t)0;
        }
        uint32_t h3[3] = {0u, 0u, 0u};   // seat 3's eleven cards leave the deck's bytes before they are written over them
#pragma unroll
        for (int i = 0; i < 11; i++) h3[i / 4] |= (uint32_t)B(DECK + 41 - 4 * i) << (8 * (i % 4));
        L(12) = h3[0];
        L(13) = h3[1];
        L(14) = h3[2];
#pragma unroll 1
        for (int w = 15; w < SCRATCH_WORDS; w++) L(w) = 0u;
        L(W_NH) = 12u | 11u << 8 | 11u << 16 | 11u << 24;
        L(W_META) = (uint32_t)NO_OWNER << 5 | (uint32_t)first << 10;
        refresh();
    }

    // ---- envs/scout.py _build_observation_vector for seat p ----------------------------------------------------------
    template <int POS>
    __device__ static __forceinline__ void put10(uint32_t (&bits)[NB], uint32_t v)
    {
        constexpr int W = POS / 32, S = POS % 32;
        bits[W] |= v << S;
        if constexpr (S > 22) bits[W + 1] |= v >> (32 - S);
    }
    template <int PLANE, int I>
    __device__ static __forceinline__ void put_cards(uint32_t (&bits)[NB], const uint32_t (&w)[4])
    {
        if constexpr (I < HAND) {
            const uint32_t c = (w[I / 4] >> (8 * (I % 4))) & 255u;
            // a zero byte (no card) sets nothing: (1 << 0) >> 1
            put10<PLANE + 10 * I>(bits, (1u << (c & 15u)) >> 1);
            put10<PLANE + 160 + 10 * I>(bits, (1u << (c >> 4)) >> 1);
            put_cards<PLANE, I + 1>(bits, w);
        }
    }
    __device__ __forceinline__ void observe(int p, uint32_t (&bits)[NB]) const
    {
#pragma unroll
        for (int w = 0; w < NB; w++) bits[w] = 0u;
        p &= 3;
        uint32_t hw[4], tw[4];
#pragma unroll
        for (int q = 0; q < 4; q++) {
            hw[q] = L(4 * p + q);
            tw[q] = L(W_TABLE + q);
        }
        put_cards<0, 0>(bits, hw);
        put_cards<320, 0>(bits, tw);
        const uint32_t counts = L(W_NH);
        const int n = (counts >> (8 * p)) & 255, tl = tlen(), ow = owner();
        bits[20] = ((1u << n) - 1u) | ((1u << tl) - 1u) << 16;   // occupancy: bytes 640..655 and 656..671
        bits[21] = ow < NO_OWNER ? 1u << ow : 0u;                  // bytes 672..675
        const uint32_t pts = (uint32_t)score(p);
        const uint32_t front = tl > 0 ? tw[0] & 15u : 0u;
        const uint32_t back = tl > 0 ? (uint32_t)table(tl - 1) & 15u : 0u;
        bits[NBITS + 0] = (ow < NO_OWNER ? 0u : 1u) | (uint32_t)scouts() << 8 | counts << 16;
        bits[NBITS + 1] = counts >> 16 | pts << 16;
        bits[NBITS + 2] = (uint32_t)tl | (uint32_t)forced() << 8 | front << 16 | back << 24;
    }

    template <class Rng>
    __device__ __forceinline__ void step(int a, Rng&)
    {
        const Legal256 lg = legal();
        if (legal_empty(lg)) return;
        if (a < 0 || a >= A || !legal_has(lg, a)) a = legal_lowest(lg);   // this ABI's fallback: lowest legal id
        const int cur = current(), n = nh(cur), tl = tlen();
        const bool was_forced = forced();
        L(W_META) |= 1u << (12 + cur);   // the first move locks the orientation
        if (a < scout::NPLAY) {   // PlayAction: hand[s:e] becomes the table set
            int st = 0;
            while (st < HAND - 1 && a >= scout::play_base(st + 1)) st++;
            const int len = a - scout::play_base(st) + 1;
            if (tl > 0) add_score(cur, tl);
#pragma unroll 1
            for (int i = 0; i < HAND; i++) table(i) = i < len ? hand(cur, st + i) : (uint8_t)0;
#pragma unroll 1
            for (int i = st; i < n; i++) hand(cur, i) = i + len < n ? hand(cur, i + len) : (uint8_t)0;
            L(W_NH) -= (uint32_t)len << (8 * cur);
            set_meta(0, 31u, len);
            set_meta(5, 7u, cur);
            set_meta(8, 3u, 0);
        } else {   // ScoutAction: the table's front or back card into the hand
            const int k = a - scout::NPLAY, ins = k >> 2;
            const bool back = k & 2, flipped = k & 1;
            int c = back ? table(tl - 1) : table(0);
            if (!back) {
#pragma unroll 1
                for (int i = 0; i + 1 < tl; i++) table(i) = table(i + 1);
            }
            table(tl - 1) = 0;
            if (flipped) c = scout::flip(c);
#pragma unroll 1
            for (int i = n; i > ins; i--) hand(cur, i) = hand(cur, i - 1);
            hand(cur, ins) = (uint8_t)c;
            L(W_NH) += 1u << (8 * cur);
            set_meta(0, 31u, tl - 1);
            const int ow = owner();
            if (was_forced && ow < NO_OWNER) add_score(ow, 1);
            int sc = scouts() + 1;
            if (tl - 1 == 0) {
                set_meta(5, 7u, NO_OWNER);
                sc = 0;
            }
            set_meta(8, 3u, sc);
            if (sc == STREAK && owner() < NO_OWNER) L(W_META) |= 1u << 31;
        }
        set_meta(10, 3u, (cur + 1) & 3);
        refresh();
        if (legal_empty(legal())) L(W_META) |= 1u << 31;
    }

    __device__ __forceinline__ void payoffs(float (&r)[P]) const
    {
#pragma unroll
        for (int p = 0; p < P; p++) r[p] = (float)(score(p) - nh(p));
    }
};

}  // namespace cs
