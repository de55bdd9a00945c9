// cs_scout_rules.h -- Scout's slice validity, strength comparison and the 204-bit legal mask as plain host-and-device
// functions (no HIP types): the game kernel (cs_scout.h) and a host program (tools/scout_rules_main.cpp) compile the same
// statements.
//
// Restated (reference file):
//   rlcard/games/scout/utils/utils.py   get_action_list: ids 0..135 play-s-e for s = 0..15, e = s + 1..16 (s-major), then
//                                136 + 4 i + k for insertion point i = 0..16: k = 0 scout-front-i-normal, 1 front flipped,
//                                2 back normal, 3 back flipped. is_valid_scout_segment: all ranks equal (a group), or every
//                                step +1, or every step -1 (a run). segment_strength_rank: (0, rank) for one card, (2, rank)
//                                for a group, (1, the larger end rank) for a run, (0, the largest rank) for anything else.
//                                find_all_scout_segments: every valid slice of two or more cards, then every single card.
//   rlcard/games/scout/round.py         _is_stronger_set: longer wins; at equal length the higher (kind, rank) pair wins;
//                                anything beats an empty table. get_legal_actions: the slices stronger than the table,
//                                then, when the table is not empty and the hand holds fewer than 16 cards, the scouts for
//                                every insertion point 0..len(hand): front, and back when the table holds two or more.
// A card is one byte: top in the low nibble, bottom in the high one (1..10 each, different); its rank is its top.
// A prefix of a group is a group and a prefix of a run is a run, so the valid slices from start s are the lengths
// 1..maxlen(s), and maxlen(s) follows from the 15 comparisons of neighbours: one more than the count of consecutive set
// bits from bit s in the mask of equal pairs, of +1 pairs or of -1 pairs (at most one of the three has bit s set).
#pragma once
#include <stdint.h>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define CS_SCOUT_HD __host__ __device__ inline
#else
#define CS_SCOUT_HD inline
#endif

namespace cs {
namespace scout {

constexpr int HAND_MAX = 16, NPLAY = 136, NSCOUT = 68, NACT = NPLAY + NSCOUT, NCARDS = 45;
constexpr int SINGLE = 0, RUN = 1, GROUP = 2;

CS_SCOUT_HD int top_of(int c) { return c & 15; }
CS_SCOUT_HD int bottom_of(int c) { return (c >> 4) & 15; }
CS_SCOUT_HD int flip(int c) { return ((c & 15) << 4) | ((c >> 4) & 15); }
CS_SCOUT_HD bool is_card(int c)
{
    const int t = c & 15, b = (c >> 4) & 15;
    return c >= 0 && c < 256 && t >= 1 && t <= 10 && b >= 1 && b <= 10 && t != b;
}
// the card whatever its orientation: 0..44 in the deck's order (top-major over top < bottom)
CS_SCOUT_HD int card_index(int c)
{
    const int t = c & 15, b = (c >> 4) & 15;
    const int lo = t < b ? t : b, hi = t < b ? b : t;
    return (lo - 1) * 10 - (lo - 1) * lo / 2 + (hi - lo - 1);
}
// id of play-s-e
CS_SCOUT_HD constexpr int play_base(int s) { return 16 * s - s * (s - 1) / 2; }
CS_SCOUT_HD constexpr int play_id(int s, int e) { return play_base(s) + (e - s - 1); }
CS_SCOUT_HD constexpr int scout_id(int ins, bool front, bool flipped) { return NPLAY + 4 * ins + (front ? 0 : 2) + (flipped ? 1 : 0); }

// segment_strength_rank of n ranks as kind << 8 | rank (0 for no card: nothing to beat)
CS_SCOUT_HD int strength(const uint8_t* r, int n)
{
    if (n <= 0) return 0;
    if (n == 1) return SINGLE << 8 | r[0];
    bool grp = true, up = true, down = true;
    int hi = r[0];
    for (int i = 0; i + 1 < n; i++) {
        const int d = (int)r[i + 1] - (int)r[i];
        grp = grp && d == 0;
        up = up && d == 1;
        down = down && d == -1;
        hi = r[i + 1] > hi ? r[i + 1] : hi;
    }
    if (grp) return GROUP << 8 | r[0];
    if (up || down) return RUN << 8 | (r[0] > r[n - 1] ? r[0] : r[n - 1]);
    return SINGLE << 8 | hi;   // (no valid set: the reference's fallback)
}
// the same for the first n of 16 ranks with every index a constant once the loops are unrolled (the table set on the
// device: no rank array in scratch memory)
CS_SCOUT_HD int strength16(const uint8_t (&r)[HAND_MAX], int n)
{
    if (n <= 0) return 0;
    if (n == 1) return SINGLE << 8 | r[0];
    uint32_t eq = 0, up = 0, dn = 0;
    int hi = r[0];
#if defined(__HIP_DEVICE_COMPILE__)
#pragma unroll
#endif
    for (int i = 0; i < HAND_MAX - 1; i++) {
        const int d = (int)r[i + 1] - (int)r[i];
        const bool in = i + 1 < n;
        eq |= (uint32_t)(in && d == 0) << i;
        up |= (uint32_t)(in && d == 1) << i;
        dn |= (uint32_t)(in && d == -1) << i;
        hi = (in && r[i + 1] > hi) ? r[i + 1] : hi;
    }
    const uint32_t all = (1u << (n - 1)) - 1u;
    if (eq == all) return GROUP << 8 | r[0];
    if (up == all) return RUN << 8 | (r[0] + n - 1);
    if (dn == all) return RUN << 8 | r[0];
    return SINGLE << 8 | hi;
}
CS_SCOUT_HD bool is_valid_slice(const uint8_t* r, int n)
{
    if (n < 2) return true;
    const int s = strength(r, n) >> 8;
    return s == GROUP || s == RUN;
}
// _is_stronger_set on (length, strength) pairs
CS_SCOUT_HD bool stronger(int len, int str, int tlen, int tstr)
{
    if (tlen == 0) return true;
    if (len != tlen) return len > tlen;
    return str > tstr;   // kind first, then rank: the pair's order is the packed value's
}

// count of consecutive set bits of x from bit 0
CS_SCOUT_HD int ones_from0(uint32_t x)
{
    const uint32_t y = ~x;   // (bits 16.. of ~x are set: never zero)
    return __builtin_ctz(y);
}

// ids 0..135 of the slices of the hand's n ranks that beat the table (tlen cards of strength tstr) into m[0..2]:
// the 15 neighbour comparisons, then per start the contiguous bits of its lengths
CS_SCOUT_HD void play_mask(const uint8_t* r, int n, int tlen, int tstr, uint64_t (&m)[4])
{
    uint32_t eq = 0, up = 0, dn = 0;
#if defined(__HIP_DEVICE_COMPILE__)
#pragma unroll
#endif
    for (int i = 0; i < HAND_MAX - 1; i++) {
        const int d = (int)r[i + 1] - (int)r[i];
        const bool in = i + 1 < n;
        eq |= (uint32_t)(in && d == 0) << i;
        up |= (uint32_t)(in && d == 1) << i;
        dn |= (uint32_t)(in && d == -1) << i;
    }
    const int tk = tstr >> 8, tr = tstr & 255;
#if defined(__HIP_DEVICE_COMPILE__)
#pragma unroll
#endif
    for (int s = 0; s < HAND_MAX; s++) {
        const bool g = (eq >> s) & 1u, u = (up >> s) & 1u;
        const uint32_t x = (g ? eq : (u ? up : dn)) >> s;
        const int maxlen = 1 + ones_from0(x);
        uint32_t lens = (1u << maxlen) - 1u;              // bit l - 1: length l is a valid slice from s
        if (tlen > 0) {
            lens &= ~((1u << tlen) - 1u);                 // longer than the table
            if (tlen <= maxlen) {                         // as long as the table: kind, then rank
                const int kind = tlen == 1 ? SINGLE : (g ? GROUP : RUN);
                const int rank = (tlen > 1 && u) ? r[s] + tlen - 1 : r[s];   // a run's larger end
                if (kind > tk || (kind == tk && rank > tr)) lens |= 1u << (tlen - 1);
            }
        }
        if (s >= n) lens = 0u;
        const int pos = play_base(s), w = pos >> 6, sh = pos & 63;   // (constants once the loop is unrolled)
        m[w] |= (uint64_t)lens << sh;
        if (sh > 48) m[w + 1] |= (uint64_t)lens >> (64 - sh);
    }
}
// the same slice by slice, as the reference enumerates them (the check of play_mask; an A/B variant on the device)
CS_SCOUT_HD void play_mask_naive(const uint8_t* r, int n, int tlen, int tstr, uint64_t (&m)[4])
{
    for (int s = 0; s < n; s++) {
        for (int e = s + 1; e <= n; e++) {
            if (!is_valid_slice(r + s, e - s)) continue;
            if (!stronger(e - s, strength(r + s, e - s), tlen, tstr)) continue;
            const int id = play_id(s, e);
            m[0] |= id < 64 ? 1ull << (id & 63) : 0ull;
            m[1] |= (id >= 64 && id < 128) ? 1ull << (id & 63) : 0ull;
            m[2] |= id >= 128 ? 1ull << (id & 63) : 0ull;
        }
    }
}
// ids 136.. of the scouts: insertion points 0..n, front normal / flipped, back normal / flipped with two cards or more
CS_SCOUT_HD void scout_mask(int n, int tlen, uint64_t (&m)[4])
{
    if (tlen <= 0 || n >= HAND_MAX) return;
    const uint64_t pat = (tlen > 1 ? 0xFull : 0x3ull) * 0x1111111111111111ull;
    const int bits = 4 * (n + 1);   // at most 64
    const uint64_t s = bits >= 64 ? pat : pat & ((1ull << bits) - 1ull);
    m[2] |= s << (NPLAY - 128);
    m[3] |= s >> (64 - (NPLAY - 128));
}
// get_legal_actions as an id mask; *forced: no slice was kept (current_player_forced_scout)
CS_SCOUT_HD void legal_mask(const uint8_t* r, int n, int tlen, int tstr, uint64_t (&m)[4], bool* forced, bool naive = false)
{
    m[0] = m[1] = m[2] = m[3] = 0ull;
    if (naive) play_mask_naive(r, n, tlen, tstr, m);
    else play_mask(r, n, tlen, tstr, m);
    *forced = (m[0] | m[1] | m[2]) == 0ull;
    scout_mask(n, tlen, m);
}

}  // namespace scout
}  // namespace cs
