// cs_mahjong_hu.h -- Mahjong's win judge (rlcard/games/mahjong/judger.py judge_hu / cal_set / check_consecutive) as a
// plain function of (ordered hand bytes, hand size, pile count): no wave intrinsics, no LDS, so the game kernels
// (cs_mahjong.h), the test hook (cs_debug_mahjong_hu) and a host program compile the same statements.
//
// A hand is 16 bytes in four u32 words, tile i in byte i % 4 of word i / 4 (the layout of the state words); a tile is
// its action id: bamboo 0..8, characters 9..17, dots 18..26, dragons 27..29, winds 30..33.
//
// judge_hu: >= 4 piles win at once. Otherwise the distinct tiles of the hand are visited in the order of their first
// occurrence (a dict built from the hand list), those already in `used` skipped; each tile held exactly twice is taken
// out as the pair and cal_set counts the sets of the rest: every tile held 3 or 4 times is one set, then per suit a
// greedy run search over the sorted remaining values, which the reference walks with enumerate() while popping from the
// list it walks. The tiles of the runs found go into `used`, whether the try won or not, so the order of the hand
// decides which pairs are tried: it is observable. piles + sets >= 4 wins.
// After the pair and the triplets a suit holds 0..2 of each value, so the sorted list is a word of nine 4-bit counts:
// values[k] is the k-th value of that multiset, popping the first occurrence of a value lowers its count.
#pragma once
#include <stdint.h>

#if defined(__HIPCC__)
#define CS_MJ_HD __host__ __device__ __forceinline__
#else
#define CS_MJ_HD inline
#endif

namespace cs {
namespace mj {

constexpr int TILES = 34, HAND_MAX = 14;

CS_MJ_HD int hand_tile(const uint32_t (&h)[4], int i)
{
    const int k = i >> 2;
    const uint32_t w = k == 0 ? h[0] : k == 1 ? h[1] : k == 2 ? h[2] : h[3];
    return (int)((w >> (8 * (i & 3))) & 255u);
}
CS_MJ_HD int suit_of(int t) { return t >= 27 ? 3 : t >= 18 ? 2 : t >= 9 ? 1 : 0; }

// counts per tile: one u64 per suit (the honours are the fourth), 4 bits per value
struct Counts {
    uint64_t s[4];
};
CS_MJ_HD void count_add(Counts& c, int t)
{
    const int su = suit_of(t);
    const uint64_t one = 1ull << (4 * (t - 9 * su));
    for (int k = 0; k < 4; k++) c.s[k] += k == su ? one : 0ull;
}
CS_MJ_HD uint64_t count_word(const Counts& c, int su)
{
    return su == 0 ? c.s[0] : su == 1 ? c.s[1] : su == 2 ? c.s[2] : c.s[3];
}

// values[k] of a suit's sorted value list
CS_MJ_HD int nth_value(uint64_t w, int k)
{
    int r = 0;
    for (; r < 9; r++) {
        k -= (int)((w >> (4 * r)) & 15u);
        if (k < 0) break;
    }
    return r;
}

// cal_set's run search over one suit: the number of runs it takes; bit v of used_values set for the values taken.
// `for index, _ in enumerate(values)` over the list it pops from: the index goes up by one per round and the loop ends
// when it reaches the list's current length. test_case is values[0..2] at index 0, the last three at the last index,
// else the three around index; at index == len - 1 == 1 values[index - 2] wraps to the last value, a case of two equal
// values that check_consecutive never accepts.
CS_MJ_HD int suit_runs(uint64_t w, uint32_t& used_values)
{
    int len = 0;
    for (int r = 0; r < 9; r++) len += (int)((w >> (4 * r)) & 15u);
    int sets = 0;
    if (len <= 2) return 0;
    for (int index = 0; index < len; index++) {
        const int p0 = index == 0 ? 0 : (index == len - 1 ? index - 2 : index - 1);
        if (p0 < 0) continue;
        const int a = nth_value(w, p0), b = nth_value(w, p0 + 1), c = nth_value(w, p0 + 2);
        if (b == a + 1 && c == a + 2) {   // sorted(l) == range(min, max + 1)
            w -= 0x111ull << (4 * a);
            len -= 3;
            sets++;
            used_values |= 7u << a;
        }
    }
    return sets;
}

// cal_set on the counts of a hand without its pair: sets found; `used` gains the tiles of the runs (bit = tile id)
CS_MJ_HD int cal_set(Counts c, uint64_t& used)
{
    constexpr uint64_t LOW = 0x111111111ull;
    int sets = 0;
    for (int k = 0; k < 4; k++) {   // a tile held 3 or 4 times is one set (honours too)
        const uint64_t w = c.s[k], t3 = ((w & (w >> 1)) | (w >> 2)) & LOW;
        sets += __builtin_popcountll(t3);
        c.s[k] = w & ~(t3 * 15ull);
    }
    for (int k = 0; k < 3; k++) {
        uint32_t u = 0;
        sets += suit_runs(c.s[k], u);
        used |= (uint64_t)u << (9 * k);
    }
    return sets;
}

CS_MJ_HD bool judge_hu(const uint32_t (&h)[4], int n, int piles)
{
    if (piles >= 4) return true;
    if (n > HAND_MAX) n = HAND_MAX;
    // every set cal_set counts takes at least three tiles of the n - 2 left without the pair: a hand too short for
    // 4 - piles sets cannot win whatever its order (in play: every seat but the one that has just drawn)
    if (n < 2 + 3 * (4 - piles)) return false;
    Counts cnt{{0, 0, 0, 0}};
    for (int i = 0; i < n; i++) {
        const int t = hand_tile(h, i);
        if (t < TILES) count_add(cnt, t);
    }
    uint64_t seen = 0, used = 0;
    for (int i = 0; i < n; i++) {
        const int t = hand_tile(h, i);
        if (t >= TILES) continue;
        const uint64_t bit = 1ull << t;
        if ((seen | used) & bit) {
            seen |= bit;
            continue;
        }
        seen |= bit;
        const int su = suit_of(t), sh = 4 * (t - 9 * su);
        if (((count_word(cnt, su) >> sh) & 15u) != 2u) continue;
        Counts c = cnt;
        for (int k = 0; k < 4; k++) c.s[k] -= k == su ? 2ull << sh : 0ull;
        if (piles + cal_set(c, used) >= 4) return true;
    }
    return false;
}

}  // namespace mj
}  // namespace cs
