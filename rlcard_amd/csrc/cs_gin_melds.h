// cs_gin_melds.h -- Gin Rummy's meld judge as plain host-and-device functions (no HIP types): the game kernel
// (cs_gin_rummy.h), the test hook (cs_debug_gin_melds) and a host program compile the same statements.
//
// A card is its id = rank + 13 * suit (games/gin_rummy/utils/utils.py:36-39; ranks A 2 .. 9 T J Q K = 0..12, suits
// S H D C = 0..3); a hand is a 52-bit mask plus, where the reference's order is observable, its ordered byte list,
// packed four cards to a word (card i in byte i % 4 of word i / 4).
//
// Restated (reference file:line):
//   utils/melding.py:59-84    get_all_run_melds: the hand sorted by card id, every maximal run of three or more cards of
//                             one suit in rank order (ace low only), and per maximal run every slice [i, j) of three or
//                             more cards, i ascending, then j
//   utils/melding.py:85-106   get_all_set_melds: sorted(hand, key=card.rank) -- rank as a STRING, so the ranks come in
//                             the order 2..9, A, J, K, Q, T, and the sort is stable, so the cards of a rank keep the
//                             hand's order; per rank held three or four times the whole set, then for four of a kind
//                             the set without its first, second, third and fourth card
//   utils/melding.py:19-44    get_meld_clusters: all melds = runs + sets; every meld, every disjoint pair i < j, every
//                             disjoint triple i < j < k, in that nesting (cluster [i], then [i, j], then [i, j, k] ...)
//   player.py:27-52, 53-109   the player's memoised lists hold the same melds as SETS OF CARDS in another order (sets by
//                             rank id, then runs by suit); judge.get_legal_actions reads that one (judge.py:37), and
//                             only whether the gin set is empty and which cards can knock -- both order-free
//   utils/melding.py:45-58, utils/utils.py:44-59   best deadwood of 10 cards: the minimum over the clusters of the summed
//                             deadwood values outside the cluster (A 1, 2..9 face value, T J Q K 10); the plain sum
//                             with no meld
//   judge.py:105-141          _get_going_out_cards(hand of 11): per cluster, no deadwood -> the first card of the
//                             cluster's first meld of four or more cards gins; one deadwood card -> it gins; otherwise
//                             with count <= 10 + the largest value, every deadwood card whose removal leaves <= 10 knocks
//   round.py:116-131          gin: gin_cards[0] of list(set) -- the set filled in cluster order by
//                             judge.get_going_out_cards (judge.py:89-101: the FRESH clusters of melding.py, runs first),
//                             every meld a list(frozenset(cards)), Card.__hash__ = rank + 100 * suit
//                             (games/base.py:33-36) and CPython hashing a small int to itself: set_first below
// Walks in the reference's order: the meld list (build), the cluster loop of going_out where it takes a meld's first
// card, and gin_card. Order-free: best_deadwood, the knock mask, whether the gin mask is empty.
#pragma once
#include <stdint.h>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define CS_GIN_HD __host__ __device__ inline
#else
#define CS_GIN_HD inline
#endif

namespace cs {
namespace gin {

constexpr int HAND_MAX = 11, HAND_WORDS = 3;
// melds of at most 11 cards: a run of L cards has (L - 1)(L - 2) / 2 slices, 45 for all 11 cards in one run -- convex in
// L, so splitting the cards over runs and sets gives fewer (the runs of 7 + 4 cards give 18, two fours of a kind and a
// set of three 11); the builder stops at the bound whatever the input
constexpr int MELDS_MAX = 48;
constexpr uint64_t CARDS52 = (1ull << 52) - 1;

// a meld: bits 0..51 its cards, bits 52..59 their summed deadwood value
struct Melds {
    uint64_t m[MELDS_MAX];
    int n;
};

CS_GIN_HD int card_at(const uint32_t (&hw)[HAND_WORDS], int i)
{
    const uint32_t w = i < 4 ? hw[0] : (i < 8 ? hw[1] : hw[2]);
    return (int)((w >> (8 * (i & 3))) & 255u);
}
CS_GIN_HD int card_value(int card)
{
    const int r = card % 13;
    return r >= 9 ? 10 : r + 1;
}
CS_GIN_HD int ctz52(uint64_t x) { return __builtin_ctzll(x); }   // (x != 0 at every call)
CS_GIN_HD int popc52(uint64_t x) { return __builtin_popcountll(x); }
CS_GIN_HD int mask_value(uint64_t cards)
{
    int v = 0;
    while (cards) {
        v += card_value(ctz52(cards));
        cards &= cards - 1;
    }
    return v;
}
CS_GIN_HD uint64_t hand_mask(const uint32_t (&hw)[HAND_WORDS], int n)
{
    uint64_t m = 0;
    for (int i = 0; i < n && i < HAND_MAX; i++) {
        const int c = card_at(hw, i);
        if (c < 52) m |= 1ull << c;
    }
    return m;
}
CS_GIN_HD void meld_push(Melds& ms, uint64_t cards)
{
    if (ms.n < MELDS_MAX) ms.m[ms.n++] = cards | (uint64_t)mask_value(cards) << 52;
}

// melding.get_meld_clusters' all_melds of the hand: runs, then sets (see the header)
CS_GIN_HD void build(const uint32_t (&hw)[HAND_WORDS], int n, Melds& ms)
{
    ms.n = 0;
    const uint64_t hand = hand_mask(hw, n);
    for (int s = 0; s < 4; s++) {
        const uint32_t suit = (uint32_t)(hand >> (13 * s)) & 0x1FFFu;
        int a = 0;
        while (a < 13) {
            if (!((suit >> a) & 1u)) {
                a++;
                continue;
            }
            int b = a;
            while (b < 13 && ((suit >> b) & 1u)) b++;
            const int len = b - a;
            for (int i = 0; i + 3 <= len; i++)
                for (int j = i + 3; j <= len; j++)
                    meld_push(ms, (((1ull << (j - i)) - 1ull) << (a + i)) << (13 * s));
            a = b;
        }
    }
    for (int k = 0; k < 13; k++) {
        // card.rank as a string: '2'..'9' (rank ids 1..8), 'A' (0), 'J' (10), 'K' (12), 'Q' (11), 'T' (9)
        const int r = k < 8 ? k + 1 : (k == 8 ? 0 : (k == 9 ? 10 : (k == 10 ? 12 : (k == 11 ? 11 : 9))));
        const uint64_t all = (hand >> r) & 0x0000008004002001ull;   // bits 0, 13, 26, 39
        const int cnt = popc52(all);
        if (cnt < 3) continue;
        const uint64_t full = all << r;
        meld_push(ms, full);
        if (cnt == 4) {
            for (int i = 0; i < n && i < HAND_MAX; i++) {   // without its first, second, ... card in hand order
                const int c = card_at(hw, i);
                if (c < 52 && c % 13 == r) meld_push(ms, full & ~(1ull << c));
            }
        }
    }
}

CS_GIN_HD uint64_t meld_cards(uint64_t m) { return m & CARDS52; }
CS_GIN_HD int meld_value(uint64_t m) { return (int)(m >> 52); }

// the largest summed value of up to three disjoint melds none of which holds a card of `without`
CS_GIN_HD int best_melded(const Melds& ms, uint64_t without)
{
    int best = 0;
    for (int i = 0; i < ms.n; i++) {
        const uint64_t a = meld_cards(ms.m[i]);
        if (a & without) continue;
        const int va = meld_value(ms.m[i]);
        best = va > best ? va : best;
        for (int j = i + 1; j < ms.n; j++) {
            const uint64_t b = meld_cards(ms.m[j]);
            if (b & (a | without)) continue;
            const int vb = va + meld_value(ms.m[j]);
            best = vb > best ? vb : best;
            for (int k = j + 1; k < ms.n; k++) {
                const uint64_t c = meld_cards(ms.m[k]);
                if (c & (a | b | without)) continue;
                const int vc = vb + meld_value(ms.m[k]);
                best = vc > best ? vc : best;
            }
        }
    }
    return best;
}

// utils.get_deadwood_count of the best cluster of a hand (10 cards in the reference; any count here)
CS_GIN_HD int best_deadwood(const uint32_t (&hw)[HAND_WORDS], int n)
{
    Melds ms;
    build(hw, n, ms);
    return mask_value(hand_mask(hw, n)) - best_melded(ms, 0ull);
}

// "first element, in iteration order, of a CPython set that received these small non-negative ints in this order"
// (Objects/setobject.c set_add_entry / set_insert_clean / set_table_resize: a table of 8 slots, slot = hash & mask, up
// to LINEAR_PROBES = 9 further slots while slot + 9 <= mask, then slot = (5 slot + 1 + (perturb >>= 5)) & mask; after
// an insert that makes fill * 5 >= mask * 3 the table is rebuilt at the first power of two above 4 * used, its entries
// reinserted in slot order). n <= 11 distinct values: one growth, from 8 slots to 32, at the fifth insert.
CS_GIN_HD void set_put(int16_t (&tab)[32], int mask, int h)
{
    int i = h & mask;
    uint32_t perturb = (uint32_t)h;
    for (int guard = 0; guard < 64; guard++) {
        const int probes = i + 9 <= mask ? 9 : 0;
        for (int e = i; e <= i + probes; e++) {
            if (tab[e] < 0) {
                tab[e] = (int16_t)h;
                return;
            }
        }
        perturb >>= 5;
        i = (int)(((uint32_t)i * 5u + 1u + perturb) & (uint32_t)mask);
    }
}
CS_GIN_HD int set_first(const int16_t* seq, int n)
{
    int16_t tab[32];
    for (int i = 0; i < 32; i++) tab[i] = -1;
    int mask = 7, fill = 0;
    for (int t = 0; t < n && t < HAND_MAX; t++) {
        set_put(tab, mask, seq[t]);
        fill++;
        if (fill * 5 >= mask * 3 && mask < 31) {
            int size = 8;
            while (size <= 4 * fill && size < 32) size <<= 1;
            int16_t old[8];
            for (int i = 0; i < 8; i++) {
                old[i] = tab[i];
                tab[i] = -1;
            }
            mask = size - 1;
            for (int i = 0; i < 8; i++)
                if (old[i] >= 0) set_put(tab, mask, old[i]);
        }
    }
    for (int i = 0; i <= mask; i++)
        if (tab[i] >= 0) return tab[i];
    return -1;
}
CS_GIN_HD int card_hash(int card) { return card % 13 + 100 * (card / 13); }
CS_GIN_HD int hash_card(int h) { return h % 100 + 13 * (h / 100); }

// list(frozenset(meld))[0] of a meld as melding.py builds its card list: a run in card-id order, a set in hand order
CS_GIN_HD int meld_first(uint64_t cards, const uint32_t (&hw)[HAND_WORDS], int n)
{
    int16_t seq[HAND_MAX];
    int k = 0;
    const int lo = ctz52(cards);
    const bool run = ((cards >> lo) & 3ull) == 3ull && lo % 13 != 12;   // a set's next card is 13 ids further
    if (run) {
        for (uint64_t c = cards; c && k < HAND_MAX; c &= c - 1) seq[k++] = (int16_t)card_hash(ctz52(c));
    } else {
        for (int i = 0; i < n && i < HAND_MAX; i++) {
            const int c = card_at(hw, i);
            if (c < 52 && ((cards >> c) & 1ull) && k < HAND_MAX) seq[k++] = (int16_t)card_hash(c);
        }
    }
    return hash_card(set_first(seq, k));
}

// judge._get_going_out_cards over the fresh clusters. EXACT: the gin mask holds the reference's cards (a cluster
// without deadwood gives the first card of its first meld of four or more cards); otherwise such a cluster sets
// bit 63 of *gin_out, which is all the legal set needs. order != nullptr: the distinct gin cards' hashes in the
// order the reference's set receives them (*norder of them).
template <bool EXACT>
CS_GIN_HD void going_out(const uint32_t (&hw)[HAND_WORDS], int n, uint64_t* knock_out, uint64_t* gin_out,
                         int16_t* order = nullptr, int* norder = nullptr)
{
    Melds ms;
    build(hw, n, ms);
    const uint64_t hand = hand_mask(hw, n);
    const int total = mask_value(hand);
    uint64_t knock = 0, gin = 0;
    int no = 0;
    auto cluster = [&](uint64_t a, uint64_t b, uint64_t c, int melded) {
        const uint64_t dead = hand & ~(meld_cards(a) | meld_cards(b) | meld_cards(c));
        const int nd = popc52(dead);
        uint64_t g = 0;
        if (nd == 0) {
            if constexpr (EXACT) {
                const uint64_t first = popc52(meld_cards(a)) >= 4 ? a : (popc52(meld_cards(b)) >= 4 ? b : c);
                if (popc52(meld_cards(first)) >= 4) g = 1ull << meld_first(meld_cards(first), hw, n);
            } else {
                gin |= 1ull << 63;
            }
        } else if (nd == 1) {
            g = dead;
        } else {
            const int count = total - melded;
            if (count > 20) return;   // (no card is worth more than 10: nothing passes the two tests below)
            int maxv = 0;
            for (uint64_t d = dead; d; d &= d - 1) {
                const int v = card_value(ctz52(d));
                maxv = v > maxv ? v : maxv;
            }
            if (count <= 10 + maxv) {
                for (uint64_t d = dead; d; d &= d - 1) {
                    const int cd = ctz52(d);
                    if (count - card_value(cd) <= 10) knock |= 1ull << cd;
                }
            }
        }
        if (g && !(gin & g)) {
            if (order && no < HAND_MAX) order[no++] = (int16_t)card_hash(ctz52(g));
        }
        gin |= g;
    };
    for (int i = 0; i < ms.n; i++) {
        const uint64_t a = ms.m[i];
        cluster(a, 0ull, 0ull, meld_value(a));
        for (int j = i + 1; j < ms.n; j++) {
            const uint64_t b = ms.m[j];
            if (meld_cards(b) & meld_cards(a)) continue;
            cluster(a, b, 0ull, meld_value(a) + meld_value(b));
            for (int k = j + 1; k < ms.n; k++) {
                const uint64_t c = ms.m[k];
                if (meld_cards(c) & (meld_cards(a) | meld_cards(b))) continue;
                cluster(a, b, c, meld_value(a) + meld_value(b) + meld_value(c));
            }
        }
    }
    *knock_out = knock;
    *gin_out = gin;
    if (norder) *norder = no;
}

// round.gin's card: gin_cards[0] (-1 with an empty gin set)
CS_GIN_HD int gin_card(const uint32_t (&hw)[HAND_WORDS], int n)
{
    uint64_t knock, gin;
    int16_t order[HAND_MAX];
    int no = 0;
    going_out<true>(hw, n, &knock, &gin, order, &no);
    return no > 0 ? hash_card(set_first(order, no)) : -1;
}

// get_payoff_gin_rummy_v1's -deadwood_count / 100 (utils/scorers.py:68, a float64 quotient) as the engine's f32: the
// float64 division, then one rounding to f32 (the count is negated as an integer: no deadwood pays +0.0)
CS_GIN_HD float deadwood_payoff(int deadwood) { return (float)((double)(-deadwood) / 100.0); }

}  // namespace gin
}  // namespace cs
