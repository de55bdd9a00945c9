// cs_bridge_rules.h -- Bridge's call legality, trick winner and payoff as plain host-and-device functions (no HIP
// types): the game kernel (cs_bridge.h) and a host program (tools/bridge_rules_main.cpp) compile the same statements.
//
// Restated (reference file):
//   rlcard/games/bridge/utils/action_event.py   ids: 0 no_bid (never legal), 1..35 bids = 1 + 5 * (amount - 1) + strain
//                                (strain C D H S NT = 0..4), 36 pass, 37 dbl, 38 rdbl, 39 + card plays the card
//   rlcard/games/bridge/utils/bridge_card.py    card id = 13 * suit + rank, suits C D H S, ranks 2..A
//   rlcard/games/bridge/judger.py               get_legal_actions: pass, every bid above the last one, dbl when the last
//                                bid is the opponents' and no dbl or rdbl has followed it, rdbl when the standing dbl is
//                                the opponents'; a card of the led suit if the hand has one while the trick holds one to
//                                three cards, else any card of the hand
//   rlcard/games/bridge/round.py                play_card: a card of the winning card's suit wins by higher id, otherwise
//                                a trump takes over, NT has no trump
//   rlcard/envs/bridge.py                       DefaultBridgePayoffDelegate: the side of the last bidder gets bid + 6 + 2
//                                if it took at least bid + 6 tricks, otherwise won - (bid + 6); the other side its tricks
// A dbl is only ever legal for the opponents of the last bidder, so the side of a standing dbl is the other side of the
// last bidder and the doubling cube alone says who may rdbl.
#pragma once
#include <stdint.h>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define CS_BRIDGE_HD __host__ __device__ inline
#else
#define CS_BRIDGE_HD inline
#endif

namespace cs {
namespace bridge {

constexpr int NO_BID = 0, FIRST_BID = 1, LAST_BID = 35, PASS = 36, DBL = 37, RDBL = 38, PLAY = 39, NCARDS = 52;
constexpr int NT = 4;                               // strain of a bid: (id - 1) % 5, suits 0..3 as the cards' suits
constexpr int CUBE_1 = 0, CUBE_DBL = 1, CUBE_RDBL = 2;   // the doubling cube 1, 2, 4 as a code
constexpr uint64_t CARDS52 = (1ull << 52) - 1;

CS_BRIDGE_HD int bid_amount(int bid) { return 1 + (bid - FIRST_BID) / 5; }
CS_BRIDGE_HD int bid_strain(int bid) { return (bid - FIRST_BID) % 5; }

// the legal calls of seat `cur` as an id mask (bits 1..38); last_bid 0: no bid yet
CS_BRIDGE_HD uint64_t legal_calls(int last_bid, int last_bidder, int cube, int cur)
{
    uint64_t m = 1ull << PASS;
    if (last_bid < NO_BID || last_bid > LAST_BID) last_bid = LAST_BID;
    m |= ((1ull << (LAST_BID + 1)) - 1) & ~((1ull << (last_bid + 1)) - 1);
    if (last_bid > NO_BID) {
        const bool theirs = ((last_bidder ^ cur) & 1) != 0;
        if (theirs && cube == CUBE_1) m |= 1ull << DBL;
        if (!theirs && cube == CUBE_DBL) m |= 1ull << RDBL;
    }
    return m;
}

// the playable cards of a hand (card mask); led: the first card of a trick of one to three cards, < 0 otherwise
CS_BRIDGE_HD uint64_t legal_cards(uint64_t hand, int led)
{
    hand &= CARDS52;
    if (led < 0 || led >= NCARDS) return hand;
    const uint64_t suit = hand & (0x1FFFull << (13 * (led / 13)));
    return suit ? suit : hand;
}

// which of a trick's four cards (in play order) wins; strain 0..3 trumps, NT none
CS_BRIDGE_HD int trick_winner(int c0, int c1, int c2, int c3, int strain)
{
    const int c[4] = {c0, c1, c2, c3};
    int win = 0, wc = c0;
    for (int i = 1; i < 4; i++) {
        if (c[i] / 13 == wc / 13) {
            if (c[i] > wc) {
                wc = c[i];
                win = i;
            }
        } else if (strain != NT && c[i] / 13 == strain) {
            wc = c[i];
            win = i;
        }
    }
    return win;
}

// the four payoffs; won[s]: tricks of side s (seat % 2); last_bid 0 (passed out): zeros
CS_BRIDGE_HD void payoffs(int last_bid, int last_bidder, int won0, int won1, int (&out)[4])
{
    int decl = 0, def = 0;
    const int side = last_bidder & 1;
    if (last_bid >= FIRST_BID && last_bid <= LAST_BID) {
        const int need = bid_amount(last_bid) + 6;
        const int dw = side ? won1 : won0;
        decl = need <= dw ? need + 2 : dw - need;
        def = side ? won0 : won1;
        for (int p = 0; p < 4; p++) out[p] = (p & 1) == side ? decl : def;
    } else {
        for (int p = 0; p < 4; p++) out[p] = 0;
    }
}

}  // namespace bridge
}  // namespace cs
