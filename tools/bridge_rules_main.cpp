// bridge_rules_main.cpp -- Bridge's rules (rlcard_amd/csrc/cs_bridge_rules.h, the statements the kernels compile) as a
// stand-alone host program, built by tests/test_bridge.py with -fsanitize=address,undefined. Reads commands from stdin,
// one per line, and answers one line each:
//   C last_bid last_bidder cube cur   -> the legal calls as an id mask (hex)
//   K hand led                        hand as a card mask (hex), led card or -1 -> the playable cards (hex)
//   T c0 c1 c2 c3 strain              a trick in play order -> the place (0..3) of the winning card
//   P last_bid last_bidder won0 won1  -> the four payoffs
//   E s0 s1 s2 strain                 every ordered trick of four different cards of the suits s0, s1, s2 (the cards in
//                                     ascending id order, the first card slowest) -> the winners' places as one string
// Test infrastructure only.
#include <cstdio>
#include "../rlcard_amd/csrc/cs_bridge_rules.h"

int main()
{
    char cmd[8];
    while (scanf("%7s", cmd) == 1) {
        if (cmd[0] == 'C') {
            int b, who, cube, cur;
            if (scanf("%d %d %d %d", &b, &who, &cube, &cur) != 4) return 2;
            printf("%llx\n", (unsigned long long)cs::bridge::legal_calls(b, who, cube, cur));
        } else if (cmd[0] == 'K') {
            unsigned long long hand;
            int led;
            if (scanf("%llx %d", &hand, &led) != 2) return 2;
            printf("%llx\n", (unsigned long long)cs::bridge::legal_cards(hand, led));
        } else if (cmd[0] == 'T') {
            int c[4], strain;
            if (scanf("%d %d %d %d %d", &c[0], &c[1], &c[2], &c[3], &strain) != 5) return 2;
            for (int i = 0; i < 4; i++) {
                if (c[i] < 0 || c[i] >= cs::bridge::NCARDS) return 2;
            }
            printf("%d\n", cs::bridge::trick_winner(c[0], c[1], c[2], c[3], strain));
        } else if (cmd[0] == 'E') {
            int s[3], strain, pool[39], n = 0;
            if (scanf("%d %d %d %d", &s[0], &s[1], &s[2], &strain) != 4) return 2;
            for (int c = 0; c < cs::bridge::NCARDS; c++) {
                if (c / 13 == s[0] || c / 13 == s[1] || c / 13 == s[2]) pool[n++] = c;
            }
            for (int a = 0; a < n; a++)
                for (int b = 0; b < n; b++)
                    for (int c = 0; c < n; c++)
                        for (int d = 0; d < n; d++) {
                            if (a == b || a == c || a == d || b == c || b == d || c == d) continue;
                            putchar('0' + cs::bridge::trick_winner(pool[a], pool[b], pool[c], pool[d], strain));
                        }
            putchar('\n');
        } else if (cmd[0] == 'P') {
            int b, who, w0, w1, out[4];
            if (scanf("%d %d %d %d", &b, &who, &w0, &w1) != 4) return 2;
            cs::bridge::payoffs(b, who, w0, w1, out);
            printf("%d %d %d %d\n", out[0], out[1], out[2], out[3]);
        } else {
            return 2;
        }
    }
    return 0;
}
