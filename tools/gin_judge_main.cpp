// gin_judge_main.cpp -- Gin Rummy's meld judge (rlcard_amd/csrc/cs_gin_melds.h, the statements the kernels compile)
// as a stand-alone host program, built by tests/test_gin_rummy.py with -fsanitize=address,undefined. Reads commands
// from stdin, one per line, and answers one line each:
//   H len c0 .. c10   an ordered hand -> "deadwood knock gin gin_card" (the masks in hex; knock / gin / gin_card are
//                     0 0 -1 unless len is 11)
//   S n h0 .. h(n-1)  small ints inserted into a fresh CPython set in this order -> the set's first element
//   P                 the 101 payoffs -deadwood / 100 as f32 bit patterns (hex), one line
// Test infrastructure only.
#include <cstdio>
#include <cstring>
#include "../rlcard_amd/csrc/cs_gin_melds.h"

int main()
{
    char cmd[8];
    while (scanf("%7s", cmd) == 1) {
        if (cmd[0] == 'H') {
            int len, c;
            uint32_t h[cs::gin::HAND_WORDS] = {0, 0, 0};
            if (scanf("%d", &len) != 1 || len < 0 || len > cs::gin::HAND_MAX) return 2;
            for (int k = 0; k < cs::gin::HAND_MAX; k++) {
                if (scanf("%d", &c) != 1) return 2;
                h[k >> 2] |= (uint32_t)(c & 255) << (8 * (k & 3));
            }
            uint64_t knock = 0, gin = 0;
            int card = -1;
            if (len == cs::gin::HAND_MAX) {
                cs::gin::going_out<true>(h, len, &knock, &gin);
                card = cs::gin::gin_card(h, len);
                uint64_t k2 = 0, g2 = 0;   // the kernels' form: the same knock set, and whether the gin set is empty
                cs::gin::going_out<false>(h, len, &k2, &g2);
                if (k2 != knock || (g2 != 0) != (gin != 0)) return 3;
            }
            printf("%d %llx %llx %d\n", cs::gin::best_deadwood(h, len), (unsigned long long)knock,
                   (unsigned long long)gin, card);
        } else if (cmd[0] == 'S') {
            int n, v;
            int16_t seq[cs::gin::HAND_MAX];
            if (scanf("%d", &n) != 1 || n < 0 || n > cs::gin::HAND_MAX) return 2;
            for (int k = 0; k < n; k++) {
                if (scanf("%d", &v) != 1) return 2;
                seq[k] = (int16_t)v;
            }
            printf("%d\n", cs::gin::set_first(seq, n));
        } else if (cmd[0] == 'P') {
            for (int d = 0; d <= 100; d++) {
                const float f = cs::gin::deadwood_payoff(d);
                uint32_t u;
                memcpy(&u, &f, 4);
                printf("%x%c", u, d == 100 ? '\n' : ' ');
            }
        } else {
            return 2;
        }
    }
    return 0;
}
