// scout_rules_main.cpp -- Scout's rules (rlcard_amd/csrc/cs_scout_rules.h, the statements the kernels compile) as a
// stand-alone host program, built by tests/test_scout.py with -fsanitize=address,undefined. Reads commands from stdin,
// one per line, and answers one line each:
//   L n r0 .. r(n-1) t q0 .. q(t-1)   the ranks of a hand of n cards and of a table set of t cards (0..16 each) -> the
//                                     204-bit legal mask as four hex words, low word first, and the forced-scout flag;
//                                     built from the neighbour comparisons and slice by slice, which must agree
//   S n r0 .. r(n-1) t q0 .. q(t-1)   two card lists -> 1 if the first is stronger than the second, else 0, then kind
//                                     and rank of each
//   V n r0 .. r(n-1)                  -> 1 if the list is a valid slice
// Test infrastructure only.
#include <cstdio>
#include <cstring>
#include "../rlcard_amd/csrc/cs_scout_rules.h"

namespace sc = cs::scout;

static bool read_list(uint8_t (&r)[sc::HAND_MAX], int& n)
{
    memset(r, 0, sizeof(r));
    if (scanf("%d", &n) != 1 || n < 0 || n > sc::HAND_MAX) return false;
    for (int i = 0; i < n; i++) {
        int v;
        if (scanf("%d", &v) != 1 || v < 1 || v > 10) return false;
        r[i] = (uint8_t)v;
    }
    return true;
}

int main()
{
    char cmd[8];
    uint8_t a[sc::HAND_MAX], b[sc::HAND_MAX];
    int n, t;
    while (scanf("%7s", cmd) == 1) {
        if (cmd[0] == 'L') {
            if (!read_list(a, n) || !read_list(b, t)) return 2;
            const int ts = sc::strength(b, t);
            if (ts != sc::strength16(b, t)) return 3;
            uint64_t m[4], k[4];
            bool fm, fk;
            sc::legal_mask(a, n, t, ts, m, &fm, false);
            sc::legal_mask(a, n, t, ts, k, &fk, true);
            if (memcmp(m, k, sizeof(m)) != 0 || fm != fk) return 3;
            printf("%llx %llx %llx %llx %d\n", (unsigned long long)m[0], (unsigned long long)m[1],
                   (unsigned long long)m[2], (unsigned long long)m[3], (int)fm);
        } else if (cmd[0] == 'S') {
            if (!read_list(a, n) || !read_list(b, t)) return 2;
            const int sa = sc::strength(a, n), sb = sc::strength(b, t);
            if (sa != sc::strength16(a, n) || sb != sc::strength16(b, t)) return 3;
            printf("%d %d %d %d %d\n", (int)sc::stronger(n, sa, t, sb), sa >> 8, sa & 255, sb >> 8, sb & 255);
        } else if (cmd[0] == 'V') {
            if (!read_list(a, n)) return 2;
            printf("%d\n", (int)sc::is_valid_slice(a, n));
        } else {
            return 2;
        }
    }
    return 0;
}
