// Prints what the strip-claim arithmetic of octree-tracer_amd/csrc/svo_sched.h says, for tests/test_claims_host.py to hold against
// itself.  One command per input line:
//   deal N           the no-schedule deal of N strips.  Per list one line "L l len s0 s1 ..." with the strips behind entries
//                    0 .. len + 16 (4294967295 = past the end), then one line "P l0 k0 l1 k1 ..." with every strip's place.
//   claims LEN B W l a list of LEN entries, l, in a grid of B workgroups of W waves.  "R reserved", "S rank counter ..." for every
//                    wave that starts on the list, then per counter j "C j e0 e1 ... | k e has ..." : the entries it hands out while
//                    counter_has_entry holds, and for the four answers after that the entry and the predicate.
#include <cstdio>
#include <cstring>

#include "svo_sched.h"

int main() {
    char cmd[16];
    while (scanf("%15s", cmd) == 1) {
        if (!strcmp(cmd, "deal")) {
            unsigned n;
            if (scanf("%u", &n) != 1) return 1;
            for (uint32_t l = 0; l < svo::kShards; l++) {
                const uint32_t len = svo::dealt_length(l, n);
                printf("L %u %u", l, len);
                for (uint32_t k = 0; k < len + 17u; k++) printf(" %u", svo::dealt_strip(l, k, n));
                printf("\n");
            }
            printf("P");
            for (uint32_t s = 0; s < n; s++) {
                uint32_t l, k;
                svo::dealt_place(s, l, k);
                printf(" %u %u", l, k);
            }
            printf("\n");
        } else if (!strcmp(cmd, "claims")) {
            unsigned len, blocks, waves, l;
            if (scanf("%u %u %u %u", &len, &blocks, &waves, &l) != 4) return 1;
            const uint32_t reserved = svo::waves_starting_on(l, blocks, waves);
            printf("R %u\nS", reserved);
            for (uint32_t b = 0; b < blocks; b++)
                for (uint32_t w = 0; w < waves; w++)
                    if (svo::starting_counter(b) / svo::kSubs == l) printf(" %u %u", svo::starting_rank(b, w, waves), svo::starting_counter(b) % svo::kSubs);
            printf("\n");
            for (uint32_t j = 0; j < svo::kSubs; j++) {
                printf("C %u", j);
                uint32_t k = 0;
                for (; svo::counter_has_entry(k, j, reserved, len); k++) printf(" %u", svo::claimed_entry(k, j, reserved));
                printf(" |");
                for (uint32_t t = 0; t < 4; t++, k++) printf(" %u %u %d", k, svo::claimed_entry(k, j, reserved), (int)svo::counter_has_entry(k, j, reserved, len));
                printf("\n");
            }
        } else {
            return 1;
        }
    }
}
