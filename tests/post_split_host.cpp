// post_split_host.cpp — pss_post_split.h with the host compiler alone (the header must not need HIP), built with -fsanitize=address,undefined
// and run as a program of its own by tests/test_post_split.py.  For every batch of 1 .. 6000 frame groups, every grid size, skew and
// early-zone size below it checks what k_spectrum_post relies on: the workgroups' ranges follow each other without a gap or an overlap from
// group 0 to the last group (every group is walked exactly once — also counted literally, group by group, for the small batches and a stride
// of the large ones), no range passes the batch, share_late >= 1, and the skew is the one asked for wherever the batch is large enough to
// allow it.  Prints "post_split_host: ok".
#include <algorithm>
#include <cstdio>
#include <vector>

#include "pss_post_split.h"

static int failures = 0;
#define CHECK(c)                                                                                                          \
    do {                                                                                                                  \
        if (!(c) && failures++ < 20) std::printf("FAILED %s (line %d): groups %ld n_wg %ld d %ld n_early %ld\n", #c, __LINE__, groups, n_wg, d, n_early); \
    } while (0)

int main()
{
    const long wgs[] = {1, 2, 255, 256, 257, 511, 512};
    const long ds[] = {0, 1, 7, 16, 31, 32, 1000};
    std::vector<int> seen(6000);
    long cases = 0;
    for (long groups = 1; groups <= 6000; groups++)
        for (long n_wg : wgs)
            for (long d : ds) {
                const long earlies[] = {0, 1, 256, n_wg};
                for (long n_early : earlies) {
                    const PssPostSplit s = pss_post_split_shares(groups, n_wg, n_early, d);
                    const long ne = n_early > n_wg ? n_wg : n_early;
                    CHECK(s.n_early == ne);
                    CHECK(s.share_late >= 1);
                    CHECK(s.share_early >= s.share_late && s.share_early - s.share_late <= d);
                    if (ne > 0 && ne < n_wg && n_wg + ne * d <= groups) CHECK(s.share_early - s.share_late == d);      // nothing to clamp
                    if (ne == 0 || ne == n_wg) CHECK(s.share_early == s.share_late);
                    if (groups >= n_wg) {
                        const long covered = ne * s.share_early + (n_wg - ne) * s.share_late;
                        CHECK(covered <= groups && groups - covered < n_wg);      // the remainder: at most one more group per workgroup
                    }
                    const bool literal = groups <= 600 || groups % 97 == 0;
                    if (literal) std::fill(seen.begin(), seen.begin() + groups, 0);
                    long at = 0;
                    for (long b = 0; b < n_wg; b++) {
                        long g0, g1;
                        pss_post_split_range(groups, n_wg, s.n_early, s.share_early, s.share_late, b, &g0, &g1);
                        CHECK(g0 == at && g0 <= g1 && g1 <= groups);
                        if (groups >= n_wg) CHECK(g1 - g0 >= (b < ne ? s.share_early : s.share_late) && g1 - g0 <= (b < ne ? s.share_early : s.share_late) + 1);
                        if (literal)
                            for (long g = g0; g < g1 && g < groups; g++) seen[g]++;
                        at = g1;
                    }
                    CHECK(at == groups);
                    if (literal)
                        for (long g = 0; g < groups; g++) CHECK(seen[g] == 1);
                    cases++;
                }
            }
    if (failures) return 1;
    std::printf("post_split_host: ok (%ld cases)\n", cases);
    return 0;
}
