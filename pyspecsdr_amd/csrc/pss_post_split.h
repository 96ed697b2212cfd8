// pss_post_split.h — how k_spectrum_post's one-round grid divides the frame groups of a batch (pss_spec_post.h, pss_fft.hip).
// Every workgroup owns ONE contiguous range of groups, decided before the launch: the first n_early workgroups take share_early groups each,
// the others share_late, and what the shares leave over goes, one group each, to the LAST workgroups.  Beside a resident backward pass
// (k_nfm_bwd) only one workgroup per CU starts at once — the early ones, which therefore get the larger share; everywhere else the two
// shares are equal.  Plain C++ and nothing from HIP in here: the host compiles the same two functions and a test walks them exhaustively.
#pragma once

#if defined(__HIPCC__)
#define PSS_SPLIT_HD __host__ __device__
#else
#define PSS_SPLIT_HD
#endif

struct PssPostSplit {
    long n_early;       // workgroups 0 .. n_early - 1 take share_early groups each
    long share_early;
    long share_late;    // >= 1
};

// The shares of n_wg workgroups (>= 1) over `groups` groups (>= 1) with share_early - share_late = d where the batch allows it: d is cut
// back until share_late >= 1, and to 0 where there is no early or no late workgroup.  groups < n_wg: one group each, the last
// workgroups' ranges are empty.
PSS_SPLIT_HD inline PssPostSplit pss_post_split_shares(long groups, long n_wg, long n_early, long d)
{
    PssPostSplit s;
    s.n_early = n_early < 0 ? 0 : (n_early > n_wg ? n_wg : n_early);
    if (d < 0 || s.n_early == 0 || s.n_early == n_wg) d = 0;
    if (groups < n_wg) {
        s.share_early = s.share_late = 1;
        return s;
    }
    if (d > 0 && n_wg + s.n_early * d > groups) d = (groups - n_wg) / s.n_early;     // share_late would fall below 1
    s.share_late = (groups - s.n_early * d) / n_wg;
    s.share_early = s.share_late + d;
    return s;
}

// The range [*begin, *end) of workgroup b of n_wg: its share, one more group for each of the last `left` workgroups (left = what the shares
// do not cover, < n_wg for the shares above), cut at `groups`.
PSS_SPLIT_HD inline void pss_post_split_range(long groups, long n_wg, long n_early, long share_early, long share_late, long b, long *begin, long *end)
{
    const long covered = n_early * share_early + (n_wg - n_early) * share_late;
    const long left = groups > covered ? groups - covered : 0;
    const long first_extra = n_wg - left;                     // workgroups first_extra .. n_wg - 1 take one more
    long g0 = b < n_early ? b * share_early : n_early * share_early + (b - n_early) * share_late;
    long len = b < n_early ? share_early : share_late;
    if (b > first_extra) g0 += b - first_extra;
    if (b >= first_extra) len += 1;
    long g1 = g0 + len;
    if (g0 > groups) g0 = groups;
    if (g1 > groups) g1 = groups;
    *begin = g0;
    *end = g1;
}
