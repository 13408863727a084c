// slab_plan.h -- the integer bookkeeping of a slab partition (slab.h): the offsets by owner, the halo offsets of a rank and the piece offsets of an
// all-to-all-v, from the count table the partition kernels leave.  Plain C++ (no HIP): tests/cpu/slab_plan_check.cpp includes this header alone; both
// slab loops (kcg.hip: kcg_slab_loop, xtb_slab.inc: xtb_cg_slab) and their emulated exchanges (slab.h) call the same functions.
#pragma once
#include <stddef.h>

#define XS_MAXR 32                                   // ranks (owner masks are 32 bit)
#define XS_BINS 4096                                 // histogram bins of the lateral coordinate
// the int buffer of the partition kernels: hist[XS_BINS] | cuts[XS_MAXR + 2] | tab[XS_MAXR * (XS_MAXR + 2)]
#define XS_CUTS_AT XS_BINS
#define XS_TAB_AT (XS_BINS + XS_MAXR + 2)
#define XS_TAB_MAX (XS_MAXR * (XS_MAXR + 2))
inline size_t slab_tab_bytes() { return (size_t)(XS_TAB_AT + XS_TAB_MAX) * sizeof(int); }
inline size_t slab_tab_ints(int nr) { return (size_t)nr * (nr + 2); }      // the count table of nr ranks: nown[nr] | nmark[nr] | hal[nr * nr]

// The partition as the host sees it: the downloaded count table and the offsets by owner.
struct SlabPlan {
    int nr = 0, maxown = 0;                          // ranks; rows of the largest slab
    int tab[XS_TAB_MAX];                             // nown | nmark | hal, as k_slab_count wrote it
    int rowoff[XS_MAXR + 1];                         // distributed rows of owner r: rows_by_owner[rowoff[r] ... rowoff[r + 1])
    int markoff[XS_MAXR + 1];                        // marked rows of owner r (X: its S rows)
    const int *nown() const { return tab; }
    const int *nmark() const { return tab + nr; }
    int hal(int s, int d) const { return tab[2 * nr + s * nr + d]; }      // rows of s that d reads
    bool covers(int rows, int marked) const { return rowoff[nr] == rows && markoff[nr] == marked; }      // the slabs add up to the expected rows
    SlabPlan(const int *htab, int nr_) : nr(nr_)
    {
        for (size_t i = 0; i < slab_tab_ints(nr); ++i) tab[i] = htab[i];
        rowoff[0] = markoff[0] = 0;
        for (int r = 0; r < nr; ++r) { rowoff[r + 1] = rowoff[r] + tab[r]; markoff[r + 1] = markoff[r] + tab[nr + r]; if (tab[r] > maxown) maxown = tab[r]; }
    }
};
// halo lists of rank v: what it sends to d at hsend[hsoff[d] ...), what it receives from s at hrecv[hroff[s] ...); v itself takes no room; the
// totals are hsoff[nr] and hroff[nr]
struct SlabHalo {
    int hsoff[XS_MAXR + 1], hroff[XS_MAXR + 1];
    SlabHalo(const SlabPlan &P, int v)
    {
        hsoff[0] = hroff[0] = 0;
        for (int r = 0; r < P.nr; ++r) { hsoff[r + 1] = hsoff[r] + (r == v ? 0 : P.hal(v, r)); hroff[r + 1] = hroff[r] + (r == v ? 0 : P.hal(r, v)); }
    }
};
// All-to-all-v with the count table cnt[a * nr + d] (doubles a sends to d): the pieces lie in destination order in a's send buffer and in source
// order in d's receive buffer.  Where piece a -> d starts in either; d = nr (a = nr) gives the total a sends (d receives).
inline long long slab_send_off(const long long *cnt, int nr, int a, int d) { long long o = 0; for (int d2 = 0; d2 < d; ++d2) o += cnt[(size_t)a * nr + d2]; return o; }
inline long long slab_recv_off(const long long *cnt, int nr, int a, int d) { long long o = 0; for (int a2 = 0; a2 < a; ++a2) o += cnt[(size_t)a2 * nr + d]; return o; }
// doubles a rank receives from the OTHER ranks, largest over the ranks
inline long long slab_recv_max(const long long *cnt, int nr)
{
    long long mx = 0;
    for (int d = 0; d < nr; ++d) { const long long t = slab_recv_off(cnt, nr, nr, d) - cnt[(size_t)d * nr + d]; if (t > mx) mx = t; }
    return mx;
}
