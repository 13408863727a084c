// kbw_plan.h -- host side of the windowed blocked form of K (kcg.hip: kbw_build).  Plain C++ (no HIP): the plan is built once per pattern
// from host copies of the pattern and the row coordinates.
//
// Rows are ordered spatially: the lateral plane is cut into columns of w x w (w = the largest lateral reach |dy| of a stored entry, so that
// every neighbour of a row lies in its own strip of columns or the two next to it), the columns are walked in serpentine order (strip by
// strip in y, alternating direction in z) and the rows of a column in x, again alternating direction from column to column.  Consecutive
// rows are then spatial neighbours, and a block of R consecutive rows -- a stretch of one strip -- touches the same stretch of the two
// neighbouring strips: its window (the union of the rows its entries read) is a few contiguous SEGMENTS of that order (3 inside a strip, up
// to 6 where a block turns a strip end), which the product copies into LDS one after the other.  The stored columns are rewritten as
// offsets into that LDS image; the row's own offset is its padding (skipped by the product), as in the single-window blocked form.
#pragma once
#include <algorithm>
#include <cmath>
#include <cstdint>
#include <vector>

#define KBW_MAXSEG 16           // segments per block window (fixed: the table has KBW_MAXSEG entries per block)
#define KBW_GAP 256             // rows of the order between two used runs that are copied rather than starting a new segment

// The 2-byte layout of a row's stored words (dkmc_set_k_window_word_bytes(2)): position, in 16-bit words from the start of the row, of entry e of a
// row padded to `width` (32 or 64) entries.  The product gives a row 4 lanes, and lane l holds entries 4l..4l+3 and 16+4l..16+4l+3 (of a 64-wide row
// also 32+4l.. and 48+4l..) in that order; with 16-bit words those eight entries are the 16-byte chunk l of the row (the second eight: chunk 4 + l),
// so one 16-byte load per lane and chunk delivers them in the same slots.  A permutation of 0..width-1; -1 outside the row or for another width.
// (constexpr: k_kbw_assemble calls it on the device, the host and the tests through dkmc_debug_kbw_halfword_pos)
constexpr inline int kbw_halfword_pos(int width, int e)
{
    if ((width != 32 && width != 64) || e < 0 || e >= width) return -1;
    const int j = e / 16, l = e % 16 / 4, u = e % 4;          // j: which four-entry group of the lane (ints 16 j + 4 l ...)
    return ((j / 2 * 4 + l) * 2 + j % 2) * 4 + u;
}

struct KbwI4 { int x, y, z, w; };
struct KbwPlan {
    int R = 0, nb = 0, total = 0, maxwin = 0, maxints = 0, maxseg = 0;
    long long winsum = 0, segsum = 0;
    std::vector<int> perm;          // [m] row of the blocked order -> row of the pattern
    std::vector<int> pcol;          // [total] LDS offsets into the block's window; padding = the row's own offset
    std::vector<KbwI4> blk;         // [nb] {window doubles, LDS offset of the block's first row, first int of the block in pcol, rows padded to 64}
    std::vector<KbwI4> seg;         // [nb * KBW_MAXSEG] {LDS offset, length, first row in the blocked order, 0}; unused: {INT32_MAX, 0, 0, 0}
};

// 0: plan built.  1: a row has more than 64 off-diagonal entries; 2: no block size lets every window fit `budget` doubles within at most
// `maxseg` segments with at most `maxblocks` blocks.  ncu: blocks at least (one per CU).
inline int kbw_plan(int m, const int *rp, const int *ci, const double *x, const double *y, const double *z, int ncu, int budget, int maxseg,
                    int maxblocks, KbwPlan &P)
{
    if (m < 1 || ncu < 1 || maxseg < 1 || maxseg > KBW_MAXSEG) return 2;
    auto offdiag = [&](int r) { int n = 0; for (int p = rp[r]; p < rp[r + 1]; ++p) n += ci[p] != r; return n; };
    for (int r = 0; r < m; ++r) if (offdiag(r) > 64) return 1;
    // ---- spatial order ----
    double w = 0.0, y0 = y[0], y1 = y[0], z0 = z[0], z1 = z[0], x0 = x[0], x1 = x[0];
    for (int r = 0; r < m; ++r) {
        y0 = std::min(y0, y[r]); y1 = std::max(y1, y[r]); z0 = std::min(z0, z[r]); z1 = std::max(z1, z[r]); x0 = std::min(x0, x[r]); x1 = std::max(x1, x[r]);
        for (int p = rp[r]; p < rp[r + 1]; ++p) w = std::max(w, std::fabs(y[ci[p]] - y[r]));
    }
    w = std::max(w, std::max(y1 - y0, z1 - z0) / 65536.0);
    w = std::max(w, 1e-12);
    // strips and columns of equal width >= w (no thin last strip: its blocks would reach far along z)
    const long long nsy = std::max(1LL, (long long)((y1 - y0) / w)), ncz = std::max(1LL, (long long)((z1 - z0) / w));
    const double wy = (y1 - y0) / nsy * (1.0 + 1e-12) + 1e-300, wz = (z1 - z0) / ncz * (1.0 + 1e-12) + 1e-300;
    const double xs = x1 > x0 ? 2147483646.0 / (x1 - x0) : 0.0;
    std::vector<long long> key(m);
    for (int r = 0; r < m; ++r) {
        const long long sy = std::min(nsy - 1, (long long)((y[r] - y0) / wy)), cz = std::min(ncz - 1, (long long)((z[r] - z0) / wz));
        const long long col = sy * ncz + ((sy & 1) ? ncz - 1 - cz : cz);
        long long xq = (long long)((x[r] - x0) * xs);
        if (col & 1) xq = 2147483646LL - xq;
        key[r] = (col << 31) | xq;
    }
    std::vector<int> order(m);
    for (int i = 0; i < m; ++i) order[i] = i;
    std::stable_sort(order.begin(), order.end(), [&](int a, int b) { return key[a] < key[b]; });
    // ---- blocks: R from one block per CU down until every window fits ----
    const int rmin = (m + maxblocks - 1) / maxblocks;
    int R = (m + ncu - 1) / ncu;
    std::vector<int> inv(m), stamp(m, -1), used;
    for (int attempt = 0; attempt < 12; ++attempt) {
        if (R < rmin || R < 1) return 2;
        const int nb = (m + R - 1) / R;
        P.perm = order;
        std::vector<KbwI4> blk(nb);
        long long total = 0;
        int maxints = 0;
        for (int b = 0; b < nb; ++b) {
            const int lo = b * R, hi = std::min(m, lo + R);
            auto mid = std::stable_partition(P.perm.begin() + lo, P.perm.begin() + hi, [&](int r) { return offdiag(r) > 32; });
            const int nl = (int)(mid - (P.perm.begin() + lo));
            blk[b] = KbwI4{0, 0, (int)total, nl};
            total += (long long)nl * 64 + (long long)(hi - lo - nl) * 32;
            maxints = std::max(maxints, nl * 64 + (hi - lo - nl) * 32);
        }
        if (total > 2147483647LL) return 2;
        for (int i = 0; i < m; ++i) inv[P.perm[i]] = i;
        std::fill(stamp.begin(), stamp.end(), -1);
        std::vector<KbwI4> seg((size_t)nb * KBW_MAXSEG, KbwI4{2147483647, 0, 0, 0});
        int maxwin = 0, maxs = 0;
        long long winsum = 0, segsum = 0;
        bool fits = true;
        for (int b = 0; b < nb && fits; ++b) {
            const int lo = b * R, hi = std::min(m, lo + R);
            used.clear();
            for (int i = lo; i < hi; ++i) {
                if (stamp[i] != b) { stamp[i] = b; used.push_back(i); }
                const int r = P.perm[i];
                for (int p = rp[r]; p < rp[r + 1]; ++p) { const int c = inv[ci[p]]; if (stamp[c] != b) { stamp[c] = b; used.push_back(c); } }
            }
            std::sort(used.begin(), used.end());
            int ns = 0, off = 0;
            size_t k = 0;
            while (k < used.size()) {
                const int s0 = used[k];
                int s1 = s0;
                while (k + 1 < used.size() && used[k + 1] - s1 <= KBW_GAP) s1 = used[++k];
                ++k;
                if (ns == maxseg) { fits = false; break; }
                seg[(size_t)b * KBW_MAXSEG + ns] = KbwI4{off, s1 - s0 + 1, s0, 0};
                off += s1 - s0 + 1; ++ns;
            }
            if (!fits) break;
            blk[b].x = off;
            for (int s = 0; s < ns; ++s) {          // the block's own rows are contiguous, hence inside one run
                const KbwI4 &g = seg[(size_t)b * KBW_MAXSEG + s];
                if (lo >= g.z && hi <= g.z + g.y) blk[b].y = g.x + (lo - g.z);
            }
            maxwin = std::max(maxwin, off); maxs = std::max(maxs, ns);
            winsum += off; segsum += ns;
        }
        if (fits && maxwin > budget) fits = false;
        if (!fits) {                                               // a window too large or too fragmented: smaller blocks
            const long long Rn = maxwin > budget ? (long long)((double)R * budget / maxwin * 0.97) : (long long)(R * 0.7);
            R = (int)std::min<long long>(Rn, R - 1);
            continue;
        }
        // ---- columns -> LDS offsets ----
        std::vector<int> pcol((size_t)total);
        for (int b = 0; b < nb; ++b) {
            const int lo = b * R, hi = std::min(m, lo + R), nl = blk[b].w;
            const KbwI4 *sg = seg.data() + (size_t)b * KBW_MAXSEG;
            for (int i = lo; i < hi; ++i) {
                const int k2 = i - lo, width = k2 < nl ? 64 : 32;
                int *dst = pcol.data() + blk[b].z + (k2 < nl ? (size_t)k2 * 64 : (size_t)nl * 64 + (size_t)(k2 - nl) * 32);
                const int r = P.perm[i], self = blk[b].y + k2;
                int n = 0;
                for (int p = rp[r]; p < rp[r + 1]; ++p) {
                    if (ci[p] == r) continue;
                    const int c = inv[ci[p]];
                    int s = 0;
                    while (s + 1 < KBW_MAXSEG && sg[s + 1].z <= c && sg[s + 1].y > 0) ++s;
                    dst[n++] = sg[s].x + (c - sg[s].z);
                }
                std::sort(dst, dst + n);
                for (; n < width; ++n) dst[n] = self;
            }
        }
        P.R = R; P.nb = nb; P.total = (int)total; P.maxwin = maxwin; P.maxints = maxints; P.maxseg = maxs; P.winsum = winsum; P.segsum = segsum;
        P.pcol.swap(pcol); P.blk.swap(blk); P.seg.swap(seg);
        return 0;
    }
    return 2;
}
