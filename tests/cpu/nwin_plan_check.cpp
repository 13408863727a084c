// Stand-alone check of csrc/nwin_plan.h (tests/test_nwin_plan.py compiles it with -fsanitize=address,undefined and runs it): the window plan of the
// LDS-windowed packed N product on synthetic patterns.  The slots of a row are formed as k_xtb_npack forms them (entries outside N, driver rows and
// the padding of a slice name the row itself -- rows past m: row m - 1 -- with weight 0), the LDS image as k_xtb_nmulw fills it (LDS row i = panel
// row lo + i).  usage: nwin_plan_check <pattern> <m> <B> <cap_bytes>; prints "ok slots S inwin I flagged F blocks NB winrows W" or the first violation.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "nwin_plan.h"

static unsigned long long g_seed = 1;
static unsigned rnd() { g_seed = g_seed * 6364136223846793005ull + 1442695040888963407ull; return (unsigned)(g_seed >> 33); }

#define FAIL(...) do { std::printf("FAIL " __VA_ARGS__); std::printf("\n"); return 1; } while (0)

int main(int argc, char **argv)
{
    if (argc != 5) { std::fprintf(stderr, "usage: nwin_plan_check <pattern> <m> <B> <cap_bytes>\n"); return 2; }
    const char *pat = argv[1];
    const int m = std::atoi(argv[2]), Bin = std::atoi(argv[3]), cap_bytes = std::atoi(argv[4]);
    if (m < 1) return 2;
    g_seed = 12345u + (unsigned)m;
    // ---- the pattern: columns of every row -------------------------------------------------------------------------------------------------
    std::vector<std::vector<int>> rows(m);
    auto put = [&](int r, long long c) { if (c >= 0 && c < m) rows[r].push_back((int)c); };
    for (int r = 0; r < m; ++r) {
        if (!std::strcmp(pat, "band")) {                       // bands at +-85 and +-170 (one and two atomic layers), three entries wide, and the diagonal
            for (int d : {-170, -85, 85, 170}) for (int j = -1; j <= 1; ++j) put(r, (long long)r + d + j);
            put(r, r); put(r, 0); put(r, 1);
        } else if (!std::strcmp(pat, "far10")) {               // as band, one entry in ten anywhere
            for (int d : {-170, -85, 85, 170}) for (int j = -1; j <= 1; ++j) { if (rnd() % 10 == 0) put(r, rnd() % m); else put(r, (long long)r + d + j); }
        } else if (!std::strcmp(pat, "allfar")) {              // every column at least 5000 rows away: outside any window the cap allows
            for (int j = 0; j < 9; ++j) put(r, ((long long)r + 5000 + (long long)(rnd() % 1000)) % m);
        } else if (!std::strcmp(pat, "wide")) {                // rows of 0, 1, 17, 33 and 70 entries in turn, rows 8 ... 11 empty
            static const int ln[5] = {0, 1, 17, 33, 70};
            const int n = (r >= 8 && r < 12) ? 0 : ln[r % 5];
            for (int j = 0; j < n; ++j) put(r, (long long)r - 40 + (long long)(rnd() % 81));
        } else if (!std::strcmp(pat, "random")) {
            const int n = (int)(rnd() % 24);
            for (int j = 0; j < n; ++j) put(r, rnd() % m);
        } else return 2;
    }
    // ---- the plan ----------------------------------------------------------------------------------------------------------------------------
    const int B = nwin_block_rows(Bin), cap_rows = nwin_cap_rows(cap_bytes), nb = nwin_blocks(m, B);
    if (B % 16 != 0 || B < 16) FAIL("block %d", B);
    if (cap_rows * NWIN_ROW_BYTES > cap_bytes && cap_bytes >= 0) FAIL("cap rows %d above %d bytes", cap_rows, cap_bytes);
    const int lds = nwin_lds_bytes(m, B, cap_rows);
    if (lds < NWIN_ROW_BYTES || (lds > cap_bytes && lds > NWIN_ROW_BYTES)) FAIL("lds bytes %d, cap %d", lds, cap_bytes);
    // blocks cover every row once
    if ((long long)nb * B < m || (long long)(nb - 1) * B >= m) FAIL("blocks %d of %d do not cover %d rows once", nb, B, m);
    std::vector<int> covered(m, 0);
    long long slots = 0, inwin = 0, flagged = 0, winrows = 0;
    int prev_hi = 0, prev_lo = -1;
    for (int b = 0; b < nb; ++b) {
        const NwinWindow W = nwin_window(m, B, cap_rows, b);
        // the segment list of a block is one segment: inside [0, m), within the cap and the launch's LDS, moving forward with the blocks
        if (W.n < 0 || W.lo < 0 || W.lo + W.n > m) FAIL("block %d: window [%d, %d) outside [0, %d)", b, W.lo, W.lo + W.n, m);
        if (W.n > cap_rows || W.n * NWIN_ROW_BYTES > lds) FAIL("block %d: window of %d rows above the cap %d / lds %d", b, W.n, cap_rows, lds);
        if (W.n > 0 && (W.lo < prev_lo || W.lo + W.n < prev_hi)) FAIL("block %d: window moves backwards", b);
        if (cap_rows == 0 && W.n != 0) FAIL("block %d: a window with cap 0", b);
        if (W.n > 0) { prev_lo = W.lo; prev_hi = W.lo + W.n; }
        winrows += W.n;
        std::vector<int> image(W.n > 0 ? W.n : 0);              // LDS row -> panel row, as the copy fills it
        for (int i = 0; i < W.n; ++i) image[i] = W.lo + i;
        const int r0 = b * B, r1 = r0 + B;                      // the block's slices may reach past m (the padding rows of the last slice)
        for (int q = r0 / 4; q < r1 / 4 && 4 * q < m; ++q) {
            int w = 0;
            for (int r = 4 * q; r < 4 * q + 4; ++r) if (r < m && r >= 2) w = (int)rows[r].size() > w ? (int)rows[r].size() : w;
            for (int r = 4 * q; r < 4 * q + 4; ++r) {
                if (r < m) ++covered[r];
                for (int k = 0; k < w; ++k) {
                    int c = (r < m && r >= 2 && k < (int)rows[r].size()) ? rows[r][k] : -1;
                    if (c < 2 || c == r) c = r < m ? r : m - 1;            // k_xtb_npack: weight 0 on the row itself
                    const int code = nwin_code(c, W);
                    ++slots;
                    if (code >= 0) {
                        if (code >= W.n || image[code] != c) FAIL("row %d slot %d: LDS row %d does not hold column %d", r, k, code, c);
                        ++inwin;
                    } else {
                        if (~code != c) FAIL("row %d slot %d: flag carries %d, column %d", r, k, ~code, c);
                        if (c >= W.lo && c < W.lo + W.n) FAIL("row %d slot %d: column %d flagged inside the window", r, k, c);
                        ++flagged;
                    }
                }
            }
        }
        // a cap that holds a block: the block's own rows are in the window (what the padding slots name)
        if (cap_rows >= B) for (int r = r0; r < r1 && r < m; ++r) if (nwin_code(r, W) < 0) FAIL("block %d: its row %d outside its window", b, r);
    }
    for (int r = 0; r < m; ++r) if (covered[r] != 1) FAIL("row %d covered %d times", r, covered[r]);
    if (cap_rows == 0 && inwin != 0) FAIL("cap 0: %lld slots in a window", inwin);
    if (nwin_use(0, m, 1) || !nwin_use(1, m, 1 << 30) || nwin_use(2, m, m + 1) || !nwin_use(2, m, m)) FAIL("switch");
    std::printf("ok slots %lld inwin %lld flagged %lld blocks %d winrows %lld\n", slots, inwin, flagged, nb, winrows);
    return 0;
}
