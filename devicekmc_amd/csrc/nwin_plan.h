// nwin_plan.h -- the window plan of the LDS-windowed packed N product (xtb_precond.h: k_xtb_nmulw).  Plain C++ (no HIP): tests/cpu/nwin_plan_check.cpp
// includes this header alone; the kernel and its host side call the same functions, so what the check sees is what runs.
//
// The rows of the packed N are cut into blocks of B consecutive rows (B a multiple of 16: whole slices of four rows, whole 16-row groups).  In
// structure order the neighbours of an atom sit one and two atomic layers away (median |row - col| 85 ... 94, 99 % within 182 in a single cell), so
// the window of a block is ONE contiguous segment of panel rows: the block and an equal halo on either side, as many rows as the LDS cap leaves,
// clipped to [0, m).  That makes the plan pure arithmetic of (m, B, cap, block): nothing is stored per solve and nothing is built per solve.  A
// slot's code is formed from its packed column in registers: the row inside the window, or -- outside it (the cross-cell neighbours of a lateral
// tiling, far columns) -- the complement of the global column, a negative number: "gather from memory as before".  Padding and zero-weight slots
// name the row itself, which lies in its block's window whenever the cap holds a block.
#pragma once

#ifdef __HIPCC__
#define NWIN_HD __host__ __device__
#else
#define NWIN_HD
#endif

#define NWIN_ROW_BYTES 128                  // a panel row: 16 vectors of 8 bytes
#define NWIN_CAP_BYTES (76 * 1024)          // LDS of a workgroup at most: two workgroups share the 160 KiB of a CU
#define NWIN_BLOCK 320                      // rows of a block: 80 slices, five per wave of the kernel; the halo is then 144 rows (fastest of 192 ... 512 at 642 101 rows)
#define NWIN_BLOCK_MAX 1024                 // ... at most

struct NwinWindow { int lo, n; };           // panel rows lo ... lo + n - 1; n = 0: no window, every slot is flagged

// rows the cap holds
NWIN_HD inline int nwin_cap_rows(int cap_bytes) { return cap_bytes > 0 ? cap_bytes / NWIN_ROW_BYTES : 0; }
// a block size the kernel can run: a multiple of 16 in 16 ... 1024, else the default
NWIN_HD inline int nwin_block_rows(int B) { return (B >= 16 && B <= NWIN_BLOCK_MAX && B % 16 == 0) ? B : NWIN_BLOCK; }
// blocks of m rows
NWIN_HD inline int nwin_blocks(int m, int B) { return m > 0 ? (m + B - 1) / B : 0; }
// the window of block b: the block's rows r0 ... r1 - 1 and a halo of (cap_rows - B) / 2 rows on either side, clipped to [0, m); a cap below a block:
// the first cap_rows rows of the block
NWIN_HD inline NwinWindow nwin_window(int m, int B, int cap_rows, int b)
{
    const int r0 = b * B, r1 = r0 + B < m ? r0 + B : m;
    if (cap_rows <= 0 || r0 >= m) return {0, 0};
    if (cap_rows < B) return {r0, r1 - r0 < cap_rows ? r1 - r0 : cap_rows};
    const int h = (cap_rows - B) / 2, lo = r0 - h > 0 ? r0 - h : 0, hi = r1 + h < m ? r1 + h : m;
    return {lo, hi - lo};
}
// the code of a slot of column c (0 <= c): >= 0 the row of the window that holds panel row c, < 0 the complement of c (outside the window)
NWIN_HD inline int nwin_code(int c, NwinWindow W) { const int rel = c - W.lo; return (unsigned)rel < (unsigned)W.n ? rel : ~c; }
// LDS bytes of a launch: the largest window of any block, one row at least (a flagged lane's LDS read names row 0)
NWIN_HD inline int nwin_lds_bytes(int m, int B, int cap_rows)
{
    int n = B + 2 * ((cap_rows - B) / 2);
    if (cap_rows < B) n = cap_rows;
    if (n > m) n = m;
    return (n > 1 ? n : 1) * NWIN_ROW_BYTES;
}
// The switch (dkmc_set_x_nmul_window): 0 off, 1 on wherever the packed 16-byte form runs without a row list, 2 by size: systems of at least
// gate_rows rows.
NWIN_HD inline bool nwin_use(int mode, int m, int gate_rows) { return mode == 1 || (mode == 2 && m >= gate_rows); }
