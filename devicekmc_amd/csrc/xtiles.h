// xtiles.h -- layout of the tiled form of X shared by xt.hip (assembly, single-vector CG, power pass) and xtb.hip (block-CG with
// the MFMA tile x panel product).  See the head of xt.hip for the storage scheme.
#pragma once
#include "xshared.h"
#include "cg_host.h"

#define XT_R 32                      // S-rows per tile
#define XT_C 256                     // S-columns per tile
#define XT_SBW 32                    // columns per sub-block
#define XT_SUB (XT_R * XT_SBW)       // doubles per sub-block (8 KiB)
#define XT_NT 256
#define XT_MAXKC 32                   // largest nominal run length (tiles) of a wave: min(XT_MAXKC, tiles / ranks / 4096); 16 until round 5 (profiles/r05_ab_tile_run_lists.jsonl)

typedef double dbl2 __attribute__((ext_vector_type(2)));
// fp32 image of the tile values (dkmc_set_x_tile_f32): the sub-block layout at half width.  A sub-block is 4 consecutive 1-KiB wave loads; lane
// (rr, cc) of load u holds the two fp64 loads 2 u, 2 u + 1 of its lane: rows 8 u + rr and 8 u + 4 + rr, columns 2 cc, 2 cc + 1.
// Position (floats) of element (row r, column c) inside its sub-block:
__host__ __device__ static inline int xt_tval32_pos(int r, int c) { return (((r >> 3) * 64 + (r & 3) * 16 + (c >> 1)) << 2) + (((r >> 2) & 1) << 1) + (c & 1); }

struct __attribute__((aligned(16))) XTile { int k, w; unsigned mask; int soff; };   // cell (k, w); present sub-blocks; first sub-block slot
struct __attribute__((aligned(32))) XItem { int t0, t1, w, c, k0; unsigned mask0; int soff0, pad; };   // tiles [t0, t1) of strip w; c = position of the run in its strip; descriptor of tile t0; pad = record of its column sums, colpart[pad * 256]: the run's own (c = 0; pad = its index in the item list) or, on one GPU, one record per aligned group of four runs -- the four waves of a workgroup (c = 1; pad = index / 4; every strip's run count padded to a multiple of four with empty runs)
struct XCtrl { double rr[2]; int done_local, sharded; int done; int iters; int abort_local, aborted; int pad[2]; int xchg_timeout, pad2; };
// `done` (non-zero) gates every kernel of the loop; see k_xt_step for its iteration stamp.  Single GPU: set by the step kernel.  Sharded solve: the direction kernel only sets
// done_local; rank 0's done_local travels in the all-reduced buffer (slot ns) and k_xt_rows_apply turns it into `done` on every
// rank in the same iteration -- all control flow derives from data every rank received from the same collective, so the ranks
// cannot leave the loop at different iterations even if their arithmetic differed in a bit.

struct SNodes {                      // S in rank order, padded to a multiple of XT_C (flag 0 = no entries)
    const double *x, *y, *z, *cb;
    const int *flag, *slot, *mr;     // class flags; row of the coefficient cache (vacancies) / column (metals), -1 if none
    const int *slotA;                // row of the cache's part A (sharded solve: left-contact columns of this rank's vacancies), -1 if none
};

struct XTState {
    // shape of the last assembly
    int Nsub = 0, ns = 0, ns_pad = 0, nK = 0, nW = 0, ntiles = 0, nitems = 0, kc = 1, maxchunk = 1, rec_shift = 0;
    long long nsub_total = 0, xs_nnz = 0;
    unsigned long long t_upper = 0;
    // this rank's share
    int item_lo = 0, item_n = 0, tile_lo = 0, tile_n = 0, w_lo = 0, w_hi = 0; long long sub_base = 0, sub_n = 0;
    bool valid = false;
};

struct XTBuffers {
    SNodes S; int *srow; XTile *tiles; XItem *items; int2 *wrange; int *nitem_w; double *tval, *rowpart, *colpart;
    int *wlist;                      // per row block: nW + 1 ints, the count and the ascending windows that hold a tile (k_xt_wrange; the list fold of xtb.hip)
    float *tval32;                   // fp32 image of tval for the block-CG's sweeps (dkmc_set_x_tile_f32; xt_tval32_pos), null if none
    xrp_t *rp, *dpos; int *ci; double *val; int *nsrank;
    unsigned *cmask; int *toff;      // census of the last assembly (kept for dkmc_xt_time_share)
    const double *ax, *ay, *az;      // atom positions of the last assembly (dkmc_xtb_emulate_slabs)
};

extern XTState g_xt;
extern XTBuffers g_xb;

// the live view of the resident tile list (xt_live.h; dkmc_set_x_tile_drop): what the sweeps of the one-GPU preconditioned block-CG launch on instead of
// the full view when state == 1 -- the tiles with a scaled entry at or above the threshold, their fp32 sub-blocks compacted, their own items,
// nitem_w, wrange and records.  info / ms: the report of dkmc_get_x_tile_live_info (info[0] is `state`)
struct XLive {
    int state = 0;                   // 0 off or not applicable, 1 usable, -1 no buffer for the compact image, -2 nothing to drop
    const XTile *tiles = nullptr; const XItem *items = nullptr; int item_n = 0; const int2 *wrange = nullptr; const int *nitem_w = nullptr; int nrecords = 0;
    const int *wlist = nullptr;      // the live tiles' windows by row block (the layout of XTBuffers::wlist)
    int nitems = 0;                 // runs of the live view (what dkmc_stats.xt_items reports after a solve whose sweeps ran on it)
    const float *tval32 = nullptr;   // the compact image (sub-block slot = the live tile's soff; with dkmc_set_x_tile_drop_unit(1) only the live sub-blocks of a tile, its mask reduced to them)
    const int *tflag = nullptr;      // per STORED tile: 1 live, 0 dead
    long long info[8] = {0, 0, 0, 0, 0, 0, 0, 0}; double ms[2] = {0.0, 0.0};
};
extern XLive g_xlive;                // the last solve's
int xt_live_build(double theta, int unit, const double *sS, XLive *lv);
double xtl_drop_rule(long long stored_subblocks, long long gate_override);      // auto mode's threshold for a stored X of that many sub-blocks (xt_live.h)
void xt_live_zero_dead(const XLive &lv, double *rowpartB, int so);
int xt_live_for_test(XLive *lv);

// ---- block-CG on the tiled X (xtb.hip) ----
#define DKMC_XTB_AGAIN 1001          // xtb_cg_body (preconditioned solve): the true residual does not meet the stop test yet; y holds the iterate reached
#define DKMC_XTB_BREAKDOWN 1000      // xtb_cg: an s x s system lost definiteness; y holds the last good iterate (not an error)
struct XtbArgs {
    int m, ns, ns_pad, nK, nW;                    // system rows; |S|; padded |S|; row blocks; windows
    int s;                                        // block width (2 ... 16)
    const XItem *items; int item_n;               // this rank's runs (padded to groups of four per strip)
    const XTile *tiles; int sub_base; const double *tval;
    const float *tval32;                          // fp32 image of tval (null: none): the sweeps of the one-GPU preconditioned loop stream it (dkmc_set_x_tile_f32)
    const int2 *wrange; const int *nitem_w; int nrecords;
    const int *wlist;                             // windows holding a tile, by row block (XTBuffers::wlist); null: the folds walk wrange
    const int *srow; const double *sS; const int *nsrank;
    const xrp_t *rp; const int *ci; const double *val;      // neighbour part Xs (CSR, unscaled, diagonal included)
    const double *sc;                             // Jacobi scaling 1 / sqrt(diag)
    const double *ax, *ay, *az;                   // position of the atom of row r >= 2 at [r - 2] (smooth auxiliary columns; may be null)
    const double *b;                              // scaled right-hand side
    double *y;                                    // in: scaled start vector y / s; out: scaled solution
    double *yaux; int yaux_valid;                 // UNSCALED solutions of the auxiliary columns, [m][16] (may be null): in (if valid) the previous solve's, out this solve's
    XCtrl *ctrl; double tol2; bool nt_loads;
    bool sharded; int w_lo, w_hi;                 // sharded solve (comm.hip): windows of this rank's tiles
    bool warm;                                    // y holds the previous solve's solution (current.hip: the warm-start copy was loaded); auto mode of the live view needs it
    long long stored_subblocks;                   // sub-blocks of the stored X, all ranks (the size auto mode's gate is stated in)
};
int xtb_cg(const XtbArgs &A, int *iters_out, double *rr_out);
// one rank's share of the work items of an nranks-way split (xt.hip: xt_build_items)
struct XShare { int nitems, maxchunk, item_lo, item_n, tile_lo, tile_n, w_lo, w_hi; long long sub_base, sub_n; XItem *items; int *nitem_w; int rec_shift; };
// the slab-distributed block-CG with nr VIRTUAL ranks in this process (xtb_slab.inc); times_us[8]: mean kernel times of virtual rank time_rank
// (apply, neighbour part, fold, rows, Gram reduction, s x s algebra, step, pack + unpack); xdoubles[3]: doubles a rank receives per sweep in the three exchanges
int xtb_cg_slab_emulate(const XtbArgs &A, int nr, const XShare *shares, int time_rank, int sweep_cap, int *iters_out, double *rr_out, double *times_us, long long *xdoubles);
__global__ void k_xt_vec_mul(int m, double *__restrict__ y, const double *__restrict__ s);
