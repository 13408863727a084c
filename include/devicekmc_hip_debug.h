/*
 * devicekmc_hip_debug.h -- test and measurement aids exported by libdevicekmc_hip.so.  NOT part of the drop-in boundary
 * (include/devicekmc_hip.h): nothing here replaces a reference symbol; tests/ and bench.py bind them through devicekmc_amd/lib.py.
 */
#ifndef DEVICEKMC_HIP_DEBUG_H
#define DEVICEKMC_HIP_DEBUG_H
#include "devicekmc_hip.h"
#ifdef __cplusplus
extern "C" {
#endif

/* measurement aid (bench.py's strong-scaling model): on the tiled X left resident by the last single-GPU update_power, the time per CG
 * iteration of what ONE rank of an nranks-way sharded solve runs -- apply_us: the apply kernel over that rank's share of the tiles
 * (work items sized as an nranks run sizes them) + the neighbour part; side_us[4]: partial row sums, finish, vector step, and -- nranks > 1 or a multi-GB sweep, where apply_us is the tile pass alone -- the
 * neighbour part that a sharded solve runs on a second stream beside the exchange (each timed on its own).  The
 * all-reduce between them cannot be measured on one GPU.  Scratch vectors are overwritten; results of the last solve already
 * delivered (potentials, I_macro, power) are not. */
int dkmc_xt_time_share(int nranks, int rank, int reps, double *apply_us, double *side_us /* [4] */, int *items_out, long long *subblocks_out);
/* Test aid: emulates on ONE GPU the tile pass of an nranks-way sharded matrix-vector product over the X of the last single-GPU solve
 * (every rank's work items built as a sharded assembly builds them, partial arrays zeroed per rank, partial row sums restricted to
 * the rank's windows) and compares the sum of the ranks' results with the one-GPU pass.  subblocks_sum / items_sum: totals over the
 * shares (must equal the stored sub-blocks / items_total: every tile in exactly one share). */
int dkmc_xt_check_shares(int nranks, double *max_abs_diff, double *max_abs, long long *subblocks_sum, long long *items_sum, int *items_total);
/* Test aid: on the X left resident by the last single-GPU solve, the MFMA tile x panel product of the block-CG (16 test vectors, one
 * sweep) against 16 passes of the single-vector tile kernel; largest absolute deviation and largest sum over the S rows. */
int dkmc_xtb_check_product(int width, double *max_abs_diff, double *max_abs);
/* Test aids of the split polynomial preconditioner L = p(N) of the block-CG (dkmc_set_x_poly; csrc/xtb_precond.h).
 * dkmc_xtb_poly_coeffs: its coefficients pc[0 ... degree] (monomial basis, Horner order of the solve); host code only, no GPU needed.  degree: 1 ... 16.
 * dkmc_xtb_test_nstep: ONE Horner step out = ca add + cb (N in) of the production kernels over a caller-given CSR (m rows, rp[m] entries, columns in
 * [0, m)) and host panels in / add / out of [m][16]: out_r = ca add_r - cb sc_r sum val sc_c in_c over the entries with c >= 2 and c != r; rows 0 / 1
 * take ca add.  form 1: N packed first (the default form of a solve), 0: the CSR form.  rowlist (nlist rows, may be null): the row-list variants of
 * the slab-distributed loop -- only those rows are written.  nsrank (may be null; ranks -1 ... ns - 1): QS of out as well, returned as qs [ns][16] =
 * sc_r out_r at the rows of rank >= 0 (0 where nothing was written).  out is read before the step and written back after it.
 * dkmc_xtb_check_poly: L in (the full Horner sequence with QS, as a sweep applies it) on the X left resident by the last single-GPU solve, with that
 * solve's scaling, neighbour part and S ranks: in / out [m][16], m = rows of X; qs [ns][16].  Leaves the next solve's start and launch batch alone. */
int dkmc_xtb_poly_coeffs(int degree, double *pc);
/* The degree rule of the one-GPU preconditioned loop (dkmc_set_x_poly_auto; csrc/xtb_precond.h: xtb_poly_rule).
 * dkmc_xtb_poly_rule: the degree it gives a system of m rows (0 for m <= 2); host code only, no GPU needed.
 * dkmc_set_x_poly_auto_rows: test aid -- overrides the rule's two breakpoints (rows below n0: first step, below n1: second, else third) so that
 * every branch can be reached at a small size; (0, 0) restores the measured ones. */
int dkmc_xtb_poly_rule(int m);
void dkmc_set_x_poly_auto_rows(int n0, int n1);
int dkmc_xtb_test_nstep(int m, const long long *rp, const int *ci, const double *val, const double *sc, const double *in, const double *add,
                        double ca, double cb, int form, const int *rowlist, int nlist, const int *nsrank, int ns, double *out, double *qs);
int dkmc_xtb_check_poly(int degree, int form, const double *in, double *out, double *qs);
/* Test aid of dkmc_set_x_nmul_window: the LDS bytes a window may take (0 ... 77824; 0: every slot gathers from memory, a small value: both operand
 * paths inside one row) and the rows of a block (a multiple of 16 in 16 ... 1024).  Out-of-range values restore 77824 and 320.  Same bits at any setting.
 * dkmc_xtb_check_poly and dkmc_xtb_test_nstep (form 1, no row list) follow dkmc_set_x_nmul_window and this aid as a solve does. */
void dkmc_debug_set_x_nmul_window(int cap_bytes, int block_rows);
/* Measurement aid: mean duration [us] of ONE N product inside L = p(N) of the given degree (1 ... 16), `reps` applications of L back to back on the X
 * left resident by the last single-GPU solve, packed form, under the current dkmc_set_x_nmul_lane_bytes / dkmc_set_x_nmul_window. */
int dkmc_xtb_time_poly(int degree, int reps, double *us);
/* Test aids of the last four launches of a preconditioned block-CG sweep (csrc/xtb.hip): the PRODUCTION kernels, with production's launch shapes, on data
 * the caller supplies.  They keep buffers and an XCtrl of their own: the resident X, the solver's XCtrl, the warm start and the launch batch of the next
 * solve are left alone.  Every argument is checked first; a bad one returns non-zero and launches nothing.  Panels are host arrays of [m][16] doubles.
 * dkmc_xtb_ctrl (below) mirrors the XCtrl of csrc/xtiles.h; ctrl_out receives the aid's own XCtrl after the launches.
 *
 * dkmc_xtb_test_gram: k_xtb_rows<0, 0, 1> (the form of a preconditioned sweep: T final in every row) over ng workgroups (1 ... 4096), then k_xtb_gred.
 *   nsrank[m]: -1, or an S rank 0 ... ns - 1 (each once); the aid builds srow from it, nK = ceil(ns / 32), and zeroed wrange / nitem_w arrays.
 *   done_word presets the stop word (non-zero: nothing is written).  gfin [6 * 256] is read (the pre-fill) and written: six 16 x 16 matrices in the order
 *   P'T, P'R, T'R, T'T, R'R, P'P (X'Z = sum over the rows of x_i z_j).  Entry (i, j) of matrix g sits at
 *       gfin[g * 256 + 64 * (i / 4) + 16 * (i % 4) + j]
 *   -- the row kernel's accumulator map: word 64 u + l of a matrix is register u of lane l, and that is entry (i, j) = (l / 16 + 4 u, l % 16).
 *   k_xtb_small reads its Gram blocks in the same map.
 * dkmc_xtb_test_small: ONE launch of k_xtb_small for iteration `it` (-1: the set-up pass) and block width s (1 ... 16).  gblocks [nrg][6 * 256 + 2]
 *   (nrg 1 ... 64): per rank the six matrices in the map above, a spare word, and the rank's abort word (read only when nrg > 1).  tol2: the stop bound
 *   (on rr for it >= 0, on sqrt(rr) for it = -1).  ctrl_in: the XCtrl the kernel starts from (sharded, done, pad[1] ...).  mats [4 * 256] is read (the
 *   pre-fill) and written: c | M1 = -W | M2 = beta W | M3 = c M1, each row-major [i * 16 + j].
 * dkmc_xtb_test_step: ONE launch of k_xtb_step for iteration `it` with the stop word preset to done_word, on the grid a solve gives it (at most 2048
 *   workgroups of four 16-row groups).  y0 [m], R, P and (may be null) Ypanel are read and written, T, sc [m], nsrank [m] (as above), mats are read.
 *   rowlist (nlist distinct rows, may be null): the row-list form of the slab-distributed loop -- only those rows are touched.  qs [ns][16] (null only with
 *   ns = 0): the pre-fill of QS and, afterwards, QS, both in natural order (the aid applies and undoes the kernel's interleaving of row pairs). */
typedef struct dkmc_xtb_ctrl { double rr[2]; int done_local, sharded; int done; int iters; int abort_local, aborted; int pad[2]; int xchg_timeout, pad2; } dkmc_xtb_ctrl;
int dkmc_xtb_test_gram(int m, const double *P, const double *T, const double *R, const int *nsrank, int ns, int ng, int done_word, double *gfin,
                       dkmc_xtb_ctrl *ctrl_out);
int dkmc_xtb_test_small(int it, int s, int nrg, const double *gblocks, double tol2, const dkmc_xtb_ctrl *ctrl_in, double *mats, dkmc_xtb_ctrl *ctrl_out);
int dkmc_xtb_test_step(int m, int it, const double *mats, int done_word, double *y0, double *R, double *P, const double *T, const double *sc,
                       const int *nsrank, int ns, const int *rowlist, int nlist, double *Ypanel, double *qs);
/* The one-polynomial form of the preconditioned loop (dkmc_set_x_poly_form).
 * dkmc_xtb_poly1_coeffs: coefficients pc[0 ... n] of q (monomial basis), n in 1 ... 20, and (qmin may be null) the smallest q over the 4001 equidistant
 *   points of [-1, 1]; host code only, no GPU needed.
 * dkmc_debug_set_x_poly1_degree: measurement aid -- n > 0 overrides the degree map n(d) of that form (at most 20); 0 restores the map.
 * dkmc_xtb_test_gram1: k_xtb_gram1 over ng workgroups (1 ... 4096), then k_xtb_gred, on six host panels of [m][16] in the order Pt, Pi, Q, U, Rt, Z.
 *   gfin as in dkmc_xtb_test_gram: Pt'Q, Pt'Rt, Q'Z, Q'U, Rt'Z, Pt'Pi; the last three symmetrised.
 * dkmc_xtb_test_step1: ONE launch of k_xtb_step1 for iteration `it` with the stop word preset to done_word.  panels as above: Pt, Pi, Rt, Z and y0 [m] are read
 *   and written, Q and U read; sc, nsrank, ns, mats and qs as in dkmc_xtb_test_step. */
int dkmc_xtb_poly1_coeffs(int n, double *pc, double *qmin);
void dkmc_debug_set_x_poly1_degree(int n);
int dkmc_xtb_test_gram1(int m, const double *const *panels, int ng, int done_word, double *gfin);
int dkmc_xtb_test_step1(int m, int it, const double *mats, int done_word, double *y0, double *const *panels, const double *sc, const int *nsrank, int ns,
                        double *qs);
/* The norm stop test of that form (dkmc_set_x_stop_form; csrc/xtb.hip: k_xtb_stop_norm).
 * dkmc_xtb_test_step1_norm: dkmc_xtb_test_step1 for it >= 0 with the kernel's partial sums of Rt+(i, 0)^2 switched on (pre-filled with NaN), then ONE
 *   launch of k_xtb_stop_norm against bound2, on an XCtrl with done = done_word and rr = {rr_in, rr_in}.  rec3 is read (the pre-fill) and written:
 *   the sum, rr_in as the kernel read it, 1.0 where the test set the stop word (done = it + 2, iters = it + 1); ctrl_out receives the XCtrl.
 * dkmc_debug_get_x_stop_rt0: column 0 of Rt as the last round of the last one-polynomial solve left it -- the panel whose norm dkmc_get_x_stop_info
 *   reports under form 1; rt0 [m], m = rows of X.  Fails where there was no such round or m differs. */
int dkmc_xtb_test_step1_norm(int m, int it, const double *mats, int done_word, double *y0, double *const *panels, const double *sc, const int *nsrank, int ns,
                             double *qs, double bound2, double rr_in, double *rec3, dkmc_xtb_ctrl *ctrl_out);
int dkmc_debug_get_x_stop_rt0(int m, double *rt0);
/* The size rule of dkmc_set_x_stop_form(2) (csrc/xtb_precond.h: xtb_stop_rule): 1 when a system of m rows runs the norm test; host code only. */
int dkmc_xtb_stop_rule(int m);
/* Measurement aid: average duration [us] of the tile x panel kernel of the block-CG over the X left resident by the last single-GPU solve
 * (`reps` launches).  variant 0: as a solve runs it; on the round-4 form of the loop: 1: without its matrix instructions (tile stream + LDS
 * traffic); 2: without re-reading the tile stream (matrix instructions + LDS traffic); 3: operand stages of one k-pair; 4: without LDS
 * traffic; 7: the matrix instructions alone; 10: the product form without re-reading the tile stream; 12: the product form with the partial
 * tiles skipped.  Variants other than 0 exist only in a library built with DKMC_MEASURE_VARIANTS=1 (python __graft_entry__.py); the shipped one
 * returns error 13 for them. */
int dkmc_xtb_time_apply(int width, int variant, int reps, double *us);
/* Measurement aid: how the resident X fills its tiles -- hist[c] = tiles with c of their 8 sub-blocks present (c = 0 .. 8), hist[9] = tiles inside a
 * chain (>= 2) of full tiles of a run, hist[10] = runs.  hist: 11 entries. */
int dkmc_xt_tile_census(long long *hist);
/* Measurement aid for the run list of the tile kernels (takes effect at the next assembly of X): kc > 0 overrides the nominal run length in tiles
 * (default min(32, tiles / ranks / 4096)); 0 restores it. */
void dkmc_set_x_items(int kc);
/* Same-box comparison aid: 1 = the solves (and variant 0 above) run the round-4 form of the tile x panel loop (stages issued in bursts,
 * conditional loads at the tile end, panel rows loaded directly) instead of the product form; same results bit for bit.  Default 0. */
/* test aid: the next true-residual check that ends a round of the preconditioned block-CG reports "above tolerance" once (host side; nothing on
 * the device changes): the solve is re-entered as after a real miss (dkmc_stats.x_tile_f64_rounds) */
void dkmc_debug_fail_true_residual_once(void);
/* test aid: the tile x panel product of dkmc_xtb_check_product's 16 test vectors (vector v of S rank r: 0.25 + (((r * 2654435761) ^ (v * 40503)) >> 20)
 * / 4096 + 0.125 v in 32-bit unsigned arithmetic) on the X left by the last single-GPU solve, streamed from the fp64 store (stored_bytes 8) or from its
 * fp32 image (4, dkmc_set_x_tile_f32; fails when the last assembly made none).  out (host): the tile sums of S rank r, vector v at [r * so + v],
 * so = width rounded up to a multiple of 4, before any row scaling.  stored_bytes -4: from the compact image of the live tiles at the current
 * dkmc_set_x_tile_drop threshold and dkmc_set_x_tile_drop_unit (unit 1: of the live sub-blocks), on its launch view (built afresh with the last
 * solve's scaling; fails when there is none, e.g. nothing to drop). */
int dkmc_xtb_tile_product(int width, int stored_bytes, double *out);
/* test aid: tile list (four ints per tile: row block k, column window w, mask of its present 32 x 32 sub-blocks, slot of its first one) and the fp64
 * values of the stored sub-blocks (element (row r, column c) of slot sl at [(sl * 32 + r) * 32 + c]: S ranks 32 k + r and 256 w + 32 q + c for the
 * q-th bit of the mask) of the last single-GPU assembly.  Null arrays: the counts only. */
int dkmc_xt_get_tiles(long long *ntiles, long long *nsub, int *tiles4, double *tval);
/* measurement aid: dkmc_xtb_time_apply of the kernel as a solve runs it, on the fp64 store (stored_bytes 8) or its fp32 image (4); stored_bytes -4:
 * on the live view and its compact image at the current dkmc_set_x_tile_drop threshold and dkmc_set_x_tile_drop_unit, built afresh as for
 * dkmc_xtb_tile_product (error 13 where there is no such view); what it streamed: dkmc_xt_get_live_masks / dkmc_get_x_tile_live_info */
int dkmc_xtb_time_apply_stored(int width, int stored_bytes, int reps, double *us);
/* Report of dkmc_set_x_tile_drop for the last current solve.  info8: [0] state -- 0 off or not applicable, 1 the compact image of the live tiles was
 * streamed, -1 no buffer for it, -2 nothing to drop (fewer than 1 / 64 of the sub-blocks); [1] tiles stored; [2] tiles live; [3] sub-blocks stored;
 * [4] sub-blocks in live tiles; [5] sub-blocks live on their own (what dkmc_set_x_tile_drop_unit(1) streams; with unit 0 the image does not use
 * it); [6] bytes of the compact image: 4096 x ([4] + 4) with unit 0, 4096 x ([5] + 4) with unit 1; [7] sweeps run on it.  [1]-[5] and [7] mean the
 * same in both units.  ms2 (written only with dkmc_set_profiling on): census + scan, compaction + view build. */
int dkmc_get_x_tile_live_info(long long *info8, double *ms2);
/* The size rule of dkmc_set_x_tile_drop_auto (csrc/xt_live.h: xtl_drop_rule).  dkmc_xtl_drop_rule: the threshold it gives a stored X of that many
 * sub-blocks -- 1e-10 at or above the gate, 0.0 below it and for sizes <= 0; host code only, no GPU needed.  dkmc_set_x_tile_drop_auto_subblocks: test
 * aid -- moves the gate so that a small workload reaches the live view; 0 (or less) selects the measured gate. */
/* The census of the live view (csrc/xt_live.h).  Form 1: from the fp32 image, with a guard band of 2^-22 around the threshold and an fp64 re-read of the
 * sub-blocks inside it -- the same flags, masks and counts as form 0, the census on the fp64 store, at half the bytes; taken only where there is an
 * image and theta >= 1e-290; the call returns the form that was set before.  dkmc_debug_xtl_census_reread: sub-blocks the last census read again from the fp64 store (0 with form 0). */
int dkmc_debug_xtl_census_form(int form);
long long dkmc_debug_xtl_census_reread(void);
double dkmc_xtl_drop_rule(long long stored_subblocks);
void dkmc_set_x_tile_drop_auto_subblocks(long long gate);
/* Test aid: for the X left by the last one-GPU solve, the live flag (1 / 0) of every stored tile at threshold theta, in dkmc_xt_get_tiles order, and
 * that solve's scaling by S rank (sS_out[xt_ns]).  Either array may be null. */
int dkmc_xt_get_live(double theta, int *live_per_tile, double *sS_out);
/* Test aid: from the same census, the mask of the sub-blocks LIVE ON THEIR OWN of every stored tile at threshold theta (a subset of the tile's stored
 * mask; 0 = dead tile), in dkmc_xt_get_tiles order: what dkmc_set_x_tile_drop_unit(1) streams of the tile. */
int dkmc_xt_get_live_masks(double theta, int *mask_per_tile);
/* The fold of the tile launch's row partial sums in the one-GPU preconditioned block-CG (csrc/xtb.hip: k_xtb_fold_rows).  Form 1 (default): it adds only
 * the cells of the launch view's tiles, by the per-row-block window lists of the assembly and of the live view; nothing zeroes the partial-sum array, and
 * the two one-column fp64 products that frame a solve run at one vector group.  Form 0: every cell of a row block's window range, over a per-solve
 * memset and k_xtl_zero_dead.  Same bits; other values select 1.  Every other loop keeps the range form.
 * dkmc_debug_poison_fold_cells: test aid, sticky until called with 0 -- a solve in form 1 fills the whole partial-sum array with NaN where form 0 zeroes
 *   it; a correct list fold never reads one.
 * dkmc_xt_get_fold_lists: test aid -- the window lists of the last one-GPU assembly (live 0) or of the live view of the last solve (live 1; error 13
 *   where that solve had none): rows[k * (nW + 1)] = windows of row block k that hold a tile of the view, then the windows, ascending.  rows may be
 *   null: the shape only. */
void dkmc_set_x_fold_form(int form);
int dkmc_get_x_fold_form(void);
void dkmc_debug_poison_fold_cells(int on);
int dkmc_xt_get_fold_lists(int live, int *nK, int *nW, int *rows);
/* Self-check of dkmc_set_x_static_tiles (csrc/xt_static.h); returns the setting before.  On: every assembly in metals-first order is followed by
 * the FULL census and a FULL fill of the resident tile list into buffers of their own (a second store: tests and small sizes only; the resident
 * store is only read), compared with what the assembly left.  dkmc_debug_get_x_static_verify, for the last solve: v4[0] differing words of the
 * cell masks, [1] differing 64-bit words of the fp64 store, [2] differing 32-bit words of the fp32 image, [3] |X_nnz as reported - recounted|;
 * their sum is info8[7] of dkmc_get_x_static_info.  dkmc_x_static_strips: the strips nM metals allow to keep, nM / 256 (0: a full fill); host
 * code only.  dkmc_xt_get_srow: the system row of every S rank of the last one-GPU assembly (srow_out[ns]; null: the count only).
 * dkmc_xt_get_diag: the row sums of the tunnelling block T of that assembly by SYSTEM row (d_out[rows of X], 0 outside S) -- the diagonal pass,
 * summed in the S order of that assembly. */
int dkmc_debug_x_static_verify(int on);
int dkmc_debug_get_x_static_verify(long long *v4);
int dkmc_x_static_strips(int n_metals);
/* The size rule of dkmc_set_x_static_tiles(2) (csrc/common.h: x_static_rule): 1 when a tunnelling set of that many members takes the metals-first order
 * -- at and above the measured gate of 32 768 members (profiles/ab_bench_x_static_tiles.txt); host code only.  dkmc_debug_set_x_static_gate: test aid --
 * moves the gate so that a small workload takes the new order under mode 2; 0 (or less) selects the measured gate. */
int dkmc_x_static_rule(int members);
void dkmc_debug_set_x_static_gate(int members);
int dkmc_xt_get_srow(int *ns_out, int *srow_out);
int dkmc_xt_get_diag(double *d_out);
void dkmc_set_x_apply_form(int form);
int dkmc_get_x_apply_form(void);
/* Test aid for the error path of a sharded current solve (no counterpart in the reference): the calling rank fails ONCE, in the
 * assembly of X (phase 1) or on the host side of CG iteration `iteration` (phase 2).  Every rank's dkmc_update_power_gpu_sparse then
 * returns non-zero (the failing rank its own code, the others 46) instead of blocking in a collective: the ranks agree on the
 * outcome of the local set-up before the first collective, and inside the loop an abort word travels with every all-reduce. */
void dkmc_debug_inject_fault(int phase, int iteration);
/* test aid: one launch of the CG step kernel of iteration `it` over m elements with the stop word preset to done_word; *updated = elements of y it
 * changed (0 / it + 2: all; 1 ... it + 1: none), *done_after = the stop word afterwards (csrc/xt.hip: k_xt_step's iteration-stamped stop word) */
int dkmc_debug_step_stop_word(int m, int it, int done_word, int *updated, int *done_after);

/* Test / measurement aid: the slab-distributed block-CG (csrc/xtb_slab.inc) with nranks VIRTUAL ranks inside this process, on the X left resident
 * by the last single-GPU solve: the same system solved by the one-GPU block-CG and by the distributed loop (shares of the tiles as a sharded
 * assembly builds them, rows owned by lateral slabs, exchanges as device copies), both from a zero start to `tol`.  rel_diff: largest deviation of
 * the two solutions / largest entry; times_us[8]: mean kernel times of virtual rank time_rank (apply, neighbour part, fold, rows, Gram reduction,
 * s x s algebra, step, pack + unpack); xdoubles[3]: doubles a rank receives per sweep in the three exchanges; rows_min_max[2]: rows of the smallest
 * and largest slab.  sweep_cap > 0: measurement run -- the distributed loop stops after that many sweeps, the one-GPU solve is skipped, rel_diff = -1.  Fails if the virtual ranks leave the loop at different sweeps or end with different bits. */
int dkmc_xtb_emulate_slabs(int nranks, int width, double tol, int time_rank, int sweep_cap, double *rel_diff, int *iters_slab, int *iters_ref,
                           double *times_us, long long *xdoubles, int *rows_min_max);

/* Measurement aid: the last slab-distributed block-CG solve or emulation -- exchanges per sweep (3, or 2 d + 3 with dkmc_set_x_slab_poly(1); 2 with
 * one rank), doubles a rank receives per halo exchange of the preconditioned loop (largest over the ranks; the halo share of exchange 3), and
 * nmul_us: the mean duration of one N x panel product of the timed virtual rank (0 when untimed or unpreconditioned).  The times_us[8] classes of
 * dkmc_xtb_emulate_slabs keep their meaning; with the switch on, "rows" includes the fold pass and "pack + unpack" the halo exchanges, and its
 * one-GPU reference runs with dkmc_get_x_poly() instead of 0. */
int dkmc_xtb_slab_last(int *exchanges_per_sweep, long long *halo_doubles_per_exchange, double *nmul_us);

/* Test / measurement aid: the slab-distributed CG on K (csrc/kcg.hip) with nranks VIRTUAL ranks inside this process: the background-potential
 * system of the buffer's current state solved from the buffer's current potential by the one-GPU reference-order loop and by the distributed loop
 * (exchanges as device copies), into scratch copies.  max_abs_diff [V]; times_us[4]: product, update, direction, halo pack + unpack of virtual
 * rank time_rank; halo_rows[2]: doubles received per iteration in the halo exchange (largest over the ranks), rows of the largest slab.
 * iter_cap > 0: measurement run (the distributed loop stops after that many iterations, max_abs_diff = -1). */
int dkmc_kcg_emulate_slabs(dkmc_gpubuf *buf, int N, int N_left, int N_right, double Vd, double high_G, double low_G, int num_metals, int nranks, int time_rank,
                           int iter_cap, double *max_abs_diff, int *iters_slab, int *iters_ref, double *times_us, long long *halo_rows);

/* Test aid: the slab partition both distributed loops share (csrc/slab.h, csrc/slab_plan.h), on a pattern the caller supplies -- the host functions
 * of slab.h exactly as the loops call them (one partition step, the count table to the host, rows_by_owner, the halo lists of rank v), with K's row
 * pointer type (X's instantiation differs in that type only), on buffers of its own: nothing a solve reads is touched.  All arrays are host arrays.
 * In: m rows with the CSR pattern rp[m + 1] / ci[rp[m]] (columns in [0, m); bit 31 of a column word is ignored, as in K), of which rows >= first
 * are distributed; coord[m - first] the lateral coordinate of row first + i, binned over lo ... hi; nr ranks (1 ... 32); mark[m] (may be null):
 * rows with mark >= 0 are counted per owner; v the rank whose lists are wanted.
 * Out: owner[m] (0 for rows < first), mask[m] (bit d: the row has an entry in a row of owner d != its own; 0 for rows < first), tab[nr * (nr + 2)] =
 * rows per owner | marked rows per owner | hal[s * nr + d] rows of s that d reads, rows_by_owner[m - first] (grouped by owner, ascending inside a
 * group), hsend = the rows v sends, pieces in destination order (sum over d != v of hal[v][d] entries), hrecv = the rows v receives, pieces in
 * source order (sum over s != v of hal[s][v]).  hsend and hrecv may both be null: the table and the per-row outputs only. */
int dkmc_debug_slab_plan(int m, int first, const int *rp, const int *ci, const double *coord, double lo, double hi, int nr, const int *mark, int v,
                         int *owner, unsigned *mask, int *tab, int *rows_by_owner, int *hsend, int *hrecv);

/* Measurement aid: the form the K solve of this buffer's pattern runs on (built by initialize_sparsity) and its window statistics.  info[9]: form
 * (0 CSR positions, 1 blocked, 2 windowed blocked), rows, rows per block, blocks, doubles of the largest window, doubles of all windows, segments of
 * the most fragmented window, segments of all windows, stored column ints. */
int dkmc_kcg_form_info(dkmc_gpubuf *buf, long long *info /* [9] */);
/* Measurement aid: the stored words of the windowed blocked form of this buffer's pattern.  info[3]: bytes of a stored word (4 or 2,
 * dkmc_set_k_window_word_bytes when the pattern was built; 0 when the pattern has no windowed form: the other two are 0 then too), stored words,
 * bytes of the assembled words one product reads (words x word bytes). */
int dkmc_kcg_form_words(dkmc_gpubuf *buf, long long *info /* [3] */);
/* Test aid: the K system a solve of this buffer's state would assemble (rule 0: background potential, 1: CB edge, 2: CB edge on atoms only, with
 * the contacts at VL and VR), on the form the buffer's pattern holds (CSR positions or blocked; the windowed blocked form is refused).  All four
 * arrays are host arrays of m = N - N_left - N_right doubles, row r = site N_left + r: diag_site and rhs_site are the assembled diagonal and
 * right-hand side; t_site = K v_site, formed by ONE launch of the form's own product kernel with unit scaling and a cleared stop word (a row that
 * launch does not write comes back as NaN).  Changes no field of the buffer and nothing a later solve reads. */
int dkmc_debug_k_system(dkmc_gpubuf *buf, int rule, int N, int N_left, int N_right, double VL, double VR, double high_G, double low_G, int num_metals,
                        const double *v_site, double *t_site, double *diag_site, double *rhs_site);
/* Test aid: position, in 16-bit words from the start of its row, of stored entry `entry` of a row padded to `width` (32 or 64) entries in the 2-byte
 * layout of the windowed blocked form (csrc/kbw_plan.h: kbw_halfword_pos); -1 for any other width or an entry outside the row. */
int dkmc_debug_kbw_halfword_pos(int width, int entry);
/* Test aid: caps the segments of a window of the windowed blocked form of K (dkmc_set_k_blocked_large) below its fixed maximum (16) for the
 * patterns built afterwards, so that the builder refuses and the solve falls back to the CSR positions.  cap <= 0 restores 16. */
void dkmc_debug_kbw_segment_cap(int cap);
/* Measurement aid: the last pair sum (dkmc_poisson_gridless_gpu) made with profiling on; fails before the first one.  info[6]: form that ran
 * (dkmc_set_pair_form); kernel that summed (0 k_pairwise, 1 k_pairwise_cells); its workgroups (of the cell-list launch those that own a chunk of
 * sites); lane slots form 0 spends on the expensive part of a term, 64 x the (wave, list entry) steps with at least one site inside the cut-off;
 * lane slots form 1 issued for it, 64 x its batches; 0 (reserved).  The two slot counts are taken by the form-1 kernels and are -1 after a form-0
 * call.  ms[2]: HIP-event time of the whole call (dkmc_stats.pair_ms: compaction, binning and sum) and of the sum kernels alone. */
int dkmc_get_pair_sum_info(long long *info /* [6] */, double *ms /* [2] */);
/* Test aid for the chained transient sub-steps of the local heat model (dkmc_set_heat_form(1), csrc/heat.hip).  on = 0: every sub-step is polled by
 * the host (the chain is off); on != 0 (default): chained.  budget > 0 fixes the iterations enqueued per chained sub-step (default 0: 64 for the first
 * batch, then the largest count seen, rounded up to a multiple of 8, plus 8), so that a budget below what a solve needs forces the resume path.
 * The temperatures are the same bits either way. */
void dkmc_debug_heat_chain(int on, int budget);
/* Test aid of dkmc_find_clusters (csrc/clusters.hip): the cap on the labelling's rounds, 1 ... 4096; cap <= 0 restores the default 64.  A labelling
 * that needs more rounds than the cap fails with a message instead of delivering labels.
 * Measurement aid: with dkmc_set_profiling(1), ms2 = HIP-event time of the last call's membership pass + labelling rounds (the host's read-backs
 * between them included) and of its summaries (per-root atomics, scan, table, info); both 0 with profiling off. */
void dkmc_debug_set_cluster_round_cap(int cap);
int dkmc_debug_get_cluster_times(double *ms2);
/* Test and measurement aid of dkmc_find_gaps (csrc/gaps.hip): on != 0 (default) a searching member skips every neighbour cell whose members all
 * carry its own node (a per-cell word, recomputed every round: inside the contact slabs whole cells are one node); 0: every cell is scanned.  What
 * it saves are the reads of those members' node words -- a pair of one node is never distance-tested --, so the results, info8[5] included, are
 * the same bytes either way. */
void dkmc_debug_set_gap_cell_skip(int on);
/* Test aid of dkmc_find_paths (csrc/paths.hip): the cap on the search's rounds, 1 ... 4096; cap <= 0 restores the default 4096.  A search that
 * needs more rounds than the cap fails with a message, sets both hop arrays to -1 and leaves the getters failing.
 * Measurement aid: with dkmc_set_profiling(1), ms2 = HIP-event time of the last call's seeding + search rounds (the host's read-backs between
 * them included) and of its summaries (outputs, profile, predecessors, walk); both 0 with profiling off. */
void dkmc_debug_set_path_round_cap(int cap);
int dkmc_debug_get_path_times(double *ms2);
/* Test aid of dkmc_track_clusters (csrc/track.hip): mode 0 (default) = the rule, a key starts probing at its hash; mode 1 = every key starts
 * probing at the last slot of the pair table, so that the longest chains and the wrap-around are exercised.  The capacity is unchanged, so every
 * insert still ends; the results are the same bytes either way.
 * Measurement aid: with dkmc_set_profiling(1), ms2 = HIP-event time of the last call's pair pass (with the clearing of its table) and of
 * everything after it (lineage, codes, scans, tables); both 0 with profiling off. */
void dkmc_debug_set_track_hash(int mode);
int dkmc_debug_get_track_times(double *ms2);
/* Test aid of the cut-site analysis (csrc/cuts.hip): the cap on the rounds of its off-path labelling, by default 64 as for the filament analysis
 * (<= 0 restores the default; at most 4096).  A labelling that needs more rounds than the cap fails with a message, sets both site arrays to -1
 * and leaves the getters failing.
 * Measurement aid: with dkmc_set_profiling(1), ms2 = HIP-event time of the last call's off-path labelling rounds (the host's read-backs between
 * them included) and of everything else (positions, validation, attachment, roles, scans, tables); both 0 with profiling off. */
void dkmc_debug_set_cut_round_cap(int cap);
int dkmc_debug_get_cut_times(double *ms2);
/* Test aid of the min-cut analysis (csrc/flow.hip): the cap on the rounds of ONE of its searches, 1 ... 4096; cap <= 0 restores the default 4096.
 * A search that needs more rounds than the cap fails with a message, sets both site arrays to -1 and leaves the getters failing.
 * Measurement aid: with dkmc_set_profiling(1), ms3 = HIP-event time of the last call's strand searches (seeding, rounds with the host's read-backs,
 * predecessor passes and the one-thread walks), of its two closing searches (the one that finds no exit and the mirrored one; 0 at status 2 and
 * 3) and of the tables with their copy-out; all 0 with profiling off. */
void dkmc_debug_set_flow_round_cap(int cap);
int dkmc_debug_get_flow_times(double *ms3);
/* Measurement aid of the event phase (csrc/events.hip): with dkmc_set_profiling(1), ms2 = HIP-event time of k_ev_build and of the rate census
 * (dkmc_set_event_census; 0 when none ran) of the last dkmc_execute_kmc_step_gpu that built a table; both 0 before the first such call. */
int dkmc_debug_get_event_times(double *ms2);
/* Test aid of the event loop (csrc/events.hip): the PRODUCTION loop k_ev_loop on a table the caller supplies, so that a test can feed rates whose
 * sums are exact (through dkmc_execute_kmc_step_gpu every rate comes out of exp()).
 * resume == 0: d_ev_prob_in [N * nn] (device) is copied into the engine's own table; the row sums are formed by the row_sum() the loop's repair uses,
 *   the two upper levels of the sum tree by the kernel of the production build; then the loop runs.  The caller's table is only read.
 * resume == 1: the loop alone, on the table and tree the last call (of this aid, with the same N and nn) left behind; d_ev_prob_in is not read.
 * Everything after the table build is the code of dkmc_execute_kmc_step_gpu, and so are the meanings of d_site_element, d_site_charge (device, updated
 * in place), d_freq (device), h_uniform / n_uniform (host; two draws per event, the loop stops with *exhausted_out = 1 before a selection for which
 * 2 * events + 1 >= n_uniform), h_event_log (host, may be null: 4 ints per event -- slot, i, j, type -- room for n_uniform / 2 events),
 * *event_time_out (the waiting time of the last event) and the return code: error 7 when no positive rate is left (the events before it are
 * delivered, *event_time_out is infinite).
 * CONTRACT -- the loop trusts its index, as it may in production, where the index comes from the neighbour search; nothing here validates it:
 *   - every entry of d_neigh_idx [N * nn] lies in [-1, N): the loop dereferences every non-negative entry of the rows of i and j.  The table BUILD
 *     tolerates entries >= N (their rate is 0); the LOOP does not -- it would read and write out of bounds;
 *   - the index is symmetric: j is in row i if and only if i is in row j.  The loop zeroes the slots that target i or j only inside the rows of
 *     the neighbours of i and j;
 *   - the table holds finite values >= 0;
 *   - N * nn < 2^31 (the log holds the slot as an int);
 *   - a call to the aid overwrites the engine's table and tree: it discards a pending resume of dkmc_execute_kmc_step_gpu. */
int dkmc_debug_event_loop(int N, int nn, const int *d_neigh_idx, const double *d_ev_prob_in, int *d_site_element, int *d_site_charge, const double *d_freq,
                          const double *h_uniform, int n_uniform, int resume,
                          int *n_events_out, int *exhausted_out, int *h_event_log, double *event_time_out);

#ifdef __cplusplus
}
#endif
#endif
