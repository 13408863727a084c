/*
 * devicekmc_hip.h -- C ABI of the MI355X (gfx950) KMC-superstep engine.
 *
 * Drop-in boundary for DeviceKMC's GPU path: every entry point below replaces one symbol of the
 * reference's gpu_solvers.h / gpu_buffers.h surface (cited per function, paths relative to
 * /root/reference/src).  Plain C types only: device pointers, sizes and scalars.  The C++ shim
 * include/gpu_solvers.h + include/gpu_buffers.h re-exposes the reference's own names and
 * signatures (GPUBuffers&, std::vector, RandomNumberGenerator&) on top of this header.
 *
 * Conventions
 *  - all pointers named d_* are DEVICE pointers; h_* are host pointers;
 *  - ELEMENT / EVENTTYPE are 4-byte ints with the reference's enum values (utils.h:37-60);
 *  - one process drives one GPU; all work is enqueued on one HIP stream (dkmc_set_stream);
 *  - functions return 0 on success, non-zero HIP/engine error code otherwise; the message is
 *    available from dkmc_last_error().  (The reference prints CUDA errors and carries on,
 *    utils.h:145-153; the shim does the same with the message.)
 */
#ifndef DEVICEKMC_HIP_H
#define DEVICEKMC_HIP_H

#ifdef __cplusplus
extern "C" {
#endif

/* Mirror of the public members of class GPUBuffers (gpu_buffers.h:16-52). */
/* Element arrays hold the 4-byte ELEMENT enum (utils.h:37-44).  A C++ host that has the enum type defines DKMC_ELEMENT_T to it before
 * including this header (include/gpu_buffers.h does): the members then have the reference's own type, `ELEMENT *`, and the
 * reference's call sites (potential_solver.cpp:152, KMCProcess.cpp:269-274) compile unchanged.  Same layout either way. */
#ifndef DKMC_ELEMENT_T
#define DKMC_ELEMENT_T int
#endif
typedef struct dkmc_gpubuf {
    int *site_charge;
    double *site_power, *site_potential_boundary, *site_potential_charge, *site_temperature;
    double *site_CB_edge;
    double *T_bg;
    double *atom_power;
    double *atom_CB_edge;
    double *atom_virtual_potentials;
    int *atom_charge;
    DKMC_ELEMENT_T *site_element;
    DKMC_ELEMENT_T *atom_element;
    double *site_x, *site_y, *site_z;
    double *atom_x, *atom_y, *atom_z;
    DKMC_ELEMENT_T *metal_types;
    double *sigma, *k, *lattice, *freq;
    int *neigh_idx, *site_layer;
    int *Device_row_ptr_d, *Device_col_indices_d;
    int *contact_left_row_ptr, *contact_left_col_indices;
    int *contact_right_row_ptr, *contact_right_col_indices;
    int Device_nnz, contact_left_nnz, contact_right_nnz;
    int num_metal_types_, N_, nn_, N_atom_;
} dkmc_gpubuf;

/* Per-call statistics of the last solver invocations (no reference twin; the reference prints
 * "# CG steps" to stdout, iterative_solvers_gpu.cu:456). */
typedef struct dkmc_stats {
    int cg_iters_K, cg_iters_CB, cg_iters_X;
    double cg_rr_K, cg_rr_CB, cg_rr_X;     /* final ||r||^2 of the scaled system */
    int n_events;                          /* events executed by the last execute_kmc_step */
    int n_charged;                         /* charged sites seen by the last poisson_gridless */
    int N_atom;                            /* atoms found by the last update_power */
    long long X_nnz;
    double psum_last;                      /* sum of rates before the last executed event */
    /* kernel profile (dkmc_set_profiling(1)): HIP-event time of the SpMV launches (A*p) of the last CG solve
     * on X, split into the wave-per-row kernel (long rows) and the 16-lanes-per-row kernel (short rows) */
    double spmv_long_ms, spmv_short_ms;
    int spmv_long_launches, spmv_short_launches;
    long long spmv_long_nnz, spmv_short_nnz;
    int spmv_long_rows, spmv_short_rows;
    /* dense-run mode: k_spmv_segs work items and the matrix entries they cover (spmv_long_ms then times that kernel alone,
     * spmv_short_ms the row kernel that follows it) */
    int spmv_segments, spmv_pad;
    long long spmv_segment_entries;
    /* sharded current solve (dkmc_comm_*): ranks, the segments this rank multiplied in the last solve, doubles per rank in
     * the all-gather (row sums of the owned long rows, padded to the largest share), and (profiling on) the HIP-event time
     * of the sampled exchange steps (row-sum kernel + all-gather) */
    int comm_ranks, comm_local_segments;
    long long comm_count_per_rank;
    double comm_ms;
    int comm_launches, comm_pad;
    /* tiled X: 32 x 256 tiles of the tunnelling block (read once per iteration for both triangles) and the entries of the
     * upper triangle they hold */
    int spmv_tiles, spmv_pad2;
    long long spmv_tile_entries;
    /* tiled X (dkmc_set_x_format(1), the default): stored 32 x 32 sub-blocks of the tunnelling block (8 KiB each; all ranks /
     * this rank), work items of the apply kernel and tiles per item, entries of the neighbour part Xs, size of the tunnelling set;
     * spmv_tiles / spmv_tile_entries then count the 32 x 256 tiles and the entries of the upper triangle they hold */
    long long xt_subblocks, xt_local_subblocks;
    int xt_items, xt_kc;
    long long xt_sparse_nnz;
    int xt_ns, xt_split_launch;           /* 1: sharded solve, the neighbour part of A*p runs on a second stream beside the exchange */
    /* profiling on: HIP-event time of the whole iteration loop of the last CG solve on K (and the iterations it covers), and
     * of the last pair-sum kernel */
    double kcg_ms;
    int kcg_iters_timed, kcg_blocked;      /* kcg_blocked: 1 if the last K solve ran on the blocked form of the pattern (dkmc_set_k_blocked),
                                            * 2 if it ran on the windowed blocked form above 262 144 rows (dkmc_set_k_blocked_large), 0 on the CSR positions */
    double pair_ms;
    long long pair_evaluated;              /* (site, charged site) pairs inside the screening cut-off of the last pair sum (profiling on) */
    long long pair_tested;                 /* pairs whose distance was tested (all N x N_charged without the cell list; the 3 x 3 columns with it) */
    long long xt_records;                  /* records of column partial sums one matrix-vector product writes (= runs; runs / 4 on one GPU, where the four waves of a workgroup share one) */
    long long tcache_bytes;                /* bytes of tunnelling-coefficient cache THIS rank holds (sharded solve on the tiled X: what its tiles read) */
    long long kcg_bytes;                   /* bytes one iteration of the last K solve moves: column/class words (2 B each on the windowed form with dkmc_set_k_window_word_bytes(2)) + the q windows (or one read of q per row) + 14 (15) vector touches */
    int xb_aux, xb_poly_used;              /* 1: the last block solve used the smooth auxiliary columns (dkmc_set_x_aux); degree of the split polynomial preconditioner the last current solve ran (0: plain loop; dkmc_set_x_poly / dkmc_set_x_poly_auto) */
    int xb_width, xb_fallback;             /* block-CG width of the last current solve (1 = single-vector loop); 1 if the block loop lost definiteness and the single-vector loop finished the solve */
    int x_tile_stream, x_tile_f64_rounds;  /* tile values the sweeps of the last block solve's first round streamed: 0 the fp64 store, 1 its fp32 image (dkmc_set_x_tile_f32), -1 the fp64 store because the image could not be allocated; rounds of that solve that ran on the fp64 store (one-GPU loop: all of them at 0 / -1; at 1 only the re-entry rounds after a true-residual check above the stop test) */
    long long x_tile_f32_bytes;            /* bytes of the fp32 image of the tile values (0: none was made) */
} dkmc_stats;

const char *dkmc_last_error(void);
void dkmc_clear_error(void);
const dkmc_stats *dkmc_get_stats(void);

/* kmc_events.cu:15-32 */
int dkmc_get_gpu_info(char *gpu_string, int capacity, int dev);
int dkmc_set_gpu(int dev);
/* stream all kernels are enqueued on (hipStream_t); NULL = the null stream (reference behaviour) */
int dkmc_set_stream(void *hip_stream);
int dkmc_synchronize(void);
/* tolerance of solve_sparse_CG_Jacobi; the reference hard-codes 1e-6 (iterative_solvers_gpu.cu:322) */
void dkmc_set_cg_tolerance(double tol);
/* Domain of the system update_CB_edge_gpu_sparse solves.  0 (default): every site, as potential_solver_gpu.cu:595-694 of the reference
 * snapshot does.  1: atoms only -- links to interstitial sites (DEFECT, OXYGEN_DEFECT) are left out and those sites get CB edge 0.  The
 * reference's own artefacts (X pattern dump timing_2.5nm/fullmatrix_assembly, the 19 currents of timing_7.5nm/output_noguess.txt) were
 * written by a revision that solved on atoms (its host twin still shows `gesv(.., &N_atom, ..)` as a comment, potential_solver.cpp:98):
 * with 1 they are reproduced to every entry / printed digit, with 0 the current is 0.83 % lower. */
void dkmc_set_cb_edge_domain(int atoms_only);
/* Memory the tunnelling-coefficient cache of the current solve may take (one row per vacancy site x one column per inner-contact
 * metal, 8 B each: 27 GB at 9.4e5 sites).  -1 (default): a third of the device memory that is free when the cache is (re)built, between
 * 8 and 128 GiB.  When one row per vacancy does not fit, the contact->trap integrals are evaluated directly while the tiles are filled,
 * every step -- same function, same bits, slower assembly.  Takes effect at the next rebuild of the cache (new bias point / structure). */
void dkmc_set_tcache_budget(long long bytes);
/* Screening cut-off of poisson_gridless_gpu.  A term of the pair sum is q erfc(x) k Q / r with x = r / (sigma sqrt 2); terms beyond
 * x_cut are not evaluated.  Default 6.5 (erfc < 3.8e-20: all omitted terms of a 1e6-site stack together stay below 2e-17 V, under the
 * rounding of the sum and under the last-bit noise of the reference's atomicAdd order).  0: every pair, exactly the terms the reference
 * sums (potential_solver_gpu.cu:908-958) -- for a parity run. */
void dkmc_set_pair_cutoff(double x_cut);
/* The pair sum keeps the grouping of the sites by (y, z) column between calls, keyed on the position / lattice arrays, N, pbc and the
 * cut-off; freeing or re-initialising a GPUBuffers drops it.  A host that rewrites site positions IN PLACE behind the same device pointers
 * (only possible through the raw-pointer entry dkmc_poisson_gridless_gpu; the reference never moves a site) calls this afterwards. */
void dkmc_reset_pair_sum_cache(void);
/* Form of the two sum kernels of the pair sum (csrc/potential.hip).  0 (default): a lane evaluates a term where it tests it, so a wave pays
 * erfc / sqrt / the divisions whenever any of its 64 sites is inside the cut-off.  1: a wave queues the passing (site, charged site) pairs in LDS
 * and evaluates them 64 at a time with every lane busy; the terms are added per site in the same order into the same partial sums, so every
 * potential keeps its bits.  Any other value is kept as 0.  Read at every call of dkmc_poisson_gridless_gpu, on one GPU and on several. */
void dkmc_set_pair_form(int form);
int dkmc_get_pair_form(void);
/* Width s of the block-CG of the current solve on the tiled X (csrc/xtb.hip).  1: the reference's single-vector loop
 * (solve_sparse_CG_Jacobi, iterative_solvers_gpu.cu:309-480: same iterate sequence, same start vector).  2 ... 16: block-CG over s
 * columns -- column 0 carries the physical right-hand side and start vector, columns 1 ... s - 1 fixed-seed auxiliary right-hand sides
 * that only enlarge the Krylov space; every 32 x 32 sub-block of the tunnelling block is streamed ONCE per sweep and multiplied (it and
 * its transpose) into 32 x 16 panels by v_mfma_f64_16x16x4_f64 -- the contraction the reference's unfinished split path applies as a
 * GEMV (add_submatrix_product, iterative_solvers_gpu.cu:634-652).  Same stop test on column 0 (||r||^2 <= tol^2); the solution agrees
 * with the single-vector loop to the stop tolerance, NOT iterate by iterate.  85 071 sites: 666 -> 208 / 133 / 95 sweeps at s = 4 / 8 / 16. */
void dkmc_set_x_block(int s);
int dkmc_get_x_block(void);
/* More than one rank (dkmc_comm_*): 1 (default) distributes the STATE of the block-CG by spatial row slabs -- a rank owns the rows of one lateral
 * slab of the device: neighbour part, Gram pass and panel updates run on its rows only; per sweep the tile sums of the S rows go to their owners
 * (all-to-all-v), 6 x 256 Gram entries are all-gathered and added in rank order, the own rows of Q = S P and the halo rows of P go out
 * (all-to-all-v) (csrc/xtb_slab.inc).  0: the all-gather variant -- only the tile stream is sharded, everything else replicated. */
/* Split polynomial preconditioner of the block-CG of the current solve (csrc/xtb_precond.h): degree d > 0 runs the block loop on L A L with
 * L = p(N), p the degree-d Chebyshev interpolant of (1 - x)^(-1/2) on [-1, 1 - min(0.5, 1.6 / d^2)], N = I - (neighbour part + diagonal of the
 * Jacobi-scaled X).  A sweep then costs 2 d more sparse panel products and the loop needs 2-3x fewer sweeps (tools/precond_block_proto.py); the start
 * vector enters through the right-hand side L (b - A y0), the result meets the reference's stop test in the TRUE residual (checked, the loop is
 * re-entered if it does not).  d in 0 ... 16 (clamped), 0 = off; base degree 8.  Applies to the one-GPU loop; the slab-distributed loop of more than one
 * rank carries it only with dkmc_set_x_slab_poly(1), at the base / pinned degree.
 * By default (dkmc_set_x_poly_auto(1)) the one-GPU loop takes its degree from the rows of the system: a step function measured on steady warm-started
 * steps (profiles/x_poly_degree_by_size.jsonl) -- the N products weigh less in a sweep the larger the tile pass is, so larger systems run a
 * higher degree.  dkmc_set_x_poly(d) pins d (d > 0) or turns the preconditioner off (0) and clears the rule; dkmc_set_x_poly_auto(1) turns the rule
 * back on (a base degree of 0 returns to 8).  dkmc_get_x_poly(): the pinned or base degree; dkmc_stats.xb_poly_used: the degree the last solve ran. */
void dkmc_set_x_poly(int degree);
int dkmc_get_x_poly(void);
void dkmc_set_x_poly_auto(int on);
int dkmc_get_x_poly_auto(void);
/* Form of the one-GPU preconditioned loop.  The split form pays 2 d N products per sweep for p^2, a polynomial of degree 2 d with d free parameters.
 * The one-polynomial form takes M^-1 = q(N), q the degree-n Chebyshev interpolant of (1 - x)^-1 on [-1, 1 - min(0.5, 3.2 / n^2)], n = n(d) ~ 1.25 d
 * (at most 20), and runs the same block-CG in the variables Pt = L P, Rt = L^-1 R, so that no L is ever applied: n N products per sweep, the iterate
 * already in the unpreconditioned space, the same true-residual check and re-entry (csrc/xtb.hip: k_xtb_gram1, k_xtb_step1).
 * 0: split form everywhere, bit for bit the loop on L A L.  1: one polynomial in every preconditioned one-GPU solve.  2 (default): one polynomial where the degree comes from the size
 * rule (dkmc_set_x_poly_auto(1)), split form where dkmc_set_x_poly(d) pinned a degree.  The slab-distributed and sharded loops keep the split form.
 * dkmc_get_x_poly_form_used(): 1 if the last one-GPU block solve ran the one-polynomial form; dkmc_get_x_poly_products(): its N products per sweep
 * (2 d, n(d), or 0 for the plain loop).  dkmc_stats.xb_poly_used keeps reporting the level d. */
void dkmc_set_x_poly_form(int form);
int dkmc_get_x_poly_form(void);
int dkmc_get_x_poly_form_used(void);
int dkmc_get_x_poly_products(void);
/* Stop test of the one-polynomial form.  Its loop works with Rt and Z = q(N) Rt and tests (Rt'Z)_00 <= tol^2 min q, which BOUNDS what the contract
 * names -- ||Rt(:, 0)||_2 <= tol on the Jacobi-scaled system -- and so solves further than asked.
 * dkmc_set_x_stop_form(0): that bound alone, bit for bit the loop without the feature.  1: beside it the norm itself, ||Rt+(:, 0)||_2 <= kappa tol, from partial sums the panel-step
 * kernel writes for its rows and one workgroup adds in a fixed order (csrc/xtb.hip: k_xtb_step1, k_xtb_stop_norm; no atomics); whichever fires first
 * ends the loop.  First round of a one-GPU one-polynomial solve only: the true-residual check behind the loop and the re-entry rounds (which stop on
 * the bound alone) are as before; the split form, the plain, sharded and slab loops are untouched.  2 (default): 1 for systems of 96 000 rows and
 * more, 0 below -- where it was measured to pay (profiles/ab_bench_x_stop_form.txt): at 9.4e5 sites 36.05 -> 30.9 sweeps per step.  Other
 * values select 0.  Solutions under 1 differ from those under 0 within the stop test (I_macro by 1.4e-7 relative at 9.4e5 sites); events are the same.
 * dkmc_set_x_stop_margin(kappa): kappa in (0, 1], default 1 (anything else restores it) -- the largest of {1, 0.8, 1 / 1.5} without a re-entry round over
 * 100 steps at 9.4e5 sites; a smaller one leaves slack for the fp32 tile image's perturbation (the true residual exceeded the norm by 1 % at the most).
 * dkmc_get_x_stop_info, for the last round of the last one-polynomial solve (returns 1 and fired = 0 where there was none): fired 1 = the bound (or a
 * breakdown) ended it, 2 = the norm test; norm = ||Rt(:, 0)|| at the stop (-1 under form 0: not measured); rz = (Rt'Z)_00 there; true_residual =
 * ||A y - b|| of column 0 from the pass behind the loop.  Any pointer may be null. */
void dkmc_set_x_stop_form(int form);
int dkmc_get_x_stop_form(void);
void dkmc_set_x_stop_margin(double kappa);
double dkmc_get_x_stop_margin(void);
int dkmc_get_x_stop_info(int *fired, double *norm, double *rz, double *true_residual);
/* How the preconditioner's N products read N: 1 (default) from a copy packed once per solve -- slices of four rows as wide as their longest row,
 * the column's scaling folded into the weights (csrc/xtb_precond.h: k_xtb_npack, k_xtb_nmulp16 / k_xtb_nmulp); 0 from the CSR of the neighbour part (k_xtb_nmul).
 * Both give the same bits; 0 is kept for comparisons. */
void dkmc_set_x_nmul_form(int form);
int dkmc_get_x_nmul_form(void);
/* Tile values inside the sweeps of the preconditioned block-CG.  1 (auto, default): on one GPU with block width > 1 and dkmc_set_x_poly > 0 the
 * assembly keeps a float image of every stored tunnelling entry beside the fp64 store (4 KiB per 32 x 32 sub-block), and at cg_tol >= 1e-8 the
 * sweeps stream that image and widen it to fp64 in front of the matrix instructions; accumulation and everything downstream stay fp64.  The
 * rounding perturbs A = S X S symmetrically by at most 2^-24 |At| (1e-10 of ||A||: the tunnelling block is 2e-3 of it); the diagonal, the
 * scaling, the first product A y0 and the TRUE residual that ends every solve use the fp64 store, and a solve whose check fails is re-entered
 * on the fp64 store: the result meets the reference's stop test on column 0 as before, not bit for bit.  Below 1e-8, with the preconditioner
 * off, at width 1, on more than one rank, or when the image does not fit in memory the loop is the fp64 one, bit for bit (dkmc_stats.x_tile_stream).
 * 0: never. */
void dkmc_set_x_tile_f32(int mode);
int dkmc_get_x_tile_f32(void);
/* Opt-in: sweeps that skip the tunnelling tiles too small to matter.  theta > 0: wherever the sweeps stream the fp32 image above (one GPU, block
 * width > 1, dkmc_set_x_poly > 0, tol^2 >= 1e-16, an image exists) they stream a COMPACTED image that holds only the LIVE tiles -- stored 32 x 256
 * tiles with at least one stored entry of sc_i |v_ij| sc_j >= theta (sc: the Jacobi scaling of the solve, v: the fp64 stored value) -- on a launch
 * view of its own (census, scan, compaction and view once per solve: csrc/xt_live.h).  The tile x panel kernel is the same.  The first product A y0,
 * the diagonal, the scaling, the TRUE residual that ends every solve and every re-entry round keep the full fp64 store, and the start vector goes
 * through the right-hand side, so the dropped entries act on the correction only; a solve whose check fails is re-entered on the fp64 store.  The
 * stored X is unchanged (dkmc_get_last_X).  When fewer than 1 / 64 of the stored sub-blocks would go, or the compact buffer does not fit, the
 * existing image and views are streamed (never an error).  IGNORED by the slab-distributed and sharded loops, at width 1, with dkmc_set_x_poly(0)
 * and with dkmc_set_x_tile_f32(0).  0 (default) = off: every solve as without the switch, bit for bit.  theta <= 0 or NaN turns it off; values
 * above 1e-4 are kept as 1e-4; recommended 1e-10.  Read at every current solve.  What the last solve did: dkmc_get_x_tile_live_info
 * (devicekmc_hip_debug.h). */
void dkmc_set_x_tile_drop(double theta);
double dkmc_get_x_tile_drop(void);
/* Opt-in: what dkmc_set_x_tile_drop drops.  0 (default): whole tiles, as described above -- every solve exactly as without this switch, bit for bit.
 * 1: SUB-BLOCKS.  A stored 32 x 32 sub-block is live when one of its stored entries has (sc_i |v_ij|) sc_j >= theta (fp64 stored value, this order
 * of the multiplications); a tile is live when one of its sub-blocks is, so the set of live tiles is the same in both units; the compact image and
 * the launch view hold only the live sub-blocks of the live tiles (a live tile keeps its cell and carries a reduced mask).  A dropped sub-block
 * loses its row sums and its column sums together -- both triangles come from the one stored value --, so the streamed operator stays symmetric,
 * and every dropped entry is below theta, as with whole tiles.  The tile x panel kernel is the same; everything that keeps the full fp64 store
 * above keeps it here.  Any other value is stored as 0.  Read at every current solve.  Without effect while dkmc_set_x_tile_drop is 0 and wherever
 * that switch is ignored (slab-distributed and sharded loops, width 1, dkmc_set_x_poly(0), dkmc_set_x_tile_f32(0), tol^2 < 1e-16).  The "fewer
 * than 1 / 64 of the stored sub-blocks would go" rule counts the sub-blocks this unit would drop.  What it is worth: DESIGN.md section 6. */
void dkmc_set_x_tile_drop_unit(int unit);
int dkmc_get_x_tile_drop_unit(void);
/* AUTO MODE of the live view, on by default.  While dkmc_set_x_tile_drop is 0 (an explicit threshold applies as described there, cold starts
 * included), a current solve runs its sweeps on the live tiles at 1e-10 when (a) it starts from the previous solution (dkmc_set_current_warm_start(1)
 * and the copy of matching size was loaded: from a zero start the dropped part acts on the whole solution and costs an fp64 re-entry round) and (b) the
 * stored X has at least the measured number of sub-blocks from which the live view pays for its per-solve census and compaction
 * (profiles/x_tile_drop_by_size.jsonl).  Below the gate, from a zero start and wherever dkmc_set_x_tile_drop is ignored every
 * solve is as with auto mode off, bit for bit.  dkmc_set_x_tile_drop_auto(0) switches it off: the full view everywhere unless a threshold is set.
 * dkmc_get_x_tile_drop_used: the threshold the sweeps of the LAST current solve ran on, 0.0 for the full view.  After a solve on the live view the
 * dkmc_stats fields xt_local_subblocks, spmv_tiles, xt_items and xt_records carry the live view's counts (what a sampled tile launch streamed);
 * xt_subblocks, spmv_tile_entries and X_nnz always describe the stored X. */
void dkmc_set_x_tile_drop_auto(int on);
int dkmc_get_x_tile_drop_auto(void);
double dkmc_get_x_tile_drop_used(void);
/* Order of the tunnelling set S and the tunnelling tiles kept across current solves (csrc/xt_static.h).  0: S in atom order (the reference's: left
 * contact, vacancies, right contact) and every stored sub-block generated at every solve, bit for bit as without the switch.  1: on wherever it
 * can be -- one GPU, not sharded, not slab-distributed, the tiled X (dkmc_set_x_format(1)); everywhere else S keeps atom order and the fill is
 * full, as with 0.  2 (default): as 1, from the measured size on -- a tunnelling set of at least 32 768 members (between the benchmark's tile:5
 * and tile:6; below it the new order ties or loses: DESIGN.md section 6); smaller systems as with 0.
 * On: S = [inner-contact metals in atom order | vacancies in atom order].  With nM metals the column strips w < nM / 256 of the tile store hold
 * contact x contact entries only, which depend on the metals' positions and CB edges and on nothing an event changes; they are a prefix of the
 * tile list, of the fp64 store and of its fp32 image.  After a solve the library keeps that prefix and, at the next solve, generates only the
 * tiles behind it -- provided the metals (count, positions, CB edges, flags: compared bitwise on the device), the parameters the entries
 * depend on, the two allocations and the tile-list prefix itself are what they were.  Anything else is a full fill; a failed solve keeps
 * nothing.  The stored X is the same set of entries with the same values as in atom order; sums over a row of T run in the new order, so results
 * agree to rounding, not bit for bit (dkmc_get_last_X exports rows by system row in either order).  Any other value selects 2.  Read at every
 * current solve.  dkmc_get_x_static_info, for the last current solve: info8[0] 1 = S was in metals-first order; [1] strips that can be kept
 * (nM / 256); [2] tiles kept; [3] tiles filled; [4] sub-blocks kept; [5] sub-blocks filled; [6] why nothing was kept: 0 = the prefix was kept,
 * 1 first solve on this GPUBuffers (or the one before it failed), 2 metals changed, 3 parameters changed, 4 store moved, 5 image changed
 * (made now and not before, or the reverse), 6 tile-list prefix differs, 7 not applicable (atom order, or fewer than 256 metals); [7] the
 * self-check of devicekmc_hip_debug.h: -1 not run, else the number of differences it found. */
void dkmc_set_x_static_tiles(int mode);
int dkmc_get_x_static_tiles(void);
int dkmc_get_x_static_info(long long *info8);
/* How the packed N products (dkmc_set_x_nmul_form(1)) gather the panel rows: 16 (default) takes two slots of a matrix row per instruction, 16 bytes
 * per lane on eight lanes each (k_xtb_nmulp16); 8 one slot, 8 bytes per lane on sixteen lanes (k_xtb_nmulp).  Same packed N; every element is formed
 * by the same sequence of fp64 operations: the same bits.  8 is kept for comparisons; any other value selects 16. */
void dkmc_set_x_nmul_lane_bytes(int bytes);
int dkmc_get_x_nmul_lane_bytes(void);
/* Where the packed 16-byte N products (k_xtb_nmulp16) take their panel operands from.  The windowed form (k_xtb_nmulw; csrc/nwin_plan.h) cuts the rows
 * into blocks of 320, copies a block's window -- the block and a halo on either side, at most 76 KiB, so that two workgroups share a CU -- from the
 * input panel into LDS once and serves every slot whose column lies inside it from there; the other slots gather from memory as before.  Every
 * element is formed by the same sequence of fp64 operations on the same operands: the same bits.  0 = off, 1 = on wherever the packed 16-byte form
 * runs on one GPU (the row-list products of the slab-distributed loop keep k_xtb_nmulp16), 2 (default) = by size: systems of at least the measured
 * number of rows (csrc/xtb_precond.h: xb_nwin_rows).  Any other value selects 2.  Read when a solve packs N. */
void dkmc_set_x_nmul_window(int mode);
int dkmc_get_x_nmul_window(void);
void dkmc_set_x_slab(int on);
int dkmc_get_x_slab(void);
/* Opt-in: 1 runs the slab-distributed block-CG (dkmc_set_x_slab(1), more than one rank) on L A L with the degree and the coefficients of the one-GPU
 * loop (dkmc_get_x_poly() > 0; 0 leaves it plain).  Every N product runs on the rank's own rows -- each row formed as on one GPU, bit for bit -- with
 * one halo exchange of its input before it: 2 d + 3 exchanges per sweep instead of 3 (csrc/xtb_slab.inc).  Same solution to rounding, about the
 * sweep count of the one-GPU preconditioned loop, the same bits on every rank; the true residual is checked at the end and the solve re-entered as
 * on one GPU; no auxiliary columns are kept for the next solve.  Unchanged by it: the all-gather variant (dkmc_set_x_slab(0)) and a communicator
 * of one rank (both run the plain loop).  Default 0. */
void dkmc_set_x_slab_poly(int on);
int dkmc_get_x_slab_poly(void);
/* More than one rank, K system above the size of the blocked form (262 144 rows): 1 (default) distributes the CG on K (background potential, CB
 * edge) by the same lateral row slabs -- product, update and direction on the own rows, the two dot products of an iteration completed by
 * all-gathers of block partials added in one fixed order on every rank, the halo of the scaled direction by an all-to-all-v (csrc/kcg.hip;
 * SURVEY 8e row "K-CG").  0: the solve is replicated on every rank. */
void dkmc_set_k_slab(int on);
int dkmc_get_k_slab(void);
/* Auxiliary right-hand sides of the block-CG (a free choice: only their block Krylov space matters; column 0 is always the physical system).
 * 0: fixed-seed hash of (row, column), uniform in [-1, 1).  1: smooth set, column v = cos(v pi xi) / s with xi the atom's x coordinate scaled to
 * [0, 1] -- rich in the low modes of the neighbour part of X: 20-35 % fewer sweeps at the default tolerance.  2 (default): the smooth set at
 * tolerances of 1e-8 and looser, the hash set below (smooth systems converge before the physical column does and the s x s systems then lose
 * rank close to a converged tolerance).  No counterpart in the reference. */
void dkmc_set_x_aux(int mode);
int dkmc_get_x_aux(void);
/* With dkmc_set_current_warm_start(1).  1: the auxiliary columns of the hash set start from the solutions the previous solve left for them (their
 * right-hand sides never change), and at tolerances of 1e-8 and looser the set is half smooth (zero start) + half hash (warm): the residuals the
 * warm columns start with carry what the previous solve had not resolved yet.  0 (default): every auxiliary column starts from zero.  On the
 * oracle's X of the 2.5 nm device the warm auxiliary start halves the sweeps (33 -> 16-19, tools/warm_aux_proto.py); measured on the GPU it gains
 * nothing from 85 k sites up (profiles/r05_ab_aux_warm.json: 9.4e5 sites 435 -> 425-445 sweeps), hence off.  Column 0 and the contract
 * (solution within the stop test) are unaffected either way. */
void dkmc_set_x_aux_warm(int on);
int dkmc_get_x_aux_warm(void);
/* 1 (default): initialize_sparsity also builds the blocked form of the K pattern (csrc/kcg.hip) for systems of up to 262 144 device rows:
 * the CG on K (background potential, CB edge: solve_sparse_CG_Jacobi on K, iterative_solvers_gpu.cu:309-480) then runs in an internal
 * x-sorted row order, one block of rows per CU with its window of the direction vector in LDS; site order outside the solve is untouched.
 * 0: the solve uses the CSR positions of the pattern (the only form above that size).  Read when a pattern is built. */
void dkmc_set_k_blocked(int on);
int dkmc_get_k_blocked(void);
/* 0 (default): above 262 144 device rows the CG on K runs on the CSR positions of the pattern.  1: initialize_sparsity builds the WINDOWED blocked
 * form for such patterns instead (csrc/kcg.hip, kbw_plan.h): rows in an internal spatial order (lateral columns of one neighbour distance in
 * serpentine order, x within a column), blocks of rows whose window of the direction vector -- a few contiguous segments of that order -- is
 * copied into LDS, and the K solve of the pattern runs there on one GPU (dkmc_stats.kcg_blocked = 2); nullptr-safe: a pattern whose windows do
 * not fit falls back to the CSR positions.  Takes effect with dkmc_set_k_blocked(1) (the default); systems up to 262 144 rows keep the blocked
 * form whatever this says, and the slab-distributed K loop (more than one rank attached) stays on the CSR positions.  Read when a pattern is built. */
void dkmc_set_k_blocked_large(int on);
int dkmc_get_k_blocked_large(void);
/* Bytes of a stored word of the windowed blocked form (dkmc_set_k_blocked_large(1), above 262 144 rows, one GPU).  4 (default): one int per stored
 * entry.  2: 16 bits per entry -- the entry is an offset into the block's LDS window (at most 14 336 doubles: bits 0-13) and the class of the link
 * (bit 15) --, a row of 64 or 128 bytes laid out so that one 16-byte load per lane delivers the entries the lane holds with 4-byte words, in the same
 * slots: every element of the product is formed by the same sequence of fp64 operations, the same bits, half the column bytes.  Any other value
 * selects 4.  Nothing else changes: the blocked form up to 262 144 rows, the CSR positions and the slab-distributed K loop keep their words;
 * dkmc_stats.kcg_blocked stays 2.  Read when a pattern is built. */
void dkmc_set_k_window_word_bytes(int bytes);
int dkmc_get_k_window_word_bytes(void);
/* Start vector of the current solve.  1 (default): the previous step's solution, from a private unscaled copy kept per GPUBuffers -- what
 * the reference's own comment asks for ("use the previous solution as the initial guess", current_solver_gpu.cu:976-977).  0: whatever
 * gpubuf.atom_virtual_potentials holds, exactly as the reference code does -- and that buffer was scaled by G0 in place after the previous
 * solve (current_solver_gpu.cu:1013-1016), so the reference starts from G0*m, i.e. practically from zero: the reference-order switch
 * (with dkmc_set_x_block(1): the reference's iterate sequence).  Either way the contract is the solution within the stop test; the first
 * solve of a run starts from the buffer in both modes.  dkmc_get/set_current_warm_vector export and restore the private copy (restart). */
void dkmc_set_current_warm_start(int mode);
int dkmc_get_current_warm_start(void);
int dkmc_get_current_warm_vector(const dkmc_gpubuf *buf, double *h_out, int capacity, int *n_out);
int dkmc_set_current_warm_vector(const dkmc_gpubuf *buf, const double *h_in, int n);
/* the same for the solutions of the block-CG's auxiliary columns (dkmc_set_x_aux_warm): [rows][16] doubles */
int dkmc_get_current_warm_aux(const dkmc_gpubuf *buf, double *h_out, long long capacity, long long *n_out);
int dkmc_set_current_warm_aux(const dkmc_gpubuf *buf, const double *h_in, long long n);
/* 1: bracket every SpMV launch of the CG solves with HIP events on the engine's stream and accumulate
 * their durations into dkmc_stats (measurement aid for bench.py; off by default) */
void dkmc_set_profiling(int on);
/* layout of the current-solve matrix X (update_power_gpu_sparse).  1 (default): tiled X -- the neighbour part as a small CSR,
 * the tunnelling block generated straight into symmetric 32 x 256 tiles (upper triangle only, no column indices, one copy);
 * per-rank storage and assembly when a communicator is attached.  0: CSR X exactly as the reference stores it
 * (Assemble_X_sparsity / Assemble_X2), solved by reading every stored entry; both agree to rounding.  dkmc_get_last_X
 * returns the same column-sorted CSR in both modes. */
void dkmc_set_x_format(int tiled);
int dkmc_get_x_format(void);

/* ---- GPUBuffers (gpu_buffers.h:73-158, gpu_buffers.cpp:10-118) ---------------------------- */
/* allocates every array of the struct with hipMalloc and uploads the constant ones */
int dkmc_gpubuf_create(dkmc_gpubuf *buf, int N, int N_atom, int nn, int num_metal_types,
                       const int *h_site_layer, const double *h_site_x, const double *h_site_y,
                       const double *h_site_z, const int *h_neigh_idx, const int *h_metals,
                       double freq, double sigma, double k, const double *h_lattice);
int dkmc_gpubuf_free(dkmc_gpubuf *buf);
/* sync_HostToGPU / sync_GPUToHost: the nine arrays of gpu_buffers.cpp:10-55 */
int dkmc_gpubuf_sync_host_to_gpu(dkmc_gpubuf *buf, const int *h_site_element, const int *h_site_charge,
                                 const double *h_site_power, const double *h_site_CB_edge,
                                 const double *h_site_potential_boundary, const double *h_site_potential_charge,
                                 const double *h_site_temperature, const double *h_atom_CB_edge, double T_bg);
int dkmc_gpubuf_sync_gpu_to_host(const dkmc_gpubuf *buf, int *h_site_element, int *h_site_charge,
                                 double *h_site_power, double *h_site_CB_edge,
                                 double *h_site_potential_boundary, double *h_site_potential_charge,
                                 double *h_site_temperature, double *h_atom_CB_edge, double *T_bg);
int dkmc_copy_power_from_gpu(const dkmc_gpubuf *buf, double *h_power);          /* gpu_buffers.cpp:58-72 */
int dkmc_copy_charge_to_gpu(dkmc_gpubuf *buf, const int *h_charge);             /* :88-93 */
int dkmc_copy_Tbg_to_gpu(dkmc_gpubuf *buf, double T_bg);                        /* :75-80 */

/* copytoConstMemory (kmc_events.cu:369-375): per-layer zero-field energies, at most 5 layers */
int dkmc_copy_to_const_memory(const double *h_E_gen, const double *h_E_rec, const double *h_E_Vdiff,
                              const double *h_E_Odiff, int num_layers);

/* ---- neighbour index: Device::constructSiteNeighborList + padding (Device.cpp:98-136, :69-80) ------- */
/* Row i of d_neigh_out[N * nn] holds every j != i with site_dist(i, j) < nn_dist, ascending, -1 padded; nn = global maximum.
 * Two calls: d_neigh_out == NULL computes nn into *nn_out; the second call fills d_neigh_out using nn = *nn_out. */
int dkmc_build_neighbor_index(int N, const double *d_x, const double *d_y, const double *d_z, const double *h_lattice,
                              int pbc, double nn_dist, int *nn_out, int *d_neigh_out);

/* ---- sparsity of K: initialize_sparsity (iterative_solvers_gpu.cu:96-109) ------------------- */
/* fills Device_*, contact_left_*, contact_right_* of buf (allocated by the library) */
int dkmc_initialize_sparsity(dkmc_gpubuf *buf, int pbc, double nn_dist, int num_atoms_contact);
/* frees the six pattern arrays initialize_sparsity allocated and the solver state kept for this buffer (dkmc_gpubuf_free does both
 * for buffers created by dkmc_gpubuf_create) */
int dkmc_free_sparsity(dkmc_gpubuf *buf);

/* ---- potential ------------------------------------------------------------------------------ */
/* update_charge_gpu (potential_solver_gpu.cu:54-63) */
int dkmc_update_charge_gpu(const int *d_site_element, int *d_site_charge, const int *d_neigh_idx,
                           int N, int nn, const int *d_metals, int num_metals);
/* update_CB_edge_gpu_sparse (potential_solver_gpu.cu:595-694) */
int dkmc_update_CB_edge_gpu_sparse(dkmc_gpubuf *buf, int N, int N_left_tot, int N_right_tot, double Vd,
                                   int pbc, double high_G, double low_G, double nn_dist, int num_metals);
/* background_potential_gpu_sparse (potential_solver_gpu.cu:696-781) */
int dkmc_background_potential_gpu_sparse(dkmc_gpubuf *buf, int N, int N_left_tot, int N_right_tot, double Vd,
                                         int pbc, double high_G, double low_G, double nn_dist,
                                         int num_metals, int kmc_step_count);
/* poisson_gridless_gpu (potential_solver_gpu.cu:960-978) */
int dkmc_poisson_gridless_gpu(int num_atoms_contact, int pbc, int N, const double *d_lattice,
                              const double *d_sigma, const double *d_k,
                              const double *d_posx, const double *d_posy, const double *d_posz,
                              const int *d_site_charge, double *d_site_potential_charge);

/* solve_sparse_CG_Jacobi (iterative_solvers_gpu.cu:309-480): solves A y = x; overwrites A_data
 * (scaled) and x (scaled rhs); y holds the warm start on entry and the solution on exit. */
int dkmc_solve_sparse_CG_Jacobi(double *d_A_data, const int *d_A_row_ptr, const int *d_A_col_indices,
                                int A_nnz, int m, double *d_x, double *d_y, int *iters_out, double *rr_out);

/* ---- KMC events: execute_kmc_step_gpu (kmc_events.cu:146-365) ------------------------------- */
/* solve_sparse_CG_splitmatrix (iterative_solvers_gpu.cu:656-821; unfinished in the reference: it prints the solution and calls
 * exit(1)) with add_submatrix_product (:634-652): UNPRECONDITIONED CG on (A + P^T M P) y = x, A in CSR (m rows), M dense msub x msub
 * (row-major, device), (P v)_k = v[insertion_indices[k] + index_offset] (the reference hard-codes + 2: node = atom + 2).  Loop while
 * ||r||_2 > tol (1e-5 in the source).  A and M are read only; y: start vector in, solution out.  The product's own current solve
 * keeps the dense block as symmetric tiles instead (dkmc_set_x_format(1)); this entry point completes the reference's split API. */
int dkmc_solve_sparse_CG_splitmatrix(const double *d_M, int msub, const double *d_A_data, const int *d_A_row_ptr, const int *d_A_col_indices,
                                     int A_nnz, int m, const int *d_insertion_indices, int index_offset, const double *d_x, double *d_y,
                                     double tol, int *iters_out, double *rnorm_out);

/* The reference draws two numbers per executed event from the host RandomNumberGenerator
 * (kmc_events.cu:221,348).  Here the caller passes the next n_uniform numbers of that stream
 * (h_uniform[2e] selects event e, h_uniform[2e+1] draws its waiting time); *n_events_out tells how
 * many events ran, i.e. 2 * n_events numbers were consumed.  If the stream runs out before the
 * stop criterion (event_time >= 1/freq) is met, *exhausted_out is set and the call can be repeated
 * with more numbers (state is kept in the site arrays).  h_event_log (optional, 4 ints per event):
 * slot index, i, j, event type.  Returns the last event time through *event_time_out. */
int dkmc_execute_kmc_step_gpu(int N, int nn, const int *d_neigh_idx, const int *d_site_layer,
                              const double *d_lattice, int pbc, const double *d_T_bg, const double *d_freq,
                              const double *d_sigma, const double *d_k,
                              const double *d_posx, const double *d_posy, const double *d_posz,
                              const double *d_site_potential_boundary, const double *d_site_potential_charge,
                              const double *d_site_temperature, int *d_site_element, int *d_site_charge,
                              const double *h_uniform, int n_uniform, int resume,
                              int *n_events_out, int *exhausted_out, int *h_event_log, double *event_time_out);
/* build_event_list only (kmc_events.cu:34-126); d_event_type may be NULL */
int dkmc_build_event_list(int N, int nn, const int *d_neigh_idx, const int *d_site_layer,
                          const double *d_lattice, int pbc, const double *d_T_bg, const double *d_freq,
                          const double *d_sigma, const double *d_k,
                          const double *d_posx, const double *d_posy, const double *d_posz,
                          const double *d_site_potential_boundary, const double *d_site_potential_charge,
                          const int *d_site_element, const int *d_site_charge,
                          int *d_event_type, double *d_event_prob);

/* ---- event rates on the local site temperature (opt-in, default 0; csrc/events.hip) ----
 * The reference computes every rate at the one global temperature T_bg: its kinetic term is commented out (Ekin = 0, kmc_events.cu:65,81,99,118;
 * KMCProcess.cpp:99,116,135,156), and so does mode 0, bit for bit.  Modes 1 and 2 let the local heat model reach the vacancy and ion kinetics.
 *   deciding site  For every slot (i, j) that has an event class one site s supplies T_s = d_site_temperature[s]; s is the site the reference's
 *                  commented-out lines name: j for GENERATION, i for RECOMBINATION, VACANCY DIFFUSION and ION DIFFUSION.
 *   mode 0         (default) EA = E0 - En - 0, P = exp(-EA / (kB T_bg)) freq: today's table.  d_site_temperature is never dereferenced and may be NULL.
 *   mode 1         "kinetic", the reference authors' term: Ekin = kB (T_s - T_bg), EA = E0 - En - Ekin, P = exp(-EA / (kB T_bg)) freq.
 *   mode 2         "Arrhenius": EA = E0 - En, P = exp(-EA / (kB T_s)) freq.
 *   identities     Where T_s equals T_bg as a double, modes 1 and 2 give mode 0's P bit for bit, whatever the rest of the field holds.
 *   bad values     Modes 1, 2: an event-class slot whose T_s is not finite or not > 0 gets P = 0 (its type is still written) and is counted in a
 *                  device word.  dkmc_execute_kmc_step_gpu then runs NO event: it returns error 16, the message names the count, site_element and
 *                  site_charge are untouched, *n_events_out = 0 and no random number was consumed.  Modes 1, 2 with d_site_temperature == NULL
 *                  fail with the bad-argument code (13) before any launch.
 *   when           The temperature enters when the table is built; invalidation after an event never recomputes a rate, and a resume call
 *                  (resume != 0) needs nothing new.
 * Values outside 0 ... 2 are taken as 0.  The mode is read at every dkmc_execute_kmc_step_gpu and dkmc_build_event_list(_T).  Modes 1 and 2 are
 * only meaningful where site_temperature is maintained, i.e. with the local heat model (dkmc_update_temperature_local); with global heating only
 * T_bg moves and site_temperature keeps what the host put there.  The library does not second-guess the caller.
 * dkmc_build_event_list_T: dkmc_build_event_list + the temperature and an optional device word d_n_bad, zeroed by the caller, that receives the
 * count of bad-temperature slots (modes 1, 2).  dkmc_build_event_list itself has no temperature: it fails (13) while the mode is not 0. */
void dkmc_set_event_temperature(int mode);
int dkmc_get_event_temperature(void);
int dkmc_build_event_list_T(int N, int nn, const int *d_neigh_idx, const int *d_site_layer,
                            const double *d_lattice, int pbc, const double *d_T_bg, const double *d_freq,
                            const double *d_sigma, const double *d_k,
                            const double *d_posx, const double *d_posy, const double *d_posz,
                            const double *d_site_potential_boundary, const double *d_site_potential_charge,
                            const int *d_site_element, const int *d_site_charge,
                            int *d_event_type, double *d_event_prob, const double *d_site_temperature, int *d_n_bad);
/* Rate census of an event table (csrc/ev_census.hip; no counterpart in the reference): which class carries the total rate and how hot the sites
 * that fire are, computed on the device.  A pure function of the caller's table d_ev_prob[N * nn] (e.g. of dkmc_build_event_list_T).  A LIVE slot
 * has a finite P > 0; its class is recomputed from (site_element[i], site_element[j]) exactly as the table's builder does, s as above.
 *   info16   [0..3]   live slots per class (GENERATION, RECOMBINATION, VACANCY DIFFUSION, ION DIFFUSION), exact integers in doubles;
 *            [4..7]   sum of P per class;
 *            [8..11]  sum of P T_s per class, all 0 when d_site_temperature is NULL: [8 + c] / [4 + c] is the rate-weighted temperature of class c;
 *            [12]     the largest finite P > 0 (0 when there is none), [13] its slot index i nn + c, the smallest among ties, -1 when no slot is live;
 *            [14]     slots with a non-finite P (inf, NaN): excluded from every other entry;
 *            [15]     the total of [0..3].
 * Every sum is added in a fixed order (no floating-point atomics): the same table gives the same bits on every call.
 * dkmc_set_event_census(1) (default 0): every dkmc_execute_kmc_step_gpu with resume == 0 also takes the census of its own table right after the build,
 * before the first event (dkmc_get_event_census_on: the switch); dkmc_get_event_census returns the last one and fails (17) when none has been taken. */
int dkmc_event_rate_census(int N, int nn, const int *d_neigh_idx, const int *d_site_element, const double *d_site_temperature,
                           const double *d_ev_prob, double *h_info16);
void dkmc_set_event_census(int on);
int dkmc_get_event_census_on(void);
int dkmc_get_event_census(double *info16);

/* ---- current / power: update_power_gpu_sparse (current_solver_gpu.cu:854-1147) --------------- */
int dkmc_update_power_gpu_sparse(dkmc_gpubuf *buf, int num_source_inj, int num_ground_ext, int num_layers_contact,
                                 double Vd, int pbc, double high_G, double low_G, double loop_G, double G0,
                                 double tol, double nn_dist, double m_e, double V0, int num_metals,
                                 double *h_imacro, int solve_heating_local, int solve_heating_global, double alpha_disp);
/* Assemble_X_sparsity + Assemble_X2 of the last update_power call, copied to host for inspection
 * (dump_csr_matrix_txt twin, iterative_solvers_gpu.cu:142-169).  Pass NULL pointers to query sizes. */
int dkmc_get_last_X(int *rows_out, long long *nnz_out, int *h_row_ptr, int *h_col, double *h_data);
/* Atom-resolved current map from the solved current system (opt-in, default 0; no counterpart in the reference).  With the switch on, every
 * dkmc_update_power_gpu_sparse call also computes, on the device and from the potentials m exactly as they stay in atom_virtual_potentials when
 * the call returns (G0-scaled, and shifted when heating is on), on both layouts of X and whether or not heating is on:
 *   bond current   J_ic = x_ic (m_i - m_c) for every off-diagonal entry of a row i >= 2 (node i = atom i - 2; nodes 0, 1 are the drivers;
 *                  Nsub = N_atom + 1 rows, the last atom is dropped), site = the atom's site;
 *   thr_all[site]  = 1/2 sum_{c != i} |J_ic| over all columns, the driver columns 0 and 1 included: the current passing through the atom;
 *   thr_tun[site]  = 1/2 sum_{c in T} |J_ic| over the tunnelling block T only (the non-neighbour pairs of S: what the tiles hold; on the CSR
 *                  layout the entries with both ends in S and site_dist >= nn_dist);
 *   net_tun[site]  = sum_{c in T} J_ic, signed.  T is symmetric and has no driver columns, so the sum of net_tun over an atom set A is the
 *                  tunnelling current leaving A (e.g. all sites with x below a plane: the tunnelling current crossing it).
 * Three fp64 arrays of N sites; every entry is written by every call, sites without a row are 0, metal atoms are included (unlike site_power).
 * info8: [0] I_macro (the bits h_imacro received); [1] sum_{c >= 2} x_0c (m_c - m_0), the driver-0 side current; [2] max_i |sum_{c != i} J_ic|
 * over the atom rows (the continuity defect of the solve in amperes); [3] sum thr_all; [4] sum thr_tun; [5] rows covered; [6] tile passes run
 * (2 on the tiled layout with a non-empty S, else 0: one per rule over the fp64 tile store); [7] 0.  All sums are added in a fixed order (no
 * floating-point atomics): two calls on the same state give the same bits; in a sharded solve every rank ends with the same arrays.  Nothing
 * else changes: with the switch off no launch and no allocation is added.  The arrays are kept per GPUBuffers (freed with its solver state);
 * the two getters fail (dkmc_last_error names the call) for a buffer that has had no solve with the switch on.  Any pointer of
 * dkmc_copy_current_map_from_gpu may be NULL. */
void dkmc_set_current_map(int on);
int dkmc_get_current_map(void);
int dkmc_copy_current_map_from_gpu(const dkmc_gpubuf *buf, double *h_thr_all, double *h_thr_tun, double *h_net_tun);
int dkmc_get_current_map_info(const dkmc_gpubuf *buf, double *info8);

/* ---- filament analysis: conducting clusters and contact bridging (csrc/clusters.hip; no counterpart in the reference) ----
 * Connected components of the MEMBER sites over a padded neighbour index, with per-component summaries, contact flags and a bridging verdict, all
 * computed on the device.  A pure function of its arguments: no field of GPUBuffers, no engine state a later phase reads and no other kernel changes.
 *   members     bit mask.  bit 0: metal sites (site_element in d_metals[num_metals]); bit 1: VACANCY sites; bit 2: of the vacancies only the
 *               neutral ones, site_charge == 0 (the set the current solve links with its high conductance).  d_site_charge is read only with bit 2.
 *   link        members u, v are linked when v occurs in row u of the index OR u occurs in row v: symmetric even where the index is not.
 *   index       d_index[N][nn] int32, any nn >= 1, an ARGUMENT: gpubuf.neigh_idx gives the nearest-neighbour filament, an index built by
 *               dkmc_build_neighbor_index at a larger radius a gap-tolerant one.  Entries < 0 (and >= N) are padding, anywhere in a row.
 *   label       d_label[site] (device, N ints, written by the call) = the smallest site index of the site's component, -1 for a non-member:
 *               canonical, independent of the algorithm, its races and the launch geometry.
 *   table       one row per component in ascending order of label: root (= label), size, n_vacancy, flags (bit 0: touches the left contact, bit 1:
 *               the right), xmin, xmax = min / max of d_site_x over the component -- the input doubles themselves (compared through an
 *               order-preserving integer key: -0.0 orders below +0.0; NaN coordinates are not supported).
 *   seeds       left: the members with index < n_left_sites; right: the members with index >= N - n_right_sites (both clamped to 0 ... N).
 *   info8       [0] n_members, [1] n_components, [2] bridged (1: some component has both flag bits), [3] bridge_root (the smallest such root, or
 *               -1), [4] largest_free_size (largest component touching neither contact), [5] rounds (hook + compress rounds the labelling ran,
 *               the one that changed nothing included: what the synchronous model needs, the same on every call), [6], [7] 0.
 *   x3          [0] tip_left_x = max of xmax over the components that touch left and not right (-inf: none), [1] tip_right_x = min of xmin over
 *               those that touch right and not left (+inf: none), [2] gap_x = tip_right_x - tip_left_x, exactly 0.0 when bridged.  (The Euclidean
 *               gap between the two clusters, and the chain of islands between them: dkmc_find_gaps below.)
 * dkmc_find_clusters labels, summarises and keeps table and info of the LAST call in the library; it returns after they are complete.  The
 * labelling runs min-hooking + pointer jumping in rounds from the host, at most 64 rounds (7.5 nm device: 5; a randomly numbered chain of 200 000
 * sites: 12); at the cap the call fails (dkmc_last_error), d_label is set to -1 everywhere and the two getters fail until a call succeeds.
 * dkmc_copy_cluster_table copies the first min(capacity, n_components) rows to host arrays (any may be NULL) and reports them in *rows_out; the
 * true count is info8[1].  Every output is an integer or one of the input doubles: the same inputs give the same bytes on every call. */
enum { DKMC_MEMBERS_METAL = 1, DKMC_MEMBERS_VACANCY = 2, DKMC_MEMBERS_NEUTRAL_ONLY = 4 };
int dkmc_find_clusters(int N, int nn, const int *d_index, const int *d_site_element, const int *d_site_charge, const double *d_site_x,
                       const int *d_metals, int num_metals, int members, int n_left_sites, int n_right_sites, int *d_label);
int dkmc_copy_cluster_table(int capacity, int *h_root, int *h_size, int *h_n_vacancy, int *h_flags, double *h_xmin, double *h_xmax,
                            int *rows_out);
int dkmc_get_cluster_info(int *info8, double *x3);

/* ---- gap analysis: closest pairs, island graph, tunnelling chain (csrc/gaps.hip; no counterpart in the reference) ----
 * Where the filament is not bridged: the Euclidean gap between the two contact clusters, the graph of the islands between them and the chain of
 * hops whose widest one is as narrow as possible, all from per-site work on the device.  A pure function of its arguments: no field of GPUBuffers,
 * no engine state a later phase reads and no other kernel changes.
 *   members     site i is a member when 0 <= d_label[i] < N; its component is the label value (any other value: not a member).  The labels are
 *               those of dkmc_find_clusters, but nothing else of that call is used.
 *   nodes       a component touches the left contact when it has a member with index < n_left_sites, the right one when it has a member with
 *               index >= N - n_right_sites (both clamped to 0 ... N): the rule of the cluster table's flags, recomputed from the labels.  Node L
 *               is the union of the left-touching components, node R of the right-touching ones; a component that touches both makes the device
 *               bridged, and L and R are then one node.  Every other component is a node of its own.
 *   distance    for sites u != v, a = min(u, v), b = max(u, v): dx = x[a] - x[b]; with pbc fy = (y[a] - y[b]) / lattice[1], fy -= round(fy),
 *               dy = fy * lattice[1], and the same for z with lattice[2] (the arithmetic of the reference's site_dist); without pbc the plain
 *               differences.  d2 = (dx * dx + dy * dy) + dz * dz with every product and every sum rounded on its own (no contraction), so that
 *               numpy reproduces the bits.  The library reports d2; the square root is the caller's.  h_lattice (host, 3 doubles) is read with pbc.
 *   edge order  strictly by the key (d2, a, b), lexicographically: crystalline inputs hold exact ties of d2, the tie-break is part of the contract.
 *   candidates  the member pairs whose nodes differ and whose d2 <= r_max * r_max (one rounded product).
 *   island graph  the minimum spanning forest of the nodes over the candidates under that order: unique, whatever computes it.  One row per forest
 *               edge in ascending key order: site_a < site_b, root_a = d_label[site_a], root_b = d_label[site_b], d2.
 *   chain       present when neither contact set is empty, the device is not bridged and L and R lie in one tree: the tree path from L to R, whose
 *               largest hop is the smallest possible over all L -> R paths of the candidate graph.  Rows in order from L to R: from_site (the
 *               end nearer to L), to_site, d2.  Consecutive hops need not share a site: a hop lands anywhere on an island.
 *   direct gap  the smallest candidate between L and R themselves, if one lies within r_max: the Euclidean tip-to-tip gap.
 *   info8       (long long) [0] number of components (distinct labels), [1] forest edges, [2] status: 0 = no chain within r_max or a contact set is
 *               empty, 1 = chain found, 2 = bridged, [3] hops in the chain, [4] rounds (below), [5] distance tests made (a diagnostic: it depends
 *               on the cell grid), [6] direct_a, [7] direct_b (-1, -1: none).
 *   d2x2        [0] bottleneck d2 = the largest hop of the chain; exactly 0.0 when bridged, +inf at status 0.  [1] direct d2, +inf if none.
 * dkmc_find_gaps bins the members into cells of edge >= r_max (a periodic axis may have fewer than 3 cells, r_max may exceed the box: every distinct
 * neighbour cell is visited once) and runs Boruvka rounds: every node picks its smallest candidate by integer atomic minima, the picks are
 * recorded and contracted; a round in which no node has a candidate ends the loop, and rounds counts the rounds run, that one included -- a function
 * of the input alone, at most 32.  It keeps the results of the LAST call in the library and returns after they are complete; the three getters
 * fail (dkmc_last_error) before any successful call.  Any output pointer may be NULL; capacity truncates and *rows_out reports the rows copied (the
 * true counts are info8[1] and info8[3]).  N == 0, or no member at all, succeeds with empty tables and status 0.  N < 0, a null array with N > 0,
 * r_max not finite or <= 0 fail with code 3 before any launch.  No floating-point atomics, no order-dependent sums: the same inputs give the same
 * bytes on every call. */
int dkmc_find_gaps(int N, const double *d_x, const double *d_y, const double *d_z, const double *h_lattice, int pbc,
                   const int *d_label, int n_left_sites, int n_right_sites, double r_max);
int dkmc_get_gap_info(long long *info8, double *d2x2);
int dkmc_copy_gap_edges(int capacity, int *h_site_a, int *h_site_b, int *h_root_a, int *h_root_b, double *h_d2, int *rows_out);
int dkmc_copy_gap_chain(int capacity, int *h_from, int *h_to, double *h_d2, int *rows_out);

/* ---- conduction-path analysis: hops, shortest path, constriction (csrc/paths.hip; no counterpart in the reference) ----
 * Where the filament is bridged: how long the shortest conducting path between the contacts is, which sites lie on a left-to-right walk at most
 * slack links longer, how wide that corridor is level by level, and where it is narrowest.  A pure function of its arguments: no field of
 * GPUBuffers, no engine state a later phase reads and no other kernel changes.
 *   members     site i is a member when 0 <= d_label[i] < N (the rule of dkmc_find_gaps); nothing else of the labels is used.
 *   link        members u and v are linked when v occurs in row u of d_index[N][nn] OR u occurs in row v (the rule of dkmc_find_clusters, symmetric
 *               even where the index is not).  Entries < 0 or >= N are padding, anywhere in a row.
 *   seeds       left: the members with index < n_left_sites; right: the members with index >= N - n_right_sites (both clamped to 0 ... N).
 *   hops        d_hops_left[i] is the smallest number of links from any left seed to i: 0 on a left seed, -1 on a non-member and on a member no left
 *               seed reaches.  d_hops_right is the same from the right seeds.  Device arrays of N int32, always written completely.
 *   status, H   status 1 when some right seed has hops_left >= 0; H is then the smallest such value (= the smallest hops_right over the left seeds).
 *               Otherwise -- an empty seed set, contacts not connected through members -- status 0 and H = -1.
 *   path        at status 1, H + 1 rows: site[H] is the smallest-index right seed with hops_left == H, site[k - 1] the smallest-index member linked
 *               to site[k] with hops_left == k - 1.  Row k has hops_left == k, row 0 is a left seed: canonical, whatever computes it.
 *   corridor    the members with hops_left >= 0, hops_right >= 0 and hops_left + hops_right <= H + slack: exactly the sites on some left-to-right
 *               walk of at most H + slack links.
 *   profile     at status 1, H + slack + 1 rows: row k holds the count of the corridor sites with hops_left == k and xmin, xmax of d_site_x over
 *               them -- the input doubles themselves.  A row with count == 0 holds +inf / -inf; so does every row when d_site_x is NULL.
 *   constriction  the row k in 0 ... H with the smallest count, the smallest k on ties (each of those rows has count >= 1).
 *   info8       (long long) [0] status, [1] H, [2] rounds (below), [3] members reached from the left (hops_left >= 0), [4] from the right,
 *               [5] corridor sites, [6] constriction level, [7] constriction width.  At status 0, [5], [6], [7] are 0, -1, 0.
 * dkmc_find_paths runs a level-synchronous breadth-first search from both contacts at once: round k sets hop k + 1 in both fields in one pass over
 * the member rows; the first round that sets nothing in either field ends the loop, and rounds counts the rounds run, that one included:
 * max(largest hops_left, largest hops_right, 0) + 1, a function of the input alone (0 when N == 0).  A search that needs more than 4096 rounds
 * fails (dkmc_last_error): both hop arrays are then -1 everywhere and the getters fail until a call succeeds.  It keeps the results of the LAST
 * call in the library and returns after they are complete; the three getters fail before any successful call.  Any getter pointer may be NULL;
 * capacity truncates and *rows_out reports the rows copied (the true counts are H + 1 and H + slack + 1).  N == 0, no member or no seed at all
 * succeed with empty tables and status 0.  N < 0, nn < 1, slack < 0 or > 65536, or d_index, d_label, d_hops_left or d_hops_right null with N > 0
 * fail with code 3 before any launch.  Integer atomics only, no order-dependent sums: the same inputs give the same bytes on every call. */
int dkmc_find_paths(int N, int nn, const int *d_index, const int *d_label, const double *d_site_x,
                    int n_left_sites, int n_right_sites, int slack, int *d_hops_left, int *d_hops_right);
int dkmc_get_path_info(long long *info8);
int dkmc_copy_path_sites(int capacity, int *h_site, int *rows_out);
int dkmc_copy_path_profile(int capacity, int *h_count, double *h_xmin, double *h_xmax, int *rows_out);

/* ---- cluster tracking: lineage, merges, splits, rupture sites (csrc/track.hip; no counterpart in the reference) ----
 * Switching is a change between two states: two labellings of one device are compared -- which sites joined or left the clusters, which clusters
 * fused or broke, whether the bridging verdict turned, and at which sites.  A pure function of its arguments: no field of GPUBuffers, no engine
 * state a later phase reads and no other kernel changes.
 *   sides       a(i) = d_label_prev[i] if 0 <= d_label_prev[i] < N, else -1; b(i) the same from d_label_now: the membership rule of dkmc_find_gaps /
 *               dkmc_find_paths.  Any label value in range is a component id; canonical labels are not required.  d_label_prev == d_label_now (the
 *               same pointer) is allowed.
 *   site_change d_site_change[i] (device, N int32, always written completely): 0 a = b = -1; 2 joined (a < 0 <= b); 3 left (b < 0 <= a); 1 stayed on
 *               the main line: a, b >= 0, main_child(a) == b and main_parent(b) == a; 4 regrouped: a, b >= 0 otherwise.
 *   pairs       the distinct (a, b) != (-1, -1), each with count = the number of sites carrying the pair and first_site = the smallest site index
 *               carrying it.  Rows in ascending first_site: canonical, whatever computes it.
 *   now table   one row per distinct b >= 0, ascending: root = b; size = sites with that b; joined = count(-1, b); n_parents = the number of a >= 0
 *               with count(a, b) > 0; main_parent = the a >= 0 with the largest count(a, b), the smallest a on ties, -1 if none; flags: bit 0 touches
 *               the left contact (a member with index < n_left_sites), bit 1 the right one (index >= N - n_right_sites; both clamped to 0 ... N, the
 *               seeds of dkmc_find_clusters), bit 2 BORN (n_parents == 0), bit 3 MERGED (n_parents >= 2), bit 4 FRAGMENT (its main parent has
 *               n_children >= 2).
 *   prev table  the same from the other side: root, size, left = count(a, -1), n_children, main_child (largest count, smallest b on ties, -1 if
 *               none), flags: bits 0, 1 the contact bits on the prev labels, bit 2 DIED (n_children == 0), bit 3 SPLIT (n_children >= 2), bit 4
 *               ABSORBED (its main child has n_parents >= 2).
 *   verdicts    a side is bridged when one of its components has both contact bits; bridge_prev / bridge_now = the smallest such root, or -1.
 *               transition: 0 open -> open, 1 closed (open -> bridged), 2 ruptured (bridged -> open), 3 bridged -> bridged.
 *   critical    at transition 1 the sites with b = bridge_now and a = -1: those whose arrival closed the filament; at transition 2 the sites with
 *               a = bridge_prev and b = -1: those whose loss broke it; otherwise none.  In ascending site index.
 *   x2          [0], [1] = min / max of d_site_x over the critical sites -- the input doubles themselves, compared through the integer key of
 *               dkmc_find_clusters; +inf / -inf with no critical site or d_site_x == NULL.
 *   info16      (long long) [0] prev components, [1] now components, [2] pairs, [3] stayed sites (codes 1 + 4), [4] joined, [5] left, [6] regrouped
 *               (code 4), [7] transition, [8] bridge_prev, [9] bridge_now, [10] BORN rows, [11] DIED rows, [12] MERGED rows, [13] SPLIT rows,
 *               [14] critical sites, [15] 0.
 * dkmc_track_clusters collects the pairs in an open-addressing table of 64-bit keys with at least 2 N slots (a wave whose lanes carry one pair
 * sends one set of atomics), derives both tables from one pass over the pairs and keeps the results of the LAST call in the library; it returns
 * after they are complete.  The four row getters and dkmc_get_track_info fail (dkmc_last_error) before the first successful call.  Any getter
 * pointer may be NULL; capacity truncates and *rows_out reports the rows copied (the true counts are info16[2], [1], [0] and [14]).  N == 0, or no
 * member on either side, succeeds with empty tables, transition 0 and bridge roots -1.  N < 0, N > 2^30, or d_label_prev, d_label_now or
 * d_site_change NULL with N > 0 fail with code 3 before any launch.  Integer atomics only (counts, minima, maxima of packed words), no
 * floating-point arithmetic: the same inputs give the same bytes on every call. */
enum { DKMC_TRACK_LEFT = 1, DKMC_TRACK_RIGHT = 2, DKMC_TRACK_BORN = 4, DKMC_TRACK_MERGED = 8, DKMC_TRACK_FRAGMENT = 16,
       DKMC_TRACK_DIED = 4, DKMC_TRACK_SPLIT = 8, DKMC_TRACK_ABSORBED = 16 };
int dkmc_track_clusters(int N, const int *d_label_prev, const int *d_label_now, const double *d_site_x, int n_left_sites, int n_right_sites,
                        int *d_site_change);
int dkmc_get_track_info(long long *info16, double *x2);
int dkmc_copy_track_pairs(int capacity, int *h_prev, int *h_now, int *h_count, int *h_first_site, int *rows_out);
int dkmc_copy_track_now(int capacity, int *h_root, int *h_size, int *h_joined, int *h_n_parents, int *h_main_parent, int *h_flags, int *rows_out);
int dkmc_copy_track_prev(int capacity, int *h_root, int *h_size, int *h_left, int *h_n_children, int *h_main_child, int *h_flags, int *rows_out);
int dkmc_copy_track_critical(int capacity, int *h_site, int *rows_out);

/* ---- cut-site analysis: the sites every conducting path crosses (csrc/cuts.hip; no counterpart in the reference) ----
 * Where the filament is bridged: which atoms hold it together -- the members whose loss alone opens the device --, from one left-to-right path,
 * per-site work and one more component labelling.  A pure function of its arguments: no field of GPUBuffers, no engine state a later phase reads
 * and no other kernel changes.
 *   members     site i is a member when 0 <= d_label[i] < N (the rule of dkmc_find_gaps); nothing else of the labels is used.
 *   link        members u and v are linked when v occurs in row u of d_index[N][nn] OR u occurs in row v (the rule of dkmc_find_clusters, symmetric
 *               even where the index is not).  Entries < 0 or >= N are padding, anywhere in a row.
 *   seeds       left: the members with index < n_left_sites; right: the members with index >= N - n_right_sites (both clamped to 0 ... N).
 *   cut site    a member v such that, with v deleted, no left seed other than v is connected to a right seed other than v (connected: a walk of
 *               zero or more links over members other than v).
 *   path        d_path (device, path_len int32): the sites p_0 ... p_{L-1} of ANY simple left-to-right path, normally the rows of
 *               dkmc_copy_path_sites: distinct members, row 0 a left seed, the last row a right seed, consecutive rows linked.  It is validated on
 *               the device.  Every cut site lies on it, and the cut set does not depend on which path is given.  Row k sits at position k; the
 *               left seeds hang on a virtual node at position -1, the right seeds on one at position L = path_len.
 *   off-path    the members that are not on the path, and their connected components over the links between them.  d_site_bypass[i] (device, N
 *               int32, always written completely) = the smallest site index of the off-path component of i: canonical; -1 for a non-member and
 *               for a path site.
 *   attachment  the positions an off-path component touches: k for every path site p_k linked to one of its sites, -1 if it holds a left seed,
 *               L if it holds a right seed.  lo and hi are the smallest and the largest of them.
 *   chord       a link between two path sites at positions a < b with b - a >= 2; a path site at k >= 1 that is a left seed gives the chord
 *               (-1, k), one at k <= L - 2 that is a right seed the chord (k, L).
 *   the rule    p_k is a cut site if and only if no off-path component has lo < k < hi and no chord has a < k < b.
 *   site_role   d_site_role[i] (device, N int32, always written completely), the DKMC_CUT_ROLE_ values: 0 non-member; 1 path site that is a cut
 *               site; 2 other path site; 3 bypass: off-path, its component has hi - lo >= 2; 4 side: off-path, its component has an attachment
 *               but spans no position; 5 apart: off-path, no attachment.  At status 0 every member is 5.
 *   path table  path_len rows: site, n_bypass = the number of off-path components with lo < k < hi, chord = 1 if some chord has a < k < b, else 0
 *               (a flag, not a count: a link entered in both rows of the index and one entered in one row give the same bytes), cut = 1 iff
 *               n_bypass == 0 and chord == 0.
 *   bypass table  one row per off-path component with hi - lo >= 2, in ascending root: root (= its d_site_bypass value), size, lo, hi.
 *   neck table  the maximal runs of consecutive cut positions, ascending: first, last, xmin, xmax = min / max of d_site_x over the run's sites --
 *               the input doubles themselves, compared through the integer key of dkmc_find_clusters; +inf / -inf when d_site_x is NULL.
 *   info16      (long long) [0] status: 1 = a path was given and is valid, 0 = empty path (the "not bridged" answer), [1] path_len, [2] cut sites,
 *               [3] necks, [4] length of the longest neck (0: none), [5] its first position, the smallest on ties (-1: none), [6] bypass
 *               components, [7] off-path components in all, [8] off-path members, [9] the largest n_bypass, [10] path positions under a chord,
 *               [11] rounds (below), [12] ... [15] 0.
 * dkmc_find_cuts labels the off-path members by min-hooking + pointer jumping in rounds from the host, as dkmc_find_clusters does, with the same
 * cap; rounds counts the hook + compress rounds run, the one that changed nothing included: what the synchronous model needs, the same on every
 * call (0 when N == 0).  With path_len == 0 it succeeds with status 0: the off-path components (all members) are still labelled, the three tables
 * are empty.  A path that is none fails (dkmc_last_error names the first offending row and what is wrong with it), and so does a labelling that
 * reaches the cap: d_site_role and d_site_bypass are then -1 everywhere and the getters fail until a call succeeds.  It keeps the results of the
 * LAST call in the library and returns after they are complete; the four getters fail before any successful call.  Any getter pointer may be NULL;
 * capacity truncates and *rows_out reports the rows copied (the true counts are info16[1], [6] and [3]).  N < 0, nn < 1, path_len < 0 or > N,
 * d_index, d_label, d_site_role or d_site_bypass null with N > 0, or d_path null with path_len > 0 fail with code 3 before any launch; d_site_x is
 * the only optional array.  Integer atomics only (minima, maxima, counts): the same inputs give the same bytes on every call. */
enum { DKMC_CUT_ROLE_NONE = 0, DKMC_CUT_ROLE_CUT = 1, DKMC_CUT_ROLE_PATH = 2, DKMC_CUT_ROLE_BYPASS = 3, DKMC_CUT_ROLE_SIDE = 4, DKMC_CUT_ROLE_APART = 5 };
int dkmc_find_cuts(int N, int nn, const int *d_index, const int *d_label, const double *d_site_x, int n_left_sites, int n_right_sites,
                   const int *d_path, int path_len, int *d_site_role, int *d_site_bypass);
int dkmc_get_cut_info(long long *info16);
int dkmc_copy_cut_path(int capacity, int *h_site, int *h_n_bypass, int *h_chord, int *h_cut, int *rows_out);
int dkmc_copy_cut_bypasses(int capacity, int *h_root, int *h_size, int *h_lo, int *h_hi, int *rows_out);
int dkmc_copy_cut_necks(int capacity, int *h_first, int *h_last, double *h_xmin, double *h_xmax, int *rows_out);

/* ---- min-cut analysis: disjoint conducting paths and the narrowest cross-section (csrc/flow.hip; no counterpart in the reference) ----
 * Where the filament is bridged: how thick it is at its thinnest, in atoms, and where -- the largest number of conducting paths that share no
 * atom, and the two smallest sets of atoms nearest either contact whose loss opens the device.  A maximum flow with unit vertex capacities.  A
 * pure function of its arguments: no field of GPUBuffers, no engine state a later phase reads and no other kernel changes.
 *   members     site i is a member when 0 <= d_label[i] < N (the rule of dkmc_find_paths); nothing else of the labels is used.
 *   link        members u and v are linked when v occurs in row u of d_index[N][nn] OR u occurs in row v.  Entries < 0 or >= N are padding,
 *               anywhere in a row.
 *   seeds       left: the members with index < n_left_sites; right: the members with index >= N - n_right_sites (both clamped to 0 ... N).
 *   interior    the members that are no seed.  Only they carry capacity, one path each; the seeds of a side act as one terminal.
 *   near-left   an interior site linked to a left seed; near-right likewise.
 *   strand      interior sites v_1 ... v_m (m >= 1), consecutive ones linked, v_1 near-left and v_m near-right.  A family of strands is disjoint
 *               when no site lies on two of them.
 *   W           the largest size of a disjoint family = the smallest number of interior sites whose deletion leaves no left seed connected to a
 *               right seed (Menger).
 *   contacts touch  some member is both a left and a right seed, or a left seed is linked to a right seed: W is unbounded, status 2, W = -1.
 *   left-most minimum cut C_L  the minimum separator whose left shore -- the members still connected to a left seed once the separator is
 *               deleted, the left seeds included -- lies inside the left shore of every other minimum separator.  Unique: the interior sites
 *               whose in-node is reachable from the source in the residual graph of ANY maximum flow while their out-node is not.  C_R, the
 *               right-most minimum cut, and the right shore are the mirror image.  Every strand of a maximum family crosses C_L in exactly one
 *               site and C_R in exactly one.
 *   site_zone   d_site_zone[i] (device, N int32, always written completely), a mask of the DKMC_FLOW_ bits: 1 member, 2 on the left shore, 4 in
 *               C_L, 8 in C_R, 16 on the right shore.  A non-member is 0; a site may carry both cut bits.  At status 0 the shores are the members
 *               connected to each contact (its seeds included) and no cut bit is set; at status 2 and 3 only the member bit is set.
 *   info16      (long long) [0] status: 0 not connected (W = 0), 1 W found, 2 contacts touch, 3 stopped at max_strands (W >= max_strands; cuts
 *               and shores not computed), [1] W (-1 at status 2), [2] left-shore members, [3] right-shore members, [4] sites in both C_L and C_R,
 *               [5] interior members, [6] near-left sites, [7] near-right sites, [8] searches run, [9] rounds (below), [10] longest strand,
 *               [11] shortest strand (both 0 without a strand), [12] ... [15] 0.  [2], [3], [4] are 0 at status 2 and 3.
 *   x4          min, max of d_site_x over C_L, then over C_R -- the input doubles themselves, compared through the integer key of
 *               dkmc_find_clusters; +inf / -inf with no cut or when d_site_x is NULL.
 * All of the above is a property of the input.  The following describe ONE maximum family, made canonical by the search rule below:
 *   site_strand d_site_strand[i] (device, N int32, always written completely): the row of the strand through i, -1 otherwise.
 *   strand table  one row per strand, in ascending first site: first_site, last_site, length, offset into the strand sites, left_seed = the
 *               smallest left seed linked to first_site, right_seed = the smallest right seed linked to last_site, cut_left_site, cut_left_pos,
 *               cut_right_site, cut_right_pos = the strand's site in C_L / C_R and its position along the strand (0 = first_site); -1 at status 3.
 *   strand sites  the strands' sites concatenated in table order, each from its left end to its right end.
 * The search rule (a synchronous model; tests/flow_ref.py implements it literally).  Nodes: the source S and, for every interior site v, the
 * in-node 2 v and the out-node 2 v + 1, ordered by these numbers with S before all.  Per interior site the flow state is pred and succ, its
 * neighbours on its strand, with the contact itself at a strand's first and last site; v is on a strand when it has them.  Residual arcs:
 * S -> v_in for every near-left v, always (the terminal arc has no capacity limit); v_in -> v_out if v is on no strand, v_out -> v_in if it is
 * on one; v_out -> w_in for linked interior v, w unless succ[v] = w; w_in -> v_out if succ[v] = w.  v_out is an exit if v is near-right and not
 * a last site.  A search labels levels breadth-first: S has level 0, round k = 0, 1, ... gives level k + 1 to every unlabelled node with an arc
 * from a node of level k.  It stops after the first round that labels an exit -- the end node is the smallest exit of that level -- or that
 * labels nothing.  The augmenting path is walked back from the end node, at every node to the smallest predecessor one level lower; forward
 * link arcs on it become flow, backward ones cancel it, the end site becomes a last site and the path's first site a first site.  Searches repeat
 * until one finds no exit (W is reached) or max_strands strands exist (status 3).  The levels of that last search give C_L (in-node labelled,
 * out-node not) and the left shore (out-node labelled, and the left seeds); one more search on the mirrored problem -- left and right seeds,
 * pred and succ, in-node and out-node change places -- gives C_R and the right shore.
 * Counting: a search's rounds are the rounds that labelled something plus ONE closing round -- the round that labelled nothing, or, after an
 * exit, the round that sees the exit and does nothing: the largest level labelled + 1.  info16[9] is the total over all searches and info16[8]
 * their number, the mirrored one included: W + 2 at status 0 and 1, max_strands at status 3, 0 at status 2 and when N == 0.  Both are
 * functions of the input alone.
 * dkmc_find_flow runs every round as one pass over the member rows; after a successful search one atomicMin pass fixes the smallest
 * predecessors and one thread walks the path back.  A search that needs more than 4096 rounds fails (dkmc_last_error): both site arrays are then
 * -1 everywhere and the getters fail until a call succeeds.  It keeps the results of the LAST call in the library and returns after they are
 * complete; the three getters fail before any successful call.  Any getter pointer may be NULL; capacity truncates and *rows_out reports the
 * rows copied (the true counts are W and the sum of the lengths).  N == 0, no member or an empty seed set succeed with status 0 and empty
 * tables.  max_strands outside 1 ... 4096, N < 0, nn < 1, or d_index, d_label, d_site_zone or d_site_strand NULL with N > 0 fail with code 3
 * before any launch; d_site_x is the only optional array.  Integer atomics only (minima, maxima, counts): the same inputs give the same bytes
 * on every call. */
enum { DKMC_FLOW_MEMBER = 1, DKMC_FLOW_LEFT_SHORE = 2, DKMC_FLOW_LEFT_CUT = 4, DKMC_FLOW_RIGHT_CUT = 8, DKMC_FLOW_RIGHT_SHORE = 16 };
int dkmc_find_flow(int N, int nn, const int *d_index, const int *d_label, const double *d_site_x, int n_left_sites, int n_right_sites,
                   int max_strands, int *d_site_zone, int *d_site_strand);
int dkmc_get_flow_info(long long *info16, double *x4);
int dkmc_copy_flow_strands(int capacity, int *h_first_site, int *h_last_site, int *h_length, int *h_offset, int *h_left_seed, int *h_right_seed,
                           int *h_cut_left_site, int *h_cut_left_pos, int *h_cut_right_site, int *h_cut_right_pos, int *rows_out);
int dkmc_copy_flow_strand_sites(int capacity, int *h_site, int *rows_out);

/* ---- heat ------------------------------------------------------------------------------------ */
/* update_temperatureglobal_gpu (heat_solver_gpu.cu:52-69), the reference's (uncalled) device form */
int dkmc_update_temperatureglobal_gpu(const double *d_site_power, double *d_T_bg, int N, double a_coeff,
                                      double b_coeff, double number_steps, double C_thermal, double small_step);
/* the form the reference actually runs, on the host (heat_solver.cpp:316-350), done on the device */
int dkmc_update_temperature_global_analytic(const double *d_site_power, double *d_T_bg, int N, double event_time,
                                            double dissipation_constant, double t_ox, double A, double c_p,
                                            double *h_P_tot);

/* ---- local temperature model (host-only dense code in the reference: heat_solver.cpp:40-246, 286-308, 354-513) ----
 * Sparse form of the same linear systems, solved with the Jacobi-CG.
 * dkmc_construct_laplacian = Device::constructLaplacian: N_left_tot / N_right_tot are get_num_in_contacts (:5-37) evaluated
 * by the caller on the host copy of site_element, gamma = 1/(delta*(k_th_interface/k_th_metal + 1)) (:86).
 * dkmc_update_temperature_local = the local branch of Device::updateTemperature (:286-308): one steady-state solve when
 * step_time > 1e3*delta_t, else int(step_time/delta_t)+1 transient solves; reads gpubuf.site_power, updates
 * gpubuf.site_temperature and gpubuf.T_bg.  Tolerance of these solves: dkmc_set_heat_cg_tolerance (default 1e-10; the
 * reference applies an explicit inverse). */
void dkmc_set_heat_cg_tolerance(double tol);
/* Where the solves of the local model run.  0 (default): every solve writes the matrix out (8-byte values) and runs the general CSR loop of the
 * Jacobi-CG (csrc/cg.hip), the host polling the stop word per solve.  1: dkmc_construct_laplacian additionally builds, for the heat pattern, the
 * form the K solve would choose for it (csrc/kcg.hip: the blocked form up to 262 144 interface rows, above that the windowed blocked form with
 * dkmc_set_k_blocked_large(1), else -- or when the builder refuses, or with dkmc_set_k_blocked(0) -- the CSR positions), always with 4-byte stored
 * words, and the solves run on the pattern-only CG of the K solve: I - s L and -L have one off-diagonal value, so the matrix is never written out
 * and the Jacobi scaling is applied to the vectors; with more than one transient sub-step the solves are chained on the device and the host
 * synchronises once per batch of 16 sub-steps (a sub-step whose iteration budget was too small is solved again by the polled loop).  Same model,
 * same stop test (dkmc_set_heat_cg_tolerance); results agree with 0 to the tolerance, not bit for bit.  The model itself stays unpinned against the
 * reference, which ships nothing that exercises it: the switch changes how the systems are solved, not what pins them.
 * Read by dkmc_construct_laplacian. */
void dkmc_set_heat_form(int form);
int dkmc_get_heat_form(void);
/* The last dkmc_update_temperature_local.  info8: form of its solves (0 CSR positions, 1 blocked, 2 windowed blocked form of csrc/kcg.hip; -1 the
 * general CSR loop of dkmc_set_heat_form(0)), rows, stored words, sub-steps (solves), host synchronisations of the solves (form -1: the polls the
 * batch plan of the CSR loop makes for the iteration counts it reported), sub-steps that the chain handed back to the polled loop, bytes one
 * iteration moves, 0 (reserved). */
int dkmc_get_heat_info(long long *info8);
int dkmc_construct_laplacian(const dkmc_gpubuf *buf, int N_left_tot, int N_right_tot, double gamma);
int dkmc_update_temperature_local(dkmc_gpubuf *buf, double step_time, double delta_t, double tau, double background_temp,
                                  double k_th_interface, double k_th_vacancies, double nn_dist, int num_atoms_contact,
                                  int *n_solves_out, int *steady_out, int *cg_iters_out, double *T_bg_out);

/* (test and measurement aids of the library -- dkmc_xt_time_share, dkmc_xt_check_shares, dkmc_xtb_check_product, dkmc_xtb_time_apply,
 * dkmc_debug_* -- are declared in devicekmc_hip_debug.h: they are exported by the .so but are not part of the drop-in surface) */

/* ---- multi-GPU: one simulation advanced in lockstep by N processes, one GPU each (no reference counterpart) ----
 * While a communicator is attached, update_power_gpu_sparse generates, stores and streams the tunnelling block of X in per-rank
 * shares (tiled X, the default) and completes the S-rows' sums with ONE in-place all-reduce of |S| + 1 doubles per matrix-vector
 * product; all ranks receive the same bits -- including rank 0's stop decision, from which every rank takes its control flow --
 * and the result equals the single-GPU one to rounding.  With dkmc_set_x_format(0) (CSR X) the long rows are dealt to the ranks
 * and an all-gather of row sums keeps the result bit-identical to the single-GPU one.  poisson_gridless_gpu sums a slab of sites
 * per rank and all-gathers the potentials (bit-identical).  Every other phase is computed redundantly and identically on every
 * rank, so all ranks hold the same state after every call.  Every rank must make the same sequence of
 * calls with the same inputs.
 * Transports: RCCL over xGMI (unique id from rank 0, distributed by the caller), or a host callback that all-gathers a
 * pinned host buffer in place (rehearsal on machines where the ranks share a GPU, which RCCL refuses). */
enum { DKMC_COMM_NONE = 0, DKMC_COMM_RCCL = 1, DKMC_COMM_HOST = 2 };
/* host_buf holds nranks chunks of bytes_per_rank bytes, the caller's own chunk (index rank) filled in; on return all are */
typedef int (*dkmc_allgather_fn)(void *host_buf, size_t bytes_per_rank, int rank, int nranks, void *user);
int dkmc_comm_unique_id(char *id128);                                   /* ncclGetUniqueId; 128 bytes out */
int dkmc_comm_init_rccl(int nranks, int rank, const char *id128);       /* after dkmc_set_gpu / dkmc_set_stream */
int dkmc_comm_init_host(int nranks, int rank, dkmc_allgather_fn fn, void *user);
int dkmc_comm_allgather_host(double *host_buf, size_t count_per_rank);  /* the callback transport's host half (no GPU needed) */
int dkmc_comm_info(int *nranks, int *rank, int *transport);
int dkmc_comm_destroy(void);
/* One-shot peer-write exchange of the sharded block-CG (csrc/comm.hip): beside an attached communicator, every rank
 * exports an exchange buffer of 2 x nranks slots of slot_doubles doubles and a row of sequence words (hipIpc; fine-grained device memory, so
 * that a peer DEVICE's stores are visible without a kernel boundary); prepare returns this rank's two handles + its device identity (192
 * bytes), the host all-gathers them through its process group and hands all of them (nranks x 192 bytes, rank order) to attach.  attach
 * refuses (error 49) a group whose ranks sit on different devices unless DKMC_PEER_CROSS_DEVICE=1 -- that case has never been run.  A sweep's exchange is then push + signal + bounded wait on the engine's stream and the slots are added in rank order; a solve
 * whose slots do not fit uses the communicator's all-gather.  Tested with two processes on one GPU; opt-in.  The reference has no counterpart. */
int dkmc_comm_peer_prepare(size_t slot_doubles, char *handles192);
int dkmc_comm_peer_attach(const char *all_handles);
int dkmc_comm_peer_detach(void);
int dkmc_comm_peer_info(int *ready, long long *slot_doubles, long long *exchanges, double *mean_us);

#ifdef __cplusplus
}
#endif
#endif
