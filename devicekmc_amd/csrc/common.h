// common.h -- shared device helpers and the process-wide engine state (one GPU per process).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <stdio.h>
#include <string.h>
#include <math.h>
#include "../../include/devicekmc_hip.h"
#include "../../include/devicekmc_hip_debug.h"

// ELEMENT / EVENTTYPE (utils.h:37-60)
enum { DEFECT = 0, OXYGEN_DEFECT = 1, VACANCY = 2, O_EL = 3, Hf_EL = 4, Ni_EL = 5, Ti_EL = 6, Pt_EL = 7, N_EL = 8, NULL_ELEMENT = 9 };
enum { EV_GEN = 0, EV_REC = 1, EV_VDIFF = 2, EV_IDIFF = 3, EV_NULL = 4 };

#define DKMC_KB 8.617333262e-5       // kmc_events.cu:4
#define DKMC_Q 1.60217663e-19        // gpu_solvers.h:261
#define DKMC_HBAR 1.054571817e-34    // iterative_solvers_gpu.cu:8
#define DKMC_MAX_LAYERS 5            // kmc_events.cu:7
#define WAVE 64

// the list of metallic elements stays in device memory, as in the reference (is_in_array_gpu, gpu_solvers.h:211-220)
struct MetalSet { int n; const int *e; };

__device__ __forceinline__ bool is_metal(int el, const MetalSet &ms)
{
    bool r = false;
    for (int t = 0; t < ms.n; ++t) r |= (ms.e[t] == el);
    return r;
}

// gpu_solvers.h:225-257
__device__ __forceinline__ double site_dist(double x1, double y1, double z1, double x2, double y2, double z2,
                                            double laty, double latz, int pbc)
{
    if (pbc) {
        double dx = x1 - x2;
        double fy = (y1 - y2) / laty; fy -= round(fy);
        double fz = (z1 - z2) / latz; fz -= round(fz);
        double dy = fy * laty, dz = fz * latz;
        return sqrt(dx * dx + dy * dy + dz * dz);
    }
    double dx = x2 - x1, dy = y2 - y1, dz = z2 - z1;
    return sqrt(dx * dx + dy * dy + dz * dz);
}

// gpu_solvers.h:259-265
__device__ __forceinline__ double v_solve(double r, int charge, double sigma, double k)
{
    return (double)charge * erfc(r / (sigma * sqrt(2.0))) * k * DKMC_Q / r;
}

// ---- lane exchange without the LDS ------------------------------------------------------------
// hipcc lowers every __shfl_xor to ds_bpermute_b32 -- an LDS instruction per 32 bits, two per double.  Inside a row of 16 lanes the exchange
// "lane i <- lane i ^ OFF" (OFF = 1, 2, 4, 8) is a DPP move on the vector ALU (tools/probe_dpp_xor.hip: identical to __shfl_xor on gfx950); the
// per-row reductions of the sparse kernels were bound by the bpermutes, not by their memory traffic.  Offsets 16 / 32 stay on __shfl_xor.
template <int OFF> __device__ __forceinline__ int xor_lane_i(int x)
{
    static_assert(OFF == 1 || OFF == 2 || OFF == 4 || OFF == 8 || OFF == 16 || OFF == 32, "xor_lane: power of two below the wave size");
    if constexpr (OFF == 1) return __builtin_amdgcn_update_dpp(0, x, 0xB1, 0xf, 0xf, false);        // quad_perm [1,0,3,2]
    else if constexpr (OFF == 2) return __builtin_amdgcn_update_dpp(0, x, 0x4E, 0xf, 0xf, false);   // quad_perm [2,3,0,1]
    else if constexpr (OFF == 4) {                                                                   // row_shl:4 into banks 0, 2; row_shr:4 into banks 1, 3
        const int t = __builtin_amdgcn_update_dpp(0, x, 0x104, 0xf, 0x5, false);
        return __builtin_amdgcn_update_dpp(t, x, 0x114, 0xf, 0xa, false);
    }
    else if constexpr (OFF == 8) return __builtin_amdgcn_update_dpp(0, x, 0x128, 0xf, 0xf, false);  // row_ror:8
    else return __shfl_xor(x, OFF, WAVE);
}
template <int OFF> __device__ __forceinline__ double xor_lane(double x)
{
    if constexpr (OFF >= 16) return __shfl_xor(x, OFF, WAVE);
    else return __hiloint2double(xor_lane_i<OFF>(__double2hiint(x)), xor_lane_i<OFF>(__double2loint(x)));
}
// butterfly sum over groups of W lanes (W a power of two), offsets W / 2, ..., 1 in that order: every lane of a group ends with the group's sum
template <int W> __device__ __forceinline__ double group_sum(double v)
{
    if constexpr (W >= 64) v += xor_lane<32>(v);
    if constexpr (W >= 32) v += xor_lane<16>(v);
    if constexpr (W >= 16) v += xor_lane<8>(v);
    if constexpr (W >= 8) v += xor_lane<4>(v);
    if constexpr (W >= 4) v += xor_lane<2>(v);
    if constexpr (W >= 2) v += xor_lane<1>(v);
    return v;
}
template <int W> __device__ __forceinline__ int group_sum_i(int v)
{
    if constexpr (W >= 64) v += xor_lane_i<32>(v);
    if constexpr (W >= 32) v += xor_lane_i<16>(v);
    if constexpr (W >= 16) v += xor_lane_i<8>(v);
    if constexpr (W >= 8) v += xor_lane_i<4>(v);
    if constexpr (W >= 4) v += xor_lane_i<2>(v);
    if constexpr (W >= 2) v += xor_lane_i<1>(v);
    return v;
}

// ---- wave64 / block reductions with a fixed combination order (deterministic) -----------------
// (lane 0 of the butterfly sees the same additions in the same order as the shift-down form it replaces: same bits)
__device__ __forceinline__ double wave_sum(double v) { return group_sum<WAVE>(v); }       // valid in lane 0 (and everywhere)
__device__ __forceinline__ double wave_sum_all(double v) { return group_sum<WAVE>(v); }   // same value in every lane
__device__ __forceinline__ int wave_sum_all_i(int v) { return group_sum_i<WAVE>(v); }
// minimum / maximum of an integer (int, unsigned long long) across the wave, the same value in every lane; no order dependence
template <class T> __device__ __forceinline__ T wave_min(T v)
{
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) { const T t = __shfl_xor(v, off, WAVE); v = t < v ? t : v; }
    return v;
}
template <class T> __device__ __forceinline__ T wave_max(T v)
{
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) { const T t = __shfl_xor(v, off, WAVE); v = t > v ? t : v; }
    return v;
}
// inclusive scan across the wave
__device__ __forceinline__ double wave_scan_incl(double v, int lane)
{
#pragma unroll
    for (int off = 1; off < WAVE; off <<= 1) { double t = __shfl_up(v, off, WAVE); if (lane >= off) v += t; }
    return v;
}
__device__ __forceinline__ int wave_scan_incl_i(int v, int lane)
{
#pragma unroll
    for (int off = 1; off < WAVE; off <<= 1) { int t = __shfl_up(v, off, WAVE); if (lane >= off) v += t; }
    return v;
}

// block sum, result broadcast to all threads; red must hold blockDim.x/64 doubles
template <int NT>
__device__ __forceinline__ double block_sum_all(double v, double *red)
{
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    v = wave_sum(v);
    __syncthreads();
    if (lane == 0) red[w] = v;
    __syncthreads();
    double s = 0.0;
#pragma unroll
    for (int i = 0; i < NT / 64; ++i) s += red[i];
    return s;
}

// ---- integer forms of doubles, relaxed agent-scope words, contact seeds (clusters.hip, gaps.hip)
// order-preserving 64-bit key of a double (unsigned compare): negative values flip every bit, the others the sign bit.  -0.0 orders below +0.0.
__host__ __device__ __forceinline__ unsigned long long dbl_key(double v)
{
    const unsigned long long b = __builtin_bit_cast(unsigned long long, v);
    return (b >> 63) ? ~b : (b | 0x8000000000000000ull);
}
__host__ __device__ __forceinline__ double key_dbl(unsigned long long k)
{
    return __builtin_bit_cast(double, (k >> 63) ? (k & 0x7fffffffffffffffull) : ~k);
}
__device__ __forceinline__ int ld_agent(const int *p) { return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }
__device__ __forceinline__ void st_agent(int *p, int v) { __hip_atomic_store(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }
// contact seeds: site i is a left seed (bit 0) iff i < n_left, a right seed (bit 1) iff i >= N - n_right; the entry points clamp both to [0, N]
__device__ __forceinline__ int seed_bits(int i, int N, int n_left, int n_right) { return (i < n_left ? 1 : 0) | (i >= N - n_right ? 2 : 0); }
inline void clamp_seeds(int N, int &n_left, int &n_right)
{
    n_left = n_left < 0 ? 0 : (n_left > N ? N : n_left);
    n_right = n_right < 0 ? 0 : (n_right > N ? N : n_right);
}

// blocked form of a K pattern (kcg.hip: kblocked_build, once per pattern; device arrays)
struct KBlocked {
    int m, R, nb, total, maxwin, maxints;      // maxints: ints of the largest block's padded rows
    long long winsum;   // columns in all windows together
    int *perm;          // [m] row of the blocked order -> row of the pattern
    int *pcol;          // [total] columns in the blocked order, rows padded to 64 / 32 entries with the row itself, diagonal left out
    int4 *blk;          // [nb] {first column of the window, columns in the window, first int of the block in pcol, rows padded to 64}
    // form 2: the windowed form above KB_MAXROWS rows (dkmc_set_k_blocked_large): pcol holds LDS offsets into the block's window, blk is
    // {window doubles, LDS offset of the block's first row, first int of the block in pcol, rows padded to 64}, and the window is copied
    // from the segments seg[KBW_MAXSEG * b ...] {LDS offset, length, first row in the blocked order, 0}
    int form = 1;
    int maxseg = 0;     // segments of the most fragmented window
    long long segsum = 0;
    int4 *seg = nullptr;
    int word_bytes = 4; // form 2: bytes of a stored word of the assembled cf (dkmc_set_k_window_word_bytes when the pattern was built); pcol stays 32-bit
};
// ---- host side ---------------------------------------------------------------------------------
constexpr double X_STOP_MARGIN_DEFAULT = 1.0;      // Engine::x_stop_margin
constexpr int X_POLY_DEFAULT = 8;   // base degree of the split polynomial preconditioner (Engine::x_poly)
// how the last round of a one-polynomial block solve stopped (dkmc_get_x_stop_info): fired 0 = no such round, 1 = the bound test of k_xtb_small (or a
// breakdown), 2 = the norm test; with_norm: the norm test ran beside the bound; rows of the system; ||Rt(:, 0)|| at the stop (-1: not measured),
// (Rt'Z)_00 at the stop, the true residual ||A y - b|| behind it
struct XStopLast { int fired = 0, with_norm = 0, m = 0; double norm = -1.0, rz = 0.0, true_res = 0.0; };
struct Engine {
    hipStream_t stream = nullptr;
    int device = 0;
    double cg_tol = 1e-6;
    int current_warm_start = 1;    // start vector of the current solve (dkmc_set_current_warm_start): 1 previous solution (private unscaled copy), 0 the reference code's G0-scaled buffer
    int profiling = 0;
    int cb_edge_domain = 0;        // 0: CB-edge system over every site (snapshot source); 1: over atoms only (dkmc_set_cb_edge_domain)
    long long tcache_budget = -1;  // bytes the tunnelling-coefficient cache may take; -1 = a third of the free device memory, 8-128 GiB (dkmc_set_tcache_budget)
    double pair_cut = 6.5;         // screening cut-off of the pair sum in units of sigma sqrt 2 (dkmc_set_pair_cutoff; 0 = all pairs like the reference)
    int pair_form = 0;             // sum kernels of the pair sum: 0 = a term is evaluated where it is tested; 1 = a wave queues the passing pairs and evaluates 64 at a time; same bits (dkmc_set_pair_form; potential.hip)
    int k_blocked = 1;             // build the blocked form of K patterns (dkmc_set_k_blocked; kcg.hip)
    int k_blocked_large = 0;       // 1: above KB_MAXROWS rows build the windowed blocked form instead (dkmc_set_k_blocked_large; kcg.hip)
    int k_window_word_bytes = 4;   // stored words of the windowed blocked form: 4 = one int per entry, 2 = 16 bits per entry (14-bit LDS offset + class bit 15); same results (dkmc_set_k_window_word_bytes; kcg.hip)
    int x_aux = 2;                 // auxiliary columns of the block-CG (dkmc_set_x_aux; xtb.hip): 0 hash set, 1 smooth set, 2 smooth at tolerances >= 1e-8
    int x_slab = 1;                // > 1 rank: distribute the STATE of the block-CG by row slabs (xtb_slab.inc; dkmc_set_x_slab); 0: all-gather variant (tile stream sharded only)
    int k_slab = 1;                // > 1 rank, system above the size of the blocked form: CG on K distributed by row slabs (kcg.hip; dkmc_set_k_slab); 0: replicated
    int x_poly = X_POLY_DEFAULT;                // degree d of the split polynomial preconditioner of the block-CG (dkmc_set_x_poly; xtb_precond.h): the loop runs on L A L, L = the degree-d Chebyshev interpolant of (1 - x)^(-1/2) in N (neighbour part); 0 = off.  With x_poly_auto it is the base degree: on (> 0) or off, the one-GPU loop takes its degree from the system size
    int x_poly_auto = 1;           // 1 (default): the one-GPU preconditioned loop takes its degree from the rows of the system (xtb_poly_rule, xtb_precond.h); dkmc_set_x_poly(d) pins d and clears it, dkmc_set_x_poly_auto(1) sets it again
    int x_poly_rows[2] = {0, 0};   // test aid (dkmc_set_x_poly_auto_rows): breakpoints of that rule; {0, 0} = the measured ones
    int x_poly_form = 2;           // form of the one-GPU preconditioned loop (dkmc_set_x_poly_form; xtb.hip): 0 = split, CG on L A L (2 d N products per sweep); 1 = one polynomial q(N) ~ (I - N)^-1 as M^-1, in transformed variables (n(d) products); 2 = one polynomial where the degree comes from the rule (x_poly_auto), split where a degree is pinned
    int x_poly1_degree = 0;        // measurement aid (dkmc_debug_set_x_poly1_degree): > 0 overrides the degree n(d) of the one-polynomial form
    int x_poly_form_used = 0, x_poly_products = 0;      // the last one-GPU block solve: 1 = it ran the one-polynomial form; its N products per sweep (dkmc_get_x_poly_form_used / _products)
    int x_stop_form = 2;           // stop test of the one-polynomial loop (dkmc_set_x_stop_form; xtb.hip): 0 = the bound rt'q(N)rt <= tol^2 min q alone; 1 = beside it the norm it bounds, ||Rt(:, 0)|| <= x_stop_margin tol (k_xtb_stop_norm), whichever fires first; 2 (default) = 1 from the measured size gate on (xtb_stop_rule, xtb_precond.h), 0 below it
    double x_stop_margin = X_STOP_MARGIN_DEFAULT;   // kappa of that test (dkmc_set_x_stop_margin): the largest of {1, 0.8, 1 / 1.5} without a re-entry round over 100 steps at 9.4e5 sites (profiles/x_stop_soak_tile10.jsonl)
    XStopLast x_stop_last{};       // the stop of the last one-polynomial round (dkmc_get_x_stop_info)
    int x_slab_poly = 0;          // 1: the slab-distributed block-CG (> 1 rank, x_slab) runs on L A L too (dkmc_set_x_slab_poly; xtb_slab.inc); 0 (default): plain
    int x_aux_warm = 0;            // 1: with the warm start of the current solve the hash auxiliary columns start from the previous solve's solutions too (dkmc_set_x_aux_warm; off: no gain beyond 1e4 rows, profiles/r05_ab_aux_warm.json)
    int x_items_kc = 0;            // > 0: overrides the nominal run length kc (tiles) of the tile runs (dkmc_set_x_items; measurement)
    int x_apply_form = 0;          // tile x panel kernel of the block-CG: 0 = the product form, 1 = the round-4 form of its loop (same results; same-box comparisons, dkmc_set_x_apply_form)
    int x_tile_f32 = 1;            // tile values of the block-CG's sweeps: 1 (auto) = the fp32 image inside the one-GPU preconditioned loop at cg_tol >= 1e-8, when the copy could be made; 0 = always the fp64 store (dkmc_set_x_tile_f32; xtb.hip)
    double x_tile_drop = 0.0;      // > 0: where the sweeps stream the fp32 image they stream a compacted one of the LIVE tiles only -- stored 32 x 256 tiles with a scaled entry sc_i |v_ij| sc_j >= this threshold (dkmc_set_x_tile_drop; xt_live.h); 0 (default) = off
    int x_tile_drop_unit = 0;      // what x_tile_drop drops: 0 (default) whole tiles, 1 the sub-blocks (32 x 32) without such an entry inside the live tiles too (dkmc_set_x_tile_drop_unit; xt_live.h)
    int x_tile_drop_auto = 1;      // 1 (default): with x_tile_drop at 0 a WARM-STARTED solve whose stored X reaches the measured size gate runs its sweeps on the live tiles at 1e-10 (xtl_drop_rule, xt_live.h; dkmc_set_x_tile_drop_auto); an explicit x_tile_drop > 0 applies as it is, cold starts included
    long long x_tile_drop_gate = 0;     // test aid (dkmc_set_x_tile_drop_auto_subblocks): stored sub-blocks at and above which that rule switches the live view on; 0 = the measured gate
    double x_tile_drop_used = 0.0;      // the threshold the sweeps of the last current solve ran on, 0 = the full view (dkmc_get_x_tile_drop_used)
    int xtl_census_form = 1;       // census of the live view: 1 (default; 0.87 of form 0's time per solve at 9.4e5 sites, profiles/x_tile_census_forms_tile10.jsonl) = from the fp32 image with a guard band and an fp64 re-read of the undecided sub-blocks, 0 = from the fp64 store; same result (dkmc_debug_xtl_census_form; xt_live.h)
    int x_static_tiles = 2;        // S with the inner-contact metals FIRST, and the all-metal strips of the tile store kept from solve to solve (dkmc_set_x_static_tiles; current.hip step 2, xt_static.h): 0 = atom order and a full fill, 1 = on, 2 (default) = on where it applies (one GPU, tiled X)
    int x_static_gate = 0;         // test aid (dkmc_debug_set_x_static_gate): members of S at and above which mode 2 takes the metals-first order; 0 = the measured gate (x_static_rule)
    int x_static_nM = -1;          // this solve's S is in metals-first order with that many metals in front; -1 = atom order (set by current.hip step 2, read by xt.hip)
    int x_static_verify = 0;       // test aid (dkmc_debug_x_static_verify): every assembly in metals-first order is followed by a full census and a full fill into separate buffers, compared word by word
    int x_tile_f32_fail_once = 0;  // test aid (dkmc_debug_fail_true_residual_once): the next true-residual check of the preconditioned loop reports "above tolerance" once, on the host side
    int x_fold_form = 1;           // fold of the tile launch's row partial sums in the one-GPU preconditioned loop: 1 (default) = only the cells of the launch view's tiles, by the window lists (xtb_wlist_sum2; no zeroed cells, the one-column products at one vector group), 0 = every cell of wrange[k] with the per-solve memset and k_xtl_zero_dead; same bits (dkmc_set_x_fold_form; xtb.hip)
    int x_fold_poison = 0;         // test aid (dkmc_debug_poison_fold_cells, sticky): a solve in fold form 1 fills the row partial sums with NaN where form 0 zeroes them
    int x_nmul_form = 1;           // N products of the split polynomial preconditioner: 1 = on the per-solve packed copy of N (k_xtb_nmulp16 / k_xtb_nmulp, x_nmul_lane_bytes), 0 = on the CSR of Xs (k_xtb_nmul); same results (dkmc_set_x_nmul_form)
    int x_nmul_lane_bytes = 16;    // gathers of the packed N products: 16 = two slots of a row per instruction, 16 bytes per lane (k_xtb_nmulp16), 8 = one slot, 8 bytes per lane (k_xtb_nmulp); same results (dkmc_set_x_nmul_lane_bytes)
    int x_nmul_window = 2;         // panel operands of the packed 16-byte N products from LDS row windows (k_xtb_nmulw, nwin_plan.h): 0 = off, 1 = on, 2 = by size (xb_nwin_rows); same results (dkmc_set_x_nmul_window)
    int x_nmul_window_cap = 76 * 1024;   // test aid (dkmc_debug_set_x_nmul_window): LDS bytes of a window at most (0: every slot gathers from memory) ...
    int x_nmul_window_block = 320;       // ... and the rows of a block
    int x_block = 16;              // block-CG width of the current solve on the tiled X (dkmc_set_x_block; xtb.hip): 16 by default, 1 = the reference's single-vector loop (its iterate sequence)
    int x_format = 1;              // 1: tiled X (xt.hip, default); 0: CSR X as the reference stores it (current.hip + cg.hip)
    int current_map = 0;           // 1: every current solve also leaves the atom-resolved current map of its GPUBuffers (dkmc_set_current_map; current.hip step 6 1/2)
    int x_iter_hint = 0;           // iteration count of the previous CG solve of X (sizes the first launch batch)
    int event_temperature = 0;     // rate model of the event table (dkmc_set_event_temperature; events.hip): 0 the reference as compiled (one global T_bg), 1 the reference authors' kinetic term on the local site temperature, 2 Arrhenius on it
    int event_census = 0;          // 1: every dkmc_execute_kmc_step_gpu that builds a table also takes its rate census (dkmc_set_event_census; ev_census.hip)
    int event_census_valid = 0;    // ... and the last one taken (dkmc_get_event_census)
    double event_census_info[16] = {0};
    dkmc_stats stats{};
    char err[512] = {0};
    int err_code = 0;
    // per-layer energies (copytoConstMemory)
    double E_gen[DKMC_MAX_LAYERS] = {0}, E_rec[DKMC_MAX_LAYERS] = {0}, E_Vdiff[DKMC_MAX_LAYERS] = {0}, E_Odiff[DKMC_MAX_LAYERS] = {0};
    int num_layers = 0;
    // named persistent device buffers (grown on demand, never shrunk)
    static const int NBUF = 192;
    void *buf[NBUF] = {nullptr};
    size_t bufsz[NBUF] = {0};
};

// Size rule of dkmc_set_x_static_tiles(2): 1 = a tunnelling set of ns members takes the metals-first order.  Measured on whole supersteps against atom
// order (profiles/ab_bench_x_static_tiles.txt): 7.5nm (8 353 members) and tile:5 (23 224) lose or tie, tile:6 (33 445) and everything above gain.
constexpr int X_STATIC_GATE = 32768;
static inline int x_static_rule(int ns, int gate_override) { return ns >= (gate_override > 0 ? gate_override : X_STATIC_GATE) ? 1 : 0; }
Engine &eng();
int dkmc_fail(int code, const char *what, const char *file, int line);
// persistent scratch: returns a device buffer of at least `bytes`, identified by slot
void *scratch(int slot, size_t bytes);
// the same for a buffer the caller can do without: null and NO error recorded when the allocation fails
void *scratch_try(int slot, size_t bytes);
// blocks for `work` items at `per_block` each, at least 1 and at most `cap`
static inline int grid_blocks(long long work, int per_block, int cap)
{
    long long b = (work + per_block - 1) / per_block;
    if (b < 1) b = 1;
    if (b > cap) b = cap;
    return (int)b;
}
inline MetalSet load_metals(const int *d_metals, int num_metals) { MetalSet ms; ms.n = num_metals; ms.e = d_metals; return ms; }

#define HIPCHK(x) do { hipError_t e__ = (x); if (e__ != hipSuccess) return dkmc_fail((int)e__, hipGetErrorString(e__), __FILE__, __LINE__); } while (0)
#define KCHK() do { hipError_t e__ = hipGetLastError(); if (e__ != hipSuccess) return dkmc_fail((int)e__, hipGetErrorString(e__), __FILE__, __LINE__); } while (0)

// scratch slots
enum {
    S_CG_S = 0, S_CG_R, S_CG_P, S_CG_T, S_CG_PART, S_CG_CTRL, S_CG_RUNS, S_CG_REM, S_CG_NRUNS, S_CG_PS, S_CG_SEGOFF, S_CG_SEGS, S_CG_SEGPART, S_CG_XCHG, S_CG_PARTS,
    S_K_DATA, S_K_RHS,
    S_PW_LIST, S_PW_CNT, S_PW_CELLS, S_PW_PERM, S_PW_LIST2,
    S_EV_PROB, S_EV_ROWSUM, S_EV_G2, S_EV_G3, S_EV_CTRL, S_EV_UNI, S_EV_LOG,
    S_SCAN_TMP, S_SCAN_TMP2, S_SCAN_OFF64, S_SCAN_INTILE,
    S_AT_FLAG, S_AT_SITE, S_AT_OFSITE, S_AT_NEIGH,
    S_X_ROWPTR, S_X_COL, S_X_DATA, S_X_DATA2, S_X_CNT, S_X_SLIST, S_X_SCB, S_X_SFLAG, S_X_RHS, S_X_SRANK,
    S_P_IMACRO, S_HEAT, S_HEAT_A, S_HEAT_B, S_HEAT_Y,
    S_MISC0, S_MISC1, S_MISC2, S_MISC3,
    S_XT_DPOS, S_XT_SNODE_D, S_XT_SNODE_I, S_XT_CMASK, S_XT_ISTILE, S_XT_NSUBC, S_XT_TOFF, S_XT_SOFF, S_XT_TILES, S_XT_NITEMW, S_XT_WRANGE,
    S_XT_ITEMS, S_XT_SPLIT, S_XT_TVAL, S_XT_TVAL32, S_XT_ROWPART, S_XT_COLPART, S_XT_CNT, S_XT_Q,
    S_XT_T_NITEMW, S_XT_T_ITEMS, S_XT_T_SPLIT, S_XT_T_COLPART, S_XT_T_MISC,
    S_XTB_PANELS, S_XTB_QS, S_XTB_ROWPART, S_XTB_COLPART, S_XTB_GRAM, S_XTB_SMALL, S_XTB_XI,
    S_XTB_SLAB_BOX, S_XTB_SLAB_TAB, S_XTB_SLAB_OWNER, S_XTB_SLAB_LISTS, S_XTB_SLAB_SDST, S_XTB_SLAB_FLAG, S_XTB_SLAB_RLISTS, S_XTB_SLAB_GX, S_XTB_SLAB_S1, S_XTB_SLAB_S3, S_XTB_SLAB_R3,
    S_XTB_EMU_Y, S_XTB_EMU_CTRL, S_XTB_YPANEL, S_XTB_PRE_V, S_XTB_PRE_W1, S_XTB_PRE_W2, S_XTB_PRE_Z, S_XTB_PRE_U,
    S_XTB_NPACK_CNT, S_XTB_NPACK_OFF, S_XTB_NPACK_COL, S_XTB_NPACK_W,
    S_XTL_CELLS, S_XTL_TFLAG, S_XTL_TVAL32, S_XTL_TILES, S_XTL_WRANGE, S_XTL_NITEMW, S_XTL_ITEMS, S_XTL_SPLIT,      // live view of the tile list (xt_live.h)
    S_XT_WLIST, S_XTL_WLIST,       // windows holding a tile, by row block: the full view's and the live view's (k_xt_wrange; the list fold of xtb.hip)
    S_KS_TAB, S_KS_OWNER, S_KS_LISTS, S_KS_FLAG, S_KS_BOX, S_KS_RLISTS, S_KS_XA, S_KS_XB, S_KS_SEND, S_KS_RECV, S_KS_YBUF, S_KS_EMU,
    // test aids of the preconditioner (xtb_precond.h: dkmc_xtb_test_nstep, dkmc_xtb_check_poly): their own buffers, nothing a solve reads
    S_XTB_TEST_RP, S_XTB_TEST_CI, S_XTB_TEST_VAL, S_XTB_TEST_SC, S_XTB_TEST_NSR, S_XTB_TEST_LIST, S_XTB_TEST_IN, S_XTB_TEST_ADD, S_XTB_TEST_OUT,
    S_XTB_TEST_W1, S_XTB_TEST_W2, S_XTB_TEST_QS, S_XTB_TEST_CTRL, S_XTB_TEST_NPCNT, S_XTB_TEST_NPOFF, S_XTB_TEST_NPCOL, S_XTB_TEST_NPW,
    S_P_CMAP,       // current map (dkmc_set_current_map): tile sums of S and the row kernel's partials
    // test aids of the sweep's Gram, s x s and panel-step kernels (xtb.hip: dkmc_xtb_test_gram / _small / _step): their own buffers, as above
    S_XTB_ALG_PANELS, S_XTB_ALG_INTS, S_XTB_ALG_GRAM, S_XTB_ALG_QS, S_XTB_ALG_CTRL,
    // filament analysis (clusters.hip: dkmc_find_clusters): the forest, the per-root summaries, root flags + positions, the component table, change words + info
    S_CL_PARENT, S_CL_SUMS, S_CL_POS, S_CL_TABLE, S_CL_CTRL,
    // event rates on the local temperature (events.hip): the bad-temperature word of a build; rate census (ev_census.hip): workgroup partials, info
    S_EV_NBAD, S_EV_CENSUS_PART, S_EV_CENSUS_INFO,
    // gap analysis (gaps.hip: dkmc_find_gaps): per-site words (component flags, cell, node), control block + box partials, the cell list, the members
    // in cell order, the per-node picks and pointers, the forest's edges
    S_GAP_SITE, S_GAP_CTRL, S_GAP_CELLS, S_GAP_SORTED, S_GAP_NODES, S_GAP_EDGES,
    // conduction-path analysis (paths.hip: dkmc_find_paths): the hop pairs, the predecessors, the profile rows + path, change words + stat block
    S_PT_HOP, S_PT_PRED, S_PT_ROWS, S_PT_CTRL,
    // cluster tracking (track.hip: dkmc_track_clusters): the pair table, the per-component words of both sides, per-site slot + flags + positions,
    // the rows of the tables, the control block
    S_TR_HASH, S_TR_COMP, S_TR_SITE, S_TR_ROWS, S_TR_CTRL,
    // cut-site analysis (cuts.hip: dkmc_find_cuts): per-site words (position, forest, lo / hi, size, root flag + position), the bypass table, the
    // per-position rows (difference arrays, path table, necks), change words + stat block
    S_CUT_SITE, S_CUT_TABLE, S_CUT_ROWS, S_CUT_CTRL,
    // min-cut analysis (flow.hip: dkmc_find_flow): per-site words (strand neighbours, the level pairs of both closing searches, the nearest seeds,
    // predecessors, first-site flag + rank, the strand sites), the strand table, change words + stat block
    S_FL_SITE, S_FL_ROWS, S_FL_CTRL,
    // norm stop test of the one-polynomial block loop (xtb.hip: k_xtb_step1's partial sums, k_xtb_stop_norm's record)
    S_XTB_STOPN,
    S_NSLOTS
};
static_assert(S_NSLOTS <= Engine::NBUF, "scratch slots");

// exchange step of the sharded current solve (comm.hip)
int comm_attached();
int comm_nranks();
int comm_rank();
int comm_allgather_f64(double *buf, size_t count);     // in place on the engine's stream; rank r owns buf[r*count, (r+1)*count)
int comm_alltoallv_f64(const double *sendbuf, double *recvbuf, const long long *cnt);   // rank s sends cnt[s * nranks + d] doubles to rank d (full table on every rank; pieces packed in destination / source order)
int comm_allreduce_sum_f64(double *buf, size_t count); // in place; the sum over the ranks (grouping of the additions is the transport's)
int comm_agree(int local_rc, const char *what);         // agreement point: non-zero on EVERY rank if any rank passed a non-zero local_rc (comm.hip)
int comm_agree_count();
int comm_peer_ready(size_t count);                      // the one-shot peer-write exchange is attached and its slots hold `count` doubles (comm.hip)
double *comm_peer_slots(int parity);
void comm_peer_drop();                                  // after a failed solve: the peers' sequence counters may have drifted (comm.hip)
int comm_peer_exchange(int parity, size_t count, int *ctrl_done, int *ctrl_aborted, int *ctrl_timeout, int stamp);
int comm_bcast0_f64(double *buf, size_t count);        // in place; every rank ends with rank 0's bits

// rate census of an event table (ev_census.hip): enqueues the two kernels on the engine's stream; *d_info16 = the device copy of the 16 doubles
int ev_census_enqueue(int N, int nn, const int *neigh, const int *element, const double *temperature, const double *ev_prob, double **d_info16);

// shared primitives (scan.hip)
// exclusive prefix sum of n ints (in -> out, out may alias in); total written to d_total (device int) if non-null
int dkmc_exclusive_scan_i32(const int *d_in, int *d_out, int n, int *d_total);
// same with 64-bit offsets (counts stay 32 bit)
int dkmc_exclusive_scan_i32_i64(const int *d_in, long long *d_out, int n, long long *d_total);
