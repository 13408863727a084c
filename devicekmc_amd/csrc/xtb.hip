// xtb.hip -- block-CG of the current solve on the tiled X, with the tile x panel product on the matrix cores (dkmc_set_x_block(s), s = 2 ... 16).
//
// What it replaces: solve_sparse_CG_Jacobi (iterative_solvers_gpu.cu:309-480) as update_power_gpu_sparse calls it
// (current_solver_gpu.cu:963-994), and -- for the tunnelling block -- the dense tile product of the reference's unfinished split path
// (add_submatrix_product, iterative_solvers_gpu.cu:634-652; solve_sparse_CG_splitmatrix :656-821), which applies the tile as a GEMV.
// X changes every superstep and has ONE physical right-hand side, so there is nothing to batch -- but a block-CG whose other columns are
// AUXILIARY right-hand sides (fixed-seed pseudo-random, zero start) searches the block Krylov space of all s columns and deflates the
// outlying part of X's spectrum (loop_G = 1e12, high_G = 1e5, low_G = 1e-8 nodes): on the oracle's X of the 85 071-site device the
// reference's stop test on the physical column is met after 666 / 208 / 133 / 95 sweeps at s = 1 / 4 / 8 / 16 (tools/blockcg_proto.py).
// One sweep streams every stored 32 x 32 sub-block ONCE (8 KiB, both triangles from one read, as the single-vector kernel does) and
// multiplies it and its transpose into 32 x 16 panels: 4 s flops per 8 bytes -- at s = 16 a contraction of 8 flop/B, which is what
// north_star reserves the matrix cores for.
//
// Algorithm (scaled system A = S X S, sign convention of the reference: R = A Y - B, first direction -R):
//     T = A P                                            one sweep
//     c = -(P'T)^-1 P'R ;  Y += P c ;  R+ = R + T c
//     beta = (P'T)^-1 (T'R + T'T c)                      = (P'T)^-1 T'R+ : makes the new directions A-conjugate to P
//     P+ = (-R+ + P beta) W                              W = inverse transposed Cholesky factor of the Gram matrix of (-R+ + P beta):
//                                                        directions stay orthonormal, the s x s systems well conditioned
// Every s x s matrix (P'T, P'R, T'R, T'T, R'R) comes from ONE pass over the panels (k_xtb_rows, MFMA with the rows as the contraction
// index); R+'R+ and the Gram matrix of the new directions follow from them algebraically (exact for the R+ actually formed, the
// identity the single-vector loop of xt.hip uses for r'.r'), so an iteration has no second global reduction:
//     k_xtb_apply (+ k_xtb_neigh)   T = A P: tiles on the matrix cores; neighbour part Xs as CSR x panel
//     k_xtb_rows                    partial sums -> S rows of T; partial Gram matrices
//     k_xtb_gred + k_xtb_small      Gram matrices in a fixed order; ONE wave: the s x s algebra, stop test on column 0 (||r||^2 <= tol^2)
//     k_xtb_step                    Y, R, P, Q = S P as 16-row x 16 x 16 MFMA products
// Column 0 carries the reference's right-hand side and start vector; the result is its solution, to the same stop test.  The iterate
// sequence is NOT the reference's (s = 1 keeps that: xt.hip).
//
// Tile x panel product (k_xtb_apply), per 32 x 32 sub-block (instruction and lane maps: see the kernel):
//   column sums  Yc[col][v] += sum_row T[row][col] Qr[row][v]:  the 8 wave loads of the stream (lane (cc, rr) holds rows 4 j + rr, columns
//                2 cc, 2 cc + 1) ARE the A operands (tile row on the k index): no data movement.
//   row sums     Yr[row][v] += sum_col T[row][col] Qc[col][v]:  needs the sub-block with the COLUMN on the k index: one round trip through
//                wave-private LDS (8 ds_write_b128 into an XOR-swizzled image, 8 ds_read_b128, both conflict-free).
// Column sums stay in accumulator registers over the run of tiles (one 256-column strip), the four waves of a workgroup leave one
// combined record; row sums (32 x s) go to a grid-indexed array per tile.
// Only column 0 of Y is kept (a vector): the auxiliary solutions are never needed.  The neighbour part gathers P and the scaling, so no
// scaled full-length copy of P exists; the compact scaled copy over S (QS) feeds the tiles.
// The split polynomial preconditioner (dkmc_set_x_poly) and the row gather the neighbour part shares with it: xtb_precond.h.  Its one-polynomial form
// (dkmc_set_x_poly_form: the same loop in transformed variables, one q(N) per sweep): k_xtb_gram1, k_xtb_step1 and the `one` branches of xtb_cg_body.
// The fold of the grid-indexed row sums in that loop reads only the cells of the launch view's tiles (dkmc_set_x_fold_form: xtb_wlist_sum2, `listf` in
// xtb_cg_body); every other loop folds the window range of a row block over zeroed cells (xtb_list_sum2).
#include "xtiles.h"
#include "slab.h"
#include <hip/hip_ext.h>
#include <algorithm>
#include <functional>
#include <type_traits>
#include <vector>

#define XB_SP 16                      // vectors per panel row (padded block width)
#define XB_MAXPOLY 16                 // largest degree of the split polynomial preconditioner (dkmc_set_x_poly)
#define XB_MAXPOLY1 20                // largest degree of the one-polynomial form (dkmc_set_x_poly_form): what monomial Horner carries
#define XB_DSPLIT 8                   // workgroups per driver row of Xs
#define XB_NG 6                       // Gram matrices per pass: P'T, P'R, T'R, T'T, R'R, P'P
typedef double dbl4 __attribute__((ext_vector_type(4)));
#define XB_MFMA(a, b, c) __builtin_amdgcn_mfma_f64_16x16x4f64((a), (b), (c), 0, 0, 0)
#define XB_MFMA4(a, b, c) __builtin_amdgcn_mfma_f64_4x4x4f64((a), (b), (c), 0, 0, 0)

// auxiliary right-hand sides: a hash of (row, column) -> uniform in [-1, 1); the same on every rank and in tools/blockcg_proto.py
__device__ __forceinline__ double xtb_aux(int row, int col)
{
    unsigned long long h = (unsigned long long)row * 0x9E3779B97F4A7C15ull + (unsigned long long)col * 0xC2B2AE3D27D4EB4Full + 12345ull;
    h ^= h >> 29; h *= 0xBF58476D1CE4E5B9ull; h ^= h >> 32;
    return (double)(h >> 11) * (1.0 / 4503599627370496.0) - 1.0;
}
// column v of the scaled right-hand side panel at a row: the physical one, an auxiliary one, or padding.
// Auxiliary columns are a free choice (only their block Krylov space matters).  aux != nullptr: the SMOOTH set -- column v is
// cos(kx pi xi) cos(ky pi eta) cos(kz pi zeta) / s_row, (xi, eta, zeta) the atom's position scaled to the unit box and (kx, ky, kz) the v-th
// lowest mode of the Laplacian of the device's bounding box (k_xtb_modes: adapts to the aspect ratio -- along x for a narrow stack, lateral
// for a wide one).  The neighbour part of X is a graph Laplacian: its low modes are smooth, and right-hand sides rich in them deflate that end
// of the spectrum from the first sweeps (oracle's X, tools/blockcg_proto.py, x modes: 6.4e3 rows 48 -> 31 sweeps, 5.8e4 rows 95 -> 76).
// Smooth systems also CONVERGE sooner than the physical column; close to a converged tolerance (1e-10 and below) their residual columns
// vanish and the s x s systems lose rank, so below 1e-8 the hash set stays (dkmc_set_x_aux).
struct XbAux { double lo[3], hi[3]; int k[16][3]; unsigned long long mm[6]; int hs, pad_; };      // hs: columns 1 ... hs - 1 take the smooth set, hs ... s - 1 the hash set
__device__ __forceinline__ double xtb_rhs(const double *__restrict__ b, int row, int v, int s, const XbAux *__restrict__ aux = nullptr,
                                          const double *__restrict__ ax = nullptr, const double *__restrict__ ay = nullptr, const double *__restrict__ az = nullptr,
                                          const double *__restrict__ sc = nullptr)
{
    if (v == 0) return b[row];
    if (v >= s) return 0.0;
    if (!aux || v >= aux->hs) return xtb_aux(row, v);
    // rows 0 / 1: the ground-side and the source-side driver node, at the two ends of x, in the middle of the cross-section
    double u[3];
    if (row < 2) { u[0] = row == 0 ? 1.0 : 0.0; u[1] = 0.5; u[2] = 0.5; }
    else {
        const double c[3] = {ax[row - 2], ay[row - 2], az[row - 2]};
#pragma unroll
        for (int d = 0; d < 3; ++d) u[d] = aux->hi[d] > aux->lo[d] ? (c[d] - aux->lo[d]) / (aux->hi[d] - aux->lo[d]) : 0.0;
    }
    return cospi((double)aux->k[v][0] * u[0]) * cospi((double)aux->k[v][1] * u[1]) * cospi((double)aux->k[v][2] * u[2]) / sc[row];
}
// bounding box of the atoms (order-preserving integer image of c + 2^20 > 0: the result does not depend on the order of the atomics)
__global__ __launch_bounds__(256) void k_xtb_box(int na, const double *__restrict__ ax, const double *__restrict__ ay, const double *__restrict__ az, XbAux *aux)
{
    // wave minima / maxima first: one atomic per wave and bound instead of one per atom (6 x 5.8e4 atomics on six words cost 1 ms at 85 k sites)
    unsigned long long lo[3] = {~0ull, ~0ull, ~0ull}, hi[3] = {0ull, 0ull, 0ull};
    for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < na; i += gridDim.x * blockDim.x) {
        const double c[3] = {ax[i], ay[i], az[i]};
#pragma unroll
        for (int d = 0; d < 3; ++d) {
            const unsigned long long u = (unsigned long long)__double_as_longlong(c[d] + 1048576.0);
            lo[d] = u < lo[d] ? u : lo[d]; hi[d] = u > hi[d] ? u : hi[d];
        }
    }
#pragma unroll
    for (int d = 0; d < 3; ++d) {
#pragma unroll
        for (int off = 32; off > 0; off >>= 1) {
            const unsigned long long l2 = __shfl_xor(lo[d], off, WAVE), h2 = __shfl_xor(hi[d], off, WAVE);
            lo[d] = l2 < lo[d] ? l2 : lo[d]; hi[d] = h2 > hi[d] ? h2 : hi[d];
        }
        if ((threadIdx.x & 63) == 0) { atomicMin(&aux->mm[2 * d], lo[d]); atomicMax(&aux->mm[2 * d + 1], hi[d]); }
    }
}
// the s - 1 lowest non-constant modes of the box: (kx / Lx)^2 + (ky / Ly)^2 + (kz / Lz)^2 ascending over kx, ky, kz < 8, ties with the larger
// kx (then ky) first; x_only: (v, 0, 0).  One workgroup of 512: thread = candidate, its rank by counting.
__global__ __launch_bounds__(512) void k_xtb_modes(XbAux *aux, int x_only)
{
    __shared__ double ev[512];
    const int code = threadIdx.x, kx = code >> 6, ky = (code >> 3) & 7, kz = code & 7;         // code = kx * 64 + ky * 8 + kz
    double L[3];
#pragma unroll
    for (int d = 0; d < 3; ++d) {
        const double lo = __longlong_as_double((long long)aux->mm[2 * d]) - 1048576.0, hi = __longlong_as_double((long long)aux->mm[2 * d + 1]) - 1048576.0;
        if (code == 0) { aux->lo[d] = lo; aux->hi[d] = hi; }
        L[d] = hi - lo;
        if (!(L[d] > 1e-6)) L[d] = 1e-6;
    }
    ev[code] = (kx / L[0]) * (kx / L[0]) + (ky / L[1]) * (ky / L[1]) + (kz / L[2]) * (kz / L[2]);
    __syncthreads();
    if (code == 0) { aux->k[0][0] = aux->k[0][1] = aux->k[0][2] = 0; return; }
    if (x_only) { if (code < 16) { aux->k[code][0] = code; aux->k[code][1] = 0; aux->k[code][2] = 0; } return; }
    const double mine = ev[code];
    int rank = 0;
    for (int c = 1; c < 512; ++c) rank += (ev[c] < mine || (ev[c] == mine && c > code)) ? 1 : 0;
    if (rank < 15) { aux->k[rank + 1][0] = kx; aux->k[rank + 1][1] = ky; aux->k[rank + 1][2] = kz; }
}
// position of (S rank r, vector v) in the compact panel QS: rows pairwise interleaved, [r / 2][v][r % 2] -- two consecutive rows of one
// vector are one 16-byte read (two k-steps of the row product).  (The LDS copy of a strip's window adds a swizzle: k_xtb_apply.)
__device__ __forceinline__ size_t xtb_qs_pos(int r, int v) { return (size_t)(r >> 1) * 32 + 2 * v + (r & 1); }

// ---- tiles x panel -----------------------------------------------------------------------------------------------------------------
// One run of tiles per wave, the four runs of a workgroup in one strip (the run list is padded to groups of four per strip: xt.hip).
// v_mfma_f64_4x4x4_4b_f64 (four independent 4 x 4 x 4 products per instruction; lane maps probed on gfx950, tools/probe_mfma_f64_4x4x4.hip:
// A[i][k] of block n: lane i + 4 n + 16 k; B[k][j]: lane j + 4 n + 16 k; D[i][j]: lane j + 4 n + 16 i) issues every 18 cycles -- 68 TFLOP/s
// measured chip-wide, twice the 16x16x4 form (tools/bench_mfma_f64.hip: 140 cycles, 34 TFLOP/s).  The four blocks of an instruction are
// four groups of tile rows (row sums) or columns (column sums) against the SAME four vectors, so the panel operand is replicated over the
// blocks and the cost scales with NG = ceil(s / 4) vector groups: 32 NG instructions per 32 x 32 sub-block.
// TV: the stored type of the tile values.  double: the fp64 store, 8 wave loads of 16 bytes per lane and sub-block.  float (dkmc_set_x_tile_f32): its
// fp32 image at half width (xt_tval32_pos), 4 wave loads per sub-block, each lane's float4 widened (v_cvt_f64_f32) into the two dbl2 the fp64 loads
// 2 u, 2 u + 1 would have brought -- where the registers are first used (the image write, XB_WIMG / XB_COL), so everything behind the load is the same
// instruction stream on the same fp64 operands.
typedef float flt4 __attribute__((ext_vector_type(4)));
__device__ __forceinline__ void xtb_widen(const dbl2 (&s)[8], dbl2 (&v)[8])
{
#pragma unroll
    for (int j = 0; j < 8; ++j) v[j] = s[j];
}
__device__ __forceinline__ void xtb_widen(const flt4 (&s)[4], dbl2 (&v)[8])
{
#pragma unroll
    for (int u = 0; u < 4; ++u) { v[2 * u].x = (double)s[u].x; v[2 * u].y = (double)s[u].y; v[2 * u + 1].x = (double)s[u].z; v[2 * u + 1].y = (double)s[u].w; }
}
template <int NTL, int NG, int variant = 0, typename TV = double>
__global__ __launch_bounds__(XT_NT) __attribute__((amdgpu_waves_per_eu(1, 1)))
void k_xtb_apply(int nitems, const XItem *__restrict__ items, const XTile *__restrict__ tiles, int sub_base, const TV *__restrict__ tval,
                 const double *__restrict__ QS, int nW, double *__restrict__ rowpartB, double *__restrict__ colpartB, const XCtrl *ctrl)
{
    // variant 0 = the product kernel.  Every other value is the ROUND-4 FORM of the loop (stages issued in bursts, conditional loads at the tile end,
    // panel rows loaded directly), kept for same-box comparisons (dkmc_set_x_apply_form(1) = variant 8, same results as 0) and as the carrier of the
    // measurement variants of dkmc_xtb_time_apply: 1 = no matrix instructions (stream + LDS traffic only), 2 = the tile stream is not re-read
    // (matrix instructions + LDS traffic only), 3 = operand stages of one k-pair, 4 = no LDS traffic (the row sums replaced by as many products on
    // the loaded registers), 7 = 2 and 4 together (the matrix instructions alone); 10 = the PRODUCT form without re-reading the tile stream; the
    // results of 1, 2, 4, 7 and 10 are meaningless
    constexpr int so = 4 * NG;                                                 // vectors per row of the partial-sum arrays
    constexpr bool PF = variant == 0 || variant == 10 || variant == 12;        // product form of the loop (12, measurement: partial tiles skipped)
    constexpr bool F32 = sizeof(TV) == 4;
    constexpr int NL = F32 ? 4 : 8;                                            // wave loads (16 bytes per lane) per sub-block
    typedef typename std::conditional<F32, flt4, dbl2>::type XV;               // what a lane loads at once
    __shared__ __attribute__((aligned(16))) double qc[XT_C * XB_SP];          // the strip's 256 panel rows in QS order (32 KiB)
    __shared__ __attribute__((aligned(16))) double ts[4 * 2 * XT_SUB];        // per wave: two sub-block images (2 x 8 KiB)
    __shared__ __attribute__((aligned(16))) double brs[PF ? 4 * XT_R * XB_SP : 2];   // per wave: the next tile's 32 panel rows (4 KiB)
    const int wv = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    const int lane = threadIdx.x & 63, cc = lane & 15, rr = lane >> 4, jv = lane & 3, blk = cc >> 2;
    const int item = (int)blockIdx.x * 4 + wv;
    const XItem it = items[min(item, nitems - 1)];
    if (ctrl->done) return;                                                    // uniform over the launch
    {   // the window of the strip, 16-byte chunks (vector v of a row pair) in QS order except for a swizzle of the vector index by
        // 4 (row pair % 4): the four row pairs a wave reads at once then sit on different LDS banks
        const dbl2 *src = reinterpret_cast<const dbl2 *>(QS + (size_t)it.w * XT_C * XB_SP);
        dbl2 *dst = reinterpret_cast<dbl2 *>(qc);
#pragma unroll
        for (int u = 0; u < 8; ++u) { const int ch = threadIdx.x + 256 * u; dst[ch ^ (((ch >> 4) & 3) << 2)] = src[ch]; }
    }
    __syncthreads();
    double *tsw = ts + (size_t)wv * 2 * XT_SUB;
    double *brw = brs + (PF ? (size_t)wv * XT_R * XB_SP : 0);
    double Yc[8][2][NG];
#pragma unroll
    for (int q = 0; q < 8; ++q)
#pragma unroll
        for (int e = 0; e < 2; ++e)
#pragma unroll
            for (int g = 0; g < NG; ++g) Yc[q][e][g] = 0.0;
    // LDS offsets (doubles) of this lane.  Sub-block image: g(r, c) = 32 r + (c ^ ((r & 15) << 1)), written as the loads arrive (lane
    // (cc, rr) holds rows 4 j + rr, columns 2 cc, 2 cc + 1), read with the row on the lane (row 16 mb + cc, columns 8 kk + 2 rr, + 1)
    int woff[8];
#pragma unroll
    for (int j = 0; j < 8; ++j) { const int r = 4 * j + rr; woff[j] = 32 * r + ((2 * cc) ^ ((r & 15) << 1)); }
    const int roff = 32 * cc;                                                  // + 512 mb + ((8 kk + 2 rr) ^ (cc << 1))
    // panel operands: vector 4 g + jv of panel row rho sits at xtb_qs_pos(rho, 4 g + jv); for rho = 32 q + 8 kk + 2 rr (+ 1): one 16-byte read
    int qoff[NG];
#pragma unroll
    for (int g = 0; g < NG; ++g) qoff[g] = rr * 32 + ((2 * (4 * g + jv)) ^ (rr << 3));      // + (16 q + 4 kk) * 32
    // the stream registers of `dst` are dst_s (as loaded); dst itself holds the fp64 operands from XB_WIDEN on
#define XB_LD(dst, slot) if ((variant != 2 && variant != 7 && variant != 10) || (slot) < 2) { _Pragma("unroll") for (int j_ = 0; j_ < NL; ++j_) dst##_s[j_] = NTL ? __builtin_nontemporal_load(base + (size_t)(NL * (slot) + j_) * 64) : base[(size_t)(NL * (slot) + j_) * 64]; }
#define XB_WIDEN(vv) xtb_widen(vv##_s, vv);
    // panel operands of the column sums: rows 4 j + rr of a tile's 32 panel rows, vectors 4 g + jv (the same in all four blocks)
#define XB_LDBR(k_)                                                                                                            \
    {                                                                                                                           \
        const double *qr_ = QS + (size_t)(k_) * XT_R * XB_SP;                                                                   \
        _Pragma("unroll") for (int j_ = 0; j_ < 8; ++j_) {                                                                      \
            const int rho_ = 4 * j_ + rr, r32_ = rho_ >> 1;                                                                     \
            _Pragma("unroll") for (int g_ = 0; g_ < NG; ++g_) br[j_][g_] = qr_[r32_ * 32 + 2 * (4 * g_ + jv) + (rho_ & 1)];      \
        }                                                                                                                       \
    }
    // the same rows by way of LDS -- four coalesced 16-byte loads per lane EARLY in the tile (LDBN), a plain copy into brw (WBN), read back in br's
    // lane map once the tile's last column sums are issued (RDBRH).  vmcnt retires in order: loaded at the END of a tile (round-4 form) these rows sat
    // behind the prefetched sub-blocks and the next tile's first stage drained the queue
#define XB_LDBN(k_) { const dbl2 *qn_ = reinterpret_cast<const dbl2 *>(QS + (size_t)(k_) * XT_R * XB_SP) + lane; _Pragma("unroll") for (int u_ = 0; u_ < 4; ++u_) bn[u_] = qn_[64 * u_]; }
#define XB_WBN() { dbl2 *bw_ = reinterpret_cast<dbl2 *>(brw) + lane; _Pragma("unroll") for (int u_ = 0; u_ < 4; ++u_) bw_[64 * u_] = bn[u_]; }
    // One sub-block = four stages of 8 NG matrix instructions each, software-pipelined by hand: hipcc issues an LDS read right in front of
    // the instructions that use it (measured: one exposed LDS latency per 4 matrix instructions, 3.5 ms per sweep at 9.4e5 sites where the
    // instructions alone take 1.9), so the operands of the row sums are requested one stage ahead and sched_barriers keep the order:
    //   image -> LDS | read operands of k-pairs 0, 1 | COLUMN sums, loads 0-3 | read operands of k-pairs 2, 3 | ROW sums, k-pairs 0, 1 |
    //   COLUMN sums, loads 4-7 | ROW sums, k-pairs 2, 3
    // Column sums come straight from the loaded registers (they are the A operands with the tile ROW on the k index); row sums from the
    // image read back with the tile COLUMN on the k index.
    struct RowOps { dbl2 a0[2], a1[2], bc[2][NG]; };
#define XB_RDROW(R, q, bufi, kk0)                                                                                              \
    {                                                                                                                           \
        const double *img_ = tsw + (bufi) * XT_SUB;                                                                             \
        _Pragma("unroll") for (int h_ = 0; h_ < 2; ++h_) {                                                                      \
            const int sw_ = (8 * ((kk0) + h_) + 2 * rr) ^ (cc << 1);                                                            \
            R.a0[h_] = *reinterpret_cast<const dbl2 *>(img_ + roff + sw_);                                                      \
            R.a1[h_] = *reinterpret_cast<const dbl2 *>(img_ + roff + 512 + sw_);                                                \
            _Pragma("unroll") for (int g_ = 0; g_ < NG; ++g_)                                                                   \
                R.bc[h_][g_] = *reinterpret_cast<const dbl2 *>(qc + qoff[g_] + (16 * (q) + 4 * ((kk0) + h_)) * 32);             \
        }                                                                                                                       \
    }
#define XB_COLH(vv, q, j0)                                                                                                     \
    if (variant != 1) {                                                                                                         \
        _Pragma("unroll") for (int j_ = (j0); j_ < (j0) + 4; ++j_)                                                              \
            _Pragma("unroll") for (int g_ = 0; g_ < NG; ++g_) {                                                                 \
                Yc[q][0][g_] = XB_MFMA4(vv[j_].x, br[j_][g_], Yc[q][0][g_]);                                                    \
                Yc[q][1][g_] = XB_MFMA4(vv[j_].y, br[j_][g_], Yc[q][1][g_]);                                                    \
            }                                                                                                                   \
    }
#define XB_ROWH(R)                                                                                                             \
    _Pragma("unroll") for (int h_ = 0; h_ < 2; ++h_)                                                                            \
        _Pragma("unroll") for (int g_ = 0; g_ < NG; ++g_) {                                                                     \
            if (variant != 1) {                                                                                                 \
                Yr[0][g_] = XB_MFMA4(R.a0[h_].x, R.bc[h_][g_].x, Yr[0][g_]); Yr[1][g_] = XB_MFMA4(R.a1[h_].x, R.bc[h_][g_].x, Yr[1][g_]); \
                Yr[0][g_] = XB_MFMA4(R.a0[h_].y, R.bc[h_][g_].y, Yr[0][g_]); Yr[1][g_] = XB_MFMA4(R.a1[h_].y, R.bc[h_][g_].y, Yr[1][g_]); \
            } else { Yr[0][g_] += R.a0[h_].x + R.bc[h_][g_].x; Yr[1][g_] += R.a1[h_].y + R.bc[h_][g_].y; }                       \
        }
    // variant 3 (measurement): stages of ONE k-pair (16 matrix instructions at s = 16) instead of two: half the staging registers
    struct RowOps1 { dbl2 a0, a1, bc[NG]; };
#define XB_RD1(R, q, bufi, kk_)                                                                                                \
    {                                                                                                                           \
        const double *img_ = tsw + (bufi) * XT_SUB;                                                                             \
        const int sw_ = (8 * (kk_) + 2 * rr) ^ (cc << 1);                                                                       \
        R.a0 = *reinterpret_cast<const dbl2 *>(img_ + roff + sw_);                                                              \
        R.a1 = *reinterpret_cast<const dbl2 *>(img_ + roff + 512 + sw_);                                                        \
        _Pragma("unroll") for (int g_ = 0; g_ < NG; ++g_) R.bc[g_] = *reinterpret_cast<const dbl2 *>(qc + qoff[g_] + (16 * (q) + 4 * (kk_)) * 32); \
    }
#define XB_ROW1(R)                                                                                                             \
    _Pragma("unroll") for (int g_ = 0; g_ < NG; ++g_) {                                                                         \
        Yr[0][g_] = XB_MFMA4(R.a0.x, R.bc[g_].x, Yr[0][g_]); Yr[1][g_] = XB_MFMA4(R.a1.x, R.bc[g_].x, Yr[1][g_]);               \
        Yr[0][g_] = XB_MFMA4(R.a0.y, R.bc[g_].y, Yr[0][g_]); Yr[1][g_] = XB_MFMA4(R.a1.y, R.bc[g_].y, Yr[1][g_]);               \
    }
#define XB_COLQ(vv, q, j0)                                                                                                     \
    _Pragma("unroll") for (int j_ = (j0); j_ < (j0) + 2; ++j_)                                                                  \
        _Pragma("unroll") for (int g_ = 0; g_ < NG; ++g_) {                                                                     \
            Yc[q][0][g_] = XB_MFMA4(vv[j_].x, br[j_][g_], Yc[q][0][g_]);                                                        \
            Yc[q][1][g_] = XB_MFMA4(vv[j_].y, br[j_][g_], Yc[q][1][g_]);                                                        \
        }
#define XB_SB() __builtin_amdgcn_sched_barrier(0);
#define XB_COL(vv, q, bufi)                                                                                                    \
    {                                                                                                                           \
        double *img_ = tsw + (bufi) * XT_SUB;                                                                                   \
        XB_WIDEN(vv)                                                                                                            \
        if (variant != 4 && variant != 7) { _Pragma("unroll") for (int j_ = 0; j_ < 8; ++j_) *reinterpret_cast<dbl2 *>(img_ + woff[j_]) = vv[j_]; } \
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");                                                                  \
        __builtin_amdgcn_wave_barrier();                                                                                        \
        __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");                                                                  \
        if (variant == 4 || variant == 7) {                                                                                     \
            XB_COLH(vv, q, 0) XB_COLH(vv, q, 4)                                                                                 \
            _Pragma("unroll") for (int j_ = 0; j_ < 8; ++j_)                                                                    \
                _Pragma("unroll") for (int g_ = 0; g_ < NG; ++g_) {                                                             \
                    Yr[0][g_] = XB_MFMA4(vv[j_].x, br[j_][g_], Yr[0][g_]); Yr[1][g_] = XB_MFMA4(vv[j_].y, br[j_][g_], Yr[1][g_]); \
                }                                                                                                               \
        } else if (variant == 3) {                                                                                              \
            XB_RD1(Ra, q, bufi, 0) XB_SB() XB_COLQ(vv, q, 0) XB_SB() XB_RD1(Rb, q, bufi, 1) XB_SB() XB_ROW1(Ra) XB_SB()         \
            XB_COLQ(vv, q, 2) XB_SB() XB_RD1(Ra, q, bufi, 2) XB_SB() XB_ROW1(Rb) XB_SB() XB_COLQ(vv, q, 4) XB_SB()              \
            XB_RD1(Rb, q, bufi, 3) XB_SB() XB_ROW1(Ra) XB_SB() XB_COLQ(vv, q, 6) XB_SB()                                        \
        } else {                                                                                                                \
        XB_RDROW(R0, q, bufi, 0)                                                                                                \
        __builtin_amdgcn_sched_barrier(0);                                                                                      \
        XB_COLH(vv, q, 0)                                                                                                       \
        __builtin_amdgcn_sched_barrier(0);                                                                                      \
        XB_RDROW(R1, q, bufi, 2)                                                                                                \
        __builtin_amdgcn_sched_barrier(0);                                                                                      \
        XB_COLH(vv, q, 4)                                                                                                       \
        __builtin_amdgcn_sched_barrier(0);                                                                                      \
        }                                                                                                                       \
    }
#define XB_ROW(q, bufi)                                                                                                        \
    {                                                                                                                           \
        if (variant == 4 || variant == 7) { }                                                                                   \
        else if (variant == 3) { XB_ROW1(Rb) XB_SB() }                                                                          \
        else { XB_ROWH(R0) __builtin_amdgcn_sched_barrier(0); XB_ROWH(R1) __builtin_amdgcn_sched_barrier(0); }                  \
    }
    // PRODUCT FORM (variant 0): the same four stages of 8 NG matrix instructions, but nothing is issued in a burst BETWEEN stages: the LDS reads of the row operands,
    // the image write of the next sub-block and the stream loads ride INSIDE a stage, spread over its matrix instructions by sched_group_barriers
    // (an instruction of another pipe issues in the shadow of a matrix instruction; a burst of 12-20 LDS instructions leaves the matrix pipe idle):
    //   S1: read row operands k 0,1 of q     + COLUMN sums loads 0-3        S3: load sub-block q + 2 into the free set + ROW sums k 0,1
    //   S2: read row operands k 2,3 of q     + COLUMN sums loads 4-7        S4: write the image of sub-block q + 1   + ROW sums k 2,3
#define XB_G(mask_, n_) __builtin_amdgcn_sched_group_barrier(mask_, n_, 0);
#define XB_GREP(cnt_, body_) _Pragma("unroll") for (int gi_ = 0; gi_ < (cnt_); ++gi_) { body_ }
#define XB_WIMG(vv, bufi)                                                                                                      \
    {                                                                                                                           \
        double *img_ = tsw + (bufi) * XT_SUB;                                                                                   \
        XB_WIDEN(vv)                                                                                                            \
        _Pragma("unroll") for (int j_ = 0; j_ < 8; ++j_) *reinterpret_cast<dbl2 *>(img_ + woff[j_]) = vv[j_];                    \
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");                                                                  \
        __builtin_amdgcn_wave_barrier();                                                                                        \
        __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");                                                                  \
    }
#define XB_RDBRH(j0)                                                                                                           \
    _Pragma("unroll") for (int j_ = (j0); j_ < (j0) + 4; ++j_) {                                                                \
        const int rho_ = 4 * j_ + rr; const int r32_ = rho_ >> 1;                                                                          \
        _Pragma("unroll") for (int g_ = 0; g_ < NG; ++g_) br[j_][g_] = brw[r32_ * 32 + 2 * (4 * g_ + jv) + (rho_ & 1)];         \
    }
    // groups: 0x008 matrix instruction, 0x020 VMEM read, 0x100 LDS read, 0x200 LDS write.  MF = matrix instructions of a stage (8 NG)
    // (fp32 stream: the two conversions of an image write, 0x002 VALU, ride in front of it; a stage carries NL stream loads)
#define XB_GV(n_) if (F32) { XB_G(0x002, n_) }
#define XB6_S1(vv, q) { XB_RDROW(R0, q, (q) & 1, 0) XB_COLH(vv, q, 0) XB_GREP(2 + NG, XB_G(0x008, 2) XB_G(0x100, 2)) XB_G(0x008, 8 * NG - 2 * (2 + NG)) } XB_SB()
#define XB6_S2(vv, q) { XB_RDROW(R1, q, (q) & 1, 2) XB_COLH(vv, q, 4) XB_GREP(2 + NG, XB_G(0x008, 2) XB_G(0x100, 2)) XB_G(0x008, 8 * NG - 2 * (2 + NG)) } XB_SB()
#define XB6_S3(LOAD, EXTRA, NEX) { LOAD EXTRA XB_ROWH(R0) XB_GREP(NL + (NEX), XB_G(0x008, 1) XB_G(0x020, 1)) XB_G(0x008, 8 * NG - NL - (NEX)) } XB_SB()
#define XB6_S4(vo, qn, EXTRA, NEX) { XB_WIMG(vo, (qn) & 1) EXTRA XB_ROWH(R1) XB_GREP(8 + (NEX), XB_G(0x008, 1) XB_GV(2) XB_G(0x200, 1)) XB_G(0x008, 8 * NG - 8 - (NEX)) } XB_SB()
#define XB6_SUB(vv, vo, q, LOAD, E3, N3, E4, N4) XB6_S1(vv, q) XB6_S2(vv, q) XB6_S3(LOAD, E3, N3) XB6_S4(vo, (q) + 1, E4, N4)
#define XB_SUBBLOCK(vv, q, bufi) XB_COL(vv, q, bufi) XB_ROW(q, bufi)
    // The stream is pipelined ACROSS tiles: the first two sub-blocks of the next tile of the run (contiguous in the store) and its panel
    // rows are requested inside the last sub-block of this one -- one wave per SIMD holds two sub-blocks in flight, and a tile that
    // starts with a cold load exposes a full HBM latency per 8 phases of ~1.2 us (measured: 3.6 against 2.9 ms per sweep at 9.4e5 sites).
    XTile td; td.k = it.k0; td.w = it.w; td.mask = it.mask0; td.soff = it.soff0;
    double br[8][NG];
    RowOps R0, R1;
    RowOps1 Ra, Rb;
    if (it.t0 < it.t1) XB_LDBR(td.k)
    // row sums of a tile: D[i][j] of block n of Yr[mb][g]: row 16 mb + 4 n + i (i = rr, n = blk), vector 4 g + jv
#define XB_ROWSUMS()                                                                                                           \
    {                                                                                                                           \
        double *rp_ = rowpartB + (((size_t)td.k * nW + td.w) * XT_R + 4 * blk + rr) * so + jv;                                  \
        _Pragma("unroll") for (int g_ = 0; g_ < NG; ++g_) { rp_[4 * g_] = Yr[0][g_]; rp_[(size_t)16 * so + 4 * g_] = Yr[1][g_]; } \
    }
    int t = it.t0;
#pragma unroll 1
    while (t < it.t1) {
        if (td.mask != 0xffu) {
            // partial tile (a few per cent of the storage): one sub-block at a time
            double Yr[2][NG];
#pragma unroll
            for (int g = 0; g < NG; ++g) { Yr[0][g] = 0.0; Yr[1][g] = 0.0; }
            const XV *base = reinterpret_cast<const XV *>(tval + (size_t)(td.soff - sub_base) * XT_SUB) + lane;
            int sl = 0;
#pragma unroll
            for (int q = 0; q < 8; ++q) {
                if (variant != 12 && ((td.mask >> q) & 1u)) {
                    dbl2 vp[8]; XV vp_s[NL];
                    XB_LD(vp, sl)
                    XB_SUBBLOCK(vp, q, q & 1)
                    ++sl;
                }
            }
            XB_ROWSUMS()
            ++t;
            if (t < it.t1) { td = tiles[t]; XB_LDBR(td.k) }
            continue;
        }
        // a chain of full tiles (64 KiB each, contiguous in the store): two sub-blocks in flight, primed once per chain and carried across
        // its tiles (a ring of four was measured: no faster, the registers are better spent on the operand pipeline above)
        dbl2 va[8], vb[8]; XV va_s[NL], vb_s[NL];
        {
            const XV *base = reinterpret_cast<const XV *>(tval + (size_t)(td.soff - sub_base) * XT_SUB) + lane;
            XB_LD(va, 0)
            XB_LD(vb, 1)
            if (PF) XB_WIMG(va, 0)
        }
        bool chain;
        dbl2 bn[4];
#pragma unroll 1
        do {
            XTile nxt = td;
            const bool more = t + 1 < it.t1;
            if (PF) nxt = tiles[min(t + 1, it.t1 - 1)];            // the tile itself at the end of the run
            else if (more) nxt = tiles[t + 1];
            chain = more && nxt.mask == 0xffu;
            double Yr[2][NG];
#pragma unroll
            for (int g = 0; g < NG; ++g) { Yr[0][g] = 0.0; Yr[1][g] = 0.0; }
            const XV *base = reinterpret_cast<const XV *>(tval + (size_t)(td.soff - sub_base) * XT_SUB) + lane;
            // (the stream registers of a sub-block are free once its image is written and its COLUMN sums are issued -- the row sums read the image --:
            // the loads of sub-block n + 2 go out there, a sub-block and a half ahead of their use instead of one: at 1.1 us of matrix work per
            // sub-block the loaded HBM latency of ~1.8 us was exposed on every sub-block)
            if (PF) {
                // No load under a condition in the body of a chain: hipcc's vmcnt counts must assume a conditional load was NOT issued, and the wait
                // for an older one then waits for it too (round-4 form: a full drain in sub-block 7 and at every tile start).  Past the end of a chain
                // the two slots re-read the first KiB of this tile (stride 0: cache hits, discarded)
                const XV *base1 = base;
                const size_t lstr = chain ? 64 : 0;
#define XB_LDN(dst, slot) if (variant != 10) { _Pragma("unroll") for (int j_ = 0; j_ < NL; ++j_) dst##_s[j_] = NTL ? __builtin_nontemporal_load(base1 + (size_t)(NL * (slot) + j_) * lstr) : base1[(size_t)(NL * (slot) + j_) * lstr]; }
                XB6_SUB(va, vb, 0, XB_LD(va, 2), , 0, , 0)
                XB6_SUB(vb, va, 1, XB_LD(vb, 3), XB_LDBN(nxt.k), 4, , 0)
                XB6_SUB(va, vb, 2, XB_LD(va, 4), , 0, , 0)
                XB6_SUB(vb, va, 3, XB_LD(vb, 5), , 0, , 0)
                XB6_SUB(va, vb, 4, XB_LD(va, 6), , 0, , 0)
                XB6_SUB(vb, va, 5, XB_LD(vb, 7), , 0, XB_WBN(), 4)
                XB6_SUB(va, vb, 6, XB_LDN(va, 8), , 0, , 0)
                // the tile's last column sums are issued after S2: the next tile's panel rows come back from LDS inside S3 and S4
                XB6_S1(vb, 7) XB6_S2(vb, 7)
                { XB_LDN(vb, 9) XB_RDBRH(0) XB_ROWH(R0)
                  XB_GREP(4 * NG, XB_G(0x008, 1) XB_G(0x100, 1)) XB_GREP(NL, XB_G(0x008, 1) XB_G(0x020, 1)) XB_G(0x008, 4 * NG - NL) } XB_SB()
                { XB_WIMG(va, 0) XB_RDBRH(4) XB_ROWH(R1)
                  XB_GREP(8, XB_G(0x008, 1) XB_GV(2) XB_G(0x200, 1)) XB_GREP(4 * NG, XB_G(0x008, 1) XB_G(0x100, 1)) XB_G(0x008, 4 * NG - 8) } XB_SB()
#undef XB_LDN
            } else {
                // round-4 form
                XB_COL(va, 0, 0) XB_LD(va, 2) XB_ROW(0, 0)
                XB_COL(vb, 1, 1) XB_LD(vb, 3) XB_ROW(1, 1)
                XB_COL(va, 2, 0) XB_LD(va, 4) XB_ROW(2, 0)
                XB_COL(vb, 3, 1) XB_LD(vb, 5) XB_ROW(3, 1)
                XB_COL(va, 4, 0) XB_LD(va, 6) XB_ROW(4, 0)
                XB_COL(vb, 5, 1) XB_LD(vb, 7) XB_ROW(5, 1)
                XB_COL(va, 6, 0)
                if (chain) { XB_LD(va, 8) }                                 // the next tile's first sub-block
                XB_ROW(6, 0)
                XB_COL(vb, 7, 1)
                if (more) XB_LDBR(nxt.k)                                    // this tile's column sums are issued: the panel registers are free
                if (chain) { XB_LD(vb, 9) }
                XB_ROW(7, 1)
            }
            XB_ROWSUMS()
            td = nxt;
            ++t;
        } while (chain);
    }
#undef XB_ROWSUMS
#undef XB_LD
#undef XB_WIDEN
#undef XB_GV
#undef XB_LDBR
#undef XB_LDBN
#undef XB_WBN
#undef XB_COL
#undef XB_ROW
#undef XB_RD1
#undef XB_ROW1
#undef XB_COLQ
#undef XB_SB
#undef XB_RDROW
#undef XB_COLH
#undef XB_ROWH
#undef XB_SUBBLOCK
#undef XB_G
#undef XB_GREP
#undef XB_WIMG
#undef XB_RDBRH
#undef XB6_S1
#undef XB6_S2
#undef XB6_S3
#undef XB6_S4
#undef XB6_SUB
    // one record of column sums per workgroup: the four waves' accumulators are added in a fixed order through LDS, four sub-block
    // positions per round.  Yc[q][e][g] of lane (block n = blk, i = rr, j = jv) is column 32 q + 8 n + 2 i + e, vector 4 g + jv.
    double *rec = colpartB + (size_t)it.pad * XT_C * so;
#pragma unroll
    for (int h = 0; h < 2; ++h) {
        __syncthreads();                                                     // every wave is done with its images (and with the previous round)
#pragma unroll
        for (int q4 = 0; q4 < 4; ++q4)
#pragma unroll
            for (int e = 0; e < 2; ++e)
#pragma unroll
                for (int g = 0; g < NG; ++g) tsw[((q4 * 2 + e) * NG + g) * 64 + lane] = Yc[4 * h + q4][e][g];
        __syncthreads();
#pragma unroll
        for (int e = 0; e < 2; ++e)
#pragma unroll
            for (int g = 0; g < NG; ++g) {
                const int idx = ((wv * 2 + e) * NG + g) * 64 + lane;
                const double sum = (ts[idx] + ts[2 * XT_SUB + idx]) + (ts[4 * XT_SUB + idx] + ts[6 * XT_SUB + idx]);
                rec[(size_t)(32 * (4 * h + wv) + 8 * blk + 2 * rr + e) * so + 4 * g + jv] = sum;
            }
    }
}

#include "xtb_precond.h"

// ---- neighbour part Xs x panel ------------------------------------------------------------------------------------------------------
// Workgroups [0, 2 XB_DSPLIT): the two driver rows (thousands of entries each), XB_DSPLIT slices per row, partial sums to drvpart (finished
// by k_xtb_rows).  The rest: 16 atom rows per workgroup, 16 lanes per row (one per vector).  Non-S rows are finished (scaled) here; S rows
// leave their sparse sum in T for k_xtb_rows.
// Slab-distributed solve (rowlist != nullptr): the atom rows are the nlist rows of this rank's list; a driver row's partial sums run over the
// columns this rank OWNS (the drivers' own columns 0 / 1 count for rank 0), the owners' partials are added in rank order by k_xtb_rows_slab.
__global__ __launch_bounds__(XT_NT) void k_xtb_neigh(int m, const xrp_t *__restrict__ rp, const int *__restrict__ ci, const double *__restrict__ val,
                                                     const double *__restrict__ P, const double *__restrict__ sc, const int *__restrict__ nsrank,
                                                     const XCtrl *ctrl, double *__restrict__ T, double *__restrict__ drvpart,
                                                     const int *__restrict__ rowlist = nullptr, int nlist = 0, const int *__restrict__ dlist = nullptr, int nd0 = 0, int nd1 = 0)
{
    __shared__ double red[16][16];
    if (ctrl->done) return;
    const int v = threadIdx.x & 15, g = threadIdx.x >> 4;
    if (blockIdx.x < 2 * XB_DSPLIT) {
        const int row = blockIdx.x / XB_DSPLIT, part = blockIdx.x % XB_DSPLIT;
        const xrp_t p0 = rp[row], p1 = rp[row + 1];
        const xrp_t len = p1 - p0, a = p0 + len * part / XB_DSPLIT, b = p0 + len * (part + 1) / XB_DSPLIT;
        double s0 = 0.0, s1 = 0.0, s2 = 0.0, s3 = 0.0;
        xrp_t p = a + g;
        if (dlist) {
            // slab-distributed solve: dlist = positions of the entries of row 0 (nd0 of them) and row 1 (nd1) whose column this rank owns
            const int n = row == 0 ? nd0 : nd1, l0 = row == 0 ? 0 : nd0;
            const int ia = l0 + (int)((long long)n * part / XB_DSPLIT), ib = l0 + (int)((long long)n * (part + 1) / XB_DSPLIT);
            int i = ia + g;
            for (; i + 48 < ib; i += 64) {
                const int q0 = dlist[i], q1 = dlist[i + 16], q2 = dlist[i + 32], q3 = dlist[i + 48];
                const int c0 = ci[q0], c1 = ci[q1], c2 = ci[q2], c3 = ci[q3];
                s0 += val[q0] * (sc[c0] * P[(size_t)c0 * XB_SP + v]); s1 += val[q1] * (sc[c1] * P[(size_t)c1 * XB_SP + v]);
                s2 += val[q2] * (sc[c2] * P[(size_t)c2 * XB_SP + v]); s3 += val[q3] * (sc[c3] * P[(size_t)c3 * XB_SP + v]);
            }
            for (; i < ib; i += 16) { const int q0 = dlist[i], c0 = ci[q0]; s0 += val[q0] * (sc[c0] * P[(size_t)c0 * XB_SP + v]); }
            p = b;
        }
        for (; p + 48 < b; p += 64) {
            const int c0 = ci[p], c1 = ci[p + 16], c2 = ci[p + 32], c3 = ci[p + 48];
            const double a0 = val[p], a1 = val[p + 16], a2 = val[p + 32], a3 = val[p + 48];
            s0 += a0 * (sc[c0] * P[(size_t)c0 * XB_SP + v]); s1 += a1 * (sc[c1] * P[(size_t)c1 * XB_SP + v]);
            s2 += a2 * (sc[c2] * P[(size_t)c2 * XB_SP + v]); s3 += a3 * (sc[c3] * P[(size_t)c3 * XB_SP + v]);
        }
        for (; p < b; p += 16) { const int c0 = ci[p]; s0 += val[p] * (sc[c0] * P[(size_t)c0 * XB_SP + v]); }
        red[g][v] = (s0 + s1) + (s2 + s3);
        __syncthreads();
        if (g == 0) {
            double s = 0.0;
#pragma unroll
            for (int u = 0; u < 16; ++u) s += red[u][v];
            drvpart[(row * XB_DSPLIT + part) * XB_SP + v] = s;
        }
        return;
    }
    // atom rows (<= nn + 3 entries): the 16 lanes of a row first fetch ALL its entries, up to four per lane (64 entries per trip), and fold the column's
    // scaling into the values; then, batch of 16 by batch of 16, every entry is handed round the group and the 16 panel reads of the batch are issued
    // together (xn_batch16, xtb_precond.h).  A latency-bound kernel (its bytes need 0.05 ms per sweep at 9.4e5 sites, it took 0.27): what counts is dependent memory
    // rounds per row x registers per wave.  Round 4 fetched the entries of a batch inside the batch loop -- two dependent rounds per batch; here the row
    // pointer, the entries and one round per batch, at the same registers.  The additions keep the entry order of the row: same bits.
    const int li = xtb_xcd_block((int)gridDim.x - 2 * XB_DSPLIT, (int)blockIdx.x - 2 * XB_DSPLIT) * 16 + g;       // XCD-contiguous row blocks (2 XB_DSPLIT is a multiple of 8)
    const int row = rowlist ? (li < nlist ? rowlist[li] : m) : 2 + li;
    const bool ok = row < m;
    const xrp_t p0 = ok ? rp[row] : 0, p1 = ok ? rp[row + 1] : 0;
    const int nsr = ok ? nsrank[row] : 0;
    const double scr = ok ? sc[row] : 0.0;
    XnSums s = {0.0, 0.0, 0.0, 0.0};
    for (xrp_t base = p0; base < p1; base += 64) {
        int cm[4]; double wm[4];
#pragma unroll
        for (int b = 0; b < 4; ++b) { const xrp_t pe = base + 16 * b + v; cm[b] = pe < p1 ? ci[pe] : -1; wm[b] = pe < p1 ? val[pe] : 0.0; }
#pragma unroll
        for (int b = 0; b < 4; ++b) wm[b] = cm[b] >= 0 ? wm[b] * sc[cm[b]] : 0.0;
#pragma unroll
        for (int b = 0; b < 4; ++b) {
            if (base + 16 * b >= p1) break;
            s = xn_batch16(P, v, xn_entry(cm[b], wm[b]), s);
        }
    }
    const double sum = (s.s0 + s.s1) + (s.s2 + s.s3);
    if (ok) T[(size_t)row * XB_SP + v] = nsr < 0 ? scr * sum : sum;
}

// ---- row kernel: partial sums -> S rows of T, then the partial Gram matrices of this workgroup's rows ------------------------------------
// Thread (r4 = tid / 16, v = tid % 16) owns vector v of S rows r4 and r4 + 16 of a row block; wave wv thus holds rows 4 wv ... 4 wv + 3
// (and + 16) in exactly the operand map of v_mfma_f64_16x16x4_f64 with the ROW on the k index: X'Z over four rows is one MFMA.
// INIT: T = A Y0 has just been formed; R = T - B is stored and only R'R is accumulated.
__device__ __forceinline__ double xtb_list_sum(const double *__restrict__ p, size_t stride, int first, int n, int step)
{
    // terms first, first + step, ... < n of a strided list; 16 loads in flight (the tail predicated, not looped); term j goes to
    // accumulator j % 4 whatever the batching
    double a0 = 0.0, a1 = 0.0, a2 = 0.0, a3 = 0.0;
    for (int c = first; c < n; c += 16 * step) {
        double x[16];
#pragma unroll
        for (int u = 0; u < 16; ++u) { const int cu = c + u * step; x[u] = cu < n ? p[(size_t)cu * stride] : 0.0; }
#pragma unroll
        for (int u = 0; u < 16; u += 4) { a0 += x[u]; a1 += x[u + 1]; a2 += x[u + 2]; a3 += x[u + 3]; }
    }
    return (a0 + a1) + (a2 + a3);
}
// two lists of the same shape (the thread's rows r4 and r4 + 16, `off` doubles apart; p points at the thread's vector v of row r4).  Loaded as 16-byte
// pairs: the even lane of a pair takes vectors (v, v + 1) of row r4, the odd one (v - 1, v) of row r4 + 16 -- twice the bytes per load instruction of
// the 8-byte form at the same number of loads in flight -- and one DPP exchange hands each lane the sum it does not hold.  Every (row, vector) list is
// still added by ONE thread in the same grouping (term j to accumulator j % 4): same bits as the 8-byte form.
__device__ __forceinline__ void xtb_list_sum2(const double *__restrict__ p, size_t stride, size_t off, int first, int n, int v, double &sa, double &sb)
{
    const bool odd = (v & 1) != 0;
    const dbl2 *__restrict__ q = reinterpret_cast<const dbl2 *>(odd ? p - 1 + off : p);
    const size_t st2 = stride >> 1;
    double a0 = 0.0, a1 = 0.0, a2 = 0.0, a3 = 0.0, b0 = 0.0, b1 = 0.0, b2 = 0.0, b3 = 0.0;
    for (int c = first; c < n; c += 16) {
        dbl2 x[16];
#pragma unroll
        for (int u = 0; u < 16; ++u) { const int cu = c + u; x[u] = cu < n ? __builtin_nontemporal_load(q + (size_t)cu * st2) : (dbl2)(0.0); }      // (read once per sweep: non-temporal)
#pragma unroll
        for (int u = 0; u < 16; u += 4) { a0 += x[u].x; a1 += x[u + 1].x; a2 += x[u + 2].x; a3 += x[u + 3].x; b0 += x[u].y; b1 += x[u + 1].y; b2 += x[u + 2].y; b3 += x[u + 3].y; }
    }
    const double sx = (a0 + a1) + (a2 + a3), sy = (b0 + b1) + (b2 + b3);
    const double got = xor_lane<1>(odd ? sx : sy);
    sa = odd ? got : sx; sb = odd ? sy : got;
}
// The LIST FORM of the same sum over the windows of a row block (dkmc_set_x_fold_form(1); k_xtb_fold_rows): wl[0 ... n) are the windows whose cell holds
// a tile of the launch view, ascending (k_xt_wrange: the same for every thread of the workgroup, so they arrive by scalar loads); only those cells are
// loaded, 16 in flight, with the pair loads and the exchange of xtb_list_sum2.  The range form walks every window of [wl[0], wl[n - 1] + 1) and gives
// the term of window w to accumulator (w - wl[0]) % 4; a window without a tile of the view contributes +0.0 there (a zeroed cell), and x + (+0.0) = x
// bit for bit for every x an accumulator can hold (it starts at +0.0 and a sum in round-to-nearest is -0.0 only when both terms are).  Here the term of
// window w goes to the same accumulator, in the same increasing order of w, and the +0.0 terms are left out: the same bits, and no cell outside the
// list is read, so nothing has to zero one.
__device__ __forceinline__ void xtb_wlist_sum2(const double *__restrict__ p, size_t stride, size_t off, const int *__restrict__ wl, int n, int v, double &sa, double &sb)
{
    const bool odd = (v & 1) != 0;
    const dbl2 *__restrict__ q = reinterpret_cast<const dbl2 *>(odd ? p - 1 + off : p);
    const size_t st2 = stride >> 1;
    double a0 = 0.0, a1 = 0.0, a2 = 0.0, a3 = 0.0, b0 = 0.0, b1 = 0.0, b2 = 0.0, b3 = 0.0;
    const int w0 = n > 0 ? wl[0] : 0;
    for (int c = 0; c < n; c += 16) {
        dbl2 x[16]; int sel[16];
#pragma unroll
        for (int u = 0; u < 16; ++u) {
            const int cu = c + u, w = cu < n ? wl[cu] : w0;
            sel[u] = cu < n ? (w - w0) & 3 : 4;                                // (4: the predicated tail, added nowhere)
            x[u] = cu < n ? __builtin_nontemporal_load(q + (size_t)w * st2) : (dbl2)(0.0);
        }
#pragma unroll
        for (int u = 0; u < 16; ++u) {                                         // (sel is uniform over the workgroup: scalar branches)
            if (sel[u] == 0) { a0 += x[u].x; b0 += x[u].y; }
            else if (sel[u] == 1) { a1 += x[u].x; b1 += x[u].y; }
            else if (sel[u] == 2) { a2 += x[u].x; b2 += x[u].y; }
            else if (sel[u] == 3) { a3 += x[u].x; b3 += x[u].y; }
        }
    }
    const double sx = (a0 + a1) + (a2 + a3), sy = (b0 + b1) + (b2 + b3);
    const double got = xor_lane<1>(odd ? sx : sy);
    sa = odd ? got : sx; sb = odd ? sy : got;
}
// ---- sharded solve: this rank's tile sums of every S row -> the exchange buffer xbuf[ns][so]; behind them the control words: rank 0's stop
// decision and any rank's abort word.  [w_lo, w_hi): windows that can hold this rank's partial sums (every other cell of its arrays is zero)
__global__ __launch_bounds__(XT_NT) void k_xtb_fold_local(int ns, int nK, int nW, int so, const int2 *__restrict__ wrange, const int *__restrict__ nitem_w,
                                                          const double *__restrict__ rowpartB, const double *__restrict__ colpartB, double *__restrict__ xbuf,
                                                          const XCtrl *ctrl, int flag_rank0, int w_lo, int w_hi, const long long *__restrict__ sdst = nullptr)
{
    // sdst (slab-distributed solve): S rank q's so tile sums go to xbuf[sdst[q]] -- the piece for the rank that owns the row (the control words are
    // written by k_xtb_slab_tail)
    if (ctrl->done) return;
    const int v = threadIdx.x & 15, r4 = threadIdx.x >> 4;
    const int rec_shift = nitem_w[2 * (nW + 2)];
    for (int k = blockIdx.x; k < nK; k += gridDim.x) {
        int2 wr = wrange[k];
        wr.x = max(wr.x, w_lo); wr.y = min(wr.y, w_hi);
        const int wk = k / (XT_C / XT_R);
        const bool mine = wk >= w_lo && wk < w_hi;
        const int nc = mine ? nitem_w[wk] >> rec_shift : 0, cbase = nitem_w[nW + 2 + wk] >> rec_shift;
        double tA = 0.0, tB = 0.0;
        if (v < so) {
            const double *rpp = rowpartB + ((size_t)k * nW * XT_R + r4) * so + v;
            const double *cpp = colpartB + ((size_t)cbase * XT_C + (XT_R * (k % (XT_C / XT_R)) + r4)) * so + v;
            const size_t rs = (size_t)XT_R * so, cs = (size_t)XT_C * so;
            double cA, cB, rA_, rB_;
            xtb_list_sum2(cpp, cs, (size_t)16 * so, 0, nc, v, cA, cB);
            xtb_list_sum2(rpp, rs, (size_t)16 * so, wr.x, wr.y, v, rA_, rB_);
            tA = cA + rA_; tB = cB + rB_;
            const int sA = XT_R * k + r4, sB = sA + 16;
            if (sA < ns) xbuf[(sdst ? (size_t)sdst[sA] : (size_t)sA * so) + v] = tA;
            if (sB < ns) xbuf[(sdst ? (size_t)sdst[sB] : (size_t)sB * so) + v] = tB;
        }
    }
    if (!sdst && blockIdx.x == 0 && threadIdx.x == 0) {
        xbuf[(size_t)ns * so] = (flag_rank0 && ctrl->done_local) ? 1.0 : 0.0;
        xbuf[(size_t)ns * so + 1] = ctrl->abort_local ? 1.0 : 0.0;
    }
}
__global__ void k_xtb_abort_word(XCtrl *ctrl, double *xbuf, size_t slot) { ctrl->abort_local = 1; xbuf[slot] = 1.0; }
__global__ void k_xtb_set_sharded(XCtrl *ctrl) { ctrl->sharded = 1; }

// SH: sharded solve -- xbuf holds, after the all-gather, one slot of ns so + 2 doubles per rank: that rank's tile sums of the S rows, its stop
// decision and its abort word.  Every rank adds the slots IN RANK ORDER: the same bits everywhere by construction (no transport decides the
// grouping of the additions, nothing has to be re-published from rank 0), and turns rank 0's stop decision / any rank's abort word into `done`
// here, in the same iteration.
// NF (split polynomial preconditioner, dkmc_set_x_poly): T is final in every row -- folded by k_xtb_fold_rows and carried through L -- this pass only forms R (INIT) and
// the partial Gram matrices.
template <int INIT, int SH = 0, int NF = 0>
__global__ __launch_bounds__(XT_NT) void k_xtb_rows(int ns, int nK, int nW, int m, int s, int so, const int2 *__restrict__ wrange, const int *__restrict__ nitem_w,
                                                    const double *__restrict__ rowpartB, const double *__restrict__ colpartB,
                                                    const int *__restrict__ srow, const double *__restrict__ sS, const int *__restrict__ nsrank,
                                                    const double *__restrict__ sc, const double *__restrict__ drvpart, double *__restrict__ T,
                                                    const double *__restrict__ P, double *__restrict__ R, const double *__restrict__ b,
                                                    double *__restrict__ gpart, XCtrl *ctrl, const double *__restrict__ xbuf, int it, int nr,
                                                    const XbAux *__restrict__ aux, const double *__restrict__ ax, const double *__restrict__ ay, const double *__restrict__ az)
{
    const size_t xslot = (size_t)ns * so + 2;
    __shared__ double lg[4][XB_NG / 2][4][64];                                 // the four waves' Gram accumulators, three matrices at a time (24 KiB)
    __shared__ int sdone;
    if (threadIdx.x == 0) {
        sdone = ctrl->done;
        if (SH && !sdone) {
            bool ab = false;
            for (int r = 0; r < nr; ++r) ab |= xbuf[r * xslot + (size_t)ns * so + 1] != 0.0;
            if (xbuf[(size_t)ns * so] != 0.0 || ab) {                         // rank 0's stop decision; anybody's abort word
                sdone = 1;
                // stops this iteration's step kernel too; the set-up pass (it = -1) must latch a NON-ZERO stamp as well
                if (blockIdx.x == 0) { ctrl->done = it + 1 > 0 ? it + 1 : 1; if (ab) ctrl->aborted = 1; }
            }
        }
    }
    __syncthreads();
    if (sdone) return;
    const int v = threadIdx.x & 15, r4 = threadIdx.x >> 4;
    const int wv = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const int rec_shift = nitem_w[2 * (nW + 2)];
    dbl4 G[XB_NG];
#pragma unroll
    for (int g = 0; g < XB_NG; ++g) G[g] = (dbl4)(0.0);
    // ---- S rows: fold the partial sums of this workgroup's row blocks ----
    for (int k = blockIdx.x; k < nK; k += gridDim.x) {
        const int2 wr = wrange[k];
        const int wk = k / (XT_C / XT_R);
        const int nc = nitem_w[wk] >> rec_shift, cbase = nitem_w[nW + 2 + wk] >> rec_shift;
        double tA = 0.0, tB = 0.0;
        const int sA = XT_R * k + r4, sB = sA + 16;
        if (SH) {
            if (v < so) {
                for (int r = 0; r < nr; ++r) {
                    if (sA < ns) tA += xbuf[r * xslot + (size_t)sA * so + v];
                    if (sB < ns) tB += xbuf[r * xslot + (size_t)sB * so + v];
                }
            }
        } else if (!NF && v < so) {
            const double *rpp = rowpartB + ((size_t)k * nW * XT_R + r4) * so + v;
            const double *cpp = colpartB + ((size_t)cbase * XT_C + (XT_R * (k % (XT_C / XT_R)) + r4)) * so + v;
            const size_t rs = (size_t)XT_R * so, cs = (size_t)XT_C * so;
            double cA, cB, rA_, rB_;
            xtb_list_sum2(cpp, cs, (size_t)16 * so, 0, nc, v, cA, cB);
            xtb_list_sum2(rpp, rs, (size_t)16 * so, wr.x, wr.y, v, rA_, rB_);
            tA = cA + rA_; tB = cB + rB_;
        }
        double pA = 0.0, pB = 0.0, rA = 0.0, rB = 0.0;
        if (sA < ns) {
            const int row = srow[sA]; const size_t o = (size_t)row * XB_SP + v;
            if (NF) tA = T[o]; else { tA = sS[sA] * (T[o] + tA); T[o] = tA; }
            if (INIT) { rA = tA - xtb_rhs(b, row, v, s, aux, ax, ay, az, sc); R[o] = rA; } else { pA = P[o]; rA = R[o]; }
        } else tA = 0.0;
        if (sB < ns) {
            const int row = srow[sB]; const size_t o = (size_t)row * XB_SP + v;
            if (NF) tB = T[o]; else { tB = sS[sB] * (T[o] + tB); T[o] = tB; }
            if (INIT) { rB = tB - xtb_rhs(b, row, v, s, aux, ax, ay, az, sc); R[o] = rB; } else { pB = P[o]; rB = R[o]; }
        } else tB = 0.0;
        if (!INIT) {
            G[0] = XB_MFMA(pA, tA, G[0]); G[1] = XB_MFMA(pA, rA, G[1]); G[2] = XB_MFMA(tA, rA, G[2]); G[3] = XB_MFMA(tA, tA, G[3]); G[5] = XB_MFMA(pA, pA, G[5]);
            G[0] = XB_MFMA(pB, tB, G[0]); G[1] = XB_MFMA(pB, rB, G[1]); G[2] = XB_MFMA(tB, rB, G[2]); G[3] = XB_MFMA(tB, tB, G[3]); G[5] = XB_MFMA(pB, pB, G[5]);
        }
        G[4] = XB_MFMA(rA, rA, G[4]); G[4] = XB_MFMA(rB, rB, G[4]);
    }
    // ---- the other rows of this workgroup's share of the vector (finished by k_xtb_neigh; the driver rows from their partial sums).
    // Four k-steps (16 rows) of a wave in flight: the loads do not wait for the S-rank test (every row below i1 is in bounds) ----
    {
        const int chunk = ((m + (int)gridDim.x - 1) / (int)gridDim.x + 3) & ~3;
        const int i0 = blockIdx.x * chunk, i1 = min(m, i0 + chunk);
        for (int r0 = i0 + 4 * wv; r0 < i1; r0 += 64) {
            double tv[4], pv[4], rv[4]; int sr[4];
#pragma unroll
            for (int u = 0; u < 4; ++u) {
                const int row = r0 + 16 * u + (lane >> 4);
                const bool in = row < i1;
                const size_t o = (size_t)(in ? row : i0) * XB_SP + v;
                sr[u] = in ? nsrank[row] : 0;
                tv[u] = T[o];
                if (!INIT) { pv[u] = P[o]; rv[u] = R[o]; }
            }
#pragma unroll
            for (int u = 0; u < 4; ++u) {
                const int row = r0 + 16 * u + (lane >> 4);
                if (r0 + 16 * u >= i1) break;                                 // uniform over the wave
                const bool use = row < i1 && sr[u] < 0;
                const size_t o = (size_t)row * XB_SP + v;
                double t_ = use ? tv[u] : 0.0, p_ = 0.0, r_ = 0.0;
                if (!NF && use && row < 2) {
                    double sd = 0.0;
#pragma unroll
                    for (int w = 0; w < XB_DSPLIT; ++w) sd += drvpart[(row * XB_DSPLIT + w) * XB_SP + v];
                    t_ = sc[row] * sd; T[o] = t_;
                }
                if (INIT) { if (use) { r_ = t_ - xtb_rhs(b, row, v, s, aux, ax, ay, az, sc); R[o] = r_; } }
                else if (use) { p_ = pv[u]; r_ = rv[u]; }
                if (!INIT) { G[0] = XB_MFMA(p_, t_, G[0]); G[1] = XB_MFMA(p_, r_, G[1]); G[2] = XB_MFMA(t_, r_, G[2]); G[3] = XB_MFMA(t_, t_, G[3]); G[5] = XB_MFMA(p_, p_, G[5]); }
                G[4] = XB_MFMA(r_, r_, G[4]);
            }
        }
    }
    // ---- one partial per workgroup: the four waves added in a fixed order; entry (register u, lane l) is (i = l / 16 + 4 u, j = l % 16) ----
#pragma unroll
    for (int h = 0; h < 2; ++h) {
        __syncthreads();
#pragma unroll
        for (int g = 0; g < XB_NG / 2; ++g)
#pragma unroll
            for (int u = 0; u < 4; ++u) lg[wv][g][u][lane] = G[h * (XB_NG / 2) + g][u];
        __syncthreads();
        for (int e = threadIdx.x; e < (XB_NG / 2) * 256; e += XT_NT) {
            const int g = e >> 8, u = (e >> 6) & 3, l = e & 63;
            gpart[(size_t)blockIdx.x * (XB_NG * 256) + h * (XB_NG / 2) * 256 + e] = (lg[0][g][u][l] + lg[1][g][u][l]) + (lg[2][g][u][l] + lg[3][g][u][l]);
        }
    }
}
// the fold of k_xtb_rows alone: S rows of T <- scaling x (sparse sum + tile sums), driver rows from their partial sums
// wlist != null (dkmc_set_x_fold_form(1)): the row partial sums by the launch view's window lists (xtb_wlist_sum2) instead of its window ranges
__global__ __launch_bounds__(XT_NT) void k_xtb_fold_rows(int ns, int nK, int nW, int so, const int2 *__restrict__ wrange, const int *__restrict__ wlist, const int *__restrict__ nitem_w,
                                                         const double *__restrict__ rowpartB, const double *__restrict__ colpartB, const int *__restrict__ srow,
                                                         const double *__restrict__ sS, const double *__restrict__ sc, const double *__restrict__ drvpart,
                                                         double *__restrict__ T, const XCtrl *ctrl)
{
    if (ctrl->done) return;
    const int v = threadIdx.x & 15, r4 = threadIdx.x >> 4;
    const int rec_shift = nitem_w[2 * (nW + 2)];
    if (blockIdx.x == 0 && threadIdx.x < 32) {
        const int row = threadIdx.x >> 4;
        double sd = 0.0;
#pragma unroll
        for (int w = 0; w < XB_DSPLIT; ++w) sd += drvpart[(row * XB_DSPLIT + w) * XB_SP + v];
        T[(size_t)row * XB_SP + v] = sc[row] * sd;
    }
    for (int k = blockIdx.x; k < nK; k += gridDim.x) {
        const int *wl = wlist ? wlist + (size_t)k * (nW + 1) : nullptr;
        const int2 wr = wl ? make_int2(0, 0) : wrange[k];
        const int wk = k / (XT_C / XT_R);
        const int nc = nitem_w[wk] >> rec_shift, cbase = nitem_w[nW + 2 + wk] >> rec_shift;
        double tA = 0.0, tB = 0.0;
        const int sA = XT_R * k + r4, sB = sA + 16;
        if (v < so) {
            const double *rpp = rowpartB + ((size_t)k * nW * XT_R + r4) * so + v;
            const double *cpp = colpartB + ((size_t)cbase * XT_C + (XT_R * (k % (XT_C / XT_R)) + r4)) * so + v;
            const size_t rs = (size_t)XT_R * so, cs = (size_t)XT_C * so;
            double cA, cB, rA_, rB_;
            xtb_list_sum2(cpp, cs, (size_t)16 * so, 0, nc, v, cA, cB);
            if (wl) xtb_wlist_sum2(rpp, rs, (size_t)16 * so, wl + 1, wl[0], v, rA_, rB_);
            else xtb_list_sum2(rpp, rs, (size_t)16 * so, wr.x, wr.y, v, rA_, rB_);
            tA = cA + rA_; tB = cB + rB_;
        }
        if (sA < ns) { const size_t o = (size_t)srow[sA] * XB_SP + v; T[o] = sS[sA] * (T[o] + tA); }
        if (sB < ns) { const size_t o = (size_t)srow[sB] * XB_SP + v; T[o] = sS[sB] * (T[o] + tB); }
    }
}
// ---- Gram matrices: the row kernel's partials, reduced in a fixed order ----------------------------------------------------------------
// 16 entries per workgroup, 16 slices of the partial list per entry (slice q adds partials q, q + 16, ...), the slices combined in order.
__global__ __launch_bounds__(XT_NT) void k_xtb_gred(int npart, const double *__restrict__ gpart, double *__restrict__ gfin, const XCtrl *ctrl)
{
    __shared__ double red[16][17];
    if (ctrl->done) return;
    const int el = threadIdx.x & 15, q = threadIdx.x >> 4;
    const int e = 16 * (int)blockIdx.x + el;
    red[q][el] = xtb_list_sum(gpart + e, (size_t)XB_NG * 256, q, npart, 16);
    __syncthreads();
    if (q == 0) {
        double a = 0.0;
#pragma unroll
        for (int u = 0; u < 16; ++u) a += red[u][el];
        gfin[e] = a;
    }
}

// ---- the s x s algebra of one iteration: ONE wave (no workgroup barriers; the matrices live in LDS, entry (i, j) = e / 16, e % 16 of lane
// e % 64) -----------------------------------------------------------------------------------------------------------------------------------
// mats: c | M1 = -W | M2 = beta W | M3 = c M1, each 16 x 16 row-major, zero outside s x s.  it = -1: set-up (P = 0, R = A Y0 - B): only
// R'R is read; c = M2 = M3 = 0, W from R'R, first stop test on ||r|| (iterative_solvers_gpu.cu:418), later ones on ||r||^2 (:448).
#define XB_M(name) double (*name)[17]
#define XB_WSYNC() do { __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront"); __builtin_amdgcn_wave_barrier(); __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront"); } while (0)
__device__ __forceinline__ void xtb_mm(XB_M(C), XB_M(A), XB_M(B), bool ta, double alpha, XB_M(D), double delta)
{
    // C = alpha op(A) B + delta D; op = transpose if ta; D may be null; C may alias A, B or D.  All matrices are zero outside their
    // leading s x s block, so the loops run over the full 16 (compile-time bounds: the 80 LDS reads of a lane are issued together).
    // Lane l owns entries (l / 16 + 4 u, l % 16), u = 0 ... 3: one column index, four rows.
    const int j = threadIdx.x & 15, i0 = threadIdx.x >> 4;
    double bcol[16], acc[4];
#pragma unroll
    for (int k = 0; k < 16; ++k) bcol[k] = B[k][j];
#pragma unroll
    for (int u = 0; u < 4; ++u) {
        const int i = i0 + 4 * u;
        double a0 = 0.0, a1 = 0.0;
#pragma unroll
        for (int k = 0; k < 16; k += 2) { a0 += (ta ? A[k][i] : A[i][k]) * bcol[k]; a1 += (ta ? A[k + 1][i] : A[i][k + 1]) * bcol[k + 1]; }
        acc[u] = alpha * (a0 + a1) + (D ? delta * D[i][j] : 0.0);
    }
    XB_WSYNC();
#pragma unroll
    for (int u = 0; u < 4; ++u) C[i0 + 4 * u][j] = acc[u];
    XB_WSYNC();
}
__device__ __forceinline__ void xtb_symmetrise(XB_M(A), int s)
{
    double acc[4];
#pragma unroll
    for (int u = 0; u < 4; ++u) { const int e = (int)threadIdx.x + 64 * u, i = e >> 4, j = e & 15; acc[u] = (i < s && j < s) ? 0.5 * (A[i][j] + A[j][i]) : 0.0; }
    XB_WSYNC();
#pragma unroll
    for (int u = 0; u < 4; ++u) { const int e = (int)threadIdx.x + 64 * u; A[e >> 4][e & 15] = acc[u]; }
    XB_WSYNC();
}
// in-place Cholesky of the leading s x s block (lower triangle); false on a non-positive pivot (uniform: every lane reads the same pivots)
__device__ __forceinline__ bool xtb_chol(XB_M(A), int s)
{
    bool ok = true;
    if ((int)threadIdx.x >= s && threadIdx.x < 16) A[threadIdx.x][threadIdx.x] = 1.0;      // padding: unit diagonal (the rest of it is zero)
    XB_WSYNC();
    for (int k = 0; k < s; ++k) {
        const double d = A[k][k];
        if (!(d > 0.0)) ok = false;
        const double ld = sqrt(d > 0.0 ? d : 1.0);
        XB_WSYNC();
        if ((int)threadIdx.x == k) A[k][k] = ld;
        else if ((int)threadIdx.x > k && (int)threadIdx.x < s) A[threadIdx.x][k] = A[threadIdx.x][k] / ld;
        XB_WSYNC();
        const int j = threadIdx.x & 15, i0 = threadIdx.x >> 4;
        const double ljk = A[j][k];
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            const int i = i0 + 4 * u;
            if (i > k && j > k && j <= i && i < s) A[i][j] -= A[i][k] * ljk;
        }
        XB_WSYNC();
    }
    return ok;
}
// (padding rows / columns of L beyond s carry a unit diagonal, see xtb_chol: the loops below run over the full 16 with compile-time bounds)
__device__ __forceinline__ void xtb_chol_solve(XB_M(X), XB_M(L), XB_M(B), int s)
{
    const int j = threadIdx.x & 15;
    double x[16];
    if (threadIdx.x < 16) {
#pragma unroll
        for (int i = 0; i < 16; ++i) x[i] = B[i][j];
#pragma unroll
        for (int i = 0; i < 16; ++i) {
            double a = x[i];
#pragma unroll
            for (int p = 0; p < i; ++p) a -= L[i][p] * x[p];
            x[i] = a / L[i][i];
        }
#pragma unroll
        for (int i = 15; i >= 0; --i) {
            double a = x[i];
#pragma unroll
            for (int p = i + 1; p < 16; ++p) a -= L[p][i] * x[p];
            x[i] = a / L[i][i];
        }
    }
    XB_WSYNC();                                                               // X may alias B
    if (threadIdx.x < 16) {
#pragma unroll
        for (int i = 0; i < 16; ++i) X[i][j] = (i < s && j < s) ? x[i] : 0.0;
    }
    XB_WSYNC();
}
// nrg > 1 (slab-distributed solve): gfin holds one block of gstride doubles per rank -- that rank's partial Gram matrices and, behind them, its
// abort word -- all-gathered; every rank adds the blocks IN RANK ORDER: identical matrices, hence identical decisions, on every rank.
// Launched with 256 threads: all four waves load (and, nrg > 1, add) the Gram matrices into LDS, then wave 0 does the algebra alone (one wave
// summing 24 x nrg dependent loads took 73 us at nrg = 8).
__global__ __launch_bounds__(256) void k_xtb_small(int it, int s, const double *__restrict__ gfin, double *__restrict__ mats, XCtrl *ctrl, double tol2,
                                                   int nrg = 1, int gstride = 0)
{
    __shared__ double Gm[XB_NG][16][17], Lp[16][17], Cm[16][17], Vm[16][17], Bm[16][17], Grn[16][17], Gprn[16][17], Gg[16][17], Wm[16][17], Tm[16][17];
    if (ctrl->done) return;
    if (nrg > 1) {
        bool ab = false;
        for (int r = 0; r < nrg; ++r) ab |= gfin[(size_t)r * gstride + XB_NG * 256 + 1] != 0.0;
        if (ab) { if (threadIdx.x == 0) { ctrl->aborted = 1; ctrl->done = it + 1 > 0 ? it + 1 : 1; } return; }      // uniform: every lane read the same words
    }
    // Gram matrices: entry e = (register u, lane l) of the row kernel's accumulators is (l / 16 + 4 u, l % 16); thread t of the workgroup
    // takes (u = t / 64, l = t % 64) of every matrix, the ranks' blocks added in rank order (four loads in flight)
    {
        const int u = threadIdx.x >> 6, l = threadIdx.x & 63;
#pragma unroll
        for (int g = 0; g < XB_NG; ++g) {
            const double *src = gfin + g * 256 + u * 64 + l;
            double a = src[0];
            int r = 1;
            for (; r + 3 < nrg; r += 4) {
                const double x0 = src[(size_t)r * gstride], x1 = src[(size_t)(r + 1) * gstride], x2 = src[(size_t)(r + 2) * gstride], x3 = src[(size_t)(r + 3) * gstride];
                a += x0; a += x1; a += x2; a += x3;
            }
            for (; r < nrg; ++r) a += src[(size_t)r * gstride];
            Gm[g][(l >> 4) + 4 * u][l & 15] = a;
        }
    }
    __syncthreads();
    if (threadIdx.x >= 64) return;
    const bool init = it < 0;
    double rr_new;
    if (init) {
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            const int e = (int)threadIdx.x + 64 * u, i = e >> 4, j = e & 15;
            Cm[i][j] = 0.0; Bm[i][j] = 0.0;
            const double g = (i < s && j < s) ? 0.5 * (Gm[4][i][j] + Gm[4][j][i]) : 0.0;
            Grn[i][j] = g; Gg[i][j] = g;
        }
        XB_WSYNC();
        rr_new = Grn[0][0];
    } else {
        // P'T is symmetric by construction of A; symmetrise its rounding.  Tm keeps it, Lp becomes its Cholesky factor
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            const int e = (int)threadIdx.x + 64 * u, i = e >> 4, j = e & 15;
            const double g = (i < s && j < s) ? 0.5 * (Gm[0][i][j] + Gm[0][j][i]) : 0.0;
            Lp[i][j] = g; Tm[i][j] = g;
        }
        XB_WSYNC();
        if (!xtb_chol(Lp, s)) {                                               // no step can be taken: stop BEFORE this iteration's update (uniform)
            // (sharded: every rank holds the same Gram matrices -- the all-reduce hands all of them the same bits -- and takes this branch together)
            if (threadIdx.x == 0) { ctrl->pad[0] = 1; ctrl->done = it + 1; }
            return;
        }
        xtb_chol_solve(Cm, Lp, Gm[1], s);                                     // (P'T)^-1 P'R
#pragma unroll
        for (int u = 0; u < 4; ++u) { const int e = (int)threadIdx.x + 64 * u; Cm[e >> 4][e & 15] = -Cm[e >> 4][e & 15]; }     // c = -(...)
        XB_WSYNC();
        xtb_mm(Vm, Gm[3], Cm, false, 1.0, Gm[2], 1.0);                     // V = T'T c + T'R      (= T'R+)
        xtb_chol_solve(Bm, Lp, Vm, s);                                        // beta
        // R+'R+ = R'R + c'T'R + (c'T'R)' + c'(T'T c) = R'R + c'V + (T'R)'c
        xtb_mm(Grn, Cm, Vm, true, 1.0, Gm[4], 1.0);
        xtb_mm(Grn, Gm[2], Cm, true, 1.0, Grn, 1.0);
        xtb_symmetrise(Grn, s);
        rr_new = Grn[0][0];
        // Gram matrix of D = -R+ + P beta: R+'R+ - beta'(P'R+) - (P'R+)'beta + beta'(P'P)beta, P'R+ = P'R + P'T c.  P'P is MEASURED (it is
        // the identity only as far as the previous orthonormalisation was exact), so the recurrence holds for whatever P the loop carries
        xtb_mm(Gprn, Tm, Cm, false, 1.0, Gm[1], 1.0);
        xtb_symmetrise(Gm[5], s);
        xtb_mm(Gg, Gm[5], Bm, false, 1.0, nullptr, 0.0);                      // (P'P) beta
        xtb_mm(Gg, Bm, Gg, true, 1.0, Grn, 1.0);
        xtb_mm(Gg, Bm, Gprn, true, -1.0, Gg, 1.0);
        xtb_mm(Gg, Gprn, Bm, true, -1.0, Gg, 1.0);
        xtb_symmetrise(Gg, s);
    }
    const bool stop = init ? !(sqrt(rr_new) > tol2) : !(rr_new > tol2);
    // W = L^-T of the Gram matrix's Cholesky factor: W' G W = I.  Close to convergence G can lose definiteness in its rounding (its
    // columns become dependent): the directions are then only scaled to unit length this iteration (W diagonal) -- P'P is measured, so
    // nothing downstream assumes more.  Only a non-positive DIAGONAL ends the block loop (the update of Y of this iteration stands).
    bool diag_ok = true;
    for (int k = 0; k < s; ++k) if (!(Gg[k][k] > 0.0)) diag_ok = false;
    double gdiag = (threadIdx.x < 16 && (int)threadIdx.x < s && diag_ok) ? Gg[threadIdx.x][threadIdx.x] : 1.0;
    XB_WSYNC();
    const bool cholg = xtb_chol(Gg, s);
    const bool okg = diag_ok;
    if (!cholg) {                                                             // uniform: Gg <- diag(sqrt(g_ii)) stands in for the factor
#pragma unroll
        for (int u = 0; u < 4; ++u) { const int e = (int)threadIdx.x + 64 * u, i = e >> 4, j = e & 15; Gg[i][j] = (i == j) ? 1.0 : 0.0; }
        XB_WSYNC();
        if (threadIdx.x < 16) Gg[threadIdx.x][threadIdx.x] = sqrt(gdiag);
        XB_WSYNC();
    }
    // W = (L')^-1: column j of W solves L' w = e_j (upper triangular), by lane j
    if (threadIdx.x < 16) {
        const int jj = threadIdx.x;
        double w[16];
#pragma unroll
        for (int r = 15; r >= 0; --r) {
            double a = (r == jj) ? 1.0 : 0.0;
#pragma unroll
            for (int p = r + 1; p < 16; ++p) a -= Gg[p][r] * w[p];
            w[r] = a / Gg[r][r];
        }
#pragma unroll
        for (int r = 0; r < 16; ++r) Wm[r][jj] = (r < s && jj < s && okg) ? w[r] : 0.0;
    }
    XB_WSYNC();
    xtb_mm(Vm, Bm, Wm, false, 1.0, nullptr, 0.0);                          // M2 = beta W
    xtb_mm(Tm, Cm, Wm, false, -1.0, nullptr, 0.0);                         // M3 = c M1 = -c W
#pragma unroll
    for (int u = 0; u < 4; ++u) {
        const int e = (int)threadIdx.x + 64 * u, i = e >> 4, j = e & 15;
        mats[0 * 256 + e] = Cm[i][j]; mats[1 * 256 + e] = -Wm[i][j]; mats[2 * 256 + e] = Vm[i][j]; mats[3 * 256 + e] = Tm[i][j];
    }
    if (threadIdx.x == 0) {
        ctrl->rr[(it + 1) & 1] = rr_new; ctrl->rr[it & 1] = rr_new;
        ctrl->iters = it + 1;
        if (!okg) ctrl->pad[0] = 2;
        else if (!cholg) ctrl->pad[1] += 1;                                   // iterations that only rescaled their directions (statistics)
        // the step kernel of this iteration still runs (see k_xt_step).  Sharded solve: only the local flag is set; rank 0's travels in the next
        // exchange and k_xtb_rows turns it into `done` on every rank in the same iteration (one wasted product per solve)
        if (stop || !okg) { if (ctrl->sharded) ctrl->done_local = 1; else ctrl->done = it + 2; }
    }
}

// ---- panel updates: Y += P c ; R += T c ; P = R M1 + T M3 + P M2 ; Q = S P -------------------------------------------------------------
// 16 rows per wave and step: the three panels as A operands (row on i, vector on k), the 16 x 16 matrices as B operands, Y and R as
// accumulator input.  P is formed from the ORIGINAL R, T, P (M3 = c M1), so no result has to change its register map.
// rowlist (slab-distributed solve): the rows are the m entries of this rank's list (the two driver rows, replicated, + the rows it owns).
__global__ __launch_bounds__(XT_NT) void k_xtb_step(int m, int it, const double *__restrict__ mats, double *__restrict__ y0, double *__restrict__ R,
                                                    double *__restrict__ P, const double *__restrict__ T, const double *__restrict__ sc,
                                                    const int *__restrict__ nsrank, double *__restrict__ QS, const XCtrl *ctrl,
                                                    const int *__restrict__ rowlist = nullptr, double *__restrict__ Ypanel = nullptr)
{
    __shared__ int sdone;
    if (threadIdx.x == 0) { const int d = ctrl->done; sdone = d != 0 && it + 1 >= d; }
    __syncthreads();
    if (sdone) return;
    const int lane = threadIdx.x & 63, a = lane & 15, b = lane >> 4;
    const int wv = threadIdx.x >> 6;
    double cB[4], m1B[4], m2B[4], m3B[4], c0[4];
#pragma unroll
    for (int kk = 0; kk < 4; ++kk) {
        const int o = (4 * kk + b) * 16 + a;
        cB[kk] = mats[o]; m1B[kk] = mats[256 + o]; m2B[kk] = mats[512 + o]; m3B[kk] = mats[768 + o];
        c0[kk] = mats[(4 * kk + b) * 16];                                     // column 0 of c: the physical column of Y += P c
    }
    const int ngroups = (m + 15) / 16;
    for (int g = (int)blockIdx.x * 4 + wv; g < ngroups; g += (int)gridDim.x * 4) {
        const int row0 = 16 * g;
        double pa[4], ta[4], ra[4];
        const bool oka = row0 + a < m;
        const int rowa = oka ? (rowlist ? rowlist[row0 + a] : row0 + a) : 0;
        const size_t oa = (size_t)rowa * XB_SP + b;
#pragma unroll
        for (int kk = 0; kk < 4; ++kk) { pa[kk] = oka ? P[oa + 4 * kk] : 0.0; ta[kk] = oka ? T[oa + 4 * kk] : 0.0; ra[kk] = oka ? R[oa + 4 * kk] : 0.0; }
        dbl4 rN, pN = (dbl4)(0.0), yN = (dbl4)(0.0);
        const double yold = (b == 0 && oka) ? y0[rowa] : 0.0;
        int rowu[4];
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            const int li = row0 + b + 4 * u;
            rowu[u] = li < m ? (rowlist ? rowlist[li] : li) : -1;
            rN[u] = rowu[u] >= 0 ? R[(size_t)rowu[u] * XB_SP + a] : 0.0;
            if (Ypanel) yN[u] = rowu[u] >= 0 ? Ypanel[(size_t)rowu[u] * XB_SP + a] : 0.0;
        }
        // y0[row] += sum_i P[row][i] c[i][0]: lane (a, b) holds i = 4 kk + b; the four b-groups are added in a fixed order
        double yacc = (pa[0] * c0[0] + pa[1] * c0[1]) + (pa[2] * c0[2] + pa[3] * c0[3]);
        yacc += __shfl_xor(yacc, 16, WAVE); yacc += __shfl_xor(yacc, 32, WAVE);
        if (b == 0 && oka) y0[rowa] = yold + yacc;
#pragma unroll
        for (int kk = 0; kk < 4; ++kk) {
            rN = XB_MFMA(ta[kk], cB[kk], rN);
            pN = XB_MFMA(ra[kk], m1B[kk], pN); pN = XB_MFMA(ta[kk], m3B[kk], pN); pN = XB_MFMA(pa[kk], m2B[kk], pN);
            if (Ypanel) yN = XB_MFMA(pa[kk], cB[kk], yN);                  // Y += P c, all columns (the auxiliary solutions are kept for the next solve)
        }
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            const int row = rowu[u];
            if (row >= 0) {
                const size_t o = (size_t)row * XB_SP + a;
                R[o] = rN[u]; P[o] = pN[u];
                if (Ypanel) Ypanel[o] = yN[u];
                const int sr = nsrank[row];
                if (sr >= 0) QS[xtb_qs_pos(sr, a)] = sc[row] * pN[u];
            }
        }
    }
}
// ---- one-polynomial form (dkmc_set_x_poly_form): M^-1 = q(N) ~ (I - N)^-1 in the place of L^2, the loop in the variables Pt = L P, Rt = L^-1 R ------
// so that L is never applied: Q = A Pt (tiles + neighbour part + fold), U = q(N) Q, Z = M^-1 Rt and Pi = M Pt kept by recurrence.  The six Gram matrices
// of the split form are then  P'T = Pt'Q, P'R = Pt'Rt, T'R = Q'Z, T'T = Q'U, R'R = Rt'Z, P'P = Pt'Pi  -- k_xtb_gred and k_xtb_small take them as they are.
// Gram pass over [m][16] panels: four rows per matrix instruction with the ROW on the k index, a wave's rows of its workgroup's chunk in one chain, the
// four waves and then k_xtb_gred in a fixed order -- the grouping of the non-S rows of k_xtb_rows.  Q'U, Rt'Z and Pt'Pi are symmetric only to rounding:
// every workgroup stores (G + G') / 2 of its partial, so their sums are symmetric bit for bit.
__global__ __launch_bounds__(XT_NT) void k_xtb_gram1(int m, const double *__restrict__ Pt, const double *__restrict__ Pi, const double *__restrict__ Q,
                                                     const double *__restrict__ U, const double *__restrict__ Rt, const double *__restrict__ Z,
                                                     double *__restrict__ gpart, const XCtrl *ctrl)
{
    __shared__ double lg[4][XB_NG / 2][4][64];
    if (ctrl->done) return;                                                    // uniform over the launch
    const int v = threadIdx.x & 15, wv = threadIdx.x >> 6, lane = threadIdx.x & 63;
    dbl4 G[XB_NG];
#pragma unroll
    for (int g = 0; g < XB_NG; ++g) G[g] = (dbl4)(0.0);
    const int chunk = ((m + (int)gridDim.x - 1) / (int)gridDim.x + 3) & ~3;
    const long long i0l = (long long)blockIdx.x * chunk;
    const int i0 = (int)(i0l < m ? i0l : m), i1 = (int)(i0l + chunk < m ? i0l + chunk : m);
    for (int r0 = i0 + 4 * wv; r0 < i1; r0 += 64) {
        double pv[4], iv[4], qv[4], uv[4], rv[4], zv[4]; bool in[4];
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            const int row = r0 + 16 * u + (lane >> 4);
            in[u] = row < i1;
            const size_t o = (size_t)(in[u] ? row : i0) * XB_SP + v;               // (i0 < i1 <= m inside the loop)
            pv[u] = Pt[o]; iv[u] = Pi[o]; qv[u] = Q[o]; uv[u] = U[o]; rv[u] = Rt[o]; zv[u] = Z[o];
        }
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            if (r0 + 16 * u >= i1) break;                                     // uniform over the wave
            const double p_ = in[u] ? pv[u] : 0.0, i_ = in[u] ? iv[u] : 0.0, q_ = in[u] ? qv[u] : 0.0, u_ = in[u] ? uv[u] : 0.0, r_ = in[u] ? rv[u] : 0.0,
                         z_ = in[u] ? zv[u] : 0.0;
            G[0] = XB_MFMA(p_, q_, G[0]); G[1] = XB_MFMA(p_, r_, G[1]); G[2] = XB_MFMA(q_, z_, G[2]);
            G[3] = XB_MFMA(q_, u_, G[3]); G[4] = XB_MFMA(r_, z_, G[4]); G[5] = XB_MFMA(p_, i_, G[5]);
        }
    }
    // one partial per workgroup: the four waves added in a fixed order; entry (register u, lane l) is (i = l / 16 + 4 u, j = l % 16), that is 16 i + j
#pragma unroll
    for (int h = 0; h < 2; ++h) {
        __syncthreads();
#pragma unroll
        for (int g = 0; g < XB_NG / 2; ++g)
#pragma unroll
            for (int u = 0; u < 4; ++u) lg[wv][g][u][lane] = G[h * (XB_NG / 2) + g][u];
        __syncthreads();
        for (int e = threadIdx.x; e < (XB_NG / 2) * 256; e += XT_NT) {
            const int g = e >> 8, x = e & 255, u = x >> 6, l = x & 63;
            double a = (lg[0][g][u][l] + lg[1][g][u][l]) + (lg[2][g][u][l] + lg[3][g][u][l]);
            if (h == 1) {                                                     // matrices 3, 4, 5: the symmetric ones
                const int xt = ((x & 15) << 4) | (x >> 4), ut = xt >> 6, lt = xt & 63;
                a = 0.5 * (a + ((lg[0][g][ut][lt] + lg[1][g][ut][lt]) + (lg[2][g][ut][lt] + lg[3][g][ut][lt])));
            }
            gpart[(size_t)blockIdx.x * (XB_NG * 256) + h * (XB_NG / 2) * 256 + e] = a;
        }
    }
}
// Panel step: Y += Pt c (column 0) ; Rt += Q c ; Z += U c ; Pt = Z M1 + U M3 + Pt M2 ; Pi = Rt M1 + Q M3 + Pi M2 ; QS = S Pt -- the products of k_xtb_step
// (16 rows per wave and step, panels as A operands, the 16 x 16 matrices as B operands), everything from the ORIGINAL panels.
__global__ __launch_bounds__(XT_NT) void k_xtb_step1(int m, int it, const double *__restrict__ mats, double *__restrict__ y0, double *__restrict__ Rt,
                                                     double *__restrict__ Z, double *__restrict__ Pt, double *__restrict__ Pi, const double *__restrict__ Q,
                                                     const double *__restrict__ U, const double *__restrict__ sc, const int *__restrict__ nsrank,
                                                     double *__restrict__ QS, const XCtrl *ctrl, double *__restrict__ npart = nullptr)
{
    __shared__ int sdone;
    if (threadIdx.x == 0) { const int d = ctrl->done; sdone = d != 0 && it + 1 >= d; }
    __syncthreads();
    if (sdone) return;
    const int lane = threadIdx.x & 63, a = lane & 15, b = lane >> 4;
    const int wv = threadIdx.x >> 6;
    double cB[4], m1B[4], m2B[4], m3B[4], c0[4];
#pragma unroll
    for (int kk = 0; kk < 4; ++kk) {
        const int o = (4 * kk + b) * 16 + a;
        cB[kk] = mats[o]; m1B[kk] = mats[256 + o]; m2B[kk] = mats[512 + o]; m3B[kk] = mats[768 + o];
        c0[kk] = mats[(4 * kk + b) * 16];
    }
    double nacc = 0.0;                                                        // npart: sum of Rt+(i, 0)^2 over the rows this thread stores (the lanes of column 0)
    const int ngroups = (m + 15) / 16;
    for (int g = (int)blockIdx.x * 4 + wv; g < ngroups; g += (int)gridDim.x * 4) {
        const int row0 = 16 * g;
        double pa[4], ia[4], qa[4], ua[4], ra[4], za[4];
        const bool oka = row0 + a < m;
        const int rowa = oka ? row0 + a : 0;
        const size_t oa = (size_t)rowa * XB_SP + b;
#pragma unroll
        for (int kk = 0; kk < 4; ++kk) {
            pa[kk] = oka ? Pt[oa + 4 * kk] : 0.0; ia[kk] = oka ? Pi[oa + 4 * kk] : 0.0; qa[kk] = oka ? Q[oa + 4 * kk] : 0.0;
            ua[kk] = oka ? U[oa + 4 * kk] : 0.0; ra[kk] = oka ? Rt[oa + 4 * kk] : 0.0; za[kk] = oka ? Z[oa + 4 * kk] : 0.0;
        }
        dbl4 rN, zN, pN = (dbl4)(0.0), iN = (dbl4)(0.0);
        const double yold = (b == 0 && oka) ? y0[rowa] : 0.0;
        int rowu[4];
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            const int li = row0 + b + 4 * u;
            rowu[u] = li < m ? li : -1;
            rN[u] = rowu[u] >= 0 ? Rt[(size_t)rowu[u] * XB_SP + a] : 0.0;
            zN[u] = rowu[u] >= 0 ? Z[(size_t)rowu[u] * XB_SP + a] : 0.0;
        }
        double yacc = (pa[0] * c0[0] + pa[1] * c0[1]) + (pa[2] * c0[2] + pa[3] * c0[3]);
        yacc += __shfl_xor(yacc, 16, WAVE); yacc += __shfl_xor(yacc, 32, WAVE);
        if (b == 0 && oka) y0[rowa] = yold + yacc;
#pragma unroll
        for (int kk = 0; kk < 4; ++kk) {
            rN = XB_MFMA(qa[kk], cB[kk], rN); zN = XB_MFMA(ua[kk], cB[kk], zN);
            pN = XB_MFMA(za[kk], m1B[kk], pN); pN = XB_MFMA(ua[kk], m3B[kk], pN); pN = XB_MFMA(pa[kk], m2B[kk], pN);
            iN = XB_MFMA(ra[kk], m1B[kk], iN); iN = XB_MFMA(qa[kk], m3B[kk], iN); iN = XB_MFMA(ia[kk], m2B[kk], iN);
        }
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            const int row = rowu[u];
            if (row >= 0) {
                const size_t o = (size_t)row * XB_SP + a;
                Rt[o] = rN[u]; Z[o] = zN[u]; Pt[o] = pN[u]; Pi[o] = iN[u];
                const int sr = nsrank[row];
                if (sr >= 0) QS[xtb_qs_pos(sr, a)] = sc[row] * pN[u];
                if (a == 0) nacc += rN[u] * rN[u];
            }
        }
    }
    // ||Rt+(:, 0)||^2 of this workgroup's rows (dkmc_set_x_stop_form): per thread over its rows in the order it stored them, then the workgroup tree; no
    // atomics -- the partial sums depend on m and the grid alone.  k_xtb_stop_norm adds them.  (npart is a kernel argument: uniform over the launch)
    if (npart) {
        const double t = xtb_tree256(nacc);
        if (threadIdx.x == 0) npart[blockIdx.x] = t;
    }
}
// The contract's stop test itself (dkmc_set_x_stop_form(1)): ||Rt+(:, 0)||_2 <= kappa tol on the Jacobi-scaled system, from the partial sums k_xtb_step1 of
// sweep `it` wrote.  ONE workgroup adds them in index order (the pattern of k_xtb_pre_rr).  The bound test of k_xtb_small stays beside it: this kernel ends
// the loop after sweep `it` exactly as that test's stop branch of the same sweep would have (done = it + 2: the step of the sweep has run, nothing after it
// does; iters = it + 1; rr is what k_xtb_small of the sweep wrote), unless the stop word is set already.  rec: [0] the sum, [1] (Rt+'Z+)_00 of the
// sweep, [2] 1.0 where this test ended the loop -- of the last sweep whose step ran.
__global__ __launch_bounds__(256) void k_xtb_stop_norm(int np, int it, const double *__restrict__ part, double bound2, XCtrl *ctrl, double *__restrict__ rec)
{
    __shared__ int sdone;
    if (threadIdx.x == 0) { const int d = ctrl->done; sdone = d != 0 && it + 1 >= d; }
    __syncthreads();
    if (sdone) return;                                                        // the step of this sweep did not run: its partial sums are not this sweep's
    double a = 0.0;
    for (int i = threadIdx.x; i < np; i += 256) a += part[i];
    a = xtb_tree256(a);
    if (threadIdx.x == 0) {
        const bool fire = !(a > bound2) && ctrl->done == 0;
        rec[0] = a; rec[1] = ctrl->rr[(it + 1) & 1]; rec[2] = fire ? 1.0 : 0.0;
        if (fire) { ctrl->iters = it + 1; ctrl->done = it + 2; }
    }
}
// before the first product: P = Y0 stands in for Y0 (the product below is A Y0), QS = S Y0 over S; y0 = column 0.  Column 0 starts from y;
// the auxiliary columns from zero, or -- yaux != nullptr: columns hs ... s - 1, the hash set -- from the UNSCALED solutions the previous solve left
// (their right-hand sides are the same in every solve): their residuals then carry what the previous solve had not yet resolved, which is what
// the block Krylov space of this one should contain (tools/warm_aux_proto.py).  Ypanel (may be null): the scaled block iterate Y, all columns.
__global__ void k_xtb_init(int m, const double *__restrict__ y, const double *__restrict__ sc, const int *__restrict__ nsrank,
                           double *__restrict__ y0, double *__restrict__ P, double *__restrict__ QS,
                           const double *__restrict__ yaux = nullptr, int hs = 16, int s = 16, double *__restrict__ Ypanel = nullptr)
{
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= m * XB_SP) return;
    const int row = i >> 4, v = i & 15;
    double yv = 0.0;
    if (v == 0) yv = y[row];
    else if (yaux && v >= hs && v < s) yv = yaux[i] / sc[row];
    P[i] = yv;
    if (Ypanel) Ypanel[i] = yv;
    if (v == 0) y0[row] = yv;
    const int sr = nsrank[row];
    if (sr >= 0) QS[xtb_qs_pos(sr, v)] = sc[row] * yv;
}
// the auxiliary solutions a solve leaves for the next one: unscaled (x = S y)
__global__ void k_xtb_yaux_out(int n, const int *__restrict__ rowlist, const double *__restrict__ Ypanel, const double *__restrict__ sc, double *__restrict__ yaux)
{
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n * XB_SP) return;
    const int row = rowlist ? rowlist[i >> 4] : (i >> 4), v = i & 15;
    yaux[(size_t)row * XB_SP + v] = Ypanel[(size_t)row * XB_SP + v] * sc[row];
}
__global__ void k_xtb_zero(long long n, double *__restrict__ p)
{
    const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) p[i] = 0.0;
}

// Second stream of the block loop on large systems: the neighbour part (an L2 / Infinity-Cache gather, 0.3 ms per sweep at 9.4e5 sites) runs
// BESIDE the tile x panel kernel (one wave per SIMD on the matrix pipe) instead of behind it.  Events from a ring: the host runs a whole
// batch ahead.  On small systems the two cross-stream edges cost more than the overlap gains (xt.hip measured ~15 us per iteration).
static SideStream g_xb_side;

// test aid: make this rank fail once on the host side of block-CG iteration `iteration` of a sharded solve (dkmc_debug_inject_fault(3, it))
int g_xtb_fault_iter = -1;

// ---- host loop ------------------------------------------------------------------------------------------------------------------------
// Returns 0 with the scaled solution of column 0 in A.y; DKMC_XTB_BREAKDOWN (> 0, no error recorded) when an s x s system lost
// definiteness: A.y then holds the last good iterate and the caller continues with the single-vector loop from it.
// Auxiliary columns (dkmc_set_x_aux, dkmc_set_x_aux_warm).  Returns hs: columns 1 ... hs - 1 take the SMOOTH set (lowest Laplacian modes of the
// bounding box, always from a zero start: their systems converge before the physical one does, a warm start would leave them without a
// residual), columns hs ... s - 1 the HASH set -- started from the previous solve's solutions when the caller keeps them (warm).
//   mode 0: all hash.  1 / 3: all smooth.  2 (default): at tolerances of 1e-8 and looser the smooth set -- or, with the warm auxiliary start,
//   half smooth + half hash (measured on the oracle's X, tools/warm_aux_proto.py: 2.5 nm 33 -> 16-19 sweeps, against 40 with column 0 alone
//   warm-started); below 1e-8 all hash (smooth systems lose rank close to a converged tolerance).
static int xtb_aux_split(int mode, double tol2, bool warm, int s)
{
    if (mode == 0) return 1;
    if (mode == 1 || mode == 3) return 16;
    if (!(tol2 >= 1e-16)) return 1;
    return warm ? std::max(1, s / 2) : 16;
}
// bounding box of the atoms (k_xtb_box, from the empty box) and its modes (k_xtb_modes, which also decodes lo / hi) into d; h0: the other fields
static int xtb_box_modes(XbAux *d, XbAux h0, const XtbArgs &A, int x_only, hipStream_t st)
{
    for (int k = 0; k < 3; ++k) { h0.mm[2 * k] = ~0ull; h0.mm[2 * k + 1] = 0ull; }
    HIPCHK(hipMemcpyAsync(d, &h0, sizeof(XbAux), hipMemcpyHostToDevice, st));         // (pageable source: copied before the call returns)
    hipLaunchKernelGGL(k_xtb_box, dim3(std::min((A.m - 2 + 255) / 256, 256)), dim3(256), 0, st, A.m - 2, A.ax, A.ay, A.az, d);
    hipLaunchKernelGGL(k_xtb_modes, dim3(1), dim3(512), 0, st, d, x_only);
    return 0;
}
// smooth auxiliary columns (see xtb_rhs): dkmc_set_x_aux 0 never, 1 always, 2 (default) at tolerances of 1e-8 and looser, 3 always with x modes only.
// *hs: which auxiliary columns take which set, and which start from the previous solve's solutions (A.yaux, dkmc_set_x_aux_warm): see xtb_aux_split.
// *aux: the smooth set's table, or null
static int xtb_aux_setup(const XtbArgs &A, XbAux **aux, int *hs)
{
    Engine &e = eng();
    *hs = xtb_aux_split(e.x_aux, A.tol2, A.yaux != nullptr, A.s);
    *aux = nullptr;
    if (A.ax && A.ay && A.az && A.m > 2 && *hs > 1) {
        *aux = (XbAux *)scratch(S_XTB_XI, sizeof(XbAux));
        if (!*aux) return e.err_code;
        XbAux h0{};
        h0.hs = *hs;
        if (int rc = xtb_box_modes(*aux, h0, A, e.x_aux == 3 ? 1 : 0, e.stream)) return rc;
    }
    e.stats.xb_aux = *aux ? (*hs >= A.s ? 1 : 2) : 0;
    return 0;
}
// the tile x panel kernel (one wave per tile run, four runs per workgroup) at NG = so / 4 vector groups: the product form, or the round-4 form
// (dkmc_set_x_apply_form(1) = variant 8); variant != 0 (dkmc_xtb_time_apply in a DKMC_MEASURE_VARIANTS build): a measurement variant, where one exists
// tval32 != null: the launch streams the fp32 image of the tile values instead of tval (the product form only)
struct XbApplyArgs { int n; const XItem *items; const XTile *tiles; int sub_base; const double *tval; const double *QS; int nW; double *rowpartB, *colpartB; const XCtrl *ctrl; const float *tval32 = nullptr; };
template <int NTL, int NG, int V>
static void xtb_apply_v(const XbApplyArgs &a, hipStream_t st, hipEvent_t e0, hipEvent_t e1)
{
    hipExtLaunchKernelGGL((k_xtb_apply<NTL, NG, V>), dim3((a.n + 3) / 4), dim3(XT_NT), 0, st, e0, e1, 0, a.n, a.items, a.tiles, a.sub_base, a.tval, a.QS, a.nW,
                          a.rowpartB, a.colpartB, a.ctrl);
}
template <int NTL, int NG>
static void xtb_apply_f32(const XbApplyArgs &a, hipStream_t st, hipEvent_t e0, hipEvent_t e1)
{
    hipExtLaunchKernelGGL((k_xtb_apply<NTL, NG, 0, float>), dim3((a.n + 3) / 4), dim3(XT_NT), 0, st, e0, e1, 0, a.n, a.items, a.tiles, a.sub_base, a.tval32, a.QS, a.nW,
                          a.rowpartB, a.colpartB, a.ctrl);
}
template <int NTL, int NG>
static void xtb_apply_ng(const XbApplyArgs &a, int variant, hipStream_t st, hipEvent_t e0, hipEvent_t e1)
{
#ifdef DKMC_MEASURE_VARIANTS
#define XB_V(v_) if (variant == (v_)) return xtb_apply_v<NTL, NG, v_>(a, st, e0, e1);
    if constexpr (NTL == 1 && NG == 2) { XB_V(1) XB_V(2) }
    if constexpr (NTL == 1 && NG == 4) { XB_V(1) XB_V(2) XB_V(3) XB_V(4) XB_V(7) XB_V(10) XB_V(12) }
#undef XB_V
#else
    (void)variant;
#endif
    if (a.tval32) return xtb_apply_f32<NTL, NG>(a, st, e0, e1);
    if (eng().x_apply_form == 1) xtb_apply_v<NTL, NG, 8>(a, st, e0, e1);
    else xtb_apply_v<NTL, NG, 0>(a, st, e0, e1);
}
static void xtb_apply(const XbApplyArgs &a, bool ntl, int so, int variant, hipStream_t st, hipEvent_t e0 = nullptr, hipEvent_t e1 = nullptr)
{
    static void (*const ng[2][4])(const XbApplyArgs &, int, hipStream_t, hipEvent_t, hipEvent_t) = {
        {xtb_apply_ng<0, 1>, xtb_apply_ng<0, 2>, xtb_apply_ng<0, 3>, xtb_apply_ng<0, 4>}, {xtb_apply_ng<1, 1>, xtb_apply_ng<1, 2>, xtb_apply_ng<1, 3>, xtb_apply_ng<1, 4>}};
    ng[ntl ? 1 : 0][so == 4 ? 0 : (so == 8 ? 1 : (so == 12 ? 2 : 3))](a, variant, st, e0, e1);
}
// the row kernels' first pass (INIT) launched plainly, a sweep's between the profiling events e0 / e1 (null: none)
template <int SH, int NF, class... Args>
static void xtb_rows_launch(bool init, int ng, hipStream_t st, hipEvent_t e0, hipEvent_t e1, Args... a)
{
    if (init) hipLaunchKernelGGL((k_xtb_rows<1, SH, NF>), dim3(ng), dim3(XT_NT), 0, st, a...);
    else hipExtLaunchKernelGGL((k_xtb_rows<0, SH, NF>), dim3(ng), dim3(XT_NT), 0, st, e0, e1, 0, a...);
}
// A block loop runs on cg_poll_loop (cg_host.h) with the plan LaunchPlan::hinted_three_quarters of e.x_iter_hint (an emulation: of no hint) and the
// message below.  profiling (dkmc_set_profiling): the tile and the row kernel of the sampled sweeps run between the events of one slot of g_loop_events.
static const char *const XTB_NO_CONVERGENCE = "block-CG: no convergence after 200000 iterations";
// end of a block loop: sweeps and residual to the caller, the profile to the stats; hint: the sweeps size the next solve's first batch
static int xtb_finish(const XCtrl &h, bool hint, bool again, bool prof, int *iters_out, double *rr_out)
{
    Engine &e = eng();
    if (hint) e.x_iter_hint = h.iters;
    if (iters_out) *iters_out = h.iters;
    if (rr_out) *rr_out = h.rr[h.iters & 1];
    if (prof) g_loop_events.to_stats(e.stats, false);
    if (h.pad[0]) return DKMC_XTB_BREAKDOWN;
    return again ? DKMC_XTB_AGAIN : 0;
}
static int xtb_cg_body(const XtbArgs &A, int *iters_out, double *rr_out, bool *peer_used, const XbNPack *np, bool f32, XLive *lv, bool first_round);
static int xtb_cg_slab(const XtbArgs &A, int nr, int me0, const XShare *emu_shares, int time_rank, int *iters_out, double *rr_out);
// split polynomial preconditioner: the loop stops on the residual of L A L; when the TRUE residual of column 0 does not meet the stop test yet, the
// solve is re-entered from the iterate it reached (the check and the code DKMC_XTB_AGAIN: end of xtb_cg_body / xtb_cg_slab).  A round that no longer
// reduces the true residual by a factor of four has reached what the arithmetic gives (at tolerances of 1e-12 the recurrence residual the reference's
// test -- and the plain loop -- stop on goes below what the true one can reach): the solve ends there, as the plain loop's does.  rc, rr0: the first
// round's; body(&iters, &rr) runs one more round.
template <class Body>
static int xtb_reenter(int rc, double rr0, int *iters_out, double *rr_out, Body body)
{
    for (int round = 1; rc == DKMC_XTB_AGAIN && round < 6; ++round) {
        int it2 = 0; double rr1 = 0.0;
        rc = body(&it2, &rr1);
        if (iters_out) *iters_out += it2;
        if (rc == DKMC_XTB_AGAIN && !(rr1 < 0.25 * rr0)) rc = 0;
        rr0 = rr1;
    }
    if (rc == DKMC_XTB_AGAIN) rc = 0;
    if (rr_out) *rr_out = rr0;
    return rc;
}
int xtb_cg(const XtbArgs &A, int *iters_out, double *rr_out)
{
    bool peer_used = false;
    double rr0 = 0.0;
    // more than one rank: the state of the solve is distributed by row slabs (xtb_slab.inc; dkmc_set_x_slab(0) keeps the all-gather variant
    // below, which shards the tile stream only)
    if (A.sharded && eng().x_slab && comm_nranks() > 1 && comm_nranks() <= XS_MAXR && A.ay && A.az) {
        const int nr = comm_nranks(), me = comm_rank();
        const int rc = xtb_cg_slab(A, nr, me, nullptr, -1, iters_out, &rr0);
        return xtb_reenter(rc, rr0, iters_out, rr_out, [&](int *it, double *rr) { return xtb_cg_slab(A, nr, me, nullptr, -1, it, rr); });
    }
    // the preconditioner's N packed once per solve (sc is known); the re-entry rounds below reuse it
    XbNPack npk{};
    const bool packed = !A.sharded && A.m > 2 && A.ns > 0 && eng().x_poly > 0 && eng().x_nmul_form == 1;
    if (packed) { if (int rcp = xtb_npack(A, A.m, nullptr, scratch, 0, &npk)) return rcp; }
    const XbNPack *np = packed ? &npk : nullptr;
    // tile values of the sweeps (dkmc_set_x_tile_f32): the fp32 image inside the first round of the one-GPU preconditioned loop, at tolerances where
    // its perturbation (2^-24 |At|, 1e-10 of ||A||) stays far below the stop test; a round that follows a failed true-residual check runs on the fp64
    // store -- a failed check never loops on the perturbed operator
    Engine &e = eng();
    const bool f32 = e.x_tile_f32 != 0 && A.tval32 != nullptr && !A.sharded && A.m > 2 && A.ns > 0 && e.x_poly > 0 && A.tol2 >= 1e-16;
    if (f32) e.stats.x_tile_stream = 1; else if (e.stats.x_tile_stream == 1) e.stats.x_tile_stream = 0;      // (-1, no image, stays: the assembly set it)
    e.stats.x_tile_f64_rounds = f32 ? 0 : 1;
    // live tiles only (dkmc_set_x_tile_drop, xt_live.h): where the sweeps stream the image, and a live view of the resident X is worth having and fits,
    // they stream its compact image on its own launch view; everything else of the solve -- and every re-entry round -- keeps the full view
    // The threshold of this solve: the explicit one where it is set (cold starts included); else, in auto mode, the size rule's -- for a solve that
    // starts from the previous solution only (from a zero start the dropped part acts on the whole solution: an fp64 re-entry round, not a gain)
    XLive *lv = nullptr;
    const double theta = e.x_tile_drop > 0.0 ? e.x_tile_drop : (e.x_tile_drop_auto && A.warm ? xtl_drop_rule(A.stored_subblocks, e.x_tile_drop_gate) : 0.0);
    e.x_tile_drop_used = 0.0;
    if (f32 && theta > 0.0 && A.item_n > 0 && A.tiles == g_xb.tiles && A.tval32 == g_xb.tval32) {
        if (int rcl = xt_live_build(theta, e.x_tile_drop_unit, A.sS, &g_xlive)) return rcl;
        if (g_xlive.state == 1) { lv = &g_xlive; e.x_tile_drop_used = theta; }
    }
    int rc = xtb_cg_body(A, iters_out, &rr0, &peer_used, np, f32, lv, true);
    rc = xtb_reenter(rc, rr0, iters_out, rr_out, [&](int *it, double *rr) { ++e.stats.x_tile_f64_rounds; return xtb_cg_body(A, it, rr, &peer_used, np, false, nullptr, false); });
    // a sharded solve that failed with the peer-write exchange in use: the ranks' sequence counters may have drifted (comm.hip)
    if (rc != 0 && rc != DKMC_XTB_BREAKDOWN && peer_used) comm_peer_drop();
    return rc;
}
static int xtb_cg_body(const XtbArgs &A, int *iters_out, double *rr_out, bool *peer_used, const XbNPack *np, bool f32, XLive *lv, bool first_round)
{
    Engine &e = eng(); hipStream_t st = e.stream;
    const int m = A.m, s = A.s, so = 4 * ((s + 3) / 4);                       // vector groups of four: the matrix instruction's width
    const size_t pan = (size_t)m * XB_SP;
    const long long ncell = (long long)A.nK * A.nW;
    const int ng = std::max(128, std::min(A.nK, 4096));                                     // row-kernel workgroups = partial Gram matrices (one row block each up to 1.3e5 S rows)
    double *panels = (double *)scratch(S_XTB_PANELS, (pan * 3 + m + 16) * 8);
    double *QS = (double *)scratch(S_XTB_QS, (size_t)A.ns_pad * XB_SP * 8);
    double *rowpartB = (double *)scratch(S_XTB_ROWPART, (size_t)(ncell + 1) * XT_R * so * 8);
    const int nrec = std::max(A.nrecords, lv ? lv->nrecords : 0);             // records of column sums: the larger of the two views'
    double *colpartB = (double *)scratch(S_XTB_COLPART, (size_t)(nrec + 1) * XT_C * so * 8);
    double *gpart = (double *)scratch(S_XTB_GRAM, (size_t)ng * XB_NG * 256 * 8);
    double *small = (double *)scratch(S_XTB_SMALL, (size_t)(4 * 256 + 2 * XB_DSPLIT * XB_SP + XB_NG * 256) * 8);
    if (!panels || !QS || !rowpartB || !colpartB || !gpart || !small) return e.err_code;
    double *R = panels, *P = panels + pan, *T = panels + 2 * pan, *y0 = panels + 3 * pan;
    double *mats = small, *drvpart = small + 4 * 256, *gfin = drvpart + 2 * XB_DSPLIT * XB_SP;
    // split polynomial preconditioner (dkmc_set_x_poly; one GPU): see k_xtb_nmul.  Vp = L P, Zp = A Vp before the second L, W1 / W2 the Horner steps;
    // behind Vp: m zeros (the right-hand side of column 0 once the start vector has gone into it) and one double for the true residual
    const int pd = xtb_poly_degree(e, A);                                     // pinned (dkmc_set_x_poly) or from the rows of the system (xtb_poly_rule)
    e.stats.xb_poly_used = pd;
    // one-polynomial form (dkmc_set_x_poly_form; k_xtb_gram1): P, T, R are Pt, Q, Rt; Vp holds Pi, Zp holds Z, Up holds U = q(N) Q; pn products per sweep
    const bool one = pd > 0 && xtb_poly_one(e);
    const int pn = one ? xtb_poly1_degree(e, pd) : pd;
    e.x_poly_form_used = one ? 1 : 0; e.x_poly_products = one ? pn : 2 * pd;
    double *Vp = nullptr, *W1 = nullptr, *W2 = nullptr, *Zp = nullptr, *bz = nullptr, *Up = nullptr;
    if (pd > 0) {
        Vp = (double *)scratch(S_XTB_PRE_V, (pan + m + 16) * 8); W1 = (double *)scratch(S_XTB_PRE_W1, pan * 8); W2 = (double *)scratch(S_XTB_PRE_W2, pan * 8);
        Zp = (double *)scratch(S_XTB_PRE_Z, pan * 8);
        if (!Vp || !W1 || !W2 || !Zp) return e.err_code;
        bz = Vp + pan;
        HIPCHK(hipMemsetAsync(bz, 0, (size_t)(m + 16) * 8, st));
        if (one) {
            Up = (double *)scratch(S_XTB_PRE_U, pan * 8);
            if (!Up) return e.err_code;
            HIPCHK(hipMemsetAsync(Vp, 0, pan * 8, st));                       // Pi and U of the set-up pass: its Gram pass reads them, its step multiplies them by zero
            HIPCHK(hipMemsetAsync(Up, 0, pan * 8, st));
        }
    }
    double pc[XB_MAXPOLY1 + 1] = {1.0}, qmin = 1.0;
    if (one) xtb_poly1_coeffs(pn, pc, &qmin); else xtb_poly_coeffs(pd, pc);
    // split form: ||r|| <= 1.42 ||L r||, the loop stops a little early; one polynomial: the loop tests rt'q(N)rt >= min q ||rt||^2.  The true residual is checked at the end
    const double tol2_loop = one ? A.tol2 * qmin : (pd > 0 ? A.tol2 / 2.25 : A.tol2);
    // one polynomial, dkmc_set_x_stop_form(1): beside that bound, the quantity it bounds -- ||Rt+(:, 0)||^2 from k_xtb_step1's partial sums against (kappa tol)^2
    // (k_xtb_stop_norm); whichever fires first ends the loop.  First round only: a round that follows a failed true-residual check stops on the bound alone
    const bool nstop = one && first_round && (e.x_stop_form == 1 || (e.x_stop_form == 2 && xtb_stop_rule(m) != 0));
    double *npart = nstop ? (double *)scratch(S_XTB_STOPN, (size_t)(2048 + 4) * 8) : nullptr, *nstoprec = npart ? npart + 2048 : nullptr;
    if (nstop && !npart) return e.err_code;
    if (nstop) HIPCHK(hipMemsetAsync(nstoprec, 0, 4 * 8, st));
    const double nbound2 = e.x_stop_margin * e.x_stop_margin * A.tol2;
    e.x_stop_last = XStopLast{};
    HIPCHK(hipMemsetAsync(QS, 0, (size_t)A.ns_pad * XB_SP * 8, st));
    // fold of the tile launch's row partial sums (dkmc_set_x_fold_form): the one-GPU preconditioned loop adds only the cells of the launch view's tiles, by
    // the window lists of the assembly and of the live view (xtb_wlist_sum2; same bits as the range form).  Every launch writes the whole cell of each of its
    // tiles before the fold that follows it reads them, so nothing zeroes the array (GBs at 9.4e5 sites) or the dead tiles' cells, and a launch may pick
    // its own width: the two products of ONE column that frame the solve -- A Y0 and the true-residual pass; the other columns of their panel are zero,
    // keep_aux needs pd == 0 -- run at one vector group (so1 = 4), HBM-bound where the full width is matrix-pipe-bound on columns of zeros.  Column 0 comes
    // from the same instructions on the same operands; the other columns of T are sS (0 + 0) either way.  The plain, sharded and slab loops keep the range form
    const bool listf = e.x_fold_form == 1 && pd > 0 && !A.sharded && A.wlist != nullptr && (!lv || lv->wlist != nullptr);
    const int so1 = listf ? 4 : so;
    if (!listf) HIPCHK(hipMemsetAsync(rowpartB, 0, (size_t)(ncell + 1) * XT_R * so * 8, st));
    else if (e.x_fold_poison) HIPCHK(hipMemsetAsync(rowpartB, 0xff, (size_t)(ncell + 1) * XT_R * so * 8, st));       // test aid (dkmc_debug_poison_fold_cells): NaN in every cell
    HIPCHK(hipMemsetAsync(colpartB, 0, (size_t)(nrec + 1) * XT_C * so * 8, st));
    HIPCHK(hipMemsetAsync(A.ctrl, 0, sizeof(XCtrl), st));
    // sharded solve (comm.hip): this rank streams its share of the tiles; the tile sums of the S rows are completed by ONE all-gather of
    // ns x so doubles (+ two control words) per rank and sweep, added in rank order by every rank (k_xtb_rows): a sixteenth of the
    // exchanges of the single-vector loop, and bit-identical results on every rank by construction
    const bool sharded = A.sharded;
    const int nr = sharded ? comm_nranks() : 1, me = sharded ? comm_rank() : 0;
    double *xbuf = nullptr;
    const size_t xcount = (size_t)A.ns * so + 2;
    // exchange: the one-shot peer-write exchange when it is attached (comm.hip: push + signal + wait, no collective call), else one all-gather
    const bool peer = sharded && comm_peer_ready(xcount);
    *peer_used = peer;
    int xpar = 0;
    if (sharded) {
        if (!peer) { xbuf = (double *)scratch(S_CG_XCHG, xcount * nr * 8); if (!xbuf) return e.err_code; }
        hipLaunchKernelGGL(k_xtb_set_sharded, dim3(1), dim3(1), 0, st, A.ctrl);
    }
    const bool keep_aux = A.yaux != nullptr && pd == 0;
    double *Ypanel = keep_aux ? (double *)scratch(S_XTB_YPANEL, pan * 8) : nullptr;
    if (keep_aux && !Ypanel) return e.err_code;
    XbAux *aux = nullptr; int hs = 1;
    if (int rc = xtb_aux_setup(A, &aux, &hs)) return rc;
    int local_fail = 0;
    hipLaunchKernelGGL(k_xtb_init, dim3((unsigned)((pan + 255) / 256)), dim3(256), 0, st, m, (const double *)A.y, A.sc, A.nsrank, y0, P, QS,
                       (const double *)((keep_aux && A.yaux_valid) ? A.yaux : nullptr), hs, s, Ypanel);
    // launch view of the tile kernel and of the folds of its partial sums: the full one, or -- inside product_pre, with a live view -- the live one
    struct XbView { const XItem *items; int item_n; const XTile *tiles; const int2 *wrange; const int *nitem_w; const int *wlist; };
    const XbView full{A.items, A.item_n, A.tiles, A.wrange, A.nitem_w, listf ? A.wlist : nullptr};
    const XbView live = lv ? XbView{lv->items, lv->item_n, lv->tiles, lv->wrange, lv->nitem_w, listf ? lv->wlist : nullptr} : full;
    const XbView *vw = &full;
    const int ntb = (A.item_n + 3) / 4;
    const int nnb = 2 * XB_DSPLIT + (std::max(m - 2, 1) + 15) / 16;
    const int gs = grid_blocks((m + 15) / 16, 4, 2048);
    const bool prof = e.profiling != 0;
    if (prof) if (int prc = g_loop_events.begin(EventSampler::LONG | EventSampler::SHORT)) return prc;
    // neighbour part beside the tile kernel (see g_xb_side): only in a sharded solve, where a rank's tile pass is 1 / N of the sweep and the
    // (replicated) neighbour part would otherwise be a serial 0.3 ms behind it.  On ONE GPU the overlap was measured and does not pay: the two
    // kernels share the memory system, the tile pass slows by what the neighbour part takes (9.4e5 sites: 3.95 + 0 against 3.65 + 0.32 ms; 85 k sites,
    // where both are latency-bound: 15.0 against 13.5 ms per superstep -- the two event hand-overs per sweep cost more than the overlap gains).
    const bool side = sharded && m > 20000 && ntb > 0 && side_stream_init(g_xb_side) == 0;
    const float *t32 = nullptr;                                               // the tile launch of product() streams the fp32 image (product_pre) or the fp64 store
    auto product = [&](hipEvent_t e0, hipEvent_t e1, int sw) {                 // sw: vectors per row of the partial sums this launch writes (so, or so1)
        int sl = 0;
        if (side) {
            SideStream &S = g_xb_side; sl = (int)(S.seq++ % SideStream::RING);
            (void)hipEventRecord(S.a[sl], st);                                 // P of the previous step (and the stop word) are final
            (void)hipStreamWaitEvent(S.st, S.a[sl], 0);
            hipLaunchKernelGGL(k_xtb_neigh, dim3(nnb), dim3(XT_NT), 0, S.st, m, A.rp, A.ci, A.val, (const double *)P, A.sc, A.nsrank, (const XCtrl *)A.ctrl, T, drvpart);
            (void)hipEventRecord(S.b[sl], S.st);
        }
        if (vw->item_n > 0) xtb_apply({vw->item_n, vw->items, vw->tiles, A.sub_base, A.tval, QS, A.nW, rowpartB, colpartB, A.ctrl, t32}, A.nt_loads, sw, 0, st, e0, e1);
        if (side) (void)hipStreamWaitEvent(st, g_xb_side.b[sl], 0);           // the sparse sums are in T before the row kernel reads them
        else hipLaunchKernelGGL(k_xtb_neigh, dim3(nnb), dim3(XT_NT), 0, st, m, A.rp, A.ci, A.val, (const double *)P, A.sc, A.nsrank, (const XCtrl *)A.ctrl, T, drvpart);
    };
    // dst = L src (xtb_applyL)
    const XbNRank nk{m, nullptr, np, QS, A.ctrl};
    auto applyL = [&](double *src, double *dst, bool qs) {
        xtb_applyL(st, A, pn, pc, src, dst, W1, W2, qs, [](int, double *) { return 0; }, [&](bool, auto f) { f(nk, [](double *p) { return p; }); return 0; });
    };
    auto fold_rows = [&](double *Tt, int sw) {                                 // (the width of the launch it folds)
        hipLaunchKernelGGL(k_xtb_fold_rows, dim3(std::max(ng, 1)), dim3(XT_NT), 0, st, A.ns, A.nK, A.nW, sw, vw->wrange, vw->wlist, vw->nitem_w, (const double *)rowpartB, (const double *)colpartB,
                           A.srow, A.sS, A.sc, (const double *)drvpart, Tt, (const XCtrl *)A.ctrl);
    };
    // T = L A L P
    auto product_pre = [&](hipEvent_t e0, hipEvent_t e1) {
        applyL(P, Vp, true);
        double *Pk = P, *Tk = T; P = Vp; T = Zp;                              // (the product reads P and QS, writes T)
        t32 = f32 ? A.tval32 : nullptr;                                       // (the first product A y0 and the true-residual pass call product() themselves: fp64 store)
        if (lv) { vw = &live; t32 = lv->tval32; }                             // dkmc_set_x_tile_drop: the live view and its compact image instead
        product(e0, e1, so);
        t32 = nullptr;
        P = Pk; T = Tk;
        fold_rows(Zp, so);
        vw = &full;
        applyL(Zp, T, false);
    };
    // one polynomial: Q = A Pt (into T), U = q(N) Q
    auto product_one = [&](hipEvent_t e0, hipEvent_t e1) {
        t32 = f32 ? A.tval32 : nullptr;
        if (lv) { vw = &live; t32 = lv->tval32; }
        product(e0, e1, so);
        t32 = nullptr;
        fold_rows(T, so);
        vw = &full;
        applyL(T, Up, false);
    };
    auto gram_one = [&](hipEvent_t e2, hipEvent_t e3) {
        hipExtLaunchKernelGGL(k_xtb_gram1, dim3(ng), dim3(XT_NT), 0, st, e2, e3, 0, m, (const double *)P, (const double *)Vp, (const double *)T, (const double *)Up,
                              (const double *)R, (const double *)Zp, gpart, (const XCtrl *)A.ctrl);
    };
    auto step = [&](int it) {
        if (one) {
            const bool nt = nstop && it >= 0;                                  // (the set-up pass takes no step in Rt)
            hipLaunchKernelGGL(k_xtb_step1, dim3(gs), dim3(XT_NT), 0, st, m, it, (const double *)mats, y0, R, Zp, P, Vp, (const double *)T, (const double *)Up, A.sc,
                               A.nsrank, QS, (const XCtrl *)A.ctrl, nt ? npart : (double *)nullptr);
            if (nt) hipLaunchKernelGGL(k_xtb_stop_norm, dim3(1), dim3(256), 0, st, gs, it, (const double *)npart, nbound2, A.ctrl, nstoprec);
        }
        else hipLaunchKernelGGL(k_xtb_step, dim3(gs), dim3(XT_NT), 0, st, m, it, (const double *)mats, y0, R, P, (const double *)T, A.sc, A.nsrank, QS, (const XCtrl *)A.ctrl,
                                (const int *)nullptr, Ypanel);
    };
    const double *bsel = A.b;
#define XB_ROWS_ARGS(IT_) A.ns, A.nK, A.nW, m, s, so, (lv && !init ? live : full).wrange, (lv && !init ? live : full).nitem_w, (const double *)rowpartB, (const double *)colpartB, A.srow, A.sS, A.nsrank, A.sc, \
                     (const double *)drvpart, T, (const double *)P, R, bsel, gpart, A.ctrl, (const double *)xbuf, IT_, nr, (const XbAux *)aux, A.ax, A.ay, A.az
    // S rows of T + partial Gram matrices; a sharded solve exchanges the tile sums first.  A host-side failure of this rank between two
    // collectives must not leave the peers in the all-reduce: it still joins, with the abort word set, and every rank leaves together.
    auto rows = [&](bool init, int itn, hipEvent_t e2, hipEvent_t e3) -> int {
        if (sharded) {
            if (peer) { xbuf = comm_peer_slots(xpar); }
            hipLaunchKernelGGL(k_xtb_fold_local, dim3(std::max(A.nK, 1)), dim3(XT_NT), 0, st, A.ns, A.nK, A.nW, so, A.wrange, A.nitem_w, (const double *)rowpartB,
                               (const double *)colpartB, xbuf + me * xcount, (const XCtrl *)A.ctrl, 1, A.w_lo, A.w_hi);
            if (hipGetLastError() != hipSuccess || local_fail) {
                if (!local_fail) local_fail = dkmc_fail(92, "block-CG: launch failed between two collectives", __FILE__, __LINE__);
                hipLaunchKernelGGL(k_xtb_abort_word, dim3(1), dim3(1), 0, st, A.ctrl, xbuf + me * xcount, (size_t)A.ns * so + 1);
            }
            if (peer) {
                if (int rcx = comm_peer_exchange(xpar, xcount, &A.ctrl->done, &A.ctrl->aborted, &A.ctrl->xchg_timeout, itn + 2)) return rcx;
                xpar ^= 1;
            } else if (int rcx = comm_allgather_f64(xbuf, xcount)) return rcx;
            xtb_rows_launch<1, 0>(init, ng, st, e2, e3, XB_ROWS_ARGS(itn));
        } else if (pd > 0) xtb_rows_launch<0, 1>(init, ng, st, e2, e3, XB_ROWS_ARGS(itn));
        else xtb_rows_launch<0, 0>(init, ng, st, e2, e3, XB_ROWS_ARGS(itn));
        return 0;
    };
    // ---- R = A Y0 - B ; first directions ----
    product(nullptr, nullptr, so1);
    if (one) {
        // Rt = A Y0 - B in every column (column 0 from the start vector, the auxiliary columns from zero: their right-hand sides are those of A), Z = q(N) Rt
        fold_rows(T, so1);
        if (lv && !listf) xt_live_zero_dead(*lv, rowpartB, so);
        if (int rcx = rows(true, -1, nullptr, nullptr)) return rcx;
        applyL(R, Zp, false);
        gram_one(nullptr, nullptr);
    } else if (pd > 0) {
        // the start vector goes into the right-hand side: column 0 solves L A L dh = L (b - A y0) from zero, the auxiliary columns keep their own
        fold_rows(T, so1);                                                    // T = A Y0
        if (lv && !listf) xt_live_zero_dead(*lv, rowpartB, so);                        // the sweeps fold on the live view: the dead tiles' row sums of this launch must not be added
        hipLaunchKernelGGL(k_xtb_pre_resid, dim3((unsigned)((pan + 255) / 256)), dim3(256), 0, st, m, (const double *)T, A.b, Zp);
        applyL(Zp, T, false);                                                 // T(:, 0) = L (A y0 - b), the other columns 0
        bsel = bz;                                                            // R = T - [0 | auxiliary right-hand sides]
        HIPCHK(hipMemsetAsync(y0, 0, (size_t)m * 8, st));
    }
    if (!one) if (int rcx = rows(true, -1, nullptr, nullptr)) return rcx;
    hipLaunchKernelGGL(k_xtb_gred, dim3(XB_NG * 16), dim3(XT_NT), 0, st, ng, (const double *)gpart, gfin, (const XCtrl *)A.ctrl);
    hipLaunchKernelGGL(k_xtb_small, dim3(1), dim3(256), 0, st, -1, s, (const double *)gfin, mats, A.ctrl, tol2_loop);
    hipLaunchKernelGGL(k_xtb_zero, dim3((unsigned)((pan + 255) / 256)), dim3(256), 0, st, (long long)pan, P);          // Y0 has served: P_{-1} = 0
    step(-1);
    KCHK();
    XCtrl h{};
    if (int rcx = cg_poll_loop(A.ctrl, h, LaunchPlan::hinted_three_quarters(e.x_iter_hint), st, XTB_NO_CONVERGENCE, prof && ntb > 0 && live.item_n > 0 ? &g_loop_events : nullptr,     // (no tile launch: no events)
                               [&](int it, const hipEvent_t *ev) -> int {
            if (sharded && g_xtb_fault_iter >= 0 && it >= g_xtb_fault_iter) { g_xtb_fault_iter = -1; local_fail = dkmc_fail(91, "injected fault (block-CG iteration)", __FILE__, __LINE__); }
            if (one) { product_one(ev[0], ev[1]); gram_one(ev[2], ev[3]); }
            else {
                if (pd > 0) product_pre(ev[0], ev[1]);
                else product(ev[0], ev[1], so);
                if (int rcx = rows(false, it, ev[2], ev[3])) return rcx;
            }
            hipLaunchKernelGGL(k_xtb_gred, dim3(XB_NG * 16), dim3(XT_NT), 0, st, ng, (const double *)gpart, gfin, (const XCtrl *)A.ctrl);
            hipLaunchKernelGGL(k_xtb_small, dim3(1), dim3(256), 0, st, it, s, (const double *)gfin, mats, A.ctrl, tol2_loop);
            step(it);
            return 0;
        })) return rcx;
#undef XB_ROWS_ARGS
    if (lv) lv->info[7] = h.iters;
    if (local_fail) return local_fail;                                         // the peers were told (abort word)
    if (h.xchg_timeout) return dkmc_fail(48, "block-CG: the peer-write exchange timed out waiting for a peer's slot", __FILE__, __LINE__);
    if (h.aborted) return dkmc_fail(46, "a peer rank aborted the sharded current solve", __FILE__, __LINE__);
    if (e.err_code) return e.err_code;
    bool again = false;
    if (pd > 0) {
        // y = y0 + L dh, then the TRUE residual of column 0 in the unpreconditioned system: one more pass over the tiles
        HIPCHK(hipMemsetAsync(A.ctrl, 0, sizeof(XCtrl), st));                 // (the kernels below are gated by `done`)
        if (one) HIPCHK(hipMemcpyAsync(A.y, y0, (size_t)m * 8, hipMemcpyDeviceToDevice, st));      // Y += Pt c ran in the unpreconditioned space, from the start vector
        else {
            hipLaunchKernelGGL(k_xtb_pre_col0, dim3((unsigned)((pan + 255) / 256)), dim3(256), 0, st, m, (const double *)y0, Zp);
            applyL(Zp, Vp, false);
            hipLaunchKernelGGL(k_xtb_pre_add, dim3((m + 255) / 256), dim3(256), 0, st, m, (const double *)Vp, A.y);
        }
        if (!h.pad[0]) {
            hipLaunchKernelGGL(k_xtb_pre_col0, dim3((unsigned)((pan + 255) / 256)), dim3(256), 0, st, m, (const double *)A.y, P);
            hipLaunchKernelGGL(k_xtb_qs_from, dim3((unsigned)((pan + 255) / 256)), dim3(256), 0, st, m, (const double *)P, A.sc, A.nsrank, QS, (const XCtrl *)A.ctrl);
            product(nullptr, nullptr, so1);
            fold_rows(T, so1);
            const int nrp = std::min(XB_RR_MAXPART, (m + 1023) / 1024);       // (the partial Gram matrices have served: gpart holds the partial sums)
            hipLaunchKernelGGL(k_xtb_pre_rr_part, dim3(nrp), dim3(256), 0, st, m, (const double *)T, A.b, gpart);
            hipLaunchKernelGGL(k_xtb_pre_rr, dim3(1), dim3(256), 0, st, nrp, (const double *)gpart, bz + m);
            double rr_true = 0.0, hrec[3] = {-1.0, h.rr[h.iters & 1], 0.0};
            HIPCHK(hipMemcpyAsync(&rr_true, bz + m, 8, hipMemcpyDeviceToHost, st));
            if (nstop && h.iters > 0) HIPCHK(hipMemcpyAsync(hrec, nstoprec, 3 * 8, hipMemcpyDeviceToHost, st));
            HIPCHK(hipStreamSynchronize(st));
            // the stop of this round (dkmc_get_x_stop_info): which test ended it, ||Rt(:, 0)|| there (form 1), (Rt'Z)_00 there, the true residual
            if (one) e.x_stop_last = XStopLast{hrec[2] != 0.0 ? 2 : 1, nstop ? 1 : 0, m, hrec[0] >= 0.0 ? sqrt(hrec[0]) : -1.0, hrec[1], sqrt(rr_true)};
            h.rr[h.iters & 1] = rr_true;
            again = rr_true > A.tol2;
            if (e.x_tile_f32_fail_once) { e.x_tile_f32_fail_once = 0; again = true; }       // test aid (dkmc_debug_fail_true_residual_once)
        }
    } else
    HIPCHK(hipMemcpyAsync(A.y, y0, (size_t)m * 8, hipMemcpyDeviceToDevice, st));
    if (keep_aux) hipLaunchKernelGGL(k_xtb_yaux_out, dim3((unsigned)((pan + 255) / 256)), dim3(256), 0, st, m, (const int *)nullptr, (const double *)Ypanel, A.sc, A.yaux);
    return xtb_finish(h, true, again, prof, iters_out, rr_out);
}

#include "xtb_slab.inc"
// emulation entry (xt.hip: dkmc_xtb_emulate_slabs): nr virtual ranks in this process on the resident X of a single-GPU solve
int xtb_cg_slab_emulate(const XtbArgs &A, int nr, const XShare *shares, int time_rank, int sweep_cap, int *iters_out, double *rr_out, double *times_us, long long *xdoubles)
{
    g_slab_sweep_cap = sweep_cap;
    double rr0 = 0.0;
    int rc = xtb_cg_slab(A, nr, 0, shares, time_rank, iters_out, &rr0);
    // re-entry rounds as xtb_cg runs them (preconditioned loop); the kernel times are those of the first round; a measurement run (sweep cap) has none
    const double nmul_us = g_slab_last.nmul_us;
    if (sweep_cap > 0) { if (rc == DKMC_XTB_AGAIN) rc = 0; if (rr_out) *rr_out = rr0; }
    else rc = xtb_reenter(rc, rr0, iters_out, rr_out, [&](int *it, double *rr) { return xtb_cg_slab(A, nr, 0, shares, -1, it, rr); });
    g_slab_last.nmul_us = nmul_us;
    g_slab_sweep_cap = 0;
    if (times_us) for (int c = 0; c < 8; ++c) times_us[c] = g_slab_times.us[c];
    if (xdoubles) for (int c = 0; c < 3; ++c) xdoubles[c] = g_slab_xbytes[c];
    return rc;
}
// measurement aid (devicekmc_hip_debug.h): exchanges per sweep, halo doubles per exchange and mean N x panel product time of the last slab solve
extern "C" int dkmc_xtb_slab_last(int *exchanges_per_sweep, long long *halo_doubles_per_exchange, double *nmul_us)
{
    if (exchanges_per_sweep) *exchanges_per_sweep = g_slab_last.exchanges;
    if (halo_doubles_per_exchange) *halo_doubles_per_exchange = g_slab_last.halo_doubles;
    if (nmul_us) *nmul_us = g_slab_last.nmul_us;
    return 0;
}

// ---- test aid (tests/test_gpu_block_cg.py; no counterpart in the reference) ---------------------------------------------------------------
// On the X left resident by the last single-GPU solve: the tile x panel product of 16 test vectors (k_xtb_apply + the fold of k_xtb_rows)
// against 16 passes of the single-vector tile kernel (xt_tile_sums_mv).  Reports the largest deviation and the largest sum.
__global__ void k_xtb_test_panel(int ns, double *__restrict__ QS)
{
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= ns * XB_SP) return;
    const int r = i >> 4, v = i & 15;
    QS[xtb_qs_pos(r, v)] = 0.25 + (double)((((unsigned)r * 2654435761u) ^ ((unsigned)v * 40503u)) >> 20) / 4096.0 + 0.125 * v;
}
__global__ void k_xtb_test_column(int ns, int v, const double *__restrict__ QS, double *__restrict__ vS)
{
    const int r = blockIdx.x * blockDim.x + threadIdx.x;
    if (r < ns) vS[r] = QS[xtb_qs_pos(r, v)];
}
__global__ void k_xtb_test_compare(int ns, int v, const int *__restrict__ srow, const double *__restrict__ T, const double *__restrict__ ref, double *__restrict__ out)
{
    // out[0] = max |T - ref|, out[1] = max |ref| (atomicMax on the bits of non-negative doubles)
    const int r = blockIdx.x * blockDim.x + threadIdx.x;
    if (r >= ns) return;
    const double a = T[(size_t)srow[r] * XB_SP + v], b = ref[r];
    atomicMax(reinterpret_cast<unsigned long long *>(out), (unsigned long long)__double_as_longlong(fabs(a - b)));
    atomicMax(reinterpret_cast<unsigned long long *>(out + 1), (unsigned long long)__double_as_longlong(fabs(b)));
}
int xt_tile_sums_mv(const double *vS, double *out);
extern "C" int dkmc_xtb_check_product(int width, double *max_abs_diff, double *max_abs)
{
    Engine &e = eng(); hipStream_t st = e.stream; const XTState &X = g_xt;
    if (!X.valid || comm_attached() || X.tile_n != X.ntiles || X.ns <= 0) return dkmc_fail(13, "xtb_check_product: needs the X of a single-GPU solve", __FILE__, __LINE__);
    const int m = X.Nsub, ns = X.ns, s = std::max(2, std::min(width, 16)), so = 4 * ((s + 3) / 4);
    const size_t pan = (size_t)m * XB_SP;
    const long long ncell = (long long)X.nK * X.nW;
    const int nrec = X.nitems >> X.rec_shift, ng = 64;
    double *panels = (double *)scratch(S_XTB_PANELS, (pan * 3 + m + 16) * 8);
    double *QS = (double *)scratch(S_XTB_QS, (size_t)X.ns_pad * XB_SP * 8);
    double *rowpartB = (double *)scratch(S_XTB_ROWPART, (size_t)(ncell + 1) * XT_R * so * 8);
    double *colpartB = (double *)scratch(S_XTB_COLPART, (size_t)(nrec + 1) * XT_C * so * 8);
    double *gpart = (double *)scratch(S_XTB_GRAM, (size_t)4096 * XB_NG * 256 * 8);
    double *small = (double *)scratch(S_XTB_SMALL, (size_t)(4 * 256 + 2 * XB_DSPLIT * XB_SP + XB_NG * 256) * 8);
    double *tmp = (double *)scratch(S_XT_T_MISC, (size_t)4 * X.ns_pad * 8);
    XCtrl *ctrl = (XCtrl *)scratch(S_MISC2, 256);
    double *sS = (double *)e.buf[S_CG_PS], *sc = (double *)e.buf[S_CG_S], *rhs = (double *)e.buf[S_X_RHS];
    if (!panels || !QS || !rowpartB || !colpartB || !gpart || !small || !tmp || !ctrl || !sS || !sc || !rhs) return e.err_code ? e.err_code : dkmc_fail(13, "xtb_check_product: no solver state", __FILE__, __LINE__);
    sS += X.ns_pad;
    double *T = panels + 2 * pan, *R = panels, *P = panels + pan, *drvpart = small + 4 * 256;
    double *vS = tmp, *ref = tmp + X.ns_pad, *res = tmp + 2 * (size_t)X.ns_pad;
    HIPCHK(hipMemsetAsync(tmp, 0, (size_t)4 * X.ns_pad * 8, st));
    HIPCHK(hipMemsetAsync(QS, 0, (size_t)X.ns_pad * XB_SP * 8, st));
    HIPCHK(hipMemsetAsync(panels, 0, (pan * 3 + m + 16) * 8, st));
    HIPCHK(hipMemsetAsync(small, 0, (size_t)(4 * 256 + 2 * XB_DSPLIT * XB_SP) * 8, st));
    HIPCHK(hipMemsetAsync(rowpartB, 0, (size_t)(ncell + 1) * XT_R * so * 8, st));
    HIPCHK(hipMemsetAsync(colpartB, 0, (size_t)(nrec + 1) * XT_C * so * 8, st));
    HIPCHK(hipMemsetAsync(ctrl, 0, sizeof(XCtrl), st));
    hipLaunchKernelGGL(k_xtb_test_panel, dim3((ns * XB_SP + 255) / 256), dim3(256), 0, st, ns, QS);
    const XbApplyArgs xa{X.item_n, (const XItem *)g_xb.items + X.item_lo, (const XTile *)g_xb.tiles, (int)X.sub_base, (const double *)g_xb.tval, QS, X.nW, rowpartB,
                         colpartB, ctrl};
    if (xa.n > 0) xtb_apply(xa, true, so, 0, st);                          // (a tunnelling set without a pair stores no tile: nothing to launch, all sums 0)
    hipLaunchKernelGGL((k_xtb_rows<1, 0>), dim3(ng), dim3(XT_NT), 0, st, ns, X.nK, X.nW, m, s, so, (const int2 *)g_xb.wrange, (const int *)g_xb.nitem_w, (const double *)rowpartB,
                       (const double *)colpartB, (const int *)g_xb.srow, (const double *)sS, (const int *)g_xb.nsrank, (const double *)sc, (const double *)drvpart, T,
                       (const double *)P, R, (const double *)rhs, gpart, ctrl, (const double *)nullptr, -1, 1, (const XbAux *)nullptr, (const double *)nullptr, (const double *)nullptr, (const double *)nullptr);
    KCHK();
    const int gb = (ns + 255) / 256;
    for (int v = 0; v < so; ++v) {
        hipLaunchKernelGGL(k_xtb_test_column, dim3(gb), dim3(256), 0, st, ns, v, (const double *)QS, vS);
        int rc = xt_tile_sums_mv(vS, ref); if (rc) return rc;
        // T holds sS * (tile sums): compare with sS * ref
        hipLaunchKernelGGL(k_xt_vec_mul, dim3(gb), dim3(256), 0, st, ns, ref, (const double *)sS);
        hipLaunchKernelGGL(k_xtb_test_compare, dim3(gb), dim3(256), 0, st, ns, v, (const int *)g_xb.srow, (const double *)T, (const double *)ref, res);
    }
    double h[2] = {0, 0};
    HIPCHK(hipMemcpyAsync(h, res, 16, hipMemcpyDeviceToHost, st));
    HIPCHK(hipStreamSynchronize(st));
    if (max_abs_diff) *max_abs_diff = h[0];
    if (max_abs) *max_abs = h[1];
    return e.err_code;
}

// ---- test aids (tests/test_gpu_block_cg_algebra.py; devicekmc_hip_debug.h) -----------------------------------------------------------------
// The last four launches of a preconditioned sweep -- k_xtb_rows<0, 0, 1>, k_xtb_gred, k_xtb_small, k_xtb_step -- as production launches them, on
// data the caller supplies.  Buffers of their own (S_XTB_ALG_*) and an XCtrl of their own: the resident X, the solver's XCtrl, the warm start and the
// launch batch of the next solve are not touched.  Every argument is checked before anything is launched.
#define XTB_ALG_MAXROWS (1 << 21)
static_assert(sizeof(dkmc_xtb_ctrl) == sizeof(XCtrl) && offsetof(dkmc_xtb_ctrl, pad) == offsetof(XCtrl, pad) && offsetof(dkmc_xtb_ctrl, done) == offsetof(XCtrl, done),
              "dkmc_xtb_ctrl mirrors XCtrl");
static size_t xtb_alg_up(size_t bytes) { return (bytes + 255) & ~(size_t)255; }
// nsrank[m]: -1 or an S rank 0 ... ns - 1, each rank once; srow (may be null): the row of every rank
static bool xtb_alg_sranks(int m, const int *nsrank, int ns, std::vector<int> *srow)
{
    if (ns < 0 || ns > m) return false;
    std::vector<int> sr((size_t)ns, -1);
    for (int i = 0; i < m; ++i) {
        const int r = nsrank[i];
        if (r < -1 || r >= ns) return false;
        if (r >= 0) { if (sr[r] >= 0) return false; sr[r] = i; }
    }
    for (int r = 0; r < ns; ++r) if (sr[r] < 0) return false;
    if (srow) srow->swap(sr);
    return true;
}
// [ns][16] -> QS (interleaved, xtb_qs_pos); the inverse of k_xtb_test_qs_decode
__global__ void k_xtb_test_qs_encode(int ns, const double *__restrict__ in, double *__restrict__ QS)
{
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < ns * XB_SP) QS[xtb_qs_pos(i >> 4, i & 15)] = in[i];
}
// Gram stage: k_xtb_rows<0, 0, 1> over ng workgroups, then k_xtb_gred, on host panels P, T, R of [m][16].  gfin [6 * 256] is uploaded first and read back
// afterwards (a preset stop word leaves it as it came); the row kernel's partials start as NaN, so a partial nobody wrote shows.
extern "C" int dkmc_xtb_test_gram(int m, const double *P, const double *T, const double *R, const int *nsrank, int ns, int ng, int done_word, double *gfin,
                                  dkmc_xtb_ctrl *ctrl_out)
{
    Engine &e = eng(); hipStream_t st = e.stream;
    if (m < 1 || m > XTB_ALG_MAXROWS || !P || !T || !R || !nsrank || ng < 1 || ng > 4096 || !gfin) return dkmc_fail(13, "xtb_test_gram: bad arguments", __FILE__, __LINE__);
    std::vector<int> srow;
    if (!xtb_alg_sranks(m, nsrank, ns, &srow)) return dkmc_fail(13, "xtb_test_gram: bad S ranks", __FILE__, __LINE__);
    // the row blocks of the S rows; the NF form folds nothing but still reads wrange[k], nitem_w[k / 8], nitem_w[nW + 2 + k / 8] and nitem_w[2 (nW + 2)]: zeros
    const int nK = (ns + XT_R - 1) / XT_R, nW = std::max(1, (nK + XT_C / XT_R - 1) / (XT_C / XT_R));
    const size_t pan = (size_t)m * XB_SP * 8, pan_up = xtb_alg_up(pan);
    const size_t b_nsr = xtb_alg_up((size_t)m * 4), b_srow = xtb_alg_up((size_t)std::max(ns, 1) * 4), b_wr = xtb_alg_up((size_t)std::max(nK, 1) * sizeof(int2));
    const size_t b_nit = xtb_alg_up((size_t)(2 * (nW + 2) + 1) * 4);
    const size_t b_gpart = (size_t)ng * XB_NG * 256 * 8;
    char *panels = (char *)scratch(S_XTB_ALG_PANELS, 3 * pan_up);
    char *ints = (char *)scratch(S_XTB_ALG_INTS, b_nsr + b_srow + b_wr + b_nit);
    char *gram = (char *)scratch(S_XTB_ALG_GRAM, b_gpart + (size_t)XB_NG * 256 * 8);
    XCtrl *ctrl = (XCtrl *)scratch(S_XTB_ALG_CTRL, sizeof(XCtrl));
    if (!panels || !ints || !gram || !ctrl) return e.err_code;
    double *dP = (double *)panels, *dT = (double *)(panels + pan_up), *dR = (double *)(panels + 2 * pan_up);
    int *dnsr = (int *)ints, *dsrow = (int *)(ints + b_nsr);
    int2 *dwr = (int2 *)(ints + b_nsr + b_srow);
    int *dnit = (int *)(ints + b_nsr + b_srow + b_wr);
    double *gpart = (double *)gram, *dgfin = (double *)(gram + b_gpart);
    XCtrl h{}; h.done = done_word;
    HIPCHK(hipMemcpyAsync(dP, P, pan, hipMemcpyHostToDevice, st));
    HIPCHK(hipMemcpyAsync(dT, T, pan, hipMemcpyHostToDevice, st));
    HIPCHK(hipMemcpyAsync(dR, R, pan, hipMemcpyHostToDevice, st));
    HIPCHK(hipMemcpyAsync(dnsr, nsrank, (size_t)m * 4, hipMemcpyHostToDevice, st));
    if (ns > 0) HIPCHK(hipMemcpyAsync(dsrow, srow.data(), (size_t)ns * 4, hipMemcpyHostToDevice, st));
    HIPCHK(hipMemsetAsync(dwr, 0, b_wr + b_nit, st));
    HIPCHK(hipMemsetAsync(gpart, 0xff, b_gpart, st));
    HIPCHK(hipMemcpyAsync(dgfin, gfin, (size_t)XB_NG * 256 * 8, hipMemcpyHostToDevice, st));
    HIPCHK(hipMemcpyAsync(ctrl, &h, sizeof(XCtrl), hipMemcpyHostToDevice, st));
    HIPCHK(hipStreamSynchronize(st));                                          // (the uploads read pageable host memory, srow and h among it)
    xtb_rows_launch<0, 1>(false, ng, st, nullptr, nullptr, ns, nK, nW, m, 16, 16, (const int2 *)dwr, (const int *)dnit, (const double *)nullptr, (const double *)nullptr,
                          (const int *)dsrow, (const double *)nullptr, (const int *)dnsr, (const double *)nullptr, (const double *)nullptr, dT, (const double *)dP, dR,
                          (const double *)nullptr, gpart, ctrl, (const double *)nullptr, 0, 1, (const XbAux *)nullptr, (const double *)nullptr, (const double *)nullptr,
                          (const double *)nullptr);
    hipLaunchKernelGGL(k_xtb_gred, dim3(XB_NG * 16), dim3(XT_NT), 0, st, ng, (const double *)gpart, dgfin, (const XCtrl *)ctrl);
    KCHK();
    HIPCHK(hipMemcpyAsync(gfin, dgfin, (size_t)XB_NG * 256 * 8, hipMemcpyDeviceToHost, st));
    HIPCHK(hipMemcpyAsync(&h, ctrl, sizeof(XCtrl), hipMemcpyDeviceToHost, st));
    HIPCHK(hipStreamSynchronize(st));
    if (ctrl_out) memcpy(ctrl_out, &h, sizeof(XCtrl));
    return e.err_code;
}
// Small stage: ONE launch of k_xtb_small (256 threads) on caller-given Gram blocks [nrg][6 * 256 + 2] (a block's last word: that rank's abort word), the
// caller's XCtrl and the caller's pre-filled mats [4 * 256]; mats and the XCtrl come back.
extern "C" int dkmc_xtb_test_small(int it, int s, int nrg, const double *gblocks, double tol2, const dkmc_xtb_ctrl *ctrl_in, double *mats, dkmc_xtb_ctrl *ctrl_out)
{
    Engine &e = eng(); hipStream_t st = e.stream;
    if (it < -1 || it > 0x3fffffff || s < 1 || s > XB_SP || nrg < 1 || nrg > 64 || !gblocks || !ctrl_in || !mats || !ctrl_out)
        return dkmc_fail(13, "xtb_test_small: bad arguments", __FILE__, __LINE__);
    const size_t gstr = (size_t)XB_NG * 256 + 2, b_g = xtb_alg_up((size_t)nrg * gstr * 8);
    char *gram = (char *)scratch(S_XTB_ALG_GRAM, b_g + 4 * 256 * 8);
    XCtrl *ctrl = (XCtrl *)scratch(S_XTB_ALG_CTRL, sizeof(XCtrl));
    if (!gram || !ctrl) return e.err_code;
    double *dg = (double *)gram, *dmats = (double *)(gram + b_g);
    HIPCHK(hipMemcpyAsync(dg, gblocks, (size_t)nrg * gstr * 8, hipMemcpyHostToDevice, st));
    HIPCHK(hipMemcpyAsync(dmats, mats, 4 * 256 * 8, hipMemcpyHostToDevice, st));
    HIPCHK(hipMemcpyAsync(ctrl, ctrl_in, sizeof(XCtrl), hipMemcpyHostToDevice, st));
    hipLaunchKernelGGL(k_xtb_small, dim3(1), dim3(256), 0, st, it, s, (const double *)dg, dmats, ctrl, tol2, nrg, (int)gstr);
    KCHK();
    HIPCHK(hipMemcpyAsync(mats, dmats, 4 * 256 * 8, hipMemcpyDeviceToHost, st));
    HIPCHK(hipMemcpyAsync(ctrl_out, ctrl, sizeof(XCtrl), hipMemcpyDeviceToHost, st));
    HIPCHK(hipStreamSynchronize(st));
    return e.err_code;
}
// Step stage: ONE launch of k_xtb_step with the grid of a solve.  Panels of [m][16] and y0 [m] go up, and come back afterwards; rowlist (nlist distinct
// rows, may be null): the row-list form of the slab-distributed loop; Ypanel may be null.  qs [ns][16] in natural order goes up as the pre-fill of QS and
// comes back decoded (null only with ns = 0).
extern "C" int dkmc_xtb_test_step(int m, int it, const double *mats, int done_word, double *y0, double *R, double *P, const double *T, const double *sc,
                                  const int *nsrank, int ns, const int *rowlist, int nlist, double *Ypanel, double *qs)
{
    Engine &e = eng(); hipStream_t st = e.stream;
    if (m < 1 || m > XTB_ALG_MAXROWS || it < -1 || it > 0x3fffffff || !mats || !y0 || !R || !P || !T || !sc || !nsrank || (ns > 0 && !qs))
        return dkmc_fail(13, "xtb_test_step: bad arguments", __FILE__, __LINE__);
    if (!xtb_alg_sranks(m, nsrank, ns, nullptr)) return dkmc_fail(13, "xtb_test_step: bad S ranks", __FILE__, __LINE__);
    if (rowlist) {
        if (nlist < 1 || nlist > m) return dkmc_fail(13, "xtb_test_step: bad row list", __FILE__, __LINE__);
        std::vector<char> seen((size_t)m, 0);
        for (int i = 0; i < nlist; ++i) {
            if (rowlist[i] < 0 || rowlist[i] >= m || seen[rowlist[i]]) return dkmc_fail(13, "xtb_test_step: bad row list", __FILE__, __LINE__);
            seen[rowlist[i]] = 1;
        }
    }
    const int n = rowlist ? nlist : m;
    const size_t pan = (size_t)m * XB_SP * 8, pan_up = xtb_alg_up(pan), vec_up = xtb_alg_up((size_t)m * 8);
    const size_t b_nsr = xtb_alg_up((size_t)m * 4), b_list = xtb_alg_up((size_t)n * 4);
    const size_t b_qs = xtb_alg_up((size_t)(ns + 2) * XB_SP * 8);
    char *panels = (char *)scratch(S_XTB_ALG_PANELS, 4 * pan_up + 2 * vec_up);
    char *ints = (char *)scratch(S_XTB_ALG_INTS, b_nsr + b_list);
    char *gram = (char *)scratch(S_XTB_ALG_GRAM, 4 * 256 * 8);
    char *qsb = (char *)scratch(S_XTB_ALG_QS, 2 * b_qs);
    XCtrl *ctrl = (XCtrl *)scratch(S_XTB_ALG_CTRL, sizeof(XCtrl));
    if (!panels || !ints || !gram || !qsb || !ctrl) return e.err_code;
    double *dR = (double *)panels, *dP = (double *)(panels + pan_up), *dT = (double *)(panels + 2 * pan_up), *dY = (double *)(panels + 3 * pan_up);
    double *dy0 = (double *)(panels + 4 * pan_up), *dsc = (double *)(panels + 4 * pan_up + vec_up);
    int *dnsr = (int *)ints, *dlist = rowlist ? (int *)(ints + b_nsr) : nullptr;
    double *dmats = (double *)gram, *QS = (double *)qsb, *dq = (double *)(qsb + b_qs);
    XCtrl h{}; h.done = done_word;
    HIPCHK(hipMemcpyAsync(dR, R, pan, hipMemcpyHostToDevice, st));
    HIPCHK(hipMemcpyAsync(dP, P, pan, hipMemcpyHostToDevice, st));
    HIPCHK(hipMemcpyAsync(dT, T, pan, hipMemcpyHostToDevice, st));
    if (Ypanel) HIPCHK(hipMemcpyAsync(dY, Ypanel, pan, hipMemcpyHostToDevice, st));
    HIPCHK(hipMemcpyAsync(dy0, y0, (size_t)m * 8, hipMemcpyHostToDevice, st));
    HIPCHK(hipMemcpyAsync(dsc, sc, (size_t)m * 8, hipMemcpyHostToDevice, st));
    HIPCHK(hipMemcpyAsync(dnsr, nsrank, (size_t)m * 4, hipMemcpyHostToDevice, st));
    if (dlist) HIPCHK(hipMemcpyAsync(dlist, rowlist, (size_t)n * 4, hipMemcpyHostToDevice, st));
    HIPCHK(hipMemcpyAsync(dmats, mats, 4 * 256 * 8, hipMemcpyHostToDevice, st));
    HIPCHK(hipMemsetAsync(QS, 0, b_qs, st));
    if (ns > 0) {
        HIPCHK(hipMemcpyAsync(dq, qs, (size_t)ns * XB_SP * 8, hipMemcpyHostToDevice, st));
        hipLaunchKernelGGL(k_xtb_test_qs_encode, dim3((unsigned)(((size_t)ns * XB_SP + 255) / 256)), dim3(256), 0, st, ns, (const double *)dq, QS);
    }
    HIPCHK(hipMemcpyAsync(ctrl, &h, sizeof(XCtrl), hipMemcpyHostToDevice, st));
    HIPCHK(hipStreamSynchronize(st));                                          // (h is read by the upload)
    hipLaunchKernelGGL(k_xtb_step, dim3(grid_blocks((n + 15) / 16, 4, 2048)), dim3(XT_NT), 0, st, n, it, (const double *)dmats, dy0, dR, dP, (const double *)dT,
                       (const double *)dsc, (const int *)dnsr, QS, (const XCtrl *)ctrl, (const int *)dlist, Ypanel ? dY : (double *)nullptr);
    if (ns > 0) hipLaunchKernelGGL(k_xtb_test_qs_decode, dim3((unsigned)(((size_t)ns * XB_SP + 255) / 256)), dim3(256), 0, st, ns, (const double *)QS, dq);
    KCHK();
    HIPCHK(hipMemcpyAsync(R, dR, pan, hipMemcpyDeviceToHost, st));
    HIPCHK(hipMemcpyAsync(P, dP, pan, hipMemcpyDeviceToHost, st));
    if (Ypanel) HIPCHK(hipMemcpyAsync(Ypanel, dY, pan, hipMemcpyDeviceToHost, st));
    HIPCHK(hipMemcpyAsync(y0, dy0, (size_t)m * 8, hipMemcpyDeviceToHost, st));
    if (ns > 0) HIPCHK(hipMemcpyAsync(qs, dq, (size_t)ns * XB_SP * 8, hipMemcpyDeviceToHost, st));
    HIPCHK(hipStreamSynchronize(st));
    return e.err_code;
}

// The same two stages of the one-polynomial form (tests/test_gpu_x_poly_form_kernels.py).  panels: six host panels of [m][16] in the order Pt, Pi, Q, U, Rt, Z.
// Gram stage: k_xtb_gram1 over ng workgroups, then k_xtb_gred; gfin as in dkmc_xtb_test_gram.
extern "C" int dkmc_xtb_test_gram1(int m, const double *const *panels, int ng, int done_word, double *gfin)
{
    Engine &e = eng(); hipStream_t st = e.stream;
    if (m < 1 || m > XTB_ALG_MAXROWS || !panels || ng < 1 || ng > 4096 || !gfin) return dkmc_fail(13, "xtb_test_gram1: bad arguments", __FILE__, __LINE__);
    for (int k = 0; k < 6; ++k) if (!panels[k]) return dkmc_fail(13, "xtb_test_gram1: bad arguments", __FILE__, __LINE__);
    const size_t pan = (size_t)m * XB_SP * 8, pan_up = xtb_alg_up(pan), b_gpart = (size_t)ng * XB_NG * 256 * 8;
    char *dp = (char *)scratch(S_XTB_ALG_PANELS, 6 * pan_up);
    char *gram = (char *)scratch(S_XTB_ALG_GRAM, b_gpart + (size_t)XB_NG * 256 * 8);
    XCtrl *ctrl = (XCtrl *)scratch(S_XTB_ALG_CTRL, sizeof(XCtrl));
    if (!dp || !gram || !ctrl) return e.err_code;
    double *gpart = (double *)gram, *dgfin = (double *)(gram + b_gpart);
    XCtrl h{}; h.done = done_word;
    for (int k = 0; k < 6; ++k) HIPCHK(hipMemcpyAsync(dp + k * pan_up, panels[k], pan, hipMemcpyHostToDevice, st));
    HIPCHK(hipMemsetAsync(gpart, 0xff, b_gpart, st));
    HIPCHK(hipMemcpyAsync(dgfin, gfin, (size_t)XB_NG * 256 * 8, hipMemcpyHostToDevice, st));
    HIPCHK(hipMemcpyAsync(ctrl, &h, sizeof(XCtrl), hipMemcpyHostToDevice, st));
    HIPCHK(hipStreamSynchronize(st));
#define XB_DP(k_) (const double *)(dp + (k_) * pan_up)
    hipLaunchKernelGGL(k_xtb_gram1, dim3(ng), dim3(XT_NT), 0, st, m, XB_DP(0), XB_DP(1), XB_DP(2), XB_DP(3), XB_DP(4), XB_DP(5), gpart, (const XCtrl *)ctrl);
#undef XB_DP
    hipLaunchKernelGGL(k_xtb_gred, dim3(XB_NG * 16), dim3(XT_NT), 0, st, ng, (const double *)gpart, dgfin, (const XCtrl *)ctrl);
    KCHK();
    HIPCHK(hipMemcpyAsync(gfin, dgfin, (size_t)XB_NG * 256 * 8, hipMemcpyDeviceToHost, st));
    HIPCHK(hipStreamSynchronize(st));
    return e.err_code;
}
// Step stage: ONE launch of k_xtb_step1 with the grid of a solve.  Pt, Pi, Rt, Z and y0 [m] go up and come back, Q and U go up; qs [ns][16] as in
// dkmc_xtb_test_step.  rec3 (dkmc_xtb_test_step1_norm): the kernel also writes its partial sums of Rt+(:, 0)^2 and k_xtb_stop_norm follows it, as in a solve
// under dkmc_set_x_stop_form(1), with the bound bound2 and the XCtrl the aid starts from (done_word; rr = rr_in); rec3 and ctrl_out receive its record and the XCtrl.
static int xtb_test_step1_run(int m, int it, const double *mats, int done_word, double *y0, double *const *panels, const double *sc, const int *nsrank, int ns,
                              double *qs, double bound2, double rr_in, double *rec3, dkmc_xtb_ctrl *ctrl_out)
{
    Engine &e = eng(); hipStream_t st = e.stream;
    if (m < 1 || m > XTB_ALG_MAXROWS || it < -1 || it > 0x3fffffff || !mats || !y0 || !panels || !sc || !nsrank || (ns > 0 && !qs))
        return dkmc_fail(13, "xtb_test_step1: bad arguments", __FILE__, __LINE__);
    for (int k = 0; k < 6; ++k) if (!panels[k]) return dkmc_fail(13, "xtb_test_step1: bad arguments", __FILE__, __LINE__);
    if (!xtb_alg_sranks(m, nsrank, ns, nullptr)) return dkmc_fail(13, "xtb_test_step1: bad S ranks", __FILE__, __LINE__);
    const size_t pan = (size_t)m * XB_SP * 8, pan_up = xtb_alg_up(pan), vec_up = xtb_alg_up((size_t)m * 8);
    const size_t b_qs = xtb_alg_up((size_t)(ns + 2) * XB_SP * 8);
    char *dp = (char *)scratch(S_XTB_ALG_PANELS, 6 * pan_up + 2 * vec_up);
    int *dnsr = (int *)scratch(S_XTB_ALG_INTS, xtb_alg_up((size_t)m * 4));
    double *dmats = (double *)scratch(S_XTB_ALG_GRAM, (4 * 256 + 2048 + 4) * 8);
    char *qsb = (char *)scratch(S_XTB_ALG_QS, 2 * b_qs);
    XCtrl *ctrl = (XCtrl *)scratch(S_XTB_ALG_CTRL, sizeof(XCtrl));
    if (!dp || !dnsr || !dmats || !qsb || !ctrl) return e.err_code;
    double *dy0 = (double *)(dp + 6 * pan_up), *dsc = (double *)(dp + 6 * pan_up + vec_up);
    double *QS = (double *)qsb, *dq = (double *)(qsb + b_qs);
    double *dnpart = rec3 ? dmats + 4 * 256 : nullptr, *dnrec = dmats + 4 * 256 + 2048;
    const int gs1 = grid_blocks((m + 15) / 16, 4, 2048);
    XCtrl h{}; h.done = done_word; h.rr[0] = h.rr[1] = rr_in;
    if (rec3) { HIPCHK(hipMemsetAsync(dnpart, 0xff, 2048 * 8, st)); HIPCHK(hipMemcpyAsync(dnrec, rec3, 3 * 8, hipMemcpyHostToDevice, st)); }      // (NaN in every partial sum: the kernel must write all it launches)
    for (int k = 0; k < 6; ++k) HIPCHK(hipMemcpyAsync(dp + k * pan_up, panels[k], pan, hipMemcpyHostToDevice, st));
    HIPCHK(hipMemcpyAsync(dy0, y0, (size_t)m * 8, hipMemcpyHostToDevice, st));
    HIPCHK(hipMemcpyAsync(dsc, sc, (size_t)m * 8, hipMemcpyHostToDevice, st));
    HIPCHK(hipMemcpyAsync(dnsr, nsrank, (size_t)m * 4, hipMemcpyHostToDevice, st));
    HIPCHK(hipMemcpyAsync(dmats, mats, 4 * 256 * 8, hipMemcpyHostToDevice, st));
    HIPCHK(hipMemsetAsync(QS, 0, b_qs, st));
    if (ns > 0) {
        HIPCHK(hipMemcpyAsync(dq, qs, (size_t)ns * XB_SP * 8, hipMemcpyHostToDevice, st));
        hipLaunchKernelGGL(k_xtb_test_qs_encode, dim3((unsigned)(((size_t)ns * XB_SP + 255) / 256)), dim3(256), 0, st, ns, (const double *)dq, QS);
    }
    HIPCHK(hipMemcpyAsync(ctrl, &h, sizeof(XCtrl), hipMemcpyHostToDevice, st));
    HIPCHK(hipStreamSynchronize(st));
#define XB_DP(k_) (double *)(dp + (k_) * pan_up)
    hipLaunchKernelGGL(k_xtb_step1, dim3(gs1), dim3(XT_NT), 0, st, m, it, (const double *)dmats, dy0, XB_DP(4), XB_DP(5), XB_DP(0), XB_DP(1),
                       (const double *)XB_DP(2), (const double *)XB_DP(3), (const double *)dsc, (const int *)dnsr, QS, (const XCtrl *)ctrl, dnpart);
#undef XB_DP
    if (rec3) hipLaunchKernelGGL(k_xtb_stop_norm, dim3(1), dim3(256), 0, st, gs1, it, (const double *)dnpart, bound2, ctrl, dnrec);
    if (ns > 0) hipLaunchKernelGGL(k_xtb_test_qs_decode, dim3((unsigned)(((size_t)ns * XB_SP + 255) / 256)), dim3(256), 0, st, ns, (const double *)QS, dq);
    KCHK();
    for (int k = 0; k < 6; ++k) if (k != 2 && k != 3) HIPCHK(hipMemcpyAsync(panels[k], dp + k * pan_up, pan, hipMemcpyDeviceToHost, st));
    HIPCHK(hipMemcpyAsync(y0, dy0, (size_t)m * 8, hipMemcpyDeviceToHost, st));
    if (ns > 0) HIPCHK(hipMemcpyAsync(qs, dq, (size_t)ns * XB_SP * 8, hipMemcpyDeviceToHost, st));
    if (rec3) HIPCHK(hipMemcpyAsync(rec3, dnrec, 3 * 8, hipMemcpyDeviceToHost, st));
    if (ctrl_out) HIPCHK(hipMemcpyAsync(ctrl_out, ctrl, sizeof(XCtrl), hipMemcpyDeviceToHost, st));
    HIPCHK(hipStreamSynchronize(st));
    return e.err_code;
}
extern "C" int dkmc_xtb_test_step1(int m, int it, const double *mats, int done_word, double *y0, double *const *panels, const double *sc, const int *nsrank, int ns,
                                   double *qs)
{
    return xtb_test_step1_run(m, it, mats, done_word, y0, panels, sc, nsrank, ns, qs, 0.0, 0.0, nullptr, nullptr);
}
// The step stage under dkmc_set_x_stop_form(1) (tests/test_gpu_x_stop_norm.py): k_xtb_step1 with its partial sums, then k_xtb_stop_norm against bound2.
// rec3 is read (the pre-fill) and written: the sum of Rt+(i, 0)^2, rr_in as the kernel found it in the XCtrl, 1.0 where the test set the stop word.
extern "C" int dkmc_xtb_test_step1_norm(int m, int it, const double *mats, int done_word, double *y0, double *const *panels, const double *sc, const int *nsrank,
                                        int ns, double *qs, double bound2, double rr_in, double *rec3, dkmc_xtb_ctrl *ctrl_out)
{
    if (!rec3 || !ctrl_out || it < 0) return dkmc_fail(13, "xtb_test_step1_norm: bad arguments", __FILE__, __LINE__);
    return xtb_test_step1_run(m, it, mats, done_word, y0, panels, sc, nsrank, ns, qs, bound2, rr_in, rec3, ctrl_out);
}
// Test aid: column 0 of Rt as the last round of the last one-polynomial solve left it (the panel a stop of that round measured), rt0 [m]; fails where the
// last one-GPU block solve ran no such round or m is not its row count
extern "C" int dkmc_debug_get_x_stop_rt0(int m, double *rt0)
{
    Engine &e = eng(); hipStream_t st = e.stream;
    const double *R = (const double *)e.buf[S_XTB_PANELS];
    if (!rt0 || !R || e.x_stop_last.fired == 0 || e.x_stop_last.m != m) return dkmc_fail(13, "get_x_stop_rt0: no one-polynomial round of that size", __FILE__, __LINE__);
    HIPCHK(hipMemcpy2DAsync(rt0, 8, R, (size_t)XB_SP * 8, 8, (size_t)m, hipMemcpyDeviceToHost, st));
    HIPCHK(hipStreamSynchronize(st));
    return e.err_code;
}

// Test aid (tests/test_gpu_tile_f32.py): the tile sums of the 16 test vectors of k_xtb_test_panel on the X left resident by the last single-GPU solve,
// from the fp64 store (stored_bytes = 8) or its fp32 image (4): k_xtb_apply + the fold of the partial sums (k_xtb_fold_local), before any row scaling.
// -4 (tests/test_gpu_tile_drop.py, test_gpu_tile_drop_unit.py): the compact image of the live tiles (or live sub-blocks) at the current
// dkmc_set_x_tile_drop threshold and dkmc_set_x_tile_drop_unit on its launch view, behind a full-view launch as in a solve.
// out (host): [S rank][so], so = width rounded up to a multiple of 4.
extern "C" int dkmc_xtb_tile_product(int width, int stored_bytes, double *out)
{
    Engine &e = eng(); hipStream_t st = e.stream; const XTState &X = g_xt;
    if (!X.valid || comm_attached() || X.tile_n != X.ntiles || X.ns <= 0) return dkmc_fail(13, "xtb_tile_product: needs the X of a single-GPU solve", __FILE__, __LINE__);
    if (stored_bytes != 8 && !((stored_bytes == 4 || stored_bytes == -4) && g_xb.tval32)) return dkmc_fail(13, "xtb_tile_product: no fp32 image of the tile values (dkmc_set_x_tile_f32)", __FILE__, __LINE__);
    XLive lv;                                                                 // stored_bytes -4: the compact image of the live tiles at the current threshold, on its own view
    if (stored_bytes == -4) { if (int rcl = xt_live_for_test(&lv)) return rcl; }
    const bool lvu = stored_bytes == -4;
    const int ns = X.ns, s = std::max(2, std::min(width, 16)), so = 4 * ((s + 3) / 4);
    const long long ncell = (long long)X.nK * X.nW;
    const int nrec = std::max(X.nitems >> X.rec_shift, lvu ? lv.nrecords : 0);
    double *QS = (double *)scratch(S_XTB_QS, (size_t)X.ns_pad * XB_SP * 8);
    double *rowpartB = (double *)scratch(S_XTB_ROWPART, (size_t)(ncell + 1) * XT_R * so * 8);
    double *colpartB = (double *)scratch(S_XTB_COLPART, (size_t)(nrec + 1) * XT_C * so * 8);
    double *sums = (double *)scratch(S_XTB_PANELS, ((size_t)X.ns_pad * so + 2) * 8);
    XCtrl *ctrl = (XCtrl *)scratch(S_MISC2, 256);
    if (!QS || !rowpartB || !colpartB || !sums || !ctrl) return e.err_code;
    HIPCHK(hipMemsetAsync(QS, 0, (size_t)X.ns_pad * XB_SP * 8, st));
    HIPCHK(hipMemsetAsync(rowpartB, 0, (size_t)(ncell + 1) * XT_R * so * 8, st));
    HIPCHK(hipMemsetAsync(colpartB, 0, (size_t)(nrec + 1) * XT_C * so * 8, st));
    HIPCHK(hipMemsetAsync(sums, 0, ((size_t)X.ns_pad * so + 2) * 8, st));
    HIPCHK(hipMemsetAsync(ctrl, 0, sizeof(XCtrl), st));
    hipLaunchKernelGGL(k_xtb_test_panel, dim3((ns * XB_SP + 255) / 256), dim3(256), 0, st, ns, QS);
    const XbApplyArgs xa{lvu ? lv.item_n : X.item_n, lvu ? lv.items : (const XItem *)g_xb.items + X.item_lo, lvu ? lv.tiles : (const XTile *)g_xb.tiles, (int)X.sub_base,
                         (const double *)g_xb.tval, QS, X.nW, rowpartB, colpartB, ctrl,
                         lvu ? lv.tval32 : (stored_bytes == 4 ? (const float *)g_xb.tval32 : (const float *)nullptr)};
    if (lvu) {
        // as a solve does it: a full-view launch on the fp64 store first (its first product), then the dead tiles' cells cleared, then the live view
        const XbApplyArgs xf{X.item_n, (const XItem *)g_xb.items + X.item_lo, (const XTile *)g_xb.tiles, (int)X.sub_base, (const double *)g_xb.tval, QS, X.nW, rowpartB, colpartB, ctrl};
        xtb_apply(xf, true, so, 0, st);
        xt_live_zero_dead(lv, rowpartB, so);
    }
    if (xa.n > 0) xtb_apply(xa, true, so, 0, st);
    hipLaunchKernelGGL(k_xtb_fold_local, dim3(std::max(X.nK, 1)), dim3(XT_NT), 0, st, ns, X.nK, X.nW, so, lvu ? lv.wrange : (const int2 *)g_xb.wrange, lvu ? lv.nitem_w : (const int *)g_xb.nitem_w,
                       (const double *)rowpartB, (const double *)colpartB, sums, (const XCtrl *)ctrl, 0, 0, X.nW);
    KCHK();
    if (out) HIPCHK(hipMemcpyAsync(out, sums, (size_t)ns * so * 8, hipMemcpyDeviceToHost, st));
    HIPCHK(hipStreamSynchronize(st));
    return e.err_code;
}

// ---- measurement aid (bench.py / tools; no counterpart in the reference) ------------------------------------------------------------------
// Average duration of the tile x panel kernel over the X left resident by the last single-GPU solve, `reps` launches back to back.
// variant 0: the kernel as a solve runs it; 1: without its matrix instructions; 2: without re-reading the tile stream (see k_xtb_apply).
static int xtb_time_apply(int width, int variant, int reps, bool f32, double *us, bool live = false);
extern "C" int dkmc_xtb_time_apply(int width, int variant, int reps, double *us) { return xtb_time_apply(width, variant, reps, false, us); }
// the same for the kernel as a solve runs it on the fp64 store (stored_bytes = 8) or on its fp32 image (4; fails when the last assembly made none);
// -4: on the live view and its compact image at the current dkmc_set_x_tile_drop threshold and unit (built afresh; fails where there is none)
extern "C" int dkmc_xtb_time_apply_stored(int width, int stored_bytes, int reps, double *us)
{
    if (stored_bytes != 8 && !((stored_bytes == 4 || stored_bytes == -4) && g_xb.tval32)) return dkmc_fail(13, "xtb_time_apply_stored: no fp32 image of the tile values (dkmc_set_x_tile_f32)", __FILE__, __LINE__);
    return xtb_time_apply(width, 0, reps, stored_bytes != 8, us, stored_bytes == -4);
}
static int xtb_time_apply(int width, int variant, int reps, bool f32, double *us, bool live)
{
    Engine &e = eng(); hipStream_t st = e.stream; const XTState &X = g_xt;
    if (!X.valid || comm_attached() || X.tile_n != X.ntiles || X.ns <= 0 || reps < 1) return dkmc_fail(13, "xtb_time_apply: needs the X of a single-GPU solve", __FILE__, __LINE__);
#ifndef DKMC_MEASURE_VARIANTS
    if (variant != 0) return dkmc_fail(13, "xtb_time_apply: this build carries no measurement variants (DKMC_MEASURE_VARIANTS=1 python __graft_entry__.py)", __FILE__, __LINE__);
#endif
    XLive lv;
    if (live) { if (int rcl = xt_live_for_test(&lv)) return rcl; }
    const int s = std::max(2, std::min(width, 16)), so = 4 * ((s + 3) / 4);
    const long long ncell = (long long)X.nK * X.nW;
    const int nrec = std::max(X.nitems >> X.rec_shift, live ? lv.nrecords : 0);
    double *QS = (double *)scratch(S_XTB_QS, (size_t)X.ns_pad * XB_SP * 8);
    double *rowpartB = (double *)scratch(S_XTB_ROWPART, (size_t)(ncell + 1) * XT_R * so * 8);
    double *colpartB = (double *)scratch(S_XTB_COLPART, (size_t)(nrec + 1) * XT_C * so * 8);
    XCtrl *ctrl = (XCtrl *)scratch(S_MISC2, 256);
    if (!QS || !rowpartB || !colpartB || !ctrl) return e.err_code;
    HIPCHK(hipMemsetAsync(ctrl, 0, sizeof(XCtrl), st));
    hipLaunchKernelGGL(k_xtb_test_panel, dim3((X.ns * XB_SP + 255) / 256), dim3(256), 0, st, X.ns, QS);
    const XbApplyArgs xa{live ? lv.item_n : X.item_n, live ? lv.items : (const XItem *)g_xb.items + X.item_lo, live ? lv.tiles : (const XTile *)g_xb.tiles, (int)X.sub_base,
                         (const double *)g_xb.tval, QS, X.nW, rowpartB, colpartB, ctrl, live ? lv.tval32 : (f32 ? (const float *)g_xb.tval32 : (const float *)nullptr)};
    if (live && xa.n <= 0) return dkmc_fail(13, "xtb_time_apply: the live view holds no tile", __FILE__, __LINE__);
    hipEvent_t e0, e1; HIPCHK(hipEventCreate(&e0)); HIPCHK(hipEventCreate(&e1));
    for (int r = -1; r < reps; ++r) {
        if (r == 0) HIPCHK(hipEventRecord(e0, st));
        xtb_apply(xa, true, so, variant, st);
    }
    HIPCHK(hipEventRecord(e1, st));
    HIPCHK(hipEventSynchronize(e1));
    float ms = 0.f; HIPCHK(hipEventElapsedTime(&ms, e0, e1));
    (void)hipEventDestroy(e0); (void)hipEventDestroy(e1);
    KCHK();
    if (us) *us = (double)ms * 1e3 / reps;
    return e.err_code;
}
