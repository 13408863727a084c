// kcg.hip -- Jacobi-scaled CG for the potential matrix K (background potential, CB edge).
//
// Replaces Assemble_A / Assemble_A_CB (potential_solver_gpu.cu:397-593) + solve_sparse_CG_Jacobi (iterative_solvers_gpu.cu:309-480)
// for K.  Same algorithm, sign convention and stop tests as cg.hip (r = A y - b, p = -r, alpha = r.r / p.Ap, first test on ||r||,
// later ones on ||r||^2, both against tol^2).  What is different from the general CSR solver of cg.hip:
//   * K's off-diagonal entries take only two values, -high_G and -low_G (potential_solver_gpu.cu:202-249), decided by the classes of
//     the two sites.  So the matrix is never written out: per stored entry one int (column | class bit 31), per row the diagonal.
//     4 B per non-zero in the iteration instead of 12 (value + column), and no per-step pass that forms S K S: the Jacobi scaling
//     is applied to the vectors, t = S K (S p).
//   * 8 lanes per row (26 entries on average), every load of a row issued before the first use: three dependent memory latencies
//     per row (row pointers -> columns -> q) instead of one per 16 entries.
// Bytes per iteration: 4 nnz + 4 (m + 1) + 15 vector touches of 8 m  (CSR formulation, SURVEY 8d: 12 nnz + 4 (m + 1) + 96 m).
//
// K is stored in one of three forms, each with its own assemble and product kernels; what fixes the physics and the rounding is written once:
//   CSR positions (k_kc_*)                                            any size; also what the slab-distributed loop (k_ks_*, row lists) runs on
//   blocked form (k_kb_*), one x-sorted LDS window per block          up to KB_MAXROWS rows (default there)
//   windowed blocked form (k_kbw_*), a window of up to KBW_MAXSEG segments   above KB_MAXROWS rows, opt-in (dkmc_set_k_blocked_large); its stored words
//                                                                     take 4 or, opt-in, 2 bytes (dkmc_set_k_window_word_bytes): same operations, same bits
// Shared bodies (__forceinline__, values in and out, so every kernel compiles to what its written-out text did):
//   assembly   k_link (the rule of one entry), k_word (what is stored for it), k_contacts (the two contact sums), k_assemble_tail (diagonal and rhs)
//   product    kb_rows: the pass loop of k_kb_apply and k_kbw_apply (k_kc_apply: 8 lanes per row, no LDS -- another algorithm, on its own)
//   vectors    kc_check0 / kc_update / kc_direction / kc_q<LIST>: all rows (k_kc_*) or the rows of a list (k_ks_*)
//   host       kc_with_cb, kb_raise_lds_limit, kpattern_download, kblocked_upload, cg_poll_loop (cg_host.h: the poll loop of both host loops),
//              kcg_run_* (kcg_run.h: the one-GPU loop without K's assembly; K's solve and the local heat model of heat.hip run on it)
#include "cg_host.h"
#include "slab.h"
#include "kbw_plan.h"
#include "kcg_run.h"
#include <algorithm>
#include <functional>
#include <type_traits>
#include <vector>

#define KC_NT 256

// ---- assembly: class bits + diagonal + rhs in one pass (16 lanes per row) ------------------------------------------------
// CB: 0 potential rule, 1 CB-edge rule, 2 CB-edge rule on atoms only (dkmc_set_cb_edge_domain(1): links to interstitial sites, DEFECT or
// OXYGEN_DEFECT, do not exist -- the domain the revision behind the reference's own CSR dump and current log solved the CB edge on)
__device__ __forceinline__ bool k_interstitial(int e) { return e == DEFECT || e == OXYGEN_DEFECT; }
template <int CB>
__device__ __forceinline__ bool k_high(int ei, int ej, int qi, int qj, const MetalSet &ms)
{
    const bool m1 = is_metal(ei, ms), m2 = is_metal(ej, ms);
    if (CB) return m1 || m2;                                            // potential_solver_gpu.cu:239-249
    const bool cv1 = (ei == VACANCY) && (qi == 0), cv2 = (ej == VACANCY) && (qj == 0);
    return (m1 && m2) || (cv1 && cv2);                                  // :202-217
}

// The rule of one stored entry: the link of site i (element ei, charge qi) to site j
enum { K_NOLINK = 0, K_LOW = 1, K_HIGH = 2 };
template <int CB>
__device__ __forceinline__ int k_link(int ei, int qi, int j, const int *__restrict__ element, const int *__restrict__ charge, const MetalSet &ms)
{
    const int ej = element[j];
    if (CB == 2 && (k_interstitial(ei) || k_interstitial(ej))) return K_NOLINK;
    return k_high<CB>(ei, ej, qi, charge[j], ms) ? K_HIGH : K_LOW;
}
// what is stored for a link to column c: class bit 31 (no link: the column the form's product skips, the row itself, like the padding)
__device__ __forceinline__ int k_word(int link, int c) { return link == K_HIGH ? (c | (int)0x80000000) : c; }
// the 16-bit word of the windowed form (WB = 2): c is an offset into an LDS window of at most KB_MAXWIN <= 2^14 doubles, class bit 15, bit 14 zero
__device__ __forceinline__ unsigned short k_word16(int link, int c) { return (unsigned short)(link == K_HIGH ? (c | 0x8000) : c); }
// the links of row r (site i) to the left and to the right contact, lane l of the row's LPR
struct KContacts { double kl, kr; };
template <int CB, int LPR>
__device__ __forceinline__ KContacts k_contacts(int r, int l, int m, int N_left, int ei, int qi, const int *__restrict__ element, const int *__restrict__ charge,
                                                const MetalSet &ms, double high_G, double low_G, const int *__restrict__ lrp, const int *__restrict__ lci,
                                                const int *__restrict__ rrp, const int *__restrict__ rci)
{
    double kl = 0.0, kr = 0.0;
    const bool cut = CB == 2 && k_interstitial(ei);
    for (int p = lrp[r] + l; p < lrp[r + 1] && !cut; p += LPR) { const int j = lci[p]; const int ej = element[j]; if (CB == 2 && k_interstitial(ej)) continue; kl += k_high<CB>(ei, ej, qi, charge[j], ms) ? high_G : low_G; }
    for (int p = rrp[r] + l; p < rrp[r + 1] && !cut; p += LPR) { const int j = N_left + m + rci[p]; const int ej = element[j]; if (CB == 2 && k_interstitial(ej)) continue; kr += k_high<CB>(ei, ej, qi, charge[j], ms) ? high_G : low_G; }
    return {kl, kr};
}
// diagonal and rhs of a row from its lanes' sums, stored at `row` (the row's index in the form's own order)
template <int CB, int LPR>
__device__ __forceinline__ void k_assemble_tail(int row, int l, double off, KContacts k, double VL, double VR, double *diag, double *rhs)
{
    { off = group_sum<LPR>(off); k.kl = group_sum<LPR>(k.kl); k.kr = group_sum<LPR>(k.kr); }
    if (l == 0) {
        double d = off;          // reduce_rows_into_diag: -(sum of off-diagonals)
        d += k.kl;               // add_vector_to_diagonal (left)
        d += k.kr;               // add_vector_to_diagonal (right)
        if (CB == 2 && d == 0.0) d = 1.0;      // an unlinked interstitial site: identity row, value 0
        diag[row] = d;
        rhs[row] = k.kl * VL + k.kr * VR;
    }
}
// The three assemble kernels keep what differs between the forms: how a row finds its stored entries and how a stored column maps to a site.
template <int CB>
__global__ __launch_bounds__(KC_NT) void k_kc_assemble(int m, int N_left, const int *__restrict__ element, const int *__restrict__ charge,
                                                       MetalSet ms, double high_G, double low_G,
                                                       const int *__restrict__ rp, const int *__restrict__ ci,
                                                       const int *__restrict__ lrp, const int *__restrict__ lci,
                                                       const int *__restrict__ rrp, const int *__restrict__ rci,
                                                       double VL, double VR, int *__restrict__ cf, double *__restrict__ diag, double *__restrict__ rhs)
{
    const int LPR = 16;
    const int g = threadIdx.x / LPR, l = threadIdx.x % LPR;
    const int r = blockIdx.x * (KC_NT / LPR) + g;
    if (r >= m) return;
    const int i = N_left + r;
    const int ei = element[i], qi = charge[i];
    double off = 0.0;
    for (int p = rp[r] + l; p < rp[r + 1]; p += LPR) {
        const int c = ci[p];
        if (c == r) { cf[p] = r; continue; }        // the diagonal
        const int link = k_link<CB>(ei, qi, N_left + c, element, charge, ms);
        if (link == K_NOLINK) { cf[p] = r; continue; }        // no link: stored as the row's own column, which k_kc_apply skips
        cf[p] = k_word(link, c);
        off += link == K_HIGH ? high_G : low_G;
    }
    k_assemble_tail<CB, LPR>(r, l, off, k_contacts<CB, LPR>(r, l, m, N_left, ei, qi, element, charge, ms, high_G, low_G, lrp, lci, rrp, rci), VL, VR, diag, rhs);
}

// s = 1/sqrt(diag); b *= s; y /= s; q = s y
__global__ void k_kc_scale(int m, const double *__restrict__ diag, double *__restrict__ s, double *__restrict__ b, double *__restrict__ y, double *__restrict__ q)
{
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= m) return;
    const double sv = 1.0 / sqrt(diag[i]);
    s[i] = sv;
    b[i] = b[i] * sv;
    const double ys = y[i] * 1 / sv;
    y[i] = ys;
    q[i] = sv * ys;
}

// One iteration = TWO launches (round 4; three before: apply, update, direction -- at 1.1e5 rows, the reference's crossbar, every launch is
// latency-bound and the K solve is the whole superstep).  k_kc_apply forms t = S K q and the partial sums of p.t, r.t and t.t;
// k_kc_step reduces them together with the partial sums of the TRUE r.r its predecessor left, and does the whole vector update:
//     alpha = rr / p.t ; y += alpha p ; r' = r + alpha t ; rr' = rr + alpha (2 r.t + alpha t.t)  (= r'.r' in exact arithmetic: it only
//     feeds beta, the rr of the next iteration is summed from r' itself, so nothing drifts) ; beta = rr' / rr ; p = beta p - r' ; q = s p.
// The stop test is the reference's, on the summed r.r (iterative_solvers_gpu.cu:440-456); it is evaluated by the k_kc_step that follows,
// which then changes nothing: same number of updates as the reference's loop, one product more.
#define KC_NPA 2048         // partial sums per quantity of k_kc_apply (= its largest grid)
#define KC_NP 512           // partial sums of r.r (= the largest grid of k_kc_step)
template <int NT, int NQ>
__device__ __forceinline__ void block_sum_n(double (&v)[NQ], double (*red)[NT / 64])
{
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
#pragma unroll
    for (int k = 0; k < NQ; ++k) v[k] = wave_sum(v[k]);
    __syncthreads();
    if (lane == 0) {
#pragma unroll
        for (int k = 0; k < NQ; ++k) red[k][w] = v[k];
    }
    __syncthreads();
#pragma unroll
    for (int k = 0; k < NQ; ++k) {
        double s = 0.0;
#pragma unroll
        for (int i = 0; i < NT / 64; ++i) s += red[k][i];
        v[k] = s;
    }
}
// part: p.t | r.t | t.t (KC_NPA each) | r.r read by even iterations | r.r read by odd iterations (KC_NP each)
#define KC_PART_DOUBLES (3 * KC_NPA + 2 * KC_NP)
// MODE 0: iteration.  MODE 1: start: r = t - b, p = -r, partial r.r into array 0.
// t = S K q (q = S p), CSR positions, 8 lanes per row, 4 entries per lane and pass.  The products of a row are added pairwise: t = s (d q - sum)
// cancels to a small fraction of its terms, and the rounding of that sum is what limits the residual K-CG can reach (at the crossbar log's
// 1e-12 a left-to-right sum of 16 products per lane needed 820 instead of 735 iterations and moved the KMC time in the fifth digit).
template <int MODE>
__global__ __launch_bounds__(KC_NT) void k_kc_apply(int m, const int *__restrict__ rp, const int *__restrict__ cf, const double *__restrict__ diag,
                                                    const double *__restrict__ s, const double *__restrict__ q, double high_G, double low_G,
                                                    const double *__restrict__ pv, double *__restrict__ t, double *__restrict__ part, const KCtrl *ctrl,
                                                    const double *__restrict__ b, double *__restrict__ r, double *__restrict__ p,
                                                    const int *__restrict__ rowlist = nullptr)
{
    // rowlist (slab-distributed solve): the rows are the m entries of this rank's list
    __shared__ double red[3][KC_NT / 64];
    __shared__ int sdone;
    if (MODE != 1) {
        if (threadIdx.x == 0) sdone = ctrl->done;
        __syncthreads();
        if (sdone) return;
    }
    const int g = threadIdx.x >> 3, l = threadIdx.x & 7;
    double acc[3] = {0.0, 0.0, 0.0};
    for (int ri = blockIdx.x * (KC_NT / 8) + g; ri < m; ri += gridDim.x * (KC_NT / 8)) {
        const int row = rowlist ? rowlist[ri] : ri;
        const int p0 = rp[row], p1 = rp[row + 1];
        const double qr = q[row], dg = diag[row], sv = s[row];
        const double a1 = MODE != 1 ? pv[row] : b[row], a2 = MODE == 0 ? r[row] : 0.0;      // (requested with the rest, used by lane 0 at the end)
        double sum = 0.0;
        for (int pb = p0 + l; pb < p1; pb += 32) {
            int c[4];
#pragma unroll
            for (int u = 0; u < 4; ++u) { const int pp = pb + 8 * u; c[u] = pp < p1 ? cf[pp] : row; }      // out of range / diagonal: skipped below
            double x[4];
#pragma unroll
            for (int u = 0; u < 4; ++u) x[u] = q[c[u] & 0x7fffffff];
#pragma unroll
            for (int u = 0; u < 4; ++u) x[u] = (c[u] & 0x7fffffff) == row ? 0.0 : (c[u] < 0 ? high_G : low_G) * x[u];
            sum += (x[0] + x[1]) + (x[2] + x[3]);
        }
        sum = group_sum<8>(sum);
        if (l == 0) {
            const double tv = sv * (dg * qr - sum);
            if (MODE != 1) { t[row] = tv; acc[0] += a1 * tv; acc[1] += a2 * tv; acc[2] += tv * tv; }
            else { const double rv = -a1 + tv; r[row] = rv; p[row] = -rv; acc[0] += rv * rv; }      // (q = s p: k_kc_q, after every row has read the old q)
        }
    }
    block_sum_n<KC_NT, 3>(acc, red);
    if (threadIdx.x == 0) {
        part[blockIdx.x] = acc[0];          // (MODE 1: r.r in the p.t array: k_kc_check0 moves the total into slot 0 of the first r.r array, whose other slots are zero)
        if (MODE == 0) { part[KC_NPA + blockIdx.x] = acc[1]; part[2 * KC_NPA + blockIdx.x] = acc[2]; }
    }
}

// ---- the blocked form of K (systems up to KB_MAXROWS rows) -------------------------------------------------------------------
// At 1e5 rows (the reference's crossbar, where the K solve IS the superstep) the product is bound by neither bytes nor launches but by
// the rate at which the texture path takes scattered 8-byte addresses: one read of q per non-zero, 2.7e6 of them, 0.43 per ns
// chip-wide.  Site order is the reference's contract and is not spatial (37 % of the entries of a row lie more than 8 192 rows away), so
// kblocked_build (once per pattern) sorts the ROWS OF K by x -- an internal order: y is gathered on entry and scattered on exit, nothing
// outside this file sees it -- and cuts them into one block of R rows per CU.  Every column a block touches then lies in one
// contiguous window of q (R + 2 x the rows within the neighbour distance: 7.7e3 doubles at the crossbar), which the workgroup copies
// into LDS with coalesced loads and gathers from there.  Rows are stored without row pointers: within a block the rows with more than
// 32 off-diagonal entries come first, padded to 64, the others padded to 32 (the padding is the row itself, which the product skips);
// a row's position follows from its index and the block record, so the column loads are issued at once: one global latency + LDS
// instead of three dependent global latencies.
#define KB_NT 1024
#define KB_MAXWIN 14336     // doubles of the LDS window (112 KB)
#define KB_WREG (KB_MAXWIN / KB_NT)
__device__ __forceinline__ int kb_row_base(const int4 &bi, int k, int *width)
{
    const bool lg = k < bi.w;
    *width = lg ? 64 : 32;
    return bi.z + (lg ? k * 64 : bi.w * 64 + (k - bi.w) * 32);
}
template <int CB>
__global__ __launch_bounds__(KC_NT) void k_kb_assemble(int m, int N_left, int R, const int4 *__restrict__ blk, const int *__restrict__ perm,
                                                       const int *__restrict__ pcol, const int *__restrict__ element, const int *__restrict__ charge,
                                                       MetalSet ms, double high_G, double low_G,
                                                       const int *__restrict__ lrp, const int *__restrict__ lci,
                                                       const int *__restrict__ rrp, const int *__restrict__ rci,
                                                       double VL, double VR, int *__restrict__ cf, double *__restrict__ diag, double *__restrict__ rhs)
{
    const int LPR = 16;
    const int g = threadIdx.x / LPR, l = threadIdx.x % LPR;
    const int rb = blockIdx.x * (KC_NT / LPR) + g;           // row in the blocked order
    if (rb >= m) return;
    const int bb = rb / R;
    int width;
    const int base = kb_row_base(blk[bb], rb - bb * R, &width);
    const int r = perm[rb], i = N_left + r;
    const int ei = element[i], qi = charge[i];
    double off = 0.0;
    for (int k = l; k < width; k += LPR) {
        const int c = pcol[base + k];
        if (c == rb) { cf[base + k] = rb; continue; }        // padding
        const int link = k_link<CB>(ei, qi, N_left + perm[c], element, charge, ms);
        if (link == K_NOLINK) { cf[base + k] = rb; continue; }        // no link: stored like padding
        cf[base + k] = k_word(link, c);
        off += link == K_HIGH ? high_G : low_G;
    }
    k_assemble_tail<CB, LPR>(rb, l, off, k_contacts<CB, LPR>(r, l, m, N_left, ei, qi, element, charge, ms, high_G, low_G, lrp, lci, rrp, rci), VL, VR, diag, rhs);
}
// s = 1/sqrt(diag); b *= s; yb = y[perm] / s; q = s yb   (entry into the blocked order)
__global__ void k_kb_scale(int m, const int *__restrict__ perm, const double *__restrict__ diag, double *__restrict__ s, double *__restrict__ b,
                           const double *__restrict__ y, double *__restrict__ yb, double *__restrict__ q)
{
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= m) return;
    const double sv = 1.0 / sqrt(diag[i]);
    s[i] = sv;
    b[i] = b[i] * sv;
    const double ys = y[perm[i]] * 1 / sv;
    yb[i] = ys;
    q[i] = sv * ys;
}
__global__ void k_kb_unscale(int m, const int *__restrict__ perm, const double *__restrict__ yb, const double *__restrict__ s, double *__restrict__ y)
{
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < m) y[perm[i]] = yb[i] * s[i];
}
// The stored words of one row as lane l of its 4 lanes loads them, 16 bytes per load.  WB = 4 (ints): ints 4l.. and 16+4l.. (wide rows: 32+4l.., 48+4l.. too),
// four loads.  WB = 2 (the windowed form with dkmc_set_k_window_word_bytes(2)): the same entries as 16-bit words, chunk l of the row (wide rows: chunk
// 4 + l too; kbw_plan.h: kbw_halfword_pos), two loads.  kb_unpack gives both the ints c[0..15] of the 4-byte form -- offset | class bit 31 -- in the same
// slots, so everything after it is one text.
static_assert(KB_MAXWIN <= 1 << 14, "a 16-bit stored word keeps the LDS offset in bits 0-13");
template <int WB> struct KbRow { int4 cc[WB == 2 ? 2 : 4]; bool lg; };
template <int WB>
__device__ __forceinline__ void kb_load_row(const int *__restrict__ cf, const int4 &bi, int k, int l, bool in, KbRow<WB> &row)
{
    int width;
    const int base = kb_row_base(bi, k, &width);          // in words of WB bytes
    row.lg = in && width == 64;
    if (!in) return;
    if (WB == 2) {
        const int4 *cr = (const int4 *)((const unsigned short *)cf + base) + l;
        row.cc[0] = cr[0];
        if (width == 64) row.cc[1] = cr[4];
    } else {
        const int4 *cr = (const int4 *)(cf + base) + l;
        row.cc[0] = cr[0]; row.cc[1] = cr[4];
        if (width == 64) { row.cc[2] = cr[8]; row.cc[3] = cr[12]; }
    }
}
template <int WB>
__device__ __forceinline__ void kb_unpack(const KbRow<WB> &row, int (&c)[16])
{
    if (WB == 2) {
#pragma unroll
        for (int j = 0; j < 2; ++j) {
            const unsigned v[4] = {(unsigned)row.cc[j].x, (unsigned)row.cc[j].y, (unsigned)row.cc[j].z, (unsigned)row.cc[j].w};
#pragma unroll
            for (int i = 0; i < 4; ++i) {          // low half: the even entry, high half: the odd one
                c[8 * j + 2 * i] = (int)((v[i] & 0x3fffu) | ((v[i] << 16) & 0x80000000u));
                c[8 * j + 2 * i + 1] = (int)(((v[i] >> 16) & 0x3fffu) | (v[i] & 0x80000000u));
            }
        }
    } else {
#pragma unroll
        for (int j = 0; j < 4; ++j) { c[4 * j] = row.cc[j].x; c[4 * j + 1] = row.cc[j].y; c[4 * j + 2] = row.cc[j].z; c[4 * j + 3] = row.cc[j].w; }
    }
}
// The pass loop of the two blocked products: lane l of the 4 of row k, k + KB_NT / 4, ... of a block of nrows rows that starts at row r0.
// win: the block's window of q in LDS; a stored column c is read at win[c - woff] (blocked form: woff = first column of the window; windowed
// form: a literal 0, the columns are offsets into the window) and is the row itself -- padding, no link: skipped -- when it equals self0 + k.
// row: the stored columns of the first pass, requested by the kernel before it waits for its window.
// The products of a row are added pairwise: t = s (d q - sum) cancels to a small fraction of its terms, and the rounding of that sum is what
// limits the residual K-CG can reach (k_kc_apply: at the crossbar log's 1e-12 a left-to-right sum needed 820 instead of 735 iterations).
// Every load of a pass is requested before anything is waited for -- the columns of the NEXT pass as soon as this pass's gathers are issued --:
// one global latency + LDS per pass instead of a chain.  113 VGPR (MODE 0; MODE 1: 107), no scratch: 4 waves per SIMD, what one 1024-thread
// workgroup per CU (the LDS window) runs at.  WB: bytes of a stored word (KbRow<WB>, kb_load_row, kb_unpack); only the load of a row's words and
// their unpacking differ (WB = 2: 106 / 100 VGPR, no scratch -- two int4 of words in flight per lane instead of four).
template <int MODE, int WB>
__device__ __forceinline__ void kb_rows(const double *win, int woff, int self0, int r0, int nrows, int k, int l, KbRow<WB> row0, const int4 bi, const int *__restrict__ cf,
                                        const double *__restrict__ diag, const double *__restrict__ s, double high_G, double low_G, const double *__restrict__ pv,
                                        double *__restrict__ t, double *__restrict__ part, const double *__restrict__ b, double *__restrict__ r, double *__restrict__ p,
                                        double (*red)[KB_NT / 64])
{
    KbRow<WB> cur = row0;
    double acc[3] = {0.0, 0.0, 0.0};
    for (; k < nrows; k += KB_NT / 4) {
        const int row = r0 + k, self = self0 + k;
        const double qr = win[self - woff], dg = diag[row], sv = s[row];
        const double a1 = MODE == 0 ? pv[row] : b[row], a2 = MODE == 0 ? r[row] : 0.0;
        int c[16];
        kb_unpack(cur, c);
        const bool lgc = cur.lg;
        double x[16];
#pragma unroll
        for (int u = 0; u < 8; ++u) x[u] = win[(c[u] & 0x7fffffff) - woff];
        if (lgc) {
#pragma unroll
            for (int u = 8; u < 16; ++u) x[u] = win[(c[u] & 0x7fffffff) - woff];
        }
        kb_load_row(cf, bi, k + KB_NT / 4, l, k + KB_NT / 4 < nrows, cur);      // next pass
#pragma unroll
        for (int u = 0; u < 8; ++u) x[u] = (c[u] & 0x7fffffff) == self ? 0.0 : (c[u] < 0 ? high_G : low_G) * x[u];
        double sum = ((x[0] + x[1]) + (x[2] + x[3])) + ((x[4] + x[5]) + (x[6] + x[7]));
        if (lgc) {
#pragma unroll
            for (int u = 8; u < 16; ++u) x[u] = (c[u] & 0x7fffffff) == self ? 0.0 : (c[u] < 0 ? high_G : low_G) * x[u];
            sum += ((x[8] + x[9]) + (x[10] + x[11])) + ((x[12] + x[13]) + (x[14] + x[15]));
        }
        sum = group_sum<4>(sum);
        if (l == 0) {
            const double tv = sv * (dg * qr - sum);
            if (MODE == 0) { t[row] = tv; acc[0] += a1 * tv; acc[1] += a2 * tv; acc[2] += tv * tv; }
            else { const double rv = -a1 + tv; r[row] = rv; p[row] = -rv; acc[0] += rv * rv; }
        }
    }
    block_sum_n<KB_NT, 3>(acc, red);
    if (threadIdx.x == 0) {
        part[blockIdx.x] = acc[0];
        if (MODE == 0) { part[KC_NPA + blockIdx.x] = acc[1]; part[2 * KC_NPA + blockIdx.x] = acc[2]; }
    }
}
template <int MODE>
__global__ __launch_bounds__(KB_NT) void k_kb_apply(int m, int R, const int4 *__restrict__ blk, const int *__restrict__ cf, const double *__restrict__ diag,
                                                    const double *__restrict__ s, const double *__restrict__ q, double high_G, double low_G,
                                                    const double *__restrict__ pv, double *__restrict__ t, double *__restrict__ part, const KCtrl *ctrl,
                                                    const double *__restrict__ b, double *__restrict__ r, double *__restrict__ p)
{
    extern __shared__ double win[];
    __shared__ double red[3][KB_NT / 64];
    __shared__ int sdone;
    const int4 bi = blk[blockIdx.x];
    const int wlo = bi.x, wn = bi.y;
    const int r0 = blockIdx.x * R, nrows = min(R, m - r0);
    const int g = threadIdx.x >> 2, l = threadIdx.x & 3;
    // everything the first pass needs is requested before anything is waited for
    double wv[KB_WREG];
#pragma unroll
    for (int j = 0; j < KB_WREG; ++j) { const int idx = threadIdx.x + j * KB_NT; wv[j] = idx < wn ? q[wlo + idx] : 0.0; }
    KbRow<4> row;
    kb_load_row(cf, bi, g, l, g < nrows, row);
    if (MODE == 0 && threadIdx.x == 0) sdone = ctrl->done;
#pragma unroll
    for (int j = 0; j < KB_WREG; ++j) { const int idx = threadIdx.x + j * KB_NT; if (idx < wn) win[idx] = wv[j]; }
    __syncthreads();
    if (MODE == 0 && sdone) return;
    kb_rows<MODE, 4>(win, wlo, r0, r0, nrows, g, l, row, bi, cf, diag, s, high_G, low_G, pv, t, part, b, r, p, red);
}

// ---- the windowed blocked form of K (above KB_MAXROWS rows, opt-in: dkmc_set_k_blocked_large) --------------------------------------------
// Above 2.6e5 rows one x-sorted window per block no longer fits the LDS: a block of x-sorted rows is a thin slice through the whole lateral
// plane.  kbw_build (kbw_plan.h) orders the rows spatially instead -- lateral columns of one neighbour distance, walked in serpentine order,
// rows of a column in x -- and cuts them into blocks of R rows whose window (every row the block reads) is a short list of contiguous
// segments of that order (at most KBW_MAXSEG), copied one after the other into one LDS image; the stored columns are offsets into that image.
// Same storage of the rows (no row pointers; > 32 entries first, padded to 64, the others to 32; padding = the row's own offset), same
// pass loop (kb_rows: pairwise row sums, fused partials) as k_kb_apply; more blocks than CUs run as a grid, several workgroups per CU one after the other.
// The iteration keeps the reference-order three launches (product, k_kc_update, k_kc_direction; see k_kc_update for why beta is summed directly).
// LDS budget KB_MAXWIN doubles (112 KiB of the 160 KiB per CU): one 1024-thread workgroup per CU, 16 waves = 4 per SIMD.
// k_kbw_apply<0>: 113 VGPR, 79 SGPR, no scratch (hipcc -Rpass-analysis=kernel-resource-usage, gfx950; <1>: 107 VGPR): registers and LDS window
// both allow 4 waves per SIMD, the occupancy it runs at (one workgroup of 16 waves per CU at a time).  tile:20 (3.64e6 rows, 1 143 blocks of
// 3 189 rows, windows 3.4 x the rows, 7.2 segments per window): 173 us per launch against 304 us for k_kc_apply in the same run, 783 MB
// per launch (4 B per stored entry, 36.8 per row with the padding; window copies; 5 vector touches) = 4.5 TB/s
// (profiles/kcg_forms_tile20_product_launches.txt, kcg_forms_tile20_tile10.jsonl).
// WB = 2 (dkmc_set_k_window_word_bytes(2), opt-in): a stored word is an offset into that LDS image (< KB_MAXWIN <= 2^14: bits 0-13) and the class (bit 15),
// 16 bits; a row takes 64 or 128 bytes, its words placed (kbw_plan.h: kbw_halfword_pos) so that lane l's one 16-byte load per chunk holds the entries its
// two loads of ints hold, in the same slots.  Every element of t is then the same sequence of fp64 operations as with WB = 4: the same bits.
// k_kbw_apply<0, 2>: 106 VGPR, 79 SGPR, no scratch; <1, 2>: 100 VGPR, no scratch; <0, 4> / <1, 4>: 113 / 107 as before (same command); LDS unchanged.
// tile:20: 514 MB per launch instead of 783, 135.6 us against 176.5 us for <0, 4> in the same run (3.8 against 4.4 TB/s on their bytes: no longer bound by
// HBM alone), 191 against 234 us per iteration (profiles/kcg_words_tile20_product_launches.txt, kcg_words_tile20_tile10.jsonl).
__device__ __forceinline__ int kbw_row(const int4 *sg, int off)
{
    int g = 0;
#pragma unroll
    for (int s = 0; s < KBW_MAXSEG; ++s) { const int4 v = sg[s]; if (off >= v.x) g = v.z + (off - v.x); }      // (unused entries: x = INT_MAX)
    return g;
}
// (R >= KC_NT / 16: the 16 rows of a workgroup lie in at most two blocks, whose segment tables it keeps in LDS)
// (WB = 2: cf holds 16-bit words, entry k of a row at kbw_halfword_pos(width, k); pcol, read once per solve, keeps its ints in entry order)
template <int CB, int WB>
__global__ __launch_bounds__(KC_NT) void k_kbw_assemble(int m, int N_left, int R, int nb, const int4 *__restrict__ blk, const int4 *__restrict__ seg,
                                                        const int *__restrict__ perm, const int *__restrict__ pcol, const int *__restrict__ element,
                                                        const int *__restrict__ charge, MetalSet ms, double high_G, double low_G,
                                                        const int *__restrict__ lrp, const int *__restrict__ lci,
                                                        const int *__restrict__ rrp, const int *__restrict__ rci,
                                                        double VL, double VR, int *__restrict__ cf, double *__restrict__ diag, double *__restrict__ rhs)
{
    const int LPR = 16;
    __shared__ int4 ssg[2][KBW_MAXSEG];
    const int g = threadIdx.x / LPR, l = threadIdx.x % LPR;
    const int rb = blockIdx.x * (KC_NT / LPR) + g;           // row in the blocked order
    const int bb0 = blockIdx.x * (KC_NT / LPR) / R;
    if (threadIdx.x < 2 * KBW_MAXSEG && bb0 + (int)threadIdx.x / KBW_MAXSEG < nb)
        ssg[threadIdx.x / KBW_MAXSEG][threadIdx.x % KBW_MAXSEG] = seg[(size_t)bb0 * KBW_MAXSEG + threadIdx.x];
    __syncthreads();
    if (rb >= m) return;
    const int bb = rb / R;
    const int4 bi = blk[bb];
    const int4 *sg = ssg[bb - bb0];
    int width;
    const int base = kb_row_base(bi, rb - bb * R, &width);
    const int self = bi.y + (rb - bb * R);                   // the row's own offset in the window
    const int r = perm[rb], i = N_left + r;
    const int ei = element[i], qi = charge[i];
    double off = 0.0;
    for (int k = l; k < width; k += LPR) {
        const int c = pcol[base + k];
        int link = K_NOLINK;                                      // padding, no link: stored as the row's own offset
        if (c != self) link = k_link<CB>(ei, qi, N_left + perm[kbw_row(sg, c)], element, charge, ms);
        const int cs = link == K_NOLINK ? self : c;
        if (WB == 2) ((unsigned short *)cf)[base + kbw_halfword_pos(width, k)] = k_word16(link, cs);
        else cf[base + k] = k_word(link, cs);
        if (link != K_NOLINK) off += link == K_HIGH ? high_G : low_G;
    }
    k_assemble_tail<CB, LPR>(rb, l, off, k_contacts<CB, LPR>(r, l, m, N_left, ei, qi, element, charge, ms, high_G, low_G, lrp, lci, rrp, rci), VL, VR, diag, rhs);
}
template <int MODE, int WB>
__global__ __launch_bounds__(KB_NT) void k_kbw_apply(int m, int R, const int4 *__restrict__ blk, const int4 *__restrict__ seg, const int *__restrict__ cf,
                                                     const double *__restrict__ diag, const double *__restrict__ s, const double *__restrict__ q,
                                                     double high_G, double low_G, const double *__restrict__ pv, double *__restrict__ t,
                                                     double *__restrict__ part, const KCtrl *ctrl, const double *__restrict__ b,
                                                     double *__restrict__ r, double *__restrict__ p)
{
    extern __shared__ double win[];
    __shared__ double red[3][KB_NT / 64];
    if (MODE == 0 && ctrl->done) return;                    // (a launch after the stop test: one scalar load, not a window copy)
    const int4 bi = blk[blockIdx.x];
    const int wn = bi.x, self0 = bi.y;
    const int r0 = blockIdx.x * R, nrows = min(R, m - r0);
    const int g = threadIdx.x >> 2, l = threadIdx.x & 3;
    // the segments of the window, copied into one LDS image: every load is issued before anything is waited for
    const int4 *sg = seg + (size_t)blockIdx.x * KBW_MAXSEG;
    int slo[KBW_MAXSEG], sbase[KBW_MAXSEG];
#pragma unroll
    for (int j = 0; j < KBW_MAXSEG; ++j) { const int4 v = sg[j]; slo[j] = v.x; sbase[j] = v.z - v.x; }
    double wv[KB_WREG];
#pragma unroll
    for (int j = 0; j < KB_WREG; ++j) {
        const int idx = threadIdx.x + j * KB_NT;
        int gb = 0;
#pragma unroll
        for (int u = 0; u < KBW_MAXSEG; ++u) gb = idx >= slo[u] ? sbase[u] : gb;
        wv[j] = idx < wn ? q[gb + idx] : 0.0;
    }
    KbRow<WB> row;
    kb_load_row(cf, bi, g, l, g < nrows, row);
#pragma unroll
    for (int j = 0; j < KB_WREG; ++j) { const int idx = threadIdx.x + j * KB_NT; if (idx < wn) win[idx] = wv[j]; }
    __syncthreads();
    kb_rows<MODE, WB>(win, 0, self0, r0, nrows, g, l, row, bi, cf, diag, s, high_G, low_G, pv, t, part, b, r, p, red);
}

// The vector kernels of the reference-order loop, written once: LIST = false over all rows i < n (k_kc_*), LIST = true over the n rows of a
// list (k_ks_*, the slab-distributed loop: a rank's own rows).  A compile-time flag: the dense kernels carry neither a branch nor an argument for it.
// xa: block partials of the start's r.r (n of them); LIST = false also leaves the total in *rr0 (slot 0 of the first r.r array, whose other slots are zero).
template <bool LIST>
__device__ __forceinline__ void kc_check0(int n, const double *xa, double *rr0, KCtrl *ctrl, double tol2)
{
    __shared__ double red[KC_NT / 64];
    double s = 0.0;
    for (int i = threadIdx.x; i < n; i += KC_NT) s += xa[i];
    const double rr = block_sum_all<KC_NT>(s, red);
    if (threadIdx.x == 0) { if (!LIST) *rr0 = rr; ctrl->rr[0] = rr; ctrl->rr[1] = rr; ctrl->iters = 0; ctrl->done = !(sqrt(rr) > tol2); }
}
// (rr0 points into part[]: slot 0 of the r.r array that iteration 0 reads; the partials summed are MODE 1's r.r in the p.t array)
__global__ __launch_bounds__(KC_NT) void k_kc_check0(double *part, KCtrl *ctrl, double tol2) { kc_check0<false>(KC_NPA, part, part + 3 * KC_NPA, ctrl, tol2); }
__global__ __launch_bounds__(KC_NT) void k_kc_step(int m, int it, double *__restrict__ part, double *__restrict__ p, const double *__restrict__ t,
                                                   double *__restrict__ y, double *__restrict__ r, const double *__restrict__ s, double *__restrict__ q,
                                                   KCtrl *ctrl, double tol2, int npa)
{
    // npa: slots of the p.t / r.t / t.t arrays that can be non-zero (the grid of the product, rounded up to KC_NT)
    __shared__ double red[4][KC_NT / 64];
    __shared__ int sdone;
    if (threadIdx.x == 0) sdone = ctrl->done;
    int i = blockIdx.x * KC_NT + threadIdx.x;
    double pi = 0.0, ti = 0.0, yi = 0.0, ri = 0.0, si = 0.0;
    if (i < m) { pi = p[i]; ti = t[i]; yi = y[i]; ri = r[i]; si = s[i]; }       // in flight while the partial sums are reduced
    const double *prr = part + 3 * KC_NPA + (it & 1) * KC_NP;
    double *prr_next = part + 3 * KC_NPA + ((it + 1) & 1) * KC_NP;
    double v[4] = {0.0, 0.0, 0.0, 0.0};
    for (int j = threadIdx.x; j < npa; j += KC_NT) { v[0] += part[j]; v[1] += part[KC_NPA + j]; v[2] += part[2 * KC_NPA + j]; }
#pragma unroll
    for (int k = 0; k < KC_NP / KC_NT; ++k) v[3] += prr[threadIdx.x + k * KC_NT];
    block_sum_n<KC_NT, 4>(v, red);
    if (sdone) return;
    const double rr = v[3];
    if (it > 0 && !(rr > tol2)) {            // the test the reference makes after update `it`: every workgroup takes the same decision
        if (blockIdx.x == 0 && threadIdx.x == 0) { ctrl->rr[0] = rr; ctrl->iters = it; ctrl->done = 1; }
        return;
    }
    const double alpha = rr / v[0];
    const double rr_new = rr + alpha * (2.0 * v[1] + alpha * v[2]);
    const double beta = rr_new / rr;
    double acc = 0.0;
    while (i < m) {
        y[i] = yi + alpha * pi;
        const double rn = ri + alpha * ti;
        r[i] = rn;
        acc += rn * rn;
        const double pn = pi * beta - rn;
        p[i] = pn;
        q[i] = si * pn;
        i += gridDim.x * KC_NT;
        if (i < m) { pi = p[i]; ti = t[i]; yi = y[i]; ri = r[i]; si = s[i]; }
    }
    const double tot = block_sum_all<KC_NT>(acc, red[0]);
    if (threadIdx.x == 0) {
        prr_next[blockIdx.x] = tot;
        if (blockIdx.x == 0) { ctrl->rr[0] = rr_new; ctrl->iters = it + 1; }
    }
}
// Reference-order iteration (CSR positions, systems above the size of the blocked form): product, update, direction -- three launches,
// beta from the DIRECT sum r'.r' / r.r exactly as solve_sparse_CG_Jacobi forms it (iterative_solvers_gpu.cu:424-455).  At the default
// tolerance (1e-6 on the scaled residual) K fixes phi only to cond(K) x 1e-6 -- 0.3 V on weakly coupled sites at 9.4e5 sites -- and which
// of the admissible solutions a run lands on is decided by its rounding: with beta from the recurrence (k_kc_step) the solve needs 12 % more
// iterations there (1 297 against 1 161) and lands 0.3 V away from the reference-order iterate on 1e-4 of the sites, enough to select other
// events; with the direct sums it follows the reference-order iterate to rounding and the events of the 9.4e5-site superstep are the oracle's.
// At a converged tolerance (the reference's logs: 1e-12) the two loops agree to 1e-9 V, and below 2.6e5 rows the K solve is latency-bound:
// the blocked form keeps the two-launch loop.
template <bool LIST>
__device__ __forceinline__ void kc_update(int n, const int *__restrict__ rows, int it, const double *__restrict__ part, int npa, const double *__restrict__ p,
                                          const double *__restrict__ t, double *__restrict__ y, double *__restrict__ r, double *__restrict__ part_rr, const KCtrl *ctrl)
{
    __shared__ double red[KC_NT / 64];
    __shared__ int sdone;
    if (threadIdx.x == 0) sdone = ctrl->done;
    double a = 0.0;
    for (int j = threadIdx.x; j < npa; j += KC_NT) a += part[j];
    const double pAp = block_sum_all<KC_NT>(a, red);
    if (sdone) return;
    const double alpha = ctrl->rr[it & 1] / pAp;
    double acc = 0.0;
    for (int i = blockIdx.x * KC_NT + threadIdx.x; i < n; i += gridDim.x * KC_NT) {
        const int row = LIST ? rows[i] : i;
        y[row] += alpha * p[row];
        const double rn = r[row] + alpha * t[row];
        r[row] = rn;
        acc += rn * rn;
    }
    const double tot = block_sum_all<KC_NT>(acc, red);
    if (threadIdx.x == 0) part_rr[blockIdx.x] = tot;
}
template <bool LIST>
__device__ __forceinline__ void kc_direction(int n, const int *__restrict__ rows, int it, const double *__restrict__ part_rr, int np, const double *__restrict__ r,
                                             double *__restrict__ p, const double *__restrict__ s, double *__restrict__ q, KCtrl *ctrl, double tol2)
{
    __shared__ double red[KC_NT / 64];
    __shared__ int sdone;
    if (threadIdx.x == 0) sdone = ctrl->done;
    double a = 0.0;
    for (int j = threadIdx.x; j < np; j += KC_NT) a += part_rr[j];
    const double rr_new = block_sum_all<KC_NT>(a, red);
    if (sdone) return;
    const double beta = rr_new / ctrl->rr[it & 1];
    for (int i = blockIdx.x * KC_NT + threadIdx.x; i < n; i += gridDim.x * KC_NT) {
        const int row = LIST ? rows[i] : i;
        const double pn = p[row] * beta - r[row];
        p[row] = pn;
        q[row] = s[row] * pn;
    }
    if (blockIdx.x == 0 && threadIdx.x == 0) {
        ctrl->rr[(it + 1) & 1] = rr_new;
        ctrl->iters = it + 1;
        if (!(rr_new > tol2)) ctrl->done = 1;
    }
}
__global__ __launch_bounds__(KC_NT) void k_kc_update(int m, int it, const double *__restrict__ part, int npa, const double *__restrict__ p,
                                                     const double *__restrict__ t, double *__restrict__ y, double *__restrict__ r,
                                                     double *__restrict__ part_rr, const KCtrl *ctrl)
{ kc_update<false>(m, nullptr, it, part, npa, p, t, y, r, part_rr, ctrl); }
__global__ __launch_bounds__(KC_NT) void k_kc_direction(int m, int it, const double *__restrict__ part_rr, const double *__restrict__ r,
                                                        double *__restrict__ p, const double *__restrict__ s, double *__restrict__ q, KCtrl *ctrl, double tol2)
{ kc_direction<false>(m, nullptr, it, part_rr, KC_NP, r, p, s, q, ctrl, tol2); }
template <bool LIST>
__device__ __forceinline__ void kc_q(int n, const int *__restrict__ rows, const double *__restrict__ s, const double *__restrict__ p, double *__restrict__ q)
{
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) { const int row = LIST ? rows[i] : i; q[row] = s[row] * p[row]; }
}
__global__ void k_kc_q(int m, const double *__restrict__ s, const double *__restrict__ p, double *__restrict__ q) { kc_q<false>(m, nullptr, s, p, q); }
__global__ void k_kc_unscale(int m, double *__restrict__ y, const double *__restrict__ s)
{
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < m) y[i] = y[i] * s[i];
}

// cb (0 potential rule, 1 CB-edge rule, 2 CB-edge rule on atoms only) as the CB template argument: f(std::integral_constant<int, CB>)
template <class F> static void kc_with_cb(int cb, F &&f)
{
    if (cb == 2) f(std::integral_constant<int, 2>{}); else if (cb) f(std::integral_constant<int, 1>{}); else f(std::integral_constant<int, 0>{});
}
// the dynamic-LDS limit of the two instantiations of a blocked product, raised to the largest window once per process (*set)
template <class K> static int kb_raise_lds_limit(K apply0, K apply1, bool *set)
{
    if (*set) return 0;
    HIPCHK(hipFuncSetAttribute((const void *)apply0, hipFuncAttributeMaxDynamicSharedMemorySize, KB_MAXWIN * 8));
    HIPCHK(hipFuncSetAttribute((const void *)apply1, hipFuncAttributeMaxDynamicSharedMemorySize, KB_MAXWIN * 8));
    *set = true;
    return 0;
}
// a K pattern on the host: row pointers, columns, x and (y_d, z_d not null) y, z of its rows
namespace { struct KPattern { std::vector<int> rp, ci; std::vector<double> x, y, z; }; }
static bool kpattern_download(KPattern &P, const int *rp_d, const int *ci_d, int m, int nnz, const double *x_d, const double *y_d, const double *z_d, hipStream_t st)
{
    P.rp = std::vector<int>(m + 1); P.ci = std::vector<int>(nnz); P.x = std::vector<double>(m);
    if (hipMemcpyAsync(P.rp.data(), rp_d, (size_t)(m + 1) * 4, hipMemcpyDeviceToHost, st) != hipSuccess) return false;
    if (hipMemcpyAsync(P.ci.data(), ci_d, (size_t)nnz * 4, hipMemcpyDeviceToHost, st) != hipSuccess) return false;
    if (hipMemcpyAsync(P.x.data(), x_d, (size_t)m * 8, hipMemcpyDeviceToHost, st) != hipSuccess) return false;
    if (y_d) { P.y = std::vector<double>(m); if (hipMemcpyAsync(P.y.data(), y_d, (size_t)m * 8, hipMemcpyDeviceToHost, st) != hipSuccess) return false; }
    if (z_d) { P.z = std::vector<double>(m); if (hipMemcpyAsync(P.z.data(), z_d, (size_t)m * 8, hipMemcpyDeviceToHost, st) != hipSuccess) return false; }
    return hipStreamSynchronize(st) == hipSuccess;
}
void kblocked_free(KBlocked *kb);
// the tables of a blocked form onto the device (seg: the windowed form's segment tables, or null); frees kb and returns nullptr when that fails
static KBlocked *kblocked_upload(KBlocked *kb, const int *perm, const int *pcol, const void *blk, const void *seg)
{
    const size_t nperm = (size_t)kb->m * 4, npcol = (size_t)kb->total * 4, nblk = (size_t)kb->nb * sizeof(int4), nseg = (size_t)kb->nb * KBW_MAXSEG * sizeof(int4);
    bool ok = hipMalloc((void **)&kb->perm, nperm) == hipSuccess && hipMalloc((void **)&kb->pcol, npcol) == hipSuccess &&
              hipMalloc((void **)&kb->blk, nblk) == hipSuccess && (!seg || hipMalloc((void **)&kb->seg, nseg) == hipSuccess);
    ok = ok && hipMemcpy(kb->perm, perm, nperm, hipMemcpyHostToDevice) == hipSuccess && hipMemcpy(kb->pcol, pcol, npcol, hipMemcpyHostToDevice) == hipSuccess &&
         hipMemcpy(kb->blk, blk, nblk, hipMemcpyHostToDevice) == hipSuccess && (!seg || hipMemcpy(kb->seg, seg, nseg, hipMemcpyHostToDevice) == hipSuccess);
    if (!ok) { kblocked_free(kb); (void)hipGetLastError(); return nullptr; }
    return kb;
}

// Builds the blocked form of a K pattern (host side, once per initialize_sparsity; nullptr when the system is too large for it, a row has
// more than 64 off-diagonal entries or a window does not fit the LDS: the solve then uses the CSR positions).  x: device pointer to the x
// coordinate of the pattern's rows.
#define KB_MAXROWS 262144
KBlocked *kblocked_build(const int *rp_d, const int *ci_d, int m, int nnz, const double *x_d, hipStream_t st)
{
    if (!eng().k_blocked || m < 1 || m > KB_MAXROWS || nnz < 1) return nullptr;
    KPattern H;
    if (!kpattern_download(H, rp_d, ci_d, m, nnz, x_d, nullptr, nullptr, st)) return nullptr;
    const std::vector<int> &rp = H.rp, &ci = H.ci;
    const std::vector<double> &x = H.x;
    std::vector<int> perm(m);
    for (int i = 0; i < m; ++i) perm[i] = i;
    std::stable_sort(perm.begin(), perm.end(), [&](int a, int b) { return x[a] < x[b]; });
    int R = (m + 255) / 256;
    R = (R + 63) / 64 * 64;
    const int nb = (m + R - 1) / R;
    auto offdiag = [&](int r) { int n = 0; for (int p = rp[r]; p < rp[r + 1]; ++p) n += ci[p] != r; return n; };
    std::vector<int4> blk(nb);
    long long total = 0;
    int maxints = 0;
    for (int b = 0; b < nb; ++b) {
        const int lo = b * R, hi = std::min(m, lo + R);
        for (int i = lo; i < hi; ++i) if (offdiag(perm[i]) > 64) return nullptr;
        auto mid = std::stable_partition(perm.begin() + lo, perm.begin() + hi, [&](int r) { return offdiag(r) > 32; });
        const int nl = (int)(mid - (perm.begin() + lo));
        blk[b].z = (int)total; blk[b].w = nl;
        total += (long long)nl * 64 + (long long)(hi - lo - nl) * 32;
        maxints = std::max(maxints, nl * 64 + (hi - lo - nl) * 32);
    }
    std::vector<int> inv(m);
    for (int i = 0; i < m; ++i) inv[perm[i]] = i;
    std::vector<int> pcol((size_t)total);
    int maxwin = 0;
    long long winsum = 0;
    for (int b = 0; b < nb; ++b) {
        const int lo = b * R, hi = std::min(m, lo + R);
        int cmin = lo, cmax = hi - 1;
        for (int i = lo; i < hi; ++i) {
            const int k = i - lo, nl = blk[b].w, width = k < nl ? 64 : 32;
            int *dst = pcol.data() + blk[b].z + (k < nl ? (size_t)k * 64 : (size_t)nl * 64 + (size_t)(k - nl) * 32);
            const int r = perm[i];
            int n = 0;
            for (int p = rp[r]; p < rp[r + 1]; ++p) if (ci[p] != r) dst[n++] = inv[ci[p]];
            std::sort(dst, dst + n);
            if (n) { cmin = std::min(cmin, dst[0]); cmax = std::max(cmax, dst[n - 1]); }
            for (; n < width; ++n) dst[n] = i;
        }
        blk[b].x = cmin; blk[b].y = cmax - cmin + 1;
        maxwin = std::max(maxwin, blk[b].y); winsum += blk[b].y;
    }
    if (maxwin > KB_MAXWIN) return nullptr;
    return kblocked_upload(new KBlocked{m, R, nb, (int)total, maxwin, maxints, winsum, nullptr, nullptr, nullptr}, perm.data(), pcol.data(), blk.data(), nullptr);
}
void kblocked_free(KBlocked *kb)
{
    if (!kb) return;
    if (kb->perm) (void)hipFree(kb->perm);
    if (kb->pcol) (void)hipFree(kb->pcol);
    if (kb->blk) (void)hipFree(kb->blk);
    if (kb->seg) (void)hipFree(kb->seg);
    delete kb;
}

// Builds the windowed blocked form of a K pattern above KB_MAXROWS rows (kbw_plan.h; host side, once per pattern; nullptr when a row has more
// than 64 off-diagonal entries or no block size gives windows within KB_MAXWIN doubles and g_kbw_segcap segments: the solve then uses the CSR
// positions).  x, y, z: device pointers to the coordinates of the pattern's rows.
static int g_kbw_segcap = KBW_MAXSEG;       // dkmc_debug_kbw_segment_cap (test aid)
extern "C" void dkmc_debug_kbw_segment_cap(int cap) { g_kbw_segcap = (cap < 1 || cap > KBW_MAXSEG) ? KBW_MAXSEG : cap; }
extern "C" int dkmc_debug_kbw_halfword_pos(int width, int entry) { return kbw_halfword_pos(width, entry); }
static KBlocked *kbw_build(const int *rp_d, const int *ci_d, int m, int nnz, const double *x_d, const double *y_d, const double *z_d, hipStream_t st)
{
    KPattern H;
    if (!kpattern_download(H, rp_d, ci_d, m, nnz, x_d, y_d, z_d, st)) return nullptr;
    int dev = 0, ncu = 0;
    if (hipGetDevice(&dev) != hipSuccess || hipDeviceGetAttribute(&ncu, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess || ncu < 1) ncu = 256;
    KbwPlan P;
    if (kbw_plan(m, H.rp.data(), H.ci.data(), H.x.data(), H.y.data(), H.z.data(), ncu, KB_MAXWIN, g_kbw_segcap, KC_NPA, P) || P.R < KC_NT / 16) return nullptr;
    KBlocked *kb = new KBlocked{m, P.R, P.nb, P.total, P.maxwin, P.maxints, P.winsum, nullptr, nullptr, nullptr};
    kb->form = 2; kb->maxseg = P.maxseg; kb->segsum = P.segsum; kb->word_bytes = eng().k_window_word_bytes == 2 ? 2 : 4;
    static_assert(sizeof(KbwI4) == sizeof(int4), "segment table layout");
    return kblocked_upload(kb, P.perm.data(), P.pcol.data(), P.blk.data(), P.seg.data());
}
// The form initialize_sparsity keeps for a K pattern: the windowed form above KB_MAXROWS rows when dkmc_set_k_blocked_large(1), else the
// blocked form (nullptr above KB_MAXROWS).
KBlocked *kpattern_form_build(const int *rp_d, const int *ci_d, int m, int nnz, const double *x_d, const double *y_d, const double *z_d, hipStream_t st)
{
    const Engine &e = eng();
    if (e.k_blocked && e.k_blocked_large && m > KB_MAXROWS && nnz >= 1) return kbw_build(rp_d, ci_d, m, nnz, x_d, y_d, z_d, st);
    return kblocked_build(rp_d, ci_d, m, nnz, x_d, st);
}

// ---- the one-GPU loop on an assembled system (kcg_run.h) -----------------------------------------------------------------------------------------
int kcg_run_setup(KcgRun &c, int m, const int *rp, int nnz, const KBlocked *kb, const int *cf, const double *diag, double *rhs, double *yb,
                  double w_high, double w_low, double tol, double *y_site)
{
    Engine &e = eng();
    if (kb && kb->m != m) return dkmc_fail(6, "K-CG: the blocked form belongs to another pattern", __FILE__, __LINE__);
    c = KcgRun{};
    c.m = m; c.nnz = nnz; c.rp = rp; c.kb = kb; c.cf = cf; c.diag = diag; c.rhs = rhs; c.y_site = y_site; c.y = kb ? yb : y_site;
    c.w_high = w_high; c.w_low = w_low; c.tol2 = tol * tol;
    c.kbw = kb && kb->form == 2;
    c.kbw2 = c.kbw && kb->word_bytes == 2;           // 16-bit stored words (dkmc_set_k_window_word_bytes when the pattern was built)
    c.s = (double *)scratch(S_CG_S, (size_t)m * 8); c.r = (double *)scratch(S_CG_R, (size_t)m * 8);
    c.p = (double *)scratch(S_CG_P, (size_t)m * 8); c.t = (double *)scratch(S_CG_T, (size_t)m * 8);
    c.q = (double *)scratch(S_XT_Q, (size_t)m * 8);
    c.part = (double *)scratch(S_CG_PART, (size_t)KC_PART_DOUBLES * 8);
    c.ctrl = (KCtrl *)scratch(S_CG_CTRL, sizeof(KCtrl));
    if (!c.s || !c.r || !c.p || !c.t || !c.q || !c.part || !c.ctrl) return e.err_code;
    c.vb = (m + 255) / 256;
    c.lds = kb ? (size_t)kb->maxwin * 8 : 0;
    if (kb) {
        static bool lds_set[3] = {false, false, false};
        if (int rc = c.kbw2 ? kb_raise_lds_limit(k_kbw_apply<0, 2>, k_kbw_apply<1, 2>, &lds_set[2]) : c.kbw ? kb_raise_lds_limit(k_kbw_apply<0, 4>, k_kbw_apply<1, 4>, &lds_set[1])
                                                                                                            : kb_raise_lds_limit(k_kb_apply<0>, k_kb_apply<1>, &lds_set[0])) return rc;
    }
    c.ga = kb ? kb->nb : grid_blocks(m, KC_NT / 8, KC_NPA);         // product: one block of the blocked form, or 32 rows, per workgroup and pass
    c.gv = grid_blocks(m, KC_NT, KC_NP);
    c.npa = (c.ga + KC_NT - 1) / KC_NT * KC_NT;
    return 0;
}
#define KC_APPLY(MODE, ...) do { if (c.kbw2) hipLaunchKernelGGL((k_kbw_apply<MODE, 2>), dim3(c.ga), dim3(KB_NT), c.lds, st, c.m, c.kb->R, (const int4 *)c.kb->blk, (const int4 *)c.kb->seg, __VA_ARGS__); \
                                 else if (c.kbw) hipLaunchKernelGGL((k_kbw_apply<MODE, 4>), dim3(c.ga), dim3(KB_NT), c.lds, st, c.m, c.kb->R, (const int4 *)c.kb->blk, (const int4 *)c.kb->seg, __VA_ARGS__); \
                                 else if (c.kb) hipLaunchKernelGGL((k_kb_apply<MODE>), dim3(c.ga), dim3(KB_NT), c.lds, st, c.m, c.kb->R, (const int4 *)c.kb->blk, __VA_ARGS__); \
                                 else hipLaunchKernelGGL((k_kc_apply<MODE>), dim3(c.ga), dim3(KC_NT), 0, st, c.m, c.rp, __VA_ARGS__); } while (0)
int kcg_run_scale(KcgRun &c, KCtrl *ctrl_out)
{
    hipStream_t st = eng().stream;
    if (c.kb) hipLaunchKernelGGL(k_kb_scale, dim3(c.vb), dim3(256), 0, st, c.m, (const int *)c.kb->perm, c.diag, c.s, c.rhs, (const double *)c.y_site, c.y, c.q);
    else hipLaunchKernelGGL(k_kc_scale, dim3(c.vb), dim3(256), 0, st, c.m, c.diag, c.s, c.rhs, c.y, c.q);
    HIPCHK(hipMemsetAsync(ctrl_out, 0, sizeof(KCtrl), st));
    HIPCHK(hipMemsetAsync(c.part, 0, (size_t)KC_PART_DOUBLES * 8, st));       // the slots beyond either grid stay zero
    return 0;
}
int kcg_run_start(KcgRun &c, KCtrl *ctrl_out)
{
    hipStream_t st = eng().stream;
    KC_APPLY(1, c.cf, c.diag, (const double *)c.s, (const double *)c.q, c.w_high, c.w_low,
             (const double *)nullptr, c.t, c.part, (const KCtrl *)c.ctrl, (const double *)c.rhs, c.r, c.p);
    hipLaunchKernelGGL(k_kc_q, dim3(c.vb), dim3(256), 0, st, c.m, (const double *)c.s, (const double *)c.p, c.q);
    hipLaunchKernelGGL(k_kc_check0, dim3(1), dim3(KC_NT), 0, st, c.part, ctrl_out, c.tol2);
    KCHK();
    return 0;
}
// the product of an iteration: t = S K q and the block partials of p.t, r.t and t.t, on the form c holds
static void kcg_run_product(KcgRun &c, hipStream_t st)
{
    KC_APPLY(0, c.cf, c.diag, (const double *)c.s, (const double *)c.q, c.w_high, c.w_low,
             (const double *)c.p, c.t, c.part, (const KCtrl *)c.ctrl, (const double *)nullptr, c.r, (double *)nullptr);
}
int kcg_run_iterate(KcgRun &c, int it)
{
    hipStream_t st = eng().stream;
    kcg_run_product(c, st);
    if (c.kb && !c.kbw) hipLaunchKernelGGL(k_kc_step, dim3(c.gv), dim3(KC_NT), 0, st, c.m, it, c.part, c.p, (const double *)c.t, c.y, c.r, (const double *)c.s, c.q, c.ctrl, c.tol2, c.npa);
    else {
        hipLaunchKernelGGL(k_kc_update, dim3(c.gv), dim3(KC_NT), 0, st, c.m, it, (const double *)c.part, c.npa, (const double *)c.p, (const double *)c.t, c.y, c.r, c.part + 3 * KC_NPA, (const KCtrl *)c.ctrl);
        hipLaunchKernelGGL(k_kc_direction, dim3(c.gv), dim3(KC_NT), 0, st, c.m, it, (const double *)(c.part + 3 * KC_NPA), (const double *)c.r, c.p, (const double *)c.s, c.q, c.ctrl, c.tol2);
    }
    return 0;
}
#undef KC_APPLY
int kcg_run_poll(KcgRun &c, KCtrl &h, int first)
{
    return cg_poll_loop(c.ctrl, h, LaunchPlan::doubling(8), eng().stream, "CG: no convergence after 200000 iterations", nullptr,
                        [&](int it, const hipEvent_t *) -> int { return kcg_run_iterate(c, it); }, 0, first, &c.syncs);
}
int kcg_run_unscale(KcgRun &c)
{
    hipStream_t st = eng().stream;
    if (c.kb) hipLaunchKernelGGL(k_kb_unscale, dim3(c.vb), dim3(256), 0, st, c.m, (const int *)c.kb->perm, (const double *)c.y, (const double *)c.s, c.y_site);
    else hipLaunchKernelGGL(k_kc_unscale, dim3(c.vb), dim3(256), 0, st, c.m, c.y, (const double *)c.s);
    KCHK();
    return 0;
}
long long kcg_run_bytes(const KcgRun &c)
{
    const KBlocked *kb = c.kb; const long long m = c.m;
    if (c.kbw) return (c.kbw2 ? 2LL : 4LL) * kb->total + 16LL * kb->nb * (1 + KBW_MAXSEG) + 8LL * kb->winsum + 16LL * 8 * m;       // (product 5 + update 6 + direction 5 vector touches)
    return kb ? 4LL * kb->total + 16LL * kb->nb + 8LL * kb->winsum + 14LL * 8 * m : 4LL * c.nnz + 4LL * (m + 1) + 17LL * 8 * m;
}
int kcg_run(KcgRun &c, KCtrl &h, int first)
{
    Engine &e = eng(); hipStream_t st = e.stream;
    if (int rc = kcg_run_scale(c, c.ctrl)) return rc;
    static hipEvent_t evk[2]; static bool evk_ready = false;
    const bool prof = e.profiling != 0;
    if (prof && !evk_ready) { HIPCHK(hipEventCreate(&evk[0])); HIPCHK(hipEventCreate(&evk[1])); evk_ready = true; }
    if (int rc = kcg_run_start(c, c.ctrl)) return rc;
    if (prof) HIPCHK(hipEventRecord(evk[0], st));
    if (int rc = kcg_run_poll(c, h, first)) return rc;
    if (prof) {
        HIPCHK(hipEventRecord(evk[1], st));
        HIPCHK(hipEventSynchronize(evk[1]));
        float ms = 0.f;
        HIPCHK(hipEventElapsedTime(&ms, evk[0], evk[1]));
        c.ms = ms; c.iters_timed = h.iters;
    } else { c.ms = 0.0; c.iters_timed = 0; }
    return kcg_run_unscale(c);
}

// Diagonal, right-hand side and stored words of K for the current elements / charges, in the layout of the form kb holds (null: CSR positions).
static void kcg_assemble(int cb, int m, int N_left, const int *element, const int *charge, MetalSet ms, double high_G, double low_G,
                         const int *rp, const int *ci, const int *lrp, const int *lci, const int *rrp, const int *rci,
                         double VL, double VR, const KBlocked *kb, int *cf, double *diag, double *rhs)
{
    hipStream_t st = eng().stream;
    const bool kbw = kb && kb->form == 2, kbw2 = kbw && kb->word_bytes == 2;
    const int ab = (m + 15) / 16;
    kc_with_cb(cb, [&](auto cbv) {
        constexpr int CB = decltype(cbv)::value;
        if (kbw2) hipLaunchKernelGGL((k_kbw_assemble<CB, 2>), dim3(ab), dim3(KC_NT), 0, st, m, N_left, kb->R, kb->nb, (const int4 *)kb->blk, (const int4 *)kb->seg, (const int *)kb->perm,
                                     (const int *)kb->pcol, element, charge, ms, high_G, low_G, lrp, lci, rrp, rci, VL, VR, cf, diag, rhs);
        else if (kbw) hipLaunchKernelGGL((k_kbw_assemble<CB, 4>), dim3(ab), dim3(KC_NT), 0, st, m, N_left, kb->R, kb->nb, (const int4 *)kb->blk, (const int4 *)kb->seg, (const int *)kb->perm,
                                         (const int *)kb->pcol, element, charge, ms, high_G, low_G, lrp, lci, rrp, rci, VL, VR, cf, diag, rhs);
        else if (kb) hipLaunchKernelGGL((k_kb_assemble<CB>), dim3(ab), dim3(KC_NT), 0, st, m, N_left, kb->R, (const int4 *)kb->blk, (const int *)kb->perm, (const int *)kb->pcol,
                                        element, charge, ms, high_G, low_G, lrp, lci, rrp, rci, VL, VR, cf, diag, rhs);
        else hipLaunchKernelGGL((k_kc_assemble<CB>), dim3(ab), dim3(KC_NT), 0, st, m, N_left, element, charge, ms, high_G, low_G, rp, ci, lrp, lci, rrp, rci, VL, VR, cf, diag, rhs);
    });
}

// Assemble K for the current elements / charges and solve K y = rhs in place in y (warm start = y on entry).
// kb: the blocked form of the pattern (or nullptr): the whole solve then runs in the blocked order, y is gathered on entry and scattered on exit.
static int kcg_slab_loop(int m, const int *rp, const int *cf, const double *diag, const double *s, const double *b, double high_G, double low_G, double *y, double *q0,
                         const double *coord_y, const double *coord_z, int nr, int me0, bool emu, int time_rank, double tol2, int *iters_out, double *rr_out);
// row_y / row_z: lateral coordinates of the rows (site_y + N_left, site_z + N_left) for the slab-distributed loop; may be null.
// emu_nr > 0 (dkmc_kcg_emulate_slabs): run the slab-distributed loop with emu_nr virtual ranks in this process.
int kcg_assemble_and_solve(int cb, int m, int N_left, const int *element, const int *charge, MetalSet ms, double high_G, double low_G,
                           const int *rp, const int *ci, int nnz, const int *lrp, const int *lci, const int *rrp, const int *rci,
                           double VL, double VR, double *y_site, int *iters_out, double *rr_out, const KBlocked *kb,
                           const double *row_y, const double *row_z, int emu_nr, int emu_time_rank)
{
    Engine &e = eng(); hipStream_t st = e.stream;
    if (m <= 0) { if (iters_out) *iters_out = 0; if (rr_out) *rr_out = 0; return 0; }
    if (kb && kb->m != m) return dkmc_fail(6, "K-CG: the blocked form belongs to another pattern", __FILE__, __LINE__);
    // the windowed form runs on one GPU only: more than one rank (or the emulation of it) keeps the slab-distributed loop on the CSR positions
    if (kb && kb->form == 2 && row_y && row_z && (emu_nr > 0 || (e.k_slab && comm_attached() && comm_nranks() > 1 && comm_nranks() <= XS_MAXR))) kb = nullptr;
    const bool kbw = kb && kb->form == 2;
    const bool kbw2 = kbw && kb->word_bytes == 2;           // 16-bit stored words (dkmc_set_k_window_word_bytes when the pattern was built)
    int *cf = (int *)scratch(S_K_DATA, kb ? (size_t)kb->total * (kbw2 ? 2 : 4) : (size_t)nnz * 4);
    double *rhs = (double *)scratch(S_K_RHS, (size_t)m * 8 * 3);
    if (!cf || !rhs) return e.err_code;
    double *diag = rhs + m;
    KcgRun c;
    if (int rc = kcg_run_setup(c, m, rp, nnz, kb, cf, diag, rhs, rhs + 2 * (size_t)m, high_G, low_G, e.cg_tol, y_site)) return rc;
    kcg_assemble(cb, m, N_left, element, charge, ms, high_G, low_G, rp, ci, lrp, lci, rrp, rci, VL, VR, kb, cf, diag, rhs);
    // more than one rank (or the emulation of it) on a system above the size of the blocked form: the loop distributed by row slabs
    const bool slab = !kb && row_y && row_z && (emu_nr > 0 || (e.k_slab && comm_attached() && comm_nranks() > 1 && comm_nranks() <= XS_MAXR));
    if (slab) {
        if (int rc = kcg_run_scale(c, c.ctrl)) return rc;
        int rcs = 0;
        if (emu_nr <= 0) rcs = comm_agree(e.err_code, "assembly of K");                 // local set-up done: nobody enters the collectives of the loop alone
        if (rcs) return rcs;
        rcs = kcg_slab_loop(m, rp, cf, diag, c.s, rhs, high_G, low_G, c.y, c.q, row_y, row_z, emu_nr > 0 ? emu_nr : comm_nranks(), emu_nr > 0 ? 0 : comm_rank(), emu_nr > 0,
                            emu_time_rank, c.tol2, iters_out, rr_out);
        if (rcs) return rcs;
        hipLaunchKernelGGL(k_kc_unscale, dim3(c.vb), dim3(256), 0, st, m, c.y, (const double *)c.s);
        KCHK();
        e.stats.kcg_blocked = 0; e.stats.kcg_ms = 0.0; e.stats.kcg_iters_timed = 0;
        e.stats.kcg_bytes = 4LL * nnz + 4LL * (m + 1) + 17LL * 8 * m;
        return e.err_code;
    }
    KCtrl h{};
    if (int rc = kcg_run(c, h, 0)) return rc;
    e.stats.kcg_ms = c.ms; e.stats.kcg_iters_timed = c.iters_timed;
    e.stats.kcg_blocked = kb ? kb->form : 0;
    e.stats.kcg_bytes = kcg_run_bytes(c);
    if (iters_out) *iters_out = h.iters;
    if (rr_out) *rr_out = kb && !kbw ? h.rr[0] : h.rr[h.iters & 1];
    return e.err_code;
}

// Test aid (dkmc_debug_k_system): K assembled as above on the form kb holds (null: CSR positions; the windowed form is refused), its diagonal and
// right-hand side in the pattern's row order, and t = K v from ONE launch of the form's product kernel with s = 1, q = v and a cleared stop
// word.  v, t, diag_out, rhs_out: host arrays of m doubles in the pattern's row order (the blocked order is entered and left through perm, on the
// host).  Writes only scratch that every solve rewrites before it reads it.
int kcg_debug_system(int cb, int m, int N_left, const int *element, const int *charge, MetalSet ms, double high_G, double low_G,
                     const int *rp, const int *ci, int nnz, const int *lrp, const int *lci, const int *rrp, const int *rci,
                     double VL, double VR, const KBlocked *kb, const double *v, double *t, double *diag_out, double *rhs_out)
{
    Engine &e = eng(); hipStream_t st = e.stream;
    if (m <= 0 || !v || !t || !diag_out || !rhs_out) return dkmc_fail(13, "debug_k_system: bad arguments", __FILE__, __LINE__);
    if (kb && kb->m != m) return dkmc_fail(6, "K-CG: the blocked form belongs to another pattern", __FILE__, __LINE__);
    if (kb && kb->form == 2) return dkmc_fail(13, "debug_k_system: not for the windowed blocked form", __FILE__, __LINE__);
    int *cf = (int *)scratch(S_K_DATA, kb ? (size_t)kb->total * 4 : (size_t)nnz * 4);
    double *rhs = (double *)scratch(S_K_RHS, (size_t)m * 8 * 3);
    if (!cf || !rhs) return e.err_code;
    double *diag = rhs + m;
    KcgRun c;
    if (int rc = kcg_run_setup(c, m, rp, nnz, kb, cf, diag, rhs, rhs + 2 * (size_t)m, high_G, low_G, e.cg_tol, nullptr)) return rc;
    kcg_assemble(cb, m, N_left, element, charge, ms, high_G, low_G, rp, ci, lrp, lci, rrp, rci, VL, VR, kb, cf, diag, rhs);
    std::vector<int> perm((size_t)m);
    if (kb) HIPCHK(hipMemcpyAsync(perm.data(), kb->perm, (size_t)m * 4, hipMemcpyDeviceToHost, st));
    else for (int i = 0; i < m; ++i) perm[i] = i;
    std::vector<double> h((size_t)m), ones((size_t)m, 1.0);
    HIPCHK(hipStreamSynchronize(st));
    for (int i = 0; i < m; ++i) h[i] = v[perm[i]];
    HIPCHK(hipMemcpyAsync(c.q, h.data(), (size_t)m * 8, hipMemcpyHostToDevice, st));
    HIPCHK(hipMemcpyAsync(c.s, ones.data(), (size_t)m * 8, hipMemcpyHostToDevice, st));
    HIPCHK(hipMemsetAsync(c.p, 0, (size_t)m * 8, st));
    HIPCHK(hipMemsetAsync(c.r, 0, (size_t)m * 8, st));
    HIPCHK(hipMemsetAsync(c.t, 0xff, (size_t)m * 8, st));            // a row no pass writes comes back as NaN
    HIPCHK(hipMemsetAsync(c.ctrl, 0, sizeof(KCtrl), st));
    HIPCHK(hipStreamSynchronize(st));                                // (h is refilled below)
    kcg_run_product(c, st);
    KCHK();
    const double *src[3] = {c.t, diag, rhs}; double *dst[3] = {t, diag_out, rhs_out};
    for (int k = 0; k < 3; ++k) {
        HIPCHK(hipMemcpyAsync(h.data(), src[k], (size_t)m * 8, hipMemcpyDeviceToHost, st));
        HIPCHK(hipStreamSynchronize(st));
        for (int i = 0; i < m; ++i) dst[k][perm[i]] = h[i];
    }
    return e.err_code;
}


// ---- slab-distributed CG on K (SURVEY 8(e), row "K-CG": row slabs, halo = sites within the neighbour distance of a cut, the dot products completed
// across the ranks) -- configs[4]'s "domain-decomposed potential".  No counterpart in the reference (single GPU).  For systems above the size of
// the blocked form, when a communicator with more than one rank is attached (dkmc_set_k_slab, default on).  A rank OWNS the rows of one lateral
// slab (slab.h): product, update and direction run over its row list only; per iteration, in the reference's order (product, update, direction:
// beta from the direct sum r'.r', see k_kc_update):
//   product (own rows)    t = S K q, block partials of p.t          -> exchange 1: all-gather of the partials; every rank adds ALL of them in one
//   update (own rows)     alpha, y, r, block partials of r'.r'      -> exchange 2: the same                      fixed order: identical alpha, beta
//   direction (own rows)  beta, p, q = S p, stop test               -> exchange 3: all-to-all-v of the q entries a neighbour slab reads (halo)
// -- identical scalars on every rank by construction, so all ranks stop at the same iteration and no flag has to travel.  Vectors keep their full
// length on every rank (29 MB each at 3.6e6 rows); entries a rank neither owns nor reads are never touched.  The solution's own rows are
// all-gathered once at the end.  The same host loop runs N VIRTUAL ranks in one process (dkmc_kcg_emulate_slabs): how it is tested on one GPU.
// (the block partials per rank are KC_NPA / KC_NP as on one GPU -- k_kc_apply stores at KC_NPA strides --: 16 KB per rank in exchange 1, 4 KB in exchange 2)
__global__ __launch_bounds__(KC_NT) void k_ks_check0(int n, const double *__restrict__ xa, KCtrl *ctrl, double tol2) { kc_check0<true>(n, xa, nullptr, ctrl, tol2); }
__global__ __launch_bounds__(KC_NT) void k_ks_update(int n, const int *__restrict__ rows, int it, const double *__restrict__ xa, int na, const double *__restrict__ p,
                                                     const double *__restrict__ t, double *__restrict__ y, double *__restrict__ r, double *__restrict__ xb_mine, const KCtrl *ctrl)
{ kc_update<true>(n, rows, it, xa, na, p, t, y, r, xb_mine, ctrl); }
__global__ __launch_bounds__(KC_NT) void k_ks_direction(int n, const int *__restrict__ rows, int it, const double *__restrict__ xb, int nb, const double *__restrict__ r,
                                                        double *__restrict__ p, const double *__restrict__ s, double *__restrict__ q, KCtrl *ctrl, double tol2)
{ kc_direction<true>(n, rows, it, xb, nb, r, p, s, q, ctrl, tol2); }
__global__ void k_ks_q(int n, const int *__restrict__ rows, const double *__restrict__ s, const double *__restrict__ p, double *__restrict__ q) { kc_q<true>(n, rows, s, p, q); }
__global__ void k_ks_gather(int n, const int *__restrict__ list, const double *__restrict__ v, double *__restrict__ out)
{
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) out[i] = v[list[i]];
}
__global__ void k_ks_scatter(int n, const int *__restrict__ list, const double *__restrict__ in, double *__restrict__ v)
{
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) v[list[i]] = in[i];
}
// the solution: block r of the gathered buffer (stride doubles apart) holds the rows of owner r in list order
__global__ void k_ks_scatter_all(int nr, int me, int stride, const int *__restrict__ rows_by_owner, const int *__restrict__ rowoff, const double *__restrict__ in, double *__restrict__ y)
{
    const int r = blockIdx.y;
    if (r == me) return;
    const int n = rowoff[r + 1] - rowoff[r];
    for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < n; i += gridDim.x * blockDim.x) y[rows_by_owner[rowoff[r] + i]] = in[(size_t)r * stride + i];
}

struct KsRank { int v = 0, n_own = 0, nhs = 0, nhr = 0; int *own = nullptr, *hsend = nullptr, *hrecv = nullptr; double *y = nullptr, *r = nullptr, *p = nullptr, *t = nullptr, *q = nullptr,
                *xa = nullptr, *xb = nullptr, *send = nullptr, *recv = nullptr, *ybuf = nullptr; KCtrl *ctrl = nullptr; };
static double g_ks_times[4] = {0, 0, 0, 0};       // emulation: mean kernel times of the timed virtual rank (product, update, direction, halo pack + unpack)
static long long g_ks_halo[2] = {0, 0};           // doubles a rank receives per iteration in exchange 3 (largest over the ranks); rows of the largest slab
static int g_ks_iter_cap = 0;

// cf / diag / s / b: the assembled, scaled system (replicated); y: scaled start vector in, scaled solution out (all rows, every rank).
// emu: nr virtual ranks in this process, exchanges as device copies.  coord_y / coord_z: lateral coordinates of the rows.
static int kcg_slab_loop(int m, const int *rp, const int *cf, const double *diag, const double *s, const double *b, double high_G, double low_G, double *y, double *q0,
                         const double *coord_y, const double *coord_z, int nr, int me0, bool emu, int time_rank, double tol2, int *iters_out, double *rr_out)
{
    Engine &e = eng(); hipStream_t st = e.stream;
    const int nv = emu ? nr : 1;
    SlabArena arena{st, "K-CG slab emulation: out of device memory"};
    if (nr < 1 || nr > XS_MAXR) return dkmc_fail(43, "slab-distributed K-CG: 1 ... 32 ranks", __FILE__, __LINE__);
    // ---- ownership (slab.h): slabs along the wider lateral axis, balanced by row count ----
    void *itab = scratch(S_KS_TAB, slab_tab_bytes());
    void *owner = scratch(S_KS_OWNER, slab_owner_bytes(m));
    int *rows_by_owner = (int *)scratch(S_KS_LISTS, ((size_t)m + XS_MAXR + 8) * 4);
    void *flag = scratch(S_KS_FLAG, slab_flag_bytes(m));
    double *mm = (double *)scratch(S_KS_BOX, 64);
    if (!itab || !owner || !rows_by_owner || !flag || !mm) return e.err_code;
    const SlabWork W = slab_work(itab, owner, flag, m);
    int *rowoff_d = rows_by_owner + m;
    // extent of the two lateral coordinates (host: one pass over 2 x m doubles per solve would cost more than it saves to do on the device -- the
    // extents are those of the site arrays and do not change: cached per coordinate pointer)
    static const double *ext_key = nullptr; static int ext_m = 0; static double ext[4];
    if (ext_key != coord_y || ext_m != m) {
        std::vector<double> hy((size_t)m), hz((size_t)m);
        HIPCHK(hipMemcpyAsync(hy.data(), coord_y, (size_t)m * 8, hipMemcpyDeviceToHost, st));
        HIPCHK(hipMemcpyAsync(hz.data(), coord_z, (size_t)m * 8, hipMemcpyDeviceToHost, st));
        HIPCHK(hipStreamSynchronize(st));
        ext[0] = *std::min_element(hy.begin(), hy.end()); ext[1] = *std::max_element(hy.begin(), hy.end());
        ext[2] = *std::min_element(hz.begin(), hz.end()); ext[3] = *std::max_element(hz.begin(), hz.end());
        ext_key = coord_y; ext_m = m;
    }
    const bool use_z = ext[3] - ext[2] > ext[1] - ext[0];
    const double *coord = use_z ? coord_z : coord_y;
    const double lo = use_z ? ext[2] : ext[0], hi = use_z ? ext[3] : ext[1];
    if (int rc = slab_partition(st, m, 0, rp, cf, coord, lo, hi, nr, (const int *)nullptr, W)) return rc;
    std::vector<int> htab;
    if (int rc = slab_download_tab(st, W, nr, htab)) return rc;
    const SlabPlan P(htab.data(), nr);
    const int *rowoff = P.rowoff, maxown = std::max(1, P.maxown);
    if (!P.covers(m, 0)) return dkmc_fail(13, "slab-distributed K-CG: the slabs do not cover the rows", __FILE__, __LINE__);
    HIPCHK(hipMemcpyAsync(rowoff_d, rowoff, (size_t)(nr + 1) * 4, hipMemcpyHostToDevice, st));
    for (int r = 0; r < nr; ++r) if (int rc = slab_rows_of_owner(st, m, 0, W, P, r, rows_by_owner)) return rc;
    std::vector<long long> cnt3((size_t)nr * nr);
    for (int a = 0; a < nr; ++a) for (int d = 0; d < nr; ++d) cnt3[(size_t)a * nr + d] = a == d ? 0 : P.hal(a, d);
    g_ks_halo[0] = slab_recv_max(cnt3.data(), nr); g_ks_halo[1] = maxown;
    // ---- per (virtual) rank: lists, vectors, exchange buffers ----
    std::vector<KsRank> RK((size_t)nv);
    for (int iv = 0; iv < nv; ++iv) {
        KsRank &K = RK[iv]; const int v = emu ? iv : me0; K.v = v; K.n_own = P.nown()[v];
        const SlabHalo H(P, v);
        K.nhs = H.hsoff[nr]; K.nhr = H.hroff[nr];
        int *li = (int *)arena.get(iv, S_KS_RLISTS, ((size_t)K.nhs + K.nhr + 8) * 4);
        double *vec = iv == 0 ? nullptr : (double *)arena.get(iv, 0, (size_t)m * 8 * 5);
        K.xa = (double *)arena.get(iv, S_KS_XA, (size_t)nr * KC_NPA * 8); K.xb = (double *)arena.get(iv, S_KS_XB, (size_t)nr * KC_NP * 8);
        K.send = (double *)arena.get(iv, S_KS_SEND, (size_t)(K.nhs + 8) * 8); K.recv = (double *)arena.get(iv, S_KS_RECV, (size_t)(K.nhr + 8) * 8);
        K.ybuf = (double *)arena.get(iv, S_KS_YBUF, (size_t)nr * maxown * 8);
        K.ctrl = iv == 0 ? (KCtrl *)scratch(S_CG_CTRL, sizeof(KCtrl)) : (KCtrl *)arena.get(iv, 0, sizeof(KCtrl));
        if (iv == 0) {
            K.y = y; K.q = q0;
            K.r = (double *)scratch(S_CG_R, (size_t)m * 8); K.p = (double *)scratch(S_CG_P, (size_t)m * 8); K.t = (double *)scratch(S_CG_T, (size_t)m * 8);
            if (!K.r || !K.p || !K.t) return e.err_code;
        } else if (vec) {
            K.y = vec; K.r = vec + m; K.p = vec + 2 * (size_t)m; K.t = vec + 3 * (size_t)m; K.q = vec + 4 * (size_t)m;
            HIPCHK(hipMemcpyAsync(K.y, y, (size_t)m * 8, hipMemcpyDeviceToDevice, st));
            HIPCHK(hipMemcpyAsync(K.q, q0, (size_t)m * 8, hipMemcpyDeviceToDevice, st));
        }
        if (arena.fail || !K.ctrl) return arena.fail ? arena.fail : e.err_code;
        K.own = rows_by_owner + rowoff[v]; K.hsend = li; K.hrecv = li + K.nhs;
        if (int rc = slab_halo_lists(st, W, P, H, v, rows_by_owner, K.hsend, K.hrecv)) return rc;
        HIPCHK(hipMemsetAsync(K.ctrl, 0, sizeof(KCtrl), st));
        HIPCHK(hipMemsetAsync(K.xa, 0, (size_t)nr * KC_NPA * 8, st));
        HIPCHK(hipMemsetAsync(K.xb, 0, (size_t)nr * KC_NP * 8, st));
    }
    KCHK();
    // ---- exchanges ----
    auto xchg = [&](int which) -> int {          // 1: product partials, 2: r.r partials (all-gathers); 3: halo of q (all-to-all-v); 4: the solution's own rows (all-gather)
        if (!emu) {
            KsRank &K = RK[0];
            if (which == 1) return comm_allgather_f64(K.xa, (size_t)KC_NPA);
            if (which == 2) return comm_allgather_f64(K.xb, (size_t)KC_NP);
            if (which == 3) return comm_alltoallv_f64(K.send, K.recv, cnt3.data());
            return comm_allgather_f64(K.ybuf, (size_t)maxown);
        }
        if (which == 1) return slab_emu_allgather(st, nr, (size_t)KC_NPA, [&](int r) { return RK[r].xa; });
        if (which == 2) return slab_emu_allgather(st, nr, (size_t)KC_NP, [&](int r) { return RK[r].xb; });
        if (which == 3) return slab_emu_alltoallv(st, nr, cnt3.data(), [&](int r) { return RK[r].send; }, [&](int r) { return RK[r].recv; });
        return slab_emu_allgather(st, nr, (size_t)maxown, [&](int r) { return RK[r].ybuf; });
    };
    const bool timing = emu && time_rank >= 0 && time_rank < nr;
    SlabTimer timer{st};
    if (timing) if (int rc = timer.create()) return rc;
    double tsum[4] = {0, 0, 0, 0}; int tcount = 0;
    auto timed = [&](int iv, int cls, bool on, const std::function<void()> &launch) -> int {
        float ms = 0.f;
        if (int rc = timer.run(timing && on && RK[iv].v == time_rank, launch, &ms)) return rc;
        tsum[cls] += ms;
        return 0;
    };
    auto halo = [&](bool on) -> int {
        if (nr == 1) return 0;
        for (int iv = 0; iv < nv; ++iv) { KsRank &K = RK[iv]; if (K.nhs > 0) { int rc = timed(iv, 3, on, [&]() { hipLaunchKernelGGL(k_ks_gather, dim3((K.nhs + 255) / 256), dim3(256), 0, st, K.nhs, (const int *)K.hsend, (const double *)K.q, K.send); }); if (rc) return rc; } }
        if (int rcx = xchg(3)) return rcx;
        for (int iv = 0; iv < nv; ++iv) { KsRank &K = RK[iv]; if (K.nhr > 0) { int rc = timed(iv, 3, on, [&]() { hipLaunchKernelGGL(k_ks_scatter, dim3((K.nhr + 255) / 256), dim3(256), 0, st, K.nhr, (const int *)K.hrecv, (const double *)K.recv, K.q); }); if (rc) return rc; } }
        return 0;
    };
    // ---- r = A y - b, p = -r, q = S p ----
    for (int iv = 0; iv < nv; ++iv) {
        KsRank &K = RK[iv];
        const int ga = grid_blocks(K.n_own, KC_NT / 8, KC_NPA);
        if (K.n_own > 0) {
            hipLaunchKernelGGL((k_kc_apply<1>), dim3(ga), dim3(KC_NT), 0, st, K.n_own, rp, cf, diag, s, (const double *)K.q, high_G, low_G, (const double *)nullptr, K.t,
                               K.xa + (size_t)K.v * KC_NPA, (const KCtrl *)K.ctrl, b, K.r, K.p, (const int *)K.own);
            hipLaunchKernelGGL(k_ks_q, dim3((K.n_own + 255) / 256), dim3(256), 0, st, K.n_own, (const int *)K.own, s, (const double *)K.p, K.q);
        }
    }
    if (int rcx = xchg(1)) return rcx;
    for (int iv = 0; iv < nv; ++iv) hipLaunchKernelGGL(k_ks_check0, dim3(1), dim3(KC_NT), 0, st, nr * KC_NPA, (const double *)RK[iv].xa, RK[iv].ctrl, tol2);
    if (int rcx = halo(false)) return rcx;
    KCHK();
    KCtrl h{};
    if (int rc = cg_poll_loop(RK[0].ctrl, h, LaunchPlan::doubling(8), st, "CG: no convergence after 200000 iterations", nullptr, [&](int it, const hipEvent_t *) -> int {
        const bool on = timing && it >= 2 && tcount < 24;
        for (int iv = 0; iv < nv; ++iv) {
            KsRank &K = RK[iv];
            if (K.n_own <= 0) continue;
            int rc = timed(iv, 0, on, [&]() {
                hipLaunchKernelGGL((k_kc_apply<2>), dim3(grid_blocks(K.n_own, KC_NT / 8, KC_NPA)), dim3(KC_NT), 0, st, K.n_own, rp, cf, diag, s, (const double *)K.q, high_G, low_G,
                                   (const double *)K.p, K.t, K.xa + (size_t)K.v * KC_NPA, (const KCtrl *)K.ctrl, (const double *)nullptr, K.r, (double *)nullptr, (const int *)K.own);
            }); if (rc) return rc;
        }
        if (int rcx = xchg(1)) return rcx;
        for (int iv = 0; iv < nv; ++iv) {
            KsRank &K = RK[iv];
            int rc = timed(iv, 1, on, [&]() {
                hipLaunchKernelGGL(k_ks_update, dim3(grid_blocks(std::max(K.n_own, 1), KC_NT, KC_NP)), dim3(KC_NT), 0, st, K.n_own, (const int *)K.own, it, (const double *)K.xa, nr * KC_NPA,
                                   (const double *)K.p, (const double *)K.t, K.y, K.r, K.xb + (size_t)K.v * KC_NP, (const KCtrl *)K.ctrl);
            }); if (rc) return rc;
        }
        if (int rcx = xchg(2)) return rcx;
        for (int iv = 0; iv < nv; ++iv) {
            KsRank &K = RK[iv];
            int rc = timed(iv, 2, on, [&]() {
                hipLaunchKernelGGL(k_ks_direction, dim3(grid_blocks(std::max(K.n_own, 1), KC_NT, KC_NP)), dim3(KC_NT), 0, st, K.n_own, (const int *)K.own, it, (const double *)K.xb, nr * KC_NP,
                                   (const double *)K.r, K.p, s, K.q, K.ctrl, tol2);
            }); if (rc) return rc;
        }
        if (int rcx = halo(on)) return rcx;
        if (on) ++tcount;
        return 0;
    }, emu ? g_ks_iter_cap : 0)) return rc;
    if (e.err_code) return e.err_code;
    if (emu) {
        for (int iv = 1; iv < nv; ++iv) {
            KCtrl hv{};
            HIPCHK(hipMemcpy(&hv, RK[iv].ctrl, sizeof(KCtrl), hipMemcpyDeviceToHost));
            if (hv.iters != h.iters || hv.done != h.done || memcmp(hv.rr, h.rr, sizeof(h.rr)) != 0) return dkmc_fail(13, "K-CG slab emulation: the virtual ranks disagree on the iteration or on r.r", __FILE__, __LINE__);
        }
    }
    // ---- the solution on every rank ----
    if (nr > 1) {
        for (int iv = 0; iv < nv; ++iv) { KsRank &K = RK[iv]; if (K.n_own > 0) hipLaunchKernelGGL(k_ks_gather, dim3((K.n_own + 255) / 256), dim3(256), 0, st, K.n_own, (const int *)K.own, (const double *)K.y, K.ybuf + (size_t)K.v * maxown); }
        if (int rcx = xchg(4)) return rcx;
        for (int iv = 0; iv < nv; ++iv) { KsRank &K = RK[iv]; hipLaunchKernelGGL(k_ks_scatter_all, dim3(std::min((maxown + 255) / 256, 256), nr), dim3(256), 0, st, nr, K.v, maxown, (const int *)rows_by_owner, (const int *)rowoff_d, (const double *)K.ybuf, K.y); }
    }
    if (emu && nv > 1)
        if (int rc = slab_same_bits(st, nv, (size_t)m, [&](int iv) { return RK[iv].y; }, "K-CG slab emulation: the virtual ranks hold different solutions")) return rc;
    KCHK();
    HIPCHK(hipStreamSynchronize(st));
    if (timing) for (int c = 0; c < 4; ++c) g_ks_times[c] = tcount ? tsum[c] * 1e3 / tcount : 0.0;
    if (iters_out) *iters_out = h.iters;
    if (rr_out) *rr_out = h.rr[h.iters & 1];
    return e.err_code;
}

// doubles received per iteration in the halo exchange (largest over the ranks), rows of the largest slab, kernel times of the timed virtual rank
void kcg_slab_report(double *times_us, long long *halo_rows) { for (int c = 0; c < 4; ++c) if (times_us) times_us[c] = g_ks_times[c]; if (halo_rows) { halo_rows[0] = g_ks_halo[0]; halo_rows[1] = g_ks_halo[1]; } }
void kcg_slab_iter_cap(int cap) { g_ks_iter_cap = cap; }

// Test aid (devicekmc_hip_debug.h): slab.h's host functions as the two loops call them, on a caller-given pattern and on buffers of its own
extern "C" int dkmc_debug_slab_plan(int m, int first, const int *rp, const int *ci, const double *coord, double lo, double hi, int nr, const int *mark, int v,
                                    int *owner_out, unsigned *mask_out, int *tab_out, int *rows_by_owner_out, int *hsend_out, int *hrecv_out)
{
    Engine &e = eng(); hipStream_t st = e.stream;
    if (m < 1 || first < 0 || first >= m || !rp || !ci || !coord || nr < 1 || nr > XS_MAXR || v < 0 || v >= nr || !owner_out || !mask_out || !tab_out || !rows_by_owner_out)
        return dkmc_fail(13, "debug_slab_plan: bad arguments", __FILE__, __LINE__);
    for (int i = 0; i < m; ++i) if (rp[i] < 0 || rp[i + 1] < rp[i]) return dkmc_fail(13, "debug_slab_plan: bad row pointers", __FILE__, __LINE__);
    for (int p = 0; p < rp[m]; ++p) if ((ci[p] & 0x7fffffff) >= m) return dkmc_fail(13, "debug_slab_plan: column out of range", __FILE__, __LINE__);
    SlabArena arena{st, "debug_slab_plan: out of device memory"};
    const int nnz = rp[m], nd = m - first;
    int *d_rp = (int *)arena.get(1, 0, (size_t)(m + 1) * 4), *d_ci = (int *)arena.get(1, 0, (size_t)nnz * 4), *d_mark = mark ? (int *)arena.get(1, 0, (size_t)m * 4) : nullptr;
    double *d_coord = (double *)arena.get(1, 0, (size_t)nd * 8);
    int *rows_by_owner = (int *)arena.get(1, 0, (size_t)m * 4);
    const SlabWork W = slab_work(arena.get(1, 0, slab_tab_bytes()), arena.get(1, 0, slab_owner_bytes(m)), arena.get(1, 0, slab_flag_bytes(m)), m);
    if (arena.fail) return arena.fail;
    HIPCHK(hipMemcpyAsync(d_rp, rp, (size_t)(m + 1) * 4, hipMemcpyHostToDevice, st));
    HIPCHK(hipMemcpyAsync(d_ci, ci, (size_t)nnz * 4, hipMemcpyHostToDevice, st));
    HIPCHK(hipMemcpyAsync(d_coord, coord, (size_t)nd * 8, hipMemcpyHostToDevice, st));
    if (mark) HIPCHK(hipMemcpyAsync(d_mark, mark, (size_t)m * 4, hipMemcpyHostToDevice, st));
    if (int rc = slab_partition(st, m, first, (const int *)d_rp, (const int *)d_ci, (const double *)d_coord, lo, hi, nr, (const int *)d_mark, W)) return rc;
    std::vector<int> htab;
    if (int rc = slab_download_tab(st, W, nr, htab)) return rc;
    const SlabPlan P(htab.data(), nr);
    if (P.rowoff[nr] != nd) return dkmc_fail(13, "debug_slab_plan: the slabs do not cover the rows", __FILE__, __LINE__);
    for (int r = 0; r < nr; ++r) if (int rc = slab_rows_of_owner(st, m, first, W, P, r, rows_by_owner)) return rc;
    const SlabHalo H(P, v);
    int *li = (int *)arena.get(1, 0, ((size_t)H.hsoff[nr] + H.hroff[nr] + 8) * 4);
    if (arena.fail) return arena.fail;
    if (hsend_out && hrecv_out) {
        if (int rc = slab_halo_lists(st, W, P, H, v, rows_by_owner, li, li + H.hsoff[nr])) return rc;
        HIPCHK(hipMemcpyAsync(hsend_out, li, (size_t)H.hsoff[nr] * 4, hipMemcpyDeviceToHost, st));
        HIPCHK(hipMemcpyAsync(hrecv_out, li + H.hsoff[nr], (size_t)H.hroff[nr] * 4, hipMemcpyDeviceToHost, st));
    }
    KCHK();
    HIPCHK(hipMemcpyAsync(owner_out, W.owner, (size_t)m * 4, hipMemcpyDeviceToHost, st));
    HIPCHK(hipMemcpyAsync(mask_out, W.mask, (size_t)m * 4, hipMemcpyDeviceToHost, st));
    HIPCHK(hipMemcpyAsync(rows_by_owner_out, rows_by_owner, (size_t)nd * 4, hipMemcpyDeviceToHost, st));
    HIPCHK(hipStreamSynchronize(st));
    memcpy(tab_out, htab.data(), htab.size() * 4);
    return e.err_code;
}
