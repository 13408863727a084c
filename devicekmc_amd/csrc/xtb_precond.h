// xtb_precond.h -- the split polynomial preconditioner of the block-CG (dkmc_set_x_poly(d)): N x panel products, the packed N, the Horner steps of L = p(N), its
// coefficients, its test aids; and the 16-lanes-per-row gather they share with k_xtb_neigh.  Included by xtb.hip (one translation unit) in front of k_xtb_neigh.
//
// The block loop runs on L A L, A = S X S the Jacobi-scaled operator, L = sum_j c_j N^j the degree-d truncation of the series of (I - N)^(-1/2),
// N = I - An, An = the neighbour part of A with A's full (unit) diagonal -- the couplings of the two driver nodes stay outside N.  CG on A
// preconditioned with An EXACTLY needs 8 iterations where A needs 666 (85 k sites, tools/precond_proto.py): the ill-conditioning of X lives in its
// sparse part, and 2 d sparse panel products per sweep buy 2-3x fewer passes over the tiles (tools/precond_block_proto.py).  The loop's algebra
// is untouched: it sees another SPD operator.  A start vector y0 enters as the right-hand side: A d = b - A y0, d = L dh, dh from zero.
#pragma once
#include "nwin_plan.h"
// ---- the row gather: 16 lanes per row (one per vector), batches of 16 entries ----------------------------------------------------------------
// Lane v of a row's group holds entry v of a batch (column c, weight w); every entry is handed round the group and the 16 panel reads of the batch
// are issued together; entry u goes to accumulator u % 4 in increasing u.  k_xtb_neigh (atom rows), k_xtb_nmul and k_xtb_nmulp are built from these
// pieces -- and k_xtb_nmulp16 from their two-slot forms, with the same sequence of operations per element --, so a row is formed with the same bits by
// all of them.  The pieces take and return VALUES (small structs), no references: whatever a kernel carries round its loop stays a plain local of
// the kernel, and the compiler allocates its registers as it does for the text written out.
//
// XCD-aware order of the row blocks: workgroups b and b + 8 share an XCD (and its 4 MiB L2), so XCD x takes the x-th CONTIGUOUS eighth of the
// nb row blocks -- neighbouring rows (atoms in structure order: neighbours in space) then re-read panel rows from their own L2 instead of each of
// the eight L2s pulling the whole panel from the Infinity Cache (1.4 GB of 128-byte gathers per sweep at 9.4e5 sites)
__device__ __forceinline__ int xtb_xcd_block(int nb, int b) { const int xq = nb >> 3, xr = nb & 7, xc = b & 7; return xc * xq + min(xc, xr) + (b >> 3); }
// entry U of the batch to all 16 lanes of the row's group: DPP row_newbcast (a VALU move; __shfl would be an LDS ds_bpermute per value -- three
// per entry, 1.6e7 of them per sweep at 9.4e5 sites: that, not the gathers, was what the kernel took its time for)
template <int U> __device__ __forceinline__ int xn_bc(int x) { return __builtin_amdgcn_update_dpp(0, x, 0x150 + U, 0xf, 0xf, false); }
// two-slot form: entry 2 J to lanes 0 ... 7, entry 2 J + 1 to lanes 8 ... 15 of every row (row broadcasts under the bank masks 0x3 / 0xC)
template <int J> __device__ __forceinline__ int xn_bc2(int x) { return __builtin_amdgcn_update_dpp(__builtin_amdgcn_update_dpp(0, x, 0x150 + 2 * J, 0xf, 0x3, false), x, 0x151 + 2 * J, 0xf, 0xc, false); }
// a lane's entry as it is handed round: its column and the two halves of its weight
struct XnEntry { int c, wlo, whi; };
__device__ __forceinline__ XnEntry xn_entry(int c, double w) { return {c, __double2loint(w), __double2hiint(w)}; }
// the weight of an entry, reassembled from the broadcasts of its two halves
template <int U> __device__ __forceinline__ double xn_w(XnEntry e) { return __hiloint2double(xn_bc<U>(e.whi), xn_bc<U>(e.wlo)); }
template <int J> __device__ __forceinline__ double xn_w2(XnEntry e) { return __hiloint2double(xn_bc2<J>(e.whi), xn_bc2<J>(e.wlo)); }
// vector v of the panel rows of entries U ... U + 3.  MASKED: a negative column (no entry) yields 0.0 and is not read
// (32-bit byte offsets from the panel's base: the panel is m x 128 B, far below 4 GB)
template <bool MASKED, int U> __device__ __forceinline__ double xn_gather(const double *panel, int v, int c)
{
    const int cu = xn_bc<U>(c);
    return (!MASKED || cu >= 0) ? *reinterpret_cast<const double *>(reinterpret_cast<const char *>(panel) + ((unsigned)cu * (unsigned)(XB_SP * 8) + (unsigned)(v * 8))) : 0.0;
}
struct XnX4 { double x0, x1, x2, x3; };                  // four consecutive entries of one vector
template <bool MASKED, int U> __device__ __forceinline__ XnX4 xn_gather4(const double *panel, int v, int c)
{
    return {xn_gather<MASKED, U>(panel, v, c), xn_gather<MASKED, U + 1>(panel, v, c), xn_gather<MASKED, U + 2>(panel, v, c), xn_gather<MASKED, U + 3>(panel, v, c)};
}
// two-slot form: vectors 2 v8, 2 v8 + 1 (16 bytes) of the panel row of entry 2 J (lanes 0 ... 7) / 2 J + 1 (lanes 8 ... 15)
template <int J> __device__ __forceinline__ double2 xn_gather2(const double *panel, int v8, int c)
{ return *reinterpret_cast<const double2 *>(reinterpret_cast<const char *>(panel) + ((unsigned)xn_bc2<J>(c) * (unsigned)(XB_SP * 8) + (unsigned)(v8 * 16))); }
// the four accumulators over entries U ... U + 3, in that order
struct XnSums { double s0, s1, s2, s3; };
template <int U> __device__ __forceinline__ XnSums xn_acc4(XnEntry e, XnX4 x, XnSums s)
{
    s.s0 += xn_w<U>(e) * x.x0; s.s1 += xn_w<U + 1>(e) * x.x1; s.s2 += xn_w<U + 2>(e) * x.x2; s.s3 += xn_w<U + 3>(e) * x.x3; return s;
}
// two-slot form, pairs J, J + 1 (xj, xj1: entries 2 J ... 2 J + 3) of two vectors: the low half's A is s0, its B s2, the high half's s1 and s3
struct XnSums2 { double A0, A1, B0, B1; };
template <int J> __device__ __forceinline__ XnSums2 xn_acc2(XnEntry e, double2 xj, double2 xj1, XnSums2 s)
{
    const double wa = xn_w2<J>(e), wb = xn_w2<J + 1>(e); s.A0 += wa * xj.x; s.A1 += wa * xj.y; s.B0 += wb * xj1.x; s.B1 += wb * xj1.y; return s;
}
// a whole batch of a CSR row (k_xtb_neigh, k_xtb_nmul): lane v's entry e, missing entries masked
__device__ __forceinline__ XnSums xn_batch16(const double *panel, int v, XnEntry e, XnSums s)
{
    const XnX4 x0 = xn_gather4<true, 0>(panel, v, e.c), x4 = xn_gather4<true, 4>(panel, v, e.c), x8 = xn_gather4<true, 8>(panel, v, e.c), x12 = xn_gather4<true, 12>(panel, v, e.c);
    return xn_acc4<12>(e, x12, xn_acc4<8>(e, x8, xn_acc4<4>(e, x4, xn_acc4<0>(e, x0, s))));
}
// a row of out = ca * add + cb * (N in) from its four accumulators
__device__ __forceinline__ double xn_result(double ca, double av, double cb, double scr, XnSums s) { return ca * av - cb * (scr * ((s.s0 + s.s1) + (s.s2 + s.s3))); }

// ---- N x panel products ------------------------------------------------------------------------------------------------------------------
// out = ca * add + cb * (N in): 16 lanes per row (the row gather above); rows 0 / 1 (driver nodes) and their columns take no part in N.
// LIST (slab-distributed loop, xtb_slab.inc): the rows are the m entries of rowlist (a rank's two driver rows + the rows it owns); every row is
// formed exactly as without the list: the same bits.
template <bool LIST>
__global__ __launch_bounds__(XT_NT) void k_xtb_nmul(int m, const xrp_t *__restrict__ rp, const int *__restrict__ ci, const double *__restrict__ val,
                                                    const double *__restrict__ sc, const double *__restrict__ in, const double *__restrict__ add,
                                                    double ca, double cb, double *__restrict__ out, const XCtrl *ctrl, const int *__restrict__ rowlist)
{
    if (ctrl->done) return;
    const int v = threadIdx.x & 15, g = threadIdx.x >> 4;
    const int li = xtb_xcd_block((int)gridDim.x, (int)blockIdx.x) * 16 + g;
    const bool ok = li < m;
    const int row = LIST ? (ok ? rowlist[li] : 0) : li;
    const bool atom = ok && row >= 2;
    const xrp_t p0 = atom ? rp[row] : 0, p1 = atom ? rp[row + 1] : 0;
    const double scr = ok ? sc[row] : 0.0;
    const double av = ok ? add[(size_t)row * XB_SP + v] : 0.0;
    XnSums s = {0.0, 0.0, 0.0, 0.0};
    for (xrp_t base = p0; base < p1; base += 64) {
        int cm[4]; double wm[4];
#pragma unroll
        for (int bq = 0; bq < 4; ++bq) { const xrp_t pe = base + 16 * bq + v; int c = pe < p1 ? ci[pe] : -1; if (c < 2 || c == row) c = -1; cm[bq] = c; wm[bq] = c >= 0 ? val[pe] : 0.0; }
#pragma unroll
        for (int bq = 0; bq < 4; ++bq) wm[bq] = cm[bq] >= 0 ? wm[bq] * sc[cm[bq]] : 0.0;
#pragma unroll
        for (int bq = 0; bq < 4; ++bq) {
            if (base + 16 * bq >= p1) break;
            s = xn_batch16(in, v, xn_entry(cm[bq], wm[bq]), s);
        }
    }
    if (ok) out[(size_t)row * XB_SP + v] = xn_result(ca, av, cb, scr, s);
}
// N packed for the solve (dkmc_set_x_nmul_form(1), the default): sc and Xs do not change during a solve, so the 2 d N products of every sweep
// read a copy with the column's scaling folded in.  Slice q = rows 4 q ... 4 q + 3 (one wave of k_xtb_nmulp16 / k_xtb_nmulp); it is as wide as its longest row,
// w_q slots; slot k of row 4 q + r at off[q] + 4 k + r (a wave's 16 slots x 4 rows are 64 contiguous entries).  Slot k of a row is its CSR
// position rp[row] + k, so the sums run in the same order as k_xtb_nmul's; entries outside N (driver columns, the diagonal), the driver rows 0 / 1,
// rows past m and the padding are zero weights on a column whose panel row is read anyway (the row itself): they add exactly +0.
// rowlist != nullptr (slab-distributed loop): slice q = list entries 4 q ... 4 q + 3 of the m entries of a rank's row list, same slots per row.
__global__ void k_xtb_npack_width(int m, const xrp_t *__restrict__ rp, int *__restrict__ cnt, const int *__restrict__ rowlist = nullptr)
{
    const int q = blockIdx.x * blockDim.x + threadIdx.x;
    if (q >= (m + 3) / 4) return;
    int w = 0;
    for (int r = 0; r < 4; ++r) {
        const int li = 4 * q + r; if (li >= m) continue;
        const int row = rowlist ? rowlist[li] : li;
        if (row >= 2) w = max(w, (int)(rp[row + 1] - rp[row]));
    }
    cnt[q] = 4 * w;
}
// one wave per slice; the weight is the product k_xtb_nmul forms in its register (val * sc[col], same rounding)
__global__ __launch_bounds__(256) void k_xtb_npack(int m, const xrp_t *__restrict__ rp, const int *__restrict__ ci, const double *__restrict__ val,
                                                   const double *__restrict__ sc, const long long *__restrict__ off, int *__restrict__ pcol, double *__restrict__ pw,
                                                   const int *__restrict__ rowlist = nullptr)
{
    const int q = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
    if (q >= (m + 3) / 4) return;
    const long long o0 = off[q], n = off[q + 1] - o0;
    for (long long i = lane; i < n; i += 64) {
        const int r = (int)(i & 3), k = (int)(i >> 2), li = 4 * q + r;
        const int row = rowlist ? rowlist[li < m ? li : m - 1] : li;
        const bool atom = row >= 2 && li < m;
        const xrp_t p0 = atom ? rp[row] : 0, len = atom ? rp[row + 1] - p0 : 0;
        int c = k < len ? ci[p0 + k] : -1;
        double w = 0.0;
        if (c < 2 || c == row) c = rowlist ? row : (row < m ? row : m - 1);
        else w = val[p0 + k] * sc[c];
        pcol[o0 + i] = c; pw[o0 + i] = w;
    }
}
// head of the packed kernels: the wave's slice (XCD-contiguous row blocks of four slices; slices past (m + 3) / 4 do not exist) and, for the 16 lanes of
// matrix row r of slice q (ok: one of the m rows), the row, the slice's width w and the row's slots (slot k at cq[4 k], wq[4 k])
__device__ __forceinline__ int xn_wave_slice() { return xtb_xcd_block((int)gridDim.x, (int)blockIdx.x) * 4 + __builtin_amdgcn_readfirstlane(threadIdx.x >> 6); }
struct XnRow { int row, w; const int *cq; const double *wq; };
template <bool LIST>
__device__ __forceinline__ XnRow xn_packed_row(const long long *off, const int *pcol, const double *pw, const int *rowlist, int q, int r, bool ok)
{
    const int row = LIST ? (ok ? rowlist[4 * q + r] : 0) : 4 * q + r;
    const long long o0 = off[q]; const int w = (int)((off[q + 1] - o0) >> 2);
    return {row, w, pcol + o0 + r, pw + o0 + r};
}
// slot k of the row; slots past the width (lanes of the last batch): weight 0 on column 0
struct XnSlot { double w; int c; };
__device__ __forceinline__ XnSlot xn_slot(XnRow R, int k) { const int c = k < R.w ? R.cq[4 * k] : 0; return {k < R.w ? R.wq[4 * k] : 0.0, c}; }
// out = ca * add + cb * (N in) on the packed N: the loop runs the slice's width, no row pointers, no scaling gather, no filter.  Entry e of a row goes
// to accumulator e % 4 in increasing e, the result is formed as in k_xtb_nmul: the same bits.  QSF: also QS (as k_xtb_qs_from) from the rows in registers.
// LIST (slab-distributed loop): N packed over the m entries of rowlist (k_xtb_npack with a row list); row = rowlist[4 q + r].
template <bool QSF, bool LIST = false>
__global__ __launch_bounds__(XT_NT) void k_xtb_nmulp(int m, const long long *__restrict__ off, const int *__restrict__ pcol, const double *__restrict__ pw,
                                                     const double *__restrict__ sc, const double *__restrict__ in, const double *__restrict__ add,
                                                     double ca, double cb, double *__restrict__ out, const XCtrl *ctrl, const int *__restrict__ nsrank, double *__restrict__ QS,
                                                     const int *__restrict__ rowlist = nullptr)
{
    if (ctrl->done) return;
    const int v = threadIdx.x & 15, r = (threadIdx.x >> 4) & 3;
    const int q = xn_wave_slice(); if (q >= (m + 3) / 4) return;
    const bool ok = 4 * q + r < m;
    const XnRow R = xn_packed_row<LIST>(off, pcol, pw, rowlist, q, r, ok);
    const double scr = ok ? sc[R.row] : 0.0;
    const double av = ok ? add[(size_t)R.row * XB_SP + v] : 0.0;
    XnSums s = {0.0, 0.0, 0.0, 0.0}; XnSlot n = xn_slot(R, v);
    for (int k0 = 0; k0 < R.w; k0 += 16) {
        const int t = R.w - k0; const XnEntry e = xn_entry(n.c, n.w);
        if (t > 16) n = xn_slot(R, k0 + 16 + v);                               // next batch in flight
        XnX4 x[4];
        x[0] = xn_gather4<false, 0>(in, v, e.c);
        if (t > 4) x[1] = xn_gather4<false, 4>(in, v, e.c);
        if (t > 8) x[2] = xn_gather4<false, 8>(in, v, e.c);
        if (t > 12) x[3] = xn_gather4<false, 12>(in, v, e.c);
        s = xn_acc4<0>(e, x[0], s);
        if (t > 4) s = xn_acc4<4>(e, x[1], s);
        if (t > 8) s = xn_acc4<8>(e, x[2], s);
        if (t > 12) s = xn_acc4<12>(e, x[3], s);
    }
    if (ok) {
        const double o = xn_result(ca, av, cb, scr, s);
        out[(size_t)R.row * XB_SP + v] = o;
        if (QSF) { const int sr = nsrank[R.row]; if (sr >= 0) QS[xtb_qs_pos(sr, v)] = sc[R.row] * o; }
    }
}
// k_xtb_nmulp with 16 bytes per lane (dkmc_set_x_nmul_lane_bytes(16), the default): the same packed N, the same slices, half the gather instructions.  A 16-lane row still
// owns matrix row r and lane v still loads slot k0 + v of it, but one gather takes two slots: lanes 0 ... 7 read columns 2 v, 2 v + 1 of slot 2 j's panel
// row, lanes 8 ... 15 those of slot 2 j + 1's (column and weight reach the halves by row broadcasts under the bank masks 0x3 / 0xC: xn_bc2).  The low half so
// holds k_xtb_nmulp's s0 (slots 0 mod 4, A) and s2 (2 mod 4, B) of two columns, the high half s1 and s3, each summed in increasing slot index over the
// same batches and groups of four; the halves meet once per row (row_ror:8) as (s0 + s1) + (s2 + s3): every element is k_xtb_nmulp's sequence of
// operations, the same bits.  add, out: 16 bytes from the low eight lanes.
template <bool QSF, bool LIST = false>
__global__ __launch_bounds__(XT_NT) void k_xtb_nmulp16(int m, const long long *__restrict__ off, const int *__restrict__ pcol, const double *__restrict__ pw,
                                                       const double *__restrict__ sc, const double *__restrict__ in, const double *__restrict__ add,
                                                       double ca, double cb, double *__restrict__ out, const XCtrl *ctrl, const int *__restrict__ nsrank, double *__restrict__ QS,
                                                       const int *__restrict__ rowlist = nullptr)
{
    if (ctrl->done) return;
    const int v = threadIdx.x & 15, r = (threadIdx.x >> 4) & 3, v8 = v & 7;
    const int q = xn_wave_slice(); if (q >= (m + 3) / 4) return;
    const bool ok = 4 * q + r < m, wr = ok && v < 8;
    const XnRow R = xn_packed_row<LIST>(off, pcol, pw, rowlist, q, r, ok);
    const double scr = ok ? sc[R.row] : 0.0;
    const double2 av = wr ? *reinterpret_cast<const double2 *>(add + (size_t)R.row * XB_SP + 2 * v8) : make_double2(0.0, 0.0);
    XnSums2 s = {0.0, 0.0, 0.0, 0.0}; XnSlot n = xn_slot(R, v);
    for (int k0 = 0; k0 < R.w; k0 += 16) {
        const int t = R.w - k0; const XnEntry e = xn_entry(n.c, n.w);
        if (t > 16) n = xn_slot(R, k0 + 16 + v);                               // next batch in flight
        double2 x[8];
        x[0] = xn_gather2<0>(in, v8, e.c); x[1] = xn_gather2<1>(in, v8, e.c);
        if (t > 4) { x[2] = xn_gather2<2>(in, v8, e.c); x[3] = xn_gather2<3>(in, v8, e.c); }
        if (t > 8) { x[4] = xn_gather2<4>(in, v8, e.c); x[5] = xn_gather2<5>(in, v8, e.c); }
        if (t > 12) { x[6] = xn_gather2<6>(in, v8, e.c); x[7] = xn_gather2<7>(in, v8, e.c); }
        s = xn_acc2<0>(e, x[0], x[1], s);
        if (t > 4) s = xn_acc2<2>(e, x[2], x[3], s);
        if (t > 8) s = xn_acc2<4>(e, x[4], x[5], s);
        if (t > 12) s = xn_acc2<6>(e, x[6], x[7], s);
    }
    // the other half's sums (row_ror:8); on the low half (A + tA) + (B + tB) is (s0 + s1) + (s2 + s3)
    const double tA0 = xor_lane<8>(s.A0), tA1 = xor_lane<8>(s.A1), tB0 = xor_lane<8>(s.B0), tB1 = xor_lane<8>(s.B1);
    if (wr) {
        const double o0 = xn_result(ca, av.x, cb, scr, {s.A0, tA0, s.B0, tB0}), o1 = xn_result(ca, av.y, cb, scr, {s.A1, tA1, s.B1, tB1});
        *reinterpret_cast<double2 *>(out + (size_t)R.row * XB_SP + 2 * v8) = make_double2(o0, o1);
        if (QSF) { const int sr = nsrank[R.row]; if (sr >= 0) { const double sq = sc[R.row]; QS[xtb_qs_pos(sr, 2 * v8)] = sq * o0; QS[xtb_qs_pos(sr, 2 * v8 + 1)] = sq * o1; } }
    }
}
// k_xtb_nmulp16 with the panel operands served from LDS (dkmc_set_x_nmul_window; the plan: nwin_plan.h).  What bounds k_xtb_nmulp16 is the address rate of
// the vector-memory path: every padded slot sends a 128-byte panel row through it, four times the launch's compulsory bytes.  Here a workgroup owns a
// block of B consecutive rows, copies the block's window -- the block and a halo on either side, where structure order keeps an atom's neighbours -- from
// `in` into LDS once, with coalesced 16-byte loads, and then runs k_xtb_nmulp16's loop over its slices: same slots, same order, same accumulators, same
// result formation, the same bits.  Only the operand's source differs: ds_read_b128 for a slot whose column lies in the window, the global gather for a
// flagged one (nwin_code < 0: far columns, the cross-cell neighbours of a lateral tiling).  The code is formed from the packed column in registers;
// the packed N is read as it is.
// 16 waves, 64 rows per pass over the block.  Two workgroups share a CU (LDS), so a SIMD holds 8 waves and a wave 64 registers: what hides the latency of the
// slot loads and of the flagged gathers is the number of waves -- with 8 and 12 waves per workgroup (80 registers) the kernel lost to, then tied with, k_xtb_nmulp16
#define XN_WIN_NT 1024
// the operand of pair J: the code goes round as the column does (xn_bc2 -- here, in front of the branch: a DPP move reads nothing from a lane that is
// switched off, so it must not stand inside it); every lane reads LDS (a flagged one row 0 of the window), the flagged ones then gather
// The window is read through a pointer of the LDS address space: through a generic one the compiler folds the two loads into ONE flat load of a
// selected address, and a flat load goes down the vector-memory path again.
typedef const __attribute__((address_space(3))) char *xn_lds_t;
typedef double xn_d2 __attribute__((ext_vector_type(2)));
template <int J> __device__ __forceinline__ double2 xn_operand2(const double *panel, xn_lds_t win, int v8, int code)
{
    const int cu = xn_bc2<J>(code);
    const xn_d2 l = *reinterpret_cast<const __attribute__((address_space(3))) xn_d2 *>(win + ((unsigned)max(cu, 0) * (unsigned)NWIN_ROW_BYTES + (unsigned)(v8 * 16)));
    double2 x = make_double2(l.x, l.y);
    if (cu < 0) x = *reinterpret_cast<const double2 *>(reinterpret_cast<const char *>(panel) + ((unsigned)~cu * (unsigned)(XB_SP * 8) + (unsigned)(v8 * 16)));
    return x;
}
// head of a slice of the block: its offset and width from the block's offsets in LDS (one global load less in front of the slots), and lane v's slot of
// the first batch of row r
struct XnHeadW { long long o0; int w; XnSlot n; };
__device__ __forceinline__ XnHeadW xn_head_w(const long long *boff, const int *pcol, const double *pw, int sl, int r, int v)
{
    const long long o0 = boff[sl]; const int w = (int)((boff[sl + 1] - o0) >> 2);
    return {o0, w, xn_slot({0, w, pcol + o0 + r, pw + o0 + r}, v)};
}
template <bool QSF>
__global__ __launch_bounds__(XN_WIN_NT) __attribute__((amdgpu_waves_per_eu(8, 8))) void k_xtb_nmulw(int m, const long long *__restrict__ off, const int *__restrict__ pcol, const double *__restrict__ pw,
                                                         const double *__restrict__ sc, const double *__restrict__ in, const double *__restrict__ add,
                                                         double ca, double cb, double *__restrict__ out, const XCtrl *ctrl, const int *__restrict__ nsrank, double *__restrict__ QS,
                                                         int B, int cap_rows)
{
    extern __shared__ double2 xn_win[];
    __shared__ long long xn_boff[NWIN_BLOCK_MAX / 4 + 1];
    if (ctrl->done) return;
    const int blk = xtb_xcd_block((int)gridDim.x, (int)blockIdx.x);
    const NwinWindow W = nwin_window(m, B, cap_rows, blk);
    const int q0 = blk * (B / 4), nq = min(B / 4, (m + 3) / 4 - q0);             // the block's slices (the last block: those that exist)
    for (int i = threadIdx.x; i <= nq; i += XN_WIN_NT) xn_boff[i] = off[q0 + i];
    {   // the window: W.n rows of eight 16-byte pieces
        const double2 *src = reinterpret_cast<const double2 *>(in + (size_t)W.lo * XB_SP);
        const int n16 = W.n * 8;
#pragma unroll 4
        for (int i = threadIdx.x; i < n16; i += XN_WIN_NT) xn_win[i] = src[i];
    }
    __syncthreads();
    const xn_lds_t win = (xn_lds_t)xn_win;
    const int v = threadIdx.x & 15, r = (threadIdx.x >> 4) & 3, v8 = v & 7;
    // a wave takes every (XN_WIN_NT / 64)-th slice of the block; the offsets come from LDS
    for (int sl = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6); sl < nq; sl += XN_WIN_NT / 64) {
        const XnHeadW C = xn_head_w(xn_boff, pcol, pw, sl, r, v);
        const int q = q0 + sl;
        const bool ok = 4 * q + r < m, wr = ok && v < 8;
        const XnRow R = {4 * q + r, C.w, pcol + C.o0 + r, pw + C.o0 + r};
        const double scr = ok ? sc[R.row] : 0.0;
        // (the QS-writing form reads `add` behind the loop: it has no registers to hold it across)
        double2 av = (!QSF && wr) ? *reinterpret_cast<const double2 *>(add + (size_t)R.row * XB_SP + 2 * v8) : make_double2(0.0, 0.0);
        XnSums2 s = {0.0, 0.0, 0.0, 0.0}; XnSlot n = C.n;
        for (int k0 = 0; k0 < R.w; k0 += 16) {
            const int t = R.w - k0; const XnEntry e = xn_entry(nwin_code(n.c, W), n.w);
            if (t > 16) n = xn_slot(R, k0 + 16 + v);                           // next batch in flight
            double2 x[4];                                                      // two halves of the batch: LDS answers soon, and four operands in flight keep the kernel at 64 registers
            x[0] = xn_operand2<0>(in, win, v8, e.c); x[1] = xn_operand2<1>(in, win, v8, e.c);
            if (t > 4) { x[2] = xn_operand2<2>(in, win, v8, e.c); x[3] = xn_operand2<3>(in, win, v8, e.c); }
            s = xn_acc2<0>(e, x[0], x[1], s);
            if (t > 4) s = xn_acc2<2>(e, x[2], x[3], s);
            if (t > 8) {
                x[0] = xn_operand2<4>(in, win, v8, e.c); x[1] = xn_operand2<5>(in, win, v8, e.c);
                if (t > 12) { x[2] = xn_operand2<6>(in, win, v8, e.c); x[3] = xn_operand2<7>(in, win, v8, e.c); }
                s = xn_acc2<4>(e, x[0], x[1], s);
                if (t > 12) s = xn_acc2<6>(e, x[2], x[3], s);
            }
        }
        if (QSF && wr) av = *reinterpret_cast<const double2 *>(add + (size_t)R.row * XB_SP + 2 * v8);
        const double tA0 = xor_lane<8>(s.A0), tA1 = xor_lane<8>(s.A1), tB0 = xor_lane<8>(s.B0), tB1 = xor_lane<8>(s.B1);
        if (wr) {
            const double o0 = xn_result(ca, av.x, cb, scr, {s.A0, tA0, s.B0, tB0}), o1 = xn_result(ca, av.y, cb, scr, {s.A1, tA1, s.B1, tB1});
            *reinterpret_cast<double2 *>(out + (size_t)R.row * XB_SP + 2 * v8) = make_double2(o0, o1);
            if (QSF) { const int sr = nsrank[R.row]; if (sr >= 0) { QS[xtb_qs_pos(sr, 2 * v8)] = scr * o0; QS[xtb_qs_pos(sr, 2 * v8 + 1)] = scr * o1; } }      // (scr is sc[row] here)
        }
    }
}
// QS (the compact, interleaved copy of the S rows the tile kernel reads) of an arbitrary panel
__global__ void k_xtb_qs_from(int m, const double *__restrict__ V, const double *__restrict__ sc, const int *__restrict__ nsrank, double *__restrict__ QS, const XCtrl *ctrl)
{
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= m * XB_SP || ctrl->done) return;
    const int row = i >> 4, v = i & 15;
    const int sr = nsrank[row];
    if (sr >= 0) QS[xtb_qs_pos(sr, v)] = sc[row] * V[i];
}
// start of a preconditioned solve: W <- [T(:, 0) - b | 0 ... 0] (T = A Y0: the residual of the start vector, sign r = A y - b)
__global__ void k_xtb_pre_resid(int m, const double *__restrict__ T, const double *__restrict__ b, double *__restrict__ W)
{
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= m * XB_SP) return;
    W[i] = (i & 15) == 0 ? T[i] - b[i >> 4] : 0.0;
}
// W <- [y | 0 ... 0]
__global__ void k_xtb_pre_col0(int m, const double *__restrict__ y, double *__restrict__ W)
{
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= m * XB_SP) return;
    W[i] = (i & 15) == 0 ? y[i >> 4] : 0.0;
}
// end of a preconditioned solve: y <- y + Z(:, 0)  (Z = L dh, the correction)
__global__ void k_xtb_pre_add(int m, const double *__restrict__ Z, double *__restrict__ y)
{
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < m) y[i] += Z[(size_t)i * XB_SP];
}
// ||T(:, 0) - b||^2, the TRUE residual of the unpreconditioned scaled system, for the stop test a caller relies on: two stages in a fixed order (the
// result depends on m alone, not on the launch).  Stage 1: up to XB_RR_MAXPART workgroups, thread t of workgroup g adds rows 256 g + t, + 256 G, ...,
// then a tree over the workgroup; stage 2: one workgroup adds the partial sums the same way.  (One workgroup of 1024 for everything took 1.1 ms at
// 9.4e5 rows, a launch at 0.007 TB/s.)
#define XB_RR_MAXPART 1024
__device__ __forceinline__ double xtb_tree256(double a)
{
    __shared__ double red[256];
    red[threadIdx.x] = a;
    __syncthreads();
    for (int o = 128; o > 0; o >>= 1) { if ((int)threadIdx.x < o) red[threadIdx.x] += red[threadIdx.x + o]; __syncthreads(); }
    return red[0];
}
__global__ __launch_bounds__(256) void k_xtb_pre_rr_part(int m, const double *__restrict__ T, const double *__restrict__ b, double *__restrict__ part)
{
    double a = 0.0;
    for (int i = blockIdx.x * 256 + threadIdx.x; i < m; i += gridDim.x * 256) { const double d = T[(size_t)i * XB_SP] - b[i]; a += d * d; }
    a = xtb_tree256(a);
    if (threadIdx.x == 0) part[blockIdx.x] = a;
}
__global__ __launch_bounds__(256) void k_xtb_pre_rr(int np, const double *__restrict__ part, double *__restrict__ out)
{
    double a = 0.0;
    for (int i = threadIdx.x; i < np; i += 256) a += part[i];
    a = xtb_tree256(a);
    if (threadIdx.x == 0) out[0] = a;
}

// ---- host side: the packed N of a solve, one Horner step, L = p(N) and its coefficients -----------------------------------------------------
// the packed N of one solve (k_xtb_npack): slice offsets, columns, weights
// win_B > 0: the products run k_xtb_nmulw on blocks of win_B rows with windows of at most win_rows panel rows (dkmc_set_x_nmul_window; nwin_plan.h)
struct XbNPack { const long long *off; const int *col; const double *w; int lane_bytes; int win_B, win_rows; };      // lane_bytes: 16 = k_xtb_nmulp16, 8 = k_xtb_nmulp (dkmc_set_x_nmul_lane_bytes)
// Where the windowed form runs by size (dkmc_set_x_nmul_window(2)): rows from which it paid.  One N product, k_xtb_nmulp16 -> k_xtb_nmulw, median of 8 alternating
// timings (tools/time_nmul_window.py, profiles/nmul_window_by_size.jsonl): 57 782 rows 11.1 -> 16.7 us, 160 526 rows 23.1 -> 23.3 us (the panel fits the L2s,
// a launch is short against the window copy), 642 101 rows 119.0 -> 106.3 us.  Nothing was measured in between, so the gate is the degree rule's last
// breakpoint (xb_poly_rows[1]): the sizes that run degree 16.
static const int xb_nwin_rows = 450000;
// N packed over n rows: rows 0 ... n - 1, or the entries of rowlist (a rank of the slab loop).  alloc(slot, bytes) provides the buffers (scratch, or a
// virtual rank's own); pad: spare slots behind the packed ones
template <class Alloc>
static int xtb_npack(const XtbArgs &A, int n, const int *rowlist, Alloc alloc, long long pad, XbNPack *np)
{
    Engine &e = eng(); hipStream_t st = e.stream;
    const int nsl = (n + 3) / 4;
    int *cnt = (int *)alloc(S_XTB_NPACK_CNT, (size_t)nsl * 4);
    long long *off = (long long *)alloc(S_XTB_NPACK_OFF, (size_t)(nsl + 1) * 8);
    if (!cnt || !off) return e.err_code;
    hipLaunchKernelGGL(k_xtb_npack_width, dim3((nsl + 255) / 256), dim3(256), 0, st, n, A.rp, cnt, rowlist);
    if (int rc = dkmc_exclusive_scan_i32_i64(cnt, off, nsl, off + nsl)) return rc;
    long long nslot = 0;
    HIPCHK(hipMemcpyAsync(&nslot, off + nsl, sizeof(long long), hipMemcpyDeviceToHost, st));
    HIPCHK(hipStreamSynchronize(st));
    int *col = (int *)alloc(S_XTB_NPACK_COL, (size_t)(nslot + pad) * 4);
    double *w = (double *)alloc(S_XTB_NPACK_W, (size_t)(nslot + pad) * 8);
    if (!col || !w) return e.err_code;
    hipLaunchKernelGGL(k_xtb_npack, dim3((nsl + 3) / 4), dim3(256), 0, st, n, A.rp, A.ci, A.val, A.sc, (const long long *)off, col, w, rowlist);
    KCHK();
    np->off = off; np->col = col; np->w = w; np->lane_bytes = e.x_nmul_lane_bytes;
    // the window plan of the solve is arithmetic of (n, block, cap): nothing to build (nwin_plan.h); row lists keep k_xtb_nmulp16
    const bool win = !rowlist && np->lane_bytes == 16 && nwin_use(e.x_nmul_window, n, xb_nwin_rows);
    np->win_B = win ? nwin_block_rows(e.x_nmul_window_block) : 0;
    np->win_rows = win ? nwin_cap_rows(std::min(std::max(e.x_nmul_window_cap, 0), NWIN_CAP_BYTES)) : 0;
    return 0;
}
// one rank's N for the preconditioner's products: n rows (rowlist: the entries of a rank's list, the slab loop), packed (np) or CSR (np null), the
// rank's QS and control words
struct XbNRank { int n; const int *rowlist; const XbNPack *np; double *QS; const XCtrl *ctrl; };
// one Horner step out = ca add + cb (N in); qsf: QS of out as well, from the rows in registers (packed form)
template <bool LIST>
static void xtb_nstep(hipStream_t st, const XtbArgs &A, const XbNRank &R, const double *in, const double *add, double ca, double cb, double *out, bool qsf)
{
    const dim3 g((R.n + 15) / 16), b(XT_NT);
    if (!R.np) { hipLaunchKernelGGL(k_xtb_nmul<LIST>, g, b, 0, st, R.n, A.rp, A.ci, A.val, A.sc, in, add, ca, cb, out, R.ctrl, R.rowlist); return; }
    if (!LIST && R.np->win_B > 0) {
        const int B = R.np->win_B, lds = nwin_lds_bytes(R.n, B, R.np->win_rows);
        const auto kw = qsf ? k_xtb_nmulw<true> : k_xtb_nmulw<false>;
        static bool big_lds = false;                                           // more than 64 KiB of dynamic LDS: once per process
        if (!big_lds) {
            (void)hipFuncSetAttribute((const void *)k_xtb_nmulw<true>, hipFuncAttributeMaxDynamicSharedMemorySize, NWIN_CAP_BYTES);
            (void)hipFuncSetAttribute((const void *)k_xtb_nmulw<false>, hipFuncAttributeMaxDynamicSharedMemorySize, NWIN_CAP_BYTES);
            big_lds = true;
        }
        hipLaunchKernelGGL(kw, dim3(nwin_blocks(R.n, B)), dim3(XN_WIN_NT), lds, st, R.n, R.np->off, R.np->col, R.np->w, A.sc, in, add, ca, cb, out, R.ctrl,
                           qsf ? A.nsrank : (const int *)nullptr, qsf ? R.QS : (double *)nullptr, B, R.np->win_rows);
        return;
    }
    const bool b16 = R.np->lane_bytes == 16;
    const auto k = qsf ? (b16 ? k_xtb_nmulp16<true, LIST> : k_xtb_nmulp<true, LIST>) : (b16 ? k_xtb_nmulp16<false, LIST> : k_xtb_nmulp<false, LIST>);
    hipLaunchKernelGGL(k, g, b, 0, st, R.n, R.np->off, R.np->col, R.np->w, A.sc, in, add, ca, cb, out, R.ctrl, qsf ? A.nsrank : (const int *)nullptr,
                       qsf ? R.QS : (double *)nullptr, R.rowlist);
}
// dst = L src (Horner: pd N products out = c_j src + N in, j = pd - 1 - i, the first step carries c_d); out rotates over w1 / w2 and is dst on the last
// step, so dst must be none of src, w1, w2.  qs: QS of dst as well -- the packed form writes it from the last step's registers, the CSR form by
// k_xtb_qs_from.  Panels are named by Pn: ranks(product, f) calls f(R, at) for every rank of the loop (one GPU: one), R its N and at(p) its panel p
// (product: f issues an N product -- the slab loop times those); pre(i, in) runs before step i (the slab loop's halo exchange of the step's input).
template <class Pn, class Pre, class Ranks>
static int xtb_applyL(hipStream_t st, const XtbArgs &A, int pd, const double *pc, Pn src, Pn dst, Pn w1, Pn w2, bool qs, Pre pre, Ranks ranks)
{
    Pn in = src;
    for (int i = 0; i < pd; ++i) {
        const Pn out = (i == pd - 1) ? dst : ((i & 1) ? w2 : w1);
        const int j = pd - 1 - i;
        const double cb = i == 0 ? pc[pd] : 1.0;
        if (int rc = pre(i, in)) return rc;
        if (int rc = ranks(true, [&](const XbNRank &R, auto at) {
                (R.rowlist ? xtb_nstep<true> : xtb_nstep<false>)(st, A, R, at(in), at(src), pc[j], cb, at(out), qs && i == pd - 1);
            })) return rc;
        in = out;
    }
    if (!qs || pd <= 0) return 0;
    return ranks(false, [&](const XbNRank &R, auto at) {
        if (!R.np) hipLaunchKernelGGL(k_xtb_qs_from, dim3((unsigned)(((size_t)A.m * XB_SP + 255) / 256)), dim3(256), 0, st, A.m, (const double *)at(dst), A.sc, A.nsrank,
                                      R.QS, R.ctrl);
    });
}
// Chebyshev interpolant of degree d of f on [-1, b] in the monomial basis (Horner): pc[0 ... d]
template <class F>
static void xtb_cheb_monomial(int d, double b, F f, double *pc)
{
    const int n = d + 1;
    const double a = -1.0;
    double fx[XB_MAXPOLY1 + 1], c[XB_MAXPOLY1 + 1], pt[XB_MAXPOLY1 + 1] = {0}, Tm2[XB_MAXPOLY1 + 1] = {0}, Tm1[XB_MAXPOLY1 + 1] = {0};
    for (int k = 0; k < n; ++k) { const double t = cos(M_PI * (k + 0.5) / n), x = 0.5 * (b - a) * t + 0.5 * (b + a); fx[k] = f(x); }
    for (int j = 0; j < n; ++j) { double acc = 0.0; for (int k = 0; k < n; ++k) acc += fx[k] * cos(M_PI * j * (k + 0.5) / n); c[j] = acc * 2.0 / n; }
    c[0] *= 0.5;
    Tm2[0] = 1.0; Tm1[1] = 1.0;                                               // T_0, T_1 in powers of t
    pt[0] += c[0]; pt[1] += c[1];
    for (int j = 2; j <= d; ++j) {
        double Tj[XB_MAXPOLY1 + 1];
        for (int i = 0; i <= XB_MAXPOLY1; ++i) Tj[i] = (i >= 1 ? 2.0 * Tm1[i - 1] : 0.0) - Tm2[i];
        for (int i = 0; i <= XB_MAXPOLY1; ++i) { pt[i] += c[j] * Tj[i]; Tm2[i] = Tm1[i]; Tm1[i] = Tj[i]; }
    }
    const double al = 2.0 / (b - a), be = -(a + b) / (b - a);                 // t = al x + be
    double res[XB_MAXPOLY1 + 2] = {0}; res[0] = pt[d]; int deg = 0;
    for (int i = d - 1; i >= 0; --i) {
        double nr[XB_MAXPOLY1 + 2] = {0};
        for (int q = 0; q <= deg; ++q) { nr[q] += res[q] * be; nr[q + 1] += res[q] * al; }
        ++deg; nr[0] += pt[i];
        for (int q = 0; q <= XB_MAXPOLY1 + 1; ++q) res[q] = nr[q];
    }
    for (int q = 0; q <= d; ++q) pc[q] = res[q];
}
// coefficients pc[0 ... pd] of the preconditioner L = p(N) (dkmc_set_x_poly; shared by the one-GPU and the slab-distributed loop)
static void xtb_poly_coeffs(int pd, double *pc)
{
    // coefficients of L = p(N), p ~ (1 - x)^(-1/2): the Chebyshev interpolant of degree d on [-1, 1 - delta], delta = min(0.5, 1.6 / d^2), in the monomial
    // basis (Horner).  Against the Taylor series of the same degree -- which is exact at 0 and weakest where it matters, towards x -> 1 (the largest
    // eigenvalue of N is 0.99994 at 9.4 k sites) -- the block loop needs a third fewer sweeps (85 k sites, d = 4: 34 -> 24, 95 without preconditioner).
    if (pd > 0) xtb_cheb_monomial(pd, 1.0 - std::min(0.5, 1.6 / (double)(pd * pd)), [](double x) { return 1.0 / sqrt(1.0 - x); }, pc);
}
// One-polynomial form (dkmc_set_x_poly_form): coefficients pc[0 ... n] of M^-1 = q(N), q ~ (1 - x)^-1 fitted directly -- the Chebyshev interpolant of
// degree n on [-1, 1 - min(0.5, 3.2 / n^2)].  The split form pays 2 d products for p^2, a polynomial of degree 2 d with d free parameters; q reaches its
// conditioning at n ~ 1.25 d.  Monomial Horner loses digits with the degree (relative error 1.3e-11 at 20, 1e-9 at 24): the cap is 20.
// *qmin: the smallest q over 4001 equidistant points of [-1, 1] (q > 0 there: q(N) is positive definite; r'q(N)r >= qmin r'r scales the loop's stop test)
static void xtb_poly1_coeffs(int n, double *pc, double *qmin)
{
    xtb_cheb_monomial(n, 1.0 - std::min(0.5, 3.2 / (double)(n * n)), [](double x) { return 1.0 / (1.0 - x); }, pc);
    double lo = 1e300;
    for (int k = 0; k <= 4000; ++k) {
        const double x = -1.0 + (double)k / 2000.0;
        double q = pc[n];
        for (int j = n - 1; j >= 0; --j) q = q * x + pc[j];
        lo = std::min(lo, q);
    }
    if (qmin) *qmin = lo;
}
// degree n(d) of the one-polynomial form at the level d (pinned or from xtb_poly_rule): ceil(1.25 d), at most XB_MAXPOLY1, except where a level of the
// rule was measured (profiles/x_poly_form_by_size.jsonl, steady warm-started steps; the fastest n of the level's size, or its lower neighbour inside the
// size's spread): level 8 -> 10 (7.5nm: n = 8 / 10 / 12 take 4.46 / 4.38 / 4.62 ms, tile:5: 20.9 / 19.3 / 19.9 ms), level 10 -> 10 (tile:7: n = 10 / 13 / 16 take
// 55.1 / 55.5 / 56.0 ms, a tie inside the spread of 1.6 %), level 16 -> 18 (tile:10: n = 12 / 14 / 16 / 18 / 20 take 212.4 / 204.8 / 206.3 / 204.1 / 210.4 ms)
static int xtb_poly1_degree(const Engine &e, int d)
{
    if (e.x_poly1_degree > 0) return std::min(e.x_poly1_degree, XB_MAXPOLY1);
    if (d == 10) return 10;
    if (d == 16) return 18;
    return std::min((5 * d + 3) / 4, XB_MAXPOLY1);
}
// which form a preconditioned one-GPU solve runs (dkmc_set_x_poly_form): a pinned degree is a statement about L and keeps the split form under 2
static bool xtb_poly_one(const Engine &e) { return e.x_poly_form == 1 || (e.x_poly_form == 2 && e.x_poly_auto != 0); }
// Where the norm stop test runs by size (dkmc_set_x_stop_form(2)): rows from which it paid.  Same-box A/B against the bound alone, three alternating runs each
// (profiles/ab_bench_x_stop_form.txt), margin 1: 57 782 rows 226.1 -> 223.8 steps/s (-1.0 %, inside the spread of 2.6 %: the loop runs 8.6 sweeps there and
// saves 0.2, the fold launch costs as much), 160 526 rows 52.54 -> 57.69 (+9.8 %, 3 x the spread is 5.2 %), 642 101 rows 6.419 -> 7.215 (+12.4 %, 3 x the
// spread is 0.5 %).  Nothing was measured in between: the gate is the geometric midpoint of the first two sizes.
static const int xb_stop_rows = 96000;
static int xtb_stop_rule(int m) { return m >= xb_stop_rows ? 1 : 0; }
extern "C" int dkmc_xtb_stop_rule(int m) { return xtb_stop_rule(m); }         // host code only (no HIP call)
// ---- the degree a solve runs ---------------------------------------------------------------------------------------------------------------
// A sweep costs (tile pass + row passes) + 2 d N products and the sweep count falls with d, so the best degree grows with the share of the tile pass,
// that is with the rows m of the system.  Step function of m from profiles/x_poly_degree_by_size.jsonl (steady warm-started steps, degrees 6 ... 16,
// the fastest degree of a size, the lower neighbour where that lies within the size's run-to-run spread): 8 at 57.8 k and 160 526 rows (at 160 526
// degree 10 ties with it), 10 at 314 630 (12 is 1.3 % ahead of it, inside the spread; 8 is 3.3 % behind), 16 at 642 101 (1.13 x degree 8).  The
// breakpoints are the geometric midpoints between those sizes.
// rows = {0, 0}: these breakpoints; anything else overrides them (dkmc_set_x_poly_auto_rows: lets a test reach every branch at a small size).
static const int xb_poly_rows[2] = {225000, 450000};                          // rows below the first: step 0, below the second: step 1, else step 2
static const int xb_poly_steps[3] = {8, 10, 16};
static int xtb_poly_rule(int m, const int *rows)
{
    if (m <= 2) return 0;
    const int *n = (rows && (rows[0] > 0 || rows[1] > 0)) ? rows : xb_poly_rows;
    return std::min(xb_poly_steps[m < n[0] ? 0 : (m < n[1] ? 1 : 2)], XB_MAXPOLY);
}
// degree of the one-GPU loop's solve: 0 where it runs plain (base degree 0, no tunnelling set, sharded), the pinned degree, or the rule's
static int xtb_poly_degree(const Engine &e, const XtbArgs &A)
{
    if (A.sharded || A.m <= 2 || A.ns <= 0 || e.x_poly <= 0) return 0;
    return e.x_poly_auto ? xtb_poly_rule(A.m, e.x_poly_rows) : std::min(e.x_poly, XB_MAXPOLY);
}

// ---- test aids of the split polynomial preconditioner (tests/test_precond_coeffs.py, tests/test_gpu_precond_reference.py) -------------------
// The production path (xtb_npack, xtb_nstep, xtb_applyL) on buffers of their own (S_XTB_TEST_*): nothing a solve reads or keeps is touched.
// coefficients pc[0 ... degree] of L = p(N); host code only (no HIP call)
extern "C" int dkmc_xtb_poly_coeffs(int degree, double *pc)
{
    if (degree < 1 || degree > XB_MAXPOLY || !pc) return dkmc_fail(13, "xtb_poly_coeffs: degree outside 1 ... 16", __FILE__, __LINE__);
    xtb_poly_coeffs(degree, pc);
    return 0;
}
// coefficients pc[0 ... n] of the one-polynomial form and the smallest q on [-1, 1]; host code only (no HIP call)
extern "C" int dkmc_xtb_poly1_coeffs(int n, double *pc, double *qmin)
{
    if (n < 1 || n > XB_MAXPOLY1 || !pc) return dkmc_fail(13, "xtb_poly1_coeffs: degree outside 1 ... 20", __FILE__, __LINE__);
    xtb_poly1_coeffs(n, pc, qmin);
    return 0;
}
// the degree the rule gives a one-GPU solve of m rows (breakpoints of dkmc_set_x_poly_auto_rows included); host code only (no HIP call)
extern "C" int dkmc_xtb_poly_rule(int m) { return xtb_poly_rule(m, eng().x_poly_rows); }
// QS (interleaved, xtb_qs_pos) -> [ns][16]
__global__ void k_xtb_test_qs_decode(int ns, const double *__restrict__ QS, double *__restrict__ out)
{
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < ns * XB_SP) out[i] = QS[xtb_qs_pos(i >> 4, i & 15)];
}
// the packed N of a test aid in its own slots (xtb_npack's alloc)
static void *xtb_test_alloc(int slot, size_t bytes)
{
    return scratch(slot == S_XTB_NPACK_CNT ? S_XTB_TEST_NPCNT : slot == S_XTB_NPACK_OFF ? S_XTB_TEST_NPOFF : slot == S_XTB_NPACK_COL ? S_XTB_TEST_NPCOL : S_XTB_TEST_NPW, bytes);
}
// QS of the test aids zeroed, then decoded into qs [ns][16] after the step(s)
static int xtb_test_qs_out(hipStream_t st, int ns, const double *QS, double *qs)
{
    double *dq = (double *)scratch(S_XTB_TEST_ADD, (size_t)ns * XB_SP * 8);      // (the add panel of a step is spent by now)
    if (!dq) return eng().err_code;
    hipLaunchKernelGGL(k_xtb_test_qs_decode, dim3((unsigned)(((size_t)ns * XB_SP + 255) / 256)), dim3(256), 0, st, ns, QS, dq);
    KCHK();
    HIPCHK(hipMemcpyAsync(qs, dq, (size_t)ns * XB_SP * 8, hipMemcpyDeviceToHost, st));
    return 0;
}
// One Horner step out = ca add + cb (N in) over a caller-given CSR (m rows, rp[m] entries) and [m][16] panels: form 1 packs N (xtb_npack) first and runs the
// packed kernel dkmc_set_x_nmul_lane_bytes selects, form 0 runs on the CSR; rowlist (nlist rows): the LIST instantiations; nsrank (ns S rows): QS of out as well -- packed: from the step's registers, CSR:
// k_xtb_qs_from over all m rows, as xtb_applyL takes it on its last step.  out is read before the step and written back after it.
extern "C" int dkmc_xtb_test_nstep(int m, const long long *rp, const int *ci, const double *val, const double *sc, const double *in, const double *add,
                                   double ca, double cb, int form, const int *rowlist, int nlist, const int *nsrank, int ns, double *out, double *qs)
{
    Engine &e = eng(); hipStream_t st = e.stream;
    if (m < 1 || !rp || !sc || !in || !add || !out || (form != 0 && form != 1)) return dkmc_fail(13, "xtb_test_nstep: bad arguments", __FILE__, __LINE__);
    const long long nnz = rp[m];
    if (rp[0] != 0 || nnz < 0 || nnz > 0x7fffffffll || (nnz > 0 && (!ci || !val))) return dkmc_fail(13, "xtb_test_nstep: bad row pointers", __FILE__, __LINE__);
    for (int i = 0; i < m; ++i) if (rp[i + 1] < rp[i]) return dkmc_fail(13, "xtb_test_nstep: bad row pointers", __FILE__, __LINE__);
    for (long long p = 0; p < nnz; ++p) if (ci[p] < 0 || ci[p] >= m) return dkmc_fail(13, "xtb_test_nstep: column outside the rows", __FILE__, __LINE__);
    if (rowlist) {
        if (nlist < 1 || nlist > m) return dkmc_fail(13, "xtb_test_nstep: bad row list", __FILE__, __LINE__);
        for (int i = 0; i < nlist; ++i) if (rowlist[i] < 0 || rowlist[i] >= m) return dkmc_fail(13, "xtb_test_nstep: bad row list", __FILE__, __LINE__);
    }
    if (nsrank) {
        if (ns < 1 || !qs) return dkmc_fail(13, "xtb_test_nstep: bad S ranks", __FILE__, __LINE__);
        for (int i = 0; i < m; ++i) if (nsrank[i] < -1 || nsrank[i] >= ns) return dkmc_fail(13, "xtb_test_nstep: bad S ranks", __FILE__, __LINE__);
    }
    const size_t pan = (size_t)m * XB_SP * 8;
    xrp_t *drp = (xrp_t *)scratch(S_XTB_TEST_RP, (size_t)(m + 1) * sizeof(xrp_t));
    int *dci = (int *)scratch(S_XTB_TEST_CI, (size_t)nnz * 4);
    double *dval = (double *)scratch(S_XTB_TEST_VAL, (size_t)nnz * 8), *dsc = (double *)scratch(S_XTB_TEST_SC, (size_t)m * 8);
    double *din = (double *)scratch(S_XTB_TEST_IN, pan), *dadd = (double *)scratch(S_XTB_TEST_ADD, pan), *dout = (double *)scratch(S_XTB_TEST_OUT, pan);
    int *dns = nsrank ? (int *)scratch(S_XTB_TEST_NSR, (size_t)m * 4) : nullptr;
    int *dlist = rowlist ? (int *)scratch(S_XTB_TEST_LIST, (size_t)nlist * 4) : nullptr;
    double *QS = nsrank ? (double *)scratch(S_XTB_TEST_QS, (size_t)(ns + 2) * XB_SP * 8) : nullptr;
    XCtrl *ctrl = (XCtrl *)scratch(S_XTB_TEST_CTRL, sizeof(XCtrl));
    if (!drp || !dci || !dval || !dsc || !din || !dadd || !dout || (nsrank && (!dns || !QS)) || (rowlist && !dlist) || !ctrl) return e.err_code;
    HIPCHK(hipMemcpyAsync(drp, rp, (size_t)(m + 1) * sizeof(xrp_t), hipMemcpyHostToDevice, st));
    if (nnz > 0) {
        HIPCHK(hipMemcpyAsync(dci, ci, (size_t)nnz * 4, hipMemcpyHostToDevice, st));
        HIPCHK(hipMemcpyAsync(dval, val, (size_t)nnz * 8, hipMemcpyHostToDevice, st));
    }
    HIPCHK(hipMemcpyAsync(dsc, sc, (size_t)m * 8, hipMemcpyHostToDevice, st));
    HIPCHK(hipMemcpyAsync(din, in, pan, hipMemcpyHostToDevice, st));
    HIPCHK(hipMemcpyAsync(dadd, add, pan, hipMemcpyHostToDevice, st));
    HIPCHK(hipMemcpyAsync(dout, out, pan, hipMemcpyHostToDevice, st));
    if (dns) HIPCHK(hipMemcpyAsync(dns, nsrank, (size_t)m * 4, hipMemcpyHostToDevice, st));
    if (dlist) HIPCHK(hipMemcpyAsync(dlist, rowlist, (size_t)nlist * 4, hipMemcpyHostToDevice, st));
    if (QS) HIPCHK(hipMemsetAsync(QS, 0, (size_t)(ns + 2) * XB_SP * 8, st));
    HIPCHK(hipMemsetAsync(ctrl, 0, sizeof(XCtrl), st));
    XtbArgs A{};
    A.m = m; A.ns = ns; A.rp = drp; A.ci = dci; A.val = dval; A.sc = dsc; A.nsrank = dns;
    const int n = rowlist ? nlist : m;
    XbNPack npk{};
    if (form == 1) { if (int rc = xtb_npack(A, n, (const int *)dlist, xtb_test_alloc, 0, &npk)) return rc; }
    const XbNRank R{n, dlist, form == 1 ? &npk : nullptr, QS, ctrl};
    (rowlist ? xtb_nstep<true> : xtb_nstep<false>)(st, A, R, din, dadd, ca, cb, dout, nsrank != nullptr);
    if (nsrank && form == 0)
        hipLaunchKernelGGL(k_xtb_qs_from, dim3((unsigned)((pan / 8 + 255) / 256)), dim3(256), 0, st, m, (const double *)dout, (const double *)dsc, (const int *)dns, QS, (const XCtrl *)ctrl);
    KCHK();
    HIPCHK(hipMemcpyAsync(out, dout, pan, hipMemcpyDeviceToHost, st));
    if (nsrank) { if (int rc = xtb_test_qs_out(st, ns, QS, qs)) return rc; }
    HIPCHK(hipStreamSynchronize(st));
    return e.err_code;
}
// L in (xtb_applyL with QS, as product_pre calls it) on the X left resident by the last single-GPU solve, with that solve's sc, Xs and S ranks:
// in / out [m][16] (m = rows of X), qs [ns][16].  Neither the warm start nor the iteration hint of the next solve is touched.
extern "C" int dkmc_xtb_check_poly(int degree, int form, const double *in, double *out, double *qs)
{
    Engine &e = eng(); hipStream_t st = e.stream; const XTState &X = g_xt;
    if (!X.valid || comm_attached() || X.tile_n != X.ntiles || X.ns <= 0) return dkmc_fail(13, "xtb_check_poly: needs the X of a single-GPU solve", __FILE__, __LINE__);
    if (degree < 1 || degree > XB_MAXPOLY || (form != 0 && form != 1) || !in || !out || !qs) return dkmc_fail(13, "xtb_check_poly: bad arguments", __FILE__, __LINE__);
    const int m = X.Nsub;
    const size_t pan = (size_t)m * XB_SP * 8;
    double *sc = (double *)e.buf[S_CG_S];
    double *din = (double *)scratch(S_XTB_TEST_IN, pan), *dout = (double *)scratch(S_XTB_TEST_OUT, pan);
    double *W1 = (double *)scratch(S_XTB_TEST_W1, pan), *W2 = (double *)scratch(S_XTB_TEST_W2, pan);
    double *QS = (double *)scratch(S_XTB_TEST_QS, (size_t)X.ns_pad * XB_SP * 8);
    XCtrl *ctrl = (XCtrl *)scratch(S_XTB_TEST_CTRL, sizeof(XCtrl));
    if (!din || !dout || !W1 || !W2 || !QS || !ctrl) return e.err_code;
    if (!sc || !g_xb.rp || !g_xb.ci || !g_xb.val || !g_xb.nsrank) return dkmc_fail(13, "xtb_check_poly: no solver state", __FILE__, __LINE__);
    HIPCHK(hipMemcpyAsync(din, in, pan, hipMemcpyHostToDevice, st));
    HIPCHK(hipMemsetAsync(QS, 0, (size_t)X.ns_pad * XB_SP * 8, st));
    HIPCHK(hipMemsetAsync(ctrl, 0, sizeof(XCtrl), st));
    XtbArgs A{};
    A.m = m; A.ns = X.ns; A.ns_pad = X.ns_pad; A.rp = g_xb.rp; A.ci = g_xb.ci; A.val = g_xb.val; A.sc = sc; A.nsrank = g_xb.nsrank;
    XbNPack npk{};
    if (form == 1) { if (int rc = xtb_npack(A, m, nullptr, xtb_test_alloc, 0, &npk)) return rc; }
    const XbNRank nk{m, nullptr, form == 1 ? &npk : nullptr, QS, ctrl};
    double pc[XB_MAXPOLY + 1] = {1.0};
    xtb_poly_coeffs(degree, pc);
    if (int rc = xtb_applyL(st, A, degree, pc, din, dout, W1, W2, true, [](int, double *) { return 0; },
                            [&](bool, auto f) { f(nk, [](double *p) { return p; }); return 0; })) return rc;
    KCHK();
    HIPCHK(hipMemcpyAsync(out, dout, pan, hipMemcpyDeviceToHost, st));
    if (int rc = xtb_test_qs_out(st, X.ns, QS, qs)) return rc;
    HIPCHK(hipStreamSynchronize(st));
    return e.err_code;
}
// Measurement aid (tools/time_nmul_window.py): mean duration of one N product inside L = p(N), `reps` applications of L back to back on the resident X
// (dkmc_xtb_check_poly's set-up, packed form, the current switches); the input panel is whatever the test buffers hold -- timing does not depend on it
extern "C" int dkmc_xtb_time_poly(int degree, int reps, double *us)
{
    Engine &e = eng(); hipStream_t st = e.stream; const XTState &X = g_xt;
    if (!X.valid || comm_attached() || X.tile_n != X.ntiles || X.ns <= 0) return dkmc_fail(13, "xtb_time_poly: needs the X of a single-GPU solve", __FILE__, __LINE__);
    if (degree < 1 || degree > XB_MAXPOLY || reps < 1 || !us) return dkmc_fail(13, "xtb_time_poly: bad arguments", __FILE__, __LINE__);
    const int m = X.Nsub;
    const size_t pan = (size_t)m * XB_SP * 8;
    double *sc = (double *)e.buf[S_CG_S];
    double *din = (double *)scratch(S_XTB_TEST_IN, pan), *dout = (double *)scratch(S_XTB_TEST_OUT, pan);
    double *W1 = (double *)scratch(S_XTB_TEST_W1, pan), *W2 = (double *)scratch(S_XTB_TEST_W2, pan);
    double *QS = (double *)scratch(S_XTB_TEST_QS, (size_t)X.ns_pad * XB_SP * 8);
    XCtrl *ctrl = (XCtrl *)scratch(S_XTB_TEST_CTRL, sizeof(XCtrl));
    if (!din || !dout || !W1 || !W2 || !QS || !ctrl) return e.err_code;
    if (!sc || !g_xb.rp || !g_xb.ci || !g_xb.val || !g_xb.nsrank) return dkmc_fail(13, "xtb_time_poly: no solver state", __FILE__, __LINE__);
    HIPCHK(hipMemsetAsync(din, 0, pan, st));
    HIPCHK(hipMemsetAsync(ctrl, 0, sizeof(XCtrl), st));
    XtbArgs A{};
    A.m = m; A.ns = X.ns; A.ns_pad = X.ns_pad; A.rp = g_xb.rp; A.ci = g_xb.ci; A.val = g_xb.val; A.sc = sc; A.nsrank = g_xb.nsrank;
    XbNPack npk{};
    if (int rc = xtb_npack(A, m, nullptr, xtb_test_alloc, 0, &npk)) return rc;
    const XbNRank nk{m, nullptr, &npk, QS, ctrl};
    double pc[XB_MAXPOLY + 1] = {1.0};
    xtb_poly_coeffs(degree, pc);
    hipEvent_t e0, e1; HIPCHK(hipEventCreate(&e0)); HIPCHK(hipEventCreate(&e1));
    for (int r = -1; r < reps; ++r) {
        if (r == 0) HIPCHK(hipEventRecord(e0, st));
        if (int rc = xtb_applyL(st, A, degree, pc, din, dout, W1, W2, true, [](int, double *) { return 0; },
                                [&](bool, auto f) { f(nk, [](double *p) { return p; }); return 0; })) return rc;
    }
    HIPCHK(hipEventRecord(e1, st));
    HIPCHK(hipEventSynchronize(e1));
    float ms = 0.f; HIPCHK(hipEventElapsedTime(&ms, e0, e1));
    (void)hipEventDestroy(e0); (void)hipEventDestroy(e1);
    KCHK();
    *us = (double)ms * 1e3 / ((double)reps * degree);
    return e.err_code;
}
