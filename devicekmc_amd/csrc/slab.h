// slab.h -- partition of the rows of a sparse symmetric pattern into spatial slabs, shared by the slab-distributed block-CG on X (xtb_slab.inc)
// and the slab-distributed CG on K (kcg.hip); SURVEY 8(e): "row slabs; halo = sites within 3.5 A of a cut".  No counterpart in the reference.
// Rows [first, m) are distributed (X: first = 2, the two driver rows are replicated; K: first = 0); coord[row - first] is the lateral coordinate.
// Everything here works on replicated data with integer counts only: every rank computes the same partition.
#pragma once
#include "common.h"
#include "slab_plan.h"                               // XS_MAXR, XS_BINS; the offsets every list and exchange below goes by
#include <string.h>
#include <vector>

static __global__ void k_slab_hist(int m, int first, const double *__restrict__ coord, double lo, double hi, int *__restrict__ hist)
{
    const int row = first + blockIdx.x * blockDim.x + threadIdx.x;
    if (row >= m) return;
    const double u = hi > lo ? (coord[row - first] - lo) / (hi - lo) : 0.0;
    int b = (int)(u * XS_BINS); b = b < 0 ? 0 : (b >= XS_BINS ? XS_BINS - 1 : b);
    atomicAdd(&hist[b], 1);                          // integer counts: the result does not depend on the order
}
// cuts[r] = first bin of slab r: the smallest bin with at least r / nr of the rows below it (one thread: 4096 bins)
static __global__ void k_slab_cuts(int nr, int nrows, const int *__restrict__ hist, int *__restrict__ cuts)
{
    if (blockIdx.x || threadIdx.x) return;
    int r = 1; long long cum = 0;
    cuts[0] = 0;
    for (int b = 0; b < XS_BINS && r < nr; ++b) {
        while (r < nr && cum * nr >= (long long)r * nrows) cuts[r++] = b;
        cum += hist[b];
    }
    for (; r <= nr; ++r) cuts[r] = XS_BINS;
}
static __global__ void k_slab_owner(int m, int first, const double *__restrict__ coord, double lo, double hi, int nr, const int *__restrict__ cuts, int *__restrict__ owner)
{
    const int row = blockIdx.x * blockDim.x + threadIdx.x;
    if (row >= m) return;
    if (row < first) { owner[row] = 0; return; }     // (replicated rows: the entry is never used as an owner)
    const double u = hi > lo ? (coord[row - first] - lo) / (hi - lo) : 0.0;
    int b = (int)(u * XS_BINS); b = b < 0 ? 0 : (b >= XS_BINS ? XS_BINS - 1 : b);
    int o = 0;
    for (int r = 1; r < nr; ++r) o += cuts[r] <= b ? 1 : 0;
    owner[row] = o;
}
// bit d of mask[row]: row has an entry in a row owned by d != owner[row] (the pattern is symmetric: d reads this row's vector entry).
// Column words may carry a class bit 31 (K): masked off.
template <typename RP>
static __global__ void k_slab_mask(int m, int first, const RP *__restrict__ rp, const int *__restrict__ ci, const int *__restrict__ owner, unsigned *__restrict__ mask)
{
    const int row = blockIdx.x * blockDim.x + threadIdx.x;
    if (row >= m) return;
    unsigned mk = 0;
    if (row >= first) {
        const int o = owner[row];
        for (RP p = rp[row]; p < rp[row + 1]; ++p) { const int c = ci[p] & 0x7fffffff; if (c >= first) { const int oc = owner[c]; if (oc != o) mk |= 1u << oc; } }
    }
    mask[row] = mk;
}
// tab: [nr] rows per owner | [nr] marked rows per owner (mark[row] >= 0; X: the rows of S) | [nr * nr] halo rows s -> d
static __global__ __launch_bounds__(256) void k_slab_count(int m, int first, int nr, const int *__restrict__ owner, const unsigned *__restrict__ mask, const int *__restrict__ mark, int *__restrict__ tab)
{
    __shared__ int lt[XS_MAXR * (XS_MAXR + 2)];
    const int nt = nr * (nr + 2);
    for (int i = threadIdx.x; i < nt; i += blockDim.x) lt[i] = 0;
    __syncthreads();
    for (int row = first + blockIdx.x * blockDim.x + threadIdx.x; row < m; row += gridDim.x * blockDim.x) {
        const int o = owner[row];
        atomicAdd(&lt[o], 1);
        if (mark && mark[row] >= 0) atomicAdd(&lt[nr + o], 1);
        unsigned mk = mask[row];
        while (mk) { const int d = __ffs((int)mk) - 1; mk &= mk - 1; atomicAdd(&lt[2 * nr + o * nr + d], 1); }
    }
    __syncthreads();
    for (int i = threadIdx.x; i < nt; i += blockDim.x) if (lt[i]) atomicAdd(&tab[i], lt[i]);
}
// list building: flag -> exclusive scan -> scatter (ascending order kept)
static __global__ void k_slab_flag_rows(int m, int first, const int *__restrict__ owner, int r, int *__restrict__ flag)
{
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < m) flag[i] = (i >= first && owner[i] == r) ? 1 : 0;
}
static __global__ void k_slab_scatter_rows(int m, const int *__restrict__ flag, const int *__restrict__ pos, int base, int *__restrict__ rows_by_owner)
{
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < m && flag[i]) rows_by_owner[base + pos[i]] = i;
}
// over positions [j0, j1) of rows_by_owner: rows with bit `bit` of their mask set
static __global__ void k_slab_flag_halo(int j0, int j1, const int *__restrict__ rows_by_owner, const unsigned *__restrict__ mask, int bit, int *__restrict__ flag)
{
    const int j = j0 + blockIdx.x * blockDim.x + threadIdx.x;
    if (j < j1) flag[j - j0] = (mask[rows_by_owner[j]] >> bit) & 1u;
}
static __global__ void k_slab_scatter_halo(int j0, int j1, const int *__restrict__ rows_by_owner, const int *__restrict__ flag, const int *__restrict__ pos, int base, int *__restrict__ out)
{
    const int j = j0 + blockIdx.x * blockDim.x + threadIdx.x;
    if (j < j1 && flag[j - j0]) out[base + pos[j - j0]] = rows_by_owner[j];
}

// ---- host side: what both slab loops do around the kernels above, on the engine's stream st ----
// work buffers of a partition of m rows: itab (slab_tab_bytes()), owner | mask (slab_owner_bytes(m)), flag | pos (slab_flag_bytes(m))
struct SlabWork { int *hist, *cuts, *tab, *owner; unsigned *mask; int *flag, *pos; };
static inline size_t slab_owner_bytes(int m) { return (size_t)m * 4 * 2; }
static inline size_t slab_flag_bytes(int m) { return (size_t)(m + 8) * 4 * 2; }
static inline SlabWork slab_work(void *itab, void *owner, void *flag, int m)
{
    return {(int *)itab, (int *)itab + XS_CUTS_AT, (int *)itab + XS_TAB_AT, (int *)owner, (unsigned *)owner + m, (int *)flag, (int *)flag + m + 8};
}
// one partition along coord (lo ... hi) into nr slabs: owner, mask and the count table (mark: may be null)
template <typename RP>
static int slab_partition(hipStream_t st, int m, int first, const RP *rp, const int *ci, const double *coord, double lo, double hi, int nr, const int *mark, const SlabWork &W)
{
    const int nb = (m + 255) / 256;
    HIPCHK(hipMemsetAsync(W.hist, 0, slab_tab_bytes(), st));
    hipLaunchKernelGGL(k_slab_hist, dim3(nb), dim3(256), 0, st, m, first, coord, lo, hi, W.hist);
    hipLaunchKernelGGL(k_slab_cuts, dim3(1), dim3(1), 0, st, nr, m - first, (const int *)W.hist, W.cuts);
    hipLaunchKernelGGL(k_slab_owner, dim3(nb), dim3(256), 0, st, m, first, coord, lo, hi, nr, (const int *)W.cuts, W.owner);
    hipLaunchKernelGGL((k_slab_mask<RP>), dim3(nb), dim3(256), 0, st, m, first, rp, ci, (const int *)W.owner, W.mask);
    hipLaunchKernelGGL(k_slab_count, dim3(std::min(nb, 512)), dim3(256), 0, st, m, first, nr, (const int *)W.owner, (const unsigned *)W.mask, mark, W.tab);
    return 0;
}
// its count table on the host (synchronises the stream)
static int slab_download_tab(hipStream_t st, const SlabWork &W, int nr, std::vector<int> &htab)
{
    htab.resize(slab_tab_ints(nr));
    HIPCHK(hipMemcpyAsync(htab.data(), W.tab, htab.size() * 4, hipMemcpyDeviceToHost, st));
    HIPCHK(hipStreamSynchronize(st));
    return 0;
}
// rows_by_owner[P.rowoff[r] ...) = the rows >= first of owner r, ascending; called for every r
static int slab_rows_of_owner(hipStream_t st, int m, int first, const SlabWork &W, const SlabPlan &P, int r, int *rows_by_owner)
{
    const int nb = (m + 255) / 256;
    hipLaunchKernelGGL(k_slab_flag_rows, dim3(nb), dim3(256), 0, st, m, first, (const int *)W.owner, r, W.flag);
    if (int rc = dkmc_exclusive_scan_i32(W.flag, W.pos, m, nullptr)) return rc;
    hipLaunchKernelGGL(k_slab_scatter_rows, dim3(nb), dim3(256), 0, st, m, (const int *)W.flag, (const int *)W.pos, P.rowoff[r], rows_by_owner);
    return 0;
}
// halo lists of rank v at the offsets H(P, v): what it sends to d (its rows with bit d), what it receives from d (the rows of d with
// bit v) -- the same test on replicated data gives the sender's and the receiver's list
static int slab_halo_lists(hipStream_t st, const SlabWork &W, const SlabPlan &P, const SlabHalo &H, int v, const int *rows_by_owner, int *hsend, int *hrecv)
{
    auto list = [&](int s, int bit, int n, int base, int *out) -> int {      // the n rows of s with that bit -> out[base ...)
        const int j0 = P.rowoff[s], j1 = P.rowoff[s + 1], nb = (j1 - j0 + 255) / 256;
        if (j1 <= j0 || n <= 0) return 0;
        hipLaunchKernelGGL(k_slab_flag_halo, dim3(nb), dim3(256), 0, st, j0, j1, rows_by_owner, (const unsigned *)W.mask, bit, W.flag);
        if (int rc = dkmc_exclusive_scan_i32(W.flag, W.pos, j1 - j0, nullptr)) return rc;
        hipLaunchKernelGGL(k_slab_scatter_halo, dim3(nb), dim3(256), 0, st, j0, j1, rows_by_owner, (const int *)W.flag, (const int *)W.pos, base, out);
        return 0;
    };
    for (int d = 0; d < P.nr; ++d) {
        if (d == v) continue;
        if (int rc = list(v, d, P.hal(v, d), H.hsoff[d], hsend)) return rc;
        if (int rc = list(d, v, P.hal(d, v), H.hroff[d], hrecv)) return rc;
    }
    return 0;
}
// Buffers of the (virtual) ranks of a loop: rank 0's from the scratch slots, those of the virtual ranks > 0 (emulation) from hipMalloc, freed on
// every exit path.  A failure is kept in `fail`; oom: the caller's message.
struct SlabArena {
    hipStream_t st; const char *oom; int fail = 0; std::vector<void *> owned;
    ~SlabArena() { if (!owned.empty()) (void)hipStreamSynchronize(st); for (void *p : owned) (void)hipFree(p); }
    void *get(int iv, int slot, size_t bytes)
    {
        if (iv == 0) { void *p = scratch(slot, bytes); if (!p) fail = eng().err_code ? eng().err_code : 2; return p; }
        void *p = nullptr;
        if (hipMalloc(&p, bytes ? bytes : 8) != hipSuccess) { (void)hipGetLastError(); fail = dkmc_fail(2, oom, __FILE__, __LINE__); return nullptr; }
        owned.push_back(p);
        return p;
    }
};
// The exchanges of an emulation as device copies between the virtual ranks' buffers (buf(r), send(r), recv(r): rank r's).  All-gather: rank a owns
// block a of n doubles.  All-to-all-v: the pieces at the offsets of slab_plan.h, the layout of comm_alltoallv_f64.
template <class Buf> static int slab_emu_allgather(hipStream_t st, int nr, size_t n, Buf buf)
{
    for (int a = 0; a < nr; ++a) for (int d = 0; d < nr; ++d)
        if (a != d) HIPCHK(hipMemcpyAsync(buf(d) + (size_t)a * n, buf(a) + (size_t)a * n, n * 8, hipMemcpyDeviceToDevice, st));
    return 0;
}
template <class Send, class Recv> static int slab_emu_alltoallv(hipStream_t st, int nr, const long long *cnt, Send send, Recv recv)
{
    for (int a = 0; a < nr; ++a) for (int d = 0; d < nr; ++d)
        if (const long long n = cnt[(size_t)a * nr + d])
            HIPCHK(hipMemcpyAsync(recv(d) + slab_recv_off(cnt, nr, a, d), send(a) + slab_send_off(cnt, nr, a, d), (size_t)n * 8, hipMemcpyDeviceToDevice, st));
    return 0;
}
// timing of one virtual rank's launches (emulation): on -- the launch between two events, host-synchronised, *ms its duration; else the launch alone
struct SlabTimer {
    hipStream_t st; hipEvent_t ev[2] = {nullptr, nullptr};
    ~SlabTimer() { for (int i = 0; i < 2; ++i) if (ev[i]) (void)hipEventDestroy(ev[i]); }
    int create() { HIPCHK(hipEventCreate(&ev[0])); HIPCHK(hipEventCreate(&ev[1])); return 0; }
    template <class F> int run(bool on, const F &launch, float *ms)
    {
        if (!on) { launch(); return 0; }
        HIPCHK(hipEventRecord(ev[0], st)); launch(); HIPCHK(hipEventRecord(ev[1], st)); HIPCHK(hipEventSynchronize(ev[1]));
        HIPCHK(hipEventElapsedTime(ms, ev[0], ev[1]));
        return 0;
    }
};
// emulation: vec(iv), m doubles, must hold the same bits on every virtual rank; what: the caller's message
template <class Vec> static int slab_same_bits(hipStream_t st, int nv, size_t m, Vec vec, const char *what)
{
    std::vector<double> y0(m), yv(m);
    HIPCHK(hipMemcpyAsync(y0.data(), vec(0), m * 8, hipMemcpyDeviceToHost, st));
    HIPCHK(hipStreamSynchronize(st));
    for (int iv = 1; iv < nv; ++iv) {
        HIPCHK(hipMemcpy(yv.data(), vec(iv), m * 8, hipMemcpyDeviceToHost));
        if (memcmp(y0.data(), yv.data(), m * 8) != 0) return dkmc_fail(13, what, __FILE__, __LINE__);
    }
    return 0;
}
