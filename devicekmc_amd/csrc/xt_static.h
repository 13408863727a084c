// xt_static.h -- the all-metal strips of the tile store, kept from solve to solve (dkmc_set_x_static_tiles; included by xt.hip).
//
// With S in metals-first order (current.hip step 2: [inner-contact metals in atom order | vacancies in atom order], nM metals) the strips
// w < w_static = nM / 256 hold only metal columns and, in the upper triangle, only metal rows (row rank < column rank < 256 w_static <= nM).
// An entry between two contact metals depends on their positions, their CB edges and a handful of parameters -- all fixed for a bias point --
// and not on the coefficient cache (contact x contact is the closed form of wkb_T, kind 2).  The tile list is strip-major, so the tiles of these
// strips are a PREFIX of tiles[], their sub-blocks a prefix of the fp64 store and of its fp32 image, whatever the vacancies behind them do
// (nK may change: the cells below the diagonal are empty either way).  After a fill that completed the assembly keeps
//   * the tile-list prefix (k, w, mask, soff) with its tile, sub-block and non-zero counts;
//   * a device snapshot of the metals: per metal x, y, z, CB edge, flag (and their count);
//   * the XParams fields k_xt_census, xt_tvalue, wkb_T and site_dist read;
//   * the identity of the two allocations (pointer and capacity of S_XT_TVAL / S_XT_TVAL32) and whether the image was written,
// and the next assembly fills tiles[t_static ...] only if ALL of that compares equal, bitwise, the device parts on the device (their verdict
// travels with the counts the assembly synchronises on anyway).  Any doubt is a full fill.  The kept state is dropped when an assembly starts
// and set again only when its solve has passed its last synchronisation: a failed assembly or solve never leaves a prefix behind.
// The census skips the cells of the kept strips in the same way: their masks are scattered from the kept tile prefix.
#pragma once

enum { XS_KEPT = 0, XS_FIRST = 1, XS_METALS = 2, XS_PARAMS = 3, XS_STORE = 4, XS_IMAGE = 5, XS_PREFIX = 6, XS_NA = 7 };      // info[6] of dkmc_get_x_static_info

struct XStatic {
    bool valid = false;
    const void *key = nullptr;                      // the GPUBuffers (its site_x array, as current.hip keys its per-buffer state)
    int nM = 0, w_static = 0, t_static = 0; long long sub_static = 0; unsigned long long nnz_static = 0;
    double par[6] = {0, 0, 0, 0, 0, 0}; int pbc = 0;     // tol, nn_dist, m_e, V0, laty, latz
    void *tval = nullptr, *tval32 = nullptr; size_t tval_cap = 0, tval32_cap = 0; bool img = false;
    XTile *tiles = nullptr; size_t tiles_cap = 0;   // device: the kept prefix
    double *snap_d = nullptr; int *snap_f = nullptr; int snap_cap = 0;       // device: x | y | z | cb of the nM metals; their flags
    int *flags = nullptr;                           // device: [0] metals differ, [1] tile prefix differs
    // the assembly under way: what becomes the kept state once the solve has passed its last synchronisation
    bool pending = false, reused = false;
    long long verify_nnz = -1;                      // non-zeros the self-check's full fill counted (-1: not run)
    long long info[8] = {0, 0, 0, 0, 0, 0, XS_NA, -1}, verify[4] = {0, 0, 0, 0};
};
static XStatic g_xs;
void xt_static_invalidate() { g_xs.valid = false; g_xs.pending = false; }

static inline int xs_w_static(int nM) { return nM > 0 ? nM / XT_C : 0; }      // (dkmc_x_static_strips, engine.hip, is the same arithmetic for the tests)

__device__ __forceinline__ bool xs_same(double a, double b) { return __double_as_longlong(a) == __double_as_longlong(b); }
__global__ void k_xs_cmp_metals(int nM, SNodes S, const double *__restrict__ d, const int *__restrict__ f, int *flags)
{
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= nM) return;
    if (!xs_same(S.x[i], d[i]) || !xs_same(S.y[i], d[nM + i]) || !xs_same(S.z[i], d[2 * (size_t)nM + i]) || !xs_same(S.cb[i], d[3 * (size_t)nM + i]) || S.flag[i] != f[i]) flags[0] = 1;
}
__global__ void k_xs_snapshot(int nM, SNodes S, double *__restrict__ d, int *__restrict__ f)
{
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= nM) return;
    d[i] = S.x[i]; d[nM + i] = S.y[i]; d[2 * (size_t)nM + i] = S.z[i]; d[3 * (size_t)nM + i] = S.cb[i]; f[i] = S.flag[i];
}
__global__ void k_xs_cmp_tiles(int n, const XTile *__restrict__ a, const XTile *__restrict__ b, int *flags)
{
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const XTile x = a[i], y = b[i];
    if (x.k != y.k || x.w != y.w || x.mask != y.mask || x.soff != y.soff) flags[1] = 1;
}
// masks of the kept strips' cells from the kept tile prefix (the cells were zeroed first; nK is this assembly's).  Nothing if the metals differ:
// k_xt_census then takes these cells like any other
__global__ void k_xs_scatter_masks(int n, const XTile *__restrict__ kept, int nK, const int *__restrict__ flags, unsigned *__restrict__ cmask)
{
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n || flags[0]) return;
    const XTile t = kept[i];
    cmask[(long long)t.w * nK + t.k] = t.mask;
}
template <typename T>
__global__ void k_xs_count_diff(long long n, const T *__restrict__ a, const T *__restrict__ b, unsigned long long *cnt)
{
    const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    int d = (i < n && a[i] != b[i]) ? 1 : 0;
    d = wave_sum_all_i(d);
    if ((threadIdx.x & 63) == 0 && d) atomicAdd(cnt, (unsigned long long)d);
}

// S_XT_TVAL / S_XT_TVAL32 grown WITH their first keep_bytes (scratch() frees before it allocates).  *kept = false where the old contents are gone
static void *xs_scratch_keep(int slot, size_t bytes, size_t keep_bytes, bool may_fail, bool *kept)
{
    Engine &e = eng();
    *kept = true;
    if (e.bufsz[slot] >= bytes) return e.buf[slot];
    const size_t want = bytes + bytes / 8 + 256;
    void *nb = nullptr;
    if (!e.buf[slot] || keep_bytes > e.bufsz[slot] || hipMalloc(&nb, want) != hipSuccess) {
        (void)hipGetLastError(); *kept = false;
        return may_fail ? scratch_try(slot, bytes) : scratch(slot, bytes);
    }
    (void)hipStreamSynchronize(e.stream);
    if (hipMemcpy(nb, e.buf[slot], keep_bytes, hipMemcpyDeviceToDevice) != hipSuccess) { (void)hipGetLastError(); *kept = false; }
    (void)hipFree(e.buf[slot]);
    e.buf[slot] = nb; e.bufsz[slot] = want;
    return nb;
}
static int xs_reserve(int nM, int ntiles_prefix)
{
    XStatic &K = g_xs;
    if (!K.flags) HIPCHK(hipMalloc((void **)&K.flags, 4 * sizeof(int)));
    if (K.snap_cap < nM) {
        if (K.snap_d) (void)hipFree(K.snap_d);
        if (K.snap_f) (void)hipFree(K.snap_f);
        K.snap_d = nullptr; K.snap_f = nullptr; K.snap_cap = 0;
        HIPCHK(hipMalloc((void **)&K.snap_d, (size_t)nM * 4 * 8)); HIPCHK(hipMalloc((void **)&K.snap_f, (size_t)nM * 4));
        K.snap_cap = nM;
    }
    if (K.tiles_cap < (size_t)ntiles_prefix) {
        if (K.tiles) (void)hipFree(K.tiles);
        K.tiles = nullptr; K.tiles_cap = 0;
        const size_t cap = (size_t)ntiles_prefix + ntiles_prefix / 8 + 16;
        HIPCHK(hipMalloc((void **)&K.tiles, cap * sizeof(XTile)));
        K.tiles_cap = cap;
    }
    return 0;
}

// Self-check (dkmc_debug_x_static_verify; tests and small sizes: it holds a second store): the full census and a full fill of the resident tile
// list (the plain form of the fill kernel throughout) into buffers of their own, compared with what the assembly left -- differing words of cmask, of the fp64 store, of the fp32 image.  The
// resident store is only read.
static int xs_verify(const XParams &P, int ns, int nK, int nW, long long ncell, const SNodes &SN, const TCacheView &TC, const unsigned *cmask,
                     const XTile *tiles, int ntiles, long long nsub, const double *tval, const float *tval32)
{
    Engine &e = eng(); hipStream_t st = e.stream; XStatic &K = g_xs;
    unsigned *vmask = nullptr; double *vval = nullptr; float *vval32 = nullptr; unsigned long long *vc = nullptr;
    unsigned long long h[6] = {0, 0, 0, 0, 0, 0};
    auto body = [&]() -> int {
        HIPCHK(hipMalloc((void **)&vmask, (size_t)(ncell + 4) * 4));
        HIPCHK(hipMalloc((void **)&vval, (size_t)(nsub + 4) * XT_SUB * 8));
        if (tval32) HIPCHK(hipMalloc((void **)&vval32, (size_t)(nsub + 4) * XT_SUB * 4));
        HIPCHK(hipMalloc((void **)&vc, sizeof(h)));
        HIPCHK(hipMemsetAsync(vc, 0, sizeof(h), st));
        hipLaunchKernelGGL(k_xt_census, dim3((unsigned)((ncell + 3) / 4)), dim3(XT_NT), 0, st, P, ns, nK, nW, SN, vmask, (const int *)nullptr, 0ll);
        hipLaunchKernelGGL((k_xs_count_diff<unsigned>), dim3((unsigned)((ncell + 255) / 256)), dim3(256), 0, st, ncell, cmask, (const unsigned *)vmask, vc + 2);
        if (ntiles > 0) {
            hipLaunchKernelGGL((k_xt_fill<0>), dim3(ntiles), dim3(XT_NT), 0, st, P, ns, tiles, 0, SN, TC, vval, vc, vval32, 0);
            const long long n = nsub * XT_SUB;
            hipLaunchKernelGGL((k_xs_count_diff<unsigned long long>), dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st, n, (const unsigned long long *)tval,
                               (const unsigned long long *)vval, vc + 3);
            if (tval32) hipLaunchKernelGGL((k_xs_count_diff<unsigned>), dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st, n, (const unsigned *)tval32, (const unsigned *)vval32, vc + 4);
        }
        KCHK();
        HIPCHK(hipMemcpyAsync(h, vc, sizeof(h), hipMemcpyDeviceToHost, st));
        HIPCHK(hipStreamSynchronize(st));
        return 0;
    };
    const int rc = body();
    if (vmask) (void)hipFree(vmask);
    if (vval) (void)hipFree(vval);
    if (vval32) (void)hipFree(vval32);
    if (vc) (void)hipFree(vc);
    if (rc) return rc;
    K.verify[0] = (long long)h[2]; K.verify[1] = (long long)h[3]; K.verify[2] = (long long)h[4]; K.verify[3] = 0;
    K.verify_nnz = (long long)(h[0] + h[1]);
    return 0;
}

// ---- report (include/devicekmc_hip.h, include/devicekmc_hip_debug.h) ------------------------------------------------------------------------
// info: [0] 1 = the last assembly ran in metals-first order, [1] w_static, [2] tiles kept, [3] tiles filled, [4] sub-blocks kept, [5] sub-blocks
// filled, [6] why nothing was kept (XS_*; 0 = the prefix was kept), [7] the self-check: -1 not run, else the sum of its four counts
extern "C" int dkmc_get_x_static_info(long long *info8)
{
    if (info8) for (int c = 0; c < 8; ++c) info8[c] = g_xs.info[c];
    return 0;
}
// the self-check's counts of the last solve: differing words of cmask, of the fp64 store, of the fp32 image; |X_nnz as reported - recounted|
extern "C" int dkmc_debug_get_x_static_verify(long long *v4)
{
    if (v4) for (int c = 0; c < 4; ++c) v4[c] = g_xs.verify[c];
    return 0;
}
// Test aids: the system row of every S rank of the last one-GPU assembly (srow_out[ns]), and the tunnelling block's row sums T.1 per system row
// (the diagonal pass; d_out[Nsub], 0 for the rows outside S) -- the same operator in either S order, summed in that order
extern "C" int dkmc_xt_get_srow(int *ns_out, int *srow_out)
{
    Engine &e = eng(); const XTState &X = g_xt;
    if (!X.valid || comm_attached()) return dkmc_fail(13, "xt_get_srow: needs the X of a single-GPU solve", __FILE__, __LINE__);
    HIPCHK(hipStreamSynchronize(e.stream));
    if (ns_out) *ns_out = X.ns;
    if (srow_out && X.ns > 0) HIPCHK(hipMemcpy(srow_out, g_xb.srow, (size_t)X.ns * 4, hipMemcpyDeviceToHost));
    return 0;
}
extern "C" int dkmc_xt_get_diag(double *d_out)
{
    Engine &e = eng(); hipStream_t st = e.stream; const XTState &X = g_xt;
    if (!X.valid || comm_attached() || !d_out) return dkmc_fail(13, "xt_get_diag: needs the X of a single-GPU solve", __FILE__, __LINE__);
    for (int i = 0; i < X.Nsub; ++i) d_out[i] = 0.0;
    if (X.ns <= 0) return 0;
    double *ones = nullptr, *sums = nullptr;
    std::vector<double> h((size_t)X.ns); std::vector<int> srow((size_t)X.ns);
    auto body = [&]() -> int {
        HIPCHK(hipMalloc((void **)&ones, (size_t)X.ns_pad * 8)); HIPCHK(hipMalloc((void **)&sums, (size_t)X.ns_pad * 8));
        HIPCHK(hipMemsetAsync(ones, 0, (size_t)X.ns_pad * 8, st));
        hipLaunchKernelGGL(k_xt_fill_f64, dim3((X.ns + 255) / 256), dim3(256), 0, st, ones, (long long)X.ns, 1.0);
        if (int rc = xt_tile_sums<0>(ones, sums, 1)) return rc;
        HIPCHK(hipStreamSynchronize(st));
        HIPCHK(hipMemcpy(h.data(), sums, (size_t)X.ns * 8, hipMemcpyDeviceToHost));
        HIPCHK(hipMemcpy(srow.data(), g_xb.srow, (size_t)X.ns * 4, hipMemcpyDeviceToHost));
        return 0;
    };
    const int rc = body();
    if (ones) (void)hipFree(ones);
    if (sums) (void)hipFree(sums);
    if (rc) return rc;
    for (int s = 0; s < X.ns; ++s) d_out[srow[s]] = h[s];
    return e.err_code;
}
