// xt_live.h -- the LIVE VIEW of the tiled tunnelling block: the sweeps of the one-GPU preconditioned block-CG stream only the tiles that matter
// (dkmc_set_x_tile_drop(theta); included by xt.hip, which owns the tile list and its builders; xtb.hip launches on the view).
//
// The tunnelling block is dense by class and its entries are WKB factors that fall off steeply with lateral distance: most stored 32 x 256 tiles hold
// nothing the sweeps can see.  A stored tile is LIVE when any stored entry has sS_i |v_ij| sS_j >= theta (sS: the Jacobi scaling of this solve by S
// rank, v: the fp64 stored value).  Per solve, once the scaling is known:
//   k_xtl_census    one workgroup per stored tile: the largest scaled magnitude of each stored sub-block, from the FP64 STORE (the rule is stated on
//                   the fp64 value; the image's rounding, 2^-24, would move tiles that sit at the threshold) -> a live flag per tile, the cell mask of
//                   the live tiles (the stored mask, or 0), counts.  By default k_xtl_census_img stands in for it: the same census read from the fp32
//                   image, exact by a guard band and an fp64 re-read of the sub-blocks inside it (below)
//   scans           (scan.hip) over the cells: slots of the live tiles in the live list and of their sub-blocks in the compact image
//   k_xtl_compact   the fp32 sub-blocks of the live tiles, in tile-list order, into a second grow-only buffer -- layout of a sub-block unchanged
//                   (xt_tval32_pos); the tiles of a run stay contiguous, which the chain prefetch of k_xtb_apply relies on
//   k_xt_tile_list, k_xt_wrange, xt_build_items   the builders of the assembly on the live cell mask: a complete second launch view (tiles with the
//                   same k, w, mask and a new soff; items; nitem_w; wrange and the window lists; records) -- the view of a one-rank share whose tile list is the live list
// k_xtb_apply is not touched: it gets another tile list, item list and image pointer.
// SUB-BLOCK UNIT (dkmc_set_x_tile_drop_unit(1)): the same rule one level down -- a stored sub-block is live when one of its stored entries reaches theta,
// a tile when one of its sub-blocks is, so the SET OF LIVE TILES is the same in both units (tflag, k_xtl_zero_dead and the argument below stand as
// they are).  The census then writes the live tiles' REDUCED masks, the compaction copies the selected sub-blocks (source slot by the stored mask,
// destination slot by the live one), and the builders, being functions of the cell mask, give tiles with the reduced mask: k_xtb_apply walks them in
// its partial-tile branch.  A sub-block carries its row sums and its column sums (both triangles from one stored value): the operator stays symmetric.
// What stays on the full view and the fp64 store: the first product A y0, the diagonal, the scaling, the true-residual pass that ends every solve and
// every re-entry round.  The start vector goes through the right-hand side, so the perturbation acts on the correction only.
// The partial-sum arrays of the block loop are grid- and record-indexed and a launch rewrites only the cells of its own tiles: after a full-view launch
// the cells of the dead tiles hold that launch's sums, which the live view's fold would add -- xt_live_zero_dead clears exactly those cells (the dead
// tiles' 32 x so doubles each; the whole array is GBs at 9.4e5 sites).  Going back to the full view needs nothing: it rewrites every stored cell.
// That holds for the range fold (dkmc_set_x_fold_form(0)).  The list fold (the default) adds only the cells of the view's own tiles, which its launch has
// just written: the dead tiles' cells are never read and nothing clears them.
// AUTO MODE (dkmc_set_x_tile_drop_auto, on by default): with no explicit threshold set, a WARM-STARTED solve (it starts from the previous solution, so
// the dropped part acts on the correction only; from a zero start it acts on the whole solution and costs an fp64 re-entry round) whose stored X has at
// least XTL_DROP_GATE sub-blocks runs its sweeps on the live view at XTL_DROP_AUTO_THETA.  The gate is measured on whole supersteps, not chosen: the
// geometric midpoint between the largest size at which the live view does not gain and the smallest at which it does
// (tools/x_tile_drop_by_size.py -> profiles/x_tile_drop_by_size.jsonl; tests/test_x_tile_drop_rule.py holds the rule to those lines).
#pragma once

XLive g_xlive;

constexpr double XTL_DROP_AUTO_THETA = 1e-10;
constexpr long long XTL_DROP_GATE = 246272;        // sqrt(125 218 x 484 356): tile:5 does not gain, tile:7 does
// threshold of auto mode for a stored X of stored_subblocks sub-blocks; gate_override > 0 replaces the measured gate (test aid).  Host arithmetic only.
double xtl_drop_rule(long long stored_subblocks, long long gate_override)
{
    const long long gate = gate_override > 0 ? gate_override : XTL_DROP_GATE;
    return stored_subblocks > 0 && stored_subblocks >= gate ? XTL_DROP_AUTO_THETA : 0.0;
}
extern "C" double dkmc_xtl_drop_rule(long long stored_subblocks) { return xtl_drop_rule(stored_subblocks, eng().x_tile_drop_gate); }

__global__ __launch_bounds__(XT_NT) void k_xtl_census(int nK, const XTile *__restrict__ tiles, int sub_base, const double *__restrict__ tval,
                                                      const double *__restrict__ sS, double theta, int unit, unsigned *__restrict__ lcmask,
                                                      int *__restrict__ tflag, unsigned long long *__restrict__ cnt)
{
    // thread (q = tid / 32, c = tid % 32) owns column 32 q + c of the tile and walks its 32 rows (the map of k_xt_fill); cnt: live tiles, sub-blocks in
    // live tiles, sub-blocks live on their own (integer atomics: the sums do not depend on their order).  unit 1: a live tile's cell mask holds the
    // sub-blocks live on their own only (not empty: the tile's largest magnitude is one of theirs)
    __shared__ double rs[XT_R], mx[XT_C / XT_SBW];
    const XTile td = tiles[blockIdx.x];
    const int tid = threadIdx.x, q = tid >> 5, c = tid & 31;
    if (tid < XT_R) rs[tid] = sS[XT_R * td.k + tid];                           // < ns_pad: sS is padded (with zeros)
    __syncthreads();
    double m = 0.0;
    if ((td.mask >> q) & 1u) {
        const int sl = __popc(td.mask & ((1u << q) - 1u));
        const double *src = tval + ((size_t)(td.soff - sub_base) + sl) * XT_SUB + c;
        const double scc = sS[XT_C * td.w + XT_SBW * q + c];
#pragma unroll 8
        for (int r = 0; r < XT_R; ++r) m = fmax(m, (rs[r] * fabs(src[r * XT_SBW])) * scc);
    }
#pragma unroll
    for (int off = 16; off > 0; off >>= 1) m = fmax(m, __shfl_xor(m, off, WAVE));      // the 32 lanes of a sub-block
    if (c == 0) mx[q] = m;
    __syncthreads();
    if (tid == 0) {
        double tm = 0.0; int own = 0; unsigned lm = 0u;
#pragma unroll
        for (int u = 0; u < XT_C / XT_SBW; ++u) if ((td.mask >> u) & 1u) { tm = fmax(tm, mx[u]); if (mx[u] >= theta) { ++own; lm |= 1u << u; } }
        const bool live = tm >= theta;
        lcmask[(size_t)td.w * nK + td.k] = live ? (unit == 1 ? lm : td.mask) : 0u;
        tflag[blockIdx.x] = live ? 1 : 0;
        if (live) { atomicAdd(cnt, 1ull); atomicAdd(cnt + 1, (unsigned long long)__popc(td.mask)); }
        if (own) atomicAdd(cnt + 2, (unsigned long long)own);
    }
}
// THE SAME CENSUS FROM THE FP32 IMAGE, EXACT (census form 1): half the bytes of the fp64 store.  The rule stays the one on the fp64 value; the image
// decides a sub-block only where its rounding cannot matter, and the sub-blocks it cannot decide are read again from the fp64 store.
//   v32 = float(v64), round to nearest: for a normal float |v64 - v32| <= 2^-24 |v32|; a v64 that rounds to zero or a subnormal has |v64| < FLT_MIN.
//   e(x) = fl(fl(rs x) scc), the census's two fp64 products, is monotone non-decreasing in x (each rounding is).  With a = |v32|:
//     e(|v64|) <= e(a (1 + 2^-24)) <= e(a) (1 + 2^-24)(1 + 2^-51) < e(a) (1 + 2^-22)        (a normal; with max(a, FLT_MIN) for the others)
//     e(|v64|) >= e(a (1 - 2^-24)) >= e(a) (1 - 2^-24)(1 - 2^-51) > e(a) (1 - 2^-22)        (a normal)
//   up = max over the sub-block of e(max(a, FLT_MIN)), lo = max over its NORMAL floats of e(a):
//     up (1 + 2^-22) <  theta  ->  every e(|v64|) < theta: DEAD, as the fp64 census finds
//     lo (1 - 2^-22) >= theta  ->  one e(|v64|) >= theta: LIVE, as the fp64 census finds
//     otherwise the 32 lanes read the fp64 sub-block and apply k_xtl_census's test itself (cnt[3] counts these sub-blocks).
//   (the relative bounds need the products to be normal doubles: the host takes this form only for theta >= 1e-290, far above where fp64 goes subnormal.)
// The maximum does not depend on the order: the lanes take the image by float4 (lane l of a sub-block's 32, load it: float4 32 it + l = rows
// 8 (it / 2) + 2 (it % 2) + l / 16 and + 4, columns 2 (l % 16) and + 1: xt_tval32_pos), 8 coalesced loads per sub-block.
__global__ __launch_bounds__(XT_NT) void k_xtl_census_img(int nK, const XTile *__restrict__ tiles, int sub_base, const double *__restrict__ tval,
                                                          const float4 *__restrict__ tval32, const double *__restrict__ sS, double theta, int unit,
                                                          unsigned *__restrict__ lcmask, int *__restrict__ tflag, unsigned long long *__restrict__ cnt)
{
    constexpr double BAND = 1.0 / 4194304.0, FMIN = 1.1754943508222875e-38, FMAX = 3.4028234663852886e+38;
    __shared__ double rs[XT_R]; __shared__ int lvq[XT_C / XT_SBW];
    const XTile td = tiles[blockIdx.x];
    const int tid = threadIdx.x, q = tid >> 5, l = tid & 31;
    if (tid < XT_R) rs[tid] = sS[XT_R * td.k + tid];
    __syncthreads();
    const bool present = (td.mask >> q) & 1u;
    const size_t slot = (size_t)(td.soff - sub_base) + __popc(td.mask & ((1u << q) - 1u));
    double up = 0.0, lo = 0.0;
    if (present) {
        const float4 *src = tval32 + slot * (XT_SUB / 4) + l;
        const double s0 = sS[XT_C * td.w + XT_SBW * q + 2 * (l & 15)], s1 = sS[XT_C * td.w + XT_SBW * q + 2 * (l & 15) + 1];
        auto one = [&](float v, double r, double sc) {
            const double a = fabs((double)v);
            up = fmax(up, (r * fmax(a, FMIN)) * sc);
            if (a >= FMIN && a <= FMAX) lo = fmax(lo, (r * a) * sc);
        };
#pragma unroll
        for (int it = 0; it < 8; ++it) {
            const float4 v = src[it * 32];
            const int r0 = 8 * (it >> 1) + 2 * (it & 1) + (l >> 4);
            const double ra = rs[r0], rb = rs[r0 + 4];
            one(v.x, ra, s0); one(v.y, ra, s1); one(v.z, rb, s0); one(v.w, rb, s1);
        }
    }
#pragma unroll
    for (int off = 16; off > 0; off >>= 1) { up = fmax(up, __shfl_xor(up, off, WAVE)); lo = fmax(lo, __shfl_xor(lo, off, WAVE)); }      // the 32 lanes of a sub-block
    // (the same decision in all 32 lanes)
    const bool dead = up * (1.0 + BAND) < theta, sure = lo * (1.0 - BAND) >= theta;
    const bool again = present && !dead && !sure;
    double m = 0.0;
    if (again) {                                                               // k_xtl_census's own pass over this sub-block: lane l owns column l
        const double *src = tval + slot * XT_SUB + l;
        const double scc = sS[XT_C * td.w + XT_SBW * q + l];
#pragma unroll 8
        for (int r = 0; r < XT_R; ++r) m = fmax(m, (rs[r] * fabs(src[r * XT_SBW])) * scc);
    }
#pragma unroll
    for (int off = 16; off > 0; off >>= 1) m = fmax(m, __shfl_xor(m, off, WAVE));
    const bool lives = again ? m >= theta : (present && sure);
    if (l == 0) lvq[q] = again ? (lives ? 2 : -1) : (lives ? 1 : 0);           // > 0 live, <= 0 dead or absent; 2 / -1: decided by the fp64 pass
    __syncthreads();
    if (tid == 0) {
        int own = 0, re = 0; unsigned lm = 0u;
#pragma unroll
        for (int u = 0; u < XT_C / XT_SBW; ++u) { if (lvq[u] > 0) { ++own; lm |= 1u << u; } if (lvq[u] == 2 || lvq[u] == -1) ++re; }
        const bool live = own > 0;
        lcmask[(size_t)td.w * nK + td.k] = live ? (unit == 1 ? lm : td.mask) : 0u;
        tflag[blockIdx.x] = live ? 1 : 0;
        if (live) { atomicAdd(cnt, 1ull); atomicAdd(cnt + 1, (unsigned long long)__popc(td.mask)); }
        if (own) atomicAdd(cnt + 2, (unsigned long long)own);
        if (re) atomicAdd(cnt + 3, (unsigned long long)re);
    }
}
// one workgroup per stored tile: a live tile's selected fp32 sub-blocks (1024 floats = 256 float4 each; lcmask: all of them, or the live ones -- a
// subset of the stored mask) to their slots in the compact image: from the slot counted on the STORED mask to the slot counted on the LIVE mask
__global__ __launch_bounds__(XT_NT) void k_xtl_compact(int nK, const XTile *__restrict__ tiles, int sub_base, const unsigned *__restrict__ lcmask,
                                                       const int *__restrict__ lsoff, const float4 *__restrict__ src32, float4 *__restrict__ dst32)
{
    const XTile td = tiles[blockIdx.x];
    const size_t ci = (size_t)td.w * nK + td.k;
    const unsigned lm = lcmask[ci] & td.mask;
    if (!lm) return;
    const float4 *s = src32 + (size_t)(td.soff - sub_base) * (XT_SUB / 4) + threadIdx.x;
    float4 *d = dst32 + (size_t)lsoff[ci] * (XT_SUB / 4) + threadIdx.x;
    int dl = 0;
#pragma unroll
    for (int q = 0; q < XT_C / XT_SBW; ++q)
        if ((lm >> q) & 1u) { d[(size_t)dl * (XT_SUB / 4)] = s[(size_t)__popc(td.mask & ((1u << q) - 1u)) * (XT_SUB / 4)]; ++dl; }
}
// the DEAD tiles' cells of the block loop's grid-indexed row sums (per = 32 x so doubles per cell) <- 0; one thread per double of a stored tile's cell
__global__ __launch_bounds__(XT_NT) void k_xtl_zero_dead(long long n, int per, int nW, const XTile *__restrict__ tiles, const int *__restrict__ tflag,
                                                         double *__restrict__ rowpartB)
{
    const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const int t = (int)(i / per);
    if (tflag[t]) return;
    const XTile td = tiles[t];
    rowpartB[((size_t)td.k * nW + td.w) * per + (size_t)(i % per)] = 0.0;
}

static hipEvent_t g_xl_ev[3]; static bool g_xl_ev_ready = false;

// census of the resident X (one GPU: this rank holds every tile) against theta with the scaling sS (device, by S rank, padded): lcmask (cells),
// tflag (stored tiles) and the counts h4 (host; [3]: sub-blocks the image form read again from the fp64 store) -- the stream is synchronised.
// unit: what lcmask holds for a live tile (k_xtl_census).  Form (dkmc_debug_xtl_census_form): 1 = from the fp32 image with the guard band, where
// there is an image and theta is in the band's range; 0 = from the fp64 store.  Same flags, masks and counts by construction.
static long long g_xtl_reread = 0;       // cnt[3] of the last census
static int xt_live_census(double theta, int unit, const double *sS, unsigned **lcmask_out, int **tflag_out, unsigned long long *h4)
{
    Engine &e = eng(); hipStream_t st = e.stream; const XTState &X = g_xt;
    const long long ncell = (long long)X.nK * X.nW;
    unsigned *lcmask = (unsigned *)scratch(S_XTL_CELLS, (size_t)(ncell + 4) * 4 * 3);
    int *tflag = (int *)scratch(S_XTL_TFLAG, (size_t)(X.ntiles + 8) * 4 + 32);
    if (!lcmask || !tflag) return e.err_code;
    unsigned long long *cnt = reinterpret_cast<unsigned long long *>(tflag + ((X.ntiles + 7) & ~7));      // (8-byte aligned: the slot is, and the offset is a multiple of 8 ints; 32 bytes fit: (ntiles + 7) * 4 + 32 <= the slot)
    HIPCHK(hipMemsetAsync(lcmask, 0, (size_t)(ncell + 4) * 4, st));
    HIPCHK(hipMemsetAsync(cnt, 0, 32, st));
    if (e.xtl_census_form == 1 && g_xb.tval32 && theta >= 1e-290)
        hipLaunchKernelGGL(k_xtl_census_img, dim3(X.ntiles), dim3(XT_NT), 0, st, X.nK, (const XTile *)g_xb.tiles, (int)X.sub_base, (const double *)g_xb.tval,
                           reinterpret_cast<const float4 *>(g_xb.tval32), sS, theta, unit, lcmask, tflag, cnt);
    else
        hipLaunchKernelGGL(k_xtl_census, dim3(X.ntiles), dim3(XT_NT), 0, st, X.nK, (const XTile *)g_xb.tiles, (int)X.sub_base, (const double *)g_xb.tval, sS, theta,
                           unit, lcmask, tflag, cnt);
    KCHK();
    HIPCHK(hipMemcpyAsync(h4, cnt, 32, hipMemcpyDeviceToHost, st));
    HIPCHK(hipStreamSynchronize(st));
    g_xtl_reread = (long long)h4[3];
    *lcmask_out = lcmask; *tflag_out = tflag;
    return 0;
}
extern "C" int dkmc_debug_xtl_census_form(int form) { const int was = eng().xtl_census_form; eng().xtl_census_form = form == 1 ? 1 : 0; return was; }
extern "C" long long dkmc_debug_xtl_census_reread(void) { return g_xtl_reread; }

// Builds the live view of the resident X for this solve into lv (state, the launch view, the report).  Never an error for a view that is not worth
// having or does not fit: the caller streams the existing image then (state -2 / -1).  unit 0: whole tiles, 1: the live sub-blocks of the live tiles.
int xt_live_build(double theta, int unit, const double *sS, XLive *lv)
{
    Engine &e = eng(); hipStream_t st = e.stream; const XTState &X = g_xt;
    *lv = XLive{};
    if (!(theta > 0.0) || !X.valid || comm_attached() || X.tile_n != X.ntiles || X.ntiles <= 0 || !g_xb.tval32 || !sS) return 0;
    const bool prof = e.profiling != 0;
    if (prof && !g_xl_ev_ready) { for (auto &ev : g_xl_ev) HIPCHK(hipEventCreate(&ev)); g_xl_ev_ready = true; }
    if (prof) HIPCHK(hipEventRecord(g_xl_ev[0], st));
    const int nK = X.nK, nW = X.nW;
    const long long ncell = (long long)nK * nW;
    unsigned *lcmask = nullptr; int *tflag = nullptr; unsigned long long h3[4] = {0, 0, 0, 0};
    if (int rc = xt_live_census(theta, unit, sS, &lcmask, &tflag, h3)) return rc;
    lv->tflag = tflag;
    lv->info[1] = X.ntiles; lv->info[2] = (long long)h3[0]; lv->info[3] = X.nsub_total; lv->info[4] = (long long)h3[1]; lv->info[5] = (long long)h3[2];
    const int nlive = (int)h3[0]; const long long nsub_live = (long long)h3[unit == 1 ? 2 : 1];      // the sub-blocks streamed
    // every tile live, or none dead enough to matter (fewer than 1 / 64 of the sub-blocks would go): the existing image and views
    if ((X.nsub_total - nsub_live) * 64 < X.nsub_total) { lv->state = -2; return 0; }
    int *ltoff = (int *)lcmask + (ncell + 4), *lsoff = ltoff + (ncell + 4);
    hipLaunchKernelGGL(k_xt_cell_counts, dim3((unsigned)((ncell + 255) / 256)), dim3(256), 0, st, ncell, (const unsigned *)lcmask, ltoff, lsoff);
    if (int rc = dkmc_exclusive_scan_i32(ltoff, ltoff, (int)ncell, ltoff + ncell)) return rc;
    if (int rc = dkmc_exclusive_scan_i32(lsoff, lsoff, (int)ncell, lsoff + ncell)) return rc;
    if (prof) HIPCHK(hipEventRecord(g_xl_ev[1], st));
    const size_t bytes = (size_t)(nsub_live + 4) * XT_SUB * 4;                 // (the slack of the full image: the product requests two sub-blocks beyond a full tile)
    float *c32 = (float *)scratch_try(S_XTL_TVAL32, bytes);
    if (!c32) { lv->state = -1; return 0; }
    XTile *ltiles = (XTile *)scratch(S_XTL_TILES, (size_t)(nlive + 1) * sizeof(XTile));
    int2 *lwrange = (int2 *)scratch(S_XTL_WRANGE, (size_t)(nK + 4) * sizeof(int2));
    int *lwlist = (int *)scratch(S_XTL_WLIST, ((size_t)nK * (nW + 1) + 4) * sizeof(int));
    if (!ltiles || !lwrange || !lwlist) return e.err_code;
    hipLaunchKernelGGL(k_xtl_compact, dim3(X.ntiles), dim3(XT_NT), 0, st, nK, (const XTile *)g_xb.tiles, (int)X.sub_base, (const unsigned *)lcmask, (const int *)lsoff,
                       reinterpret_cast<const float4 *>(g_xb.tval32), reinterpret_cast<float4 *>(c32));
    hipLaunchKernelGGL(k_xt_tile_list, dim3((unsigned)((ncell + 255) / 256)), dim3(256), 0, st, nK, ncell, (const unsigned *)lcmask, (const int *)ltoff, (const int *)lsoff, ltiles);
    hipLaunchKernelGGL(k_xt_wrange, dim3((nK + 255) / 256), dim3(256), 0, st, nK, nW, (const unsigned *)lcmask, lwrange, lwlist);
    KCHK();
    XShare sh{};
    if (int rc = xt_build_items(nK, nW, X.kc, nlive, nsub_live, ltoff, ltiles, 1, 0, S_XTL_NITEMW, S_XTL_ITEMS, S_XTL_SPLIT, &sh, 2)) return rc;
    if ((sh.item_lo | sh.item_n) & 3) return dkmc_fail(48, "live view: run list not padded to groups of four", __FILE__, __LINE__);
    if (prof) {
        HIPCHK(hipEventRecord(g_xl_ev[2], st));
        HIPCHK(hipEventSynchronize(g_xl_ev[2]));
        float ms = 0.f;
        HIPCHK(hipEventElapsedTime(&ms, g_xl_ev[0], g_xl_ev[1])); lv->ms[0] = ms;
        HIPCHK(hipEventElapsedTime(&ms, g_xl_ev[1], g_xl_ev[2])); lv->ms[1] = ms;
    }
    lv->tiles = ltiles; lv->items = sh.items ? sh.items + sh.item_lo : nullptr; lv->item_n = sh.item_n; lv->wrange = lwrange; lv->wlist = lwlist; lv->nitem_w = sh.nitem_w;
    lv->nrecords = sh.nitems >> sh.rec_shift; lv->nitems = sh.nitems; lv->tval32 = c32;
    lv->info[6] = (long long)bytes;
    lv->state = 1;
    return 0;
}
// after a full-view launch of the block loop's tile kernel, before the first on the live view (see the head of this file); so: vectors per row of rowpartB
void xt_live_zero_dead(const XLive &lv, double *rowpartB, int so)
{
    const XTState &X = g_xt;
    if (lv.info[2] >= X.ntiles) return;
    const int per = XT_R * so;
    const long long n = (long long)X.ntiles * per;
    hipLaunchKernelGGL(k_xtl_zero_dead, dim3((unsigned)((n + XT_NT - 1) / XT_NT)), dim3(XT_NT), 0, eng().stream, n, per, X.nW, (const XTile *)g_xb.tiles, lv.tflag, rowpartB);
}

// ---- report and test aids (include/devicekmc_hip_debug.h) --------------------------------------------------------------------------------
extern "C" int dkmc_get_x_tile_live_info(long long *info8, double *ms2)
{
    if (info8) { for (int c = 0; c < 8; ++c) info8[c] = g_xlive.info[c]; info8[0] = g_xlive.state; }
    if (ms2 && eng().profiling) { ms2[0] = g_xlive.ms[0]; ms2[1] = g_xlive.ms[1]; }
    return 0;
}
// the window lists (XTBuffers::wlist) of the last one-GPU assembly, or of the live view the last solve ran on
extern "C" int dkmc_xt_get_fold_lists(int live, int *nK_out, int *nW_out, int *rows)
{
    Engine &e = eng(); const XTState &X = g_xt;
    if (!X.valid || comm_attached() || X.tile_n != X.ntiles || !g_xb.wlist) return dkmc_fail(13, "xt_get_fold_lists: needs the X of a single-GPU solve", __FILE__, __LINE__);
    if (live && (g_xlive.state != 1 || !g_xlive.wlist)) return dkmc_fail(13, "xt_get_fold_lists: the last solve had no live view", __FILE__, __LINE__);
    HIPCHK(hipStreamSynchronize(e.stream));
    if (nK_out) *nK_out = X.nK;
    if (nW_out) *nW_out = X.nW;
    if (rows && X.nK > 0) HIPCHK(hipMemcpy(rows, live ? g_xlive.wlist : (const int *)g_xb.wlist, (size_t)X.nK * (X.nW + 1) * sizeof(int), hipMemcpyDeviceToHost));
    return 0;
}
// the scaling by S rank of the last one-GPU solve (device, padded), or null
static const double *xt_live_sS()
{
    const double *vS = (const double *)eng().buf[S_CG_PS];
    return vS ? vS + g_xt.ns_pad : nullptr;
}
extern "C" int dkmc_xt_get_live(double theta, int *live_per_tile, double *sS_out)
{
    Engine &e = eng(); const XTState &X = g_xt;
    const double *sS = xt_live_sS();
    if (!X.valid || comm_attached() || X.tile_n != X.ntiles || X.ntiles <= 0 || !sS) return dkmc_fail(13, "xt_get_live: needs the X of a single-GPU solve", __FILE__, __LINE__);
    unsigned *lcmask = nullptr; int *tflag = nullptr; unsigned long long h3[4];
    if (int rc = xt_live_census(theta, 0, sS, &lcmask, &tflag, h3)) return rc;
    if (live_per_tile) HIPCHK(hipMemcpy(live_per_tile, tflag, (size_t)X.ntiles * 4, hipMemcpyDeviceToHost));
    if (sS_out) HIPCHK(hipMemcpy(sS_out, sS, (size_t)X.ns * 8, hipMemcpyDeviceToHost));
    return e.err_code;
}
// the sub-block unit's live mask of every stored tile (0: dead tile), from the same census
__global__ void k_xtl_tile_masks(int ntiles, int nK, const XTile *__restrict__ tiles, const unsigned *__restrict__ lcmask, int *__restrict__ out)
{
    const int t = blockIdx.x * blockDim.x + threadIdx.x;
    if (t < ntiles) out[t] = (int)lcmask[(size_t)tiles[t].w * nK + tiles[t].k];
}
extern "C" int dkmc_xt_get_live_masks(double theta, int *mask_per_tile)
{
    Engine &e = eng(); const XTState &X = g_xt;
    const double *sS = xt_live_sS();
    if (!X.valid || comm_attached() || X.tile_n != X.ntiles || X.ntiles <= 0 || !sS) return dkmc_fail(13, "xt_get_live_masks: needs the X of a single-GPU solve", __FILE__, __LINE__);
    unsigned *lcmask = nullptr; int *tflag = nullptr; unsigned long long h3[4];
    if (int rc = xt_live_census(theta, 1, sS, &lcmask, &tflag, h3)) return rc;
    if (mask_per_tile) {
        // (tflag has served: the masks take its place, tile by tile)
        hipLaunchKernelGGL(k_xtl_tile_masks, dim3((X.ntiles + 255) / 256), dim3(256), 0, e.stream, X.ntiles, X.nK, (const XTile *)g_xb.tiles, (const unsigned *)lcmask, tflag);
        KCHK();
        HIPCHK(hipMemcpyAsync(mask_per_tile, tflag, (size_t)X.ntiles * 4, hipMemcpyDeviceToHost, e.stream));
        HIPCHK(hipStreamSynchronize(e.stream));
    }
    return e.err_code;
}
// xtb.hip (dkmc_xtb_tile_product and dkmc_xtb_time_apply_stored with stored_bytes = -4): the live view of the resident X at the current theta and unit,
// built afresh into *lv; state 1 or an error
int xt_live_for_test(XLive *lv)
{
    const double *sS = xt_live_sS();
    if (int rc = xt_live_build(eng().x_tile_drop, eng().x_tile_drop_unit, sS, lv)) return rc;
    if (lv->state != 1) return dkmc_fail(13, "no live image at the current threshold and unit (dkmc_set_x_tile_drop; dkmc_get_x_tile_live_info)", __FILE__, __LINE__);
    return 0;
}
