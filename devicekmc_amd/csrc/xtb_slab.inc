// xtb_slab.inc -- the block-CG of the current solve with its STATE distributed by spatial row slabs (SURVEY 8(e): "row slabs; halo = sites
// within 3.5 A of a cut; fused all-reduce of a few doubles per iteration").  Included by xtb.hip; no counterpart in the reference (single GPU:
// kmc_main.cpp:35-37 selects one device, Device.h:20 has its mpi.h commented out).
//
// The all-gather variant above (xtb_cg with A.sharded, dkmc_set_x_slab(0)) shards the tile stream only: every rank still runs the neighbour
// part, the Gram pass and the panel updates over ALL rows -- 0.86 ms of a 4.35 ms sweep at 9.4e5 sites, which caps 8 ranks at 3x.  Here a rank
// OWNS the rows of one lateral slab of the device (atoms binned along the wider lateral axis, cuts balanced by row count) and only its rows
// of R, P, T, y are ever current on it:
//   tiles            as before: a rank streams the tiles of its column windows (k_xtb_apply) and folds its partial sums of EVERY S row;
//   exchange 1       all-to-all-v: the partial sums of the S rows rank d owns go to d (+ the two driver rows' partials + the abort word);
//   rows / Gram      the owner adds the N partials IN RANK ORDER, finishes its rows of T, forms its partial Gram matrices (k_xtb_rows_slab);
//   exchange 2       all-gather of 6 x 256 doubles + the abort word per rank; every rank adds the blocks in rank order (k_xtb_small): the same
//                    s x s algebra, the same stop decision on every rank -- no stop word has to travel;
//   step             R, P, y of the own rows (k_xtb_step over the rank's row list); Q = S P of the own S rows;
//   exchange 3       all-to-all-v: the own rows of QS to everybody (the tile pass of every rank reads all of S) + the P rows a neighbour slab
//                    reads (halo: own rows with a neighbour-part entry in a row of that slab; the pattern of X is symmetric, so the same
//                    test on replicated data gives the sender's and the receiver's list).
// The two driver rows (thousands of entries across all slabs) are REPLICATED: every rank forms its partial sums over the columns it owns, the
// partials travel with exchange 1 and every rank adds them in rank order -- identical driver rows everywhere, counted in the Gram matrices by
// rank 0 only.  Memory is not distributed (the panels keep their full length on every rank, 0.36 GB at 9.4e5 sites): what is distributed is the
// work and the traffic; rows a rank neither owns nor reads are simply never touched.
// Exchanges at N = 8, 9.4e5 sites: 1.5 MB per pair in exchanges 1 and 3 (against one 11.9 MB slot from every peer in the all-gather variant).
//
// The same host loop runs N VIRTUAL ranks inside one process (emulation on one GPU: dkmc_xtb_emulate_slabs) -- every virtual rank with its own
// panels, lists and exchange buffers, the exchanges as device copies -- which is how the partition, the lists and the rank-order sums are
// tested for N = 2, 5, 8 on the one-GPU development box, and how the per-rank kernel times of the strong-scaling model are measured.
// Partition, halo lists, virtual ranks' buffers and emulated exchanges: slab.h, shared with the K loop; the offsets (SlabMeta): slab_plan.h
#define XS_DRV (2 * XB_SP)                           // the two driver rows' partial sums in a piece of exchange 1
#define XS_GSTR (XB_NG * 256 + 2)                    // one rank's block of exchange 2: partial Gram matrices, spare, abort word

struct SlabMeta {                                    // by value to the pack / unpack kernels (device tables would need a copy per solve and rank)
    int nr, me;
    int soffs[XS_MAXR + 1];                          // S ranks of owner r: S_by_owner[soffs[r] ... soffs[r + 1])
    int rowoff[XS_MAXR + 1];                         // rows >= 2 of owner r: rows_by_owner[rowoff[r] ...)
    int hsoff[XS_MAXR + 1];                          // halo rows this rank sends to d: hsend[hsoff[d] ...)
    int hroff[XS_MAXR + 1];                          // halo rows this rank receives from s: hrecv[hroff[s] ...)
    long long p3s[XS_MAXR + 1], p3r[XS_MAXR + 1];    // piece offsets (doubles) of exchange 3 in the send / receive buffer
};

__global__ void k_slab_flag_S(int ns, const int *__restrict__ srow, const int *__restrict__ owner, int r, int *__restrict__ flag)
{
    const int q = blockIdx.x * blockDim.x + threadIdx.x;
    if (q < ns) flag[q] = owner[srow[q]] == r ? 1 : 0;
}
// S_by_owner[base + pos] = q; sdst[q] = where S rank q's so partial sums start in a rank's send buffer of exchange 1 (piece of owner r: the S rows
// of r in list order, then XS_DRV + 2 tail words)
__global__ void k_slab_scatter_S(int ns, const int *__restrict__ flag, const int *__restrict__ pos, int base, int r, int so, int *__restrict__ S_by_owner, long long *__restrict__ sdst)
{
    const int q = blockIdx.x * blockDim.x + threadIdx.x;
    if (q < ns && flag[q]) { const int j = base + pos[q]; S_by_owner[j] = q; sdst[q] = (long long)j * so + (long long)(XS_DRV + 2) * r; }
}
// entries of the two driver rows whose column rank `me` owns (the drivers' own columns 0 / 1: rank 0)
__global__ void k_slab_flag_drv(int n, const int *__restrict__ ci, const int *__restrict__ owner, int me, int *__restrict__ flag)
{
    const int p = blockIdx.x * blockDim.x + threadIdx.x;
    if (p < n) { const int c = ci[p]; flag[p] = ((c < 2 ? 0 : owner[c]) == me) ? 1 : 0; }
}
__global__ void k_slab_scatter_drv(int n, const int *__restrict__ flag, const int *__restrict__ pos, int *__restrict__ dlist)
{
    const int p = blockIdx.x * blockDim.x + threadIdx.x;
    if (p < n && flag[p]) dlist[pos[p]] = p;
}
__global__ void k_slab_steplist(int n_own, const int *__restrict__ own_rows, int *__restrict__ steplist)
{
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n_own + 2) steplist[i] = i < 2 ? i : own_rows[i - 2];
}

// tail of every piece of exchange 1: the two driver rows' partial sums over this rank's columns (the XB_DSPLIT slices added in a fixed order) and
// the control words (spare, abort)
__global__ void k_xtb_slab_tail(int nr, int so, SlabMeta M, const double *__restrict__ drvpart, const XCtrl *ctrl, double *__restrict__ send1)
{
    const int d = blockIdx.x, t = threadIdx.x;       // XS_DRV + 2 threads
    if (d >= nr || t >= XS_DRV + 2) return;
    double *tail = send1 + (size_t)M.soffs[d + 1] * so + (size_t)(XS_DRV + 2) * d;
    if (t < XS_DRV) {
        const int row = t / XB_SP, v = t % XB_SP;
        double sd = 0.0;
#pragma unroll
        for (int w = 0; w < XB_DSPLIT; ++w) sd += drvpart[(row * XB_DSPLIT + w) * XB_SP + v];
        tail[t] = sd;
    } else tail[t] = (t == XS_DRV + 1 && ctrl->abort_local) ? 1.0 : 0.0;
}
__global__ void k_xtb_slab_gtail(const XCtrl *ctrl, double *__restrict__ gblock) { gblock[XB_NG * 256] = 0.0; gblock[XB_NG * 256 + 1] = ctrl->abort_local ? 1.0 : 0.0; }

// ---- row kernel of a slab rank: recv1 = one piece per rank (rank order), each [nSme x so partial sums of MY S rows | XS_DRV driver partials | 2 control words]
// MODE (split polynomial preconditioner, dkmc_set_x_slab_poly): XS_FOLD -- the fold alone (the analogue of k_xtb_fold_rows): my S rows and the driver
// rows of T completed from the partials, no Gram matrices; XS_NF -- T is final in every row (folded, then carried through L), the pass only forms R
// (INIT) and the partial Gram matrices (the analogue of k_xtb_rows<..., NF = 1>)
#define XS_FOLD 1
#define XS_NF 2
template <int INIT, int MODE = 0>
__global__ __launch_bounds__(XT_NT) void k_xtb_rows_slab(int nSme, const int *__restrict__ slist, int nlist, const int *__restrict__ rowlist, int s, int so, int nr, int me,
                                                         const double *__restrict__ recv1, const int *__restrict__ srow, const double *__restrict__ sS,
                                                         const int *__restrict__ nsrank, const double *__restrict__ sc, double *__restrict__ T,
                                                         const double *__restrict__ P, double *__restrict__ R, const double *__restrict__ b,
                                                         double *__restrict__ gpart, XCtrl *ctrl, int it,
                                                         const XbAux *__restrict__ aux, const double *__restrict__ ax, const double *__restrict__ ay, const double *__restrict__ az)
{
    const size_t piece = (size_t)nSme * so + XS_DRV + 2;
    __shared__ double lg[4][XB_NG / 2][4][64];
    __shared__ int sdone;
    if (threadIdx.x == 0) {
        sdone = ctrl->done;
        if (!sdone) {
            bool ab = false;
            for (int r = 0; r < nr; ++r) ab |= recv1[r * piece + (size_t)nSme * so + XS_DRV + 1] != 0.0;
            if (ab) { sdone = 1; if (blockIdx.x == 0) { ctrl->done = it + 1 > 0 ? it + 1 : 1; ctrl->aborted = 1; } }
        }
    }
    __syncthreads();
    if (sdone) return;
    const int v = threadIdx.x & 15, r4 = threadIdx.x >> 4;
    const int wv = threadIdx.x >> 6, lane = threadIdx.x & 63;
    dbl4 G[XB_NG];
#pragma unroll
    for (int g = 0; g < XB_NG; ++g) G[g] = (dbl4)(0.0);
    // ---- my S rows, 32 list entries per step: the N partial sums of a row in rank order ----
    const int nKb = (nSme + XT_R - 1) / XT_R;
    for (int kb = blockIdx.x; kb < nKb; kb += gridDim.x) {
        const int jA = XT_R * kb + r4, jB = jA + 16;
        double tA = 0.0, tB = 0.0;
        if (MODE != XS_NF && v < so)
            for (int r = 0; r < nr; ++r) {
                if (jA < nSme) tA += recv1[r * piece + (size_t)jA * so + v];
                if (jB < nSme) tB += recv1[r * piece + (size_t)jB * so + v];
            }
        double pA = 0.0, pB = 0.0, rA = 0.0, rB = 0.0;
        if (jA < nSme) {
            const int q = slist[jA], row = srow[q]; const size_t o = (size_t)row * XB_SP + v;
            if (MODE == XS_NF) tA = T[o]; else { tA = sS[q] * (T[o] + tA); T[o] = tA; }
            if (MODE != XS_FOLD) { if (INIT) { rA = tA - xtb_rhs(b, row, v, s, aux, ax, ay, az, sc); R[o] = rA; } else { pA = P[o]; rA = R[o]; } }
        } else tA = 0.0;
        if (jB < nSme) {
            const int q = slist[jB], row = srow[q]; const size_t o = (size_t)row * XB_SP + v;
            if (MODE == XS_NF) tB = T[o]; else { tB = sS[q] * (T[o] + tB); T[o] = tB; }
            if (MODE != XS_FOLD) { if (INIT) { rB = tB - xtb_rhs(b, row, v, s, aux, ax, ay, az, sc); R[o] = rB; } else { pB = P[o]; rB = R[o]; } }
        } else tB = 0.0;
        if (MODE == XS_FOLD) continue;
        if (!INIT) {
            G[0] = XB_MFMA(pA, tA, G[0]); G[1] = XB_MFMA(pA, rA, G[1]); G[2] = XB_MFMA(tA, rA, G[2]); G[3] = XB_MFMA(tA, tA, G[3]); G[5] = XB_MFMA(pA, pA, G[5]);
            G[0] = XB_MFMA(pB, tB, G[0]); G[1] = XB_MFMA(pB, rB, G[1]); G[2] = XB_MFMA(tB, rB, G[2]); G[3] = XB_MFMA(tB, tB, G[3]); G[5] = XB_MFMA(pB, pB, G[5]);
        }
        G[4] = XB_MFMA(rA, rA, G[4]); G[4] = XB_MFMA(rB, rB, G[4]);
    }
    // ---- the two driver rows: finished identically on EVERY rank from the ranks' partials in rank order (workgroup 0, r4 = row);
    // only rank 0 counts them in the Gram matrices ----
    if (blockIdx.x == 0) {
        double t_ = 0.0, p_ = 0.0, r_ = 0.0;
        if (r4 < 2) {
            const int row = r4; const size_t o = (size_t)row * XB_SP + v;
            if (MODE == XS_NF) t_ = T[o];
            else {
                double sd = 0.0;
                for (int r = 0; r < nr; ++r) sd += recv1[r * piece + (size_t)nSme * so + row * XB_SP + v];
                t_ = sc[row] * sd; T[o] = t_;
            }
            if (MODE == XS_FOLD) {}
            else if (INIT) { r_ = t_ - xtb_rhs(b, row, v, s, aux, ax, ay, az, sc); R[o] = r_; } else { p_ = P[o]; r_ = R[o]; }
            if (me != 0) { t_ = 0.0; p_ = 0.0; r_ = 0.0; }
        }
        if (!INIT) { G[0] = XB_MFMA(p_, t_, G[0]); G[1] = XB_MFMA(p_, r_, G[1]); G[2] = XB_MFMA(t_, r_, G[2]); G[3] = XB_MFMA(t_, t_, G[3]); G[5] = XB_MFMA(p_, p_, G[5]); }
        G[4] = XB_MFMA(r_, r_, G[4]);
    }
    if (MODE == XS_FOLD) return;                                               // (uniform over the workgroup)
    // ---- my other rows (finished by k_xtb_neigh) ----
    if (nlist > 0) {
        const int chunk = ((nlist + (int)gridDim.x - 1) / (int)gridDim.x + 3) & ~3;
        const int i0 = blockIdx.x * chunk, i1 = min(nlist, i0 + chunk);
        for (int r0 = i0 + 4 * wv; r0 < i1; r0 += 64) {
            double tv[4], pv[4], rv[4]; int sr[4], rw[4];
#pragma unroll
            for (int u = 0; u < 4; ++u) {
                const int pos = r0 + 16 * u + (lane >> 4);
                const bool in = pos < i1;
                rw[u] = rowlist[in ? pos : i0];
                const size_t o = (size_t)rw[u] * XB_SP + v;
                sr[u] = in ? nsrank[rw[u]] : 0;
                tv[u] = T[o];
                if (!INIT) { pv[u] = P[o]; rv[u] = R[o]; }
            }
#pragma unroll
            for (int u = 0; u < 4; ++u) {
                const int pos = r0 + 16 * u + (lane >> 4);
                if (r0 + 16 * u >= i1) break;                                 // uniform over the wave
                const bool use = pos < i1 && sr[u] < 0;
                const size_t o = (size_t)rw[u] * XB_SP + v;
                double t_ = use ? tv[u] : 0.0, p_ = 0.0, r_ = 0.0;
                if (INIT) { if (use) { r_ = t_ - xtb_rhs(b, rw[u], v, s, aux, ax, ay, az, sc); R[o] = r_; } }
                else if (use) { p_ = pv[u]; r_ = rv[u]; }
                if (!INIT) { G[0] = XB_MFMA(p_, t_, G[0]); G[1] = XB_MFMA(p_, r_, G[1]); G[2] = XB_MFMA(t_, r_, G[2]); G[3] = XB_MFMA(t_, t_, G[3]); G[5] = XB_MFMA(p_, p_, G[5]); }
                G[4] = XB_MFMA(r_, r_, G[4]);
            }
        }
    }
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
// k_xtb_rows_slab's first pass (INIT) launched plainly, a sweep's between the profiling events e0 / e1 (null: none)
template <int MODE, class... Args>
static void xtb_rows_slab_launch(bool init, int ng, hipStream_t st, hipEvent_t e0, hipEvent_t e1, Args... a)
{
    if (init) hipLaunchKernelGGL((k_xtb_rows_slab<1, MODE>), dim3(ng), dim3(XT_NT), 0, st, a...);
    else hipExtLaunchKernelGGL((k_xtb_rows_slab<0, MODE>), dim3(ng), dim3(XT_NT), 0, st, e0, e1, 0, a...);
}

// ---- exchange 3: piece for d != me = [QS of my S rows (nS[me] x 16, list order) | the P rows d reads (halo, 16 each)] ----
__global__ void k_xtb_pack3(SlabMeta M, const int *__restrict__ S_by_owner, const int *__restrict__ hsend, const double *__restrict__ QS, const double *__restrict__ P,
                            double *__restrict__ send3)
{
    const int d = blockIdx.y;
    if (d == M.me) return;
    const int nq = M.soffs[M.me + 1] - M.soffs[M.me], nh = M.hsoff[d + 1] - M.hsoff[d];
    const long long n = (long long)(nq + nh) * XB_SP;
    double *dst = send3 + M.p3s[d];
    for (long long e = (long long)blockIdx.x * blockDim.x + threadIdx.x; e < n; e += (long long)gridDim.x * blockDim.x) {
        const int j = (int)(e >> 4), v = (int)(e & 15);
        dst[e] = j < nq ? QS[xtb_qs_pos(S_by_owner[M.soffs[M.me] + j], v)] : P[(size_t)hsend[M.hsoff[d] + j - nq] * XB_SP + v];
    }
}
__global__ void k_xtb_unpack3(SlabMeta M, const int *__restrict__ S_by_owner, const int *__restrict__ hrecv, const double *__restrict__ recv3, double *__restrict__ QS,
                              double *__restrict__ P, const XCtrl *ctrl)
{
    const int s = blockIdx.y;
    if (s == M.me) return;
    const int nq = M.soffs[s + 1] - M.soffs[s], nh = M.hroff[s + 1] - M.hroff[s];
    const long long n = (long long)(nq + nh) * XB_SP;
    const double *src = recv3 + M.p3r[s];
    for (long long e = (long long)blockIdx.x * blockDim.x + threadIdx.x; e < n; e += (long long)gridDim.x * blockDim.x) {
        const int j = (int)(e >> 4), v = (int)(e & 15);
        if (j < nq) QS[xtb_qs_pos(S_by_owner[M.soffs[s] + j], v)] = src[e];
        else P[(size_t)hrecv[M.hroff[s] + j - nq] * XB_SP + v] = src[e];
    }
    (void)ctrl;
}
// ---- halo exchange of one panel (preconditioned loop: the input of every N product): the rows of V each neighbour slab reads.  The pieces lie
// in destination (source) order, as the halo lists do: position e of the buffer is entry e / 16 of the concatenated list ----
__global__ void k_xtb_packH(long long n, const int *__restrict__ hsend, const double *__restrict__ V, double *__restrict__ sendH, const XCtrl *ctrl)
{
    if (ctrl->done) return;
    for (long long e = (long long)blockIdx.x * blockDim.x + threadIdx.x; e < n; e += (long long)gridDim.x * blockDim.x)
        sendH[e] = V[(size_t)hsend[e >> 4] * XB_SP + (int)(e & 15)];
}
__global__ void k_xtb_unpackH(long long n, const int *__restrict__ hrecv, const double *__restrict__ recvH, double *__restrict__ V, const XCtrl *ctrl)
{
    if (ctrl->done) return;
    for (long long e = (long long)blockIdx.x * blockDim.x + threadIdx.x; e < n; e += (long long)gridDim.x * blockDim.x)
        V[(size_t)hrecv[e >> 4] * XB_SP + (int)(e & 15)] = recvH[e];
}
// this rank's part of ||T(:, 0) - b||^2 (the true residual of a preconditioned solve) over its list rows in one workgroup (fixed order); the two
// driver rows (list entries 0 / 1) count on rank 0 only
__global__ __launch_bounds__(1024) void k_xtb_pre_rr_list(int n, const int *__restrict__ rowlist, int me, const double *__restrict__ T, const double *__restrict__ b,
                                                          double *__restrict__ out)
{
    __shared__ double red[1024];
    double a = 0.0;
    for (int i = threadIdx.x; i < n; i += 1024) {
        if (i < 2 && me != 0) continue;
        const int row = rowlist[i]; const double d = T[(size_t)row * XB_SP] - b[row]; a += d * d;
    }
    red[threadIdx.x] = a;
    __syncthreads();
    for (int o = 512; o > 0; o >>= 1) { if ((int)threadIdx.x < o) red[threadIdx.x] += red[threadIdx.x + o]; __syncthreads(); }
    if (threadIdx.x == 0) out[0] = red[0];
}

// ---- the solution: every rank's rows of y0 to everybody (once per solve); piece for d != me = y0 of my rows, list order ----
// w = 1: the vector y0; w = 16: a panel ([row][16], e.g. the block iterate whose auxiliary columns the next solve starts from)
__global__ void k_xtb_pack4(SlabMeta M, const int *__restrict__ rows_by_owner, const double *__restrict__ y0, double *__restrict__ send4, int w)
{
    const int n = M.rowoff[M.me + 1] - M.rowoff[M.me];
    const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= (long long)n * w) return;
    const double yv = y0[(size_t)rows_by_owner[M.rowoff[M.me] + (int)(i / w)] * w + (int)(i % w)];
    int k = 0;
    for (int d = 0; d < M.nr; ++d) { if (d == M.me) continue; send4[(size_t)k * n * w + i] = yv; ++k; }
}
__global__ void k_xtb_unpack4(SlabMeta M, const int *__restrict__ rows_by_owner, const double *__restrict__ recv4, double *__restrict__ y0, int w)
{
    // recv4: pieces in source order (the own one left out); piece of s holds the rows of s in list order
    const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    const int total = M.rowoff[M.nr] - (M.rowoff[M.me + 1] - M.rowoff[M.me]);
    if (i >= (long long)total * w) return;
    // position of the concatenation of all lists but mine -> position in rows_by_owner
    const int ir = (int)(i / w);
    const int j = ir < M.rowoff[M.me] ? ir : ir + (M.rowoff[M.me + 1] - M.rowoff[M.me]);
    y0[(size_t)rows_by_owner[j] * w + (int)(i % w)] = recv4[i];
}

// per virtual rank: share of the tiles, lists, panels, exchange buffers
struct SlabRank {
    int v = 0;
    const XItem *items = nullptr; int item_n = 0, w_lo = 0, w_hi = 0, sub_base = 0; const int *nitem_w = nullptr; int nrecords = 0;
    int n_own = 0, nS = 0;
    int *steplist = nullptr, *hsend = nullptr, *hrecv = nullptr, *dlist = nullptr; int nd0 = 0, nd1 = 0;
    double *Ypanel = nullptr;
    double *R = nullptr, *P = nullptr, *T = nullptr, *y0 = nullptr, *QS = nullptr, *rowpartB = nullptr, *colpartB = nullptr, *gpart = nullptr, *mats = nullptr,
           *drvpart = nullptr, *gx = nullptr, *send1 = nullptr, *recv1 = nullptr, *send3 = nullptr, *recv3 = nullptr;
    XCtrl *ctrl = nullptr;
    SlabMeta M{};
    long long n1s = 0, n1r = 0, n3s = 0, n3r = 0;
    // split polynomial preconditioner (dkmc_set_x_slab_poly): Vp = L P (+ m zeros: the right-hand side of column 0), Zp = A Vp, W1 / W2 the Horner
    // steps; N packed over the rank's list rows (dkmc_set_x_nmul_form(1))
    double *Vp = nullptr, *Zp = nullptr, *W1 = nullptr, *W2 = nullptr, *bz = nullptr;
    XbNPack npk{};
};
// apply, neigh, fold + tail, rows, gred, small, step, pack + unpack (preconditioned loop: rows includes the fold pass, pack + unpack the halo exchanges);
// nmul_us: one N x panel product (mean over the launches)
struct SlabTimes { double us[8] = {0, 0, 0, 0, 0, 0, 0, 0}; int n = 0; double nmul_us = 0.0; };
static SlabTimes g_slab_times;                       // filled by an emulation run with time_rank >= 0
static long long g_slab_xbytes[3] = {0, 0, 0};       // doubles a rank receives per sweep in exchanges 1, 2, 3 (largest over the ranks)
struct SlabLast { int exchanges = 0; long long halo_doubles = 0; double nmul_us = 0.0; };
static SlabLast g_slab_last;                         // dkmc_xtb_slab_last: exchanges per sweep, doubles a rank receives per halo exchange (largest), nmul_us

// Returns like xtb_cg.  emu_shares != nullptr: emulation -- nr virtual ranks in this process (X resident as after a single-GPU solve), the
// exchanges as device copies; emu_shares[v] holds virtual rank v's share of the work items.  time_rank >= 0: every kernel of that virtual rank
// is bracketed by events and its mean duration left in g_slab_times.
static int g_slab_sweep_cap = 0;                     // emulation, measurement runs: stop after this many sweeps (0: run to the stop test)
static int xtb_cg_slab(const XtbArgs &A, int nr, int me0, const XShare *emu_shares, int time_rank, int *iters_out, double *rr_out)
{
    Engine &e = eng(); hipStream_t st = e.stream;
    const bool emu = emu_shares != nullptr;
    const int nv = emu ? nr : 1;
    const int m = A.m, s = A.s, so = 4 * ((s + 3) / 4), ns = A.ns;
    const size_t pan = (size_t)m * XB_SP;
    const long long ncell = (long long)A.nK * A.nW;
    SlabArena arena{st, "slab emulation: out of device memory"};
    if (nr < 1 || nr > XS_MAXR) return dkmc_fail(43, "slab-distributed solve: 1 ... 32 ranks", __FILE__, __LINE__);
    if (!A.ay || !A.az) return dkmc_fail(43, "slab-distributed solve: needs the atom positions", __FILE__, __LINE__);

    // ---- ownership: slabs along the wider lateral axis, cuts balanced by row count (every rank computes the same from replicated data) ----
    XbAux *box = (XbAux *)scratch(S_XTB_SLAB_BOX, sizeof(XbAux));
    void *itab = scratch(S_XTB_SLAB_TAB, slab_tab_bytes());
    void *owner_mask = scratch(S_XTB_SLAB_OWNER, slab_owner_bytes(m));
    int *lists = (int *)scratch(S_XTB_SLAB_LISTS, ((size_t)m + ns + 8) * 4);
    long long *sdst = (long long *)scratch(S_XTB_SLAB_SDST, (size_t)(ns + 1) * 8);
    void *flag_pos = scratch(S_XTB_SLAB_FLAG, slab_flag_bytes(m));
    if (!box || !itab || !owner_mask || !lists || !sdst || !flag_pos) return e.err_code;
    const SlabWork W = slab_work(itab, owner_mask, flag_pos, m);
    int *const owner = W.owner, *const flag = W.flag, *const pos = W.pos;
    int *rows_by_owner = lists, *S_by_owner = lists + m;
    std::vector<int> htab;
    {
        XbAux h0{};
        if (int rc = xtb_box_modes(box, h0, A, 0, st)) return rc;
        HIPCHK(hipMemcpyAsync(&h0, box, sizeof(XbAux), hipMemcpyDeviceToHost, st));
        HIPCHK(hipStreamSynchronize(st));
        // Which lateral axis: the rows are balanced along either, the S rows (inner-contact metals, vacancies) need not be -- the inner-contact
        // window is an INDEX range of the site list (iterative_solvers_gpu.cu:894-900), and on a laterally tiled stack that range is one stripe
        // of tiles: slabs across it leave all contact rows of S on one rank (2x the exchange-1 payload at 8 ranks).  Both axes are tried (wider
        // first) and the one whose largest S share is smaller is kept.
        const int wide = (h0.hi[2] - h0.lo[2] > h0.hi[1] - h0.lo[1]) ? 2 : 1;
        int best_axis = wide; long long best_max = -1;
        for (int pass = 0; pass < 3; ++pass) {
            const int axis = pass == 0 ? wide : (pass == 1 ? 3 - wide : best_axis);
            if (pass == 2 && axis == 3 - wide) break;                         // the second try is the one kept: everything is in place
            if (int rc = slab_partition(st, m, 2, A.rp, A.ci, axis == 2 ? A.az : A.ay, h0.lo[axis], h0.hi[axis], nr, A.nsrank, W)) return rc;
            if (nr == 1) break;
            if (int rc = slab_download_tab(st, W, nr, htab)) return rc;
            long long mx = 0; for (int r = 0; r < nr; ++r) mx = std::max<long long>(mx, htab[nr + r]);
            if (pass == 2) break;
            if (best_max < 0 || mx < best_max - best_max / 16) { best_max = mx; best_axis = axis; }      // (the narrower axis must be clearly better)
        }
    }
    if (int rc = slab_download_tab(st, W, nr, htab)) return rc;
    const SlabPlan P(htab.data(), nr);
    const int *nown = P.nown(), *nSr = P.nmark();
    SlabMeta M0{}; M0.nr = nr;
    for (int r = 0; r <= nr; ++r) { M0.soffs[r] = P.markoff[r]; M0.rowoff[r] = P.rowoff[r]; }
    if (!P.covers(m - 2, ns)) return dkmc_fail(13, "slab-distributed solve: the slabs do not cover the rows", __FILE__, __LINE__);
    // rows and S ranks grouped by owner (ascending inside a group)
    for (int r = 0; r < nr; ++r) {
        int rc = slab_rows_of_owner(st, m, 2, W, P, r, rows_by_owner); if (rc) return rc;
        hipLaunchKernelGGL(k_slab_flag_S, dim3((ns + 255) / 256), dim3(256), 0, st, ns, A.srow, (const int *)owner, r, flag);
        rc = dkmc_exclusive_scan_i32(flag, pos, ns, nullptr); if (rc) return rc;
        hipLaunchKernelGGL(k_slab_scatter_S, dim3((ns + 255) / 256), dim3(256), 0, st, ns, (const int *)flag, (const int *)pos, M0.soffs[r], r, so, S_by_owner, sdst);
    }
    KCHK();

    // split polynomial preconditioner (dkmc_set_x_slab_poly; opt-in): the loop runs on L A L with the degree and coefficients of the one-GPU loop
    const int pd = (e.x_slab_poly && m > 2 && ns > 0) ? std::min(e.x_poly, XB_MAXPOLY) : 0;       // (the explicit degree: the rule of the one-GPU loop was measured there only)
    e.stats.xb_poly_used = pd;
    double pc[XB_MAXPOLY + 1] = {1.0};
    xtb_poly_coeffs(pd, pc);
    const double tol2_loop = pd > 0 ? A.tol2 / 2.25 : A.tol2;                  // as in xtb_cg_body: the true residual is checked at the end
    const bool keep_aux = A.yaux != nullptr && pd == 0;                        // (no auxiliary columns are kept by a preconditioned solve, as on one GPU)

    // ---- per (virtual) rank: lists, panels, exchange buffers ----
    xrp_t drp[3] = {0, 0, 0};
    HIPCHK(hipMemcpy(drp, A.rp, sizeof(drp), hipMemcpyDeviceToHost));
    const int ndrv = (int)drp[2];                    // entries of the two driver rows (rows 0 and 1 open the CSR)
    if (drp[0] != 0 || ndrv > m + 8) return dkmc_fail(13, "slab-distributed solve: unexpected driver rows", __FILE__, __LINE__);
    std::vector<SlabRank> RK((size_t)nv);
    // row-kernel workgroups = partial Gram matrices per rank: ~128 rows and one 32-row block of S per workgroup (170 workgroups for 8e4 rows took 63 us)
    const int ng = std::max(128, std::min(2048, (std::max(m / nr, 1) + 127) / 128 + (A.nK + nr - 1) / nr));
    std::vector<long long> cnt1((size_t)nr * nr), cnt3((size_t)nr * nr), cnt4((size_t)nr * nr), cnt5((size_t)nr * nr), cntH((size_t)nr * nr);
    for (int a = 0; a < nr; ++a) for (int d = 0; d < nr; ++d) {
        cnt1[(size_t)a * nr + d] = (long long)nSr[d] * so + XS_DRV + 2;
        cnt3[(size_t)a * nr + d] = a == d ? 0 : ((long long)nSr[a] + P.hal(a, d)) * XB_SP;
        cnt4[(size_t)a * nr + d] = a == d ? 0 : nown[a];
        cnt5[(size_t)a * nr + d] = a == d ? 0 : (long long)nown[a] * XB_SP;
        cntH[(size_t)a * nr + d] = a == d ? 0 : (long long)P.hal(a, d) * XB_SP;      // halo exchange (preconditioned loop): the halo part of exchange 3
    }
    for (int iv = 0; iv < nv; ++iv) {
        SlabRank &K = RK[iv]; const int v = emu ? iv : me0; K.v = v;
        if (emu) { const XShare &sh = emu_shares[v]; K.items = (const XItem *)sh.items + sh.item_lo; K.item_n = sh.item_n; K.w_lo = sh.w_lo; K.w_hi = sh.w_hi; K.sub_base = 0; K.nitem_w = sh.nitem_w; K.nrecords = sh.nitems >> sh.rec_shift; }
        else { K.items = A.items; K.item_n = A.item_n; K.w_lo = A.w_lo; K.w_hi = A.w_hi; K.sub_base = A.sub_base; K.nitem_w = A.nitem_w; K.nrecords = A.nrecords; }
        K.n_own = nown[v]; K.nS = nSr[v];
        SlabMeta &M = K.M; M = M0; M.me = v;
        const SlabHalo H(P, v);
        for (int r = 0; r <= nr; ++r) {
            M.hsoff[r] = H.hsoff[r]; M.hroff[r] = H.hroff[r];
            M.p3s[r] = slab_send_off(cnt3.data(), nr, v, r); M.p3r[r] = slab_recv_off(cnt3.data(), nr, r, v);
        }
        K.n1s = slab_send_off(cnt1.data(), nr, v, nr); K.n1r = slab_recv_off(cnt1.data(), nr, nr, v);
        K.n3s = M.p3s[nr]; K.n3r = M.p3r[nr];
        int *li = (int *)arena.get(iv, S_XTB_SLAB_RLISTS, ((size_t)K.n_own + 2 + M.hsoff[nr] + M.hroff[nr] + ndrv + 8) * 4);
        double *panels = (double *)arena.get(iv, S_XTB_PANELS, (pan * 3 + m + 16) * 8);
        K.QS = (double *)arena.get(iv, S_XTB_QS, (size_t)A.ns_pad * XB_SP * 8);
        K.rowpartB = (double *)arena.get(iv, S_XTB_ROWPART, (size_t)(ncell + 1) * XT_R * so * 8);
        K.colpartB = (double *)arena.get(iv, S_XTB_COLPART, (size_t)(K.nrecords + 1) * XT_C * so * 8);
        K.gpart = (double *)arena.get(iv, S_XTB_GRAM, (size_t)ng * XB_NG * 256 * 8);
        double *small = (double *)arena.get(iv, S_XTB_SMALL, (size_t)(4 * 256 + 2 * XB_DSPLIT * XB_SP + XB_NG * 256) * 8);
        K.gx = (double *)arena.get(iv, S_XTB_SLAB_GX, (size_t)nr * XS_GSTR * 8);
        if (keep_aux) K.Ypanel = (double *)arena.get(iv, S_XTB_YPANEL, pan * 8);
        if (pd > 0) {
            K.Vp = (double *)arena.get(iv, S_XTB_PRE_V, (pan + m + 16) * 8); K.W1 = (double *)arena.get(iv, S_XTB_PRE_W1, pan * 8);
            K.W2 = (double *)arena.get(iv, S_XTB_PRE_W2, pan * 8); K.Zp = (double *)arena.get(iv, S_XTB_PRE_Z, pan * 8);
        }
        const size_t n4 = ((size_t)std::max<long long>((long long)(nr - 1) * K.n_own, (long long)(m - 2 - K.n_own)) + 8) * (keep_aux ? XB_SP : 1);
        K.send1 = (double *)arena.get(iv, S_XTB_SLAB_S1, (size_t)std::max<long long>(K.n1s, (long long)n4) * 8);
        K.recv1 = (double *)arena.get(iv, S_CG_XCHG, (size_t)std::max<long long>(K.n1r, (long long)n4) * 8);
        K.send3 = (double *)arena.get(iv, S_XTB_SLAB_S3, (size_t)(K.n3s + 8) * 8);
        K.recv3 = (double *)arena.get(iv, S_XTB_SLAB_R3, (size_t)(K.n3r + 8) * 8);
        K.ctrl = iv == 0 ? A.ctrl : (XCtrl *)arena.get(iv, 0, sizeof(XCtrl));
        if (arena.fail) return arena.fail;
        K.R = panels; K.P = panels + pan; K.T = panels + 2 * pan; K.y0 = panels + 3 * pan;
        K.mats = small; K.drvpart = small + 4 * 256;
        K.steplist = li; K.hsend = li + K.n_own + 2; K.hrecv = K.hsend + M.hsoff[nr]; K.dlist = K.hrecv + M.hroff[nr];
        if (ndrv > 0) {
            hipLaunchKernelGGL(k_slab_flag_drv, dim3((ndrv + 255) / 256), dim3(256), 0, st, ndrv, A.ci, (const int *)owner, v, flag);
            int rc = dkmc_exclusive_scan_i32(flag, pos, ndrv, pos + ndrv); if (rc) return rc;
            hipLaunchKernelGGL(k_slab_scatter_drv, dim3((ndrv + 255) / 256), dim3(256), 0, st, ndrv, (const int *)flag, (const int *)pos, K.dlist);
            int hc[2] = {0, 0};      // entries of row 0 I own = pos[rp[1]]; all = pos[ndrv]
            HIPCHK(hipMemcpyAsync(&hc[0], pos + (int)drp[1], 4, hipMemcpyDeviceToHost, st));
            HIPCHK(hipMemcpyAsync(&hc[1], pos + ndrv, 4, hipMemcpyDeviceToHost, st));
            HIPCHK(hipStreamSynchronize(st));
            K.nd0 = hc[0]; K.nd1 = hc[1] - hc[0];
        }
        hipLaunchKernelGGL(k_slab_steplist, dim3((K.n_own + 2 + 255) / 256), dim3(256), 0, st, K.n_own, (const int *)rows_by_owner + M0.rowoff[v], K.steplist);
        // halo lists: what I send to d (my rows with bit d), what I receive from s (the rows of s with my bit)
        if (int rc = slab_halo_lists(st, W, P, H, v, rows_by_owner, K.hsend, K.hrecv)) return rc;
        HIPCHK(hipMemsetAsync(K.QS, 0, (size_t)A.ns_pad * XB_SP * 8, st));
        HIPCHK(hipMemsetAsync(K.rowpartB, 0, (size_t)(ncell + 1) * XT_R * so * 8, st));
        HIPCHK(hipMemsetAsync(K.colpartB, 0, (size_t)(K.nrecords + 1) * XT_C * so * 8, st));
        HIPCHK(hipMemsetAsync(K.ctrl, 0, sizeof(XCtrl), st));
        HIPCHK(hipMemsetAsync(K.send1, 0, (size_t)K.n1s * 8, st));
        HIPCHK(hipMemsetAsync(panels, 0, (pan * 3 + m + 16) * 8, st));
        if (pd > 0) {
            K.bz = K.Vp + pan;
            HIPCHK(hipMemsetAsync(K.Vp, 0, (pan + m + 16) * 8, st));
            HIPCHK(hipMemsetAsync(K.W1, 0, pan * 8, st)); HIPCHK(hipMemsetAsync(K.W2, 0, pan * 8, st)); HIPCHK(hipMemsetAsync(K.Zp, 0, pan * 8, st));
            // N packed over the list rows (dkmc_set_x_nmul_form(1)): slices of four list entries, the one-GPU slots per row
            if (e.x_nmul_form == 1)
                if (int rc = xtb_npack(A, K.n_own + 2, K.steplist, [&](int slot, size_t bytes) { return arena.get(iv, slot, bytes); }, 64, &K.npk)) return rc;
        }
    }
    KCHK();
    g_slab_xbytes[0] = slab_recv_max(cnt1.data(), nr); g_slab_xbytes[2] = slab_recv_max(cnt3.data(), nr);
    g_slab_xbytes[1] = (long long)(nr - 1) * XS_GSTR;
    e.stats.comm_count_per_rank = g_slab_xbytes[0] + g_slab_xbytes[1] + g_slab_xbytes[2];
    // preconditioned loop: exchange 3 carries QS + the halo of Vp; 2 d halo exchanges (P or Zp, then the Horner intermediates) are added per sweep
    g_slab_last.exchanges = nr > 1 ? (pd > 0 ? 2 * pd + 3 : 3) : 2;
    g_slab_last.halo_doubles = slab_recv_max(cntH.data(), nr); g_slab_last.nmul_us = 0.0;
    if (pd > 0 && nr > 1) e.stats.comm_count_per_rank += 2LL * pd * g_slab_last.halo_doubles;

    // smooth auxiliary columns (as in xtb_cg)
    XbAux *aux = nullptr; int hs = 1;
    if (int rc = xtb_aux_setup(A, &aux, &hs)) return rc;

    // ---- exchanges: the communicator (one local rank) or device copies between the virtual ranks ----
    // 1, 3, 4, 5: all-to-all-v; 2: all-gather of the Gram blocks; 6: halo exchange (all-to-all-v in the buffers of exchange 3); 7: all-gather of one
    // double per rank (gx[rank])
    auto xchg = [&](int which) -> int {
        if (!emu) {
            SlabRank &K = RK[0];
            if (which == 1) return comm_alltoallv_f64(K.send1, K.recv1, cnt1.data());
            if (which == 3) return comm_alltoallv_f64(K.send3, K.recv3, cnt3.data());
            if (which == 4) return comm_alltoallv_f64(K.send1, K.recv1, cnt4.data());
            if (which == 5) return comm_alltoallv_f64(K.send1, K.recv1, cnt5.data());
            if (which == 6) return comm_alltoallv_f64(K.send3, K.recv3, cntH.data());
            if (which == 7) return comm_allgather_f64(K.gx, 1);
            return comm_allgather_f64(K.gx, (size_t)XS_GSTR);
        }
        if (which == 2 || which == 7) return slab_emu_allgather(st, nr, which == 2 ? (size_t)XS_GSTR : 1, [&](int r) { return RK[r].gx; });
        const std::vector<long long> &cnt = which == 1 ? cnt1 : (which == 3 ? cnt3 : (which == 4 ? cnt4 : (which == 5 ? cnt5 : cntH)));
        const bool b3 = which == 3 || which == 6;
        return slab_emu_alltoallv(st, nr, cnt.data(), [&](int r) { return b3 ? RK[r].send3 : RK[r].send1; }, [&](int r) { return b3 ? RK[r].recv3 : RK[r].recv1; });
    };
    // ---- timing of one virtual rank's kernels (emulation) ----
    SlabTimes &TM = g_slab_times;
    const bool timing = emu && time_rank >= 0 && time_rank < nr;
    SlabTimer timer{st};
    if (timing) { TM = SlabTimes(); if (int rc = timer.create()) return rc; }
    std::vector<std::pair<int, float>> tsamples;
    int tphase = 0;      // sweeps timed so far
    auto timed = [&](int iv, int cls, bool on, const std::function<void()> &launch) -> int {
        const bool t = timing && on && RK[iv].v == time_rank;
        float ms = 0.f;
        if (int rc = timer.run(t, launch, &ms)) return rc;
        if (t) tsamples.push_back({cls, ms});
        return 0;
    };
    const int nnb_of = 2 * XB_DSPLIT;
    const bool prof = e.profiling != 0 && !emu;
    if (prof) if (int prc = g_loop_events.begin(EventSampler::LONG | EventSampler::SHORT)) return prc;
    int local_fail = 0;

    // panels of a rank by member: the preconditioned loop runs the same passes on Vp / Zp that the plain one runs on P / T
    typedef double *SlabRank::*Pan;
    auto product = [&](bool on, hipEvent_t e0, hipEvent_t e1, Pan pin = &SlabRank::P, Pan tout = &SlabRank::T) -> int {
        for (int iv = 0; iv < nv; ++iv) {
            SlabRank &K = RK[iv];
            const int ntb = (K.item_n + 3) / 4;
            if (ntb > 0) {
                int rc = timed(iv, 0, on, [&]() {
                    xtb_apply({K.item_n, K.items, A.tiles, K.sub_base, A.tval, K.QS, A.nW, K.rowpartB, K.colpartB, K.ctrl}, A.nt_loads, so, 0, st, e0, e1);
                }); if (rc) return rc;
            } else if (e0) { HIPCHK(hipEventRecord(e0, st)); HIPCHK(hipEventRecord(e1, st)); }
            int rc = timed(iv, 1, on, [&]() {
                hipLaunchKernelGGL(k_xtb_neigh, dim3(nnb_of + (K.n_own + 15) / 16), dim3(XT_NT), 0, st, m, A.rp, A.ci, A.val, (const double *)(K.*pin), A.sc, A.nsrank,
                                   (const XCtrl *)K.ctrl, K.*tout, K.drvpart, (const int *)K.steplist + 2, K.n_own, (const int *)K.dlist, K.nd0, K.nd1);
            }); if (rc) return rc;
            rc = timed(iv, 2, on, [&]() {
                hipLaunchKernelGGL(k_xtb_fold_local, dim3(std::max(A.nK, 1)), dim3(XT_NT), 0, st, ns, A.nK, A.nW, so, A.wrange, K.nitem_w, (const double *)K.rowpartB,
                                   (const double *)K.colpartB, K.send1, (const XCtrl *)K.ctrl, 0, K.w_lo, K.w_hi, (const long long *)sdst);
                hipLaunchKernelGGL(k_xtb_slab_tail, dim3(nr), dim3(64), 0, st, nr, so, K.M, (const double *)K.drvpart, (const XCtrl *)K.ctrl, K.send1);
            }); if (rc) return rc;
        }
        return 0;
    };
    // exchange 1; a host-side failure of this rank between two collectives still joins, with the abort word set
    auto xchg1 = [&]() -> int {
        if (!emu && (hipGetLastError() != hipSuccess || local_fail)) {
            if (!local_fail) local_fail = dkmc_fail(92, "block-CG: launch failed between two collectives", __FILE__, __LINE__);
            hipLaunchKernelGGL(k_xtb_abort_word, dim3(1), dim3(1), 0, st, RK[0].ctrl, RK[0].send1, (size_t)RK[0].M.soffs[1] * so + XS_DRV + 1);
            hipLaunchKernelGGL(k_xtb_slab_tail, dim3(nr), dim3(64), 0, st, nr, so, RK[0].M, (const double *)RK[0].drvpart, (const XCtrl *)RK[0].ctrl, RK[0].send1);
        }
        return xchg(1);
    };
#define XS_ROWS_ARGS(T_, B_) K.nS, (const int *)S_by_owner + M0.soffs[K.v], K.n_own, (const int *)K.steplist + 2, s, so, nr, K.v, (const double *)K.recv1, A.srow, A.sS, \
                     A.nsrank, A.sc, T_, (const double *)K.P, K.R, B_, K.gpart, K.ctrl, itn, (const XbAux *)aux, A.ax, A.ay, A.az
    // the Gram pass (mode 0: with the fold; XS_NF: on the final T of the preconditioned loop, against the zero right-hand side of column 0), exchange 2
    auto gram = [&](int mode, bool init, int itn, bool on, hipEvent_t e2, hipEvent_t e3) -> int {
        for (int iv = 0; iv < nv; ++iv) {
            SlabRank &K = RK[iv];
            int rc = timed(iv, 3, on, [&]() {
                if (mode == XS_NF) xtb_rows_slab_launch<XS_NF>(init, ng, st, e2, e3, XS_ROWS_ARGS(K.T, (const double *)K.bz));
                else xtb_rows_slab_launch<0>(init, ng, st, e2, e3, XS_ROWS_ARGS(K.T, A.b));
            }); if (rc) return rc;
            rc = timed(iv, 4, on, [&]() {
                hipLaunchKernelGGL(k_xtb_gred, dim3(XB_NG * 16), dim3(XT_NT), 0, st, ng, (const double *)K.gpart, K.gx + (size_t)K.v * XS_GSTR, (const XCtrl *)K.ctrl);
                hipLaunchKernelGGL(k_xtb_slab_gtail, dim3(1), dim3(1), 0, st, (const XCtrl *)K.ctrl, K.gx + (size_t)K.v * XS_GSTR);
            }); if (rc) return rc;
        }
        return xchg(2);
    };
    auto rows = [&](bool init, int itn, bool on, hipEvent_t e2, hipEvent_t e3) -> int {
        if (int rcx = xchg1()) return rcx;
        return gram(0, init, itn, on, e2, e3);
    };
    // the fold alone (preconditioned loop): my S rows and the driver rows of K.*tout from exchange 1
    auto fold = [&](int itn, bool on, Pan tout) -> int {
        for (int iv = 0; iv < nv; ++iv) {
            SlabRank &K = RK[iv];
            int rc = timed(iv, 3, on, [&]() {
                hipLaunchKernelGGL((k_xtb_rows_slab<0, XS_FOLD>), dim3(ng), dim3(XT_NT), 0, st, XS_ROWS_ARGS(K.*tout, A.b));
            }); if (rc) return rc;
        }
        return 0;
    };
#undef XS_ROWS_ARGS
    // halo exchange of one panel: the rows of it that a neighbour slab reads
    auto halo = [&](Pan pv, bool on) -> int {
        if (nr < 2) return 0;
        for (int iv = 0; iv < nv; ++iv) {
            SlabRank &K = RK[iv];
            const long long n = (long long)K.M.hsoff[nr] * XB_SP;
            if (n > 0) { int rc = timed(iv, 7, on, [&]() {
                hipLaunchKernelGGL(k_xtb_packH, dim3((unsigned)std::min<long long>(1024, (n + 255) / 256)), dim3(256), 0, st, n, (const int *)K.hsend, (const double *)(K.*pv), K.send3,
                                   (const XCtrl *)K.ctrl);
            }); if (rc) return rc; }
        }
        if (int rcx = xchg(6)) return rcx;
        for (int iv = 0; iv < nv; ++iv) {
            SlabRank &K = RK[iv];
            const long long n = (long long)K.M.hroff[nr] * XB_SP;
            if (n > 0) { int rc = timed(iv, 7, on, [&]() {
                hipLaunchKernelGGL(k_xtb_unpackH, dim3((unsigned)std::min<long long>(1024, (n + 255) / 256)), dim3(256), 0, st, n, (const int *)K.hrecv, (const double *)K.recv3, K.*pv,
                                   (const XCtrl *)K.ctrl);
            }); if (rc) return rc; }
        }
        return 0;
    };
    // dst = L src on every rank's list rows (xtb_applyL; the rows are formed as on one GPU: the same bits).  Before every product the halo of its input
    // is exchanged, except src's when the caller has made it current.  qs: QS of dst's own S rows as well (CSR form: of every S row; the other ranks'
    // rows are overwritten by exchange 3).
    auto applyL = [&](Pan src, Pan dst, bool qs, bool src_halo, bool on) -> int {
        return xtb_applyL(st, A, pd, pc, src, dst, &SlabRank::W1, &SlabRank::W2, qs, [&](int i, Pan in) { return (i > 0 || !src_halo) ? halo(in, on) : 0; },
                          [&](bool nprod, auto f) -> int {
                              for (int iv = 0; iv < nv; ++iv) {
                                  SlabRank &K = RK[iv];
                                  const XbNRank R{K.n_own + 2, K.steplist, K.npk.off ? &K.npk : nullptr, K.QS, K.ctrl};
                                  auto at = [&K](Pan p) { return K.*p; };
                                  if (!nprod) f(R, at);
                                  else if (int rc = timed(iv, 8, on, [&]() { f(R, at); })) return rc;
                              }
                              return 0;
                          });
    };
    // exchange 3: the own rows of QS to everybody + the halo of the panel the next product reads
    auto xchg3 = [&](Pan pv, bool on) -> int {
        if (nr < 2) return 0;
        for (int iv = 0; iv < nv; ++iv) {
            SlabRank &K = RK[iv];
            int rc = timed(iv, 7, on, [&]() {
                hipLaunchKernelGGL(k_xtb_pack3, dim3((unsigned)std::max<long long>(1, std::min<long long>(256, (K.n3s / std::max(nr - 1, 1) + 255) / 256)), nr), dim3(256), 0, st,
                                   K.M, (const int *)S_by_owner, (const int *)K.hsend, (const double *)K.QS, (const double *)(K.*pv), K.send3);
            }); if (rc) return rc;
        }
        if (int rcx = xchg(3)) return rcx;
        for (int iv = 0; iv < nv; ++iv) {
            SlabRank &K = RK[iv];
            int rc = timed(iv, 7, on, [&]() {
                hipLaunchKernelGGL(k_xtb_unpack3, dim3((unsigned)std::max<long long>(1, std::min<long long>(256, (K.n3r / std::max(nr - 1, 1) + 255) / 256)), nr), dim3(256), 0, st,
                                   K.M, (const int *)S_by_owner, (const int *)K.hrecv, (const double *)K.recv3, K.QS, K.*pv, (const XCtrl *)K.ctrl);
            }); if (rc) return rc;
        }
        return 0;
    };
    auto update = [&](int itn, bool on) -> int {
        for (int iv = 0; iv < nv; ++iv) {
            SlabRank &K = RK[iv];
            int rc = timed(iv, 5, on, [&]() {
                hipLaunchKernelGGL(k_xtb_small, dim3(1), dim3(256), 0, st, itn, s, (const double *)K.gx, K.mats, K.ctrl, tol2_loop, nr, (int)XS_GSTR);
            }); if (rc) return rc;
            if (itn < 0) hipLaunchKernelGGL(k_xtb_zero, dim3((unsigned)((pan + 255) / 256)), dim3(256), 0, st, (long long)pan, K.P);
            rc = timed(iv, 6, on, [&]() {
                hipLaunchKernelGGL(k_xtb_step, dim3(grid_blocks((K.n_own + 2 + 15) / 16, 4, 2048)), dim3(XT_NT), 0, st, K.n_own + 2, itn, (const double *)K.mats, K.y0, K.R, K.P,
                                   (const double *)K.T, A.sc, A.nsrank, K.QS, (const XCtrl *)K.ctrl, (const int *)K.steplist, K.Ypanel);
            }); if (rc) return rc;
        }
        // preconditioned loop: the next product reads Vp, not P -- only the halo of P travels here (the first N product of the next sweep reads it)
        return pd > 0 ? halo(&SlabRank::P, on) : xchg3(&SlabRank::P, on);
    };
    // one sweep of the preconditioned loop: T = L A L P (2 d + 3 exchanges with the two of the Gram pass and the update's halo of P)
    auto sweep_pre = [&](int itn, bool on, hipEvent_t e0, hipEvent_t e1, hipEvent_t e2, hipEvent_t e3) -> int {
        if (int rcx = applyL(&SlabRank::P, &SlabRank::Vp, true, true, on)) return rcx;
        if (int rcx = xchg3(&SlabRank::Vp, on)) return rcx;
        if (int rcx = product(on, e0, e1, &SlabRank::Vp, &SlabRank::Zp)) return rcx;
        if (int rcx = xchg1()) return rcx;
        if (int rcx = fold(itn, on, &SlabRank::Zp)) return rcx;
        if (int rcx = applyL(&SlabRank::Zp, &SlabRank::T, false, false, on)) return rcx;
        if (int rcx = gram(XS_NF, false, itn, on, e2, e3)) return rcx;
        return update(itn, on);
    };

    // ---- R = A Y0 - B ; first directions ----
    for (int iv = 0; iv < nv; ++iv) {
        SlabRank &K = RK[iv];
        hipLaunchKernelGGL(k_xtb_init, dim3((unsigned)((pan + 255) / 256)), dim3(256), 0, st, m, (const double *)A.y, A.sc, A.nsrank, K.y0, K.P, K.QS,
                           (const double *)((keep_aux && A.yaux_valid) ? A.yaux : nullptr), hs, s, K.Ypanel);
    }
    if (int rcx = product(false, nullptr, nullptr)) return rcx;
    if (pd > 0) {
        // as xtb_cg_body: column 0 solves L A L dh = L (b - A y0) from zero -- T = A Y0 (fold), W = [T(:, 0) - b | 0], T = L W, R = T - [0 | auxiliary]
        if (int rcx = xchg1()) return rcx;
        if (int rcx = fold(-1, false, &SlabRank::T)) return rcx;
        for (int iv = 0; iv < nv; ++iv)
            hipLaunchKernelGGL(k_xtb_pre_resid, dim3((unsigned)((pan + 255) / 256)), dim3(256), 0, st, m, (const double *)RK[iv].T, A.b, RK[iv].Zp);
        if (int rcx = applyL(&SlabRank::Zp, &SlabRank::T, false, false, false)) return rcx;
        if (int rcx = gram(XS_NF, true, -1, false, nullptr, nullptr)) return rcx;
        for (int iv = 0; iv < nv; ++iv) HIPCHK(hipMemsetAsync(RK[iv].y0, 0, (size_t)m * 8, st));
    } else if (int rcx = rows(true, -1, false, nullptr, nullptr)) return rcx;
    if (int rcx = update(-1, false)) return rcx;
    KCHK();
    // the launch plan of xtb_cg_body; an emulation starts without the hint and leaves it unset
    XCtrl h{};
    if (int rcx = cg_poll_loop(RK[0].ctrl, h, LaunchPlan::hinted_three_quarters(emu ? 0 : e.x_iter_hint), st, XTB_NO_CONVERGENCE, prof ? &g_loop_events : nullptr,
                               [&](int it, const hipEvent_t *ev) -> int {
            if (!emu && g_xtb_fault_iter >= 0 && it >= g_xtb_fault_iter) { g_xtb_fault_iter = -1; local_fail = dkmc_fail(91, "injected fault (block-CG iteration)", __FILE__, __LINE__); }
            const bool on = timing && it >= 2 && tphase < 24;            // sweeps 2 ... 25 of the emulation are timed, kernel by kernel
            if (pd > 0) {
                if (int rcx = sweep_pre(it, on, ev[0], ev[1], ev[2], ev[3])) return rcx;
            } else {
                if (int rcx = product(on, ev[0], ev[1])) return rcx;
                if (int rcx = rows(false, it, on, ev[2], ev[3])) return rcx;
                if (int rcx = update(it, on)) return rcx;
            }
            if (on) ++tphase;
            return 0;
        }, emu ? g_slab_sweep_cap : 0)) return rcx;
    if (local_fail) return local_fail;
    if (h.aborted) return dkmc_fail(46, "a peer rank aborted the sharded current solve", __FILE__, __LINE__);
    if (e.err_code) return e.err_code;
    if (emu) {                                                              // every virtual rank must have stopped at the same sweep
        for (int iv = 1; iv < nv; ++iv) {
            XCtrl hv{};
            HIPCHK(hipMemcpy(&hv, RK[iv].ctrl, sizeof(XCtrl), hipMemcpyDeviceToHost));
            if (hv.iters != h.iters || hv.done != h.done || hv.pad[0] != h.pad[0]) return dkmc_fail(13, "slab emulation: the virtual ranks left the loop at different sweeps", __FILE__, __LINE__);
        }
    }
    if (pd > 0) {
        // y = y0 + L dh on the own rows (y0 of every rank holds dh of its rows; L needs the halo of dh and of the Horner intermediates)
        for (int iv = 0; iv < nv; ++iv) {
            SlabRank &K = RK[iv];
            HIPCHK(hipMemsetAsync(K.ctrl, 0, sizeof(XCtrl), st));          // (the kernels below are gated by `done`)
            hipLaunchKernelGGL(k_xtb_pre_col0, dim3((unsigned)((pan + 255) / 256)), dim3(256), 0, st, m, (const double *)K.y0, K.Zp);
        }
        if (int rcx = applyL(&SlabRank::Zp, &SlabRank::Vp, false, false, false)) return rcx;
        for (int iv = 0; iv < nv; ++iv) {
            SlabRank &K = RK[iv];
            HIPCHK(hipMemcpyAsync(K.y0, A.y, (size_t)m * 8, hipMemcpyDeviceToDevice, st));
            hipLaunchKernelGGL(k_xtb_pre_add, dim3((m + 255) / 256), dim3(256), 0, st, m, (const double *)K.Vp, K.y0);
        }
    }
    // ---- the solution on every rank: own rows of y0 to everybody ----
    if (nr > 1) {
        for (int pass = 0; pass < (keep_aux ? 2 : 1); ++pass) {             // the vector; then the block iterate (the next solve's auxiliary start)
            const int w = pass ? XB_SP : 1;
            for (int iv = 0; iv < nv; ++iv) {
                SlabRank &K = RK[iv];
                if (K.n_own > 0) hipLaunchKernelGGL(k_xtb_pack4, dim3((unsigned)(((long long)K.n_own * w + 255) / 256)), dim3(256), 0, st, K.M, (const int *)rows_by_owner,
                                                    (const double *)(pass ? K.Ypanel : K.y0), K.send1, w);
            }
            if (int rcx = xchg(pass ? 5 : 4)) return rcx;
            for (int iv = 0; iv < nv; ++iv) {
                SlabRank &K = RK[iv];
                const long long tot = (long long)(m - 2 - K.n_own) * w;
                if (tot > 0) hipLaunchKernelGGL(k_xtb_unpack4, dim3((unsigned)((tot + 255) / 256)), dim3(256), 0, st, K.M, (const int *)rows_by_owner, (const double *)K.recv1,
                                                pass ? K.Ypanel : K.y0, w);
            }
        }
    }
    if (emu)                                                                // ... and all of them must hold the same bits
        if (int rc = slab_same_bits(st, nv, (size_t)m, [&](int iv) { return RK[iv].y0; }, "slab emulation: the virtual ranks hold different solutions")) return rc;
    HIPCHK(hipMemcpyAsync(A.y, RK[0].y0, (size_t)m * 8, hipMemcpyDeviceToDevice, st));
    if (keep_aux) hipLaunchKernelGGL(k_xtb_yaux_out, dim3((unsigned)((pan + 255) / 256)), dim3(256), 0, st, m, (const int *)nullptr, (const double *)RK[0].Ypanel, A.sc, A.yaux);
    bool again = false;
    if (pd > 0 && !h.pad[0]) {
        // the TRUE residual of column 0: every rank holds all of y -- QS locally, one tile pass, exchange 1, the fold; the ranks' partials of
        // ||A y - b||^2 over their rows are all-gathered and added in rank order: the same bits, the same re-entry decision on every rank
        for (int iv = 0; iv < nv; ++iv) {
            SlabRank &K = RK[iv];
            hipLaunchKernelGGL(k_xtb_pre_col0, dim3((unsigned)((pan + 255) / 256)), dim3(256), 0, st, m, (const double *)K.y0, K.P);
            hipLaunchKernelGGL(k_xtb_qs_from, dim3((unsigned)((pan + 255) / 256)), dim3(256), 0, st, m, (const double *)K.P, A.sc, A.nsrank, K.QS, (const XCtrl *)K.ctrl);
        }
        if (int rcx = product(false, nullptr, nullptr)) return rcx;
        if (int rcx = xchg1()) return rcx;
        if (int rcx = fold(-1, false, &SlabRank::T)) return rcx;
        for (int iv = 0; iv < nv; ++iv)
            hipLaunchKernelGGL(k_xtb_pre_rr_list, dim3(1), dim3(1024), 0, st, RK[iv].n_own + 2, (const int *)RK[iv].steplist, RK[iv].v, (const double *)RK[iv].T, A.b,
                               RK[iv].gx + RK[iv].v);
        if (int rcx = xchg(7)) return rcx;
        std::vector<double> part((size_t)nr);
        HIPCHK(hipMemcpyAsync(part.data(), RK[0].gx, (size_t)nr * 8, hipMemcpyDeviceToHost, st));
        XCtrl h2{};
        HIPCHK(hipMemcpyAsync(&h2, RK[0].ctrl, sizeof(XCtrl), hipMemcpyDeviceToHost, st));
        HIPCHK(hipStreamSynchronize(st));
        if (local_fail) return local_fail;                                   // (the abort word of exchange 1 stops the peers here too: no rank re-enters)
        if (h2.aborted) return dkmc_fail(46, "a peer rank aborted the sharded current solve", __FILE__, __LINE__);
        double rr_true = 0.0;
        for (int r = 0; r < nr; ++r) rr_true += part[r];
        h.rr[h.iters & 1] = rr_true;
        again = rr_true > A.tol2;
    }
    HIPCHK(hipStreamSynchronize(st));
    if (timing) {
        double sum[9] = {0, 0, 0, 0, 0, 0, 0, 0, 0}; int nmul_n = 0;
        for (auto &pr : tsamples) { sum[pr.first] += pr.second; if (pr.first == 8) ++nmul_n; }
        TM.n = tphase;
        for (int c = 0; c < 8; ++c) TM.us[c] = tphase ? sum[c] * 1e3 / tphase : 0.0;
        TM.nmul_us = nmul_n ? sum[8] * 1e3 / nmul_n : 0.0;
        g_slab_last.nmul_us = TM.nmul_us;
    }
    return xtb_finish(h, !emu, again, prof, iters_out, rr_out);
}
