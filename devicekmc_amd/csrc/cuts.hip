// cuts.hip -- cut-site analysis of the bridged filament: the members every conducting path between the contacts crosses, from ONE left-to-right
// path, the connected components of the members off that path and the chords of the path (dkmc_find_cuts; definitions: include/devicekmc_hip.h,
// the rule and its proof sketch: DESIGN.md section 4).  No counterpart in the reference.  A pure function of its arguments: nothing of GPUBuffers,
// no engine state a later phase reads and no other kernel is touched.
//
// Positions: pos[site] = k for row k of the path, -1 elsewhere, by atomicMin of k into a word that starts at -1 read as unsigned: of two rows
//   that name one site the smaller k stays, so the later row is the one reported as the duplicate.  The validation pass (one group of LPR lanes per
//   path row) looks for row k - 1's site in the index row of row k's site and the other way round, and takes the smallest {row, reason} word.
// Labelling of the off-path members ("label in range and pos < 0"): the min-hooking + compression rounds of rounds.h (label_rounds, the ones
//   dkmc_find_clusters runs): d_site_bypass holds the roots between the rounds and ends on the smallest site index of each off-path component;
//   "rounds" is the number of rounds run, the one that changed nothing included, the number the synchronous host model (tests/cut_ref.py) gives.
// Attachment: one pass over the member rows, LPR lanes per row.  A link is seen from whichever row holds it: an off-path row collects the positions
//   of its path entries (and -1 / L as a seed) in registers, a wave whose rows share one root -- the rule inside a contact slab -- combines them
//   and sends one atomicMin / atomicMax pair; a path row sends the pair for each off-path entry and marks the chords among its path entries.
// Tables: the roots with hi - lo >= 2 add +1 at lo + 1 and -1 at hi to a difference array over the positions; the chords do the same in a second
//   one; prefix sums (scan.hip) give n_bypass and the chord flag.  The bypass table is compacted by root flag + scan, the necks by the flags of
//   the run starts + scan.  Integer atomics only (minima, maxima, counts): the same bytes on every call.
#include "rounds.h"
#include <vector>

#define CU_NT 256
#define CU_CAP_DEFAULT 64
#define CU_CAP_MAX ROUND_CAP_MAX
#define CU_NONE 0x7fffffff

namespace {

struct CuStat {
    unsigned long long err;          // the smallest {path row << 3 | reason} of an invalid path, ~0 if none
    int off_members, off_comps, n_byp, n_cut, max_nb, n_chord, n_necks, pad;
};
struct CutState {
    int valid = 0;
    long long info[16];
    ResultTable<4> path;             // site, n_bypass, chord, cut
    ResultTable<4> bypasses;         // root, size, lo, hi
    ResultTable<2, 2> necks;         // first, last; xmin, xmax
    double ms_label, ms_rest;
    PhaseTimer<3> timer;
    void reset()
    {
        memset(info, 0, sizeof(info));
        info[5] = -1;
        path.clear(); bypasses.clear(); necks.clear();
        ms_label = ms_rest = 0.0;
    }
} g_cu;
int g_cu_round_cap = CU_CAP_DEFAULT;

const char *const kReason[6] = {"", "is not a member", "repeats the site of an earlier row", "is not a left seed (row 0)", "is not a right seed (the last row)",
                                "is not linked to the row before"};

// 1a. identities of the per-site words
__global__ __launch_bounds__(CU_NT) void k_cu_init(int N, int *pos, int *lo, int *hi, int *csize)
{
    const int i = blockIdx.x * CU_NT + threadIdx.x;
    if (i >= N) return;
    pos[i] = -1; lo[i] = CU_NONE; hi[i] = -CU_NONE; csize[i] = 0;
}

// 1b. positions: rows that name no member are reported and scatter nothing
__global__ __launch_bounds__(CU_NT) void k_cu_scatter(int N, int L, const int *__restrict__ path, const int *__restrict__ label, int *pos, CuStat *stat)
{
    const int k = blockIdx.x * CU_NT + threadIdx.x;
    if (k >= L) return;
    const int s = path[k];
    bool ok = s >= 0 && s < N;
    if (ok) { const int r = label[s]; ok = r >= 0 && r < N; }
    if (!ok) atomicMin(&stat->err, ((unsigned long long)k << 3) | 1ull);
    else atomicMin((unsigned int *)&pos[s], (unsigned int)k);
}

// 1c. validation, LPR lanes per path row: distinct sites, the seeds at the two ends, consecutive rows linked (v in row u OR u in row v)
template <int LPR>
__global__ __launch_bounds__(CU_NT) void k_cu_validate(int N, int nn, int L, const int *__restrict__ idx, const int *__restrict__ path,
                                                       const int *__restrict__ pos, int n_left, int n_right, CuStat *stat)
{
    const int lane = threadIdx.x % LPR, gw = (threadIdx.x & (WAVE - 1)) / LPR;            // the group's place in its wave
    const long long groups = (long long)gridDim.x * (CU_NT / LPR);
    const long long wave0 = (long long)blockIdx.x * (CU_NT / LPR) + (threadIdx.x / WAVE) * (WAVE / LPR);
    for (long long k0 = wave0; k0 < L; k0 += groups) {                                    // the same trip count in every lane of a wave
        const long long k = k0 + gw;
        const int s = k < L ? path[k] : -1;
        const bool ok = s >= 0 && s < N && pos[s] >= 0;                                   // a member (else row k is reported already)
        const int t = (ok && k > 0) ? path[k - 1] : -1;
        const bool look = t >= 0 && t < N;                                                // else row k - 1 is reported already
        bool found = false;
        if (look) {
            const int *rs = idx + (size_t)s * nn, *rt = idx + (size_t)t * nn;
            for (int e = lane; e < nn; e += LPR) found = found || rs[e] == t || rt[e] == s;
        }
        const unsigned long long fm = __ballot(found);
        const unsigned long long gm = LPR == WAVE ? ~0ull : (((1ull << (LPR & 63)) - 1ull) << (gw * LPR));
        if (lane == 0 && ok) {
            int why = 0;
            if (pos[s] != (int)k) why = 2;
            else if (k == 0 && !(s < n_left)) why = 3;
            else if (k == L - 1 && !(s >= N - n_right)) why = 4;
            else if (look && !(fm & gm)) why = 5;
            if (why) atomicMin(&stat->err, ((unsigned long long)k << 3) | (unsigned long long)why);
        }
    }
}

// 2. off-path membership as the initial root / parent (the site itself, -1 for a non-member and for a path site)
__global__ __launch_bounds__(CU_NT) void k_cu_members(int N, const int *__restrict__ label, const int *__restrict__ pos, int *root, int *parent)
{
    const int i = blockIdx.x * CU_NT + threadIdx.x;
    if (i >= N) return;
    const int r = label[i];
    root[i] = parent[i] = (r >= 0 && r < N && pos[i] < 0) ? i : -1;
}

// 3. the rounds: label_rounds (rounds.h) on root[] / parent[]

// 4. attachment: lo / hi of the off-path roots and the chord marks, one pass over the member rows (root[u] >= 0: off-path, pos[u] >= 0: on the
// path, both -1: no member).  cdiff has L + 1 words.
template <int LPR>
__global__ __launch_bounds__(CU_NT) void k_cu_attach(int N, int nn, int L, const int *__restrict__ idx, const int *__restrict__ root,
                                                     const int *__restrict__ pos, int n_left, int n_right, int *lo, int *hi, int *cdiff)
{
    const int lane = threadIdx.x % LPR, gw = (threadIdx.x & (WAVE - 1)) / LPR;
    const long long groups = (long long)gridDim.x * (CU_NT / LPR);
    const long long wave0 = (long long)blockIdx.x * (CU_NT / LPR) + (threadIdx.x / WAVE) * (WAVE / LPR);
    for (long long u0 = wave0; u0 < N; u0 += groups) {                                    // the same trip count in every lane of a wave
        const long long u = u0 + gw;
        const int ru = u < N ? root[u] : -1, pu = u < N ? pos[u] : -1;
        int mylo = CU_NONE, myhi = -CU_NONE;
        if (ru >= 0 || pu >= 0) {
            const int *row = idx + (size_t)u * nn;
            for (int e = lane; e < nn; e += LPR) {
                const int v = row[e];
                if (v < 0 || v >= N) continue;                // padding, anywhere in the row
                const int pv = pos[v];
                if (ru >= 0) {
                    if (pv >= 0) { mylo = min(mylo, pv); myhi = max(myhi, pv); }
                } else {
                    const int rv = root[v];
                    if (rv >= 0) { atomicMin(&lo[rv], pu); atomicMax(&hi[rv], pu); }
                    else if (pv >= pu + 2) { atomicAdd(&cdiff[pu + 1], 1); atomicAdd(&cdiff[pv], -1); }
                    else if (pv >= 0 && pv <= pu - 2) { atomicAdd(&cdiff[pv + 1], 1); atomicAdd(&cdiff[pu], -1); }
                }
            }
            if (lane == 0) {
                const int f = seed_bits((int)u, N, n_left, n_right);
                if (ru >= 0) {
                    if (f & 1) { mylo = min(mylo, -1); myhi = max(myhi, -1); }
                    if (f & 2) { mylo = min(mylo, L); myhi = max(myhi, L); }
                } else {                                      // a path site that is a seed away from its end: the chord from S / to T
                    if ((f & 1) && pu >= 1) { atomicAdd(&cdiff[0], 1); atomicAdd(&cdiff[pu], -1); }
                    if ((f & 2) && pu <= L - 2) { atomicAdd(&cdiff[pu + 1], 1); atomicAdd(&cdiff[L], -1); }
                }
            }
        }
        const bool has = mylo != CU_NONE;
        const unsigned long long bm = __ballot(has);
        if (bm == 0ull) continue;
        const int first = __ffsll((long long)bm) - 1;
        const int r0 = __shfl(ru, first, WAVE);
        if (__all(!has || ru == r0)) {
            const int l = wave_min(mylo), h = wave_max(myhi);
            if ((int)(threadIdx.x & (WAVE - 1)) == first) { atomicMin(&lo[r0], l); atomicMax(&hi[r0], h); }
        } else if (has) {
            atomicMin(&lo[ru], mylo); atomicMax(&hi[ru], myhi);
        }
    }
}

// 5a. per site: the role of the off-path members (path sites: provisionally "other", k_cu_path decides), the sizes of the off-path components,
// the root flags of the bypass table and the +1 / -1 of the bypass roots in bdiff (L + 1 words; no root is wide when L == 0)
__global__ __launch_bounds__(CU_NT) void k_cu_sites(int N, const int *__restrict__ root, const int *__restrict__ pos, const int *__restrict__ lo,
                                                    const int *__restrict__ hi, int *csize, int *role, int *isbyp, int *bdiff, CuStat *stat)
{
    const int i = blockIdx.x * CU_NT + threadIdx.x;
    const int r = i < N ? root[i] : -1;
    const bool off = r >= 0;
    bool wide = false;
    if (off) {
        const int l = lo[r], h = hi[r];
        wide = l != CU_NONE && h - l >= 2;
        role[i] = l == CU_NONE ? DKMC_CUT_ROLE_APART : (wide ? DKMC_CUT_ROLE_BYPASS : DKMC_CUT_ROLE_SIDE);
        if (wide && r == i) { atomicAdd(&bdiff[l + 1], 1); atomicAdd(&bdiff[h], -1); }
    } else if (i < N) role[i] = pos[i] >= 0 ? DKMC_CUT_ROLE_PATH : DKMC_CUT_ROLE_NONE;
    if (i < N) isbyp[i] = (wide && r == i) ? 1 : 0;
    const unsigned long long bm = __ballot(off);
    if (bm == 0ull) return;
    const int nroot = __popcll(__ballot(off && r == i));
    const int first = __ffsll((long long)bm) - 1;
    const int r0 = __shfl(r, first, WAVE);
    if (__all(!off || r == r0)) {
        if ((int)(threadIdx.x & (WAVE - 1)) == first) atomicAdd(&csize[r0], __popcll(bm));
    } else if (off) atomicAdd(&csize[r], 1);
    if ((int)(threadIdx.x & (WAVE - 1)) == first) {
        atomicAdd(&stat->off_members, __popcll(bm));
        if (nroot) atomicAdd(&stat->off_comps, nroot);
    }
}

// 5b. the bypass table: one row per wide root, ascending (bpos = exclusive scan of the flags)
__global__ __launch_bounds__(CU_NT) void k_cu_table(int N, const int *__restrict__ isbyp, const int *__restrict__ bpos, const int *__restrict__ csize,
                                                    const int *__restrict__ lo, const int *__restrict__ hi, int *t_root, int *t_size, int *t_lo, int *t_hi)
{
    const int i = blockIdx.x * CU_NT + threadIdx.x;
    if (i >= N || !isbyp[i]) return;
    const int p = bpos[i];
    t_root[p] = i; t_size[p] = csize[i]; t_lo[p] = lo[i]; t_hi[p] = hi[i];
}

// 6a. the path table from the two scanned difference arrays (exclusive sums: the value at position k is word k + 1), the roles of the path
// sites, the flags of the neck starts and the identities of the necks' keys
__global__ __launch_bounds__(CU_NT) void k_cu_path(int L, const int *__restrict__ path, const int *__restrict__ bsum, const int *__restrict__ csum,
                                                   int *t_nb, int *t_ch, int *t_cut, int *start, int *role, unsigned long long *kmin,
                                                   unsigned long long *kmax, CuStat *stat)
{
    const int k = blockIdx.x * CU_NT + threadIdx.x;
    int nb = 0, ch = 0, cut = 0;
    if (k < L) {
        nb = bsum[k + 1]; ch = csum[k + 1] > 0 ? 1 : 0; cut = (nb == 0 && ch == 0) ? 1 : 0;
        const bool before = k > 0 && bsum[k] == 0 && csum[k] <= 0;
        t_nb[k] = nb; t_ch[k] = ch; t_cut[k] = cut; start[k] = (cut && !before) ? 1 : 0;
        role[path[k]] = cut ? DKMC_CUT_ROLE_CUT : DKMC_CUT_ROLE_PATH;
        kmin[k] = ~0ull; kmax[k] = 0ull;
    }
    const int ncut = __popcll(__ballot(cut)), nch = __popcll(__ballot(ch)), mx = wave_max(nb);
    if ((threadIdx.x & (WAVE - 1)) == 0) {
        if (ncut) atomicAdd(&stat->n_cut, ncut);
        if (nch) atomicAdd(&stat->n_chord, nch);
        if (mx > 0) atomicMax(&stat->max_nb, mx);
    }
}

// 6b. the necks: neck j = the j-th run of cut positions (nid = exclusive scan of the start flags); a wave inside one neck sends one pair of keys
__global__ __launch_bounds__(CU_NT) void k_cu_necks(int L, const int *__restrict__ path, const double *__restrict__ x, const int *__restrict__ t_cut,
                                                    const int *__restrict__ start, const int *__restrict__ nid, int *first, int *last,
                                                    unsigned long long *kmin, unsigned long long *kmax)
{
    const int k = blockIdx.x * CU_NT + threadIdx.x;
    const bool cut = k < L && t_cut[k];
    int j = -1;
    if (cut) {
        j = nid[k] + start[k] - 1;
        if (start[k]) first[j] = k;
        if (k == L - 1 || !t_cut[k + 1]) last[j] = k;
    }
    if (!x) return;                                           // the same in every thread
    const unsigned long long key = cut ? dbl_key(x[path[k]]) : 0ull;
    const unsigned long long bm = __ballot(cut);
    if (bm == 0ull) return;
    const int f = __ffsll((long long)bm) - 1;
    const int j0 = __shfl(j, f, WAVE);
    if (__all(!cut || j == j0)) {
        const unsigned long long l = wave_min(cut ? key : ~0ull), h = wave_max(cut ? key : 0ull);
        if ((int)(threadIdx.x & (WAVE - 1)) == f) { atomicMin(&kmin[j0], l); atomicMax(&kmax[j0], h); }
    } else if (cut) {
        atomicMin(&kmin[j], key); atomicMax(&kmax[j], key);
    }
}

}   // namespace

extern "C" {

void dkmc_debug_set_cut_round_cap(int cap) { g_cu_round_cap = clamp_round_cap(cap, CU_CAP_DEFAULT); }

int dkmc_debug_get_cut_times(double *ms2)
{
    NEED_FINISHED(g_cu.valid, "dkmc_debug_get_cut_times", "dkmc_find_cuts");
    if (ms2) { ms2[0] = g_cu.ms_label; ms2[1] = g_cu.ms_rest; }
    return 0;
}

int dkmc_find_cuts(int N, int nn, const int *d_index, const int *d_label, const double *d_site_x, int n_left_sites, int n_right_sites,
                   const int *d_path, int path_len, int *d_site_role, int *d_site_bypass)
{
    g_cu.valid = 0;
    if (N < 0 || nn < 1 || path_len < 0 || path_len > N || (N > 0 && (!d_index || !d_label || !d_site_role || !d_site_bypass)) || (path_len > 0 && !d_path))
        return dkmc_fail(3, "dkmc_find_cuts: bad arguments (N >= 0, nn >= 1, 0 <= path_len <= N, device arrays of N sites, a path of path_len sites)",
                         __FILE__, __LINE__);
    clamp_seeds(N, n_left_sites, n_right_sites);
    g_cu.reset();
    if (N == 0) { g_cu.valid = 1; return 0; }
    hipStream_t st = eng().stream;
    const int cap = g_cu_round_cap, L = path_len;
    const size_t n = (size_t)N, lp = (size_t)L + 1;
    int *site = (int *)scratch(S_CUT_SITE, 7 * n * sizeof(int));
    int *tab = (int *)scratch(S_CUT_TABLE, 4 * n * sizeof(int));
    char *rows = (char *)scratch(S_CUT_ROWS, lp * (2 * sizeof(unsigned long long) + 9 * sizeof(int)));
    int *ctrl = (int *)scratch(S_CUT_CTRL, (size_t)CU_CAP_MAX * sizeof(int) + sizeof(CuStat));
    if (!site || !tab || !rows || !ctrl) return eng().err_code;
    int *pos = site, *parent = pos + n, *lo = parent + n, *hi = lo + n, *csize = hi + n, *isbyp = csize + n, *bpos = isbyp + n;
    int *t_root = tab, *t_size = t_root + n, *t_lo = t_size + n, *t_hi = t_lo + n;
    unsigned long long *kmin = (unsigned long long *)rows, *kmax = kmin + lp;
    int *bdiff = (int *)(kmax + lp), *cdiff = bdiff + lp, *start = cdiff + lp, *nid = start + lp, *t_nb = nid + lp, *t_ch = t_nb + lp, *t_cut = t_ch + lp,
        *first = t_cut + lp, *last = first + lp;
    CuStat *d_stat = (CuStat *)(ctrl + CU_CAP_MAX);
    int *root = d_site_bypass;

    const int site_blocks = (N + CU_NT - 1) / CU_NT, path_blocks = (L + CU_NT - 1) / CU_NT;
    const int lpr = lpr_of(nn);
    const int row_blocks = grid_blocks((long long)N * lpr, CU_NT, 8192);
    CuStat h_stat;
    HIPCHK(g_cu.timer.start(eng().profiling != 0, st));
    HIPCHK(hipMemsetAsync(ctrl, 0, (size_t)CU_CAP_MAX * sizeof(int) + sizeof(CuStat), st));
    HIPCHK(hipMemsetAsync(&d_stat->err, 0xff, sizeof(unsigned long long), st));
    HIPCHK(hipMemsetAsync(bdiff, 0, 2 * lp * sizeof(int), st));
    hipLaunchKernelGGL(k_cu_init, dim3(site_blocks), dim3(CU_NT), 0, st, N, pos, lo, hi, csize);
    if (L > 0) {
        // positions and validation: nothing below reads the path before it is known to be one
        hipLaunchKernelGGL(k_cu_scatter, dim3(path_blocks), dim3(CU_NT), 0, st, N, L, d_path, d_label, pos, d_stat);
        const int vblocks = grid_blocks((long long)L * lpr, CU_NT, 8192);
        LAUNCH_LPR(lpr, k_cu_validate, dim3(vblocks), dim3(CU_NT), st, N, nn, L, d_index, d_path, (const int *)pos, n_left_sites, n_right_sites, d_stat);
        KCHK();
        HIPCHK(hipMemcpyAsync(&h_stat, d_stat, sizeof(CuStat), hipMemcpyDeviceToHost, st));
        HIPCHK(hipStreamSynchronize(st));
        if (h_stat.err != ~0ull) {
            const int why = (int)(h_stat.err & 7ull);
            char msg[240];
            snprintf(msg, sizeof(msg), "dkmc_find_cuts: not a left-to-right path over the member links: row %lld %s; site_role and site_bypass set to -1",
                     (long long)(h_stat.err >> 3), kReason[why >= 1 && why <= 5 ? why : 0]);
            return abandon(st, n, {d_site_role, d_site_bypass}, msg, __FILE__, __LINE__);
        }
    }
    hipLaunchKernelGGL(k_cu_members, dim3(site_blocks), dim3(CU_NT), 0, st, N, d_label, (const int *)pos, root, parent);
    KCHK();
    HIPCHK(g_cu.timer.mark(1, st));
    int rounds = 0;
    if (int rc = label_rounds(st, N, nn, d_index, root, parent, ctrl, cap, &rounds)) return rc;
    if (!rounds) {
        char msg[240];
        snprintf(msg, sizeof(msg), "dkmc_find_cuts: off-path labelling not finished after %d rounds (the cap: dkmc_debug_set_cut_round_cap); "
                 "site_role and site_bypass set to -1", cap);
        return abandon(st, n, {d_site_role, d_site_bypass}, msg, __FILE__, __LINE__);
    }
    HIPCHK(g_cu.timer.mark(2, st));
    // attachment, roles, tables
    if (L > 0)
        LAUNCH_LPR(lpr, k_cu_attach, dim3(row_blocks), dim3(CU_NT), st, N, nn, L, d_index, (const int *)root, (const int *)pos, n_left_sites, n_right_sites,
                   lo, hi, cdiff);
    hipLaunchKernelGGL(k_cu_sites, dim3(site_blocks), dim3(CU_NT), 0, st, N, (const int *)root, (const int *)pos, (const int *)lo, (const int *)hi, csize,
                       d_site_role, isbyp, bdiff, d_stat);
    KCHK();
    if (int rc = dkmc_exclusive_scan_i32(isbyp, bpos, N, &d_stat->n_byp)) return rc;
    hipLaunchKernelGGL(k_cu_table, dim3(site_blocks), dim3(CU_NT), 0, st, N, (const int *)isbyp, (const int *)bpos, (const int *)csize, (const int *)lo,
                       (const int *)hi, t_root, t_size, t_lo, t_hi);
    KCHK();
    if (L > 0) {
        if (int rc = dkmc_exclusive_scan_i32(bdiff, bdiff, L + 1, nullptr)) return rc;
        if (int rc = dkmc_exclusive_scan_i32(cdiff, cdiff, L + 1, nullptr)) return rc;
        hipLaunchKernelGGL(k_cu_path, dim3(path_blocks), dim3(CU_NT), 0, st, L, d_path, (const int *)bdiff, (const int *)cdiff, t_nb, t_ch, t_cut, start,
                           d_site_role, kmin, kmax, d_stat);
        KCHK();
        if (int rc = dkmc_exclusive_scan_i32(start, nid, L, &d_stat->n_necks)) return rc;
        hipLaunchKernelGGL(k_cu_necks, dim3(path_blocks), dim3(CU_NT), 0, st, L, d_path, d_site_x, (const int *)t_cut, (const int *)start, (const int *)nid,
                           first, last, kmin, kmax);
        KCHK();
    }
    HIPCHK(g_cu.timer.mark(3, st));
    HIPCHK(hipMemcpyAsync(&h_stat, d_stat, sizeof(CuStat), hipMemcpyDeviceToHost, st));
    HIPCHK(hipStreamSynchronize(st));
    // the host-side tables
    const size_t nb = (size_t)h_stat.n_byp, nk = (size_t)h_stat.n_necks;
    if (h_stat.n_byp < 0 || nb > n || h_stat.n_necks < 0 || nk > (size_t)L) return dkmc_fail(4, "dkmc_find_cuts: table counts outside their range", __FILE__, __LINE__);
    std::vector<unsigned long long> h_min(nk), h_max(nk);
    if (int rc = fetch_columns(st, g_cu.bypasses, nb, {t_root, t_size, t_lo, t_hi})) return rc;
    if (int rc = fetch_columns(st, g_cu.path, (size_t)L, {d_path, t_nb, t_ch, t_cut})) return rc;
    if (int rc = fetch_columns(st, g_cu.necks, nk, {first, last})) return rc;
    if (nk) {
        HIPCHK(hipMemcpyAsync(h_min.data(), kmin, nk * sizeof(unsigned long long), hipMemcpyDeviceToHost, st));
        HIPCHK(hipMemcpyAsync(h_max.data(), kmax, nk * sizeof(unsigned long long), hipMemcpyDeviceToHost, st));
    }
    HIPCHK(hipStreamSynchronize(st));
    const std::vector<int> &n_first = g_cu.necks.i[0], &n_last = g_cu.necks.i[1];
    long long longest = 0, longest_first = -1;
    for (size_t j = 0; j < nk; ++j) {
        key_range(d_site_x != nullptr, h_min[j], h_max[j], &g_cu.necks.d[0][j], &g_cu.necks.d[1][j]);     // a neck has a site: no empty row
        const long long len = (long long)n_last[j] - n_first[j] + 1;
        if (len > longest) { longest = len; longest_first = n_first[j]; }            // ascending rows: the smallest position on ties
    }
    const long long info[12] = {L > 0 ? 1 : 0, L, h_stat.n_cut, (long long)nk, longest, longest_first, (long long)nb, h_stat.off_comps, h_stat.off_members,
                                h_stat.max_nb, h_stat.n_chord, rounds};
    memcpy(g_cu.info, info, sizeof(info));
    float ms[3] = {0.f, 0.f, 0.f};
    HIPCHK(g_cu.timer.read(ms));
    g_cu.ms_label = ms[1]; g_cu.ms_rest = ms[0] + ms[2];
    g_cu.valid = 1;
    return 0;
}

int dkmc_get_cut_info(long long *info16)
{
    NEED_FINISHED(g_cu.valid, "dkmc_get_cut_info", "dkmc_find_cuts");
    if (info16) memcpy(info16, g_cu.info, sizeof(g_cu.info));
    return 0;
}

int dkmc_copy_cut_path(int capacity, int *h_site, int *h_n_bypass, int *h_chord, int *h_cut, int *rows_out)
{
    NEED_FINISHED(g_cu.valid, "dkmc_copy_cut_path", "dkmc_find_cuts");
    g_cu.path.copy_out(capacity, rows_out, {h_site, h_n_bypass, h_chord, h_cut});
    return 0;
}

int dkmc_copy_cut_bypasses(int capacity, int *h_root, int *h_size, int *h_lo, int *h_hi, int *rows_out)
{
    NEED_FINISHED(g_cu.valid, "dkmc_copy_cut_bypasses", "dkmc_find_cuts");
    g_cu.bypasses.copy_out(capacity, rows_out, {h_root, h_size, h_lo, h_hi});
    return 0;
}

int dkmc_copy_cut_necks(int capacity, int *h_first, int *h_last, double *h_xmin, double *h_xmax, int *rows_out)
{
    NEED_FINISHED(g_cu.valid, "dkmc_copy_cut_necks", "dkmc_find_cuts");
    g_cu.necks.copy_out(capacity, rows_out, {h_first, h_last}, {h_xmin, h_xmax});
    return 0;
}

}   // extern "C"
