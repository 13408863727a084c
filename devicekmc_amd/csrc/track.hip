// track.hip -- cluster tracking: two labellings of one device compared (dkmc_track_clusters; definitions: include/devicekmc_hip.h): the distinct
// (prev, now) pairs with their counts, one lineage row per component of either side (parents / children, main line, BORN ... ABSORBED), the per-site
// change code, the transition of the bridging verdict and the sites that closed or broke the filament.  No counterpart in the reference.  A pure
// function of its arguments: nothing of GPUBuffers, no engine state a later phase reads and no other kernel is touched.
//
// The pair set: an open-addressing table of 64-bit keys ((a + 1) << 32) | (b + 1) -- all ones cannot occur and marks a free slot -- with a
//   power-of-two capacity >= 2 N, linear probing, slots claimed by a 64-bit atomicCAS.  A key's slot depends on the order of arrival, nothing that
//   leaves the call does: count is a sum (atomicAdd), first_site a minimum (atomicMin), and the rows go out in ascending first_site -- flag the site
//   that IS its pair's first_site, scan, scatter -- so the slot numbers never show.  A probe sequence that has visited every slot sets the error word
//   and gives up (it cannot happen below half load; it does not spin).
// Wave combining: the contact slabs and every large cluster put one pair on whole waves.  A wave peels its leading lane's pair TR_PEEL times: the
//   lanes that carry it are counted by a ballot and the leading lane -- the smallest site of the group -- sends one insert, one atomicAdd and one
//   atomicMin for all of them; what is left after that goes lane by lane.  (The form of k_cl_summaries, which combines one root.)
// Lineage: per pair, by the thread of its first site: size += count on both components, one atomicAdd on n_children / n_parents and one 64-bit
//   atomicMax on the packed word (count << 32 | ~id) of main_child / main_parent: the larger count wins, the smaller id on ties -- the tie-break
//   is part of the word, so the order of arrival cannot matter.  Integer atomics only, no floating-point arithmetic: the same inputs give the same
//   bytes on every call.
#include "rounds.h"
#include <vector>

#define TR_NT 256
#define TR_PEEL 4                    // pairs a wave combines before its remaining lanes go one by one
#define TR_EMPTY (~0ull)
#define TR_NMAX (1 << 30)            // the slot numbers of the pair table stay below 2^31

namespace {

// control block.  The first 16 bytes start as all ones (identities of the minima), the rest as zero.
struct TrCtrl {
    unsigned long long kmin;
    unsigned bridge_prev, bridge_now;
    unsigned long long kmax;
    int err, n_pairs, n_prev, n_now, n_crit;
    int mainline, joined, left, regrouped, born, died, merged, split, pad;
};
// per-component words of one side, indexed by the component id
struct TrSide {
    int *size, *lone, *links, *flags;         // sites, count(id, -1), components of the other side it shares sites with, contact bits
    unsigned long long *best;                  // max over those of (count << 32 | ~other id); 0: none
};
struct TrackState {
    int valid = 0;
    long long info[16];
    double x2[2];
    ResultTable<4> pairs;            // the columns of dkmc_copy_track_pairs, _now, _prev and _critical, in their order
    ResultTable<6> now, prev;
    ResultTable<1> critical;
    double ms[2];
    PhaseTimer<2> timer;
    void reset()
    {
        const long long z[16] = {0, 0, 0, 0, 0, 0, 0, 0, -1, -1, 0, 0, 0, 0, 0, 0};
        memcpy(info, z, sizeof(z));
        x2[0] = INFINITY; x2[1] = -INFINITY;
        pairs.clear(); now.clear(); prev.clear(); critical.clear();
        ms[0] = ms[1] = 0.0;
    }
} g_tr;
int g_tr_hash = 0;

__device__ __forceinline__ int tr_side(int v, int N) { return (v >= 0 && v < N) ? v : -1; }
__device__ __forceinline__ unsigned long long tr_key(int a, int b) { return ((unsigned long long)(unsigned)(a + 1) << 32) | (unsigned)(b + 1); }
__device__ __forceinline__ unsigned long long tr_pack(int count, int id) { return ((unsigned long long)(unsigned)count << 32) | (unsigned)~id; }
__device__ __forceinline__ int tr_best_id(unsigned long long w) { return w ? (int)~(unsigned)w : -1; }
__device__ __forceinline__ unsigned long long tr_mix(unsigned long long x)
{
    x ^= x >> 30; x *= 0xbf58476d1ce4e5b9ull; x ^= x >> 27; x *= 0x94d049bb133111ebull; x ^= x >> 31;
    return x;
}

// the slot of key, claimed if the key is new; -1 (and the error word) after mask + 1 probes without one
__device__ __forceinline__ int tr_insert(unsigned long long *keys, unsigned mask, int mode, unsigned long long key, int *err)
{
    const unsigned h = mode ? mask : (unsigned)tr_mix(key) & mask;
    for (unsigned p = 0; ; ++p) {
        const unsigned s = (h + p) & mask;
        unsigned long long k = __hip_atomic_load(&keys[s], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        if (k == TR_EMPTY) k = atomicCAS(&keys[s], TR_EMPTY, key);
        if (k == TR_EMPTY || k == key) return (int)s;
        if (p == mask) break;                                 // every slot seen
    }
    atomicOr(err, 1);
    return -1;
}

// 1. the pair pass: every site with a side finds or claims the slot of its pair; count, first_site, the contact bits of both components
__global__ __launch_bounds__(TR_NT) void k_tr_pairs(int N, const int *lp, const int *ln, int n_left, int n_right, unsigned mask, int mode,
                                                    unsigned long long *keys, unsigned *first, int *cnt, int *fprev, int *fnow, int *slot,
                                                    TrCtrl *ctrl)
{
    const int i = blockIdx.x * TR_NT + threadIdx.x;
    const int lane = threadIdx.x & 63;
    const bool in = i < N;
    const int a = in ? tr_side(lp[i], N) : -1, b = in ? tr_side(ln[i], N) : -1;
    const bool has = a >= 0 || b >= 0;
    const unsigned long long key = tr_key(a, b);
    const int f = has ? seed_bits(i, N, n_left, n_right) : 0;
    int s = -1;
    unsigned long long todo = __ballot(has);
    for (int round = 0; round < TR_PEEL && todo; ++round) {
        const int lead = __ffsll((long long)todo) - 1;
        const unsigned long long k0 = __shfl(key, lead, WAVE);
        const bool match = ((todo >> lane) & 1ull) && key == k0;
        const unsigned long long mm = __ballot(match);
        const int ff = (__ballot(match && (f & 1)) ? 1 : 0) | (__ballot(match && (f & 2)) ? 2 : 0);
        int s0 = -1;
        if (lane == lead) {                                   // the smallest site of the group
            s0 = tr_insert(keys, mask, mode, key, &ctrl->err);
            if (s0 >= 0) { atomicAdd(&cnt[s0], __popcll(mm)); atomicMin(&first[s0], (unsigned)i); }
            if (ff) { if (a >= 0) atomicOr(&fprev[a], ff); if (b >= 0) atomicOr(&fnow[b], ff); }
        }
        s0 = __shfl(s0, lead, WAVE);
        if (match) s = s0;
        todo &= ~mm;
    }
    if ((todo >> lane) & 1ull) {
        s = tr_insert(keys, mask, mode, key, &ctrl->err);
        if (s >= 0) { atomicAdd(&cnt[s], 1); atomicMin(&first[s], (unsigned)i); }
        if (f) { if (a >= 0) atomicOr(&fprev[a], f); if (b >= 0) atomicOr(&fnow[b], f); }
    }
    if (in) slot[i] = s;
}

// 2. per pair, by the thread of its first site: sizes, lone counts, links and the main line of both components
__global__ __launch_bounds__(TR_NT) void k_tr_links(int N, const int *lp, const int *ln, const int *slot, const unsigned *first, const int *cnt,
                                                    int *isfirst, TrSide P, TrSide Q)
{
    const int i = blockIdx.x * TR_NT + threadIdx.x;
    if (i >= N) return;
    const int s = slot[i];
    const bool rep = s >= 0 && first[s] == (unsigned)i;
    isfirst[i] = rep ? 1 : 0;
    if (!rep) return;
    const int a = tr_side(lp[i], N), b = tr_side(ln[i], N), c = cnt[s];
    if (a >= 0) atomicAdd(&P.size[a], c);
    if (b >= 0) atomicAdd(&Q.size[b], c);
    if (a >= 0 && b >= 0) {
        atomicAdd(&P.links[a], 1); atomicAdd(&Q.links[b], 1);
        atomicMax(&P.best[a], tr_pack(c, b)); atomicMax(&Q.best[b], tr_pack(c, a));
    }
    else if (a >= 0) P.lone[a] = c;                          // the pair (a, -1) exists once
    else Q.lone[b] = c;
}

// 3. per component id: the row flags of both tables, the bridging roots, the counts of BORN / DIED / MERGED / SPLIT rows
__global__ __launch_bounds__(TR_NT) void k_tr_comps(int N, TrSide P, TrSide Q, int *occ_prev, int *occ_now, TrCtrl *ctrl)
{
    const int i = blockIdx.x * TR_NT + threadIdx.x;
    const bool in = i < N;
    const bool sp = in && P.size[i] > 0, sn = in && Q.size[i] > 0;
    if (in) { occ_prev[i] = sp ? 1 : 0; occ_now[i] = sn ? 1 : 0; }
    if (sp && P.flags[i] == 3) atomicMin(&ctrl->bridge_prev, (unsigned)i);
    if (sn && Q.flags[i] == 3) atomicMin(&ctrl->bridge_now, (unsigned)i);
    const int lp_ = sp ? P.links[i] : -1, lq = sn ? Q.links[i] : -1;
    const int died = __popcll(__ballot(lp_ == 0)), split = __popcll(__ballot(lp_ >= 2));
    const int born = __popcll(__ballot(lq == 0)), merged = __popcll(__ballot(lq >= 2));
    if ((threadIdx.x & 63) == 0) {
        if (died) atomicAdd(&ctrl->died, died);
        if (split) atomicAdd(&ctrl->split, split);
        if (born) atomicAdd(&ctrl->born, born);
        if (merged) atomicAdd(&ctrl->merged, merged);
    }
}

// 4. per site: the change code, the critical flag at a closing or rupturing transition, the site counts and the x range of the critical sites
__global__ __launch_bounds__(TR_NT) void k_tr_sites(int N, const int *lp, const int *ln, const double *x, TrSide P, TrSide Q, int *site_change,
                                                    int *crit, TrCtrl *ctrl)
{
    const int i = blockIdx.x * TR_NT + threadIdx.x;
    const bool in = i < N;
    const int a = in ? tr_side(lp[i], N) : -1, b = in ? tr_side(ln[i], N) : -1;
    int code = 0;
    if (a >= 0 && b >= 0) code = (tr_best_id(P.best[a]) == b && tr_best_id(Q.best[b]) == a) ? 1 : 4;
    else if (b >= 0) code = 2;
    else if (a >= 0) code = 3;
    const unsigned bp = ctrl->bridge_prev, bn = ctrl->bridge_now;       // written by the launch before this one
    const int transition = (bp != ~0u ? 2 : 0) | (bn != ~0u ? 1 : 0);
    const bool cr = (transition == 1 && code == 2 && (unsigned)b == bn) || (transition == 2 && code == 3 && (unsigned)a == bp);
    if (in) { site_change[i] = code; crit[i] = cr ? 1 : 0; }
    const int n1 = __popcll(__ballot(code == 1)), n2 = __popcll(__ballot(code == 2)), n3 = __popcll(__ballot(code == 3)), n4 = __popcll(__ballot(code == 4));
    const unsigned long long cm = __ballot(cr);
    unsigned long long lo = TR_EMPTY, hi = 0ull;
    if (cm && x) {
        const unsigned long long k = cr ? dbl_key(x[i]) : 0ull;
        lo = wave_min(cr ? k : TR_EMPTY); hi = wave_max(k);
    }
    if ((threadIdx.x & 63) == 0) {
        if (n1) atomicAdd(&ctrl->mainline, n1);
        if (n2) atomicAdd(&ctrl->joined, n2);
        if (n3) atomicAdd(&ctrl->left, n3);
        if (n4) atomicAdd(&ctrl->regrouped, n4);
        if (cm && x) { atomicMin(&ctrl->kmin, lo); atomicMax(&ctrl->kmax, hi); }
    }
}

// the rows of one call, ints: 4 columns of n_pairs, 6 of n_now, 6 of n_prev, the critical sites
struct TrRows { int *pairs, *now, *prev, *crit; size_t np, nn, nv, nc; };
TrRows rows_of(int *base, size_t np, size_t nn, size_t nv, size_t nc)
{
    TrRows r;
    r.pairs = base; r.now = r.pairs + 4 * np; r.prev = r.now + 6 * nn; r.crit = r.prev + 6 * nv;
    r.np = np; r.nn = nn; r.nv = nv; r.nc = nc;
    return r;
}

// 5. the tables: pair rows in ascending first_site, component rows in ascending id, critical sites in ascending index (pos = exclusive scans)
__global__ __launch_bounds__(TR_NT) void k_tr_scatter(int N, const int *lp, const int *ln, const int *slot, const int *cnt, const int *flags4,
                                                      const int *pos4, TrSide P, TrSide Q, TrRows R)
{
    const int i = blockIdx.x * TR_NT + threadIdx.x;
    if (i >= N) return;
    const size_t n = (size_t)N;
    if (flags4[i]) {
        const size_t p = (size_t)pos4[i];
        R.pairs[p] = tr_side(lp[i], N); R.pairs[R.np + p] = tr_side(ln[i], N); R.pairs[2 * R.np + p] = cnt[slot[i]]; R.pairs[3 * R.np + p] = i;
    }
    if (flags4[n + i]) {                                      // prev row: DIED 4, SPLIT 8, ABSORBED 16
        const size_t p = (size_t)pos4[n + i];
        const int links = P.links[i], mc = tr_best_id(P.best[i]);
        R.prev[p] = i; R.prev[R.nv + p] = P.size[i]; R.prev[2 * R.nv + p] = P.lone[i]; R.prev[3 * R.nv + p] = links; R.prev[4 * R.nv + p] = mc;
        R.prev[5 * R.nv + p] = P.flags[i] | (links == 0 ? 4 : 0) | (links >= 2 ? 8 : 0) | ((mc >= 0 && Q.links[mc] >= 2) ? 16 : 0);
    }
    if (flags4[2 * n + i]) {                                  // now row: BORN 4, MERGED 8, FRAGMENT 16
        const size_t p = (size_t)pos4[2 * n + i];
        const int links = Q.links[i], mp = tr_best_id(Q.best[i]);
        R.now[p] = i; R.now[R.nn + p] = Q.size[i]; R.now[2 * R.nn + p] = Q.lone[i]; R.now[3 * R.nn + p] = links; R.now[4 * R.nn + p] = mp;
        R.now[5 * R.nn + p] = Q.flags[i] | (links == 0 ? 4 : 0) | (links >= 2 ? 8 : 0) | ((mp >= 0 && P.links[mp] >= 2) ? 16 : 0);
    }
    if (flags4[3 * n + i]) R.crit[pos4[3 * n + i]] = i;
}

TrSide side_of(char *base, size_t n)
{
    TrSide s;
    s.best = (unsigned long long *)base;
    s.size = (int *)(s.best + n); s.lone = s.size + n; s.links = s.lone + n; s.flags = s.links + n;
    return s;
}

// `rows` rows of T from the packed columns at src (the layout of rows_of); the end of what was read
template <int NI>
const int *unpack(ResultTable<NI> &T, size_t rows, const int *src)
{
    T.resize(rows);
    for (int c = 0; c < NI && rows; ++c) memcpy(T.i[c].data(), src + c * rows, rows * sizeof(int));
    return src + NI * rows;
}

}   // namespace

extern "C" {

void dkmc_debug_set_track_hash(int mode) { g_tr_hash = mode == 1 ? 1 : 0; }

int dkmc_debug_get_track_times(double *ms2)
{
    NEED_FINISHED(g_tr.valid, "dkmc_debug_get_track_times", "dkmc_track_clusters");
    if (ms2) memcpy(ms2, g_tr.ms, sizeof(g_tr.ms));
    return 0;
}

int dkmc_track_clusters(int N, const int *d_label_prev, const int *d_label_now, const double *d_site_x, int n_left_sites, int n_right_sites,
                        int *d_site_change)
{
    g_tr.valid = 0;
    if (N < 0 || N > TR_NMAX || (N > 0 && (!d_label_prev || !d_label_now || !d_site_change)))
        return dkmc_fail(3, "dkmc_track_clusters: bad arguments (0 <= N <= 2^30, device arrays of N sites: label_prev, label_now, site_change)", __FILE__, __LINE__);
    clamp_seeds(N, n_left_sites, n_right_sites);
    g_tr.reset();
    if (N == 0) { g_tr.valid = 1; return 0; }
    hipStream_t st = eng().stream;
    const size_t n = (size_t)N;
    size_t cap = 2;
    while (cap < 2 * n) cap <<= 1;
    char *hash = (char *)scratch(S_TR_HASH, cap * (sizeof(unsigned long long) + sizeof(unsigned) + sizeof(int)));
    char *comp = (char *)scratch(S_TR_COMP, 2 * n * (sizeof(unsigned long long) + 4 * sizeof(int)));
    int *site = (int *)scratch(S_TR_SITE, 9 * n * sizeof(int));
    TrCtrl *ctrl = (TrCtrl *)scratch(S_TR_CTRL, sizeof(TrCtrl));
    if (!hash || !comp || !site || !ctrl) return eng().err_code;
    unsigned long long *keys = (unsigned long long *)hash;
    unsigned *first = (unsigned *)(keys + cap);
    int *cnt = (int *)(first + cap);
    const TrSide P = side_of(comp, n), Q = side_of(comp + n * (sizeof(unsigned long long) + 4 * sizeof(int)), n);
    int *slot = site, *flags4 = site + n, *pos4 = site + 5 * n;           // flags / positions: pair firsts, prev ids, now ids, critical sites
    const bool timed = eng().profiling != 0;

    const int blocks = (N + TR_NT - 1) / TR_NT;
    HIPCHK(g_tr.timer.start(timed, st));
    HIPCHK(hipMemsetAsync(keys, 0xff, cap * (sizeof(unsigned long long) + sizeof(unsigned)), st));      // free slots, first_site = the identity of the minimum
    HIPCHK(hipMemsetAsync(cnt, 0, cap * sizeof(int), st));
    HIPCHK(hipMemsetAsync(comp, 0, 2 * n * (sizeof(unsigned long long) + 4 * sizeof(int)), st));
    HIPCHK(hipMemsetAsync(ctrl, 0xff, 16, st));
    HIPCHK(hipMemsetAsync((char *)ctrl + 16, 0, sizeof(TrCtrl) - 16, st));
    hipLaunchKernelGGL(k_tr_pairs, dim3(blocks), dim3(TR_NT), 0, st, N, d_label_prev, d_label_now, n_left_sites, n_right_sites, (unsigned)(cap - 1), g_tr_hash,
                       keys, first, cnt, P.flags, Q.flags, slot, ctrl);
    KCHK();
    HIPCHK(g_tr.timer.mark(1, st));
    hipLaunchKernelGGL(k_tr_links, dim3(blocks), dim3(TR_NT), 0, st, N, d_label_prev, d_label_now, (const int *)slot, (const unsigned *)first, (const int *)cnt,
                       flags4, P, Q);
    hipLaunchKernelGGL(k_tr_comps, dim3(blocks), dim3(TR_NT), 0, st, N, P, Q, flags4 + n, flags4 + 2 * n, ctrl);
    hipLaunchKernelGGL(k_tr_sites, dim3(blocks), dim3(TR_NT), 0, st, N, d_label_prev, d_label_now, d_site_x, P, Q, d_site_change, flags4 + 3 * n, ctrl);
    KCHK();
    int *totals[4] = {&ctrl->n_pairs, &ctrl->n_prev, &ctrl->n_now, &ctrl->n_crit};
    for (int k = 0; k < 4; ++k)
        if (int rc = dkmc_exclusive_scan_i32(flags4 + k * n, pos4 + k * n, N, totals[k])) return rc;
    TrCtrl h;
    HIPCHK(hipMemcpyAsync(&h, ctrl, sizeof(TrCtrl), hipMemcpyDeviceToHost, st));
    HIPCHK(hipStreamSynchronize(st));
    if (h.err) return dkmc_fail(4, "dkmc_track_clusters: a pair found no slot after probing the whole pair table", __FILE__, __LINE__);
    if (h.n_pairs < 0 || h.n_pairs > N || h.n_prev < 0 || h.n_prev > N || h.n_now < 0 || h.n_now > N || h.n_crit < 0 || h.n_crit > N)
        return dkmc_fail(4, "dkmc_track_clusters: row counts outside 0 ... N", __FILE__, __LINE__);
    const size_t np = (size_t)h.n_pairs, nv = (size_t)h.n_prev, nn = (size_t)h.n_now, nc = (size_t)h.n_crit, total = 4 * np + 6 * nn + 6 * nv + nc;
    std::vector<int> rows(total);
    if (total) {
        int *d_rows = (int *)scratch(S_TR_ROWS, total * sizeof(int));
        if (!d_rows) return eng().err_code;
        hipLaunchKernelGGL(k_tr_scatter, dim3(blocks), dim3(TR_NT), 0, st, N, d_label_prev, d_label_now, (const int *)slot, (const int *)cnt, (const int *)flags4,
                           (const int *)pos4, P, Q, rows_of(d_rows, np, nn, nv, nc));
        KCHK();
        HIPCHK(g_tr.timer.mark(2, st));
        HIPCHK(hipMemcpyAsync(rows.data(), d_rows, total * sizeof(int), hipMemcpyDeviceToHost, st));
        HIPCHK(hipStreamSynchronize(st));
    }
    else if (timed) { HIPCHK(g_tr.timer.mark(2, st)); HIPCHK(hipStreamSynchronize(st)); }
    const int *src = unpack(g_tr.pairs, np, rows.data());
    src = unpack(g_tr.now, nn, src);
    src = unpack(g_tr.prev, nv, src);
    unpack(g_tr.critical, nc, src);
    const int bp = (int)h.bridge_prev, bn = (int)h.bridge_now;          // all ones = -1: none
    const long long info[16] = {h.n_prev, h.n_now, h.n_pairs, (long long)h.mainline + h.regrouped, h.joined, h.left, h.regrouped,
                                (bp >= 0 ? 2 : 0) | (bn >= 0 ? 1 : 0), bp, bn, h.born, h.died, h.merged, h.split, h.n_crit, 0};
    memcpy(g_tr.info, info, sizeof(info));
    key_range(d_site_x && h.n_crit > 0, h.kmin, h.kmax, &g_tr.x2[0], &g_tr.x2[1]);      // else the empty range of the reset
    float ms[2] = {0.f, 0.f};
    HIPCHK(g_tr.timer.read(ms));
    g_tr.ms[0] = ms[0]; g_tr.ms[1] = ms[1];
    g_tr.valid = 1;
    return 0;
}

int dkmc_get_track_info(long long *info16, double *x2)
{
    NEED_FINISHED(g_tr.valid, "dkmc_get_track_info", "dkmc_track_clusters");
    if (info16) memcpy(info16, g_tr.info, sizeof(g_tr.info));
    if (x2) memcpy(x2, g_tr.x2, sizeof(g_tr.x2));
    return 0;
}

int dkmc_copy_track_pairs(int capacity, int *h_prev, int *h_now, int *h_count, int *h_first_site, int *rows_out)
{
    NEED_FINISHED(g_tr.valid, "dkmc_copy_track_pairs", "dkmc_track_clusters");
    g_tr.pairs.copy_out(capacity, rows_out, {h_prev, h_now, h_count, h_first_site});
    return 0;
}

int dkmc_copy_track_now(int capacity, int *h_root, int *h_size, int *h_joined, int *h_n_parents, int *h_main_parent, int *h_flags, int *rows_out)
{
    NEED_FINISHED(g_tr.valid, "dkmc_copy_track_now", "dkmc_track_clusters");
    g_tr.now.copy_out(capacity, rows_out, {h_root, h_size, h_joined, h_n_parents, h_main_parent, h_flags});
    return 0;
}

int dkmc_copy_track_prev(int capacity, int *h_root, int *h_size, int *h_left, int *h_n_children, int *h_main_child, int *h_flags, int *rows_out)
{
    NEED_FINISHED(g_tr.valid, "dkmc_copy_track_prev", "dkmc_track_clusters");
    g_tr.prev.copy_out(capacity, rows_out, {h_root, h_size, h_left, h_n_children, h_main_child, h_flags});
    return 0;
}

int dkmc_copy_track_critical(int capacity, int *h_site, int *rows_out)
{
    NEED_FINISHED(g_tr.valid, "dkmc_copy_track_critical", "dkmc_track_clusters");
    g_tr.critical.copy_out(capacity, rows_out, {h_site});
    return 0;
}

}   // extern "C"
