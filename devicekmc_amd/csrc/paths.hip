// paths.hip -- conduction-path analysis of the bridged filament: hop distances from both contacts over the member links, the canonical shortest
// path, the corridor's level profile and its constriction (dkmc_find_paths; definitions: include/devicekmc_hip.h).  No counterpart in the
// reference.  A pure function of its arguments: nothing of GPUBuffers, no engine state a later phase reads and no other kernel is touched.
//
// Labelling: level-synchronous breadth-first search from both contacts at once, the kernel boundary is the only synchronisation point.
//   hop[] holds one pair of words per site, {hops_left, hops_right}: -2 for a non-member, -1 for a member not reached yet.  Before round k every
//   word below or at k is final (induction over the rounds).  Round k looks at every index entry between two members u, v and, in each field on
//   its own, turns the end that holds -1 into k + 1 where the other end holds k.  A word is written in round k only if it held -1 when the round
//   began and has a linked member at k -- a property of the state BEFORE the round --, and every writer of it writes k + 1: the words written and
//   their values do not depend on the order of the lanes.  A reader that races with such a store sees -1 or k + 1; neither is k, so it starts
//   nothing from it, and at most it repeats the store of k + 1.  No atomic read-modify-write is needed, and the state after the launch is a
//   function of the state before it.  A round's change word is set by a lane that saw -1 and wrote, so it is set exactly when the round had
//   something to write: the first round that sets nothing in either field ends the loop, and "rounds" -- that round included -- is
//   max(largest hops_left, largest hops_right, 0) + 1, the number the synchronous host model (tests/path_ref.py) gives.
// Work shape: one pass over a row serves both fields (one 8-byte read per entry).  Non-members are skipped in place, and so is a member whose
//   two words are both settled below k (its links were all used in an earlier round).  A member row is read by LPR lanes, 16 up to 128 entries per
//   row and the whole wave above (the shape of k_lab_hook, rounds.h).  The host loop is run_rounds (rounds.h): ROUND_BATCH rounds are enqueued
//   per read-back of their change words.
// After the rounds: H = the smallest hops_left on a right seed; the corridor's rows (count, min and max of the x keys per hops_left) by integer
//   atomics, combined inside a wave whose corridor sites share a level and privatised in LDS when the rows fit; the predecessors of the sites on
//   shortest paths by one atomicMin pass, walked from the end site by one thread.  Integer atomics only: the same bytes on every call.
#include "rounds.h"
#include <vector>

#define PT_NT 256
#define PT_CAP_MAX ROUND_CAP_MAX
#define PT_SLACK_MAX 65536
#define PT_LDS_ROWS 1024             // profile rows privatised per workgroup: 20 bytes each
#define PT_NONE 0x7fffffff

namespace {

struct PtStat { int H, end, reached_left, reached_right; };
struct PathState {
    int valid = 0;
    long long info[8];
    ResultTable<1> path;             // site
    ResultTable<1, 2> profile;       // count; xmin, xmax
    double ms[2];
    PhaseTimer<2> timer;
    void reset()
    {
        const long long z[8] = {0, -1, 0, 0, 0, 0, -1, 0};
        memcpy(info, z, sizeof(z));
        path.clear(); profile.clear();
        ms[0] = ms[1] = 0.0;
    }
} g_pt;
int g_pt_round_cap = PT_CAP_MAX;

// 1. seeds: {0 on a seed, -1 on any other member, -2 on a non-member} in both fields; the predecessor words at their identity
__global__ __launch_bounds__(PT_NT) void k_pt_init(int N, const int *__restrict__ label, int n_left, int n_right, int2 *hop, int *pred)
{
    const int i = blockIdx.x * PT_NT + threadIdx.x;
    if (i >= N) return;
    const int r = label[i];
    const bool m = r >= 0 && r < N;
    const int f = seed_bits(i, N, n_left, n_right);
    hop[i] = m ? make_int2((f & 1) ? 0 : -1, (f & 2) ? 0 : -1) : make_int2(-2, -2);
    pred[i] = PT_NONE;
}

// 2. round k: LPR lanes per member row, both fields in one pass
template <int LPR>
__global__ __launch_bounds__(PT_NT) void k_pt_round(int N, int nn, const int *__restrict__ idx, int2 *hop, int *ctrl, int k)
{
    if (k > 0 && ctrl[k - 1] == 0) return;                    // the round before changed nothing: the labelling is finished
    const int lane = threadIdx.x % LPR;
    const long long groups = (long long)gridDim.x * (PT_NT / LPR);
    int changed = 0;
    for (long long u = (long long)blockIdx.x * (PT_NT / LPR) + threadIdx.x / LPR; u < N; u += groups) {
        const int2 hu = ld_pair(&hop[u]);
        if (hu.x == -2) continue;                             // not a member
        const bool al = hu.x == k || hu.x == -1, ar = hu.y == k || hu.y == -1;
        if (!al && !ar) continue;                             // both settled below k (or just set to k + 1): nothing to give, nothing to take
        const int *row = idx + (size_t)u * nn;
        for (int e = lane; e < nn; e += LPR) {
            const int v = row[e];
            if (v < 0 || v >= N) continue;                    // padding, anywhere in the row
            const int2 hv = ld_pair(&hop[v]);
            if (hv.x == -2) continue;
            if (hu.x == k && hv.x == -1) { st_agent(&hop[v].x, k + 1); changed = 1; }
            else if (hu.x == -1 && hv.x == k) { st_agent(&hop[u].x, k + 1); changed = 1; }
            if (hu.y == k && hv.y == -1) { st_agent(&hop[v].y, k + 1); changed = 1; }
            else if (hu.y == -1 && hv.y == k) { st_agent(&hop[u].y, k + 1); changed = 1; }
        }
    }
    if (changed) atomicOr(&ctrl[k], 1);
}

// 3a. the two output arrays, the members reached from either side, H = the smallest hops_left on a right seed
__global__ __launch_bounds__(PT_NT) void k_pt_finish(int N, const int2 *__restrict__ hop, int n_right, int *hl, int *hr, PtStat *stat)
{
    const int i = blockIdx.x * PT_NT + threadIdx.x;
    int l = -1, r = -1;
    if (i < N) {
        const int2 h = hop[i];
        l = h.x < 0 ? -1 : h.x; r = h.y < 0 ? -1 : h.y;
        hl[i] = l; hr[i] = r;
    }
    const int nl = __popcll(__ballot(l >= 0)), nr = __popcll(__ballot(r >= 0));
    const int h = wave_min((i < N && i >= N - n_right && l >= 0) ? l : PT_NONE);
    if ((threadIdx.x & (WAVE - 1)) == 0) {
        if (nl) atomicAdd(&stat->reached_left, nl);
        if (nr) atomicAdd(&stat->reached_right, nr);
        if (h != PT_NONE) atomicMin(&stat->H, h);
    }
}

// 3b. the corridor's rows, R of them (R > H + slack), and the end site of the path.  LDS = 1: the rows are privatised per workgroup (R <=
// PT_LDS_ROWS).  Integer atomics only; a wave whose corridor sites share one level -- the rule inside a contact layer -- sends one set of them.
template <int LDS>
__global__ __launch_bounds__(PT_NT) void k_pt_profile(int N, const int *__restrict__ hl, const int *__restrict__ hr, const double *__restrict__ x,
                                                      int slack, int n_right, int R, PtStat *stat, int *cnt, unsigned long long *kmin,
                                                      unsigned long long *kmax)
{
    __shared__ int s_cnt[LDS ? PT_LDS_ROWS : 1];
    __shared__ unsigned long long s_min[LDS ? PT_LDS_ROWS : 1], s_max[LDS ? PT_LDS_ROWS : 1];
    const int H = stat->H;
    if (H == PT_NONE) return;                                 // status 0: no rows (the same in every thread)
    if (LDS) {
        for (int j = threadIdx.x; j < R; j += PT_NT) { s_cnt[j] = 0; s_min[j] = ~0ull; s_max[j] = 0ull; }
        __syncthreads();
    }
    int *c_ = LDS ? s_cnt : cnt;
    unsigned long long *lo_ = LDS ? s_min : kmin, *hi_ = LDS ? s_max : kmax;
    const long long top = (long long)H + slack;
    for (long long base = (long long)blockIdx.x * PT_NT; base < N; base += (long long)gridDim.x * PT_NT) {
        const long long i = base + threadIdx.x;
        const int l = i < N ? hl[i] : -1, r = i < N ? hr[i] : -1;
        const bool in = l >= 0 && r >= 0 && (long long)l + r <= top && l < R;
        if (l == H && i >= N - n_right && i < N) atomicMin(&stat->end, (int)i);
        const unsigned long long key = (in && x) ? dbl_key(x[i]) : 0ull;
        const unsigned long long bm = __ballot(in);
        if (bm == 0ull) continue;
        const int first = __ffsll((long long)bm) - 1;
        const int l0 = __shfl(l, first, WAVE);
        if (__all(!in || l == l0)) {
            const unsigned long long lo = wave_min(in ? key : ~0ull), hi = wave_max(in ? key : 0ull);
            if ((int)(threadIdx.x & (WAVE - 1)) == first) {
                atomicAdd(&c_[l0], __popcll(bm));
                if (x) { atomicMin(&lo_[l0], lo); atomicMax(&hi_[l0], hi); }
            }
        } else if (in) {
            atomicAdd(&c_[l], 1);
            if (x) { atomicMin(&lo_[l], key); atomicMax(&hi_[l], key); }
        }
    }
    if (LDS) {
        __syncthreads();
        for (int j = threadIdx.x; j < R; j += PT_NT) {
            const int c = s_cnt[j];
            if (c == 0) continue;
            atomicAdd(&cnt[j], c);
            if (x) { atomicMin(&kmin[j], s_min[j]); atomicMax(&kmax[j], s_max[j]); }
        }
    }
}

__global__ __launch_bounds__(PT_NT) void k_pt_rows_init(int R, int *cnt, unsigned long long *kmin, unsigned long long *kmax, int *path, PtStat *stat)
{
    const int j = blockIdx.x * PT_NT + threadIdx.x;
    if (j == 0) { stat->H = PT_NONE; stat->end = PT_NONE; stat->reached_left = 0; stat->reached_right = 0; }
    if (j >= R) return;
    cnt[j] = 0; kmin[j] = ~0ull; kmax[j] = 0ull; path[j] = -1;
}

// 3c. predecessors: for every link between two sites that lie on shortest paths (hops_left + hops_right == H), the end one hop nearer to the
// left is a candidate predecessor of the other; the smallest index wins.  (The candidates of a site on a shortest path all lie on one.)
template <int LPR>
__global__ __launch_bounds__(PT_NT) void k_pt_pred(int N, int nn, const int *__restrict__ idx, const int *__restrict__ hl, const int *__restrict__ hr,
                                                   const PtStat *stat, int *pred)
{
    const int H = stat->H;
    if (H == PT_NONE) return;
    const int lane = threadIdx.x % LPR;
    const long long groups = (long long)gridDim.x * (PT_NT / LPR);
    for (long long u = (long long)blockIdx.x * (PT_NT / LPR) + threadIdx.x / LPR; u < N; u += groups) {
        const int lu = hl[u], ru = hr[u];
        if (lu < 0 || ru < 0 || lu + ru != H) continue;
        const int *row = idx + (size_t)u * nn;
        for (int e = lane; e < nn; e += LPR) {
            const int v = row[e];
            if (v < 0 || v >= N) continue;
            const int lv = hl[v], rv = hr[v];
            if (lv < 0 || rv < 0 || lv + rv != H) continue;
            if (lv == lu + 1) atomicMin(&pred[v], (int)u);
            else if (lu == lv + 1) atomicMin(&pred[u], v);
        }
    }
}

// 3d. the walk, one thread: from the end site back along the predecessors (path[] has more than H rows; the guards cannot trigger)
__global__ void k_pt_walk(int N, int R, const PtStat *stat, const int *__restrict__ pred, int *path)
{
    const int H = stat->H;
    if (H == PT_NONE || H >= R) return;
    int s = stat->end;
    for (int k = H; k >= 0; --k) {
        if (s < 0 || s >= N) return;
        path[k] = s;
        s = pred[s];
    }
}

}   // namespace

extern "C" {

void dkmc_debug_set_path_round_cap(int cap) { g_pt_round_cap = clamp_round_cap(cap, PT_CAP_MAX); }

int dkmc_debug_get_path_times(double *ms2)
{
    NEED_FINISHED(g_pt.valid, "dkmc_debug_get_path_times", "dkmc_find_paths");
    if (ms2) memcpy(ms2, g_pt.ms, sizeof(g_pt.ms));
    return 0;
}

int dkmc_find_paths(int N, int nn, const int *d_index, const int *d_label, const double *d_site_x, int n_left_sites, int n_right_sites, int slack,
                    int *d_hops_left, int *d_hops_right)
{
    g_pt.valid = 0;
    if (N < 0 || nn < 1 || slack < 0 || slack > PT_SLACK_MAX || (N > 0 && (!d_index || !d_label || !d_hops_left || !d_hops_right)))
        return dkmc_fail(3, "dkmc_find_paths: bad arguments (N >= 0, nn >= 1, 0 <= slack <= 65536, device arrays of N sites)", __FILE__, __LINE__);
    clamp_seeds(N, n_left_sites, n_right_sites);
    g_pt.reset();
    if (N == 0) { g_pt.valid = 1; return 0; }
    hipStream_t st = eng().stream;
    const int cap = g_pt_round_cap;
    const size_t n = (size_t)N;
    int2 *hop = (int2 *)scratch(S_PT_HOP, n * sizeof(int2));
    int *pred = (int *)scratch(S_PT_PRED, n * sizeof(int));
    int *ctrl = (int *)scratch(S_PT_CTRL, (size_t)PT_CAP_MAX * sizeof(int) + sizeof(PtStat));
    if (!hop || !pred || !ctrl) return eng().err_code;
    PtStat *d_stat = (PtStat *)(ctrl + PT_CAP_MAX);

    const int site_blocks = (N + PT_NT - 1) / PT_NT;
    HIPCHK(g_pt.timer.start(eng().profiling != 0, st));
    HIPCHK(hipMemsetAsync(ctrl, 0, (size_t)PT_CAP_MAX * sizeof(int) + sizeof(PtStat), st));
    hipLaunchKernelGGL(k_pt_init, dim3(site_blocks), dim3(PT_NT), 0, st, N, d_label, n_left_sites, n_right_sites, hop, pred);
    KCHK();
    const int lpr = lpr_of(nn);
    const int row_blocks = grid_blocks((long long)N * lpr, PT_NT, 8192);
    int rounds = 0;
    if (int rc = run_rounds(st, ctrl, cap, ROUND_BATCH, &rounds,
                            [&](int r) { LAUNCH_LPR(lpr, k_pt_round, dim3(row_blocks), dim3(PT_NT), st, N, nn, d_index, hop, ctrl, r); })) return rc;
    if (!rounds) {
        char msg[200];
        snprintf(msg, sizeof(msg), "dkmc_find_paths: labelling not finished after %d rounds (the cap: dkmc_debug_set_path_round_cap); hops set to -1", cap);
        return abandon(st, n, {d_hops_left, d_hops_right}, msg, __FILE__, __LINE__);
    }
    HIPCHK(g_pt.timer.mark(1, st));
    // summaries.  H <= rounds - 1, so R = rounds + slack rows hold every level of the profile
    const int R = rounds + slack;
    const size_t nr = (size_t)R;
    char *rows = (char *)scratch(S_PT_ROWS, nr * (2 * sizeof(unsigned long long) + 2 * sizeof(int)));
    if (!rows) return eng().err_code;
    unsigned long long *kmin = (unsigned long long *)rows, *kmax = kmin + nr;
    int *cnt = (int *)(kmax + nr), *path = cnt + nr;
    PtStat h_stat;
    hipLaunchKernelGGL(k_pt_rows_init, dim3((R + PT_NT - 1) / PT_NT), dim3(PT_NT), 0, st, R, cnt, kmin, kmax, path, d_stat);
    hipLaunchKernelGGL(k_pt_finish, dim3(site_blocks), dim3(PT_NT), 0, st, N, (const int2 *)hop, n_right_sites, d_hops_left, d_hops_right, d_stat);
    if (R <= PT_LDS_ROWS)
        hipLaunchKernelGGL(k_pt_profile<1>, dim3(grid_blocks(N, PT_NT * 4, 1024)), dim3(PT_NT), 0, st, N, (const int *)d_hops_left, (const int *)d_hops_right,
                           d_site_x, slack, n_right_sites, R, d_stat, cnt, kmin, kmax);
    else
        hipLaunchKernelGGL(k_pt_profile<0>, dim3(grid_blocks(N, PT_NT, 8192)), dim3(PT_NT), 0, st, N, (const int *)d_hops_left, (const int *)d_hops_right,
                           d_site_x, slack, n_right_sites, R, d_stat, cnt, kmin, kmax);
    LAUNCH_LPR(lpr, k_pt_pred, dim3(row_blocks), dim3(PT_NT), st, N, nn, d_index, (const int *)d_hops_left, (const int *)d_hops_right, (const PtStat *)d_stat,
               pred);
    hipLaunchKernelGGL(k_pt_walk, dim3(1), dim3(1), 0, st, N, R, (const PtStat *)d_stat, (const int *)pred, path);
    KCHK();
    HIPCHK(g_pt.timer.mark(2, st));
    HIPCHK(hipMemcpyAsync(&h_stat, d_stat, sizeof(PtStat), hipMemcpyDeviceToHost, st));
    HIPCHK(hipStreamSynchronize(st));
    g_pt.info[2] = rounds; g_pt.info[3] = h_stat.reached_left; g_pt.info[4] = h_stat.reached_right;
    if (h_stat.H != PT_NONE) {
        const int H = h_stat.H;
        if (H < 0 || H >= rounds) return dkmc_fail(4, "dkmc_find_paths: H outside the rounds run", __FILE__, __LINE__);
        const size_t np = (size_t)H + slack + 1;
        std::vector<unsigned long long> h_min(np), h_max(np);
        if (int rc = fetch_columns(st, g_pt.profile, np, {cnt})) return rc;
        HIPCHK(hipMemcpyAsync(h_min.data(), kmin, np * sizeof(unsigned long long), hipMemcpyDeviceToHost, st));
        HIPCHK(hipMemcpyAsync(h_max.data(), kmax, np * sizeof(unsigned long long), hipMemcpyDeviceToHost, st));
        if (int rc = fetch_columns(st, g_pt.path, (size_t)H + 1, {path})) return rc;
        HIPCHK(hipStreamSynchronize(st));
        const std::vector<int> &count = g_pt.profile.i[0];
        long long corridor = 0;
        int level = 0;
        for (size_t k = 0; k < np; ++k) {
            key_range(d_site_x && count[k] > 0, h_min[k], h_max[k], &g_pt.profile.d[0][k], &g_pt.profile.d[1][k]);     // an empty row: +inf, -inf
            corridor += count[k];
            if (k <= (size_t)H && count[k] < count[level]) level = (int)k;
        }
        for (int s : g_pt.path.i[0])
            if (s < 0 || s >= N) return dkmc_fail(4, "dkmc_find_paths: the path walk left the members", __FILE__, __LINE__);
        g_pt.info[0] = 1; g_pt.info[1] = H; g_pt.info[5] = corridor; g_pt.info[6] = level; g_pt.info[7] = count[level];
    }
    float ms[2] = {0.f, 0.f};
    HIPCHK(g_pt.timer.read(ms));
    g_pt.ms[0] = ms[0]; g_pt.ms[1] = ms[1];
    g_pt.valid = 1;
    return 0;
}

int dkmc_get_path_info(long long *info8)
{
    NEED_FINISHED(g_pt.valid, "dkmc_get_path_info", "dkmc_find_paths");
    if (info8) memcpy(info8, g_pt.info, sizeof(g_pt.info));
    return 0;
}

int dkmc_copy_path_sites(int capacity, int *h_site, int *rows_out)
{
    NEED_FINISHED(g_pt.valid, "dkmc_copy_path_sites", "dkmc_find_paths");
    g_pt.path.copy_out(capacity, rows_out, {h_site});
    return 0;
}

int dkmc_copy_path_profile(int capacity, int *h_count, double *h_xmin, double *h_xmax, int *rows_out)
{
    NEED_FINISHED(g_pt.valid, "dkmc_copy_path_profile", "dkmc_find_paths");
    g_pt.profile.copy_out(capacity, rows_out, {h_count}, {h_xmin, h_xmax});
    return 0;
}

}   // extern "C"
