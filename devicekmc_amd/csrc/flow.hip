// flow.hip -- min-cut analysis of the bridged filament: the largest family of conducting paths that share no interior site (W), the minimum
// separators nearest either contact with their shores, and one canonical maximum family of strands (dkmc_find_flow; definitions and the search
// rule: include/devicekmc_hip.h).  No counterpart in the reference.  A pure function of its arguments: nothing of GPUBuffers, no engine state a
// later phase reads and no other kernel is touched.
//
// State: flow[] holds one pair of words per site, {pred, succ}: the neighbours of an interior site on its strand (FL_NONE: on no strand; FL_TERM:
//   the contact itself, so pred == FL_TERM marks a first site and succ == FL_TERM a last one), FL_OUT in both for a site that is not interior.
//   Between two searches pred and succ are FL_NONE together.  lvl[] holds the pair {level_in, level_out} of a search: -2 not interior, -1 unlabelled.
// A search: level-synchronous breadth-first labelling of the split nodes, the kernel boundary is the only synchronisation point.  Round 0 gives
//   level 1 to the in-nodes of the near-left sites (the arcs of S).  Round k >= 1 looks at every index entry (u, v) between two interior sites --
//   one entry serves both directions and both kinds of arc, the flow words of u alone decide which exist (succ[v] == u is pred[u] == v) -- and at
//   the two site-local arcs of u, and turns a word that holds -1 into k + 1 where the tail of an arc into it holds k.  A word is written in round
//   k only if it held -1 when the round began and has such an arc -- a property of the state BEFORE the round --, and every writer writes k + 1:
//   the argument of paths.hip.  No atomic read-modify-write, and the state after the launch is a function of the state before it.  The lane that
//   labels the out-node of a near-right site that is no last site adds bit 1 to the round's change word: the round after it returns at once, its
//   word stays 0 and run_rounds (rounds.h) ends the search.  "rounds" of a search counts that round, or the round that labelled nothing.
// After a successful search: the smallest exit by atomicMin; the smallest predecessor of every labelled in-node by one atomicMin pass over the
//   links (an out-node has one candidate: its own in-node off a strand, its successor's on one); one thread walks back and flips the path.
// The mirrored closing search is the same round kernel on the second level array with pred / succ and the two near arrays swapped.
// Tables: zones, counts and x keys by one per-site pass with integer atomics; the strands are numbered by a scan over the first-site flags, each
//   is followed by one thread, and a scan over the lengths places their sites.  The same bytes on every call.
#include "rounds.h"
#include <vector>

#define FL_NT 256
#define FL_CAP_MAX ROUND_CAP_MAX
#define FL_STRANDS_MAX 4096
#define FL_NONE (-1)
#define FL_TERM (-2)
#define FL_OUT (-3)
#define FL_FAR 0x7fffffff
#define FL_COLS 10

namespace {

struct FlStat {
    unsigned long long kmin_l, kmax_l, kmin_r, kmax_r;
    int touch, end, interior, near_l, near_r, shore_l, shore_r, shared, n_strands, n_sites, err, pad;
};
struct FlowState {
    int valid = 0;
    long long info[16];
    double x4[4];
    ResultTable<FL_COLS> strands;    // the columns of dkmc_copy_flow_strands, in its order
    ResultTable<1> sites;
    double ms[3];
    PhaseTimer<3> timer;
    void reset()
    {
        memset(info, 0, sizeof(info));
        x4[0] = x4[2] = INFINITY; x4[1] = x4[3] = -INFINITY;
        strands.clear(); sites.clear();
        ms[0] = ms[1] = ms[2] = 0.0;
    }
} g_fl;
int g_fl_round_cap = FL_CAP_MAX;

// 1a. interior sites and the identities of the near words; a member that is a seed of both sides makes the contacts touch
__global__ __launch_bounds__(FL_NT) void k_fl_init(int N, const int *__restrict__ label, int n_left, int n_right, int2 *flow, int *near_l, int *near_r,
                                                   FlStat *stat)
{
    const int i = blockIdx.x * FL_NT + threadIdx.x;
    if (i == 0) { stat->kmin_l = stat->kmin_r = ~0ull; stat->kmax_l = stat->kmax_r = 0ull; }
    if (i >= N) return;
    const int r = label[i];
    const bool m = r >= 0 && r < N;
    const int f = seed_bits(i, N, n_left, n_right);
    flow[i] = (m && f == 0) ? make_int2(FL_NONE, FL_NONE) : make_int2(FL_OUT, FL_OUT);
    near_l[i] = near_r[i] = FL_FAR;
    if (m && f == 3) atomicOr(&stat->touch, 1);
}

// 1b. the smallest seed of either side linked to every interior site, LPR lanes per member row; a link between seeds of different sides
template <int LPR>
__global__ __launch_bounds__(FL_NT) void k_fl_near(int N, int nn, const int *__restrict__ idx, const int *__restrict__ label, int n_left, int n_right,
                                                   int *near_l, int *near_r, FlStat *stat)
{
    const int lane = threadIdx.x % LPR;
    const long long groups = (long long)gridDim.x * (FL_NT / LPR);
    for (long long u = (long long)blockIdx.x * (FL_NT / LPR) + threadIdx.x / LPR; u < N; u += groups) {
        const int ru = label[u];
        if (ru < 0 || ru >= N) continue;
        const int fu = seed_bits((int)u, N, n_left, n_right);
        const int *row = idx + (size_t)u * nn;
        for (int e = lane; e < nn; e += LPR) {
            const int v = row[e];
            if (v < 0 || v >= N) continue;                    // padding, anywhere in the row
            const int rv = label[v];
            if (rv < 0 || rv >= N) continue;
            const int fv = seed_bits(v, N, n_left, n_right);
            if (fu == 0) {
                if (fv & 1) atomicMin(&near_l[u], v);
                if (fv & 2) atomicMin(&near_r[u], v);
            } else if (fv == 0) {
                if (fu & 1) atomicMin(&near_l[v], (int)u);
                if (fu & 2) atomicMin(&near_r[v], (int)u);
            } else if ((fu | fv) == 3) atomicOr(&stat->touch, 1);
        }
    }
}

// 2a. a search begins: every interior node unlabelled, the predecessor words and the end site at their identity
__global__ __launch_bounds__(FL_NT) void k_fl_begin(int N, const int2 *__restrict__ flow, int2 *lvl, int *pin, FlStat *stat)
{
    const int i = blockIdx.x * FL_NT + threadIdx.x;
    if (i == 0) stat->end = FL_FAR;
    if (i >= N) return;
    lvl[i] = flow[i].x == FL_OUT ? make_int2(-2, -2) : make_int2(-1, -1);
    pin[i] = FL_FAR;
}

// 2b. round k.  near_s / near_t: the near words of the side the search starts from / ends at; mirror: pred and succ change places (and lvl[].x
// then holds the levels of the physical out-nodes)
template <int LPR>
__global__ __launch_bounds__(FL_NT) void k_fl_round(int N, int nn, const int *__restrict__ idx, const int2 *__restrict__ flow,
                                                    const int *__restrict__ near_s, const int *__restrict__ near_t, int mirror, int2 *lvl, int *ctrl,
                                                    int k)
{
    if (k > 0 && (ctrl[k - 1] == 0 || (ctrl[k - 1] & 2))) return;     // the round before labelled nothing, or an exit: the search is over
    const int lane = threadIdx.x % LPR;
    const long long groups = (long long)gridDim.x * (FL_NT / LPR);
    int changed = 0;
    for (long long u = (long long)blockIdx.x * (FL_NT / LPR) + threadIdx.x / LPR; u < N; u += groups) {
        const int2 lu = ld_pair(&lvl[u]);
        if (lu.x == -2) continue;                             // not interior
        if (k == 0) {                                         // the arcs of S
            if (lane == 0 && near_s[u] != FL_FAR) { st_agent(&lvl[u].x, 1); changed = 1; }
            continue;
        }
        if (lu.x != k && lu.x != -1 && lu.y != k && lu.y != -1) continue;         // both settled: nothing to give, nothing to take
        int2 f = flow[u];
        if (mirror) f = make_int2(f.y, f.x);
        const int exit_u = (near_t[u] != FL_FAR && f.y != FL_TERM) ? 3 : 1;
        if (lane == 0) {                                      // the site-local arcs: in -> out off a strand, out -> in on one
            if (f.y == FL_NONE && lu.x == k && lu.y == -1) { st_agent(&lvl[u].y, k + 1); changed |= exit_u; }
            if (f.y != FL_NONE && lu.y == k && lu.x == -1) { st_agent(&lvl[u].x, k + 1); changed |= 1; }
        }
        const int *row = idx + (size_t)u * nn;
        for (int e = lane; e < nn; e += LPR) {
            const int v = row[e];
            if (v < 0 || v >= N || v == u) continue;          // padding, anywhere in the row
            const int2 lv = ld_pair(&lvl[v]);
            if (lv.x == -2) continue;
            if (lu.y == k && lv.x == -1 && f.y != v) { st_agent(&lvl[v].x, k + 1); changed |= 1; }           // u_out -> v_in unless succ[u] == v
            if (lv.y == k && lu.x == -1 && f.x != v) { st_agent(&lvl[u].x, k + 1); changed |= 1; }           // v_out -> u_in unless succ[v] == u
            if (f.y == v && lv.x == k && lu.y == -1) { st_agent(&lvl[u].y, k + 1); changed |= exit_u; }      // v_in -> u_out if succ[u] == v
            if (f.x == v && lu.x == k && lv.y == -1) {                                                       // u_in -> v_out if succ[v] == u
                st_agent(&lvl[v].y, k + 1);
                const int2 fv = flow[v];
                changed |= (near_t[v] != FL_FAR && (mirror ? fv.x : fv.y) != FL_TERM) ? 3 : 1;
            }
        }
    }
    if (changed) atomicOr(&ctrl[k], changed);
}

// 3a. the end node: the smallest exit on level E
__global__ __launch_bounds__(FL_NT) void k_fl_end(int N, const int2 *__restrict__ lvl, const int2 *__restrict__ flow, const int *__restrict__ near_r, int E,
                                                  FlStat *stat)
{
    const int i = blockIdx.x * FL_NT + threadIdx.x;
    const bool is = i < N && lvl[i].y == E && near_r[i] != FL_FAR && flow[i].y != FL_TERM;
    const int m = wave_min(is ? i : FL_FAR);
    if ((threadIdx.x & (WAVE - 1)) == 0 && m != FL_FAR) atomicMin(&stat->end, m);
}

// 3b. predecessors of the in-nodes: the out-nodes one level lower with an arc into them, the smallest site wins
template <int LPR>
__global__ __launch_bounds__(FL_NT) void k_fl_pin(int N, int nn, const int *__restrict__ idx, const int2 *__restrict__ flow, const int2 *__restrict__ lvl,
                                                  int *pin)
{
    const int lane = threadIdx.x % LPR;
    const long long groups = (long long)gridDim.x * (FL_NT / LPR);
    for (long long u = (long long)blockIdx.x * (FL_NT / LPR) + threadIdx.x / LPR; u < N; u += groups) {
        const int2 lu = lvl[u];
        if (lu.x < 0 && lu.y < 0) continue;                   // not interior, or not reached
        const int2 f = flow[u];
        if (lane == 0 && f.y != FL_NONE && lu.y >= 0 && lu.x == lu.y + 1) atomicMin(&pin[u], (int)u);
        const int *row = idx + (size_t)u * nn;
        for (int e = lane; e < nn; e += LPR) {
            const int v = row[e];
            if (v < 0 || v >= N || v == u) continue;
            const int2 lv = lvl[v];
            if (lv.x == -2) continue;
            if (lu.y >= 0 && lv.x == lu.y + 1 && f.y != v) atomicMin(&pin[v], (int)u);
            if (lv.y >= 0 && lu.x == lv.y + 1 && f.x != v) atomicMin(&pin[u], v);
        }
    }
}

// 3c. the walk, one thread: back from the end node, at every node its predecessor is read before the arc that leaves the node is flipped.  Forward
// link arcs become flow, backward ones cancel it (only where the words still name each other: an arc flipped earlier may have set them anew).
__global__ void k_fl_walk(int N, int2 *flow, const int2 *__restrict__ lvl, const int *__restrict__ pin, int E, FlStat *stat)
{
    int cur = stat->end, nxt = -1, out = 1;
    if (cur < 0 || cur >= N) { stat->err = 1; return; }
    for (int lev = E; lev >= 1; --lev) {
        int y;
        if (out) {
            const int s = flow[cur].y;
            y = s == FL_NONE ? cur : s;
            if (y < 0 || y >= N || lvl[y].x != lev - 1) { stat->err = 2; return; }
            if (nxt < 0) flow[cur].y = FL_TERM;
            else if (nxt != cur) { flow[cur].y = nxt; flow[nxt].x = cur; }
        } else {
            if (nxt != cur) {
                if (flow[nxt].y == cur) flow[nxt].y = FL_NONE;
                if (flow[cur].x == nxt) flow[cur].x = FL_NONE;
            }
            if (lev == 1) { flow[cur].x = FL_TERM; return; }
            y = pin[cur];
            if (y < 0 || y >= N || lvl[y].y != lev - 1) { stat->err = 3; return; }
        }
        nxt = cur; cur = y; out = !out;
    }
    stat->err = 4;                                            // level 1 is an in-node: not reached
}

// 4a. zones, counts, x keys of both cuts, the first-site flags.  full = 0 (status 2, 3): the member bit only
__global__ __launch_bounds__(FL_NT) void k_fl_zone(int N, const int *__restrict__ label, int n_left, int n_right, const int2 *__restrict__ flow,
                                                   const int2 *__restrict__ lvl, const int2 *__restrict__ mlvl, const int *__restrict__ near_l,
                                                   const int *__restrict__ near_r, const double *__restrict__ x, int full, int *zone, int *strand,
                                                   int *isfirst, FlStat *stat)
{
    const int i = blockIdx.x * FL_NT + threadIdx.x;
    bool inter = false, nl = false, nr = false, sl = false, sr = false, cl = false, cr = false;
    if (i < N) {
        const int r = label[i];
        const bool m = r >= 0 && r < N;
        const int2 f = flow[i];
        inter = f.x != FL_OUT;
        nl = inter && near_l[i] != FL_FAR; nr = inter && near_r[i] != FL_FAR;
        if (full) {
            const int s = seed_bits(i, N, n_left, n_right);
            const int2 a = lvl[i], b = mlvl[i];
            sl = (m && (s & 1)) || (inter && a.y >= 0); cl = inter && a.x >= 0 && a.y < 0;
            sr = (m && (s & 2)) || (inter && b.y >= 0); cr = inter && b.x >= 0 && b.y < 0;
        }
        zone[i] = (m ? DKMC_FLOW_MEMBER : 0) | (sl ? DKMC_FLOW_LEFT_SHORE : 0) | (cl ? DKMC_FLOW_LEFT_CUT : 0) | (cr ? DKMC_FLOW_RIGHT_CUT : 0) |
                  (sr ? DKMC_FLOW_RIGHT_SHORE : 0);
        strand[i] = -1;
        isfirst[i] = (inter && f.x == FL_TERM) ? 1 : 0;
    }
    const int c_in = __popcll(__ballot(inter)), c_nl = __popcll(__ballot(nl)), c_nr = __popcll(__ballot(nr)), c_sl = __popcll(__ballot(sl)),
              c_sr = __popcll(__ballot(sr)), c_sh = __popcll(__ballot(cl && cr));
    const bool any_l = __any(cl), any_r = __any(cr);
    unsigned long long lo_l = ~0ull, hi_l = 0ull, lo_r = ~0ull, hi_r = 0ull;
    if (x && (any_l || any_r)) {                              // the same in every lane of the wave
        const unsigned long long key = (cl || cr) ? dbl_key(x[i]) : 0ull;
        lo_l = wave_min(cl ? key : ~0ull); hi_l = wave_max(cl ? key : 0ull);
        lo_r = wave_min(cr ? key : ~0ull); hi_r = wave_max(cr ? key : 0ull);
    }
    if ((threadIdx.x & (WAVE - 1)) == 0) {
        if (c_in) atomicAdd(&stat->interior, c_in);
        if (c_nl) atomicAdd(&stat->near_l, c_nl);
        if (c_nr) atomicAdd(&stat->near_r, c_nr);
        if (c_sl) atomicAdd(&stat->shore_l, c_sl);
        if (c_sr) atomicAdd(&stat->shore_r, c_sr);
        if (c_sh) atomicAdd(&stat->shared, c_sh);
        if (x && any_l) { atomicMin(&stat->kmin_l, lo_l); atomicMax(&stat->kmax_l, hi_l); }
        if (x && any_r) { atomicMin(&stat->kmin_r, lo_r); atomicMax(&stat->kmax_r, hi_r); }
    }
}

// 4b. the rows of the first sites, ascending (rank = exclusive scan of the flags)
__global__ __launch_bounds__(FL_NT) void k_fl_heads(int N, const int *__restrict__ isfirst, const int *__restrict__ rank, const int *__restrict__ near_l,
                                                    int rows, int *t_first, int *t_lseed)
{
    const int i = blockIdx.x * FL_NT + threadIdx.x;
    if (i >= N || !isfirst[i]) return;
    const int j = rank[i];
    if (j < 0 || j >= rows) return;
    t_first[j] = i; t_lseed[j] = near_l[i];
}

// 4c. one thread per strand, from the first site along succ: the strand's row in site_strand, its length, last site and the two cut columns
// (cuts = 0: they stay -1).  t = the FL_COLS columns of `rows` words in the order of the strand table.
__global__ __launch_bounds__(FL_NT) void k_fl_strand(int N, int rows, const int2 *__restrict__ flow, const int *__restrict__ zone,
                                                     const int *__restrict__ near_r, int cuts, int *t, int *strand, FlStat *stat)
{
    const int j = blockIdx.x * FL_NT + threadIdx.x;
    if (j >= rows) return;
    int v = t[j], n = 0, cls = -1, clp = -1, crs = -1, crp = -1;
    for (;;) {
        if (v < 0 || v >= N || n >= N) { stat->err = 5; return; }
        strand[v] = j;
        const int z = cuts ? zone[v] : 0;
        if (z & DKMC_FLOW_LEFT_CUT) { cls = v; clp = n; }
        if (z & DKMC_FLOW_RIGHT_CUT) { crs = v; crp = n; }
        ++n;
        const int s = flow[v].y;
        if (s == FL_TERM) break;
        v = s;
    }
    t[rows + j] = v; t[2 * rows + j] = n; t[5 * rows + j] = near_r[v];
    t[6 * rows + j] = cls; t[7 * rows + j] = clp; t[8 * rows + j] = crs; t[9 * rows + j] = crp;
}

// 4d. the strands' sites at their offsets (exclusive scan of the lengths)
__global__ __launch_bounds__(FL_NT) void k_fl_sites(int N, int rows, const int2 *__restrict__ flow, const int *__restrict__ t, int *sites, FlStat *stat)
{
    const int j = blockIdx.x * FL_NT + threadIdx.x;
    if (j >= rows) return;
    int v = t[j];
    const int len = t[2 * rows + j], off = t[3 * rows + j];
    for (int n = 0; n < len; ++n) {
        if (v < 0 || v >= N || off < 0 || off + n >= N) { stat->err = 6; return; }
        sites[off + n] = v;
        v = flow[v].y;
    }
}

}   // namespace

extern "C" {

void dkmc_debug_set_flow_round_cap(int cap) { g_fl_round_cap = clamp_round_cap(cap, FL_CAP_MAX); }

int dkmc_debug_get_flow_times(double *ms3)
{
    NEED_FINISHED(g_fl.valid, "dkmc_debug_get_flow_times", "dkmc_find_flow");
    if (ms3) memcpy(ms3, g_fl.ms, sizeof(g_fl.ms));
    return 0;
}

int dkmc_find_flow(int N, int nn, const int *d_index, const int *d_label, const double *d_site_x, int n_left_sites, int n_right_sites, int max_strands,
                   int *d_site_zone, int *d_site_strand)
{
    g_fl.valid = 0;
    if (N < 0 || nn < 1 || max_strands < 1 || max_strands > FL_STRANDS_MAX || (N > 0 && (!d_index || !d_label || !d_site_zone || !d_site_strand)))
        return dkmc_fail(3, "dkmc_find_flow: bad arguments (N >= 0, nn >= 1, 1 <= max_strands <= 4096, device arrays of N sites)", __FILE__, __LINE__);
    clamp_seeds(N, n_left_sites, n_right_sites);
    g_fl.reset();
    if (N == 0) { g_fl.valid = 1; return 0; }
    hipStream_t st = eng().stream;
    const int cap = g_fl_round_cap;
    const size_t n = (size_t)N;
    int *site = (int *)scratch(S_FL_SITE, 12 * n * sizeof(int));
    int *tab = (int *)scratch(S_FL_ROWS, (size_t)FL_COLS * FL_STRANDS_MAX * sizeof(int));
    int *ctrl = (int *)scratch(S_FL_CTRL, (size_t)FL_CAP_MAX * sizeof(int) + sizeof(FlStat));
    if (!site || !tab || !ctrl) return eng().err_code;
    int2 *flow = (int2 *)site, *lvl = flow + n, *mlvl = lvl + n;
    int *near_l = (int *)(mlvl + n), *near_r = near_l + n, *pin = near_r + n, *isfirst = pin + n, *rank = isfirst + n, *ssites = rank + n;
    FlStat *d_stat = (FlStat *)(ctrl + FL_CAP_MAX);
    FlStat h_stat;

    const int site_blocks = (N + FL_NT - 1) / FL_NT;
    const int lpr = lpr_of(nn);
    const int row_blocks = grid_blocks((long long)N * lpr, FL_NT, 8192);
    HIPCHK(g_fl.timer.start(eng().profiling != 0, st));
    HIPCHK(hipMemsetAsync(d_stat, 0, sizeof(FlStat), st));
    hipLaunchKernelGGL(k_fl_init, dim3(site_blocks), dim3(FL_NT), 0, st, N, d_label, n_left_sites, n_right_sites, flow, near_l, near_r, d_stat);
    LAUNCH_LPR(lpr, k_fl_near, dim3(row_blocks), dim3(FL_NT), st, N, nn, d_index, d_label, n_left_sites, n_right_sites, near_l, near_r, d_stat);
    KCHK();
    HIPCHK(hipMemcpyAsync(&h_stat, d_stat, sizeof(FlStat), hipMemcpyDeviceToHost, st));
    HIPCHK(hipStreamSynchronize(st));
    int status = h_stat.touch ? 2 : -1, W = 0, searches = 0;
    long long rounds_all = 0;
    // one search on lv from the side of near_s; *found = it ended on an exit of level *E
    auto search = [&](int2 *lv, const int *near_s, const int *near_t, int mirror, int *found, int *E) -> int {
        int rounds = 0;
        HIPCHK(hipMemsetAsync(ctrl, 0, (size_t)FL_CAP_MAX * sizeof(int), st));
        hipLaunchKernelGGL(k_fl_begin, dim3(site_blocks), dim3(FL_NT), 0, st, N, (const int2 *)flow, lv, pin, d_stat);
        if (int rc = run_rounds(st, ctrl, cap, ROUND_BATCH, &rounds, [&](int r) {
                LAUNCH_LPR(lpr, k_fl_round, dim3(row_blocks), dim3(FL_NT), st, N, nn, d_index, (const int2 *)flow, near_s, near_t, mirror, lv, ctrl, r);
            })) return rc;
        if (!rounds) {
            char msg[240];
            snprintf(msg, sizeof(msg), "dkmc_find_flow: search %d not finished after %d rounds (the cap: dkmc_debug_set_flow_round_cap); "
                     "site_zone and site_strand set to -1", searches + 1, cap);
            return abandon(st, n, {d_site_zone, d_site_strand}, msg, __FILE__, __LINE__);
        }
        ++searches;
        rounds_all += rounds;
        *found = rounds >= 2 && (round_words()[rounds - 2] & 2) ? 1 : 0;
        *E = rounds - 1;
        return 0;
    };
    while (status < 0) {
        int found = 0, E = 0;
        HIPCHK(g_fl.timer.mark(1, st));                       // recorded anew before every search: what stays is the start of the closing one
        if (int rc = search(lvl, near_l, near_r, 0, &found, &E)) return rc;
        if (!found) { status = W ? 1 : 0; break; }
        hipLaunchKernelGGL(k_fl_end, dim3(site_blocks), dim3(FL_NT), 0, st, N, (const int2 *)lvl, (const int2 *)flow, (const int *)near_r, E, d_stat);
        LAUNCH_LPR(lpr, k_fl_pin, dim3(row_blocks), dim3(FL_NT), st, N, nn, d_index, (const int2 *)flow, (const int2 *)lvl, pin);
        hipLaunchKernelGGL(k_fl_walk, dim3(1), dim3(1), 0, st, N, flow, (const int2 *)lvl, (const int *)pin, E, d_stat);
        KCHK();
        if (++W == max_strands) status = 3;
    }
    if (status >= 2) HIPCHK(g_fl.timer.mark(1, st));          // no closing searches
    if (status == 0 || status == 1) {
        int found = 0, E = 0;
        if (int rc = search(mlvl, near_r, near_l, 1, &found, &E)) return rc;
        if (found) return abandon(st, n, {d_site_zone, d_site_strand}, "dkmc_find_flow: the mirrored closing search found an exit", __FILE__, __LINE__);
    }
    HIPCHK(g_fl.timer.mark(2, st));
    // zones, counts, tables
    const int full = status == 0 || status == 1;
    hipLaunchKernelGGL(k_fl_zone, dim3(site_blocks), dim3(FL_NT), 0, st, N, d_label, n_left_sites, n_right_sites, (const int2 *)flow, (const int2 *)lvl,
                       (const int2 *)mlvl, (const int *)near_l, (const int *)near_r, d_site_x, full, d_site_zone, d_site_strand, isfirst, d_stat);
    KCHK();
    if (W > 0) {
        const int wb = (W + FL_NT - 1) / FL_NT;
        if (int rc = dkmc_exclusive_scan_i32(isfirst, rank, N, &d_stat->n_strands)) return rc;
        hipLaunchKernelGGL(k_fl_heads, dim3(site_blocks), dim3(FL_NT), 0, st, N, (const int *)isfirst, (const int *)rank, (const int *)near_l, W, tab,
                           tab + 4 * W);
        hipLaunchKernelGGL(k_fl_strand, dim3(wb), dim3(FL_NT), 0, st, N, W, (const int2 *)flow, (const int *)d_site_zone, (const int *)near_r, full, tab,
                           d_site_strand, d_stat);
        KCHK();
        if (int rc = dkmc_exclusive_scan_i32(tab + 2 * W, tab + 3 * W, W, &d_stat->n_sites)) return rc;
        hipLaunchKernelGGL(k_fl_sites, dim3(wb), dim3(FL_NT), 0, st, N, W, (const int2 *)flow, (const int *)tab, ssites, d_stat);
        KCHK();
    }
    HIPCHK(hipMemcpyAsync(&h_stat, d_stat, sizeof(FlStat), hipMemcpyDeviceToHost, st));
    HIPCHK(hipStreamSynchronize(st));
    if (h_stat.err || (W > 0 && (h_stat.n_strands != W || h_stat.n_sites < W || h_stat.n_sites > N))) {
        char msg[200];
        snprintf(msg, sizeof(msg), "dkmc_find_flow: the strands are not consistent (walk code %d, %d first sites for %d strands); "
                 "site_zone and site_strand set to -1", h_stat.err, h_stat.n_strands, W);
        return abandon(st, n, {d_site_zone, d_site_strand}, msg, __FILE__, __LINE__);
    }
    long long longest = 0, shortest = 0;
    if (W > 0) {
        const int *cols[FL_COLS];
        for (int c = 0; c < FL_COLS; ++c) cols[c] = tab + (size_t)c * W;
        if (int rc = fetch_columns(st, g_fl.strands, (size_t)W, cols)) return rc;
        if (int rc = fetch_columns(st, g_fl.sites, (size_t)h_stat.n_sites, {ssites})) return rc;
        HIPCHK(g_fl.timer.mark(3, st));
        HIPCHK(hipStreamSynchronize(st));
        const std::vector<int> &length = g_fl.strands.i[2];
        shortest = length[0];
        for (int len : length) { longest = len > longest ? len : longest; shortest = len < shortest ? len : shortest; }
    } else {
        HIPCHK(g_fl.timer.mark(3, st));
        HIPCHK(hipStreamSynchronize(st));
    }
    const long long info[12] = {status, status == 2 ? -1 : W, h_stat.shore_l, h_stat.shore_r, h_stat.shared, h_stat.interior, h_stat.near_l, h_stat.near_r,
                                searches, rounds_all, longest, shortest};
    memcpy(g_fl.info, info, sizeof(info));
    const bool has_x = d_site_x && full && W > 0;             // else the empty ranges of the reset
    key_range(has_x, h_stat.kmin_l, h_stat.kmax_l, &g_fl.x4[0], &g_fl.x4[1]);
    key_range(has_x, h_stat.kmin_r, h_stat.kmax_r, &g_fl.x4[2], &g_fl.x4[3]);
    float ms[3] = {0.f, 0.f, 0.f};
    HIPCHK(g_fl.timer.read(ms));
    for (int i = 0; i < 3; ++i) g_fl.ms[i] = ms[i];
    g_fl.valid = 1;
    return 0;
}

int dkmc_get_flow_info(long long *info16, double *x4)
{
    NEED_FINISHED(g_fl.valid, "dkmc_get_flow_info", "dkmc_find_flow");
    if (info16) memcpy(info16, g_fl.info, sizeof(g_fl.info));
    if (x4) memcpy(x4, g_fl.x4, sizeof(g_fl.x4));
    return 0;
}

int dkmc_copy_flow_strands(int capacity, int *h_first_site, int *h_last_site, int *h_length, int *h_offset, int *h_left_seed, int *h_right_seed,
                           int *h_cut_left_site, int *h_cut_left_pos, int *h_cut_right_site, int *h_cut_right_pos, int *rows_out)
{
    NEED_FINISHED(g_fl.valid, "dkmc_copy_flow_strands", "dkmc_find_flow");
    g_fl.strands.copy_out(capacity, rows_out, {h_first_site, h_last_site, h_length, h_offset, h_left_seed, h_right_seed, h_cut_left_site, h_cut_left_pos,
                                               h_cut_right_site, h_cut_right_pos});
    return 0;
}

int dkmc_copy_flow_strand_sites(int capacity, int *h_site, int *rows_out)
{
    NEED_FINISHED(g_fl.valid, "dkmc_copy_flow_strand_sites", "dkmc_find_flow");
    g_fl.sites.copy_out(capacity, rows_out, {h_site});
    return 0;
}

}   // extern "C"
