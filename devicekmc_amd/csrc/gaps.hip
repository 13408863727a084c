// gaps.hip -- gap analysis of the filament: the island graph (minimum spanning forest of the nodes over the member pairs within r_max), the
// tunnelling chain between the two contact nodes and the direct, Euclidean tip-to-tip gap (dkmc_find_gaps; definitions: include/devicekmc_hip.h).
// No counterpart in the reference.  A pure function of its arguments: nothing of GPUBuffers, no engine state a later phase reads and no other
// kernel is touched.
//
// Nodes: the left-touching components together are node N, the right-touching ones node N + 1 (N too when one component touches both), every
//   other component is the node of its label.  node_site[] holds the current node of every member, snode[] the same in cell order.
// Cell list over the members only (binning and walk: cellgrid.h), cells of edge >= r_max (a hair more, so that rounding in the binning cannot put a
//   pair within r_max two cells apart); the members' coordinates, sites and nodes are stored in cell order, so the lanes of a wave scan the same
//   neighbour cells.
// Boruvka rounds, the kernel boundary is the only synchronisation point:
//   search   every member scans its neighbour cells and keeps its best pair by the key (d2, a, b) among the members of another node, then
//            atomicMin(best_d2[node], key of d2);
//   pick     the members that attained best_d2[node] do atomicMin(best_pair[node], a << 32 | b).  Integer minima only: the pick of a node is a
//            function of the nodes alone, whatever the order of arrival;
//   edges    every node with a pick records it -- once where two nodes picked each other -- and points parent[node] at the node it picked (the
//            smaller of the two for a mutual pick).  Along such pointers the picked keys strictly decrease until a mutual pair, whose smaller
//            node is the root: no cycles, and every walk ends;
//   roots    every node with a pick walks parent[] (read-only in this launch) to its root; refresh moves the members to it.
//   A round in which no node had a candidate ends the loop; "rounds" counts it.  Every round at least halves the nodes that still have a
//   candidate, so 32 rounds suffice for any N.
// The picked edges of all rounds are the forest; their rows (labels and contact flags of both ends) are gathered on the device, the at most
// n_components - 1 rows are sorted by key and the L -> R tree path is walked on the host.
#include "cellgrid.h"
#include "rounds.h"
#include <algorithm>
#include <vector>

#define GP_NT CELL_NT
#define GP_BATCH 4                   // rounds enqueued per read-back of the control block
#define GP_ROUND_CAP 34
#define GP_MAX_CELLS (1 << 24)

namespace {

struct GpCtrl {
    int any[GP_ROUND_CAP + 2];       // per round: some node had a candidate
    int n_components, n_edges, flags, pad;   // flags: bit 0 a left-touching component exists, bit 1 a right-touching one, bit 2 one touches both
    unsigned long long pairs;        // distance tests made
    unsigned long long direct_key, direct_pair;
};
enum { E_A, E_B, E_RA, E_RB };      // the int columns of the edge table
struct GapState {
    int valid = 0;
    long long info[8];
    double d2x2[2];
    ResultTable<4, 1> edges;         // site_a, site_b, root_a, root_b; d2
    ResultTable<2, 1> chain;         // from, to; d2
    void reset()
    {
        const long long z[8] = {0, 0, 0, 0, 1, 0, -1, -1};
        memcpy(info, z, sizeof(z));
        d2x2[0] = d2x2[1] = INFINITY;
        edges.clear(); chain.clear();
    }
} g_gap;
int g_gap_cell_skip = 1;

const unsigned long long GP_NONE = ~0ull;

// the contract's arithmetic: every product and every sum rounded on its own (site a = the smaller index).  Contraction is switched off for the
// body itself: the headers' __dmul_rn / __dadd_rn are plain x * y and x + y, which fuse into v_fmac_f64 once they are inlined.
__device__ __forceinline__ double gp_d2(double xa, double ya, double za, double xb, double yb, double zb, double laty, double latz, int pbc)
{
#pragma clang fp contract(off)
    const double dx = xa - xb;
    double dy = ya - yb, dz = za - zb;
    if (pbc) {
        double fy = dy / laty; fy -= round(fy);
        double fz = dz / latz; fz -= round(fz);
        dy = fy * laty; dz = fz * latz;
    }
    const double xx = dx * dx, yy = dy * dy, zz = dz * dz;
    return (xx + yy) + zz;
}

__device__ __forceinline__ bool gp_member(int r, int N) { return r >= 0 && r < N; }

// 1. per component (indexed by its label): contact flags (bits 0, 1) and presence (bit 2); the components are counted as they appear
__global__ __launch_bounds__(GP_NT) void k_gp_flags(int N, const int *__restrict__ label, int n_left, int n_right, int *cflags, GpCtrl *ctrl)
{
    const int i = blockIdx.x * GP_NT + threadIdx.x;
    if (i >= N) return;
    const int r = label[i];
    if (!gp_member(r, N)) return;
    const int want = 4 | seed_bits(i, N, n_left, n_right);
    if ((ld_agent(&cflags[r]) & want) == want) return;        // an older value only costs the atomic
    const int old = atomicOr(&cflags[r], want);
    if (!(old & 4)) atomicAdd(&ctrl->n_components, 1);
}

// 2. census of the members: bounding box and count per workgroup (the host combines them), which kinds of contact node exist
__global__ __launch_bounds__(GP_NT) void k_gp_census(int N, const int *__restrict__ label, const int *__restrict__ cflags, const double *__restrict__ x,
                                                     const double *__restrict__ y, const double *__restrict__ z, double *box, int *cnt, GpCtrl *ctrl)
{
    __shared__ int s_cnt[GP_NT], s_fl[GP_NT];
    double mn[3] = {INFINITY, INFINITY, INFINITY}, mx[3] = {-INFINITY, -INFINITY, -INFINITY};
    int n = 0, fl = 0;
    for (long long i = (long long)blockIdx.x * GP_NT + threadIdx.x; i < N; i += (long long)gridDim.x * GP_NT) {
        const int r = label[i];
        if (!gp_member(r, N)) continue;
        const int f = cflags[r] & 3;
        fl |= f | (f == 3 ? 4 : 0);
        ++n;
        mn[0] = fmin(mn[0], x[i]); mx[0] = fmax(mx[0], x[i]);
        mn[1] = fmin(mn[1], y[i]); mx[1] = fmax(mx[1], y[i]);
        mn[2] = fmin(mn[2], z[i]); mx[2] = fmax(mx[2], z[i]);
    }
    block_box(mn, mx, box + blockIdx.x * 6);
    const int t = threadIdx.x;
    s_cnt[t] = n; s_fl[t] = fl;
    __syncthreads();
    for (int s = GP_NT / 2; s > 0; s >>= 1) {
        if (t < s) { s_cnt[t] += s_cnt[t + s]; s_fl[t] |= s_fl[t + s]; }
        __syncthreads();
    }
    if (t == 0) { cnt[blockIdx.x] = s_cnt[0]; if (s_fl[0]) atomicOr(&ctrl->flags, s_fl[0]); }
}

// 3. cell list of the members: k_cell_count (cellgrid.h) with the labels, then the members in cell order (the order inside a cell is the
// atomics': every result is a minimum over a cell, so it does not matter) and the initial node of every site
__global__ __launch_bounds__(GP_NT) void k_gp_scatter(int N, int M, const int *__restrict__ cell_id, const int *__restrict__ cell_start, int *cell_fill,
                                                      const int *__restrict__ label, const int *__restrict__ cflags, const GpCtrl *ctrl,
                                                      const double *__restrict__ x, const double *__restrict__ y, const double *__restrict__ z,
                                                      double *sx, double *sy, double *sz, int *ssite, int *snode, int *node_site)
{
    const int i = blockIdx.x * GP_NT + threadIdx.x;
    if (i >= N) return;
    const int c = cell_id[i];
    if (c < 0) { node_site[i] = -1; return; }
    const int r = label[i], f = cflags[r] & 3;
    const int node = f == 0 ? r : ((f & 1) || (ctrl->flags & 4) ? N : N + 1);
    node_site[i] = node;
    const int s = cell_start[c] + atomicAdd(&cell_fill[c], 1);
    if (s >= M) return;                                       // cannot happen: the counts add up to M
    sx[s] = x[i]; sy[s] = y[i]; sz[s] = z[i]; ssite[s] = i; snode[s] = node;
}

__global__ __launch_bounds__(GP_NT) void k_gp_node_init(int n, int *parent)
{
    const int i = blockIdx.x * GP_NT + threadIdx.x;
    if (i < n) parent[i] = i;
}

// per cell: the node all its members carry, -1 where they differ (or the cell is empty)
__global__ __launch_bounds__(GP_NT) void k_gp_cell_uniform(int ncell, const int *__restrict__ cell_start, const int *__restrict__ cell_cnt,
                                                           const int *__restrict__ snode, int *cell_node, const GpCtrl *ctrl, int round)
{
    if (round > 0 && ctrl->any[round - 1] == 0) return;
    const int c = blockIdx.x * GP_NT + threadIdx.x;
    if (c >= ncell) return;
    const int s0 = cell_start[c], n = cell_cnt[c];
    int u = -1;
    if (n > 0) {
        u = snode[s0];
        for (int s = s0 + 1; s < s0 + n; ++s) if (snode[s] != u) { u = -1; break; }
    }
    cell_node[c] = u;
}

// 4a. search.  DIRECT = 0: a round's search, every member against the members of the other nodes.  DIRECT = 1: the members of node L against
// those of node R only (the direct gap).  A periodic axis with fewer than 3 cells is scanned whole, so every distinct neighbour cell is visited once.
template <int DIRECT>
__global__ __launch_bounds__(GP_NT) void k_gp_search(int M, int N, CellGrid G, double r2max, const double *__restrict__ sx, const double *__restrict__ sy,
                                                     const double *__restrict__ sz, const int *__restrict__ ssite, const int *__restrict__ snode,
                                                     const int *__restrict__ cell_start, const int *__restrict__ cell_cnt,
                                                     const int *__restrict__ cell_node, int skip, unsigned long long *best_d2,
                                                     unsigned long long *mykey, unsigned long long *mypair, GpCtrl *ctrl, int round)
{
    if (!DIRECT && round > 0 && ctrl->any[round - 1] == 0) return;
    const int s = blockIdx.x * GP_NT + threadIdx.x;
    unsigned long long tests = 0;
    if (s < M) {
        const int mynode = snode[s];
        unsigned long long bk = GP_NONE, bp = GP_NONE;
        if (!DIRECT || mynode == N) {
            const int i = ssite[s];
            const double xi = sx[s], yi = sy[s], zi = sz[s];
            int cx, cy, cz; cell_of(G, xi, yi, zi, cx, cy, cz);
            for_each_neighbor_cell(G, cx, cy, cz, [&](int c) {
                if (skip) {
                    const int u = cell_node[c];
                    if (DIRECT ? (u >= 0 && u != N + 1) : (u == mynode)) return;
                }
                const int t0 = cell_start[c], t1 = t0 + cell_cnt[c];
                for (int t = t0; t < t1; ++t) {
                    const int other = snode[t];
                    if (DIRECT ? (other != N + 1) : (other == mynode)) continue;
                    const int j = ssite[t];
                    const double xj = sx[t], yj = sy[t], zj = sz[t];
                    const bool lo = i < j;
                    const double d2 = lo ? gp_d2(xi, yi, zi, xj, yj, zj, G.laty, G.latz, G.pbc) : gp_d2(xj, yj, zj, xi, yi, zi, G.laty, G.latz, G.pbc);
                    ++tests;
                    if (!(d2 <= r2max)) continue;
                    const unsigned long long k = dbl_key(d2);
                    const unsigned long long p = ((unsigned long long)(unsigned)(lo ? i : j) << 32) | (unsigned)(lo ? j : i);
                    if (k < bk || (k == bk && p < bp)) { bk = k; bp = p; }
                }
            });
            if (bk != GP_NONE && bk < __hip_atomic_load(&best_d2[mynode], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)) atomicMin(&best_d2[mynode], bk);
        }
        mykey[s] = bk; mypair[s] = bp;
    }
    // one counter update per wave
    unsigned long long w = tests;
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) w += __shfl_xor(w, off, WAVE);
    if ((threadIdx.x & (WAVE - 1)) == 0 && w) atomicAdd(&ctrl->pairs, w);
}

// 4b. pick: among the members that attained their node's best d2, the smallest (a, b)
__global__ __launch_bounds__(GP_NT) void k_gp_pick(int M, const int *__restrict__ snode, const unsigned long long *__restrict__ mykey,
                                                   const unsigned long long *__restrict__ mypair, const unsigned long long *__restrict__ best_d2,
                                                   unsigned long long *best_pair, const GpCtrl *ctrl, int round)
{
    if (round > 0 && ctrl->any[round - 1] == 0) return;
    const int s = blockIdx.x * GP_NT + threadIdx.x;
    if (s >= M) return;
    const unsigned long long k = mykey[s];
    if (k == GP_NONE) return;
    const int node = snode[s];
    if (best_d2[node] != k) return;
    const unsigned long long p = mypair[s];
    if (p < __hip_atomic_load(&best_pair[node], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)) atomicMin(&best_pair[node], p);
}

// the direct gap: node L's pick of the DIRECT search, moved to the control block; the two words are cleared for the rounds
__global__ void k_gp_save_direct(int N, unsigned long long *best_d2, unsigned long long *best_pair, GpCtrl *ctrl)
{
    ctrl->direct_key = best_d2[N]; ctrl->direct_pair = best_pair[N];
    best_d2[N] = GP_NONE; best_pair[N] = GP_NONE;
}

// 4c. edges: one thread per node id.  cur_*: this round's picks; nxt_*: the words of the next round, cleared here.
__global__ __launch_bounds__(GP_NT) void k_gp_edges(int nnode, const int *__restrict__ node_site, const unsigned long long *__restrict__ cur_d2,
                                                    const unsigned long long *__restrict__ cur_pair, unsigned long long *nxt_d2,
                                                    unsigned long long *nxt_pair, int *parent, unsigned long long *ekey, unsigned long long *epair,
                                                    int ecap, GpCtrl *ctrl, int round)
{
    if (round > 0 && ctrl->any[round - 1] == 0) return;
    const int n = blockIdx.x * GP_NT + threadIdx.x;
    if (n >= nnode) return;
    nxt_d2[n] = GP_NONE; nxt_pair[n] = GP_NONE;
    const unsigned long long k = cur_d2[n];
    if (k == GP_NONE) return;
    const unsigned long long p = cur_pair[n];
    const int a = (int)(p >> 32), b = (int)(p & 0xffffffffull);
    if (a < 0 || b < 0 || a >= nnode - 2 || b >= nnode - 2) return;      // cannot happen: a node with a best d2 has a best pair
    const int na = node_site[a], nb = node_site[b];
    const int m = na == n ? nb : na;                          // the node picked
    if (m < 0 || m >= nnode) return;                          // cannot happen: both ends are members
    const bool mutual = cur_d2[m] == k && cur_pair[m] == p;
    parent[n] = mutual ? min(n, m) : m;
    if (!mutual || n < m) {
        const int e = atomicAdd(&ctrl->n_edges, 1);
        if (e < ecap) { ekey[e] = k; epair[e] = p; }
    }
    if (ld_agent(&ctrl->any[round]) == 0) atomicOr(&ctrl->any[round], 1);
}

// 4d. roots: parent[] is read-only here; the walk is bounded by the number of nodes
__global__ __launch_bounds__(GP_NT) void k_gp_roots(int nnode, const unsigned long long *__restrict__ cur_d2, const int *__restrict__ parent, int *newroot,
                                                    const GpCtrl *ctrl, int round)
{
    if (ctrl->any[round] == 0) return;
    const int n = blockIdx.x * GP_NT + threadIdx.x;
    if (n >= nnode) return;
    int c = n;
    if (cur_d2[n] != GP_NONE)
        for (int it = 0; it < nnode; ++it) {
            const int p = parent[c];
            if (p == c || p < 0 || p >= nnode) break;
            c = p;
        }
    newroot[n] = c;
}

// 4e. refresh: every member moves to the root of its node (a root is its own parent already: the smaller node of a mutual pick)
__global__ __launch_bounds__(GP_NT) void k_gp_refresh(int M, const int *__restrict__ ssite, const int *__restrict__ newroot, int *node_site, int *snode,
                                                      const GpCtrl *ctrl, int round)
{
    if (ctrl->any[round] == 0) return;
    const int s = blockIdx.x * GP_NT + threadIdx.x;
    if (s >= M) return;
    const int r = newroot[snode[s]];
    snode[s] = r; node_site[ssite[s]] = r;
}

// 5. rows of the forest: label and contact flags of both ends
__global__ __launch_bounds__(GP_NT) void k_gp_edge_rows(int E, const unsigned long long *__restrict__ epair, const int *__restrict__ label,
                                                        const int *__restrict__ cflags, int *row4)
{
    const int e = blockIdx.x * GP_NT + threadIdx.x;
    if (e >= E) return;
    const unsigned long long p = epair[e];
    const int ra = label[(int)(p >> 32)], rb = label[(int)(p & 0xffffffffull)];
    row4[4 * e] = ra; row4[4 * e + 1] = rb; row4[4 * e + 2] = cflags[ra] & 3; row4[4 * e + 3] = cflags[rb] & 3;
}

// cells along an extent at edge h; -1 where they would be too many
int gp_cells(double ext, double h)
{
    const double q = floor(ext / h) + 1.0;
    return (q >= 1.0 && q <= (double)GP_MAX_CELLS) ? (int)q : (q < 1.0 ? 1 : -1);
}

// the L -> R path of the forest (rows sorted by key).  na, nb: the nodes of a row's ends, -1 = L, -2 = R, else the label.
void gap_chain(const std::vector<int> &na, const std::vector<int> &nb)
{
    const size_t E = na.size();
    std::vector<int> ids(na);
    ids.insert(ids.end(), nb.begin(), nb.end());
    std::sort(ids.begin(), ids.end());
    ids.erase(std::unique(ids.begin(), ids.end()), ids.end());
    auto at = [&](int v) { return (int)(std::lower_bound(ids.begin(), ids.end(), v) - ids.begin()); };
    const int V = (int)ids.size();
    if (!std::binary_search(ids.begin(), ids.end(), -1) || !std::binary_search(ids.begin(), ids.end(), -2)) return;
    std::vector<int> deg(V + 1, 0), adj(2 * E), via(V, -2), queue;
    for (size_t e = 0; e < E; ++e) { ++deg[at(na[e]) + 1]; ++deg[at(nb[e]) + 1]; }
    for (int v = 0; v < V; ++v) deg[v + 1] += deg[v];
    std::vector<int> fill(deg.begin(), deg.end() - 1);
    for (size_t e = 0; e < E; ++e) { adj[fill[at(na[e])]++] = (int)e; adj[fill[at(nb[e])]++] = (int)e; }
    const int L = at(-1), R = at(-2);
    via[L] = -1; queue.push_back(L);
    for (size_t q = 0; q < queue.size() && via[R] == -2; ++q) {
        const int v = queue[q];
        for (int k = deg[v]; k < deg[v + 1]; ++k) {
            const int e = adj[k], w = at(na[e]) == v ? at(nb[e]) : at(na[e]);
            if (via[w] == -2) { via[w] = e; queue.push_back(w); }
        }
    }
    if (via[R] == -2) return;
    std::vector<int> hop, a_first;                            // R back to L: the edge of a hop, and whether its end a is the one nearer to L
    for (int v = R; v != L;) {
        const int e = via[v];
        const bool a_near_l = at(nb[e]) == v;                  // the hop arrives at v: its other end is the one nearer to L
        hop.push_back(e); a_first.push_back(a_near_l);
        v = a_near_l ? at(na[e]) : at(nb[e]);
    }
    const ResultTable<4, 1> &T = g_gap.edges;
    const size_t hops = hop.size();
    g_gap.chain.resize(hops);
    double worst = 0.0;
    for (size_t k = 0; k < hops; ++k) {                       // the rows run from L to R
        const int e = hop[hops - 1 - k];
        g_gap.chain.i[0][k] = T.i[a_first[hops - 1 - k] ? E_A : E_B][e];
        g_gap.chain.i[1][k] = T.i[a_first[hops - 1 - k] ? E_B : E_A][e];
        g_gap.chain.d[0][k] = T.d[0][e];
        worst = fmax(worst, T.d[0][e]);
    }
    g_gap.info[2] = 1; g_gap.info[3] = (long long)hops; g_gap.d2x2[0] = worst;
}

}   // namespace

extern "C" {

void dkmc_debug_set_gap_cell_skip(int on) { g_gap_cell_skip = on ? 1 : 0; }

int dkmc_find_gaps(int N, const double *d_x, const double *d_y, const double *d_z, const double *h_lattice, int pbc,
                   const int *d_label, int n_left_sites, int n_right_sites, double r_max)
{
    g_gap.valid = 0;
    if (N < 0 || N > 0x7ffffff0 || (N > 0 && (!d_x || !d_y || !d_z || !d_label)) || !(r_max > 0.0) || !isfinite(r_max)
        || (pbc && (!h_lattice || !(h_lattice[1] > 0.0) || !(h_lattice[2] > 0.0) || !isfinite(h_lattice[1]) || !isfinite(h_lattice[2]))))
        return dkmc_fail(3, "dkmc_find_gaps: bad arguments (N >= 0, device arrays of N sites, r_max finite and > 0, a positive lattice with pbc)", __FILE__, __LINE__);
    clamp_seeds(N, n_left_sites, n_right_sites);
    g_gap.reset();
    if (N == 0) { g_gap.valid = 1; return 0; }
    hipStream_t st = eng().stream;
    const size_t n = (size_t)N, nnode = n + 2;
    const int site_blocks = (N + GP_NT - 1) / GP_NT, node_blocks = (int)((nnode + GP_NT - 1) / GP_NT);

    // components, their contact flags, the members' box
    int *persite = (int *)scratch(S_GAP_SITE, 3 * n * sizeof(int));
    char *ctrl_raw = (char *)scratch(S_GAP_CTRL, sizeof(GpCtrl) + (size_t)CELL_BOX_BLOCKS * (6 * sizeof(double) + sizeof(int)));
    if (!persite || !ctrl_raw) return eng().err_code;
    int *cflags = persite, *cell_id = persite + n, *node_site = persite + 2 * n;
    GpCtrl *ctrl = (GpCtrl *)ctrl_raw;
    double *box = (double *)(ctrl_raw + sizeof(GpCtrl));
    int *cnt = (int *)(box + CELL_BOX_BLOCKS * 6);
    HIPCHK(hipMemsetAsync(ctrl, 0, sizeof(GpCtrl), st));
    HIPCHK(hipMemsetAsync(cflags, 0, n * sizeof(int), st));
    hipLaunchKernelGGL(k_gp_flags, dim3(site_blocks), dim3(GP_NT), 0, st, N, d_label, n_left_sites, n_right_sites, cflags, ctrl);
    hipLaunchKernelGGL(k_gp_census, dim3(CELL_BOX_BLOCKS), dim3(GP_NT), 0, st, N, d_label, (const int *)cflags, d_x, d_y, d_z, box, cnt, ctrl);
    KCHK();
    static double h_box[CELL_BOX_BLOCKS * 6];
    static int h_cnt[CELL_BOX_BLOCKS];
    GpCtrl h_ctrl;
    HIPCHK(hipMemcpyAsync(h_box, box, sizeof(h_box), hipMemcpyDeviceToHost, st));
    HIPCHK(hipMemcpyAsync(h_cnt, cnt, sizeof(h_cnt), hipMemcpyDeviceToHost, st));
    HIPCHK(hipMemcpyAsync(&h_ctrl, ctrl, sizeof(GpCtrl), hipMemcpyDeviceToHost, st));
    HIPCHK(hipStreamSynchronize(st));
    double mn[3], mx[3];
    fold_boxes(h_box, mn, mx);
    long long members = 0;
    for (int b = 0; b < CELL_BOX_BLOCKS; ++b) members += h_cnt[b];
    if (members == 0) { g_gap.valid = 1; return 0; }
    if (!isfinite(mn[0]) || !isfinite(mx[0]) || !isfinite(mn[1]) || !isfinite(mx[1]) || !isfinite(mn[2]) || !isfinite(mx[2]))
        return dkmc_fail(3, "dkmc_find_gaps: a member site has a coordinate that is not finite", __FILE__, __LINE__);
    const int M = (int)members;
    const bool has_l = h_ctrl.flags & 1, has_r = h_ctrl.flags & 2, bridged = h_ctrl.flags & 4;

    // the grid: cells of edge >= r_max (2^-30 more), doubled until the cells are few enough
    CellGrid G; G.pbc = pbc ? 1 : 0; G.laty = pbc ? h_lattice[1] : 1.0; G.latz = pbc ? h_lattice[2] : 1.0;
    G.x0 = mn[0]; G.y0 = mn[1]; G.z0 = mn[2];
    long long ncell = 0;
    for (double h = r_max * (1.0 + 0x1p-30);; h *= 2.0) {
        G.nx = gp_cells(mx[0] - mn[0], h); G.hx = h;
        if (pbc) {
            G.ny = gp_cells(G.laty, h); G.nz = gp_cells(G.latz, h);
            if (G.ny > 1) --G.ny;                             // floor(lat / h) cells, at least one: each at least h wide
            if (G.nz > 1) --G.nz;
            G.hy = G.ny > 0 ? G.laty / G.ny : h; G.hz = G.nz > 0 ? G.latz / G.nz : h;
        } else {
            G.ny = gp_cells(mx[1] - mn[1], h); G.nz = gp_cells(mx[2] - mn[2], h); G.hy = G.hz = h;
        }
        if (G.nx > 0 && G.ny > 0 && G.nz > 0) {
            ncell = (long long)G.nx * G.ny * G.nz;
            if (ncell <= GP_MAX_CELLS) break;
        }
        if (!isfinite(h)) return dkmc_fail(3, "dkmc_find_gaps: no cell grid for these coordinates", __FILE__, __LINE__);
    }
    const size_t nc = (size_t)ncell + 4, m = (size_t)M;
    int *cells = (int *)scratch(S_GAP_CELLS, 4 * nc * sizeof(int));
    char *sorted = (char *)scratch(S_GAP_SORTED, m * (5 * sizeof(double) + 2 * sizeof(int)));
    char *nodes = (char *)scratch(S_GAP_NODES, nnode * (4 * sizeof(unsigned long long) + 2 * sizeof(int)));
    char *edges = (char *)scratch(S_GAP_EDGES, m * (2 * sizeof(unsigned long long) + 4 * sizeof(int)));
    if (!cells || !sorted || !nodes || !edges) return eng().err_code;
    int *cell_cnt = cells, *cell_start = cells + nc, *cell_fill = cells + 2 * nc, *cell_node = cells + 3 * nc;
    double *sx = (double *)sorted, *sy = sx + m, *sz = sy + m;
    unsigned long long *mykey = (unsigned long long *)(sz + m), *mypair = mykey + m;
    int *ssite = (int *)(mypair + m), *snode = ssite + m;
    unsigned long long *best_d2[2], *best_pair[2];
    best_d2[0] = (unsigned long long *)nodes; best_d2[1] = best_d2[0] + nnode; best_pair[0] = best_d2[1] + nnode; best_pair[1] = best_pair[0] + nnode;
    int *parent = (int *)(best_pair[1] + nnode), *newroot = parent + nnode;
    unsigned long long *ekey = (unsigned long long *)edges, *epair = ekey + m;
    int *row4 = (int *)(epair + m);
    const int mem_blocks = (M + GP_NT - 1) / GP_NT, cell_blocks = (int)((ncell + GP_NT - 1) / GP_NT);
    const int skip = g_gap_cell_skip;
    const double r2max = r_max * r_max;                       // one rounded product: __dmul_rn(r_max, r_max)

    HIPCHK(hipMemsetAsync(cells, 0, 3 * nc * sizeof(int), st));
    HIPCHK(hipMemsetAsync(best_d2[0], 0xff, 4 * nnode * sizeof(unsigned long long), st));
    hipLaunchKernelGGL(k_cell_count, dim3(site_blocks), dim3(GP_NT), 0, st, N, G, d_label, d_x, d_y, d_z, cell_id, cell_cnt);
    KCHK();
    if (int rc = dkmc_exclusive_scan_i32(cell_cnt, cell_start, (int)ncell, nullptr)) return rc;
    hipLaunchKernelGGL(k_gp_scatter, dim3(site_blocks), dim3(GP_NT), 0, st, N, M, (const int *)cell_id, (const int *)cell_start, cell_fill, d_label,
                       (const int *)cflags, (const GpCtrl *)ctrl, d_x, d_y, d_z, sx, sy, sz, ssite, snode, node_site);
    hipLaunchKernelGGL(k_gp_node_init, dim3(node_blocks), dim3(GP_NT), 0, st, (int)nnode, parent);
    if (skip)
        hipLaunchKernelGGL(k_gp_cell_uniform, dim3(cell_blocks), dim3(GP_NT), 0, st, (int)ncell, (const int *)cell_start, (const int *)cell_cnt,
                           (const int *)snode, cell_node, (const GpCtrl *)ctrl, 0);
    KCHK();
    // the direct gap, on the words of the odd rounds
    if (has_l && has_r && !bridged) {
        hipLaunchKernelGGL(k_gp_search<1>, dim3(mem_blocks), dim3(GP_NT), 0, st, M, N, G, r2max, (const double *)sx, (const double *)sy, (const double *)sz,
                           (const int *)ssite, (const int *)snode, (const int *)cell_start, (const int *)cell_cnt, (const int *)cell_node, skip,
                           best_d2[1], mykey, mypair, ctrl, 0);
        hipLaunchKernelGGL(k_gp_pick, dim3(mem_blocks), dim3(GP_NT), 0, st, M, (const int *)snode, (const unsigned long long *)mykey,
                           (const unsigned long long *)mypair, (const unsigned long long *)best_d2[1], best_pair[1], (const GpCtrl *)ctrl, 0);
        hipLaunchKernelGGL(k_gp_save_direct, dim3(1), dim3(1), 0, st, N, best_d2[1], best_pair[1], ctrl);
        KCHK();
    }
    // rounds: GP_BATCH of them per read-back of the control block (not run_rounds, rounds.h: the host needs GpCtrl's other fields too -- one copy here)
    int rounds = 0, launched = 0;
    while (!rounds && launched < GP_ROUND_CAP) {
        const int b = GP_ROUND_CAP - launched < GP_BATCH ? GP_ROUND_CAP - launched : GP_BATCH;
        for (int r = launched; r < launched + b; ++r) {
            const int cur = r & 1, nxt = cur ^ 1;
            hipLaunchKernelGGL(k_gp_search<0>, dim3(mem_blocks), dim3(GP_NT), 0, st, M, N, G, r2max, (const double *)sx, (const double *)sy,
                               (const double *)sz, (const int *)ssite, (const int *)snode, (const int *)cell_start, (const int *)cell_cnt,
                               (const int *)cell_node, skip, best_d2[cur], mykey, mypair, ctrl, r);
            hipLaunchKernelGGL(k_gp_pick, dim3(mem_blocks), dim3(GP_NT), 0, st, M, (const int *)snode, (const unsigned long long *)mykey,
                               (const unsigned long long *)mypair, (const unsigned long long *)best_d2[cur], best_pair[cur], (const GpCtrl *)ctrl, r);
            hipLaunchKernelGGL(k_gp_edges, dim3(node_blocks), dim3(GP_NT), 0, st, (int)nnode, (const int *)node_site,
                               (const unsigned long long *)best_d2[cur], (const unsigned long long *)best_pair[cur], best_d2[nxt], best_pair[nxt], parent,
                               ekey, epair, M, ctrl, r);
            hipLaunchKernelGGL(k_gp_roots, dim3(node_blocks), dim3(GP_NT), 0, st, (int)nnode, (const unsigned long long *)best_d2[cur], (const int *)parent,
                               newroot, (const GpCtrl *)ctrl, r);
            hipLaunchKernelGGL(k_gp_refresh, dim3(mem_blocks), dim3(GP_NT), 0, st, M, (const int *)ssite, (const int *)newroot, node_site, snode,
                               (const GpCtrl *)ctrl, r);
            if (skip)
                hipLaunchKernelGGL(k_gp_cell_uniform, dim3(cell_blocks), dim3(GP_NT), 0, st, (int)ncell, (const int *)cell_start, (const int *)cell_cnt,
                                   (const int *)snode, cell_node, (const GpCtrl *)ctrl, r + 1);
        }
        KCHK();
        HIPCHK(hipMemcpyAsync(&h_ctrl, ctrl, sizeof(GpCtrl), hipMemcpyDeviceToHost, st));
        HIPCHK(hipStreamSynchronize(st));
        for (int r = launched; r < launched + b && !rounds; ++r) if (!h_ctrl.any[r]) rounds = r + 1;
        launched += b;
    }
    if (!rounds) return dkmc_fail(4, "dkmc_find_gaps: the rounds did not end", __FILE__, __LINE__);
    const int E = h_ctrl.n_edges;
    if (E < 0 || (E > 0 && E >= h_ctrl.n_components)) return dkmc_fail(4, "dkmc_find_gaps: more forest edges than components", __FILE__, __LINE__);

    // the table: rows gathered on the device, sorted by (d2, a, b) here
    std::vector<unsigned long long> h_key((size_t)E), h_pair((size_t)E);
    std::vector<int> h_row((size_t)4 * E);
    if (E > 0) {
        hipLaunchKernelGGL(k_gp_edge_rows, dim3((E + GP_NT - 1) / GP_NT), dim3(GP_NT), 0, st, E, (const unsigned long long *)epair, d_label,
                           (const int *)cflags, row4);
        KCHK();
        HIPCHK(hipMemcpyAsync(h_key.data(), ekey, (size_t)E * sizeof(unsigned long long), hipMemcpyDeviceToHost, st));
        HIPCHK(hipMemcpyAsync(h_pair.data(), epair, (size_t)E * sizeof(unsigned long long), hipMemcpyDeviceToHost, st));
        HIPCHK(hipMemcpyAsync(h_row.data(), row4, (size_t)4 * E * sizeof(int), hipMemcpyDeviceToHost, st));
        HIPCHK(hipStreamSynchronize(st));
    }
    std::vector<int> order((size_t)E);
    for (int e = 0; e < E; ++e) order[e] = e;
    std::sort(order.begin(), order.end(), [&](int p, int q) { return h_key[p] != h_key[q] ? h_key[p] < h_key[q] : h_pair[p] < h_pair[q]; });
    std::vector<int> node_a((size_t)E), node_b((size_t)E);
    auto node_of = [&](int root, int f) { return f == 0 ? root : ((f & 1) || bridged ? -1 : -2); };
    ResultTable<4, 1> &T = g_gap.edges;
    T.resize((size_t)E);
    for (int k = 0; k < E; ++k) {
        const int e = order[k];
        T.i[E_A][k] = (int)(h_pair[e] >> 32); T.i[E_B][k] = (int)(h_pair[e] & 0xffffffffull);
        T.d[0][k] = key_dbl(h_key[e]);
        node_a[k] = node_of(h_row[4 * e], h_row[4 * e + 2]); node_b[k] = node_of(h_row[4 * e + 1], h_row[4 * e + 3]);
        T.i[E_RA][k] = h_row[4 * e]; T.i[E_RB][k] = h_row[4 * e + 1];
    }
    g_gap.info[0] = h_ctrl.n_components; g_gap.info[1] = E; g_gap.info[4] = rounds; g_gap.info[5] = (long long)h_ctrl.pairs;
    if (bridged) { g_gap.info[2] = 2; g_gap.d2x2[0] = 0.0; }
    else if (has_l && has_r) {
        gap_chain(node_a, node_b);
        if (h_ctrl.direct_key != GP_NONE) {
            g_gap.d2x2[1] = key_dbl(h_ctrl.direct_key);
            g_gap.info[6] = (long long)(h_ctrl.direct_pair >> 32); g_gap.info[7] = (long long)(h_ctrl.direct_pair & 0xffffffffull);
        }
    }
    g_gap.valid = 1;
    return 0;
}

int dkmc_get_gap_info(long long *info8, double *d2x2)
{
    NEED_FINISHED(g_gap.valid, "dkmc_get_gap_info", "dkmc_find_gaps");
    if (info8) memcpy(info8, g_gap.info, sizeof(g_gap.info));
    if (d2x2) memcpy(d2x2, g_gap.d2x2, sizeof(g_gap.d2x2));
    return 0;
}

int dkmc_copy_gap_edges(int capacity, int *h_site_a, int *h_site_b, int *h_root_a, int *h_root_b, double *h_d2, int *rows_out)
{
    NEED_FINISHED(g_gap.valid, "dkmc_copy_gap_edges", "dkmc_find_gaps");
    g_gap.edges.copy_out(capacity, rows_out, {h_site_a, h_site_b, h_root_a, h_root_b}, {h_d2});
    return 0;
}

int dkmc_copy_gap_chain(int capacity, int *h_from, int *h_to, double *h_d2, int *rows_out)
{
    NEED_FINISHED(g_gap.valid, "dkmc_copy_gap_chain", "dkmc_find_gaps");
    g_gap.chain.copy_out(capacity, rows_out, {h_from, h_to}, {h_d2});
    return 0;
}

}   // extern "C"
