// clusters.hip -- filament analysis: connected components of the "member" sites over a padded neighbour index, their summaries, contact flags
// and the bridging verdict (dkmc_find_clusters; definitions: include/devicekmc_hip.h).  No counterpart in the reference.  A pure function of its
// arguments: nothing of GPUBuffers, no engine state a later phase reads and no other kernel is touched.
//
// Labelling: the min-hooking + compression rounds of rounds.h (label_rounds; the argument for their soundness is there) on label[], the caller's
//   array, which ends on the smallest site index of each component; "rounds" is the number the synchronous host model (tests/cluster_ref.py) gives.
#include "rounds.h"

#define CL_NT 256
#define CL_CAP_DEFAULT 64
#define CL_CAP_MAX ROUND_CAP_MAX

namespace {

struct ClInfoDev {
    int n_members, n_components, bridged, bridge_root, largest_free_size, pad[3];
    double tip_left_x, tip_right_x, gap_x;
};
struct ClusterState {
    int valid = 0, N = 0, rounds = 0;
    ClInfoDev info{};
    double ms_label = 0.0, ms_sum = 0.0;
    PhaseTimer<2> timer;
} g_cl;
int g_round_cap = CL_CAP_DEFAULT;

// 1. membership: member flag as the initial root / parent (the site itself, -1 for a non-member), and the identities of the per-root summaries
__global__ __launch_bounds__(CL_NT) void k_cl_members(int N, const int *el, const int *charge, MetalSet ms, int members,
                                                      int *label, int *parent, int *csize, int *cvac, int *cflags,
                                                      unsigned long long *kmin, unsigned long long *kmax)
{
    const int i = blockIdx.x * CL_NT + threadIdx.x;
    if (i >= N) return;
    const int e = el[i];
    bool m = (members & 1) && is_metal(e, ms);
    if ((members & 2) && e == VACANCY) m = m || !(members & 4) || charge[i] == 0;
    label[i] = parent[i] = m ? i : -1;
    csize[i] = 0; cvac[i] = 0; cflags[i] = 0;
    kmin[i] = ~0ull; kmax[i] = 0ull;
}

// 3a. summaries per root: integer atomics only (counts, OR, min / max of the keys), so the order of arrival does not matter.  A wave whose
// members all carry one root -- the rule inside a contact slab -- combines them first and sends one set of atomics.
__global__ __launch_bounds__(CL_NT) void k_cl_summaries(int N, const int *label, const int *el, const double *x, int n_left, int n_right,
                                                        int *csize, int *cvac, int *cflags, unsigned long long *kmin, unsigned long long *kmax,
                                                        int *isroot)
{
    const int i = blockIdx.x * CL_NT + threadIdx.x;
    const int r = i < N ? label[i] : -1;
    const bool mem = r >= 0;
    if (i < N) isroot[i] = (r == i) ? 1 : 0;
    const bool vac = mem && el[i] == VACANCY;
    const int f = mem ? seed_bits(i, N, n_left, n_right) : 0;
    const unsigned long long key = mem ? dbl_key(x[i]) : 0ull;
    const unsigned long long bm = __ballot(mem);
    if (bm == 0ull) return;
    const int first = __ffsll((long long)bm) - 1;
    const int r0 = __shfl(r, first, WAVE);
    if (__all(!mem || r == r0)) {
        const int cnt = __popcll(bm), nv = __popcll(__ballot(vac));
        const int ff = (__ballot(f & 1) ? 1 : 0) | (__ballot(f & 2) ? 2 : 0);
        const unsigned long long lo = wave_min(mem ? key : ~0ull), hi = wave_max(mem ? key : 0ull);
        if ((int)(threadIdx.x & 63) == first) {
            atomicAdd(&csize[r0], cnt);
            if (nv) atomicAdd(&cvac[r0], nv);
            if (ff) atomicOr(&cflags[r0], ff);
            atomicMin(&kmin[r0], lo); atomicMax(&kmax[r0], hi);
        }
    } else if (mem) {
        atomicAdd(&csize[r], 1);
        if (vac) atomicAdd(&cvac[r], 1);
        if (f) atomicOr(&cflags[r], f);
        atomicMin(&kmin[r], key); atomicMax(&kmax[r], key);
    }
}

// 3b. the table: one row per root, ascending (pos = exclusive scan of the root flags)
__global__ __launch_bounds__(CL_NT) void k_cl_table(int N, const int *isroot, const int *pos, const int *csize, const int *cvac, const int *cflags,
                                                    const unsigned long long *kmin, const unsigned long long *kmax,
                                                    int *t_root, int *t_size, int *t_vac, int *t_flags, double *t_xmin, double *t_xmax)
{
    const int i = blockIdx.x * CL_NT + threadIdx.x;
    if (i >= N || !isroot[i]) return;
    const int p = pos[i];
    t_root[p] = i; t_size[p] = csize[i]; t_vac[p] = cvac[i]; t_flags[p] = cflags[i];
    t_xmin[p] = key_dbl(kmin[i]); t_xmax[p] = key_dbl(kmax[i]);
}

// 3c. the info block, one workgroup: sums, minima and maxima only (no order dependence)
__global__ __launch_bounds__(CL_NT) void k_cl_info(const int *d_ncomp, const int *t_root, const int *t_size, const int *t_flags,
                                                   const double *t_xmin, const double *t_xmax, ClInfoDev *out)
{
    __shared__ int s_mem[CL_NT], s_broot[CL_NT], s_free[CL_NT];
    __shared__ double s_tl[CL_NT], s_tr[CL_NT];
    const int nc = *d_ncomp, t = threadIdx.x;
    int mem = 0, broot = 0x7fffffff, fre = 0;
    double tl = -INFINITY, tr = INFINITY;
    for (int j = t; j < nc; j += CL_NT) {
        const int f = t_flags[j], s = t_size[j];
        mem += s;
        if (f == 3) broot = min(broot, t_root[j]);
        if (f == 0) fre = max(fre, s);
        if (f == 1) tl = fmax(tl, t_xmax[j]);
        if (f == 2) tr = fmin(tr, t_xmin[j]);
    }
    s_mem[t] = mem; s_broot[t] = broot; s_free[t] = fre; s_tl[t] = tl; s_tr[t] = tr;
    __syncthreads();
    for (int off = CL_NT / 2; off > 0; off >>= 1) {
        if (t < off) {
            s_mem[t] += s_mem[t + off]; s_broot[t] = min(s_broot[t], s_broot[t + off]); s_free[t] = max(s_free[t], s_free[t + off]);
            s_tl[t] = fmax(s_tl[t], s_tl[t + off]); s_tr[t] = fmin(s_tr[t], s_tr[t + off]);
        }
        __syncthreads();
    }
    if (t == 0) {
        const int bridged = s_broot[0] != 0x7fffffff;
        out->n_members = s_mem[0]; out->n_components = nc; out->bridged = bridged; out->bridge_root = bridged ? s_broot[0] : -1;
        out->largest_free_size = s_free[0]; out->pad[0] = out->pad[1] = out->pad[2] = 0;
        out->tip_left_x = s_tl[0]; out->tip_right_x = s_tr[0];
        out->gap_x = bridged ? 0.0 : s_tr[0] - s_tl[0];
    }
}

struct ClTable { int *root, *size, *vac, *flags; double *xmin, *xmax; };
ClTable table_of(void *base, size_t N)
{
    ClTable t;
    t.xmin = (double *)base; t.xmax = t.xmin + N;
    t.root = (int *)(t.xmax + N); t.size = t.root + N; t.vac = t.size + N; t.flags = t.vac + N;
    return t;
}

}   // namespace

extern "C" {

void dkmc_debug_set_cluster_round_cap(int cap) { g_round_cap = clamp_round_cap(cap, CL_CAP_DEFAULT); }

int dkmc_debug_get_cluster_times(double *ms2)
{
    NEED_FINISHED(g_cl.valid, "dkmc_debug_get_cluster_times", "dkmc_find_clusters");
    if (ms2) { ms2[0] = g_cl.ms_label; ms2[1] = g_cl.ms_sum; }
    return 0;
}

int dkmc_find_clusters(int N, int nn, const int *d_index, const int *d_site_element, const int *d_site_charge, const double *d_site_x,
                       const int *d_metals, int num_metals, int members, int n_left_sites, int n_right_sites, int *d_label)
{
    g_cl.valid = 0;
    if (N < 0 || nn < 1 || (N > 0 && (!d_index || !d_site_element || !d_site_x || !d_label)) || ((members & 4) && N > 0 && !d_site_charge)
        || ((members & 1) && num_metals > 0 && !d_metals) || num_metals < 0)
        return dkmc_fail(3, "dkmc_find_clusters: bad arguments (N >= 0, nn >= 1, device arrays of N sites; site_charge with members bit 2)", __FILE__, __LINE__);
    clamp_seeds(N, n_left_sites, n_right_sites);
    hipStream_t st = eng().stream;
    const int cap = g_round_cap;
    g_cl.N = N; g_cl.rounds = 0; g_cl.ms_label = g_cl.ms_sum = 0.0;
    if (N == 0) {
        g_cl.info = ClInfoDev{}; g_cl.info.bridge_root = -1; g_cl.info.tip_left_x = -INFINITY; g_cl.info.tip_right_x = INFINITY; g_cl.info.gap_x = INFINITY;
        g_cl.valid = 1;
        return 0;
    }
    const size_t n = (size_t)N;
    int *parent = (int *)scratch(S_CL_PARENT, n * sizeof(int));
    char *sums = (char *)scratch(S_CL_SUMS, n * (2 * sizeof(unsigned long long) + 3 * sizeof(int)));
    int *flagpos = (int *)scratch(S_CL_POS, 2 * n * sizeof(int));
    void *tab = scratch(S_CL_TABLE, n * (2 * sizeof(double) + 4 * sizeof(int)));
    int *ctrl = (int *)scratch(S_CL_CTRL, (size_t)(CL_CAP_MAX + 2) * sizeof(int) + sizeof(ClInfoDev));
    if (!parent || !sums || !flagpos || !tab || !ctrl) return eng().err_code;
    unsigned long long *kmin = (unsigned long long *)sums, *kmax = kmin + n;
    int *csize = (int *)(kmax + n), *cvac = csize + n, *cflags = cvac + n;
    int *isroot = flagpos, *pos = flagpos + n;
    int *d_ncomp = ctrl + CL_CAP_MAX;
    ClInfoDev *d_info = (ClInfoDev *)(ctrl + CL_CAP_MAX + 2);
    const ClTable T = table_of(tab, n);

    const int site_blocks = (N + CL_NT - 1) / CL_NT;
    HIPCHK(g_cl.timer.start(eng().profiling != 0, st));
    HIPCHK(hipMemsetAsync(ctrl, 0, (size_t)(CL_CAP_MAX + 2) * sizeof(int), st));
    hipLaunchKernelGGL(k_cl_members, dim3(site_blocks), dim3(CL_NT), 0, st, N, d_site_element, d_site_charge, load_metals(d_metals, (members & 1) ? num_metals : 0),
                       members, d_label, parent, csize, cvac, cflags, kmin, kmax);
    KCHK();
    int rounds = 0;
    if (int rc = label_rounds(st, N, nn, d_index, d_label, parent, ctrl, cap, &rounds)) return rc;
    if (!rounds) {
        char msg[200];
        snprintf(msg, sizeof(msg), "dkmc_find_clusters: labelling not finished after %d rounds (the cap: dkmc_debug_set_cluster_round_cap); labels set to -1", cap);
        return abandon(st, n, {d_label}, msg, __FILE__, __LINE__);
    }
    HIPCHK(g_cl.timer.mark(1, st));
    // summaries, table, info
    hipLaunchKernelGGL(k_cl_summaries, dim3(site_blocks), dim3(CL_NT), 0, st, N, (const int *)d_label, d_site_element, d_site_x, n_left_sites, n_right_sites,
                       csize, cvac, cflags, kmin, kmax, isroot);
    KCHK();
    if (int rc = dkmc_exclusive_scan_i32(isroot, pos, N, d_ncomp)) return rc;
    hipLaunchKernelGGL(k_cl_table, dim3(site_blocks), dim3(CL_NT), 0, st, N, (const int *)isroot, (const int *)pos, (const int *)csize, (const int *)cvac,
                       (const int *)cflags, (const unsigned long long *)kmin, (const unsigned long long *)kmax, T.root, T.size, T.vac, T.flags, T.xmin, T.xmax);
    hipLaunchKernelGGL(k_cl_info, dim3(1), dim3(CL_NT), 0, st, (const int *)d_ncomp, (const int *)T.root, (const int *)T.size, (const int *)T.flags,
                       (const double *)T.xmin, (const double *)T.xmax, d_info);
    KCHK();
    HIPCHK(g_cl.timer.mark(2, st));
    HIPCHK(hipMemcpyAsync(&g_cl.info, d_info, sizeof(ClInfoDev), hipMemcpyDeviceToHost, st));
    HIPCHK(hipStreamSynchronize(st));
    float ms[2] = {0.f, 0.f};
    HIPCHK(g_cl.timer.read(ms));
    g_cl.ms_label = ms[0]; g_cl.ms_sum = ms[1];
    g_cl.rounds = rounds;
    g_cl.valid = 1;
    return 0;
}

int dkmc_copy_cluster_table(int capacity, int *h_root, int *h_size, int *h_n_vacancy, int *h_flags, double *h_xmin, double *h_xmax, int *rows_out)
{
    NEED_FINISHED(g_cl.valid, "dkmc_copy_cluster_table", "dkmc_find_clusters");
    const size_t r = clamp_rows(capacity, g_cl.info.n_components, rows_out);
    if (r == 0) return 0;
    hipStream_t st = eng().stream;
    const ClTable T = table_of(eng().buf[S_CL_TABLE], (size_t)g_cl.N);
    if (h_root) HIPCHK(hipMemcpyAsync(h_root, T.root, r * sizeof(int), hipMemcpyDeviceToHost, st));
    if (h_size) HIPCHK(hipMemcpyAsync(h_size, T.size, r * sizeof(int), hipMemcpyDeviceToHost, st));
    if (h_n_vacancy) HIPCHK(hipMemcpyAsync(h_n_vacancy, T.vac, r * sizeof(int), hipMemcpyDeviceToHost, st));
    if (h_flags) HIPCHK(hipMemcpyAsync(h_flags, T.flags, r * sizeof(int), hipMemcpyDeviceToHost, st));
    if (h_xmin) HIPCHK(hipMemcpyAsync(h_xmin, T.xmin, r * sizeof(double), hipMemcpyDeviceToHost, st));
    if (h_xmax) HIPCHK(hipMemcpyAsync(h_xmax, T.xmax, r * sizeof(double), hipMemcpyDeviceToHost, st));
    HIPCHK(hipStreamSynchronize(st));
    return 0;
}

int dkmc_get_cluster_info(int *info8, double *x3)
{
    NEED_FINISHED(g_cl.valid, "dkmc_get_cluster_info", "dkmc_find_clusters");
    const ClInfoDev &I = g_cl.info;
    if (info8) {
        info8[0] = I.n_members; info8[1] = I.n_components; info8[2] = I.bridged; info8[3] = I.bridge_root; info8[4] = I.largest_free_size;
        info8[5] = g_cl.rounds; info8[6] = 0; info8[7] = 0;
    }
    if (x3) { x3[0] = I.tip_left_x; x3[1] = I.tip_right_x; x3[2] = I.gap_x; }
    return 0;
}

}   // extern "C"
