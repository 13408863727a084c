// heat.hip -- global temperature update; local temperature model.
#include "common.h"
#include "kcg_run.h"
#include "launch_plan.h"

#define HT_NT 256
__global__ __launch_bounds__(HT_NT) void k_power_partials(int N, const double *__restrict__ p, double *__restrict__ part)
{
    __shared__ double red[HT_NT / 64];
    double s = 0.0;
    for (int i = blockIdx.x * HT_NT + threadIdx.x; i < N; i += gridDim.x * HT_NT) s += p[i];
    const double t = block_sum_all<HT_NT>(s, red);
    if (threadIdx.x == 0) part[blockIdx.x] = t;
}

// mode 0: heat_solver.cpp:322-334 (what the reference runs, on the host); mode 1: heat_solver_gpu.cu:42-48
__global__ __launch_bounds__(HT_NT) void k_temp_update(const double *__restrict__ part, int npart, double *T_bg, double *P_out, int mode,
                                                       double a0, double a1, double a2, double a3, double a4)
{
    __shared__ double red[HT_NT / 64];
    double s = 0.0;
    for (int i = threadIdx.x; i < npart; i += HT_NT) s += part[i];
    const double P = block_sum_all<HT_NT>(s, red);
    if (threadIdx.x != 0) return;
    if (P_out) *P_out = P;
    if (mode == 0) {
        const double event_time = a0, diss = a1, C = a2;
        const double a = diss / C;
        const double c = (diss / C) * (*T_bg) + (1 / C) * P;
        *T_bg = (c / a) + (*T_bg - c / a) * exp(-a * event_time);
    } else {
        const double a_coeff = a0, b_coeff = a1, number_steps = a2, C_thermal = a3, small_step = a4;
        const double c_coeff = b_coeff + P / C_thermal * small_step;
        const double T_int = *T_bg;
        const int step = (int)number_steps;
        *T_bg = c_coeff * (1.0 - pow(a_coeff, (double)step)) / (1.0 - a_coeff) + pow(a_coeff, (double)step) * T_int;
    }
}

static int temp_update(const double *site_power, double *T_bg, int N, int mode, double a0, double a1, double a2, double a3, double a4, double *h_P)
{
    Engine &e = eng(); hipStream_t st = e.stream;
    int nb = (N + HT_NT - 1) / HT_NT; if (nb > 1024) nb = 1024; if (nb < 1) nb = 1;
    double *part = (double *)scratch(S_HEAT, (size_t)(nb + 2) * 8);
    if (!part) return e.err_code;
    hipLaunchKernelGGL(k_power_partials, dim3(nb), dim3(HT_NT), 0, st, N, site_power, part);
    hipLaunchKernelGGL(k_temp_update, dim3(1), dim3(HT_NT), 0, st, part, nb, T_bg, part + nb, mode, a0, a1, a2, a3, a4);
    KCHK();
    if (h_P) { HIPCHK(hipMemcpyAsync(h_P, part + nb, 8, hipMemcpyDeviceToHost, st)); HIPCHK(hipStreamSynchronize(st)); }
    return 0;
}

extern "C" int dkmc_update_temperatureglobal_gpu(const double *site_power, double *T_bg, int N, double a_coeff, double b_coeff,
                                                 double number_steps, double C_thermal, double small_step)
{
    return temp_update(site_power, T_bg, N, 1, a_coeff, b_coeff, number_steps, C_thermal, small_step, nullptr);
}

extern "C" int dkmc_update_temperature_global_analytic(const double *site_power, double *T_bg, int N, double event_time,
                                                       double dissipation_constant, double t_ox, double A, double c_p, double *h_P_tot)
{
    const double C = A * t_ox * c_p * (1e6);
    return temp_update(site_power, T_bg, N, 0, event_time, dissipation_constant, C, 0, 0, h_P_tot);
}

// =============================================================================================================================
// Local temperature model (heat_solver.cpp:40-246, 286-308, 354-513).  The reference runs it on the host: it inverts the dense
// N_interface x N_interface matrices (I - dt*tau*L) and L once (constructLaplacian) and multiplies by the dense inverses in every
// update -- O(N_interface^2) memory, which stops at a few 1e4 sites.  Here the same linear systems are solved in their sparse
// form with the Jacobi-CG of cg.hip: L is the graph Laplacian of the padded neighbour index restricted to the interface sites
// (1 per neighbour pair, diagonal -gamma*[a neighbour is metallic] - degree), so (I - s*L) and -L are symmetric positive
// definite with ~26 entries per row.
//   transient  :  (I - s L) y = T_vec + P c s ,  T = y (T_1 - T_0) + T_0           (updateLocalTemperature, :354-437)
//   steady     :  (-L) y = P c                ,  T = y (T_1 - T_0) + T_0           (updateLocalTemperatureSteadyState, :441-513:
//                                                                                   T = -(L^-1 P c)(T_1 - T_0) + T_0)
// with c = p_transfer of the site (:369-370) and T_vec = (T - T_0)/(T_1 - T_0).  T_bg = mean of site_temperature over
// [num_atoms_contact, N - num_atoms_contact) (:423-432).  The power vector is gpubuf.site_power, i.e. the one update_power just
// wrote (the reference's GPU build multiplies a host copy that is never refreshed in this branch).
int cg_solve_jacobi(double *a, const int *rp, const int *ci, int nnz, int m, double *x, double *y,
                    int uniform_rows, const int *srank, int ns, int *iters_out, double *rr_out);

#define DKMC_T1 50.0            // Device.h:117

// dkmc_set_heat_form(1): the same systems on the pattern-only CG of kcg.hip (kcg_run.h).  I - s L and -L have ONE off-diagonal value (-s, -1) and no
// contacts: K's special case with w_high = w_low.  What K's assembly would store for such a matrix is the form's own column table -- every link of the
// low class (no class bit), the diagonal (CSR positions) and the padding (blocked forms) the row's own column, which the products skip -- so the
// stored words ARE ci (CSR positions) or the form's pcol (blocked forms, 4-byte words): nothing is written per solve but the right-hand side, and the
// scaling is applied to the vectors.  4 B per non-zero and iteration instead of 12, no k_heat_system pass over the values, no scaling pass.
// With more than one transient sub-step the solves are chained on the device (heat_chain_*): a fixed budget of iterations per sub-step, k_heat_next
// between them, one host synchronisation per batch of HEAT_CHAIN_BATCH sub-steps.
#define HEAT_CHAIN_BATCH 16
struct HeatChain { KCtrl start; int fail; int iters[HEAT_CHAIN_BATCH]; };      // start: the stop word k_kc_check0 leaves, armed into the loop's by k_heat_arm
struct HeatPat {
    int N = 0, nn = 0, lo = 0, m = 0, nnz = 0;      // interface sites [lo, lo+m)
    int *rp = nullptr, *ci = nullptr;
    double *diagL = nullptr;                          // diagonal of L per interface row
    const int *neigh = nullptr;
    // dkmc_set_heat_form(1) at construct
    int form = -1;                                    // -1: the general CSR loop of cg.hip; 0 / 1 / 2: K-CG on the CSR positions / blocked / windowed blocked form
    KBlocked *kb = nullptr;                           // forms 1, 2 (stored words: kb->pcol)
    double *diag = nullptr;                           // [2 m] in the form's row order: 1 - s diagL (built for diag_s) | -diagL
    double diag_s = 0.0; bool diag_built = false;
    HeatChain *chain = nullptr;
};
static HeatPat g_heat;
static double g_heat_tol = 1e-10;
static int g_heat_form = 0;                           // dkmc_set_heat_form
static int g_heat_chain_on = 1, g_heat_chain_budget = 0;      // dkmc_debug_heat_chain
static long long g_heat_info[8] = {-1, 0, 0, 0, 0, 0, 0, 0};

KBlocked *kpattern_form_build(const int *rp_d, const int *ci_d, int m, int nnz, const double *x_d, const double *y_d, const double *z_d, hipStream_t st);
void kblocked_free(KBlocked *kb);

extern "C" void dkmc_set_heat_cg_tolerance(double tol) { g_heat_tol = tol; }
extern "C" void dkmc_set_heat_form(int form) { g_heat_form = form ? 1 : 0; }
extern "C" int dkmc_get_heat_form(void) { return g_heat_form; }
extern "C" void dkmc_debug_heat_chain(int on, int budget) { g_heat_chain_on = on ? 1 : 0; g_heat_chain_budget = budget > 0 ? budget : 0; }
extern "C" int dkmc_get_heat_info(long long *info8)
{
    if (!info8) return dkmc_fail(13, "get_heat_info: bad arguments", __FILE__, __LINE__);
    for (int k = 0; k < 8; ++k) info8[k] = g_heat_info[k];
    return 0;
}

static void heat_free(HeatPat &h)
{
    if (h.rp) (void)hipFree(h.rp);
    if (h.ci) (void)hipFree(h.ci);
    if (h.diagL) (void)hipFree(h.diagL);
    if (h.diag) (void)hipFree(h.diag);
    if (h.chain) (void)hipFree(h.chain);
    kblocked_free(h.kb);
    h = HeatPat{};
}

__global__ void k_heat_count(int m, int lo, int nn, const int *__restrict__ neigh, const int *__restrict__ element, MetalSet ms, double gamma,
                             int *__restrict__ cnt, double *__restrict__ diagL)
{
    const int r = blockIdx.x * blockDim.x + threadIdx.x;
    if (r >= m) return;
    const int *row = neigh + (size_t)(lo + r) * nn;
    int deg = 0; bool bnd = false;
    for (int s = 0; s < nn; ++s) {
        const int j = row[s];
        if (j < 0) continue;
        if (j >= lo && j < lo + m) ++deg;                 // L[ii][jj] = 1 (:120-123)
        bnd |= is_metal(element[j], ms);                  // :125-132, any neighbour, in the interface or not
    }
    cnt[r] = deg + 1;
    diagL[r] = (bnd ? -gamma : 0.0) - (double)deg;        // :142-153
}

__global__ void k_heat_fill(int m, int lo, int nn, const int *__restrict__ neigh, const int *__restrict__ rp, int *__restrict__ ci)
{
    const int r = blockIdx.x * blockDim.x + threadIdx.x;
    if (r >= m) return;
    const int i = lo + r;
    const int *row = neigh + (size_t)i * nn;
    int p = rp[r]; bool diag_done = false;
    for (int s = 0; s < nn; ++s) {
        const int j = row[s];
        if (j < lo || j >= lo + m) continue;
        if (!diag_done && j > i) { ci[p++] = r; diag_done = true; }
        ci[p++] = j - lo;
    }
    if (!diag_done) ci[p++] = r;
}

__global__ void k_set_last_h(int *rp, int m, const int *total) { if (threadIdx.x == 0 && blockIdx.x == 0) rp[m] = *total; }

// Device::constructLaplacian (heat_solver.cpp:40-246) in sparse form.  N_left_tot / N_right_tot: get_num_in_contacts (:5-37),
// computed by the caller from the host copy of site_element; gamma: :86.
extern "C" int dkmc_construct_laplacian(const dkmc_gpubuf *buf, int N_left_tot, int N_right_tot, double gamma)
{
    Engine &e = eng(); hipStream_t st = e.stream;
    HeatPat &h = g_heat;
    const int N = buf->N_, nn = buf->nn_, m = N - N_left_tot - N_right_tot;
    if (N_left_tot < 0 || N_right_tot < 0 || m <= 0) return dkmc_fail(30, "construct_laplacian: no interface sites", __FILE__, __LINE__);
    HIPCHK(hipStreamSynchronize(st));
    heat_free(h);
    HIPCHK(hipMalloc((void **)&h.rp, (size_t)(m + 1) * sizeof(int)));
    HIPCHK(hipMalloc((void **)&h.diagL, (size_t)m * sizeof(double)));
    int *cnt = (int *)scratch(S_MISC0, (size_t)m * sizeof(int));
    int *tot = (int *)scratch(S_MISC1, 4 * sizeof(int));
    if (!cnt || !tot) return e.err_code;
    MetalSet ms = load_metals(buf->metal_types, buf->num_metal_types_);
    const int blocks = (m + 255) / 256;
    hipLaunchKernelGGL(k_heat_count, dim3(blocks), dim3(256), 0, st, m, N_left_tot, nn, (const int *)buf->neigh_idx, (const int *)buf->site_element, ms,
                       gamma, cnt, h.diagL);
    int rc = dkmc_exclusive_scan_i32(cnt, h.rp, m, tot); if (rc) return rc;
    hipLaunchKernelGGL(k_set_last_h, dim3(1), dim3(1), 0, st, h.rp, m, (const int *)tot);
    int nnz = 0;
    HIPCHK(hipMemcpyAsync(&nnz, tot, sizeof(int), hipMemcpyDeviceToHost, st));
    HIPCHK(hipStreamSynchronize(st));
    HIPCHK(hipMalloc((void **)&h.ci, (size_t)nnz * sizeof(int)));
    hipLaunchKernelGGL(k_heat_fill, dim3(blocks), dim3(256), 0, st, m, N_left_tot, nn, (const int *)buf->neigh_idx, (const int *)h.rp, h.ci);
    KCHK();
    HIPCHK(hipStreamSynchronize(st));
    h.N = N; h.nn = nn; h.lo = N_left_tot; h.m = m; h.nnz = nnz; h.neigh = buf->neigh_idx;
    if (g_heat_form) {
        // the form kpattern_form_build chooses for this pattern (dkmc_set_k_blocked, dkmc_set_k_blocked_large); a pattern it refuses runs on the CSR positions
        h.kb = kpattern_form_build(h.rp, h.ci, m, nnz, buf->site_x + h.lo, buf->site_y + h.lo, buf->site_z + h.lo, st);
        if (h.kb) h.kb->word_bytes = 4;          // heat forms keep 4-byte stored words (pcol itself); dkmc_set_k_window_word_bytes is K's
        h.form = h.kb ? h.kb->form : 0;
        HIPCHK(hipMalloc((void **)&h.diag, (size_t)m * 8 * 2));
        HIPCHK(hipMalloc((void **)&h.chain, sizeof(HeatChain)));
    }
    return 0;
}

// matrix values, right-hand side and start vector of one solve.  steady = 0: A = I - s L, b = T_vec + P c s, y0 = T_vec;
// steady = 1: A = -L, b = P c, y0 = T_vec as well (any start vector gives the same solution)
__global__ __launch_bounds__(256) void k_heat_system(int m, int lo, const int *__restrict__ rp, const int *__restrict__ ci, const double *__restrict__ diagL,
                                                     const int *__restrict__ element, const double *__restrict__ T, const double *__restrict__ P,
                                                     double s, int steady, double T0, double pv, double pn,
                                                     double *__restrict__ a, double *__restrict__ b, double *__restrict__ y)
{
    const int LPR = 16;
    const int g = threadIdx.x / LPR, l = threadIdx.x % LPR;
    const int r = blockIdx.x * (256 / LPR) + g;
    if (r >= m) return;
    const double dl = diagL[r];
    for (int p = rp[r] + l; p < rp[r + 1]; p += LPR) {
        const bool dg = ci[p] == r;
        a[p] = steady ? (dg ? -dl : -1.0) : (dg ? 1.0 - s * dl : -s);
    }
    if (l == 0) {
        const int i = lo + r;
        const double tv = (T[i] - T0) / (DKMC_T1 - T0);
        const double c = (element[i] == VACANCY) ? pv : pn;
        b[r] = steady ? P[i] * c : tv + P[i] * c * s;
        y[r] = tv;
    }
}

__global__ void k_heat_store(int m, int lo, const double *__restrict__ y, double T0, double *__restrict__ T)
{
    const int r = blockIdx.x * blockDim.x + threadIdx.x;
    if (r < m) T[lo + r] = y[r] * (DKMC_T1 - T0) + T0;
}

__global__ __launch_bounds__(HT_NT) void k_mean_final(const double *__restrict__ part, int npart, double denom, double *T_bg)
{
    __shared__ double red[HT_NT / 64];
    double s = 0.0;
    for (int i = threadIdx.x; i < npart; i += HT_NT) s += part[i];
    const double tot = block_sum_all<HT_NT>(s, red);
    if (threadIdx.x == 0) *T_bg = tot / denom;
}

// ---- dkmc_set_heat_form(1): the systems on the forms of kcg.hip --------------------------------------------------------------------------------
// the two diagonals in the form's row order (perm: row of the form -> row of the pattern; null on the CSR positions)
__global__ void k_heat_diag(int m, const int *__restrict__ perm, const double *__restrict__ diagL, double s, double *__restrict__ diag)
{
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= m) return;
    const double dl = diagL[perm ? perm[i] : i];
    diag[i] = 1.0 - s * dl;
    diag[m + i] = -dl;
}
// right-hand side (form's row order) and start vector (pattern's row order) of row r from the site's temperature: the values k_heat_system forms
__device__ __forceinline__ void heat_row_system(int i, int r, int site, double T, const int *__restrict__ element, const double *__restrict__ P,
                                                double s, int steady, double T0, double pv, double pn, double *__restrict__ b, double *__restrict__ y)
{
    const double tv = (T - T0) / (DKMC_T1 - T0);
    const double c = (element[site] == VACANCY) ? pv : pn;
    b[i] = steady ? P[site] * c : tv + P[site] * c * s;
    y[r] = tv;
}
__global__ void k_heat_rhs(int m, int lo, const int *__restrict__ perm, const int *__restrict__ element, const double *__restrict__ T, const double *__restrict__ P,
                           double s, int steady, double T0, double pv, double pn, double *__restrict__ b, double *__restrict__ y)
{
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= m) return;
    const int r = perm ? perm[i] : i;
    heat_row_system(i, r, lo + r, T[lo + r], element, P, s, steady, T0, pv, pn, b, y);
}
// Between two chained transient sub-steps (after the unscale of sub-step k).  The solve stopped: what k_heat_store and the next k_heat_rhs do, row by
// row -- the temperature goes through site_temperature's value, so the bits are those of the polled path -- and the iteration count is recorded.
// It did not (the budget was too small), or an earlier sub-step of the batch did not: the failure word keeps the FIRST such sub-step (k + 1) and
// nothing else changes; k_heat_arm then leaves the loop's stop word set, so every later iteration kernel of the batch returns at once and every later
// k_heat_next is a no-op.  (K's start kernels carry no stop test: they still run, on work vectors that the host rebuilds when it resumes.)
// Every workgroup takes the same decision: nothing here writes ctrl, and the failure word only ever turns a "stopped" into a no-op.
__global__ void k_heat_next(int m, int lo, int k, const int *__restrict__ perm, const int *__restrict__ element, const double *__restrict__ P,
                            double s, double T0, double pv, double pn, const KCtrl *ctrl, HeatChain *ch, double *__restrict__ b, double *__restrict__ y,
                            double *__restrict__ T)
{
    const bool ok = ch->fail == 0 && ctrl->done != 0;
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (!ok) {
        if (i == 0 && ch->fail == 0) ch->fail = k + 1;
        return;
    }
    if (i == 0) ch->iters[k] = ctrl->iters;
    if (i >= m) return;
    const int r = perm ? perm[i] : i;
    const double Tn = y[r] * (DKMC_T1 - T0) + T0;
    T[lo + r] = Tn;
    heat_row_system(i, r, lo + r, Tn, element, P, s, 0, T0, pv, pn, b, y);
}
// after the start of a chained sub-step: the stop word k_kc_check0 left becomes the loop's, unless the batch has failed
__global__ void k_heat_arm(KCtrl *ctrl, const HeatChain *ch)
{
    if (threadIdx.x != 0 || blockIdx.x != 0) return;
    if (ch->fail) { ctrl->done = 1; return; }
    *ctrl = ch->start;
}

// the update on the forms of kcg.hip.  syncs / resumes: host synchronisations of the solves, sub-steps that took the resume path
static int heat_update_forms(dkmc_gpubuf *buf, HeatPat &h, int nsolve, int steady, double s, double T0, double pv, double pn, int *iters_total, int *syncs, int *resumes,
                             long long *bytes)
{
    Engine &e = eng(); hipStream_t st = e.stream;
    const int m = h.m, vb = (m + 255) / 256;
    double *b = (double *)scratch(S_HEAT_B, (size_t)m * 8 * 2), *y = (double *)scratch(S_HEAT_Y, (size_t)m * 8);
    if (!b || !y) return e.err_code;
    const int *perm = h.kb ? h.kb->perm : nullptr;
    if (!h.diag_built || h.diag_s != s) {          // s is known only here: the transient diagonal is rebuilt when it changes
        hipLaunchKernelGGL(k_heat_diag, dim3(vb), dim3(256), 0, st, m, perm, (const double *)h.diagL, s, h.diag);
        KCHK();
        h.diag_built = true; h.diag_s = s;
    }
    const double w = steady ? 1.0 : s;
    KcgRun c;
    if (int rc = kcg_run_setup(c, m, h.rp, h.nnz, h.kb, h.kb ? (const int *)h.kb->pcol : (const int *)h.ci, h.diag + (steady ? m : 0), b, b + m, w, w, g_heat_tol, y)) return rc;
    *bytes = kcg_run_bytes(c);
    const int *el = buf->site_element; const double *P = buf->site_power; double *T = buf->site_temperature;
    int maxit = 0, hint = 64;
    auto seen = [&](int it) { if (it > maxit) maxit = it; hint = (maxit + 7) / 8 * 8 + 8; };
    auto polled = [&](int first) -> int {
        hipLaunchKernelGGL(k_heat_rhs, dim3(vb), dim3(256), 0, st, m, h.lo, perm, el, (const double *)T, P, s, steady, T0, pv, pn, b, y);
        KCtrl hc{};
        if (int rc = kcg_run(c, hc, first)) return rc;
        if (e.err_code) return e.err_code;
        hipLaunchKernelGGL(k_heat_store, dim3(vb), dim3(256), 0, st, m, h.lo, (const double *)y, T0, T);
        KCHK();
        *iters_total += hc.iters; seen(hc.iters);
        return 0;
    };
    if (steady || nsolve < 2 || !g_heat_chain_on) {
        for (int k = 0; k < nsolve; ++k) if (int rc = polled(0)) return rc;
        *syncs = c.syncs;
        return 0;
    }
    HeatChain *ch = h.chain;
    int k = 0, batch_syncs = 0;
    while (k < nsolve) {
        const int nb = nsolve - k < HEAT_CHAIN_BATCH ? nsolve - k : HEAT_CHAIN_BATCH;
        const int B = g_heat_chain_budget > 0 ? g_heat_chain_budget : (maxit ? hint : 64);
        HIPCHK(hipMemsetAsync(ch, 0, sizeof(HeatChain), st));
        hipLaunchKernelGGL(k_heat_rhs, dim3(vb), dim3(256), 0, st, m, h.lo, perm, el, (const double *)T, P, s, 0, T0, pv, pn, b, y);
        for (int j = 0; j < nb; ++j) {
            if (int rc = kcg_run_scale(c, &ch->start)) return rc;
            if (int rc = kcg_run_start(c, &ch->start)) return rc;
            hipLaunchKernelGGL(k_heat_arm, dim3(1), dim3(64), 0, st, c.ctrl, (const HeatChain *)ch);
            for (int it = 0; it < B; ++it) if (int rc = kcg_run_iterate(c, it)) return rc;
            if (int rc = kcg_run_unscale(c)) return rc;
            hipLaunchKernelGGL(k_heat_next, dim3(vb), dim3(256), 0, st, m, h.lo, j, perm, el, P, s, T0, pv, pn, (const KCtrl *)c.ctrl, ch, b, y, T);
        }
        KCHK();
        HeatChain hc;
        HIPCHK(hipMemcpyAsync(&hc, ch, sizeof(HeatChain), hipMemcpyDeviceToHost, st));
        HIPCHK(hipStreamSynchronize(st));
        ++batch_syncs;
        const int good = hc.fail ? hc.fail - 1 : nb;
        for (int j = 0; j < good; ++j) { *iters_total += hc.iters[j]; seen(hc.iters[j]); }
        k += good;
        if (hc.fail) {          // sub-step k from its start (site_temperature holds sub-step k - 1), polled; then the chain goes on
            if (int rc = polled(hint)) return rc;
            ++*resumes; ++k;
        }
    }
    *syncs = batch_syncs + c.syncs;
    return 0;
}

// Device::updateTemperature, local branch (heat_solver.cpp:286-308): steady state when step_time > 1e3 * delta_t, otherwise
// int(step_time / delta_t) + 1 transient updates of length delta_t.  Writes gpubuf.site_temperature and gpubuf.T_bg.
extern "C" int dkmc_update_temperature_local(dkmc_gpubuf *buf, double step_time, double delta_t, double tau, double background_temp,
                                             double k_th_interface, double k_th_vacancies, double nn_dist, int num_atoms_contact,
                                             int *n_solves_out, int *steady_out, int *cg_iters_out, double *T_bg_out)
{
    Engine &e = eng(); hipStream_t st = e.stream;
    HeatPat &h = g_heat;
    if (!h.rp || h.N != buf->N_ || h.nn != buf->nn_ || h.neigh != buf->neigh_idx)
        return dkmc_fail(31, "update_temperature_local: construct_laplacian has not been called for these buffers", __FILE__, __LINE__);
    const int N = h.N, m = h.m;
    if (N - 2 * num_atoms_contact <= 0) return dkmc_fail(32, "update_temperature_local: empty averaging window", __FILE__, __LINE__);
    const double T0 = background_temp;
    const double pv = 1.0 / ((nn_dist * (1e-10) * k_th_interface) * (DKMC_T1 - background_temp));      // :369 (names as in the reference)
    const double pn = 1.0 / ((nn_dist * (1e-10) * k_th_vacancies) * (DKMC_T1 - background_temp));      // :370
    const int steady = step_time > 1e3 * delta_t;
    const int nsolve = steady ? 1 : (int)(step_time / delta_t) + 1;
    const double s = delta_t * tau;
    const double saved_tol = e.cg_tol;
    e.cg_tol = g_heat_tol;
    int iters_total = 0, rc = 0, syncs = 0, resumes = 0;
    long long bytes = 12LL * h.nnz + 4LL * (m + 1) + 96LL * m;          // the CSR formulation (kcg.hip's head comment)
    if (h.form >= 0) rc = heat_update_forms(buf, h, nsolve, steady, s, T0, pv, pn, &iters_total, &syncs, &resumes, &bytes);
    else for (int k = 0; k < nsolve && !rc; ++k) {
        double *a = (double *)scratch(S_HEAT_A, (size_t)h.nnz * 8), *b = (double *)scratch(S_HEAT_B, (size_t)m * 8), *y = (double *)scratch(S_HEAT_Y, (size_t)m * 8);
        if (!a || !b || !y) { rc = e.err_code; break; }
        hipLaunchKernelGGL(k_heat_system, dim3((m + 15) / 16), dim3(256), 0, st, m, h.lo, (const int *)h.rp, (const int *)h.ci, (const double *)h.diagL,
                           (const int *)buf->site_element, (const double *)buf->site_temperature, (const double *)buf->site_power, s, steady, T0, pv, pn, a, b, y);
        int it = 0;
        rc = cg_solve_jacobi(a, h.rp, h.ci, h.nnz, m, b, y, 1, nullptr, 0, &it, nullptr);
        iters_total += it; syncs += LaunchPlan::doubling(8).polls(it);       // the plan cg.hip runs without a hint
        if (!rc) hipLaunchKernelGGL(k_heat_store, dim3((m + 255) / 256), dim3(256), 0, st, m, h.lo, (const double *)y, T0, buf->site_temperature);
    }
    e.cg_tol = saved_tol;
    if (rc) return rc;
    {
        const long long info[8] = {h.form, m, h.form > 0 ? h.kb->total : h.nnz, nsolve, syncs, resumes, bytes, 0};
        for (int k = 0; k < 8; ++k) g_heat_info[k] = info[k];
    }
    // T_bg = mean over [num_atoms_contact, N - num_atoms_contact)
    const int cntN = N - 2 * num_atoms_contact;
    int nb = (cntN + HT_NT - 1) / HT_NT; if (nb > 1024) nb = 1024;
    double *part = (double *)scratch(S_HEAT, (size_t)(nb + 2) * 8);
    if (!part) return e.err_code;
    hipLaunchKernelGGL(k_power_partials, dim3(nb), dim3(HT_NT), 0, st, cntN, (const double *)buf->site_temperature + num_atoms_contact, part);
    hipLaunchKernelGGL(k_mean_final, dim3(1), dim3(HT_NT), 0, st, (const double *)part, nb, (double)cntN, buf->T_bg);
    KCHK();
    if (T_bg_out) { HIPCHK(hipMemcpyAsync(T_bg_out, buf->T_bg, 8, hipMemcpyDeviceToHost, st)); HIPCHK(hipStreamSynchronize(st)); }
    if (n_solves_out) *n_solves_out = nsolve;
    if (steady_out) *steady_out = steady;
    if (cg_iters_out) *cg_iters_out = iters_total;
    return 0;
}
