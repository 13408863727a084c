// events.hip -- KMC event table and residence-time event loop.
// Replaces execute_kmc_step_gpu / build_event_list / zero_out_events (kmc_events.cu:34-365).
//
// The reference runs, per executed event, a full thrust::inclusive_scan over N*nn rates, a binary
// search, ~11 one-element memcpys, a full zero_out_events pass and 4 memsets, with a host round trip
// between each.  Here the table is built once per step together with a 4-level sum
// tree (slot -> site row -> 64 rows -> 4096 rows -> total), and ONE resident workgroup then runs the
// whole event loop on the device: tree descent to pick the slot, execution, invalidation of the
// O(nn^2) slots that touch the two sites, and repair of the O(nn) tree nodes above them.  Every tree
// node is a fixed-order sum of its children, so selection is run-to-run deterministic; it equals the
// sequential-prefix definition of the host engine (utils.h:91-99, KMCProcess.cpp:303-311) except for
// draws that land within rounding distance of a bucket edge.
//
// Event rates on the local site temperature (dkmc_set_event_temperature; include/devicekmc_hip.h): slot_rate and k_ev_build are templates on the
// mode.  0 is the reference as compiled (Ekin = 0, one global T_bg) and never dereferences the temperature; 1 puts the reference's commented-out
// kinetic term back (Ekin = kB (T_s - T_bg)); 2 is Arrhenius on T_s.  T_s is the temperature of the site those commented-out lines name: j for
// generation, i for the three other classes.  The temperature enters at build time only: the event loop never recomputes a rate.
#include "common.h"

struct LayerEnergies { double gen[DKMC_MAX_LAYERS], rec[DKMC_MAX_LAYERS], vdiff[DKMC_MAX_LAYERS], odiff[DKMC_MAX_LAYERS]; };
// per-layer zero-field energies in constant memory, like the reference (kmc_events.cu:10-13); a kernel-argument struct
// indexed by layer[j] would be demoted to scratch memory
__constant__ LayerEnergies c_layerE;

struct EvOut {                 // device -> host mailbox
    double event_time, psum_last;
    int n_events, exhausted, bad, n_charged;
    int n_bad_T, pad;          // modes 1, 2: event-class slots of the build with a temperature that is not finite or not > 0 (the loop then ran no event)
};

// rate of slot (i, j): kmc_events.cu:52-122.  Returns the event type, P through *prob.
// MODE 1, 2: T_i = temperature[i] (read once per row by the caller), temperature[j] is gathered for generation slots only; a slot whose T_s is
// not finite or not > 0 keeps its type, gets P = 0 and adds 1 to *n_bad.  With T_s == T_bg both modes form mode 0's P bit for bit: Ekin is +0.0
// (x - (+0.0) is x - 0), and kB * T_s is the same product.
template <int MODE>
__device__ __forceinline__ int slot_rate(int i, int j, int N, const int *__restrict__ layer, double laty, double latz, int pbc,
                                         double T_bg, double freq, double sigma, double kk,
                                         const double *__restrict__ x, const double *__restrict__ y, const double *__restrict__ z,
                                         const double *__restrict__ pb, const double *__restrict__ pc,
                                         const int *__restrict__ element, const int *__restrict__ charge,
                                         int ei, int qi, double xi, double yi, double zi, double phii,
                                         const double *__restrict__ temperature, double T_i, int *n_bad, double *prob)
{
    int type = EV_NULL; double P = 0.0;
    if (j >= 0 && j < N) {
        const int ej = element[j];
        const bool gen = (ei == DEFECT && ej == O_EL), rec = (ei == OXYGEN_DEFECT && ej == VACANCY);
        const bool vdf = (ei == VACANCY && ej == O_EL), idf = (ei == OXYGEN_DEFECT && ej == DEFECT);
        if (gen || rec || vdf || idf) {
            const double dist = 1e-10 * site_dist(xi, yi, zi, x[j], y[j], z[j], laty, latz, pbc);
            const double dphi = phii - (pb[j] + pc[j]);
            const int qj = charge[j], lj = layer[j];
            double E0, En;
            if (gen) { En = 2 * dphi; E0 = c_layerE.gen[lj]; type = EV_GEN; }
            else if (rec) {
                const double self = v_solve(dist, 2, sigma, kk);
                const int cs = qi - qj;
                En = cs * (dphi + (cs / 2) * self);            // integer division (kmc_events.cu:77)
                E0 = c_layerE.rec[lj]; type = EV_REC;
            } else if (vdf) {
                const double self = (qi != 0) ? v_solve(dist, qi, sigma, kk) : 0.0;
                En = (qi - qj) * (dphi + self);
                E0 = c_layerE.vdiff[lj]; type = EV_VDIFF;             // layer of j (kmc_events.cu:98)
            } else {
                const double self = (qi != 0) ? v_solve(dist, 2, sigma, kk) : 0.0;
                En = (qi - qj) * (dphi - self);
                E0 = c_layerE.odiff[lj]; type = EV_IDIFF;
            }
            if constexpr (MODE == 0) {
                const double EA = E0 - En - 0;
                P = exp(-1 * EA / (DKMC_KB * T_bg)) * freq;
            } else {
                const double T_s = gen ? temperature[j] : T_i;
                if (!(T_s > 0.0) || isinf(T_s)) { P = 0.0; ++*n_bad; }
                else if constexpr (MODE == 1) {
                    const double Ekin = DKMC_KB * (T_s - T_bg);          // kmc_events.cu:65,81,99,118, as the authors left it in the comments
                    const double EA = E0 - En - Ekin;
                    P = exp(-1 * EA / (DKMC_KB * T_bg)) * freq;
                } else {
                    const double EA = E0 - En - 0;
                    P = exp(-1 * EA / (DKMC_KB * T_s)) * freq;
                }
            }
        }
    }
    *prob = P;
    return type;
}

// fixed-order sum of one row of the table (all lanes get the result)
__device__ __forceinline__ double row_sum(const double *__restrict__ row, int nn, int lane)
{
    double s = 0.0;
    for (int c = lane; c < nn; c += WAVE) s += row[c];
    return wave_sum_all(s);
}
// fixed-order sum of up to 64 consecutive entries starting at base (entries >= n count as 0)
__device__ __forceinline__ double group_sum(const double *__restrict__ v, int base, int n, int lane)
{
    const int k = base + lane;
    return wave_sum_all(k < n ? v[k] : 0.0);
}

// one wave per site row: rates of its nn slots + row sum (MODE 1, 2: + the row's bad-temperature slots added to *n_bad_out, one atomic per wave that has any)
template <int MODE>
__global__ __launch_bounds__(256) void k_ev_build(int N, int nn, const int *__restrict__ neigh, const int *__restrict__ layer,
                                                  const double *__restrict__ lattice, int pbc, const double *__restrict__ T_bg_p,
                                                  const double *__restrict__ freq_p, const double *__restrict__ sigma_p,
                                                  const double *__restrict__ k_p, const double *__restrict__ x,
                                                  const double *__restrict__ y, const double *__restrict__ z,
                                                  const double *__restrict__ pb, const double *__restrict__ pc,
                                                  const int *__restrict__ element, const int *__restrict__ charge,
                                                  int *__restrict__ ev_type, double *__restrict__ ev_prob, double *__restrict__ rowsum,
                                                  const double *__restrict__ temperature, int *__restrict__ n_bad_out)
{
    const int lane = threadIdx.x & 63;
    const int i = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (i >= N) return;
    const double laty = lattice[1], latz = lattice[2], T_bg = *T_bg_p, freq = *freq_p, sigma = *sigma_p, kk = *k_p;
    const int ei = element[i], qi = charge[i];
    const double xi = x[i], yi = y[i], zi = z[i], phii = pb[i] + pc[i];
    double T_i = 0.0; int n_bad = 0;
    if constexpr (MODE != 0) T_i = temperature[i];
    double s = 0.0;
    for (int c = lane; c < nn; c += WAVE) {
        const size_t idx = (size_t)i * nn + c;
        double P;
        const int type = slot_rate<MODE>(i, neigh[idx], N, layer, laty, latz, pbc, T_bg, freq, sigma, kk, x, y, z, pb, pc, element, charge,
                                         ei, qi, xi, yi, zi, phii, temperature, T_i, &n_bad, &P);
        ev_prob[idx] = P;
        if (ev_type) ev_type[idx] = type;
        s += P;
    }
    s = wave_sum_all(s);
    if (lane == 0 && rowsum) rowsum[i] = s;
    if constexpr (MODE != 0) {
        n_bad = wave_sum_all_i(n_bad);
        if (lane == 0 && n_bad && n_bad_out) atomicAdd(n_bad_out, n_bad);
    }
}

// one wave per tree node: out[k] = sum of in[64k .. 64k+63]
__global__ __launch_bounds__(256) void k_ev_level(int n_in, const double *__restrict__ in, int n_out, double *__restrict__ out)
{
    const int lane = threadIdx.x & 63;
    const int k = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (k >= n_out) return;
    const double s = group_sum(in, k * 64, n_in, lane);
    if (lane == 0) out[k] = s;
}

// wave-level search: first entry (index order) of v[base .. base+count) whose inclusive prefix exceeds
// `target`; returns its index relative to base (or the last positive entry if rounding leaves none) and
// the prefix before it through *before.  All lanes of the wave must call; result is wave-uniform.
__device__ __forceinline__ int wave_pick(const double *__restrict__ v, int base, int count, int limit, double target, int lane, double *before)
{
    double carry = 0.0; int last_pos = -1; double last_before = 0.0;
    for (int c0 = 0; c0 < count; c0 += WAVE) {
        const int k = base + c0 + lane;
        const double val = (c0 + lane < count && k < limit) ? v[k] : 0.0;
        const double inc = wave_scan_incl(val, lane) + carry;
        const unsigned long long hit = __ballot(inc > target);
        if (hit) {
            const int first = __ffsll((long long)hit) - 1;
            const double prev = __shfl(inc, first > 0 ? first - 1 : 0, WAVE);
            *before = first > 0 ? prev : carry;
            return c0 + first;
        }
        const unsigned long long pos = __ballot(val > 0.0);
        if (pos) {
            const int lastl = 63 - __clzll((long long)pos);
            const double prev = __shfl(inc, lastl > 0 ? lastl - 1 : 0, WAVE);
            last_pos = c0 + lastl; last_before = lastl > 0 ? prev : carry;
        }
        carry = __shfl(inc, 63, WAVE);
    }
    *before = last_before;
    return last_pos;
}

#define EVL_NT 1024
// The whole event loop of one KMC step (kmc_events.cu:210-349) in one resident workgroup.
__global__ __launch_bounds__(EVL_NT) void k_ev_loop(int N, int nn, const int *__restrict__ neigh, double *__restrict__ ev_prob,
                                                    double *__restrict__ rowsum, double *__restrict__ g2, double *__restrict__ g3,
                                                    int ng2, int ng3, int *__restrict__ element, int *__restrict__ charge,
                                                    const double *__restrict__ uniform, int n_uniform,
                                                    const double *__restrict__ freq_p, EvOut *__restrict__ out,
                                                    int *__restrict__ evlog, int max_log, const int *__restrict__ ncharged_p,
                                                    const int *__restrict__ n_bad_T_p)
{
    __shared__ int sh_i, sh_j, sh_stop;
    __shared__ double sh_psum;
    const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
    // modes 1, 2 of the rate model: the build met a temperature it cannot use -- no selection, no event (the word is the same for every thread)
    const int n_bad_T = n_bad_T_p ? *n_bad_T_p : 0;
    if (n_bad_T) {
        if (tid == 0) { out->event_time = 0.0; out->psum_last = 0.0; out->n_events = 0; out->exhausted = 0; out->bad = 0;
                        out->n_charged = ncharged_p ? *ncharged_p : -1; out->n_bad_T = n_bad_T; out->pad = 0; }
        return;
    }
    const double inv_freq = 1 / (*freq_p);
    int n_events = 0, exhausted = 0, bad = 0;
    double event_time = 0.0, psum_last = 0.0;
    for (;;) {
        if (2 * n_events + 1 >= n_uniform) { exhausted = 1; break; }
        // ---- select ----
        if (w == 0) {
            double s = 0.0;
            for (int k = lane; k < ng3; k += WAVE) s += g3[k];
            const double Psum = wave_sum_all(s);
            const double number = uniform[2 * n_events] * Psum;
            double before;
            int k3 = wave_pick(g3, 0, ng3, ng3, number, lane, &before);
            int i_sel = -1, j_sel = -1;
            if (k3 >= 0) {
                double rem = number - before;
                int k2 = wave_pick(g2, k3 * 64, 64, ng2, rem, lane, &before);
                if (k2 >= 0) {
                    rem -= before; k2 += k3 * 64;
                    int r = wave_pick(rowsum, k2 * 64, 64, N, rem, lane, &before);
                    if (r >= 0) {
                        rem -= before; r += k2 * 64;
                        const int sl = wave_pick(ev_prob + (size_t)r * nn, 0, nn, nn, rem, lane, &before);
                        if (sl >= 0) { i_sel = r; j_sel = neigh[(size_t)r * nn + sl];
                            if (lane == 0 && evlog && n_events < max_log) evlog[4 * n_events] = r * nn + sl; }
                    }
                }
            }
            if (lane == 0) { sh_i = i_sel; sh_j = j_sel; sh_psum = Psum; sh_stop = (i_sel < 0 || j_sel < 0); }
        }
        __syncthreads();
        if (sh_stop) { bad = 1; event_time = INFINITY; break; }     // no positive rate left (reference: undefined)
        const int i = sh_i, j = sh_j;
        const double Psum = sh_psum;
        // ---- execute (kmc_events.cu:249-320) ----
        if (tid == 0) {
            const int ei = element[i], ej = element[j], qi = charge[i], qj = charge[j];
            int type = EV_NULL;
            if (ei == DEFECT && ej == O_EL) { type = EV_GEN; element[i] = OXYGEN_DEFECT; element[j] = VACANCY; charge[i] = -2; charge[j] = 2; }
            else if (ei == OXYGEN_DEFECT && ej == VACANCY) { type = EV_REC; element[i] = DEFECT; element[j] = O_EL; charge[i] = 0; charge[j] = 0; }
            else if (ei == VACANCY && ej == O_EL) { type = EV_VDIFF; element[i] = ej; element[j] = ei; charge[i] = qj; charge[j] = qi; }
            else if (ei == OXYGEN_DEFECT && ej == DEFECT) { type = EV_IDIFF; element[i] = ej; element[j] = ei; charge[i] = qj; charge[j] = qi; }
            if (evlog && n_events < max_log) { evlog[4 * n_events + 1] = i; evlog[4 * n_events + 2] = j; evlog[4 * n_events + 3] = type; }
        }
        // ---- invalidate every slot whose row or target is i or j (zero_out_events + memsets) ----
        for (int c = tid; c < 2 * nn; c += EVL_NT) { const int r = c < nn ? i : j; ev_prob[(size_t)r * nn + (c < nn ? c : c - nn)] = 0.0; }
        for (int c = tid; c < 2 * nn * nn; c += EVL_NT) {
            const int a = c / nn, s = c - a * nn;
            const int n = neigh[(size_t)(a < nn ? i : j) * nn + (a < nn ? a : a - nn)];
            if (n < 0) continue;
            const int t = neigh[(size_t)n * nn + s];
            if (t == i || t == j) ev_prob[(size_t)n * nn + s] = 0.0;
        }
        __syncthreads();
        // ---- repair the sum tree above the touched rows: i, j and their neighbours ----
        const int n_aff = 2 + 2 * nn;
        for (int a = w; a < n_aff; a += EVL_NT / 64) {
            const int r = a == 0 ? i : a == 1 ? j : neigh[(size_t)(a - 2 < nn ? i : j) * nn + (a - 2 < nn ? a - 2 : a - 2 - nn)];
            if (r < 0) continue;
            const double s = row_sum(ev_prob + (size_t)r * nn, nn, lane);
            if (lane == 0) rowsum[r] = s;
        }
        __syncthreads();
        for (int a = w; a < n_aff; a += EVL_NT / 64) {
            const int r = a == 0 ? i : a == 1 ? j : neigh[(size_t)(a - 2 < nn ? i : j) * nn + (a - 2 < nn ? a - 2 : a - 2 - nn)];
            if (r < 0) continue;
            const int k2 = r >> 6;
            const double s = group_sum(rowsum, k2 * 64, N, lane);
            if (lane == 0) g2[k2] = s;
        }
        __syncthreads();
        for (int a = w; a < n_aff; a += EVL_NT / 64) {
            const int r = a == 0 ? i : a == 1 ? j : neigh[(size_t)(a - 2 < nn ? i : j) * nn + (a - 2 < nn ? a - 2 : a - 2 - nn)];
            if (r < 0) continue;
            const int k3 = r >> 12;
            const double s = group_sum(g2, k3 * 64, ng2, lane);
            if (lane == 0) g3[k3] = s;
        }
        __syncthreads();
        // ---- waiting time (kmc_events.cu:348): assigned, not accumulated ----
        event_time = -log(uniform[2 * n_events + 1]) / Psum;
        psum_last = Psum;
        ++n_events;
        if (!(event_time < inv_freq)) break;
    }
    if (tid == 0) { out->event_time = event_time; out->psum_last = psum_last; out->n_events = n_events; out->exhausted = exhausted; out->bad = bad;
                    out->n_charged = ncharged_p ? *ncharged_p : -1;       // charged-site count of the last pair sum rides along in the mailbox
                    out->n_bad_T = 0; out->pad = 0; }
}

// called by dkmc_copy_to_const_memory (engine.hip)
int events_upload_layers()
{
    Engine &e = eng(); LayerEnergies L;
    for (int i = 0; i < DKMC_MAX_LAYERS; ++i) { L.gen[i] = e.E_gen[i]; L.rec[i] = e.E_rec[i]; L.vdiff[i] = e.E_Vdiff[i]; L.odiff[i] = e.E_Odiff[i]; }
    HIPCHK(hipMemcpyToSymbol(HIP_SYMBOL(c_layerE), &L, sizeof(L)));
    return 0;
}

// ---- rate model switch (include/devicekmc_hip.h) ----
extern "C" void dkmc_set_event_temperature(int mode) { eng().event_temperature = (mode == 1 || mode == 2) ? mode : 0; }
extern "C" int dkmc_get_event_temperature(void) { return eng().event_temperature; }
extern "C" void dkmc_set_event_census(int on) { eng().event_census = on ? 1 : 0; }
extern "C" int dkmc_get_event_census_on(void) { return eng().event_census; }
extern "C" int dkmc_get_event_census(double *info16)
{
    Engine &e = eng();
    if (!info16) return dkmc_fail(13, "get_event_census: bad arguments", __FILE__, __LINE__);
    if (!e.event_census_valid) return dkmc_fail(17, "get_event_census: no census has been taken (dkmc_set_event_census(1), then a step)", __FILE__, __LINE__);
    memcpy(info16, e.event_census_info, sizeof(e.event_census_info));
    return 0;
}

// k_ev_build of the engine's mode on the engine's stream
static void ev_build_launch(int mode, int N, int nn, const int *neigh, const int *layer, const double *lattice, int pbc,
                            const double *T_bg, const double *freq, const double *sigma, const double *k,
                            const double *x, const double *y, const double *z, const double *pb, const double *pc,
                            const int *element, const int *charge, int *ev_type, double *ev_prob, double *rowsum,
                            const double *temperature, int *n_bad)
{
    const dim3 grid((N + 3) / 4), block(256);
    hipStream_t st = eng().stream;
    if (mode == 1)
        hipLaunchKernelGGL(k_ev_build<1>, grid, block, 0, st, N, nn, neigh, layer, lattice, pbc, T_bg, freq, sigma, k, x, y, z, pb, pc, element, charge,
                           ev_type, ev_prob, rowsum, temperature, n_bad);
    else if (mode == 2)
        hipLaunchKernelGGL(k_ev_build<2>, grid, block, 0, st, N, nn, neigh, layer, lattice, pbc, T_bg, freq, sigma, k, x, y, z, pb, pc, element, charge,
                           ev_type, ev_prob, rowsum, temperature, n_bad);
    else
        hipLaunchKernelGGL(k_ev_build<0>, grid, block, 0, st, N, nn, neigh, layer, lattice, pbc, T_bg, freq, sigma, k, x, y, z, pb, pc, element, charge,
                           ev_type, ev_prob, rowsum, (const double *)nullptr, (int *)nullptr);
}

extern "C" int dkmc_build_event_list_T(int N, int nn, const int *neigh, const int *layer, const double *lattice, int pbc,
                                       const double *T_bg, const double *freq, const double *sigma, const double *k,
                                       const double *x, const double *y, const double *z, const double *pb, const double *pc,
                                       const int *element, const int *charge, int *ev_type, double *ev_prob,
                                       const double *temperature, int *n_bad)
{
    const int mode = eng().event_temperature;
    if (N <= 0 || nn <= 0 || !ev_prob) return dkmc_fail(13, "build_event_list: bad arguments", __FILE__, __LINE__);
    if (mode != 0 && !temperature)
        return dkmc_fail(13, "build_event_list: dkmc_set_event_temperature is 1 or 2 and there is no site_temperature (bad arguments)", __FILE__, __LINE__);
    ev_build_launch(mode, N, nn, neigh, layer, lattice, pbc, T_bg, freq, sigma, k, x, y, z, pb, pc, element, charge, ev_type, ev_prob,
                    (double *)nullptr, temperature, n_bad);
    KCHK();
    return 0;
}

extern "C" int dkmc_build_event_list(int N, int nn, const int *neigh, const int *layer, const double *lattice, int pbc,
                                     const double *T_bg, const double *freq, const double *sigma, const double *k,
                                     const double *x, const double *y, const double *z, const double *pb, const double *pc,
                                     const int *element, const int *charge, int *ev_type, double *ev_prob)
{
    if (eng().event_temperature != 0)
        return dkmc_fail(13, "build_event_list: dkmc_set_event_temperature is 1 or 2 and this call has no site_temperature: use dkmc_build_event_list_T (bad arguments)",
                         __FILE__, __LINE__);
    ev_build_launch(0, N, nn, neigh, layer, lattice, pbc, T_bg, freq, sigma, k, x, y, z, pb, pc, element, charge, ev_type, ev_prob,
                    (double *)nullptr, (const double *)nullptr, (int *)nullptr);
    KCHK();
    return 0;
}

// measurement aid (dkmc_set_profiling(1)): HIP-event time of the last step's k_ev_build and of its census
static hipEvent_t g_ev_t[4]; static bool g_ev_t_ready = false; static double g_ev_ms[2] = {0.0, 0.0};
extern "C" int dkmc_debug_get_event_times(double *ms2)
{
    if (!ms2) return dkmc_fail(13, "debug_get_event_times: bad arguments", __FILE__, __LINE__);
    ms2[0] = g_ev_ms[0]; ms2[1] = g_ev_ms[1];
    return 0;
}

// ---- host side of the event loop, shared by the production step and the test aid (dkmc_debug_event_loop) ----
struct EvBufs { double *ev_prob, *rowsum, *g2, *g3, *uni; int *evlog; EvOut *out; int ng2, ng3, max_log; };
// the engine's table, tree, draw, log and mailbox scratch for an N x nn table; the draws are uploaded
static int ev_bufs(int N, int nn, const double *h_uniform, int n_uniform, EvBufs *b)
{
    Engine &e = eng();
    b->ng2 = (N + 63) / 64; b->ng3 = (b->ng2 + 63) / 64; b->max_log = n_uniform / 2;
    b->ev_prob = (double *)scratch(S_EV_PROB, (size_t)N * nn * 8);
    b->rowsum = (double *)scratch(S_EV_ROWSUM, (size_t)N * 8);
    b->g2 = (double *)scratch(S_EV_G2, (size_t)b->ng2 * 8); b->g3 = (double *)scratch(S_EV_G3, (size_t)b->ng3 * 8);
    b->uni = (double *)scratch(S_EV_UNI, (size_t)(n_uniform > 0 ? n_uniform : 1) * 8);
    b->evlog = (int *)scratch(S_EV_LOG, (size_t)(b->max_log > 0 ? b->max_log : 1) * 16);
    b->out = (EvOut *)scratch(S_EV_CTRL, sizeof(EvOut));
    if (!b->ev_prob || !b->rowsum || !b->g2 || !b->g3 || !b->uni || !b->evlog || !b->out) return e.err_code;
    if (n_uniform > 0) HIPCHK(hipMemcpyAsync(b->uni, h_uniform, (size_t)n_uniform * 8, hipMemcpyHostToDevice, e.stream));
    return 0;
}
// the two upper levels of the sum tree from the row sums
static void ev_levels(int N, const EvBufs &b)
{
    hipStream_t st = eng().stream;
    hipLaunchKernelGGL(k_ev_level, dim3((b.ng2 + 3) / 4), dim3(256), 0, st, N, b.rowsum, b.ng2, b.g2);
    hipLaunchKernelGGL(k_ev_level, dim3((b.ng3 + 3) / 4), dim3(256), 0, st, b.ng2, b.g2, b.ng3, b.g3);
}
// k_ev_loop on the table and tree in b, then the mailbox, the log, the statistics and the return code.  census_info (may be null): device
// buffer of a census enqueued before, delivered with the mailbox; timed: the HIP events of the build and the census were recorded.
static int ev_loop_run(int N, int nn, const int *neigh, const EvBufs &b, int *element, int *charge, const double *freq, int n_uniform,
                       const int *n_bad, const double *census_info, bool timed,
                       int *n_events_out, int *exhausted_out, int *h_event_log, double *event_time_out)
{
    Engine &e = eng(); hipStream_t st = e.stream;
    const bool census = census_info != nullptr;
    hipLaunchKernelGGL(k_ev_loop, dim3(1), dim3(EVL_NT), 0, st, N, nn, neigh, b.ev_prob, b.rowsum, b.g2, b.g3, b.ng2, b.ng3, element, charge,
                       b.uni, n_uniform, freq, b.out, h_event_log ? b.evlog : (int *)nullptr, b.max_log, (const int *)e.buf[S_PW_CNT], n_bad);
    KCHK();
    EvOut h;
    HIPCHK(hipMemcpyAsync(&h, b.out, sizeof(EvOut), hipMemcpyDeviceToHost, st));
    if (census) HIPCHK(hipMemcpyAsync(e.event_census_info, census_info, sizeof(e.event_census_info), hipMemcpyDeviceToHost, st));
    HIPCHK(hipStreamSynchronize(st));
    if (census) e.event_census_valid = 1;
    if (timed) {
        float a = 0.0f, c = 0.0f;
        HIPCHK(hipEventElapsedTime(&a, g_ev_t[0], g_ev_t[1]));
        if (census) HIPCHK(hipEventElapsedTime(&c, g_ev_t[2], g_ev_t[3]));
        g_ev_ms[0] = a; g_ev_ms[1] = c;
    }
    if (h_event_log && h.n_events > 0) HIPCHK(hipMemcpy(h_event_log, b.evlog, (size_t)h.n_events * 16, hipMemcpyDeviceToHost));
    e.stats.n_events = h.n_events; e.stats.psum_last = h.psum_last;
    if (h.n_charged >= 0) e.stats.n_charged = h.n_charged;
    if (n_events_out) *n_events_out = h.n_events;
    if (exhausted_out) *exhausted_out = h.exhausted;
    if (event_time_out) *event_time_out = h.event_time;
    if (h.n_bad_T) {
        char msg[160];
        snprintf(msg, sizeof msg, "execute_kmc_step: %d event slots have a site temperature that is not finite or not > 0; no event ran", h.n_bad_T);
        return dkmc_fail(16, msg, __FILE__, __LINE__);
    }
    if (h.bad) return dkmc_fail(7, "execute_kmc_step: no event with a positive rate", __FILE__, __LINE__);
    return 0;
}

extern "C" int dkmc_execute_kmc_step_gpu(int N, int nn, const int *neigh, const int *layer, const double *lattice, int pbc,
                                         const double *T_bg, const double *freq, const double *sigma, const double *k,
                                         const double *x, const double *y, const double *z, const double *pb, const double *pc,
                                         const double *temperature, int *element, int *charge,
                                         const double *h_uniform, int n_uniform, int resume,
                                         int *n_events_out, int *exhausted_out, int *h_event_log, double *event_time_out)
{
    // mode 0: the temperature is unused, as by the reference kernel (Ekin = 0, kmc_events.cu:65), and may be null
    Engine &e = eng(); hipStream_t st = e.stream;
    const int mode = e.event_temperature;
    if (mode != 0 && !temperature)
        return dkmc_fail(13, "execute_kmc_step: dkmc_set_event_temperature is 1 or 2 and site_temperature is null (bad arguments)", __FILE__, __LINE__);
    const bool build = !resume, census = build && e.event_census != 0, timed = build && e.profiling != 0;
    int *n_bad = nullptr; double *census_info = nullptr;
    if (build && mode != 0) { n_bad = (int *)scratch(S_EV_NBAD, sizeof(int)); if (!n_bad) return e.err_code; }
    if (timed && !g_ev_t_ready) { for (auto &t : g_ev_t) HIPCHK(hipEventCreate(&t)); g_ev_t_ready = true; }
    EvBufs b;
    if (ev_bufs(N, nn, h_uniform, n_uniform, &b)) return e.err_code;
    if (build) {
        if (n_bad) HIPCHK(hipMemsetAsync(n_bad, 0, sizeof(int), st));
        if (timed) HIPCHK(hipEventRecord(g_ev_t[0], st));
        ev_build_launch(mode, N, nn, neigh, layer, lattice, pbc, T_bg, freq, sigma, k, x, y, z, pb, pc, element, charge, (int *)nullptr, b.ev_prob,
                        b.rowsum, temperature, n_bad);
        if (timed) HIPCHK(hipEventRecord(g_ev_t[1], st));
        ev_levels(N, b);
        if (census) {       // on the step's own table, before the loop zeroes any of it
            if (timed) HIPCHK(hipEventRecord(g_ev_t[2], st));
            if (ev_census_enqueue(N, nn, neigh, element, temperature, b.ev_prob, &census_info)) return e.err_code;
            if (timed) HIPCHK(hipEventRecord(g_ev_t[3], st));
        }
    }
    return ev_loop_run(N, nn, neigh, b, element, charge, freq, n_uniform, n_bad, census_info, timed,
                       n_events_out, exhausted_out, h_event_log, event_time_out);
}

// one wave per site row of a table that is already in place: its row sum, by the row_sum() of the loop's repair
__global__ __launch_bounds__(256) void k_ev_rowsum(int N, int nn, const double *__restrict__ ev_prob, double *__restrict__ rowsum)
{
    const int lane = threadIdx.x & 63;
    const int i = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (i >= N) return;
    const double s = row_sum(ev_prob + (size_t)i * nn, nn, lane);
    if (lane == 0) rowsum[i] = s;
}

// test aid (include/devicekmc_hip_debug.h): the production loop on a caller's table
extern "C" int dkmc_debug_event_loop(int N, int nn, const int *neigh, const double *ev_prob_in, int *element, int *charge, const double *freq,
                                     const double *h_uniform, int n_uniform, int resume,
                                     int *n_events_out, int *exhausted_out, int *h_event_log, double *event_time_out)
{
    Engine &e = eng(); hipStream_t st = e.stream;
    if (N <= 0 || nn <= 0 || (long long)N * nn > 2147483647LL || !neigh || !element || !charge || !freq || n_uniform < 0 ||
        (n_uniform > 0 && !h_uniform) || (!resume && !ev_prob_in))
        return dkmc_fail(13, "debug_event_loop: bad arguments", __FILE__, __LINE__);
    EvBufs b;
    if (ev_bufs(N, nn, h_uniform, n_uniform, &b)) return e.err_code;
    if (!resume) {
        HIPCHK(hipMemcpyAsync(b.ev_prob, ev_prob_in, (size_t)N * nn * 8, hipMemcpyDeviceToDevice, st));
        hipLaunchKernelGGL(k_ev_rowsum, dim3((N + 3) / 4), dim3(256), 0, st, N, nn, b.ev_prob, b.rowsum);
        ev_levels(N, b);
    }
    return ev_loop_run(N, nn, neigh, b, element, charge, freq, n_uniform, (const int *)nullptr, (const double *)nullptr, false,
                       n_events_out, exhausted_out, h_event_log, event_time_out);
}
