// rounds.h -- what the filament analyses share (clusters.hip, gaps.hip, paths.hip, track.hip, cuts.hip, flow.hip): the min-hooking + compression labelling,
// the host loop that runs rounds until one changes nothing, the lanes-per-row rule of the row kernels, the phase timer of the debug splits, and what
// happens after the kernels have run: the guard of the get / copy entry points, the end of a call that cannot deliver, the clamp of the debug round
// caps, the fetch of device columns into a result table (result_table.h: the table, its copy-out body and clamp_rows) and the x range of a pair of
// dbl_key words.  Kernels with internal linkage and inline host helpers, as in cellgrid.h: no symbol of its own.
//
// Labelling: min-hooking + compression in rounds, the kernel boundary is the only synchronisation point.
//   root[] (the caller's array) holds, between rounds, the ROOT of every member's tree (-1: not a member); it is read-only inside a hook launch.
//   parent[] holds the forest.  A hook launch does atomicMin(parent[max(ru, rv)], min(ru, rv)) for every index entry between two members whose
//   roots differ; only root entries are targets, and the result of a set of atomicMin on one word does not depend on their order, so the forest
//   after the launch is a function of root[] alone.  The compress launch walks parent[] from every member to its root (parents strictly
//   decrease: the walk is bounded; a walker that sees an older value of a word sees an older ANCESTOR, never a wrong one, so the path halving
//   it does on the way may race freely) and writes the root -- the same value whatever the walkers did to each other -- into root[] and
//   parent[].  A round whose atomicMins lowered nothing ends the loop: "rounds" is the number of rounds run, that last one included, and is the
//   number the synchronous host model (tests/cluster_ref.py: hook_compress_rounds) needs: the same on every call.
// Work shape: the hook kernel skips non-members in place (no member list: one 4-byte read per site decides, and the callers need a per-site
//   pass anyway); a member row is read by LPR lanes, 16 up to 128 entries per row and the whole wave above.
#pragma once
#include "common.h"
#include "result_table.h"

#define ROUND_NT 256                 // threads of a workgroup in the kernels below
#define ROUND_BATCH 8                // rounds enqueued per read-back; a round after the one that changed nothing returns at once
#define ROUND_CAP_MAX 4096           // change words a round loop may use: the callers' caps stay at or below it

// ---- lanes per index row ------------------------------------------------------------------------
inline int lpr_of(int nn) { return nn <= 128 ? 16 : 64; }
// kernel<16> or kernel<64> by lpr_of's answer, on the engine's usual launch form
#define LAUNCH_LPR(lpr, kernel, grid, block, st, ...) \
    do { \
        if ((lpr) == 16) hipLaunchKernelGGL(kernel<16>, grid, block, 0, st, __VA_ARGS__); \
        else hipLaunchKernelGGL(kernel<64>, grid, block, 0, st, __VA_ARGS__); \
    } while (0)

// ---- a pair of level words (paths.hip, flow.hip) in one relaxed agent-scope read -----------------
__device__ __forceinline__ int2 ld_pair(const int2 *p)
{
    const unsigned long long w = __hip_atomic_load((const unsigned long long *)p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    return make_int2((int)(w & 0xffffffffull), (int)(w >> 32));
}

// ---- the round driver ---------------------------------------------------------------------------
inline int *round_words() { static int h_changed[ROUND_CAP_MAX]; return h_changed; }

// enqueue(r) for r = 0, 1, ... in batches of `batch`; after each batch its change words ctrl[r] (device, zero before the call) are read back, and
// the first zero one ends the loop: *rounds = r + 1.  *rounds = 0: `cap` rounds ran and every one changed something.
template <class Enqueue>
inline int run_rounds(hipStream_t st, const int *ctrl, int cap, int batch, int *rounds, Enqueue enqueue)
{
    int *h_changed = round_words();
    if (cap > ROUND_CAP_MAX) cap = ROUND_CAP_MAX;
    int launched = 0;
    *rounds = 0;
    while (!*rounds && launched < cap) {
        const int b = cap - launched < batch ? cap - launched : batch;
        for (int r = launched; r < launched + b; ++r) enqueue(r);
        KCHK();
        HIPCHK(hipMemcpyAsync(h_changed + launched, ctrl + launched, (size_t)b * sizeof(int), hipMemcpyDeviceToHost, st));
        HIPCHK(hipStreamSynchronize(st));
        for (int r = launched; r < launched + b && !*rounds; ++r) if (!h_changed[r]) *rounds = r + 1;
        launched += b;
    }
    return 0;
}

// ---- the labelling ------------------------------------------------------------------------------
// hook: LPR lanes per member row
template <int LPR>
static __global__ __launch_bounds__(ROUND_NT) void k_lab_hook(int N, int nn, const int *__restrict__ idx, const int *__restrict__ root, int *parent,
                                                              int *ctrl, int round)
{
    if (round > 0 && ctrl[round - 1] == 0) return;            // the round before changed nothing: the labelling is finished
    const int lane = threadIdx.x % LPR;
    const long long groups = (long long)gridDim.x * (ROUND_NT / LPR);
    int changed = 0;
    for (long long u = (long long)blockIdx.x * (ROUND_NT / LPR) + threadIdx.x / LPR; u < N; u += groups) {
        const int ru = root[u];
        if (ru < 0) continue;
        const int *row = idx + (size_t)u * nn;
        for (int k = lane; k < nn; k += LPR) {
            const int v = row[k];
            if (v < 0 || v >= N) continue;                    // padding, anywhere in the row
            const int rv = root[v];
            if (rv < 0 || rv == ru) continue;
            const int hi = ru > rv ? ru : rv, lo = ru > rv ? rv : ru;
            if (atomicMin(&parent[hi], lo) > lo) changed = 1;
        }
    }
    if (changed) atomicOr(&ctrl[round], 1);
}

// compress: every member to its root, with path halving on the way.  (NT = ROUND_NT; a template, like label_rounds below, so that the labelling's
// kernels exist only in the files that call label_rounds and not in every file that includes this header for its other helpers.)
template <int NT>
static __global__ __launch_bounds__(NT) void k_lab_compress(int N, int *root, int *parent, const int *ctrl, int round)
{
    if (ctrl[round] == 0) return;                             // nothing was hooked: root[] and parent[] hold the roots already
    const int i = blockIdx.x * NT + threadIdx.x;
    if (i >= N || root[i] < 0) return;
    int c = i;
    for (;;) {
        const int p = ld_agent(&parent[c]);
        if (p >= c || p < 0) break;                           // c is a root (a parent is smaller than its child: the walk ends)
        const int gp = ld_agent(&parent[p]);
        if (gp >= p || gp < 0) { c = p; break; }
        st_agent(&parent[c], gp);
        c = gp;
    }
    root[i] = c;
    st_agent(&parent[i], c);
}

// the rounds on root[] / parent[] as the caller's membership kernel left them (the site itself, -1 for a non-member) and ctrl[] (cap zero words).
// *rounds as run_rounds gives it: 0 = not finished within cap, and what becomes of root[] then is the caller's business.
template <int NT = ROUND_NT>
inline int label_rounds(hipStream_t st, int N, int nn, const int *idx, int *root, int *parent, int *ctrl, int cap, int *rounds)
{
    const int lpr = lpr_of(nn);
    const int hook_blocks = grid_blocks((long long)N * lpr, ROUND_NT, 8192), site_blocks = (N + NT - 1) / NT;
    return run_rounds(st, ctrl, cap, ROUND_BATCH, rounds, [&](int r) {
        LAUNCH_LPR(lpr, k_lab_hook, dim3(hook_blocks), dim3(ROUND_NT), st, N, nn, idx, (const int *)root, parent, ctrl, r);
        hipLaunchKernelGGL(k_lab_compress<NT>, dim3(site_blocks), dim3(NT), 0, st, N, root, parent, (const int *)ctrl, r);
    });
}

// ---- phase timer: K intervals between K + 1 marks on the stream --------------------------------
template <int K>
struct PhaseTimer {
    hipEvent_t ev[K + 1];
    bool ready = false, on = false;
    // mark 0.  timed = 0: this call records nothing, and read() leaves its argument alone
    hipError_t start(bool timed, hipStream_t st)
    {
        on = timed;
        for (int i = 0; on && !ready && i <= K; ++i)
            if (hipError_t e = hipEventCreate(&ev[i])) return e;
        ready = ready || on;
        return mark(0, st);
    }
    hipError_t mark(int i, hipStream_t st) { return on ? hipEventRecord(ev[i], st) : hipSuccess; }
    // ms[i] = mark i to mark i + 1; the stream is synchronised past the last mark
    hipError_t read(float *ms)
    {
        for (int i = 0; on && i < K; ++i)
            if (hipError_t e = hipEventElapsedTime(&ms[i], ev[i], ev[i + 1])) return e;
        return hipSuccess;
    }
};

// ---- after the kernels -------------------------------------------------------------------------
// the guard of a get / copy entry point: nothing is handed out unless the last find call finished
#define NEED_FINISHED(valid, entry, call) \
    do { if (!(valid)) return dkmc_fail(3, entry ": no finished " call " call", __FILE__, __LINE__); } while (0)

// a call that cannot deliver: no partial result goes out as valid.  The call's N-site outputs are set to -1 and msg is the error (code 4)
template <int K>
inline int abandon(hipStream_t st, size_t n, int *const (&outs)[K], const char *msg, const char *file, int line)
{
    for (int *out : outs) HIPCHK(hipMemsetAsync(out, 0xff, n * sizeof(int), st));
    HIPCHK(hipStreamSynchronize(st));
    return dkmc_fail(4, msg, file, line);
}

// a dkmc_debug_set_*_round_cap argument: 0 or less restores the default, nothing goes above the change words of run_rounds
inline int clamp_round_cap(int cap, int dflt) { return cap <= 0 ? dflt : (cap > ROUND_CAP_MAX ? ROUND_CAP_MAX : cap); }

// `rows` rows of T from the device: one copy per int column src[c], enqueued on st and not waited for; no copy at 0 rows.  The double columns are
// sized and left to the caller.
template <int NI, int ND>
inline int fetch_columns(hipStream_t st, ResultTable<NI, ND> &T, size_t rows, const int *const (&src)[NI])
{
    T.resize(rows);
    for (int c = 0; c < NI && rows; ++c) HIPCHK(hipMemcpyAsync(T.i[c].data(), src[c], rows * sizeof(int), hipMemcpyDeviceToHost, st));
    return 0;
}

// the minimum and maximum of x over some sites from their dbl_key words; has = 0 (no x given, or no such site): the empty range +inf, -inf
inline void key_range(bool has, unsigned long long kmin, unsigned long long kmax, double *lo, double *hi)
{
    *lo = has ? key_dbl(kmin) : INFINITY;
    *hi = has ? key_dbl(kmax) : -INFINITY;
}
