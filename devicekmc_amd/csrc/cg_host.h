// cg_host.h -- the host scaffold the iterative solvers share: the poll loop that runs a LaunchPlan (launch_plan.h), the sampled event profile of
// its launches and the second stream of the sharded loops.  Host code only.
#pragma once
#include "common.h"
#include "launch_plan.h"

// Kernel profile of a loop (dkmc_set_profiling; bench.py builds its roofline from it): the sampled launches of a batch (LaunchPlan::sampled) carry
// the events of one slot -- kernel A start / stop, kernel B start / stop, after the exchange.  A and B get theirs as the start / stop events of the
// dispatch itself (hipExtLaunchKernelGGL): the kernel's own begin / end timestamps, no extra marker packets in the stream.  One instance serves every
// loop: no two are ever in flight together (xt.hip calls the block loop before its own starts).
struct EventSampler {
    enum { PER_SLOT = 5 };
    enum { LONG = 1, SHORT = 2, COMM = 4 };      // intervals a loop records: A start -> A stop, B start -> B stop, A stop -> after the exchange
    hipEvent_t ev[LaunchPlan::SAMPLE_SLOTS][PER_SLOT];
    bool ready = false;
    int mask = 0;
    double long_ms = 0.0, short_ms = 0.0, comm_ms = 0.0;
    int long_n = 0, short_n = 0, comm_n = 0;

    // start of a profiled loop: the events are created on first use, the accumulators cleared
    int begin(int intervals)
    {
        if (!ready) { for (auto &slot : ev) for (auto &x : slot) HIPCHK(hipEventCreate(&x)); ready = true; }
        mask = intervals;
        long_ms = short_ms = comm_ms = 0.0; long_n = short_n = comm_n = 0;
        return 0;
    }
    // slots 0 ... nslots - 1 of the batch the stream has just finished
    int harvest(int nslots)
    {
        for (int q = 0; q < nslots; ++q) {
            float ms = 0.f;
            if (mask & LONG) { HIPCHK(hipEventElapsedTime(&ms, ev[q][0], ev[q][1])); long_ms += ms; ++long_n; }
            if (mask & SHORT) { HIPCHK(hipEventElapsedTime(&ms, ev[q][2], ev[q][3])); short_ms += ms; ++short_n; }
            if (mask & COMM) { HIPCHK(hipEventElapsedTime(&ms, ev[q][1], ev[q][4])); comm_ms += ms; ++comm_n; }
        }
        return 0;
    }
    // the profile into the stats; comm: the exchange's fields too (the block loop leaves them alone)
    void to_stats(dkmc_stats &s, bool comm) const
    {
        s.spmv_long_ms = long_ms; s.spmv_short_ms = short_ms;
        s.spmv_long_launches = long_n; s.spmv_short_launches = short_n;
        if (comm) { s.comm_ms = comm_ms; s.comm_launches = comm_n; }
    }
};
inline EventSampler g_loop_events;

// The host's poll loop of every solver: reads *ctrl_d into h (one poll), stops on done, on iter_cap (> 0: an emulation's cap) or after
// LaunchPlan::ITER_LIMIT iterations (recorded as failure 4 with the message no_convergence), else enqueues the plan's next batch through
// enqueue(it, ev), whose non-zero return ends the loop at once with that code.  ev: the PER_SLOT events of a sampled launch, or null handles
// (always without a sampler).  first > 0: that many iterations are enqueued before the first poll (a caller that knows what the solve will
// need); syncs: counts the polls.
template <class Ctrl, class Enqueue>
static int cg_poll_loop(const Ctrl *ctrl_d, Ctrl &h, const LaunchPlan &plan, hipStream_t st, const char *no_convergence, EventSampler *sampler, Enqueue &&enqueue,
                        int iter_cap = 0, int first = 0, int *syncs = nullptr)
{
    static const hipEvent_t none[EventSampler::PER_SLOT] = {nullptr, nullptr, nullptr, nullptr, nullptr};
    int it = 0, launched = 0, batch = plan.first;
    for (; it < first; ++it) if (int rc = enqueue(it, none)) return rc;
    if (first > 0) KCHK();
    for (;;) {
        HIPCHK(hipMemcpyAsync(&h, ctrl_d, sizeof(Ctrl), hipMemcpyDeviceToHost, st));
        HIPCHK(hipStreamSynchronize(st));
        if (syncs) ++*syncs;
        if (sampler) if (int rc = sampler->harvest(LaunchPlan::counted_slots(it - launched, launched, h.iters))) return rc;
        if (h.done) break;
        if (iter_cap > 0 && it >= iter_cap) break;
        if (it >= LaunchPlan::ITER_LIMIT) { dkmc_fail(4, no_convergence, __FILE__, __LINE__); break; }
        for (int b = 0; b < batch; ++b, ++it)
            if (int rc = enqueue(it, sampler && LaunchPlan::sampled(b) ? sampler->ev[LaunchPlan::slot(b)] : none)) return rc;
        launched = batch;
        KCHK();
        batch = plan.next(batch);
    }
    return 0;
}

// Second stream of a sharded loop: a part of the product runs on it beside the engine's stream.  Events from a ring: a wait refers to the record that
// preceded it, the host may run a whole batch ahead.  Re-created when the device changes.
struct SideStream {
    enum { RING = 64 };
    hipStream_t st = nullptr; hipEvent_t a[RING], b[RING]; int device = -1; unsigned seq = 0; bool ready = false;
};
inline int side_stream_init(SideStream &S)
{
    const int dev = eng().device;
    if (S.ready && S.device == dev) return 0;
    if (S.ready) { (void)hipStreamDestroy(S.st); for (int i = 0; i < SideStream::RING; ++i) { (void)hipEventDestroy(S.a[i]); (void)hipEventDestroy(S.b[i]); } S.ready = false; }
    HIPCHK(hipStreamCreateWithFlags(&S.st, hipStreamNonBlocking));
    for (int i = 0; i < SideStream::RING; ++i) {
        HIPCHK(hipEventCreateWithFlags(&S.a[i], hipEventDisableTiming));
        HIPCHK(hipEventCreateWithFlags(&S.b[i], hipEventDisableTiming));
    }
    S.device = dev; S.seq = 0; S.ready = true;
    return 0;
}
